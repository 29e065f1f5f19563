"""Canonical super-k-mer records (count_sk2.h): k_skrefine writes a record's bases in canonical
orientation, the masked bases or their reverse complement, whichever is smaller, with the flip in
bit 31 of the position word, and every consumer (k_skbucket3, k_skbucket, k_skdedup, the unmerged
k_skbucket_filt) decodes the events from (p, flip, n) with one helper, sk2_events.

Every case is bit-exact against the oracle as test_sk2_vs_oracle compares: ordered dict, contig
bytes and offsets, links, count_variant == 3.  The cases aim at what the record contract can get
wrong: every record flipped / none flipped, records equal to their own reverse complement (no
flip on the tie), records of 1 and of 16 windows, base words filled to the 32-base boundary and
to all 92 bits, every consumer kernel, the linear-probe record table's claim protocol at small
and large claim caps, and a refine whose output is overwritten by a second refine in the same call.

Not covered by any test: a position p >= 2^30.  Every caller passes read_base = 0 to
phase_count_sk2 today (ec_count_shard counts on shard-relative read ids and adds the base at the
export), so p = read * M + window reaches 2^30 only with reads * M >= 2^30, about 15 M reads of
100 bases.  That bit 31 of p is free for the flip up to the eligibility bound rests on
(read_base + reads) * 2M < 2^32 in phase_count_sk2, read in the code, not on a run.
"""
import numpy as np
import pytest

import eulerhip
import oracle
from synth import make_reads

pytestmark = pytest.mark.gpu

COMP = str.maketrans("ACGT", "TGCA")


def rc(s):
    return s.translate(COMP)[::-1]


def _packed(reads):
    buf = np.frombuffer("".join(reads).encode(), np.uint8).copy()
    off = np.zeros(len(reads) + 1, np.uint64)
    off[1:] = np.cumsum([len(x) for x in reads])
    return buf, off


def _check_packed(session, buf, off, k, limit=1, variant=3):
    """one call against the oracle, as test_sk2_vs_oracle: positions, dict in order, contig bytes and
    offsets, links, the super-k-mer count (variant None: the path is not pinned)"""
    ref = oracle.assemble_packed(buf, off, k, limit, True)
    session.run_host(buf, off, k, limit, eulerhip.EC_FLAG_WANT_DICT)
    res = session.fetch(k, True)
    if variant is not None:
        assert res.stats.count_variant == variant and res.stats.record_bytes == 16
    assert res.stats.n_positions == ref["n_positions"] and res.stats.n_dict == ref["n_dict"]
    assert [[x, c] for x, c in res.dict_items] == ref["d"]
    assert res.contig_bytes == ref["contig_chars"] and np.array_equal(res.contig_offsets, ref["contig_offsets"])
    assert res.links == oracle.unpack_links(ref)
    return res, ref


# ---- orientation ---------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [21, 22, 31, 32])
def test_orientation_vs_oracle(gpu_session, k):
    """the same reads all forward, all reverse-complemented and mixed: every record flips in one
    of the first two runs and not in the other.  Each run equals the oracle on its own input
    (dict order and contig orientation follow the first events, which move with the strand);
    the k-mer counts are the same in all three.  Odd and even k; records of n + k - 1 = 32 bases
    (the 64-bit boundary of the base words) occur at every k here."""
    counts = []
    for frac in (0.0, 1.0, 0.5):
        buf, off = make_reads(20_000, 4_000, 100, 6100 + k, rc_frac=frac)  # (same starts, other strands)
        res, ref = _check_packed(gpu_session, buf, off, k)
        counts.append(sorted((x, c) for x, c in res.dict_items))
    assert counts[0] == counts[1] == counts[2]


# ---- ties and palindromes ------------------------------------------------------------------------
def _rand(rng, n):
    return "".join("ACGT"[x] for x in rng.integers(0, 4, n))


@pytest.mark.parametrize("k", [22, 32])
def test_self_complementary_records_vs_oracle(gpu_session, k):
    """reads that are their own reverse complement (x + rc(x)): a read of exactly k bases is one
    record of one window equal to its reverse complement, and the longer ones hold centred
    super-k-mers that are -- the tie must not flip (flip would move the first events)"""
    rng = np.random.default_rng(600 + k)
    reads = []
    for i in range(300):
        x = _rand(rng, k // 2)
        reads += [x + rc(x)] * int(rng.integers(1, 4))  # n = 1, palindromic k-mer
    d, r, g = oracle.assemble(reads, k, 1)
    res = gpu_session.assemble(reads, k, 1, want_dict=True)
    assert res.stats.count_variant == 3
    assert [[x, c] for x, c in res.dict_items] == d and res.contigs == r and res.links == g
    for extra in (1, 4, 7):  # 3, 9, 15 windows a read (one length a call): one or two records
        reads = []
        for i in range(500):
            x = _rand(rng, k // 2 + extra)
            reads.append(x + rc(x))
        d, r, g = oracle.assemble(reads, k, 1)
        res = gpu_session.assemble(reads, k, 1, want_dict=True)
        assert res.stats.count_variant == 3, extra
        assert [[x, c] for x, c in res.dict_items] == d and res.contigs == r and res.links == g, extra


@pytest.mark.parametrize("k", [22, 32])
def test_palindromic_kmers_inside_records_vs_oracle(gpu_session, k):
    """even k: palindromic k-mers (inserted twice by build) inside super-k-mers of both strands,
    built as test_sk2_palindromes_vs_oracle builds them"""
    rng = np.random.default_rng(23 + k)
    parts = []
    for _ in range(40):
        parts.append(_rand(rng, 300))
        x = _rand(rng, 16)
        parts.append(x + rc(x))
    g = "".join(parts)
    reads = []
    for _ in range(3000):
        p = int(rng.integers(0, len(g) - 100))
        r = g[p:p + 100]
        reads.append(r if rng.random() < 0.5 else rc(r))
    d, r, gl = oracle.assemble(reads, k, 1)
    res = gpu_session.assemble(reads, k, 1, want_dict=True)
    assert res.stats.count_variant == 3
    assert [[x, c] for x, c in res.dict_items] == d and res.contigs == r and res.links == gl


# ---- record length extremes ----------------------------------------------------------------------
def _low_complexity_reads(n, L, seed):
    """reads over homopolymers and short tandem repeats (minimizer runs reach the 16-window cap:
    all 92 base bits used at k = 31, 32) beside random ones, both strands"""
    rng = np.random.default_rng(seed)
    units = ["A", "AC", "ACGT", "AT", "CG", "AAC", "GATC", "ACGTTGCA", "TTAGGG"]
    out = []
    for i in range(n):
        u = units[rng.integers(len(units))]
        b = list((u * (L // len(u) + 2))[:L])
        for _ in range(rng.integers(0, 3)):
            b[rng.integers(L)] = "ACGT"[rng.integers(4)]
        s = "".join(b)
        out.append(s if rng.random() < 0.5 else rc(s))
    rnd = _rand(rng, 5000)
    for i in range(n):
        p = int(rng.integers(0, len(rnd) - L))
        out.append(rnd[p:p + L])
    return out


@pytest.mark.parametrize("k", [21, 32])
def test_long_records_low_complexity_vs_oracle(gpu_session, k):
    reads = _low_complexity_reads(400, 120, 640 + k)
    d, r, g = oracle.assemble(reads, k, 1)
    res = gpu_session.assemble(reads, k, 1, want_dict=True)
    assert res.stats.count_variant == 3
    assert [[x, c] for x, c in res.dict_items] == d and res.contigs == r and res.links == g


@pytest.mark.parametrize("k", [21, 32])
def test_reads_of_length_k_vs_oracle(gpu_session, k):
    """n = 1 in every record: the base words beyond 2k bits must come out masked"""
    buf, off = make_reads(5_000, 6_000, k, 6200 + k)
    _check_packed(gpu_session, buf, off, k)


# ---- position and flip in one word ------------------------------------------------------------------
_EVENTS = {}


def _event_case():
    """2 000 reads of 100 bases, both strands, and model_count's (count, first events) of them
    from read 0 -- built once, never modified"""
    if not _EVENTS:
        from model_parallel import model_count

        buf, off = make_reads(5_000, 2_000, 100, 6350)
        text = buf.tobytes().decode()
        reads = [text[i * 100:(i + 1) * 100] for i in range(2_000)]
        _EVENTS["case"] = (buf, off, model_count(reads, 31))
    return _EVENTS["case"]


@pytest.mark.parametrize("base", [30_000_000, 0])
def test_shard_first_events_vs_model(base):
    """engine.count_shard from read id 30 000 000 and from 0, every distinct k-mer's exported
    record against model_parallel.model_count: the count and both first events (canonical string
    and twin), which are decoded from (p, flip, n) of the canonical records.  A flip bit leaking
    into p would move an event by 2^31 / M reads; a wrong flip swaps or shifts the two events.
    (The count itself runs on shard-relative ids: p stays small here, see the module docstring.)"""
    import torch

    import distributed
    from fake_engine import decode
    from model_parallel import twin

    buf, off, (cnt, first) = _event_case()
    eng = distributed.HipEngine(0)
    try:
        st = eng.count_shard(torch.from_numpy(buf).cuda(), torch.from_numpy(off.astype(np.int64)).cuda(),
                             len(off) - 1, base, 31, 0)
        assert st.count_variant == 3
        recs, counts = eng.export_by_owner(1)
        raw = np.frombuffer(recs.cpu().numpy().tobytes(), dtype=distributed.REC_DTYPE)
    finally:
        eng.sess.close()
    assert counts == [len(cnt)] and len(raw) == len(cnt)
    shift = base << 32
    got = {}
    for r in raw:
        got[decode(int(r["key"]), 31)] = (int(r["count"]), int(r["first_canon"]), int(r["first_twin"]))
    want = {c: (v, first[c] + shift, first[twin(c)] + shift) for c, v in cnt.items()}
    assert got == want


@pytest.mark.parametrize("base", [30_000_000, 0])
def test_streaming_read_base_vs_oracle(base):
    """distributed.streaming_assemble from read id 30 000 000 and from 0 on 20 000 reads: the dict
    size, the contigs and the links come out in the oracle's order, which follows the first events
    of both strands (test_shard_first_events_vs_model compares the events themselves).  The shard
    count runs on shard-relative ids and the export adds the base, so the refine sees the same
    small p in both runs: the base checks the export's side of the events, not bit 30 of p."""
    import torch

    import distributed

    buf, off = make_reads(30_000, 20_000, 100, 6300, err=0.001)
    ref = oracle.assemble_packed(buf, off, 31, 1)
    eng = distributed.HipEngine(0)
    try:
        st = eng.count_shard(torch.from_numpy(buf).cuda(), torch.from_numpy(off.astype(np.int64)).cuda(),
                             len(off) - 1, base, 31, 0)
        assert st.count_variant == 3  # (the shard count streaming_assemble runs takes the super-k-mer path)
        res, P = distributed.streaming_assemble(eng, buf, off, 31, 1, chunk_reads=20_000, read_base=base)
    finally:
        eng.sess.close()
    assert P == ref["n_positions"]
    assert res.stats.n_dict == ref["n_dict"]
    assert res.contig_bytes == ref["contig_chars"]
    assert np.array_equal(res.contig_offsets, ref["contig_offsets"])
    assert res.links == oracle.unpack_links(ref)


# ---- every consumer of the refined records ---------------------------------------------------------
@pytest.mark.parametrize("k", [31, 22])
def test_large_table_kernel_vs_oracle(gpu_session, monkeypatch, k):
    """EULERHIP_NO_SKB3: k_skbucket reads the canonical records"""
    monkeypatch.setenv("EULERHIP_NO_SKB3", "1")
    buf, off = make_reads(30_000, 8_000, 100, 6400 + k, err=0.001)
    _check_packed(gpu_session, buf, off, k)


@pytest.mark.parametrize("merge", ["0", "1", "2"])
@pytest.mark.parametrize("limit", [1, 2])
def test_error_rich_consumers_vs_oracle(gpu_session, monkeypatch, merge, limit):
    """1 % substitutions behind the seen-twice filter: k_skbucket_filt over every record (merge
    mode 0: windows rolled from the canonical record at EA + o, EB - o), k_skdedup with 4096- and
    2560-entry tables in front of it (modes 1, 2)"""
    monkeypatch.setenv("EULERHIP_FORCE_FILTER", "1")
    monkeypatch.setenv("EULERHIP_SKF_MERGE", merge)
    for k in (31, 24):
        buf, off = make_reads(30_000, 10_000, 100, 6500 + k, err=0.01)
        _check_packed(gpu_session, buf, off, k, limit)


# ---- the record table's probes and claims ----------------------------------------------------------
@pytest.mark.parametrize("cap", [1, 3, 5, 64, 400])
def test_claim_caps_vs_oracle(gpu_session, monkeypatch, cap):
    """EULERHIP_SK2_CLAIM at a single entry, a few, 64 and 400 on the input of
    test_sk2_record_overflow_list_vs_oracle (~530 distinct records a bucket): the reservation in
    front of the CAS holds the linear-probe table to the cap.  The overflow list
    takes 256 records a bucket: at cap 400 the call stays on k_skbucket3; at the small caps the
    list fills and the call is redone on another path, as designed -- exact either way"""
    monkeypatch.setenv("EULERHIP_SK2_CLAIM", str(cap))
    buf, off = make_reads(20_000, 4_000, 100, 5300, err=0.0)
    _check_packed(gpu_session, buf, off, 31, variant=3 if cap == 400 else None)


def test_table_full_default_cap_vs_oracle(gpu_session):
    """more than 832 distinct records a bucket at the default cap (a shape of
    test_sk2_record_table_full_default_cap_vs_oracle): the cap is a hard bound"""
    buf, off = make_reads(22_000, 80_000, 60, 5401, err=0.0)
    _check_packed(gpu_session, buf, off, 31)


def test_equal_records_race_vs_oracle(gpu_session):
    """a 2 kbp genome under 4 000 reads of 60 bases: a few distinct records with hundreds of copies
    each, so claims of equal content race inside one wave and must end in one count"""
    buf, off = make_reads(2_000, 4_000, 60, 6600, err=0.0)
    _check_packed(gpu_session, buf, off, 31)


def test_all_distinct_records_vs_oracle(gpu_session):
    """5 % substitutions, limit -1 (every k-mer solid): nearly every record claims an entry"""
    buf, off = make_reads(20_000, 3_000, 100, 6700, err=0.05)
    _check_packed(gpu_session, buf, off, 31, limit=-1)


# ---- the second refine ---------------------------------------------------------------------------
def test_refine_retry_twice_in_one_session(gpu_session, monkeypatch, capfd):
    """repeat_families at k = 31 outgrows a final bucket's planned capacity (see
    test_structured_gpu.py::test_default_path): the call refines again, over the first refine's
    canonical records.  Twice in one session: the second call starts from the speculative refine
    of the first call's plan and overflows it again.  EULERHIP_VERBOSE reports each second refine:
    if the planned capacities ever change so that none runs, the case fails instead of passing on
    a single refine."""
    monkeypatch.setenv("EULERHIP_VERBOSE", "1")
    from structured import oracle_of, reads_of

    buf, off = reads_of("repeat_families", 31)
    ref = oracle_of("repeat_families", 31)
    for _ in range(2):
        capfd.readouterr()
        gpu_session.run_host(buf, off, 31, 1, eulerhip.EC_FLAG_WANT_DICT)
        res = gpu_session.fetch(31, True)
        err = capfd.readouterr().err
        assert "refined again with capacity" in err, err
        assert res.stats.count_variant == 3
        assert [[x, c] for x, c in res.dict_items] == ref["d"]
        assert res.contig_bytes == ref["contig_chars"]
        assert np.array_equal(res.contig_offsets, ref["contig_offsets"])
        assert res.links == ref["links_unpacked"]
