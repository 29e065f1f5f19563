"""Super-k-mer records of up to 47 bases (count_sk2.h): at k = 31 the minimizer block is W = 17
windows wide and a run can last all 17 -- its minimizer enters as the newest m-mer and nothing
smaller arrives before it leaves.  The record holds such a run whole (length by sentinel bit,
no 4-bit n - 1 field) where the partition entry has the bit for it (M <= 128 windows a read);
reads of more windows and k = 32 (W = 18, 47 bases = 16 windows) cut at 16, k <= 30 never reaches
the cap on sequence without repeated m-mers.

Every case is compared with the oracle as test_sk2_canon_gpu compares (positions, ordered dict,
contig bytes and offsets, links, count_variant 3) and its record count with a numpy model of the
partition: m-mer hashes (superkmer.h mmer_hash of the canonical 15-mer, restated), sliding minima
over W, runs of equal minimum cut at the cap.  The model also counts the runs that fill 17
windows, so a case cannot pass without them.

The 47-base reads take 6 000 reads, not 2 000: a 47-base read holds a 17-window run only when
its smallest m-mer is the middle one of its 33 (1 in 33, ~60 of 2 000 reads), and every k = 31
shape has to show at least 100.
"""
import numpy as np
import pytest

import eulerhip
import oracle
from synth import make_reads

pytestmark = pytest.mark.gpu

SK_M = 15
COMP = str.maketrans("ACGT", "TGCA")


def rc(s):
    return s.translate(COMP)[::-1]


# ---- the partition's runs, restated ----------------------------------------------------------------
def mmer_hash(x):
    """superkmer.h mmer_hash on a uint32 array"""
    x = (x.astype(np.uint64) * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)
    return (x ^ (x >> np.uint64(15))).astype(np.uint32)


def _codes(buf, L):
    b = np.asarray(buf, np.uint8).reshape(-1, L)
    return ((b >> 1) ^ (b >> 2)) & 3  # A, C, G, T -> 0 .. 3


def window_minima(codes, k):
    """minimizer hash of every window: (reads, M) uint32"""
    n, L = codes.shape
    nm = L - SK_M + 1
    f = np.zeros((n, nm), np.uint64)
    r = np.zeros((n, nm), np.uint64)
    for t in range(SK_M):
        c = codes[:, t:t + nm].astype(np.uint64)
        f |= c << np.uint64(2 * (SK_M - 1 - t))  # first base on top
        r |= (np.uint64(3) - c) << np.uint64(2 * t)  # reverse complement
    h = mmer_hash(np.minimum(f, r).astype(np.uint32))
    W = k - SK_M + 1
    return np.lib.stride_tricks.sliding_window_view(h, W, axis=1).min(axis=2)


def model_runs(buf, L, k, cap):
    """(records, runs of >= 17 windows): runs of equal window minimum, cut every `cap` windows"""
    v = window_minima(_codes(buf, L), k)
    n, M = v.shape
    start = np.ones((n, M), bool)
    start[:, 1:] = v[:, 1:] != v[:, :-1]
    j = np.broadcast_to(np.arange(M), (n, M))
    pos = j - np.maximum.accumulate(np.where(start, j, 0), axis=1)  # windows since the run began
    recs = int((pos % cap == 0).sum())
    return recs, int((pos == 16).sum())


def nmax_of(k, L):
    """count_sk2.h sk2_nmax: 47 bases a record; 17 windows only at k = 31 with M <= 128"""
    M = L - k + 1
    return min(47 - k + 1, 17 if (k == 31 and M <= 128) else 16)


# ---- comparison with the oracle ----------------------------------------------------------------------
def _packed(reads):
    buf = np.frombuffer("".join(reads).encode(), np.uint8).copy()
    off = np.zeros(len(reads) + 1, np.uint64)
    off[1:] = np.cumsum([len(x) for x in reads])
    return buf, off


def _check_packed(session, buf, off, k, limit=1, variant=3):
    ref = oracle.assemble_packed(buf, off, k, limit, True)
    session.run_host(buf, off, k, limit, eulerhip.EC_FLAG_WANT_DICT)
    res = session.fetch(k, True)
    if variant is not None:
        assert res.stats.count_variant == variant and res.stats.record_bytes == 16
    assert res.stats.n_positions == ref["n_positions"] and res.stats.n_dict == ref["n_dict"]
    assert [[x, c] for x, c in res.dict_items] == ref["d"]
    assert res.contig_bytes == ref["contig_chars"] and np.array_equal(res.contig_offsets, ref["contig_offsets"])
    assert res.links == oracle.unpack_links(ref)
    return res


def _check_shape(session, genome, n, L, k, seed, err=0.0, limit=1, min_full=0):
    buf, off = make_reads(genome, n, L, seed, err=err)
    cap = nmax_of(k, L)
    want, full = model_runs(buf, L, k, cap)
    print("k %d L %d reads %d cap %d: model records %d, runs of >= 17 windows %d" % (k, L, n, cap, want, full))
    assert full >= min_full
    res = _check_packed(session, buf, off, k, limit)
    print("  records %d" % res.stats.n_records)
    assert res.stats.n_records == want
    return want, full


# ---- one 17-window run --------------------------------------------------------------------------------
_ONE = {}


def _one_run_read():
    """a 47-base read whose smallest m-mer lies at bases 16..30: all 17 windows hold it, one run.
    Returned in the orientation that is the canonical record (the smaller 94-bit string, base i
    at bits 2i), so its reverse complement is the record that flips."""
    if not _ONE:
        rng = np.random.default_rng(4731)
        while True:
            s = "".join("ACGT"[x] for x in rng.integers(0, 4, 47))
            codes = _codes(np.frombuffer(s.encode(), np.uint8), 47)
            h = window_minima(codes, SK_M)[0]  # (W = 1: the 33 m-mers' own hashes)
            if int(np.argmin(h)) == 16 and (h == h.min()).sum() == 1:
                v = window_minima(codes, 31)[0]
                assert len(v) == 17 and (v == h[16]).all()  # the model sees one 17-window run
                break
        val = lambda t: sum("ACGT".index(c) << (2 * i) for i, c in enumerate(t))  # noqa: E731
        _ONE["read"] = s if val(s) < val(rc(s)) else rc(s)
    return _ONE["read"]


def _family():
    """the read and its reverse complement; then ~200 copies of both among other reads"""
    r = _one_run_read()
    rng = np.random.default_rng(4732)
    g = "".join("ACGT"[x] for x in rng.integers(0, 4, 3000))
    many = []
    for i in range(200):
        many.append(r if rng.random() < 0.5 else rc(r))
    for i in range(300):
        p = int(rng.integers(0, len(g) - 47))
        many.append(g[p:p + 47] if rng.random() < 0.5 else rc(g[p:p + 47]))
    order = rng.permutation(len(many))
    return [[r, rc(r)], [many[i] for i in order]]


@pytest.mark.parametrize("which", [0, 1])
def test_one_full_run_and_its_flip_vs_oracle(gpu_session, which):
    reads = _family()[which]
    buf, off = _packed(reads)
    recs, full = model_runs(buf, 47, 31, 17)
    if which == 0:
        assert (recs, full) == (2, 2)  # one 17-window run a read
    else:
        assert full >= 200
    res = _check_packed(gpu_session, buf, off, 31)
    assert res.stats.n_records == recs


@pytest.mark.parametrize("which", [0, 1])
def test_full_run_first_events_vs_model(which):
    """every distinct k-mer's count and both first events against model_parallel.model_count, as
    test_shard_first_events_vs_model compares: a flipped 17-window record is where
    EA = B - n + 1 meets n = 17"""
    import torch

    import distributed
    from fake_engine import decode
    from model_parallel import model_count, twin

    reads = _family()[which]
    buf, off = _packed(reads)
    cnt, first = model_count(reads, 31)
    eng = distributed.HipEngine(0)
    try:
        st = eng.count_shard(torch.from_numpy(buf).cuda(), torch.from_numpy(off.astype(np.int64)).cuda(),
                             len(off) - 1, 0, 31, 0)
        assert st.count_variant == 3
        recs, counts = eng.export_by_owner(1)
        raw = np.frombuffer(recs.cpu().numpy().tobytes(), dtype=distributed.REC_DTYPE)
    finally:
        eng.sess.close()
    assert counts == [len(cnt)] and len(raw) == len(cnt)
    got = {}
    for r in raw:
        got[decode(int(r["key"]), 31)] = (int(r["count"]), int(r["first_canon"]), int(r["first_twin"]))
    want = {c: (v, first[c], first[twin(c)]) for c, v in cnt.items()}
    assert got == want


# ---- 17-window runs anywhere in a read ---------------------------------------------------------------
@pytest.mark.parametrize("L", [47, 48, 63, 64, 100, 150])
def test_k31_records_whole_vs_oracle(gpu_session, L):
    """runs cut only at 17: the record count is the model's, >= 100 runs fill all 17 windows"""
    n = 6_000 if L == 47 else 2_000
    _check_shape(gpu_session, 20_000, n, L, 31, 7100 + L, min_full=100)


def test_k31_more_than_128_windows_vs_oracle(gpu_session):
    """M > 128: the partition entry keeps 8 first-window bits and cuts at 16.  The super-k-mer
    path stages reads of up to 159 bases (kernel_grid.npf_of), so M = 129 at 159 bases is the one
    such shape at k = 31; reads of 200 bases (M = 170) are counted on the exact path, which has
    no super-k-mer records to count -- they are compared with the oracle alone"""
    assert nmax_of(31, 159) == 16
    _check_shape(gpu_session, 20_000, 1_000, 159, 31, 7301)
    buf, off = make_reads(20_000, 1_000, 200, 7300)
    res = _check_packed(gpu_session, buf, off, 31, variant=None)
    assert res.stats.count_variant != 3


@pytest.mark.parametrize("L", [47, 100, 150])
def test_k32_cap_16_vs_oracle(gpu_session, L):
    """W = 18, 47 bases hold 16 windows"""
    assert nmax_of(32, L) == 16
    _check_shape(gpu_session, 20_000, 2_000, L, 32, 7400 + L)


@pytest.mark.parametrize("k", [30, 21])
def test_small_k_unchanged_vs_oracle(gpu_session, k):
    """W <= 16: no run of distinct m-mers reaches the cap -- the count is the uncapped model's"""
    want, _ = _check_shape(gpu_session, 20_000, 2_000, 100, k, 7500 + k)
    buf, off = make_reads(20_000, 2_000, 100, 7500 + k)
    assert model_runs(buf, 100, k, 1 << 20)[0] == want


# ---- the other readers of the refined records ----------------------------------------------------------
@pytest.mark.parametrize("merge", ["1", "0"])
def test_error_rich_readers_vs_oracle(gpu_session, monkeypatch, merge):
    """0.5 % substitutions behind the seen-twice filter: k_skdedup + the merged k_skbucket_filt
    (merge 1) and the filter over every record (merge 0) read 17-window records"""
    monkeypatch.setenv("EULERHIP_FORCE_FILTER", "1")
    monkeypatch.setenv("EULERHIP_SKF_MERGE", merge)
    _check_shape(gpu_session, 50_000, 20_000, 100, 31, 7600, err=0.005, min_full=100)


def test_large_table_kernel_vs_oracle(gpu_session, monkeypatch):
    """EULERHIP_NO_SKB3: k_skbucket's roll-out on 17-window records"""
    monkeypatch.setenv("EULERHIP_NO_SKB3", "1")
    _check_shape(gpu_session, 20_000, 8_000, 100, 31, 7700, err=0.001, min_full=100)
