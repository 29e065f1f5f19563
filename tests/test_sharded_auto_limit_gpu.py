"""The solid limit chosen after the owner merge, on the device (ec_dense_spectrum,
ec_dense_refilter; csrc/dense_filter.h) and through distributed.local_sharded_assemble /
streaming_assemble / euler_run --limit auto: N simulated ranks on one MI355X, as
test_distributed_gpu.py.

  spectrum     the owners' spectra after the limit-1 merge sum to the one-GPU assembly's
  compaction   records with chosen counts: the export after ec_dense_refilter is the export before
               it with the removed records deleted, byte for byte, at the sizes around the kernel's
               per-workgroup span (dense_filter.h DF_SPAN = compact.h COMPACT_CHUNK = 16384)
  equivalence  merge at limit 1 + refilter(L) holds the record set of a merge at limit L
  end to end   contigs and links equal the oracle's at the row's limit; auto_info equals the row
  state        refusals where the dense records are gone; the owner ids of a counts-only export
  CLI          --sharded --limit auto writes what --sharded --limit L writes
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import eulerhip
import oracle
import spectrum_model
from spectrum_model import FIXED, info_of
from synth import make_reads

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUN = os.path.join(ROOT, "pycuda-euler_amd", "euler_run.py")

NBINS = 256  # the bins FIXED was computed with
SPAN = 16384  # records per workgroup of k_dense_count / k_dense_write
ROWS = {c[5]: (c, w) for c, w in FIXED if w[0]}  # k = 21, 23, 15, 31, 33 -> (case, row)
NOT_FOUND = next((c, w) for c, w in FIXED if not w[0])
WIDE_DTYPE = np.dtype([("lo", "<u8"), ("hi", "<u8"), ("count", "<u4"), ("pad", "<u4"), ("first_canon", "<u8"),
                       ("first_twin", "<u8"), ("pad2", "<u8")])


def rec_dtype(k):
    import distributed

    return distributed.REC_DTYPE if k <= 32 else WIDE_DTYPE


def key_fields(k):
    return ["key"] if k <= 32 else ["hi", "lo"]


@pytest.fixture(scope="module")
def engines():
    import distributed

    es = [distributed.HipEngine(0) for _ in range(3)]
    yield es
    for e in es:
        e.sess.close()


_rows = {}


def row_data(case):
    """(buf, off, the oracle's limit-1 spectrum, {limit: oracle result}) of a FIXED case, computed once"""
    if case not in _rows:
        G, n, L, seed, err, k = case
        buf, off = make_reads(G, n, L, seed, err=err)
        buf.setflags(write=False)
        d = oracle.assemble_packed(buf, off, k, 1, want_dict=True)["d"]
        _rows[case] = (buf, off, spectrum_model.spectrum(d, NBINS), {})
    return _rows[case]


def oracle_at(case, limit):
    buf, off, _, refs = row_data(case)
    if limit not in refs:
        refs[limit] = oracle.assemble_packed(buf, off, case[5], limit)
    return refs[limit]


def want_info(want, h):
    found, lo, d, p, floor, limit, n_solid, kept = want
    w = info_of(found, lo, d, p, floor, limit)
    w["spectrum"] = {c: v for c, v in enumerate(h) if v}
    w["n_solid_before"], w["n_solid_after"] = n_solid, kept
    return w


def received(engs, buf, off, k):
    """count, export by owner and exchange as local_sharded_assemble_shards does; per owner the
    arguments of its merge_owned_from: (records, bytes per source, read bases, lf_bits)"""
    import torch

    import distributed as D

    world, nreads = len(engs), len(off) - 1
    sends, bases = [], []
    for r, eng in enumerate(engs):
        lo, hi = D.shard_range(nreads, r, world)
        b = np.ascontiguousarray(buf[int(off[lo]):int(off[hi])])
        d_reads = torch.from_numpy(b if len(b) else np.zeros(1, np.uint8)).to(eng.device)
        d_off = torch.from_numpy((off[lo:hi + 1] - off[lo]).astype(np.int64)).to(eng.device)
        eng.set_owner_rule(D.OWNER_MINIMIZER)
        eng.count_shard(d_reads, d_off, hi - lo, lo, k, 0)
        sends.append(eng.export_by_owner(world, compact=True))
        bases.append(lo)
    got = []
    for dst in range(world):
        parts = []
        for recs, counts, lfb in sends:
            rb = D.compact_bytes(k) if lfb >= 0 else D.rec_bytes(k)
            o = sum(counts[:dst]) * rb
            parts.append(recs[o:o + counts[dst] * rb])
        got.append((torch.cat(parts) if world > 1 else parts[0], [p.numel() for p in parts], bases,
                    [s[2] for s in sends]))
    return got


def held(eng, k):
    """the session's held records on the host (ec_export_dense)"""
    return np.frombuffer(eng.export_dense().cpu().numpy().tobytes(), dtype=rec_dtype(k))


def to_dev(eng, recs):
    import torch

    return torch.from_numpy(np.frombuffer(recs.tobytes(), dtype=np.uint8).copy()).to(eng.device)


# ---- 1. spectrum ---------------------------------------------------------------------------------
_onegpu = {}


def onegpu_spectra(case):
    if case not in _onegpu:
        buf, off, _, _ = row_data(case)
        with eulerhip.Session(0) as s:
            s.run_host(buf, off, case[5], 1, 0)
            _onegpu[case] = {nb: s.kmer_spectrum(nb) for nb in (NBINS, 2048, 2)}
    return _onegpu[case]


@pytest.mark.parametrize("world", [1, 2, 3])
@pytest.mark.parametrize("k", [15, 21, 31, 33])
def test_owner_spectra_sum_to_the_one_gpu_spectrum(engines, k, world):
    case, want = ROWS[k]
    buf, off, h_oracle, _ = row_data(case)
    ref = onegpu_spectra(case)
    assert [int(x) for x in ref[NBINS]] == h_oracle
    engs = engines[:world]
    for eng, (recs, sb, bases, lfb) in zip(engs, received(engs, buf, off, k)):
        eng.merge_owned_from(recs, sb, bases, lfb, k, 1, 0, export=False)
    for nb in (NBINS, 2048, 2):  # four LDS histograms a workgroup, one, and the smallest spectrum
        hs = [eng.dense_spectrum(nb) for eng in engs]
        for eng, h in zip(engs, hs):
            assert h.dtype == np.uint64 and h.shape == (nb,)
            assert int(h.sum()) == int(eng.L.ec_dense_count(eng._h()))
        assert np.array_equal(np.sum(hs, axis=0, dtype=np.uint64), ref[nb]), nb
    assert sum(int(eng.L.ec_dense_count(eng._h())) for eng in engs) == want[6]


# ---- 2. compaction on records with chosen counts ------------------------------------------------------
def host_records(k, n, seed):
    """n exchange records built on the host: distinct canonical k-mer codes (random k-mers, each
    the smaller of itself and its reverse complement; odd k: no palindromes), distinct first
    events (record i: read i, windows 1 and 2), count 0 -- the tests choose the counts"""
    rng = np.random.default_rng(seed)
    bases = rng.integers(0, 4, (n + n // 8, k), dtype=np.uint64)

    def pack(b):  # first base most significant (wide.h K128: the 2k-bit code in (hi, lo))
        lo, hi = np.zeros(len(b), np.uint64), np.zeros(len(b), np.uint64)
        for i in range(k):
            hi = (hi << np.uint64(2)) | (lo >> np.uint64(62))
            lo = (lo << np.uint64(2)) | b[:, i]
        return hi, lo

    fh, fl = pack(bases)
    rh, rl = pack(np.uint64(3) - bases[:, ::-1])
    fwd = (fh < rh) | ((fh == rh) & (fl < rl))
    hi, lo = np.where(fwd, fh, rh), np.where(fwd, fl, rl)
    _, first = np.unique(np.stack([hi, lo], axis=1), axis=0, return_index=True)
    keep = np.sort(first)[:n]
    assert len(keep) == n
    r = np.zeros(n, rec_dtype(k))
    if k <= 32:
        assert not hi.any()
        r["key"] = lo[keep]
    else:
        r["hi"], r["lo"] = hi[keep], lo[keep]
    i = np.arange(n, dtype=np.uint64)
    r["first_canon"] = (i << np.uint64(32)) | np.uint64(1)
    r["first_twin"] = (i << np.uint64(32)) | np.uint64(2)
    return r


@pytest.fixture(scope="module")
def pool():
    """per k: 3 SPAN + 5 host-built records, never changed"""
    cache = {}

    def get(k):
        if k not in cache:
            cache[k] = host_records(k, 3 * SPAN + 5, 8800 + k)
            cache[k].setflags(write=False)
        return cache[k]

    return get


def merged(eng, recs, k):
    """merge_owned(limit = 0) of host records on the HBM table (EC_FLAG_GENERAL), whose dense order
    is the table's slot order: the same for the same keys, up to keys that raced for the slots of
    one probe run.  (The LDS-bucket merge emits its buckets in the order their workgroups finish.)
    Returns the held records: the pre-filter export."""
    m = eng.merge_owned(to_dev(eng, recs), k, 0, eulerhip.EC_FLAG_GENERAL, export=False)
    assert m == len(recs)
    return held(eng, k)


def check_filter(eng, k, P, L):
    """ec_dense_refilter(L) on the held records P: what must hold afterwards"""
    keep = P["count"] > L
    kept, info = eng.dense_refilter(L)
    removed = int((~keep).sum())
    assert info == {"limit": L, "changed": int(removed > 0), "n_removed_kmers": removed}
    assert kept == int(keep.sum()) == int(eng.L.ec_dense_count(eng._h()))
    assert int(eng.stats().n_solid) == kept
    out = held(eng, k)
    assert out.tobytes() == P[keep].tobytes()
    return out


@pytest.mark.parametrize("n", [1, 3, SPAN - 1, SPAN, SPAN + 1, 3 * SPAN + 5])
@pytest.mark.parametrize("k", [31, 41])
def test_refilter_compacts_in_order(engines, pool, k, n):
    eng = engines[0]
    recs = pool(k)[:n].copy()
    recs["count"] = 3
    P0 = merged(eng, recs, k)
    a, b = np.sort(P0, order=key_fields(k)), np.sort(recs, order=key_fields(k))
    for f in key_fields(k) + ["count", "first_canon", "first_twin"]:  # the merge holds what it was given
        assert np.array_equal(a[f], b[f]), f
    # all kept -- a limit below every count, and one at the merge's own: no byte changes
    for L in (2, 0):
        assert check_filter(eng, k, P0, L).tobytes() == P0.tobytes()
    # The patterns are laid out in held order, which only a merge tells: the position every input
    # record took in P0.  A later merge of the same keys holds them in that order except where keys
    # raced for the slots of one probe run (a few positions at most), so the spans get a margin
    # and each pattern is checked on the records the merge really held.
    pos = {x.tobytes(): i for i, x in enumerate(P0[key_fields(k)])}
    at = np.array([pos[x.tobytes()] for x in recs[key_fields(k)]])
    i = np.arange(n)
    M = 256
    in_span = (i >= SPAN - M) & (i < 2 * SPAN + M)

    def alternates(keep):  # every wave's 64 records hold kept and removed ones
        w = keep[: n - n % 64].reshape(-1, 64).sum(axis=1)
        return bool(((w > 0) & (w < 64)).all())

    def span_is(keep, v):  # the whole second span is v, with the other kind on both sides of it
        sp = keep[SPAN:2 * SPAN]
        sides = np.concatenate([keep[: SPAN - 2 * M], keep[2 * SPAN + 2 * M:]])
        return bool((sp == v).all()) and bool((sides != v).all()) and (n < 3 * SPAN or len(sides) > SPAN)

    patterns = {
        "alternating": (i % 2 == 0, alternates),
        "span removed": (~in_span, lambda keep: span_is(keep, False)),  # one whole span between kept ones
        "span kept": (in_span, lambda keep: span_is(keep, True)),
    }
    for name, (keep, laid_out) in patterns.items():
        counts = np.where(keep, 5 + i % 7, 1 + i % 4).astype(np.uint32)  # kept > 4 >= removed
        recs["count"] = counts[at]
        P = merged(eng, recs, k)
        held_keep = P["count"] > 4
        assert int(held_keep.sum()) == int(keep.sum()) and laid_out(held_keep), name
        assert len(check_filter(eng, k, P, 4)) == int(keep.sum()), name
    # all removed
    recs["count"] = 3
    P = merged(eng, recs, k)
    assert len(check_filter(eng, k, P, 3)) == 0
    assert int(eng.L.ec_dense_count(eng._h())) == 0
    assert int(eng.dense_spectrum(8).sum()) == 0  # (nothing held: zeros, nothing launched)


# ---- 3. equivalence with the merge ----------------------------------------------------------------
@pytest.mark.parametrize("world", [1, 2])
def test_refilter_equals_a_merge_at_that_limit(engines, world):
    k = 31
    case, want = ROWS[k]
    buf, off, _, _ = row_data(case)
    engs = engines[:world]
    got = received(engs, buf, off, k)
    for L in (want[5], 2):
        for eng, (recs, sb, bases, lfb) in zip(engs, got):
            eng.merge_owned_from(recs, sb, bases, lfb, k, 1, 0, export=False)
            eng.dense_refilter(L)
            a = np.sort(held(eng, k), order="key")
            eng.merge_owned_from(recs, sb, bases, lfb, k, L, 0, export=False)
            b = np.sort(held(eng, k), order="key")
            assert len(a) and a.tobytes() == b.tobytes(), L


# ---- 4. end to end ----------------------------------------------------------------------------------
E2E = [ROWS[15], ROWS[21], ROWS[31], ROWS[33], NOT_FOUND]
E2E_IDS = ["k%d%s" % (c[5], "" if w[0] else "-not-found") for c, w in E2E]


def check_result(res, ref):
    assert res.contig_bytes == ref["contig_chars"]
    assert res.links == oracle.unpack_links(ref)


@pytest.mark.parametrize("world", [1, 2, 3])
@pytest.mark.parametrize("case,want", E2E, ids=E2E_IDS)
def test_local_sharded_auto_limit_equals_oracle(engines, case, want, world):
    import distributed

    buf, off, h, _ = row_data(case)
    k = case[5]
    ref = oracle_at(case, want[5] if want[0] else 1)
    runs = [dict(finish="partitioned"), dict(finish="replicated")]
    if world == 2:
        runs.append(dict(partitioned=False))
    for kw in runs:
        info = {}
        res, P = distributed.local_sharded_assemble(engines[:world], buf, off, k, 1, auto_limit=True,
                                                    spectrum_bins=NBINS, auto_info=info, **kw)
        assert P == ref["n_positions"], kw
        check_result(res, ref)
        assert info == want_info(want, h), kw


@pytest.mark.parametrize("case,want", [ROWS[31], ROWS[33], NOT_FOUND], ids=["k31", "k33", "k21-not-found"])
def test_streaming_auto_limit_equals_oracle(engines, case, want):
    import distributed

    buf, off, h, _ = row_data(case)
    nreads = len(off) - 1
    ref = oracle_at(case, want[5] if want[0] else 1)
    info, stats = {}, {}
    res, P = distributed.streaming_assemble(engines[0], buf, off, case[5], 1, chunk_reads=-(-nreads // 4), fold=2,
                                            stats=stats, auto_limit=True, spectrum_bins=NBINS, auto_info=info)
    assert stats["chunks"] == 4 and stats["folds"] == 1
    assert P == ref["n_positions"]
    check_result(res, ref)
    assert info == want_info(want, h)
    assert stats["solid"] == want[7]


# ---- 5. state ------------------------------------------------------------------------------------------
def refused(eng):
    """both calls refuse with EC_ERR_STATE and say why"""
    hist = np.zeros(8, np.uint64)
    ri = eulerhip.RefilterInfo()
    for rc in (eng.L.ec_dense_spectrum(eng._h(), 8, hist.ctypes.data),
               eng.L.ec_dense_refilter(eng._h(), 1, ctypes.byref(ri))):
        assert rc == eulerhip.EC_ERR_STATE
        assert b"no counted or merged records" in eng.L.ec_last_error()
    return True


def test_calls_need_the_dense_records(engines):
    import torch

    import distributed

    k = 31
    case, want = ROWS[k]
    buf, off, _, _ = row_data(case)
    eng = distributed.HipEngine(0)
    try:
        eng.k = k
        assert refused(eng)  # a new session
        (recs, sb, bases, lfb), = received([eng], buf, off, k)
        d_reads = torch.from_numpy(np.array(buf)).to(eng.device)
        d_off = torch.from_numpy(off.astype(np.int64)).to(eng.device)
        eng.sess.run_device(d_reads.data_ptr(), d_off.data_ptr(), len(off) - 1, k, 1, 0)
        assert refused(eng)  # after ec_assemble_device
        ur = eng.merge_owned_from(recs, sb, bases, lfb, k, 1, 0, export=False)
        assert ur == want[6] and int(eng.dense_spectrum(NBINS).sum()) == ur
        eng.graph_place(0, ur, 1)
        assert refused(eng)  # after ec_graph_place (which moves the records)
        eng.merge_owned_from(recs, sb, bases, lfb, k, 1, 0, export=False)
        eng.sess.trim(0)
        assert refused(eng)  # after ec_session_trim(0)
        # ... and the session stays usable: the whole auto-limit flow on it
        res, _ = distributed.local_sharded_assemble([eng], buf, off, k, 1, auto_limit=True, spectrum_bins=NBINS)
        check_result(res, oracle_at(case, want[5]))
        # argument errors come before the state check
        assert eng.L.ec_dense_spectrum(eng._h(), 1, None) == eulerhip.EC_ERR_ARG
        assert eng.L.ec_dense_spectrum(eng._h(), eulerhip.EC_SPECTRUM_MAX_BINS + 1, None) == eulerhip.EC_ERR_ARG
        assert eng.L.ec_dense_refilter(eng._h(), 1, None) == eulerhip.EC_ERR_ARG
    finally:
        eng.sess.close()


def test_refilter_drops_the_cached_owner_ids(engines):
    """counts-only ec_export_by_owner, ec_dense_refilter, then the scattering export: the counts
    are those of the filtered set, and so are the records"""
    k = 31
    case, want = ROWS[k]
    buf, off, _, _ = row_data(case)
    eng = engines[0]
    (recs, sb, bases, lfb), = received([eng], buf, off, k)
    eng.merge_owned_from(recs, sb, bases, lfb, k, 1, 0, export=False)
    before = eng.owner_counts(3)
    assert sum(before) == want[6]
    kept, info = eng.dense_refilter(want[5])
    assert kept == want[7] and info == {"limit": want[5], "changed": 1, "n_removed_kmers": want[6] - want[7]}
    P = held(eng, k)
    out, counts = eng.export_by_owner(3)
    assert sum(counts) == kept == int(eng.L.ec_dense_count(eng._h()))
    got = np.frombuffer(out.cpu().numpy().tobytes(), dtype=rec_dtype(k))
    assert np.sort(got, order="key").tobytes() == np.sort(P, order="key").tobytes()


# ---- 6. command line --------------------------------------------------------------------------------------
def test_cli_sharded_limit_auto(tmp_path):
    k = 31
    case, want = ROWS[k]
    buf, off, _, _ = row_data(case)
    s = buf.tobytes().decode()
    path = tmp_path / "reads.fa"
    with open(path, "w") as f:
        for i in range(len(off) - 1):
            f.write(">r%d\n%s\n" % (i, s[int(off[i]):int(off[i + 1])]))
    outs = {}
    for name, limit in (("auto", "auto"), ("given", str(want[5]))):
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(29700 + os.getpid() % 200), RANK="0",
                   WORLD_SIZE="1", LOCAL_RANK="0", HSA_ENABLE_IPC_MODE_LEGACY="0")
        r = subprocess.run([sys.executable, RUN, "-i", str(path), "-k", str(k), "--sharded", "--limit", limit,
                            "--spectrum-bins", str(NBINS), "-o", name + ".fa", "--gfa", name + ".gfa"]
                           + (["--spectrum-out", "spec.tsv"] if limit == "auto" else []),
                           cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        outs[name] = r.stderr
    assert (tmp_path / "auto.fa").read_text() == (tmp_path / "given.fa").read_text()
    assert (tmp_path / "auto.gfa").read_text() == (tmp_path / "given.gfa").read_text()
    assert len((tmp_path / "auto.fa").read_text()) > 0
    assert "auto-limit: limit %d " % want[5] in outs["auto"]
    assert "solid k-mers %d -> %d" % (want[6], want[7]) in outs["auto"]
    assert "auto-limit" not in outs["given"]
    _, _, h, _ = row_data(case)
    assert (tmp_path / "spec.tsv").read_text() == "".join("%d\t%d\n" % (c, v) for c, v in enumerate(h) if v)
