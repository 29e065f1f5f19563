"""Every compiled variant of the count kernels against the oracle: k x read length.

The dispatch of csrc/count_phase.h picks a template instantiation from k and the read length L
(tests/kernel_grid.py restates it): k_skpart_w<NPF, W, VAL> for 21 <= k <= 32 (36 (NPF, W) pairs
in two VAL forms), k_partition<NPF, HI, R10> (12 forms), k_wbv<W> for 33 <= k <= 52 (20 widths).
This grid runs each of them, at the lengths where a wave's LDS stage is exactly full or steps to
the next size (L = 63 / 64, 111 / 112, 159 / 160), with one window per read (L = k) and a partial
first block (L = k + 1), on ~1 300 reads over a 3 000-base genome.

Every case is bit-exact against oracle.assemble_packed(..., want_dict=True) -- positions, dict
size, dict items in order, contig bytes and offsets, links -- and asserts the count path
kernel_grid.expected_path predicts for it from the dispatch's own rules: no case accepts a
fallback, and test_kernel_grid.py checks that the cases below reach every instantiation.
  A  super-k-mer grid, both VAL forms; L = 160 leaves it
  B  window records: k below 21 and EULERHIP_NO_SK2, 12- and 10-byte records
  C  wide keys: minimizer runs, hash buckets, the HBM table
  D  read-count tails around the 64-read wave tile and the 256-read tile
  E  device buffers at byte offsets 1, 7, 8 and 15 (the staged loads round the pointer)
  F  the sharded flow at every k, and its variants on both sides of every per-k switch
"""
import ctypes

import numpy as np
import pytest

import eulerhip
import kernel_grid as kg

pytestmark = pytest.mark.gpu


def _check(session, k, ref):
    """the finished call of `session` against the oracle (as test_structured_gpu.py): positions,
    dict size, dict items in order (k-mers and counts, as ec_copy_dict writes them), contig bytes
    and offsets, links"""
    res = session.fetch(k)
    assert res.stats.n_positions == ref["n_positions"]
    assert res.stats.n_dict == ref["n_dict"]
    nd = res.stats.n_dict
    km = ctypes.create_string_buffer(max(nd * k, 1))
    counts = np.zeros(max(nd, 1), dtype=np.uint32)
    eulerhip.check(eulerhip.lib().ec_copy_dict(session._h, km, counts.ctypes.data))
    assert km.raw[: nd * k] == ref["d_kmers"]
    assert np.array_equal(counts[:nd], ref["d_counts"])
    assert res.contig_bytes == ref["contig_chars"]
    assert np.array_equal(res.contig_offsets, ref["contig_offsets"])
    assert res.links == ref["links_unpacked"]
    res.dict_counts = counts[:nd]
    return res


def _check_sharded(res, P, ref, what):
    assert P == ref["n_positions"], what
    assert res.stats.n_dict == ref["n_dict"], what
    assert res.contig_bytes == ref["contig_chars"], what
    assert np.array_equal(res.contig_offsets, ref["contig_offsets"]), what
    assert res.links == ref["links_unpacked"], what


def _assert_path(stats, want, what=None):
    got = (stats.count_path, stats.count_variant, stats.record_bytes)
    assert got == want, (what, "table_retries %d" % stats.table_retries)


def _run(session, k, L, n=kg.NREADS, short=False, limit=1, no_sk2=False, r10=-1):
    buf, off = kg.reads_of(k, L, n, short)
    session.run_host(buf, off, k, limit, eulerhip.EC_FLAG_WANT_DICT)
    res = _check(session, k, kg.oracle_of(k, L, n, short, limit))
    _assert_path(res.stats, kg.expected_path(k, L, n, no_sk2, r10))
    return res


# ---- A. super-k-mer grid ------------------------------------------------------------------------
@pytest.mark.parametrize("k,L", kg.A_CELLS)
def test_superkmer_grid(gpu_session, k, L):
    """k_skpart_w<NPF, k - 14, true>: reads of one length, no prescan"""
    res = _run(gpu_session, k, L)
    assert res.stats.count_variant == 3 and res.stats.record_bytes == 16


@pytest.mark.parametrize("k,L", kg.A_CELLS)
def test_superkmer_grid_after_prescan(gpu_session, k, L):
    """k_skpart_w<NPF, k - 14, false>: the first read is shorter than k, so phase_count_v2 skips
    the fast path (count_phase.h phase_count_v2, `L >= k && npf`), k_prescan takes the lengths of the
    reads with windows (count_v2.h:81-87: one length) and phase_count_sk2 runs without `validate`
    (phase_count_v2, `if (allow_sk2)`); five more
    reads of 0 .. k - 1 bases at a wave tile's edge, inside and at the end"""
    res = _run(gpu_session, k, L, short=True)
    assert res.stats.count_variant == 3 and res.stats.record_bytes == 16


@pytest.mark.parametrize("k,L", kg.A_LONG)
def test_superkmer_grid_past_the_stage(gpu_session, k, L):
    """L = 160: no wave stage holds 64 reads (npf_of), the exact path counts (16-byte records:
    its 256-read tiles do not fit count_part.h's stage either)"""
    res = _run(gpu_session, k, L)
    assert res.stats.count_variant == 0


# ---- B. window-record grid ----------------------------------------------------------------------
@pytest.mark.parametrize("k,L,no_sk2,r10", kg.B_CASES,
                         ids=["%d-%d-%s-r10_%s" % (k, L, "nosk2" if s else "default", {-1: "auto", 0: "off", 1: "on"}[r])
                              for k, L, s, r in kg.B_CASES])
def test_window_record_grid(gpu_session, monkeypatch, k, L, no_sk2, r10):
    """k_partition<NPF, k >= 17, R10>.  k = 1 and 2 have two and ten canonical keys for the 32
    coarse buckets: their runs outgrow the fixed capacity at every length, by design
    (kernel_grid.window_record_capacity_holds), and the exact path counts them"""
    if no_sk2:
        monkeypatch.setenv("EULERHIP_NO_SK2", "1")
    if r10 >= 0:
        monkeypatch.setenv("EULERHIP_V2_R10", str(r10))
    res = _run(gpu_session, k, L, no_sk2=no_sk2, r10=r10)
    if k > 2:
        assert res.stats.count_variant == (2 if r10 == 1 else 1)
        assert res.stats.record_bytes == (10 if r10 == 1 else 12)


# ---- C. wide grid -------------------------------------------------------------------------------
@pytest.mark.parametrize("k,L", kg.C_CELLS)
def test_wide_grid(gpu_session, k, L):
    """k <= 52, L <= 160: k_wbv<k - 14> and minimizer runs (16-byte records).  L = 160 included:
    k_wbv's own stage holds 64 reads of 160 bases (count_wide.h:47), and after it the default
    flow stages no read -- k_upsweep_runs and k_downsweep_wr walk the window minimizers, the bucket
    pass gathers a run's bases from global memory -- so the 256 x 160 bytes that do not fit STAGE_W
    are never asked of it.  L = 161, and k >= 53: hash buckets (24-byte records) while a 256-read
    tile fits the staged upsweep (L <= 159), else the HBM table."""
    _run(gpu_session, k, L)


@pytest.mark.parametrize("k", kg.TWO_LENGTH_KS)
def test_wide_two_lengths_leave_the_minimizer_buckets(gpu_session, k):
    """reads of 100 and 150 bases, the first read a short one: k_wbv takes M = 100 - k + 1 windows
    a read, finds the longer reads (count_wide.h:64) and raises wbv_long, and the call is redone on
    hash buckets (count_phase.h phase_count_wpart at `mb && hsc.wbv_long`, phase_count_w: 24-byte records; a 256-read tile of <= 150 bases fits
    the staged upsweep).  k_upsweep_runs runs before the host sees the flag: it must pass over the
    longer reads, whose windows M .. 150 - k lie past their rows of the minimizer array."""
    buf, off = kg.two_length_reads(k)
    gpu_session.run_host(buf, off, k, 1, eulerhip.EC_FLAG_WANT_DICT)
    res = _check(gpu_session, k, kg.oracle_of_two_lengths(k))
    _assert_path(res.stats, (eulerhip.EC_PATH_PARTITIONED, 0, 24))


# ---- D. read-count tails ------------------------------------------------------------------------
@pytest.mark.parametrize("n", kg.D_NS)
@pytest.mark.parametrize("k,L", kg.D_CELLS)
def test_read_count_tails(gpu_session, k, L, n):
    """one read, one short of / exactly / one past a wave tile, and around the 256-read tile; at
    limit 0, so that the few reads still give a dict and contigs to compare"""
    _run(gpu_session, k, L, n=n, limit=0)


# ---- E. misaligned device buffers ---------------------------------------------------------------
@pytest.mark.parametrize("d", kg.E_OFFSETS)
@pytest.mark.parametrize("k,L", kg.E_CELLS)
def test_misaligned_device_reads(gpu_session, k, L, d):
    """the reads at byte offset d of a 16-byte aligned device buffer, with 64 bytes of slack on
    either side (the staged 16-byte loads round the first byte down and the last one up, by
    design; they must stay inside the allocation).  The stage of each cell is exactly full when
    aligned.  Equal to the aligned run and to the oracle, on the same path."""
    import torch

    buf, off = kg.reads_of(k, L)
    n, nb = len(off) - 1, len(buf)
    ref = kg.oracle_of(k, L)
    d_off = torch.from_numpy(off.astype(np.int64)).cuda()
    hold = torch.zeros(64 + 16 + nb + 64, dtype=torch.uint8, device="cuda")
    assert hold.data_ptr() % 16 == 0
    got = []
    for at in (64, 64 + d):
        hold.zero_()
        hold[at:at + nb] = torch.from_numpy(np.array(buf)).cuda()
        torch.cuda.synchronize()
        gpu_session.run_device(hold.data_ptr() + at, d_off.data_ptr(), n, k, 1, eulerhip.EC_FLAG_WANT_DICT)
        res = _check(gpu_session, k, ref)
        _assert_path(res.stats, kg.expected_path(k, L, n), at)
        got.append(res)
    a, m = got
    assert m.contig_bytes == a.contig_bytes and m.links == a.links and np.array_equal(m.dict_counts, a.dict_counts)
    assert np.array_equal(m.contig_offsets, a.contig_offsets)


# ---- F. sharded k sweep -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def engines():
    import distributed

    es = [distributed.HipEngine(0) for _ in range(3)]
    yield es
    for e in es:
        e.sess.close()


def _sharded(engines, k, world, what, **kw):
    import distributed

    buf, off = kg.reads_of(k, kg.F_L)
    res, P = distributed.local_sharded_assemble(engines[:world], buf, off, k, 1, **kw)
    _check_sharded(res, P, kg.oracle_of(k, kg.F_L), what)
    for r, e in enumerate(engines[:world]):  # every rank's shard count, on its own path
        lo, hi = distributed.shard_range(len(off) - 1, r, world)
        shard = (buf[int(off[lo]):int(off[hi])], off[lo:hi + 1] - off[lo])
        assert e.count_variant == kg.expected_path(k, kg.F_L, hi - lo, reads=shard)[1], (what, r)


@pytest.mark.parametrize("k", kg.F_KS)
def test_sharded_every_k(engines, k):
    _sharded(engines, k, 2, "world 2")


@pytest.mark.parametrize("k", kg.F_SWITCH_KS)
def test_sharded_at_the_switches(engines, k):
    """both sides of merge_sk (21..32), merge_wmb (33..52) and the owner rule (minimizer ranges
    for 21 <= k <= 52, a key hash otherwise): three ranks, both finishes, both link modes, and
    the streaming count in three chunks"""
    import distributed

    _sharded(engines, k, 3, "world 3")
    for finish in ("partitioned", "replicated"):
        _sharded(engines, k, 3, finish, finish=finish)
    for partitioned in (True, False):
        _sharded(engines, k, 3, partitioned, partitioned=partitioned)
    buf, off = kg.reads_of(k, kg.F_L)
    stats = {}
    res, P = distributed.streaming_assemble(engines[0], buf, off, k, 1, chunk_reads=(len(off) - 1) // 3 + 1, fold=2,
                                            stats=stats)
    assert stats["chunks"] == 3
    _check_sharded(res, P, kg.oracle_of(k, kg.F_L), "streaming")
