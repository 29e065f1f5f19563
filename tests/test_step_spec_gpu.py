"""Speculative launches inside a step: phase_count_sk2 queues the graph phase's
first link kernels (k_jl_init, k_jl_scan) behind its bucket kernel on the previous call's shape,
the scan reading the solid count U from device memory, while the host waits for that count.
links_local takes them over when the count stood and U fits the assumed capacity, and runs its
own otherwise; Session.spec_counts() says which happened.  The step's small results travel as one
block (k_links_small), and the emission's node maps are cleared behind the starts' read-back.

Every case is compared with oracle.assemble_packed: contig bytes, offsets and links.  Inputs are
a few ten thousand reads; the local join is forced at that size (EULERHIP_JOIN_LOCAL=1: its own
threshold is 2^21 solid k-mers) and the reads are device-resident (run_device), as in the bench:
host input arrives in chunks, which the speculative refine -- the prologue's precondition -- skips.

No launch is queued on the contig starts' read-back: "starts_taken" / "starts_redone" stay 0.  The
sequences that would redo such a launch (the contig count across SMALL_STARTS, a ranking whose one
ruler pass misses a cycle) run here in warm sessions all the same: they cross the result block's
small / large paths and the fills' new place."""
import numpy as np
import pytest

import eulerhip
import oracle
from synth import make_reads

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

_REF = {}


def _ref(key, buf, off, k, limit=1):
    """the oracle's result of an input, computed once per module run and never modified"""
    if key not in _REF:
        r = oracle.assemble_packed(buf, off, k, limit)
        _REF[key] = (r["contig_chars"], np.array(r["contig_offsets"], dtype=np.uint64), oracle.unpack_links(r))
    return _REF[key]


def _inputs(key):
    if key not in _INPUTS_DONE:
        _INPUTS_DONE[key] = _INPUTS[key]()
    return _INPUTS_DONE[key]


def _many_replicons():
    """4 600 linear replicons of 130 bases under 100-base reads at 6x: more than 4096 contigs"""
    from structured import _rand, _rng, sample_reads

    rng = _rng(77, 1)
    return sample_reads([(_rand(rng, 130), False) for _ in range(4600)], 100, 6, rng)


_INPUTS = {
    "g30k": lambda: make_reads(30_000, 20_000, 100, 9101, err=0.001),
    "g10k": lambda: make_reads(10_000, 20_000, 100, 9102, err=0.001),
    "g30k_b": lambda: make_reads(30_000, 20_000, 100, 9103, err=0.001),
    "many": _many_replicons,
}
_INPUTS_DONE = {}


def _local_join(monkeypatch):
    monkeypatch.setenv("EULERHIP_DEBUG", "1")
    monkeypatch.setenv("EULERHIP_JOIN_LINKS", "1")
    monkeypatch.setenv("EULERHIP_JOIN_LOCAL", "1")


def _run(sess, buf, off, k, limit=1):
    d_buf = torch.from_numpy(np.array(buf)).cuda()  # (a copy: the shared inputs are read-only)
    d_off = torch.from_numpy(off.astype(np.int64)).cuda()
    torch.cuda.synchronize()
    sess.run_device(d_buf.data_ptr(), d_off.data_ptr(), len(off) - 1, k, limit)
    return sess.fetch(k)


def _check(sess, key, k, limit=1, buf_off=None):
    buf, off = buf_off if buf_off is not None else _inputs(key)
    chars, coff, links = _ref((key, k, limit), buf, off, k, limit)
    res = _run(sess, buf, off, k, limit)
    assert res.contig_bytes == chars, key
    assert np.array_equal(res.contig_offsets, coff), key
    assert res.links == links, key
    return res


# ---- 1: the same input three times -------------------------------------------------------------------
def test_same_input_three_times(monkeypatch):
    _local_join(monkeypatch)
    with eulerhip.Session(0) as s:
        taken = []
        for _ in range(3):
            _check(s, "g30k", 31)
            taken.append(s.spec_counts())
    assert taken[0]["links_taken"] == 0 and taken[0]["links_redone"] == 0  # (no shape to assume yet)
    # (call 1 leaves the refine's plan and the join's shape; calls 2 and 3 launch the refine on that
    # plan, and with it standing -- the prologue's precondition -- queue the prologue)
    assert [t["links_taken"] for t in taken[1:]] == [1, 2], taken
    assert taken[2]["links_redone"] == 0
    assert taken[2]["starts_taken"] == 0 and taken[2]["starts_redone"] == 0


# ---- 2: sizes alternating ----------------------------------------------------------------------------
def test_alternating_sizes(monkeypatch):
    """20 000 reads each (the refine's plan stands) of a 30 kbp, a 10 kbp and again a 30 kbp
    genome: a third of the solid k-mers fits the assumed capacity and the prologue is kept; three
    times the capacity does not, the scan stops at the capacity and init and scan run again"""
    _local_join(monkeypatch)
    with eulerhip.Session(0) as s:
        _check(s, "g30k", 31)
        _check(s, "g30k_b", 31)
        c0 = s.spec_counts()
        small = _check(s, "g10k", 31)
        c1 = s.spec_counts()
        large = _check(s, "g30k", 31)
        c2 = s.spec_counts()
    assert large.stats.n_solid > 2 * small.stats.n_solid
    assert c1["links_taken"] == c0["links_taken"] + 1 and c1["links_redone"] == c0["links_redone"], (c0, c1)
    assert c2["links_taken"] == c1["links_taken"] and c2["links_redone"] == c1["links_redone"] + 1, (c1, c2)


# ---- 3: the contig count across SMALL_STARTS, and no solid k-mer at all ---------------------------------
def test_contig_count_across_small_starts(monkeypatch):
    _local_join(monkeypatch)
    with eulerhip.Session(0) as s:
        few = _check(s, "g30k", 31)
        many = _check(s, "many", 31)
        few2 = _check(s, "g30k", 31)
        assert few.stats.n_contigs <= 4096 < many.stats.n_contigs and few2.stats.n_contigs == few.stats.n_contigs
        _check(s, "g30k", 31)  # (warm)
        none = _check(s, "g30k", 31, limit=1_000_000)  # (no k-mer is seen that often: U = 0)
        assert none.stats.n_solid == 0 and none.stats.n_contigs == 0
        _check(s, "g30k", 31)


# ---- 4: even k --------------------------------------------------------------------------------------
def test_even_k_after_odd_k(monkeypatch):
    """even k needs k_upal between init and scan and is left unspeculated: no prologue is queued
    on or after an even-k call, and one recorded at odd k is not applied at even k"""
    _local_join(monkeypatch)
    with eulerhip.Session(0) as s:
        _check(s, "g30k", 31)
        _check(s, "g30k", 31)
        c0 = s.spec_counts()
        _check(s, "g30k", 30)
        _check(s, "g30k", 30)
        _check(s, "g30k", 30)
        assert s.spec_counts() == c0
        _check(s, "g30k", 31)
        _check(s, "g30k", 31)
        assert s.spec_counts()["links_redone"] == c0["links_redone"]


# ---- 5: the count falls back after a queued prologue -------------------------------------------------
def test_claim_cap_fallback_after_prologue(monkeypatch):
    """a warm session, then EULERHIP_SK2_CLAIM=1 on the input of test_claim_caps_vs_oracle: the
    record table overflows behind the queued prologue and the call is counted again on window
    records, whose index the local join does not take"""
    _local_join(monkeypatch)
    buf, off = make_reads(20_000, 4_000, 100, 5300, err=0.0)
    with eulerhip.Session(0) as s:
        for _ in range(2):
            _check(s, "claim", 31, buf_off=(buf, off))
        c0 = s.spec_counts()
        assert c0["links_taken"] == 1
        monkeypatch.setenv("EULERHIP_SK2_CLAIM", "1")
        _check(s, "claim", 31, buf_off=(buf, off))
        c1 = s.spec_counts()
        assert c1["links_taken"] == c0["links_taken"] and c1["links_redone"] == c0["links_redone"] + 1, (c0, c1)
        monkeypatch.delenv("EULERHIP_SK2_CLAIM")
        _check(s, "claim", 31, buf_off=(buf, off))


def test_second_refine_after_prologue(monkeypatch, capfd):
    """repeat_families at k = 31 outgrows a final bucket: the second refine reads the partition's
    records (s->recs) after the prologue's scan has written its foreign records -- into a buffer
    of its own.  EULERHIP_VERBOSE reports the second refine, so the case cannot pass without one"""
    _local_join(monkeypatch)
    monkeypatch.setenv("EULERHIP_VERBOSE", "1")
    from structured import oracle_of, reads_of

    buf, off = reads_of("repeat_families", 31)
    ref = oracle_of("repeat_families", 31)
    with eulerhip.Session(0) as s:
        for call in range(3):
            capfd.readouterr()
            res = _run(s, buf, off, 31)
            err = capfd.readouterr().err
            assert "refined again with capacity" in err, err
            assert res.contig_bytes == ref["contig_chars"], call
            assert np.array_equal(res.contig_offsets, ref["contig_offsets"]), call
            assert res.links == ref["links_unpacked"], call
        c = s.spec_counts()
    # (the overflow is seen at the read-back the prologue sits behind: queued on calls 2 and 3, never kept)
    assert c["links_taken"] == 0 and c["links_redone"] == 2, c


# ---- 6: a ranking whose one ruler pass misses a cycle, in a warm session --------------------------------
def test_rank_redo_in_warm_session(monkeypatch):
    """the inputs of test_rank_async_small_cycles_vs_oracle, all in one session: about one in
    seven leaves a cycle of chains without a ruler, the check rides on the starts' read-back, and
    the ranking and the starts run again behind the fills that now follow that read-back"""
    _local_join(monkeypatch)
    monkeypatch.setenv("EULERHIP_RANK", "2")
    with eulerhip.Session(0) as s:
        for seed in range(16):
            buf, off = make_reads(1_200 + 150 * seed, 1_500, 100, 5100 + seed, err=0.0, circular=True)
            _check(s, ("cycle", seed), 31, buf_off=(buf, off))


# ---- 7: EULERHIP_NO_SPEC, and the calls that never reach the graph phase -------------------------------
def test_no_spec_same_results(monkeypatch):
    _local_join(monkeypatch)
    monkeypatch.setenv("EULERHIP_NO_SPEC", "1")
    with eulerhip.Session(0) as s:
        for key in ("g30k", "g30k", "g30k", "g10k", "g30k", "many", "g30k"):
            _check(s, key, 31)
        _check(s, "g30k", 31, limit=1_000_000)
        _check(s, "g30k", 31)
        assert s.spec_counts() == {"links_taken": 0, "links_redone": 0, "starts_taken": 0, "starts_redone": 0}


def test_count_shard_after_warm_assemble(monkeypatch):
    """ec_count_shard never reaches links_local: no prologue is queued for it, and its export
    after warm assemble calls in the same session equals a fresh session's"""
    _local_join(monkeypatch)
    import distributed

    buf, off = _inputs("g30k")
    d_buf = torch.from_numpy(np.array(buf)).cuda()
    d_off = torch.from_numpy(off.astype(np.int64)).cuda()
    out = []
    for warm in (True, False):
        eng = distributed.HipEngine(0)
        try:
            if warm:
                for _ in range(3):
                    _check(eng.sess, "g30k", 31)
                c0 = eng.sess.spec_counts()
                assert c0["links_taken"] == 2
            eng.count_shard(d_buf, d_off, len(off) - 1, 0, 31, 0)
            if warm:
                assert eng.sess.spec_counts() == c0
            recs, counts = eng.export_by_owner(1)
            raw = np.frombuffer(recs.cpu().numpy().tobytes(), dtype=distributed.REC_DTYPE)
            out.append((np.sort(raw, order="key"), list(counts)))  # (ids inside a bucket follow no fixed order)
        finally:
            eng.sess.close()
    assert out[0][1] == out[1][1]
    for f in ("key", "count", "first_canon", "first_twin"):
        assert np.array_equal(out[0][0][f], out[1][0][f]), f
