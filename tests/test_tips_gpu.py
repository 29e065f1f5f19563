"""Tip clipping on the device (ec_clip_tips, Session.clip_tips, assembler.clip_tips,
euler_run.py --clip-tips) against the CPU statement of the contract, tips_model.py: the dict,
the contigs in order, the links and the ClipInfo must all equal the model's."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import assembler
import eulerhip
import kernel_grid as KG
import oracle
import tips_model
from conftest import GOLDEN, golden_cases
from synth import make_reads

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUN = os.path.join(ROOT, "pycuda-euler_amd", "euler_run.py")
WD = eulerhip.EC_FLAG_WANT_DICT
COUNTING = ("n_reads", "n_positions", "n_distinct_est", "n_distinct", "count_path", "count_variant", "n_buckets",
            "record_bytes", "n_records", "table_capacity", "table_retries")

_MODEL = {}


def as_list(buf, off):
    s = np.asarray(buf).tobytes().decode()
    return [s[int(off[i]):int(off[i + 1])] for i in range(len(off) - 1)]


def pack(reads):
    return eulerhip.pack_reads(reads)


def model(key, reads, k, max_tip_len=0, max_rounds=4):
    """tips_model.clip_reads, computed once per input and never changed"""
    key = (key, k, max_tip_len, max_rounds)
    if key not in _MODEL:
        _MODEL[key] = tips_model.clip_reads(reads if isinstance(reads, list) else as_list(*reads), k, 1, max_tip_len,
                                            max_rounds)
    return _MODEL[key]


def assert_model(res, info, m, with_dict=True):
    d, contigs, links, minfo, _ = m
    assert info == minfo
    assert res.contigs == contigs
    assert res.links == links
    assert res.stats.n_contigs == len(contigs) and res.stats.n_contig_chars == sum(len(c) for c in contigs)
    assert res.stats.n_links == sum(len(a) + len(b) for a, b in links)
    assert res.stats.n_dict == len(d)
    if with_dict:
        assert [[x, c] for x, c in res.dict_items] == d


def snapshot(res):
    return (res.contig_bytes, res.contig_offsets.tobytes(), res.link_offsets.tobytes(), res.link_codes.tobytes(),
            res.dict_items, res.stats.as_dict())


@pytest.fixture
def sess():
    s = eulerhip.Session(0)
    yield s
    s.close()


# ---- 1. the hand case ---------------------------------------------------------------------------
@pytest.mark.parametrize("k", [15, 33])
def test_hand_case(sess, k):
    reads = tips_model.hand_reads(k)
    buf, off = pack(reads)
    for mr, want in ((1, (1, 0, 2, 6)), (2, (2, 0, 3, 18)), (8, (2, 1, 3, 18))):
        sess.run_host(buf, off, k, 1, WD)
        assert sess.stats().n_contigs == 8
        res, info = sess.clip_tips(k, 0, mr, want_dict=True)
        assert (info["rounds"], info["converged"], info["n_tip_contigs"], info["n_tip_kmers"]) == want
        assert_model(res, info, model(("hand", 12), reads, k, 0, mr))
    assert [len(c) for c in res.contigs] == [403, k + 4]


# ---- 2. every index form the count can leave ----------------------------------------------------
CELLS = [(23, 63, 0), (17, 111, 0), (27, 160, 0), (48, 100, 0), (60, 100, 0), (23, 63, eulerhip.EC_FLAG_GENERAL)]


@pytest.mark.parametrize("k,L,flags", CELLS, ids=["%d-%d-%d" % c for c in CELLS])
def test_index_forms(sess, k, L, flags):
    """super-k-mer buckets, window records, the exact path, wide minimizer and wide hash buckets,
    and the HBM table: the kill kernel's lookups go through each index"""
    buf, off = KG.reads_of(k, L)
    m = model(("grid", L), (buf, off), k)
    assert m[3]["n_tip_contigs"] >= 1  # (a condition on the input: the model alone decides it)
    sess.run_host(buf, off, k, 1, flags)
    before = sess.stats().as_dict()
    if not flags:
        assert (before["count_path"], before["count_variant"], before["record_bytes"]) == \
            KG.expected_path(k, L, KG.NREADS)
    res, info = sess.clip_tips(k, 0, 4)
    assert_model(res, info, m, with_dict=False)
    after = res.stats.as_dict()
    assert {f: after[f] for f in COUNTING} == {f: before[f] for f in COUNTING}


# ---- 3. other entry points ----------------------------------------------------------------------
def test_assembler_clip_tips_on_shuffled_dict(sess):
    k = 15
    d0 = tips_model.clip_reads(tips_model.hand_reads(k), k, 1, 0, 1)[0]  # (one round: tips are left)
    items = [(x, c) for x, c in d0]
    order = np.random.Generator(np.random.PCG64(5)).permutation(len(items))
    d = {items[i][0]: items[i][1] for i in order}
    md, mc, ml, minfo, _ = tips_model.clip_dict(d, k)
    assert minfo["n_tip_contigs"] >= 1
    d2, G, r = assembler.clip_tips(d, k, session=sess)
    assert [[x, c] for x, c in d2.items()] == md
    assert r == mc
    assert G == {i: ([tuple(x) for x in a], [tuple(x) for x in b]) for i, (a, b) in enumerate(ml)}
    # and assembler.assemble's keyword
    reads = tips_model.hand_reads(k)
    d3, G3, r3 = assembler.assemble(reads, k, 1, session=sess, clip_tips=True)
    m = model(("hand", 12), reads, k, 0, 4)
    assert [[x, c] for x, c in d3.items()] == m[0] and r3 == m[1]


@pytest.mark.parametrize("k", [23, 48])
def test_after_assemble_from_solid(k):
    import distributed
    import torch

    buf, off = KG.reads_of(k, 63 if k == 23 else 100)
    e = distributed.HipEngine(0)
    try:
        d_reads = torch.from_numpy(np.array(buf)).to(e.device)
        d_off = torch.from_numpy(off.astype(np.int64)).to(e.device)
        e.count_shard(d_reads, d_off, len(off) - 1, 0, k)
        recs, _ = e.export_by_owner(1)
        solid = e.merge_owned(recs, k, 1).clone()
        e.assemble_from_solid(solid, k, WD, fetch=False)
        res, info = e.sess.clip_tips(k, 0, 4, want_dict=True)
    finally:
        e.sess.close()
    assert_model(res, info, model(("grid", 63 if k == 23 else 100), (buf, off), k))


def test_after_packed_host(sess):
    k, L = 23, 63
    buf, off = KG.reads_of(k, L)
    sess.run_packed_host(eulerhip.pack_2bit(buf, off), k, 1, WD)
    res, info = sess.clip_tips(k, 0, 4, want_dict=True)
    assert_model(res, info, model(("grid", L), (buf, off), k))


# ---- 4. reads with N, reads of two lengths -------------------------------------------------------
def test_reads_with_n(sess):
    k = 21
    buf, off = make_reads(2000, 1500, 50, 11, err=0.01, n_rate=0.003)
    sess.run_host(buf, off, k, 1, WD)
    res, info = sess.clip_tips(k, 0, 4, want_dict=True)
    assert_model(res, info, model("nreads", (buf, off), k))


def test_two_read_lengths(sess):
    k = 33
    buf, off = KG.two_length_reads(k)
    sess.run_host(buf, off, k, 1, WD)
    res, info = sess.clip_tips(k, 0, 4, want_dict=True)
    assert_model(res, info, model("two", (buf, off), k))


# ---- 5. tips of more than 64 windows -------------------------------------------------------------
def test_long_tips(sess):
    k = 15
    reads = tips_model.hand_reads(k, branch=100)
    m = model(("hand", 100), reads, k, 150, 8)
    assert max(h[2] for h in m[4]) > 64  # (one tip alone has 100 windows: the kill kernel loops)
    sess.run_host(*pack(reads), k, 1, WD)
    res, info = sess.clip_tips(k, 150, 8, want_dict=True)
    assert_model(res, info, m)
    # the default bound leaves the long branch in place
    sess.run_host(*pack(reads), k, 1, WD)
    res, info = sess.clip_tips(k, 0, 8, want_dict=True)
    assert_model(res, info, model(("hand", 100), reads, k, 0, 8))


# ---- 6. no-op and idempotence ---------------------------------------------------------------------
def test_no_tip_leaves_every_result_byte(sess):
    k = 25
    buf, off = make_reads(3000, 600, 80, 31, err=0.0)
    m = model("clean", (buf, off), k)
    assert m[3] == {"rounds": 0, "converged": 1, "n_tip_contigs": 0, "n_tip_kmers": 0}
    sess.run_host(buf, off, k, 1, WD)
    before = snapshot(sess.fetch(k, True))
    res, info = sess.clip_tips(k, 0, 4, want_dict=True)
    assert info == m[3]
    assert snapshot(res) == before
    assert_model(res, info, m)


def test_second_call_after_convergence_is_a_no_op(sess):
    k = 15
    reads = tips_model.hand_reads(k)
    sess.run_host(*pack(reads), k, 1, WD)
    res, info = sess.clip_tips(k, 0, 8, want_dict=True)
    assert info["converged"] == 1 and info["rounds"] == 2
    before = snapshot(res)
    res2, info2 = sess.clip_tips(k, 0, 8, want_dict=True)
    assert info2 == {"rounds": 0, "converged": 1, "n_tip_contigs": 0, "n_tip_kmers": 0}
    assert snapshot(res2) == before
    # a clip that stopped at max_rounds continues where it stopped
    sess.run_host(*pack(reads), k, 1, WD)
    sess.clip_tips(k, 0, 1)
    res3, info3 = sess.clip_tips(k, 0, 8, want_dict=True)
    assert (info3["rounds"], info3["converged"], info3["n_tip_contigs"], info3["n_tip_kmers"]) == (1, 1, 1, 12)
    assert snapshot(res3)[:5] == before[:5]


# ---- 7. session hygiene -----------------------------------------------------------------------------
def _assert_oracle(res, ref):
    assert res.contig_bytes == ref["contig_chars"]
    assert np.array_equal(res.contig_offsets, ref["contig_offsets"])
    assert np.array_equal(res.link_offsets, ref["link_offsets"])
    assert np.array_equal(res.link_codes, ref["links"])
    assert [[x, c] for x, c in res.dict_items] == ref["d"]


@pytest.mark.parametrize("trim", [False, True])
def test_assembly_after_a_clip(sess, trim):
    k = 23
    sess.run_host(*KG.reads_of(k, 63), k, 1, 0)
    _, info = sess.clip_tips(k)
    assert info["rounds"] == 1
    if trim:
        sess.trim(0)
    for k2, L2 in ((27, 160), (48, 100), (23, 63)):
        sess.run_host(*KG.reads_of(k2, L2), k2, 1, WD)
        _assert_oracle(sess.fetch(k2, True), KG.oracle_of(k2, L2))


# ---- 8. refusals ---------------------------------------------------------------------------------------
def _clip_rc(s, max_tip_len=0, max_rounds=4, info=True):
    ci = eulerhip.ClipInfo()
    L = eulerhip.lib()
    rc = L.ec_clip_tips(s._h, max_tip_len, max_rounds, ctypes.byref(ci) if info else None)
    return rc, L.ec_last_error().decode()


def _usable(s):
    """the session still assembles and clips"""
    k = 15
    reads = tips_model.hand_reads(k)
    s.run_host(*pack(reads), k, 1, WD)
    res, info = s.clip_tips(k, 0, 4, want_dict=True)
    assert_model(res, info, model(("hand", 12), reads, k, 0, 4))


def test_refused_arguments(sess):
    k = 15
    sess.run_host(*pack(tips_model.hand_reads(k)), k, 1, WD)
    before = snapshot(sess.fetch(k, True))
    for kw in ({"info": False}, {"max_rounds": 0}):
        rc, msg = _clip_rc(sess, **kw)
        assert rc == eulerhip.EC_ERR_ARG and msg
        assert snapshot(sess.fetch(k, True)) == before
    # the refused calls changed nothing: the clip still runs on the same assembly
    res, info = sess.clip_tips(k, 0, 8, want_dict=True)
    assert_model(res, info, model(("hand", 12), tips_model.hand_reads(k), k, 0, 8))


def test_refused_on_a_new_session(sess):
    rc, msg = _clip_rc(sess)
    assert rc == eulerhip.EC_ERR_STATE and "new session" in msg
    _usable(sess)


def test_refused_after_trim(sess):
    k = 15
    sess.run_host(*pack(tips_model.hand_reads(k)), k, 1, 0)
    before = snapshot(sess.fetch(k))
    sess.trim(0)
    rc, msg = _clip_rc(sess)
    assert rc == eulerhip.EC_ERR_STATE and "trim" in msg
    assert snapshot(sess.fetch(k)) == before  # (results copied to host memory survive the trim)
    _usable(sess)


def test_refused_after_a_failed_call(sess):
    k = 15
    sess.run_host(*pack(tips_model.hand_reads(k)), k, 1, 0)
    with pytest.raises(eulerhip.EulerHipError):
        sess.run_host(*pack(tips_model.hand_reads(k)), 64, 1, 0)
    rc, msg = _clip_rc(sess)
    assert rc == eulerhip.EC_ERR_STATE and "failed" in msg
    _usable(sess)


def test_refused_on_extended_alphabet_results(sess):
    case = golden_cases("extended.json", alphabet="all")[0]
    res = sess.assemble(case["reads"], case["k"], case["limit"])
    rc, msg = _clip_rc(sess)
    assert rc == eulerhip.EC_ERR_STATE and "extended alphabet" in msg
    assert sess.fetch(case["k"]).contigs == res.contigs == case["contigs"]
    _usable(sess)


STEPWISE = {"count_shard": ["count"], "merge_owned": ["count", "export", "merge"],
            "graph_load": ["count", "export", "merge", "export_dense", "load"],
            "graph_finish": ["count", "export", "merge", "export_dense", "load", "links_part", "finish"],
            "graph_place": ["count", "export", "merge", "place"], "collect_runs": None}


@pytest.mark.parametrize("upto", sorted(STEPWISE))
def test_refused_after_stepwise_calls(upto):
    import distributed
    from test_step_state_gpu import Flow

    k = 23
    buf, off = KG.reads_of(k, 63)
    e = distributed.HipEngine(0)
    try:
        e.sess.run_host(buf, off, k, 1, 0)  # (a clip-able assembly first: the stepwise calls replace it)
        f = Flow(e, buf, off, k).run(STEPWISE[upto] or Flow.RUNS)
        fetchable = upto in ("graph_finish", "collect_runs")
        before = snapshot(f.result()) if fetchable else None
        rc, msg = _clip_rc(e.sess)
        assert rc == eulerhip.EC_ERR_STATE and "stepwise" in msg
        if fetchable:
            assert snapshot(f.result()) == before
            _assert_oracle_nodict(f.result(), KG.oracle_of(k, 63))
        _usable(e.sess)
    finally:
        e.sess.close()


def _assert_oracle_nodict(res, ref):
    assert res.contig_bytes == ref["contig_chars"]
    assert np.array_equal(res.link_codes, ref["links"])


# ---- 9. command line -------------------------------------------------------------------------------------
def test_cli_clip_tips(tmp_path):
    k = 9
    fa = os.path.join(GOLDEN, "g200reads.fa")
    reads = assembler.read_fasta_records(fa)
    m = model("g200", reads, k)
    r = subprocess.run([sys.executable, RUN, "-i", fa, "-k", str(k), "--clip-tips", "-o", "c.fa"], cwd=str(tmp_path),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert (tmp_path / "c.fa").read_text() == "".join(">contig%d\n%s\n" % (i, c) for i, c in enumerate(m[1]))
    assert "clip-tips: rounds %d  converged %d  tip contigs %d  tip k-mers %d" % (
        m[3]["rounds"], m[3]["converged"], m[3]["n_tip_contigs"], m[3]["n_tip_kmers"]) in r.stderr
    # (the golden reads have no tip at limit 1) the hand case from a file, one round of longer tips
    k = 15
    reads = tips_model.hand_reads(k)
    with open(tmp_path / "hand.fa", "w") as f:
        f.write("".join(">r%d\n%s\n" % (i, x) for i, x in enumerate(reads)))
    m1 = model(("hand", 12), reads, k, 40, 1)
    assert m1[3]["n_tip_contigs"] >= 1
    r = subprocess.run([sys.executable, RUN, "-i", "hand.fa", "-k", str(k), "--clip-tips", "--tip-len", "40",
                        "--tip-rounds", "1", "-o", "c1.fa"], cwd=str(tmp_path), capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert (tmp_path / "c1.fa").read_text() == "".join(">contig%d\n%s\n" % (i, c) for i, c in enumerate(m1[1]))
    assert "clip-tips: rounds 1  converged 0  tip contigs %d  tip k-mers %d  contigs 8 -> %d" % (
        m1[3]["n_tip_contigs"], m1[3]["n_tip_kmers"], len(m1[1])) in r.stderr


def test_cli_refuses_sharded(tmp_path):
    fa = os.path.join(GOLDEN, "g200reads.fa")
    r = subprocess.run([sys.executable, RUN, "-i", fa, "-k", "9", "--clip-tips", "--sharded", "-o", "c.fa"],
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    assert "--clip-tips works on the one-process fused path only" in r.stderr
    assert not (tmp_path / "c.fa").exists()
