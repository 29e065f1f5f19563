"""Bubble popping and per-contig k-mer count sums on the device (ec_pop_bubbles,
ec_copy_contig_kmer_sums, Session.pop_bubbles / contig_kmer_sums, assembler.pop_bubbles,
euler_run.py --pop-bubbles) against the CPU statement of the contract, bubbles_model.py: the
dict, the contigs in order, the links, the PopInfo, the stats counts and the sums must all equal
the model's."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import assembler
import bubbles_model
import eulerhip
import kernel_grid as KG
import tips_model
from conftest import GOLDEN, golden_cases
from model_parallel import model_count, model_graph, twin
from synth import make_reads

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUN = os.path.join(ROOT, "pycuda-euler_amd", "euler_run.py")
WD = eulerhip.EC_FLAG_WANT_DICT
COUNTING = ("n_reads", "n_positions", "n_distinct_est", "n_distinct", "count_path", "count_variant", "n_buckets",
            "record_bytes", "n_records", "table_capacity", "table_retries")
NOTHING = {"rounds": 0, "converged": 1, "n_bubble_contigs": 0, "n_bubble_kmers": 0}

_MODEL = {}


def as_list(buf, off):
    s = np.asarray(buf).tobytes().decode()
    return [s[int(off[i]):int(off[i + 1])] for i in range(len(off) - 1)]


def pack(reads):
    return eulerhip.pack_reads(reads)


def model(key, reads, k, max_bubble_len=0, max_rounds=4):
    """bubbles_model.pop_reads, computed once per input and never changed"""
    key = (key, k, max_bubble_len, max_rounds)
    if key not in _MODEL:
        _MODEL[key] = bubbles_model.pop_reads(reads if isinstance(reads, list) else as_list(*reads), k, 1,
                                              max_bubble_len, max_rounds)
    return _MODEL[key]


def two_hap(k, L):
    key = ("2hap-reads", k, L)
    if key not in _MODEL:
        _MODEL[key] = bubbles_model.two_haplotype_reads(L, 100 + k)
    return _MODEL[key]


def assert_model(res, info, m, with_dict=True):
    d, contigs, links, minfo = m[:4]
    assert info == minfo
    assert res.contigs == contigs
    assert res.links == links
    assert res.stats.n_contigs == len(contigs) and res.stats.n_contig_chars == sum(len(c) for c in contigs)
    assert res.stats.n_links == sum(len(a) + len(b) for a, b in links)
    assert res.stats.n_dict == len(d)
    assert res.stats.n_solid == len({min(x, twin(x)) for x, _ in d})
    if with_dict:
        assert [[x, c] for x, c in res.dict_items] == d


def assert_sums(sess, m, k):
    got = sess.contig_kmer_sums()
    assert got.dtype == np.uint64
    assert got.tolist() == bubbles_model.ksums(m[1], m[0], k)


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
    reads = bubbles_model.hand_reads(k)
    buf, off = pack(reads)
    long_w = 3 * k - 10
    for mb, mr, want in ((0, 2, (1, 1, 1, k)), (4 * k, 3, (2, 1, 2, k + long_w)), (4 * k, 1, (1, 0, 1, k))):
        sess.run_host(buf, off, k, 1, WD)
        assert sess.stats().n_contigs == 7
        assert_sums(sess, _plain("hand", reads, k), k)
        res, info = sess.pop_bubbles(k, mb, mr, want_dict=True)
        assert (info["rounds"], info["converged"], info["n_bubble_contigs"], info["n_bubble_kmers"]) == want
        m = model("hand", reads, k, mb, mr)
        assert_model(res, info, m)
        assert_sums(sess, m, k)
        if (mb, mr) == (4 * k, 3):
            assert len(res.contigs) == 1 and len(res.contigs[0]) == 400


def _plain(key, reads, k):
    """the unpopped assembly as (d, contigs, links), computed once per input"""
    key = ("plain", key, k)
    if key not in _MODEL:
        rl = reads if isinstance(reads, list) else as_list(*reads)
        cnt, first = model_count(rl, k)
        _MODEL[key] = model_graph({c: v for c, v in cnt.items() if v > 1}, first, k)
    return _MODEL[key]


# ---- 2. every index form the count can leave ----------------------------------------------------
CELLS = [(23, 63, 0), (17, 111, 0), (27, 160, 0), (48, 100, 0), (60, 100, 0), (23, 63, eulerhip.EC_FLAG_GENERAL)]


@pytest.mark.parametrize("k,L,flags", CELLS, ids=["%d-%d-%d" % c for c in CELLS])
def test_index_forms(sess, k, L, flags):
    """super-k-mer buckets, window records, the exact path, wide minimizer and wide hash buckets,
    and the HBM table: the sum kernel's lookups go through each index; the contigs of thousands of
    characters the pop leaves take several tiles, in one workgroup and across two"""
    reads = two_hap(k, L)
    m = model(("2hap", L), reads, k)
    assert m[3]["n_bubble_contigs"] >= 8  # (a condition on the input: the model alone decides it)
    assert max(len(c) for c in m[1]) > 2 * 1024 + k  # (pop.h KSUM_TILE = 1024 windows)
    buf, off = pack(reads)
    sess.run_host(buf, off, k, 1, flags)
    before = sess.stats().as_dict()
    if not flags:
        assert (before["count_path"], before["count_variant"], before["record_bytes"]) == \
            KG.expected_path(k, L, len(reads))
    res, info = sess.pop_bubbles(k, 0, 4)
    assert_model(res, info, m, with_dict=False)
    after = res.stats.as_dict()
    assert {f: after[f] for f in COUNTING} == {f: before[f] for f in COUNTING}
    assert_sums(sess, m, k)


# ---- 3. the sums alone ----------------------------------------------------------------------------
def test_sums_on_many_short_contigs(sess):
    k, L = 23, 63
    buf, off = KG.reads_of(k, L)
    sess.run_host(buf, off, k, 1, WD)
    before = snapshot(sess.fetch(k, True))
    assert_sums(sess, _plain(("grid", L), (buf, off), k), k)
    assert snapshot(sess.fetch(k, True)) == before
    # ... and the call left the session's state alone: the clean-ups still run on it
    res, info = sess.pop_bubbles(k, 0, 4, want_dict=True)
    assert_model(res, info, model(("grid", L), (buf, off), k))


# ---- 4. interplay -----------------------------------------------------------------------------------
def _solid_of(d):
    return {min(x, twin(x)): v for x, v in d}


@pytest.mark.parametrize("case", ["grid", "hand"])
def test_clip_pop_clip(sess, case):
    """grid: reads with errors, mostly tips; hand: the tip case and the bubble case side by side,
    where the tips go in two rounds, then the SNP branch, and nothing is left for the last clip"""
    if case == "grid":
        k = 23
        buf, off = KG.reads_of(k, 63)
        reads = as_list(buf, off)
    else:
        k = 15
        reads = tips_model.hand_reads(k) + bubbles_model.hand_reads(k)
        buf, off = pack(reads)
    cnt, first = model_count(reads, k)
    m1 = tips_model.clip_solid({c: v for c, v in cnt.items() if v > 1}, first, k)
    m2 = bubbles_model.pop_solid(_solid_of(m1[0]), first, k)
    m3 = tips_model.clip_solid(_solid_of(m2[0]), first, k)
    assert m1[3]["n_tip_contigs"] >= 1
    if case == "hand":
        assert m2[3]["n_bubble_contigs"] == 1
    sess.run_host(buf, off, k, 1, WD)
    res, info = sess.clip_tips(k, 0, 4, want_dict=True)
    assert_model(res, info, m1)
    res, info = sess.pop_bubbles(k, 0, 4, want_dict=True)
    assert_model(res, info, m2)
    assert_sums(sess, m2, k)
    res, info = sess.clip_tips(k, 0, 4, want_dict=True)
    assert_model(res, info, m3)


def test_nothing_to_pop_leaves_every_result_byte(sess):
    k = 25
    buf, off = make_reads(3000, 600, 80, 31, err=0.0)
    m = model("clean", (buf, off), k)
    assert m[3] == NOTHING
    sess.run_host(buf, off, k, 1, WD)
    before = snapshot(sess.fetch(k, True))
    res, info = sess.pop_bubbles(k, 0, 4, want_dict=True)
    assert info == NOTHING
    assert snapshot(res) == before
    assert_model(res, info, m)


# ---- 5. other entry points ----------------------------------------------------------------------
def test_assembler_entry_points(sess):
    k = 15
    reads = bubbles_model.hand_reads(k)
    d0 = _plain("hand", reads, k)[0]
    order = np.random.Generator(np.random.PCG64(5)).permutation(len(d0))
    d = {d0[i][0]: d0[i][1] for i in order}
    md, mc, ml, minfo, _ = bubbles_model.pop_dict(d, k, 4 * k)
    assert minfo["n_bubble_contigs"] >= 1
    d2, G, r = assembler.pop_bubbles(d, k, max_bubble_len=4 * k, session=sess)
    assert [[x, c] for x, c in d2.items()] == md
    assert r == mc
    assert G == {i: ([tuple(x) for x in a], [tuple(x) for x in b]) for i, (a, b) in enumerate(ml)}
    # assemble's keyword, alone and after the tips
    d3, G3, r3 = assembler.assemble(reads, k, 1, session=sess, pop_bubbles=True)
    m = model("hand", reads, k, 0, 4)
    assert [[x, c] for x, c in d3.items()] == m[0] and r3 == m[1]
    treads = tips_model.hand_reads(k) + reads
    cnt, first = model_count(treads, k)
    m1 = tips_model.clip_solid({c: v for c, v in cnt.items() if v > 1}, first, k)
    m2 = bubbles_model.pop_solid(_solid_of(m1[0]), first, k)
    assert m1[3]["n_tip_contigs"] >= 1 and m2[3]["n_bubble_contigs"] >= 1
    d4, G4, r4 = assembler.assemble(treads, k, 1, session=sess, clip_tips=True, pop_bubbles=True)
    assert [[x, c] for x, c in d4.items()] == m2[0] and r4 == m2[1]
    assert G4 == {i: ([tuple(x) for x in a], [tuple(x) for x in b]) for i, (a, b) in enumerate(m2[2])}


@pytest.mark.parametrize("k", [23, 48])
def test_after_assemble_from_solid(k):
    import distributed
    import torch

    L = 63 if k == 23 else 100
    reads = two_hap(k, L)
    buf, off = pack(reads)
    e = distributed.HipEngine(0)
    try:
        d_reads = torch.from_numpy(np.array(buf)).to(e.device)
        d_off = torch.from_numpy(off.astype(np.int64)).to(e.device)
        e.count_shard(d_reads, d_off, len(off) - 1, 0, k)
        recs, _ = e.export_by_owner(1)
        solid = e.merge_owned(recs, k, 1).clone()
        e.assemble_from_solid(solid, k, WD, fetch=False)
        res, info = e.sess.pop_bubbles(k, 0, 4, want_dict=True)
        sums = e.sess.contig_kmer_sums().tolist()
    finally:
        e.sess.close()
    m = model(("2hap", L), reads, k)
    assert_model(res, info, m)
    assert sums == bubbles_model.ksums(m[1], m[0], k)


# ---- 6. refusals: all on the host, nothing is provoked on the device -------------------------------
def _rcs(s):
    """(rc, message) of both calls on the session as it is"""
    L = eulerhip.lib()
    pi = eulerhip.PopInfo()
    out = []
    rc = L.ec_pop_bubbles(s._h, 0, 4, ctypes.byref(pi))
    out.append((rc, L.ec_last_error().decode()))
    buf = np.zeros(1 << 16, np.uint64)
    rc = L.ec_copy_contig_kmer_sums(s._h, buf.ctypes.data)
    out.append((rc, L.ec_last_error().decode()))
    return out


def _refused(s, word):
    for rc, msg in _rcs(s):
        assert rc == eulerhip.EC_ERR_STATE and word in msg


def _usable(s):
    """the session still assembles, sums and pops"""
    k = 15
    reads = bubbles_model.hand_reads(k)
    s.run_host(*pack(reads), k, 1, WD)
    assert_sums(s, _plain("hand", reads, k), k)
    res, info = s.pop_bubbles(k, 0, 4, want_dict=True)
    assert_model(res, info, model("hand", reads, k, 0, 4))


def test_refused_arguments(sess):
    k = 15
    reads = bubbles_model.hand_reads(k)
    sess.run_host(*pack(reads), k, 1, WD)
    before = snapshot(sess.fetch(k, True))
    L = eulerhip.lib()
    pi = eulerhip.PopInfo()
    for rc in (L.ec_pop_bubbles(sess._h, 0, 4, None), L.ec_pop_bubbles(sess._h, 0, 0, ctypes.byref(pi)),
               L.ec_pop_bubbles(sess._h, 65536, 4, ctypes.byref(pi)), L.ec_copy_contig_kmer_sums(sess._h, None)):
        assert rc == eulerhip.EC_ERR_ARG and L.ec_last_error()
        assert snapshot(sess.fetch(k, True)) == before
    res, info = sess.pop_bubbles(k, 65535, 8, want_dict=True)
    assert_model(res, info, model("hand", reads, k, 65535, 8))


def test_refused_on_a_new_session(sess):
    _refused(sess, "new session")
    _usable(sess)


def test_refused_after_trim(sess):
    k = 15
    sess.run_host(*pack(bubbles_model.hand_reads(k)), k, 1, 0)
    before = snapshot(sess.fetch(k))
    sess.trim(0)
    _refused(sess, "trim")
    assert snapshot(sess.fetch(k)) == before  # (results copied to host memory survive the trim)
    _usable(sess)


def test_refused_after_a_failed_call(sess):
    k = 15
    sess.run_host(*pack(bubbles_model.hand_reads(k)), k, 1, 0)
    with pytest.raises(eulerhip.EulerHipError):
        sess.run_host(*pack(bubbles_model.hand_reads(k)), 64, 1, 0)  # (k > EC_MAX_K: refused on the host)
    _refused(sess, "failed")
    _usable(sess)


def test_refused_on_extended_alphabet_results(sess):
    case = golden_cases("extended.json", alphabet="all")[0]
    res = sess.assemble(case["reads"], case["k"], case["limit"])
    _refused(sess, "extended alphabet")
    assert sess.fetch(case["k"]).contigs == res.contigs == case["contigs"]
    _usable(sess)


@pytest.mark.parametrize("upto", ["count_shard", "graph_finish"])
def test_refused_after_stepwise_calls(upto):
    import distributed
    from test_step_state_gpu import Flow
    from test_tips_gpu import STEPWISE

    k = 23
    buf, off = KG.reads_of(k, 63)
    e = distributed.HipEngine(0)
    try:
        e.sess.run_host(buf, off, k, 1, 0)  # (a pop-able assembly first: the stepwise calls replace it)
        f = Flow(e, buf, off, k).run(STEPWISE[upto])
        before = snapshot(f.result()) if upto == "graph_finish" else None
        _refused(e.sess, "stepwise")
        if before:
            assert snapshot(f.result()) == before
        _usable(e.sess)
    finally:
        e.sess.close()


# ---- 7. command line -------------------------------------------------------------------------------------
def _fa(path, reads):
    with open(path, "w") as f:
        f.write("".join(">r%d\n%s\n" % (i, x) for i, x in enumerate(reads)))


def test_cli_pop_bubbles(tmp_path):
    k = 15
    reads = bubbles_model.hand_reads(k)
    _fa(tmp_path / "hand.fa", reads)
    m = model("hand", reads, k, 4 * k, 4)
    r = subprocess.run([sys.executable, RUN, "-i", "hand.fa", "-k", str(k), "--pop-bubbles", "--bubble-len",
                        str(4 * k), "-o", "c.fa"], cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert (tmp_path / "c.fa").read_text() == "".join(">contig%d\n%s\n" % (i, c) for i, c in enumerate(m[1]))
    assert "pop-bubbles: rounds 2  converged 1  bubble contigs 2  bubble k-mers 50  contigs 7 -> 1" in r.stderr
    # with the tips clipped first
    treads = tips_model.hand_reads(k) + reads
    _fa(tmp_path / "both.fa", treads)
    cnt, first = model_count(treads, k)
    m1 = tips_model.clip_solid({c: v for c, v in cnt.items() if v > 1}, first, k)
    m2 = bubbles_model.pop_solid(_solid_of(m1[0]), first, k)
    r = subprocess.run([sys.executable, RUN, "-i", "both.fa", "-k", str(k), "--clip-tips", "--pop-bubbles", "-o",
                        "c2.fa"], cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert (tmp_path / "c2.fa").read_text() == "".join(">contig%d\n%s\n" % (i, c) for i, c in enumerate(m2[1]))
    assert "clip-tips: rounds %d  converged %d  tip contigs %d  tip k-mers %d" % (
        m1[3]["rounds"], m1[3]["converged"], m1[3]["n_tip_contigs"], m1[3]["n_tip_kmers"]) in r.stderr
    assert "pop-bubbles: rounds %d  converged %d  bubble contigs %d  bubble k-mers %d  contigs %d -> %d" % (
        m2[3]["rounds"], m2[3]["converged"], m2[3]["n_bubble_contigs"], m2[3]["n_bubble_kmers"], len(m1[1]),
        len(m2[1])) in r.stderr


def test_cli_refuses_sharded(tmp_path):
    fa = os.path.join(GOLDEN, "g200reads.fa")
    r = subprocess.run([sys.executable, RUN, "-i", fa, "-k", "9", "--pop-bubbles", "--sharded", "-o", "c.fa"],
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    assert "--pop-bubbles works on the one-process fused path only" in r.stderr
    assert not (tmp_path / "c.fa").exists()
    r = subprocess.run([sys.executable, RUN, "-i", fa, "-k", "9", "--pop-bubbles", "--bubble-len", "65536"],
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--bubble-len" in r.stderr
