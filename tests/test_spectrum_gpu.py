"""The coverage-aware solid threshold on the device (ec_kmer_spectrum, ec_refilter,
Session.kmer_spectrum / refilter / auto_limit, assembler.assemble(auto_limit=True),
assembler.kmer_spectrum, euler_run.py --auto-limit) against the CPU statement spectrum_model.py and
against the reference: assemble(limit=1) followed by refilter(L) must be bit-identical to a fresh
assemble(limit=L) and to the oracle's build(limit=L) + all_contigs -- contigs and their order, the
link table, the dict with its order and counts, and the stats counts.

The read sets and the numbers expected of them are the fixed cases of test_spectrum.py."""
import collections
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
import oracle
import spectrum_model
import tips_model
from conftest import GOLDEN, golden_cases
from model_parallel import model_count, twin
from spectrum_model import FIXED, info_of
from synth import make_reads

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUN = os.path.join(ROOT, "pycuda-euler_amd", "euler_run.py")
WD = eulerhip.EC_FLAG_WANT_DICT
GENERAL = eulerhip.EC_FLAG_GENERAL
COUNTING = ("n_reads", "n_positions", "n_distinct_est", "n_distinct", "count_path", "count_variant", "n_buckets",
            "record_bytes", "n_records", "table_capacity", "table_retries")
RESULT = ("n_solid", "n_dict", "n_contigs", "n_contig_chars", "n_links")
ROWS = {c[5]: (c, w) for c, w in FIXED[:5]}  # by k: 21, 23, 15, 31, 33 (the rows with a limit)
LOWCOV = FIXED[5]
# the composition tests' read set: an 800-base genome, so that the pure-Python graph model, whose
# ranking walks every path from every node, stays quick on the long contigs the clean-ups leave.
# Computed with the models alone: 1850 solid k-mers; limit 5 keeps 764 of the genome's 780; at
# limit 2 there are 4 tips and 1 bubble, at limit 1 76 tips in two rounds
SMALL = ((800, 480, 100, 12, 0.02, 21), (1, 2, 5, 37, 1, 5, 1850, 764))
NBINS = (2, 32, 1024, 4096)

_CACHE = {}


def cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def reads_of(case):
    """(buf, off) of a fixed case, built once and never changed"""
    G, n, L, seed, err, _ = case
    return cached(("reads", case[:5]), lambda: make_reads(G, n, L, seed, err=err))


def as_list(buf, off):
    s = np.asarray(buf).tobytes().decode()
    return [s[int(off[i]):int(off[i + 1])] for i in range(len(off) - 1)]


def oracle_of(case, L):
    """the reference's build(limit=L) + all_contigs on a fixed case, computed once per (case, L)"""
    return cached(("oracle", case, L), lambda: oracle.assemble_packed(*reads_of(case), case[5], L, want_dict=True))


def counted(case):
    """model_count of a fixed case: (canonical -> count, string -> first event)"""
    return cached(("count", case), lambda: model_count(as_list(*reads_of(case)), case[5]))


def snapshot(res):
    return (res.contig_bytes, res.contig_offsets.tobytes(), res.link_offsets.tobytes(), res.link_codes.tobytes(),
            res.dict_items, res.stats.as_dict())


def assert_oracle(res, ref, with_dict=True):
    assert res.contig_bytes == ref["contig_chars"]
    assert np.array_equal(res.contig_offsets, ref["contig_offsets"])
    assert np.array_equal(res.link_offsets, ref["link_offsets"])
    assert np.array_equal(res.link_codes, ref["links"])
    st = res.stats
    assert (st.n_contigs, st.n_contig_chars, st.n_links) == (len(ref["contig_offsets"]) - 1,
                                                              len(ref["contig_chars"]), len(ref["links"]))
    assert st.n_dict == ref["n_dict"]
    if with_dict:
        assert [[x, c] for x, c in res.dict_items] == ref["d"]
        assert st.n_solid == len({min(x, twin(x)) for x, _ in ref["d"]})


def assert_same(res, fresh, with_dict=True):
    """res against the results of a fresh assembly on another session"""
    a, b = snapshot(res), snapshot(fresh)
    assert a[:4] == b[:4]
    if with_dict:
        assert a[4] == b[4]
    assert {f: a[5][f] for f in RESULT} == {f: b[5][f] for f in RESULT}


def assert_model(res, m, with_dict=True):
    d, contigs, links = m[:3]
    assert res.contigs == contigs
    assert res.links == links
    assert res.stats.n_contigs == len(contigs) and res.stats.n_contig_chars == sum(len(c) for c in contigs)
    assert res.stats.n_links == sum(len(a) + len(b) for a, b in links)
    assert res.stats.n_dict == len(d)
    assert res.stats.n_solid == len({min(x, twin(x)) for x, _ in d})
    if with_dict:
        assert [[x, c] for x, c in res.dict_items] == d


def assert_spectra(s, items, n_solid, nbins=NBINS):
    for nb in nbins:
        h = s.kmer_spectrum(nb)
        assert h.dtype == np.uint64 and h.shape == (nb,)
        assert h.tolist() == spectrum_model.spectrum(items, nb)
        assert int(h.sum()) == n_solid


def limits_of(want):
    return sorted({2, 3, want[5]})


@pytest.fixture(scope="module")
def sess():
    s = eulerhip.Session(0)
    yield s
    s.close()


@pytest.fixture(scope="module")
def fresh():
    s = eulerhip.Session(0)
    yield s
    s.close()


# ---- 1. the spectrum ------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, GENERAL], ids=["default", "general"])
@pytest.mark.parametrize("k", [15, 21, 31, 33])
def test_spectrum_equals_model(sess, k, flags):
    case, want = ROWS[k]
    sess.run_host(*reads_of(case), k, 1, WD | flags)
    res = sess.fetch(k, True)
    assert [[x, c] for x, c in res.dict_items] == oracle_of(case, 1)["d"]
    assert res.stats.n_solid == want[6]
    assert_spectra(sess, res.dict_items, want[6])
    h = sess.kmer_spectrum(256)
    assert eulerhip.spectrum_threshold(h) == info_of(*want[:6])
    assert int(h[want[5] + 1:].sum()) == want[7]
    if k in (15, 21):  # 32 bins: the same limit / the peak in the saturating bin
        si = eulerhip.spectrum_threshold(sess.kmer_spectrum(32))
        assert si == (info_of(*want[:6]) if k == 15 else info_of(0, 2, 4, 31, 0, 0))


@pytest.mark.parametrize("k", [4, 6])
def test_spectrum_with_palindromes(sess, k):
    """an even k: a palindrome's dict count holds 2 per occurrence, and that is what is binned"""
    reads = ["ACGTACGTACGT", "AATTCCGGAATT", "GATCGATCA", "ACGTTGCAAT", "TTGCGCAAGC"] * 2 + ["GGATCC", "ACGT"]
    res = sess.assemble(reads, k, 1, want_dict=True)
    ref = oracle.assemble(reads, k, 1)
    assert [[x, c] for x, c in res.dict_items] == ref[0]
    pal = [(x, c) for x, c in res.dict_items if x == twin(x)]
    assert pal and all(c % 2 == 0 for _, c in pal)
    assert_spectra(sess, res.dict_items, res.stats.n_solid, (2, 5, 32))
    L = 3
    res2, info = sess.refilter(k, L, want_dict=True)
    ref = oracle.assemble(reads, k, L)
    assert [[x, c] for x, c in res2.dict_items] == ref[0] and res2.contigs == ref[1] and res2.links == ref[2]
    assert info == {"limit": L, "changed": 1, "n_removed_kmers": res.stats.n_solid - res2.stats.n_solid}


def test_no_solid_kmer(sess):
    """every read shorter than k: U = 0, no kernel runs"""
    k = 15
    res = sess.assemble(["ACGTACGT", "GGATTACA", "ACG"], k, 1, want_dict=True)
    assert res.stats.n_solid == 0 and res.contigs == []
    before = snapshot(res)
    for nb in NBINS:
        assert sess.kmer_spectrum(nb).tolist() == [0] * nb
    res, info = sess.refilter(k, 3, want_dict=True)
    assert info == {"limit": 3, "changed": 0, "n_removed_kmers": 0} and snapshot(res) == before
    res, si, ri = sess.auto_limit(k, want_dict=True)
    assert si == info_of(0, 0, 0, 0, 0, 0) and ri["changed"] == 0 and snapshot(res) == before


@pytest.mark.parametrize("rem", [0, 1, 2, 3])
def test_every_tail_of_the_quad_loads(sess, rem):
    """U % 4 = 0 .. 3, from a caller's dict (ec_assemble_from_kmers state): the spectrum, then the
    re-filter against the model on that dict"""
    case, want = SMALL
    k, L = 21, 3
    items = oracle_of(case, 1)["d"]
    canon = list(collections.OrderedDict((min(x, twin(x)), None) for x, _ in items))
    U = len(canon) - 8 - ((len(canon) - rem) % 4)
    assert U % 4 == rem
    keep = set(canon[:U])
    d = collections.OrderedDict((x, c) for x, c in items if min(x, twin(x)) in keep)
    res = sess.assemble_dict(d, k, keep_dict=True)
    assert res.stats.n_solid == U
    assert_spectra(sess, d, U, (2, 64, 4096))
    m = cached(("tail", rem), lambda: spectrum_model.refilter(d, k, L))
    res, info = sess.refilter(k, L, want_dict=True)
    assert_model(res, m)
    assert info == {"limit": L, "changed": 1, "n_removed_kmers": U - res.stats.n_solid}
    assert_spectra(sess, m[0], res.stats.n_solid, (64,))


def test_spectrum_changes_no_state(sess):
    case, want = ROWS[23]
    k = 23
    sess.run_host(*reads_of(case), k, 1, WD)
    before = snapshot(sess.fetch(k, True))
    h1 = sess.kmer_spectrum(1024)
    h2 = sess.kmer_spectrum(1024)
    assert np.array_equal(h1, h2)
    assert snapshot(sess.fetch(k, True)) == before
    sums = sess.contig_kmer_sums()
    assert np.array_equal(sess.kmer_spectrum(1024), h1)
    assert np.array_equal(sess.contig_kmer_sums(), sums)
    assert snapshot(sess.fetch(k, True)) == before
    # ... and the clean-ups and the re-filter still run on it
    res, info = sess.refilter(k, want[5], want_dict=True)
    assert_oracle(res, oracle_of(case, want[5]))


# ---- 2. refilter parity -----------------------------------------------------------------------------
PARITY = [(k, 0) for k in (15, 21, 23, 31, 33)] + [(21, GENERAL), (33, GENERAL)]


@pytest.mark.parametrize("k,flags", PARITY, ids=["%d-%d" % p for p in PARITY])
def test_refilter_equals_fresh_assembly_and_oracle(sess, fresh, k, flags):
    case, want = ROWS[k]
    buf, off = reads_of(case)
    for L in limits_of(want):
        sess.run_host(buf, off, k, 1, WD | flags)
        first = sess.stats().as_dict()
        assert first["n_solid"] == want[6]
        res, info = sess.refilter(k, L, want_dict=True)
        fresh.run_host(buf, off, k, L, WD)
        assert_same(res, fresh.fetch(k, True))
        assert_oracle(res, oracle_of(case, L))
        after = res.stats.as_dict()
        assert {f: after[f] for f in COUNTING} == {f: first[f] for f in COUNTING}
        assert info == {"limit": L, "changed": 1, "n_removed_kmers": want[6] - after["n_solid"]}
        if L == want[5]:
            assert after["n_solid"] == want[7]
        assert_spectra(sess, res.dict_items, after["n_solid"], (256,))


def test_refilter_in_steps(sess):
    """the filters nest: 2, then 3, then v on one assembly end where refilter(v) alone ends"""
    case, want = ROWS[31]
    k = 31
    sess.run_host(*reads_of(case), k, 1, WD)
    left = want[6]
    for L in limits_of(want):
        res, info = sess.refilter(k, L, want_dict=True)
        assert_oracle(res, oracle_of(case, L))
        assert info == {"limit": L, "changed": 1, "n_removed_kmers": left - res.stats.n_solid}
        left = res.stats.n_solid
    assert left == want[7]
    # a lower limit afterwards finds nothing to remove
    before = snapshot(res)
    res, info = sess.refilter(k, 2, want_dict=True)
    assert info == {"limit": 2, "changed": 0, "n_removed_kmers": 0} and snapshot(res) == before


@pytest.mark.parametrize("k", [23, 33])
def test_after_assemble_from_solid(k):
    import distributed
    import torch

    case, want = ROWS[k]
    buf, off = reads_of(case)
    e = distributed.HipEngine(0)
    try:
        d_reads = torch.from_numpy(np.array(buf)).to(e.device)
        d_off = torch.from_numpy(off.astype(np.int64)).to(e.device)
        e.count_shard(d_reads, d_off, len(off) - 1, 0, k)
        recs, _ = e.export_by_owner(1)
        solid = e.merge_owned(recs, k, 1).clone()
        e.assemble_from_solid(solid, k, WD, fetch=False)
        h = e.sess.kmer_spectrum(256)
        res, info = e.sess.refilter(k, want[5], want_dict=True)
    finally:
        e.sess.close()
    assert h.tolist() == spectrum_model.spectrum(oracle_of(case, 1)["d"], 256)
    assert_oracle(res, oracle_of(case, want[5]))
    assert info == {"limit": want[5], "changed": 1, "n_removed_kmers": want[6] - want[7]}


# ---- 3. composition -----------------------------------------------------------------------------------
def _solid_of(d):
    return {min(x, twin(x)): v for x, v in d}


def _clean_models(case, L):
    """build(limit=L), then the tips clipped, then the bubbles popped: (m1, m2)"""
    def make():
        cnt, first = counted(case)
        m1 = tips_model.clip_solid({c: v for c, v in cnt.items() if v > L}, first, case[5])
        m2 = bubbles_model.pop_solid(_solid_of(m1[0]), first, case[5])
        return m1, m2
    return cached(("clean", case, L), make)


def test_refilter_then_clip_then_pop(sess):
    case, want = SMALL
    k, L = 21, 2
    m1, m2 = _clean_models(case, L)
    # (conditions on the input: limit 2 leaves error k-mers)
    assert m1[3]["n_tip_contigs"] == 4 and m2[3]["n_bubble_contigs"] == 1
    sess.run_host(*reads_of(case), k, 1, WD)
    sess.refilter(k, L)
    res, info = sess.clip_tips(k, 0, 4, want_dict=True)
    assert info == m1[3]
    assert_model(res, m1)
    res, info = sess.pop_bubbles(k, 0, 4, want_dict=True)
    assert info == m2[3]
    assert_model(res, m2)


def test_clip_then_refilter(sess):
    case, want = SMALL
    k, L = 21, 3
    m1, _ = _clean_models(case, 1)
    assert m1[3]["n_tip_contigs"] == 76 and m1[3]["rounds"] == 2
    m = cached(("clip-refilter", case, L), lambda: spectrum_model.refilter(m1[0], k, L))
    sess.run_host(*reads_of(case), k, 1, WD)
    res, info = sess.clip_tips(k, 0, 4, want_dict=True)
    assert info == m1[3]
    n0 = res.stats.n_solid
    assert_spectra(sess, m1[0], n0, (256,))
    res, info = sess.refilter(k, L, want_dict=True)
    assert_model(res, m)
    assert info == {"limit": L, "changed": 1, "n_removed_kmers": n0 - res.stats.n_solid}


def test_auto_limit_applies_the_rows_limit(sess):
    case, want = ROWS[21]
    k = 21
    sess.run_host(*reads_of(case), k, 1, WD)
    res, si, ri = sess.auto_limit(k, 256, want_dict=True)
    assert si == info_of(*want[:6])
    assert ri == {"limit": want[5], "changed": 1, "n_removed_kmers": want[6] - want[7]}
    assert res.stats.n_solid == want[7]
    assert_oracle(res, oracle_of(case, want[5]))
    # the default bins give the same
    sess.run_host(*reads_of(case), k, 1, WD)
    res2, si2, ri2 = sess.auto_limit(k, want_dict=True)
    assert (si2, ri2) == (si, ri)
    assert_same(res2, res)


def test_auto_limit_without_a_threshold_leaves_every_result_byte(sess):
    case, want = LOWCOV
    k = case[5]
    sess.run_host(*reads_of(case), k, 1, WD)
    before = snapshot(sess.fetch(k, True))
    assert before[5]["n_solid"] == want[6]
    res, si, ri = sess.auto_limit(k, 256, want_dict=True)
    assert si == info_of(*want[:6]) and si["found"] == 0
    assert ri == {"limit": 0, "changed": 0, "n_removed_kmers": 0}
    assert snapshot(res) == before


@pytest.mark.parametrize("k", [21, 33])
def test_nothing_to_remove_leaves_every_result_byte(sess, k):
    case, want = ROWS[k]
    sess.run_host(*reads_of(case), k, 1, WD)
    before = snapshot(sess.fetch(k, True))
    for L in (0, 1):
        res, info = sess.refilter(k, L, want_dict=True)
        assert info == {"limit": L, "changed": 0, "n_removed_kmers": 0}
        assert snapshot(res) == before
    res, info = sess.refilter(k, want[5], want_dict=True)  # (the session is as usable as before)
    assert_oracle(res, oracle_of(case, want[5]))


# ---- 4. refusals: all on the host, nothing is provoked on the device ------------------------------
def _rcs(s):
    """(rc, message) of the session calls on the session as it is"""
    L = eulerhip.lib()
    out = []
    buf = np.zeros(1024, np.uint64)
    rc = L.ec_kmer_spectrum(s._h, 1024, buf.ctypes.data)
    out.append((rc, L.ec_last_error().decode()))
    ri = eulerhip.RefilterInfo()
    rc = L.ec_refilter(s._h, 3, ctypes.byref(ri))
    out.append((rc, L.ec_last_error().decode()))
    try:
        s.auto_limit(21)
        out.append((eulerhip.EC_OK, ""))
    except eulerhip.EulerHipError as e:
        out.append((e.code, str(e)))
    return out


def _refused(s, word):
    for rc, msg in _rcs(s):
        assert rc == eulerhip.EC_ERR_STATE and word in msg


def _usable(s):
    """the session still assembles, reports the spectrum and re-filters"""
    case, want = ROWS[15]
    s.run_host(*reads_of(case), 15, 1, WD)
    assert_spectra(s, oracle_of(case, 1)["d"], want[6], (256,))
    res, info = s.refilter(15, want[5], want_dict=True)
    assert_oracle(res, oracle_of(case, want[5]))


def test_refused_arguments(sess):
    case, want = ROWS[15]
    k = 15
    sess.run_host(*reads_of(case), k, 1, WD)
    before = snapshot(sess.fetch(k, True))
    L = eulerhip.lib()
    ri = eulerhip.RefilterInfo()
    buf = np.zeros(4097, np.uint64)
    for rc in (L.ec_refilter(sess._h, 3, None), L.ec_kmer_spectrum(sess._h, 256, None),
               L.ec_kmer_spectrum(sess._h, 1, buf.ctypes.data), L.ec_kmer_spectrum(sess._h, 4097, buf.ctypes.data),
               L.ec_kmer_spectrum(None, 256, buf.ctypes.data), L.ec_refilter(None, 3, ctypes.byref(ri))):
        assert rc == eulerhip.EC_ERR_ARG and L.ec_last_error()
        assert snapshot(sess.fetch(k, True)) == before
    assert not buf.any()
    res, info = sess.refilter(k, want[5], want_dict=True)
    assert_oracle(res, oracle_of(case, want[5]))


def test_refused_on_a_new_session():
    with eulerhip.Session(0) as s:
        _refused(s, "new session")
        _usable(s)


def test_refused_after_trim(sess):
    case, _ = ROWS[15]
    sess.run_host(*reads_of(case), 15, 1, 0)
    before = snapshot(sess.fetch(15))
    sess.trim(0)
    _refused(sess, "trim")
    assert snapshot(sess.fetch(15)) == before  # (results copied to host memory survive the trim)
    _usable(sess)


def test_refused_after_a_failed_call(sess):
    case, _ = ROWS[15]
    sess.run_host(*reads_of(case), 15, 1, 0)
    with pytest.raises(eulerhip.EulerHipError):
        sess.run_host(*reads_of(case), 64, 1, 0)  # (k > EC_MAX_K: refused on the host)
    _refused(sess, "failed")
    _usable(sess)


def test_refused_on_extended_alphabet_results(sess):
    case = golden_cases("extended.json", alphabet="all")[0]
    res = sess.assemble(case["reads"], case["k"], case["limit"])
    _refused(sess, "extended alphabet")
    assert sess.fetch(case["k"]).contigs == res.contigs == case["contigs"]
    _usable(sess)


@pytest.mark.parametrize("upto", ["collect_runs", "count_shard", "graph_finish", "graph_load", "graph_place",
                                  "merge_owned"])
def test_refused_after_stepwise_calls(upto):
    import distributed
    from test_step_state_gpu import Flow
    from test_tips_gpu import STEPWISE

    k = 23
    buf, off = KG.reads_of(k, 63)
    e = distributed.HipEngine(0)
    try:
        e.sess.run_host(buf, off, k, 1, 0)  # (an assembly first: the stepwise calls replace it)
        f = Flow(e, buf, off, k).run(STEPWISE[upto] or Flow.RUNS)
        fetchable = upto in ("graph_finish", "collect_runs")
        before = snapshot(f.result()) if fetchable else None
        _refused(e.sess, "stepwise")
        if fetchable:
            assert snapshot(f.result()) == before
        _usable(e.sess)
    finally:
        e.sess.close()


# ---- 5. other entry points ------------------------------------------------------------------------------
def test_assembler_entry_points(sess):
    case, want = SMALL
    k = 21
    reads = as_list(*reads_of(case))
    ref = oracle_of(case, want[5])
    d, G, r = assembler.assemble(reads, k, 1, session=sess, auto_limit=True)
    assert [[x, c] for x, c in d.items()] == ref["d"]
    assert r == oracle.unpack_contigs(ref)
    assert G == {i: ([tuple(x) for x in a], [tuple(x) for x in b]) for i, (a, b) in enumerate(oracle.unpack_links(ref))}
    h = assembler.kmer_spectrum(reads, k, session=sess)
    assert h.dtype == np.uint64 and h.tolist() == spectrum_model.spectrum(oracle_of(case, 1)["d"], 1024)
    h = assembler.kmer_spectrum(reads, k, limit=3, nbins=64, session=sess)
    assert h.tolist() == spectrum_model.spectrum(oracle_of(case, 3)["d"], 64)
    # with the clean-ups: the limit first, then the tips, then the bubbles
    m1, m2 = _clean_models(case, want[5])
    d, G, r = assembler.assemble(reads, k, 1, session=sess, auto_limit=True, clip_tips=True, pop_bubbles=True)
    assert [[x, c] for x, c in d.items()] == m2[0] and r == m2[1]
    # off by default
    d, G, r = assembler.assemble(reads, k, 1, session=sess)
    assert [[x, c] for x, c in d.items()] == oracle_of(case, 1)["d"]


def _fa(path, reads):
    with open(path, "w") as f:
        f.write("".join(">r%d\n%s\n" % (i, x) for i, x in enumerate(reads)))


def test_cli_auto_limit(tmp_path):
    case, want = ROWS[21]
    k = 21
    _fa(tmp_path / "r.fa", as_list(*reads_of(case)))
    ref = oracle_of(case, want[5])
    r = subprocess.run([sys.executable, RUN, "-i", "r.fa", "-k", str(k), "--auto-limit", "--spectrum-bins", "256",
                        "--spectrum-out", "spec.tsv", "-o", "c.fa"], cwd=str(tmp_path), capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert (tmp_path / "c.fa").read_text() == "".join(
        ">contig%d\n%s\n" % (i, c) for i, c in enumerate(oracle.unpack_contigs(ref)))
    h = spectrum_model.spectrum(oracle_of(case, 1)["d"], 256)
    assert (tmp_path / "spec.tsv").read_text() == "".join("%d\t%d\n" % (c, v) for c, v in enumerate(h) if v)
    assert "auto-limit: limit %d  (spectrum lo %d  descent end %d  peak %d  floor %d)  solid k-mers %d -> %d" % (
        want[5], want[1], want[2], want[3], want[4], want[6], want[7]) in r.stderr
    # no threshold: the outputs are the plain assembly's, and the line says so
    case, want = LOWCOV
    _fa(tmp_path / "low.fa", as_list(*reads_of(case)))
    r = subprocess.run([sys.executable, RUN, "-i", "low.fa", "-k", str(case[5]), "--auto-limit", "-o", "c2.fa"],
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "auto-limit: no limit found" in r.stderr
    assert (tmp_path / "c2.fa").read_text() == "".join(
        ">contig%d\n%s\n" % (i, c) for i, c in enumerate(oracle.unpack_contigs(oracle_of(case, 1))))


def test_cli_refuses_sharded(tmp_path):
    fa = os.path.join(GOLDEN, "g200reads.fa")
    r = subprocess.run([sys.executable, RUN, "-i", fa, "-k", "9", "--auto-limit", "--sharded", "-o", "c.fa"],
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    assert "--auto-limit works on the one-process fused path only" in r.stderr
    assert not (tmp_path / "c.fa").exists()
    r = subprocess.run([sys.executable, RUN, "-i", fa, "-k", "9", "--auto-limit", "--spectrum-bins", "4097"],
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--spectrum-bins" in r.stderr
