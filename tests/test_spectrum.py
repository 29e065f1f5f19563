"""The coverage-aware solid threshold without a GPU: the CPU statement of the rule
(spectrum_model.py) against the host-only ec_spectrum_threshold on random and crafted spectra, the
argument checks and bindings of ec_kmer_spectrum / ec_spectrum_threshold / ec_refilter, and the
fixed read sets below, whose spectrum, threshold and kept k-mers the model's dict and the oracle's
dict must both reproduce.

Fixed cases: synth.make_reads(G, n, L, seed, err=e), limit 1, nbins 256, odd k (no palindromes):

  G, n, L, seed, err, k          found  lo  d   p  floor  limit  n_solid -> kept
  3000, 1800, 100, 5, 0.01, 21     1     2  4  36    0      4     4565 -> 2967
  3000, 1200, 100, 6, 0.005, 23    1     2  3  28    1      3     3291 -> 2954
  2000, 600, 80, 7, 0.01, 15       1     2  4  16    5      3     2106 -> 1931  (same with nbins 32)
  3000, 2400, 100, 8, 0.02, 31     1     2  7  32    2      5     8236 -> 2943
  3000, 2400, 100, 8, 0.02, 33     1     2  6  29    2      5     7922 -> 2940
  3000, 300, 100, 9, 0.01, 21      0     2  2   -    -      -     2895            (d == lo)

The first case with nbins 32 gives found = 0: its peak is in the saturating bin.  What is kept is
the genome (G - k + 1 k-mers) to within its low-coverage ends.
"""
import ctypes
import os

import numpy as np
import pytest

import spectrum_model
from conftest import PKG
from model_parallel import model_count
from spectrum_model import FIXED, info_of
from synth import make_reads

LIB = os.path.join(PKG, "libeulerhip.so")
needs_lib = pytest.mark.skipif(not os.path.exists(LIB), reason="libeulerhip.so not built")
FIXED_IDS = ["-".join(str(x) for x in c) for c, _ in FIXED]

def reads_list(G, n, L, seed, err):
    buf, off = make_reads(G, n, L, seed, err=err)
    s = buf.tobytes().decode()
    return [s[int(off[i]):int(off[i + 1])] for i in range(n)]


# ---- the model on hand-made spectra ---------------------------------------------------------------
CRAFTED = [
    ("all zero", [0] * 8, info_of(0, 0, 0, 0, 0, 0)),
    ("single bin", [0, 0, 5, 0, 0, 0], info_of(0, 2, 0, 0, 0, 0)),
    ("monotone falling", [0, 9, 7, 7, 3, 1, 0, 0], info_of(0, 1, 0, 0, 0, 0)),
    ("rising from lo", [0, 0, 3, 5, 9, 4, 1, 0], info_of(0, 2, 2, 0, 0, 0)),
    ("peak in the last bin", [0, 0, 50, 10, 2, 8, 30, 90], info_of(0, 2, 4, 7, 0, 0)),
    # the plateau 100, 100: the peak is its first bin; 16 (6 - 2) <= 98 picks bin 3
    ("plateau tie at the peak", [0, 0, 500, 6, 2, 40, 100, 100, 30, 0], info_of(1, 2, 4, 6, 2, 3)),
    # the floor 2 twice: v is the first of the two
    ("floor tie", [0, 400, 90, 2, 2, 50, 160, 70, 0], info_of(1, 1, 4, 6, 2, 3)),
    # the rule's last refusal, v == p, needs a spectrum no bin of which qualifies before the peak.
    # There is none: m <= h[d] < h[d + 1] <= h[p], so the floor's own bin lies before p and
    # qualifies with 16 * 0 <= h[p] - m.  The nearest case: only the floor's bin qualifies
    ("v == p cannot be reached", [0, 0, 90, 80, 100, 20, 0, 0], info_of(1, 2, 3, 4, 80, 3)),
    # 16 (h - m) <= h[p] - m exactly at equality: 16 * (7 - 1) = 96 = 97 - 1
    ("equality counts", [0, 900, 7, 1, 30, 97, 12, 0], info_of(1, 1, 3, 5, 1, 2)),
    ("one short of equality", [0, 900, 7, 1, 30, 96, 12, 0], info_of(1, 1, 3, 5, 1, 3)),
    ("two bins", [4, 9], info_of(0, 0, 0, 0, 0, 0)),
    ("descent ends in the last pair", [0, 9, 5, 2, 7], info_of(0, 1, 3, 4, 0, 0)),
]


@pytest.mark.parametrize("name,h,want", CRAFTED, ids=[c[0] for c in CRAFTED])
def test_model_crafted(name, h, want):
    assert spectrum_model.threshold(h) == want


def test_model_spectrum_counts_canonical_once():
    d = [["AAC", 3], ["GTT", 3], ["ACG", 9], ["CGT", 9], ["AAT", 4], ["ATT", 4], ["TTA", 7], ["TAA", 7]]
    assert spectrum_model.spectrum(d, 8) == [0, 0, 0, 1, 1, 0, 0, 2]
    assert spectrum_model.spectrum(d, 4) == [0, 0, 0, 4]
    assert spectrum_model.spectrum(dict((x, c) for x, c in d), 8) == [0, 0, 0, 1, 1, 0, 0, 2]
    # a palindrome is its own twin: one entry, counted once with its doubled count
    assert spectrum_model.spectrum([["ACGT", 6], ["AATT", 2]], 8) == [0, 0, 1, 0, 0, 0, 1, 0]
    assert spectrum_model.filter_dict(d, 4) == [["ACG", 9], ["CGT", 9], ["TTA", 7], ["TAA", 7]]


# ---- the model against ec_spectrum_threshold --------------------------------------------------------
def random_spectra():
    """a few hundred seeded spectra: nbins 2 .. 4096, sparse and dense, zero runs, ties, and shapes
    like a real one (an error slope, a valley, a coverage peak)"""
    rng = np.random.Generator(np.random.PCG64(20261020))
    out = []
    sizes = [2, 3, 4, 5, 7, 8, 16, 31, 32, 33, 64, 100, 255, 256, 1000, 1024, 4095, 4096]
    for i in range(360):
        n = int(sizes[i % len(sizes)]) if i % 3 else int(rng.integers(2, 4097))
        kind = i % 6
        if kind == 0:  # dense, small values: many ties
            h = rng.integers(0, 4, n)
        elif kind == 1:  # dense, large values
            h = rng.integers(0, 1 << 40, n)
        elif kind == 2:  # sparse
            h = np.where(rng.random(n) < 0.1, rng.integers(1, 1000, n), 0)
        elif kind == 3:  # zero runs at both ends and inside
            h = rng.integers(0, 50, n)
            a, b = sorted(int(x) for x in rng.integers(0, n + 1, 2))
            h[:a // 2] = 0
            h[a:b] = 0
        else:  # slope + valley + peak, with noise
            c = np.arange(n, dtype=np.float64)
            peak = rng.uniform(2, max(3.0, 0.8 * n))
            width = rng.uniform(1, max(1.5, peak / 3))
            h = 1e6 * np.exp(-c * rng.uniform(0.3, 2.0)) + rng.uniform(1e2, 1e5) * np.exp(-((c - peak) / width) ** 2)
            h = (h * rng.uniform(0.7, 1.3, n)).astype(np.int64)
            h[:int(rng.integers(0, 3))] = 0
        out.append(np.asarray(h, dtype=np.uint64))
    return out


@needs_lib
def test_threshold_equals_model_on_random_spectra():
    import eulerhip

    found = 0
    for h in random_spectra():
        want = spectrum_model.threshold(h.tolist())
        assert eulerhip.spectrum_threshold(h) == want, h.tolist()[:64]
        found += want["found"]
        # a peak inside the histogram always yields a limit below it (CRAFTED: v == p is unreachable)
        assert want["found"] == (1 if 0 < want["peak"] < len(h) - 1 else 0)
        assert not want["found"] or want["lo"] <= want["limit"] < want["peak"]
    assert found >= 40  # (a condition on the inputs: the rule's last steps are exercised)


@needs_lib
@pytest.mark.parametrize("name,h,want", CRAFTED, ids=[c[0] for c in CRAFTED])
def test_threshold_equals_model_on_crafted_spectra(name, h, want):
    import eulerhip

    assert eulerhip.spectrum_threshold(h) == want
    # the same spectrum in a wider histogram: zeros behind it change nothing but a last-bin peak
    if want["peak"] != len(h) - 1 and (want["descent_end"] or not any(h)):
        assert eulerhip.spectrum_threshold(list(h) + [0] * 5) == want


@needs_lib
def test_threshold_has_no_overflow():
    import eulerhip

    big = (1 << 64) - 1
    h = [0, big, 1 << 60, 0, 1 << 60, big - 1, 5, 0]  # (16 * 2^60 wraps to 0 in 64 bits)
    want = spectrum_model.threshold(h)
    assert want == info_of(1, 1, 3, 5, 0, 3)
    assert eulerhip.spectrum_threshold(np.array(h, dtype=np.uint64)) == want


# ---- bindings and argument checks ---------------------------------------------------------------------
@needs_lib
def test_symbols_exported_and_bound():
    import eulerhip

    L = ctypes.CDLL(LIB)
    for name in ("ec_kmer_spectrum", "ec_spectrum_threshold", "ec_refilter"):
        assert hasattr(L, name)
        assert name in eulerhip._SIGS
    assert ctypes.sizeof(eulerhip.SpectrumInfo) == 32
    assert ctypes.sizeof(eulerhip.RefilterInfo) == 16
    assert eulerhip.SpectrumInfo.floor.offset == 24
    assert eulerhip.EC_SPECTRUM_MAX_BINS == 4096 and eulerhip.EC_SPECTRUM_FLOOR_DIV == spectrum_model.FLOOR_DIV
    assert eulerhip.lib().ec_version() >= 400
    assert set(eulerhip.SpectrumInfo().as_dict()) == {"found", "lo", "descent_end", "peak", "limit", "floor"}
    assert eulerhip.RefilterInfo().as_dict() == {"limit": 0, "changed": 0, "n_removed_kmers": 0}


@needs_lib
def test_null_and_range_are_argument_errors():
    import eulerhip

    L = eulerhip.lib()
    si = eulerhip.SpectrumInfo()
    ri = eulerhip.RefilterInfo()
    buf = (ctypes.c_uint64 * 4097)()
    ARG = eulerhip.EC_ERR_ARG
    assert L.ec_kmer_spectrum(None, 1024, buf) == ARG and b"null" in L.ec_last_error()
    for nbins in (0, 1, 4097):
        assert L.ec_kmer_spectrum(None, nbins, buf) == ARG and b"nbins" in L.ec_last_error()
        assert L.ec_spectrum_threshold(buf, nbins, ctypes.byref(si)) == ARG and b"nbins" in L.ec_last_error()
    assert L.ec_spectrum_threshold(None, 8, ctypes.byref(si)) == ARG and b"null" in L.ec_last_error()
    assert L.ec_spectrum_threshold(buf, 8, None) == ARG and b"null" in L.ec_last_error()
    assert L.ec_refilter(None, 3, ctypes.byref(ri)) == ARG and b"null" in L.ec_last_error()
    assert L.ec_spectrum_threshold(buf, 2, ctypes.byref(si)) == eulerhip.EC_OK
    assert L.ec_spectrum_threshold(buf, 4096, ctypes.byref(si)) == eulerhip.EC_OK and si.found == 0
    with pytest.raises(eulerhip.EulerHipError):
        eulerhip.spectrum_threshold([1])
    with pytest.raises(ValueError):
        eulerhip.spectrum_threshold([[1, 2], [3, 4]])


# ---- the fixed read sets ----------------------------------------------------------------------------------
def _check_row(h, want, G, k):
    found, lo, d, p, floor, limit, n_solid, kept = want
    assert sum(h) == n_solid
    info = spectrum_model.threshold(h)
    assert info == info_of(found, lo, d, p, floor, limit)
    if found:
        assert sum(h[limit + 1:]) == kept
        assert kept <= G - k + 1
    return info


@pytest.mark.parametrize("case,want", FIXED, ids=FIXED_IDS)
def test_fixed_cases_from_the_models_dict(case, want):
    G, n, L, seed, err, k = case
    cnt, _ = model_count(reads_list(G, n, L, seed, err), k)
    d = [[c, v] for c, v in cnt.items() if v > 1]  # (odd k: every canonical k-mer has a distinct twin)
    h = spectrum_model.spectrum(d, 256)
    _check_row(h, want, G, k)
    if want[0]:
        assert len(spectrum_model.filter_dict(d, want[5])) == want[7]
    if case == FIXED[2][0]:
        assert spectrum_model.threshold(spectrum_model.spectrum(d, 32)) == info_of(*want[:6])
    if case == FIXED[0][0]:
        assert spectrum_model.threshold(spectrum_model.spectrum(d, 32)) == info_of(0, 2, 4, 31, 0, 0)


@pytest.mark.parametrize("case,want", FIXED, ids=FIXED_IDS)
def test_fixed_cases_from_the_oracles_dict(case, want):
    import oracle

    G, n, L, seed, err, k = case
    buf, off = make_reads(G, n, L, seed, err=err)
    d = oracle.assemble_packed(buf, off, k, 1, want_dict=True)["d"]
    assert len(d) == 2 * want[6]
    h = spectrum_model.spectrum(d, 256)
    info = _check_row(h, want, G, k)
    if os.path.exists(LIB):
        import eulerhip

        assert eulerhip.spectrum_threshold(h) == info
    if want[0]:
        # build(limit = v) is the dict filtered in order, and keeps the row's k-mers
        dv = oracle.assemble_packed(buf, off, k, want[5], want_dict=True)["d"]
        assert dv == spectrum_model.filter_dict(d, want[5])
        assert len(dv) == 2 * want[7]
