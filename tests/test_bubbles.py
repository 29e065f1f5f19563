"""Bubble popping without a GPU: the CPU statement of the contract (bubbles_model.py) on the
hand-built case and on hand-written (G, r, S), and the C ABI's argument checks and bindings of
ec_pop_bubbles / ec_copy_contig_kmer_sums."""
import ctypes
import os

import pytest

import bubbles_model
from conftest import PKG
from model_parallel import model_assemble, twin
from synth import make_genome

LIB = os.path.join(PKG, "libeulerhip.so")


def _info(rounds, converged, nc, nk):
    return {"rounds": rounds, "converged": converged, "n_bubble_contigs": nc, "n_bubble_kmers": nk}


@pytest.mark.parametrize("k", [15, 33])
def test_model_hand_case(k):
    """a SNP bubble nested inside a longer bubble: the default length pops the SNP branch only,
    4 k pops the SNP branch, then the long branch, and leaves the genome in one contig"""
    reads = bubbles_model.hand_reads(k)
    g = make_genome(400, 7).decode()
    d0, c0, _ = model_assemble(reads, k, 1)
    assert len(c0) == 7
    long_w = 2 * (k - 5) + k  # windows of the long branch: 35 / 89
    assert long_w == {15: 35, 33: 89}[k]
    for mr in (2, 8):
        d, c, _, info, hist = bubbles_model.pop_reads(reads, k, 1, 0, mr)
        assert info == _info(1, 1, 1, k) and hist == [(7, 1, k)]
        assert len(d) == len(d0) - 2 * k
    for mr in (3, 8):
        d, c, l, info, hist = bubbles_model.pop_reads(reads, k, 1, 4 * k, mr)
        assert info == _info(2, 1, 2, k + long_w)
        assert hist == [(7, 1, k), (4, 1, long_w)]
        assert c in ([g], [twin(g)]) and len(c[0]) == 400 and l == [[[], []]]
    _, c, _, info, _ = bubbles_model.pop_reads(reads, k, 1, 4 * k, 1)
    assert info == _info(1, 0, 1, k) and len(c) == 4
    # the sums: every canonical solid k-mer is a window of exactly one contig, so they add up to
    # the dict's counts, each strand pair once; the SNP branch is read 3 times, the long one twice
    S = bubbles_model.ksums(c0, d0, k)
    assert 2 * sum(S) == sum(v * (2 if x == twin(x) else 1) for x, v in d0)
    assert sorted(s // (len(c) - k + 1) for s, c in zip(S, c0) if len(c) == 2 * k - 1) == [3, 4]
    assert [s for s, c in zip(S, c0) if len(c) == long_w + k - 1] == [2 * long_w]


# hand-written (G, r, S): contig 0 = left flank, 1 = right flank, 2.. = branches from 0's tail
# (port (0, 0): a link (0, '-')) to 1's head (port (1, 1): a link (1, '+'))
def _bubble(n, blen=9):
    contigs = ["A" * 40, "C" * 40] + ["G" * blen] * n
    links = [[[[2 + b, "+"] for b in range(n)], []], [[], [[2 + b, "-"] for b in range(n)]]]
    links += [[[[1, "+"]], [[0, "-"]]] for _ in range(n)]
    return contigs, links


def test_model_rule_details():
    k = 5
    contigs, links = _bubble(2)
    pop = lambda S, **kw: bubbles_model.popped_of(contigs, links, None, k, sums=S, **kw)  # noqa: E731
    # equal coverage keeps the smaller index; the higher mean wins whatever the index
    assert pop([0, 0, 10, 10]) == [3]
    assert pop([0, 0, 10, 11]) == [2]
    # the comparison is exact: W = 5 and 2^53 + 1 against 2^53 are equal as doubles
    big = 1 << 53
    assert float(big + 1) / 5 == float(big) / 5
    assert pop([0, 0, big, big + 1]) == [2] and pop([0, 0, big + 1, big]) == [3]
    # ... and so with different window counts: S / W = (2^53 + 1) / 3 against 2^54 / 6
    contigs[3] = "G" * 10  # W: 5 and 6
    assert float(5 * big + 1) / 5 == float(6 * big) / 6
    assert pop([0, 0, 5 * big + 1, 6 * big]) == [3] and pop([0, 0, 5 * big, 6 * big + 1]) == [2]
    # max_bubble_len bounds the branches: 10 characters is no branch at 9, so 2 has no partner
    assert pop([0, 0, 1, 100], max_bubble_len=9) == []
    assert pop([0, 0, 1, 100], max_bubble_len=10) == [2]
    # three parallel branches keep one
    contigs, links = _bubble(3)
    assert bubbles_model.popped_of(contigs, links, None, k, sums=[0, 0, 7, 9, 9]) == [2, 4]
    assert bubbles_model.popped_of(contigs, links, None, k, sums=[0, 0, 7, 7, 7]) == [3, 4]
    # a contig with two links on one side is no branch
    contigs, links = _bubble(2)
    links[3][0].append([0, "+"])
    assert bubbles_model.popped_of(contigs, links, None, k, sums=[0, 0, 1, 100]) == []
    # P0 == P1 is no branch (a hairpin: both sides reach the same port)
    contigs, links = _bubble(2)
    links[2] = [[[1, "+"]], [[1, "+"]]]
    links[3] = [[[1, "+"]], [[1, "+"]]]
    assert bubbles_model.popped_of(contigs, links, None, k, sums=[0, 0, 1, 100]) == []
    # a port on the contig itself is no branch
    contigs, links = _bubble(2)
    links[2] = [[[1, "+"]], [[2, "-"]]]
    assert bubbles_model.ports_of(contigs, links, k)[2] is None
    # a partner in the opposite orientation is found: 3 runs from 1's head back to 0's tail
    contigs, links = _bubble(2)
    links[3] = [[[0, "-"]], [[1, "+"]]]
    assert bubbles_model.ports_of(contigs, links, k)[2] == bubbles_model.ports_of(contigs, links, k)[3] == (0, 3)
    assert bubbles_model.popped_of(contigs, links, None, k, sums=[0, 0, 1, 100]) == [2]


@pytest.mark.skipif(not os.path.exists(LIB), reason="libeulerhip.so not built")
def test_symbols_exported_and_bound():
    import eulerhip

    L = ctypes.CDLL(LIB)
    for name in ("ec_pop_bubbles", "ec_copy_contig_kmer_sums"):
        assert hasattr(L, name)
        assert name in eulerhip._SIGS
    assert ctypes.sizeof(eulerhip.PopInfo) == 24
    assert eulerhip.lib().ec_version() >= 300


@pytest.mark.skipif(not os.path.exists(LIB), reason="libeulerhip.so not built")
def test_null_and_range_are_argument_errors():
    import eulerhip

    L = eulerhip.lib()
    pi = eulerhip.PopInfo()
    buf = (ctypes.c_uint64 * 4)()
    assert L.ec_pop_bubbles(None, 0, 4, ctypes.byref(pi)) == eulerhip.EC_ERR_ARG
    assert L.ec_last_error()
    assert L.ec_copy_contig_kmer_sums(None, buf) == eulerhip.EC_ERR_ARG
    assert L.ec_last_error()
    assert L.ec_pop_bubbles(None, 65536, 4, ctypes.byref(pi)) == eulerhip.EC_ERR_ARG
    assert b"65535" in L.ec_last_error()
