"""The kernel grid's tables (tests/kernel_grid.py), judged without a GPU: the dispatch rule they
restate uses the sources' constants, the parametrisation reaches every compiled instantiation of
the count kernels on a case that asserts that kernel's own path, and every cell's reference
result is non-trivial, so that a later change of a table, a seed or a constant cannot make
test_kernel_grid_gpu.py vacuous.

  k_skpart_w<NPF, W, VAL>   3 x 12 (NPF, W) pairs in each VAL form          (count_sk2.h)
  k_wbv<W>                  20 widths, k = 33..52                             (count_wide.h)
  k_partition<NPF, HI, R10> 3 x 2 x 2                                         (count_v2.h)
"""
import os
import re

import numpy as np
import pytest

import kernel_grid as kg

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pycuda-euler_amd", "csrc")


def _constant(header, name):
    with open(os.path.join(CSRC, header)) as f:
        m = re.search(r"constexpr\s+\w+\s+%s\s*=\s*(\d+)\s*;" % name, f.read())
    assert m, "%s not found in %s" % (name, header)
    return int(m.group(1))


def test_constants_are_the_sources():
    assert kg.SK_M == _constant("superkmer.h", "SK_M")
    assert kg.SK_MIN_K == _constant("superkmer.h", "SK_MIN_K")
    assert kg.WMB_MAX_K == _constant("count_wide.h", "WMB_MAX_K")
    assert kg.WMB_MAXL == _constant("count_wide.h", "WMB_MAXL")
    assert kg.STAGE_W == _constant("count_wide.h", "STAGE_W")
    assert kg.STAGE_BYTES == _constant("count_part.h", "STAGE_BYTES")
    assert kg.TILE_READS == _constant("count_part.h", "TILE_READS")


def test_stage_classes():
    """the read lengths at which a 64-read wave tile steps to the next stage size"""
    assert [kg.npf_of(L) for L in (1, 63, 64, 111, 112, 159, 160)] == [4, 4, 7, 7, 10, 10, 0]
    assert {kg.npf_of(L) for L in kg.B_LS} == {4, 7, 10}
    for npf in (4, 7, 10):  # one length inside the class beside its edges
        assert any(kg.npf_of(L) == npf and L not in (63, 64, 111, 112, 159) for L in kg.B_LS)


ALL_SKPART = {(npf, w) for npf in (4, 7, 10) for w in range(7, 19)}


def test_grid_reaches_every_skpart_form():
    """both VAL forms run the same cells (the short variant differs in its first read), and each of
    the 36 (NPF, W) pairs is a cell whose asserted path is the super-k-mer count"""
    forms = {kg.skpart_form(k, L) for k, L in kg.A_CELLS if kg.expected_path(k, L, kg.NREADS)[1] == 3}
    assert forms == ALL_SKPART and len(forms) == 36
    for k, L in kg.A_CELLS:
        assert L >= k and kg.expected_path(k, L, kg.NREADS) == (kg.EC_PATH_PARTITIONED, 3, 16)
        short = kg.short_lengths(k, kg.NREADS)
        assert short[0] < k and len(short) > 3 and all(0 <= ln < k for ln in short.values())
    for k, L in kg.A_LONG:  # no stage: not the super-k-mer count
        assert kg.npf_of(L) == 0 and kg.expected_path(k, L, kg.NREADS) == (kg.EC_PATH_PARTITIONED, 0, 16)


def test_grid_reaches_every_wbv_width():
    widths = {k - kg.SK_M + 1 for k, L in kg.C_CELLS if kg.expected_path(k, L, kg.NREADS)[2] == 16}
    assert widths == set(range(19, 39)) and len(widths) == 20
    # every form the wide dispatch has is asserted somewhere: runs, hash buckets, the HBM table
    assert {kg.expected_path(k, L, kg.NREADS) for k, L in kg.C_CELLS} == {
        (kg.EC_PATH_PARTITIONED, 0, 16), (kg.EC_PATH_PARTITIONED, 0, 24), (kg.EC_PATH_GENERAL, 0, 0)}
    for k in kg.C_KS:
        assert kg.expected_path(k, 160, kg.NREADS)[2] == (16 if k <= 52 else 0)  # k_wbv's L = 160
        assert kg.expected_path(k, 161, kg.NREADS)[0] == kg.EC_PATH_GENERAL
        assert kg.expected_path(k, 159, kg.NREADS)[2] == (16 if k <= 52 else 24)


def test_grid_reaches_every_partition_form():
    """k = 1 and 2 (two and ten canonical keys for 32 coarse buckets) outgrow the window records'
    fixed capacities at every length and are asserted on the exact path; every other case, and
    through them each of the 12 forms, is asserted on k_partition's"""
    forms = set()
    for k, L, no_sk2, r10 in kg.B_CASES:
        path, variant, rbytes = kg.expected_path(k, L, kg.NREADS, no_sk2, r10)
        if k <= 2:
            assert not kg.window_record_capacity_holds(*kg.reads_of(k, L), k)
            assert (path, variant) == (kg.EC_PATH_PARTITIONED, 0), (k, L)
            continue
        npf, hi, r = kg.partition_form(k, L, r10)
        assert (path, variant, rbytes) == (kg.EC_PATH_PARTITIONED, 2 if r else 1, 10 if r else 12), (k, L, no_sk2, r10)
        forms.add((npf, hi, r))
    assert forms == {(npf, hi, r) for npf in (4, 7, 10) for hi in (False, True) for r in (False, True)}
    assert len(forms) == 12
    assert len(set(kg.B_CASES)) == len(kg.B_CASES)


def test_tails_offsets_and_sharded_cells():
    for n in kg.D_NS:
        for k, L in kg.D_CELLS:
            want = {23: 3, 17: 1, 48: 0}[k]
            assert kg.expected_path(k, L, n)[1] == want and kg.expected_path(k, L, n)[0] == kg.EC_PATH_PARTITIONED
    assert any(n % 64 and n % 256 for n in kg.D_NS) and kg.NREADS % 64 and kg.NREADS % 256
    # the misaligned cells: the stage exactly full, so the rounded loads decide whether it fits
    assert [kg.npf_of(L) for _, L in kg.E_CELLS[:2]] == [4, 7] and kg.npf_of(64) == 7 and kg.npf_of(112) == 10
    assert kg.E_CELLS[2][1] == kg.WMB_MAXL
    assert set(kg.F_SWITCH_KS) <= set(kg.F_KS) == set(range(1, 64))


def _nontrivial(ref, k, L):
    """solid k-mers, and a contig longer than k wherever a read has two windows -- unless every one
    of the 4^k k-mers is solid (k <= 5 on a 3 000-base genome): the de Bruijn graph is then
    complete, every node has four successors, and no input has a contig of more than one k-mer"""
    assert ref["n_dict"] > 0, (k, L)
    if L > k:
        off = ref["contig_offsets"]
        longest = int((off[1:] - off[:-1]).max())
        if ref["n_dict"] == 4 ** k:
            assert k <= 5 and longest == k, (k, L)
        else:
            assert longest > k, (k, L)


CELLS = sorted(set(kg.A_CELLS + kg.A_LONG + [(k, L) for k, L, _, _ in kg.B_CASES] + kg.C_CELLS + kg.E_CELLS
                   + [(k, kg.F_L) for k in kg.F_KS]))


def test_every_cell_is_nontrivial():
    """solid k-mers in every cell, and a contig longer than k wherever a read has two windows"""
    for k, L in CELLS:
        _nontrivial(kg.oracle_of(k, L), k, L)
    for k, L in kg.A_CELLS:
        ref = kg.oracle_of(k, L, short=True)
        _nontrivial(ref, k, L)
        # the short reads have no window: the windows are those of the other reads
        assert ref["n_positions"] == (kg.NREADS - len(kg.short_lengths(k, kg.NREADS))) * (L - k + 1)


@pytest.mark.parametrize("n", kg.D_NS)
def test_tail_cells_are_nontrivial(n):
    """limit 0 (every k-mer kept), so that a single read still has a dict and a contig"""
    for k, L in kg.D_CELLS:
        _nontrivial(kg.oracle_of(k, L, n, limit=0), k, L)


@pytest.mark.parametrize("k", kg.TWO_LENGTH_KS)
def test_two_length_input(k):
    """the first read is of the shorter length, later ones are longer, and a 256-read tile still
    fits the staged wide upsweep (so the redone call stays partitioned)"""
    buf, off = kg.two_length_reads(k)
    lens = np.diff(off.astype(np.int64))
    assert lens[0] == min(kg.TWO_LENGTHS) >= k and set(lens) == set(kg.TWO_LENGTHS)
    assert lens[-256:].max() == max(kg.TWO_LENGTHS) <= kg.WMB_MAXL
    assert max(int(off[min(r + 256, len(lens))] - off[r]) for r in range(0, len(lens), 256)) + 30 <= kg.STAGE_W
    _nontrivial(kg.oracle_of_two_lengths(k), k, max(kg.TWO_LENGTHS))
