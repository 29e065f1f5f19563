"""Tip clipping without a GPU: the CPU statement of the contract (tips_model.py) on the
hand-built case, and the C ABI's argument check and binding of ec_clip_tips."""
import ctypes
import os

import pytest

import tips_model
from conftest import PKG
from model_parallel import model_assemble

LIB = os.path.join(PKG, "libeulerhip.so")


@pytest.mark.parametrize("k", [15, 33])
def test_model_hand_case(k):
    """a branch that forks into a longer and a shorter tip, two equal tips at the genome's end, an
    isolated short contig: two clipping rounds, then nothing left to clip"""
    reads = tips_model.hand_reads(k)
    assert len(model_assemble(reads, k, 1)[1]) == 8
    _, c, _, info, hist = tips_model.clip_reads(reads, k, 1, 0, 1)
    assert info == {"rounds": 1, "converged": 0, "n_tip_contigs": 2, "n_tip_kmers": 6}
    assert hist == [(8, 2, 6)] and len(c) == 4
    _, c, _, info, hist = tips_model.clip_reads(reads, k, 1, 0, 2)
    assert info == {"rounds": 2, "converged": 0, "n_tip_contigs": 3, "n_tip_kmers": 18}
    assert [len(x) for x in c] == [403, k + 4]
    d8, c8, l8, info, hist = tips_model.clip_reads(reads, k, 1, 0, 8)
    assert info == {"rounds": 2, "converged": 1, "n_tip_contigs": 3, "n_tip_kmers": 18}
    assert hist == [(8, 2, 6), (4, 1, 12)] and c8 == c
    # the isolated contig and the genome have no link left; the dict lost the 18 k-mers and twins
    assert l8 == [[[], []], [[], []]]
    assert len(d8) == len(model_assemble(reads, k, 1)[0]) - 2 * 18


def test_model_rule_details():
    """the rule on hand-written (G, r): equal tips keep the later one, a stem that forks is no
    tip, isolated and two-sided contigs are never candidates, max_tip_len bounds the candidates"""
    k = 5
    # contig 0: long, its tail forks into 1 and 2 (equal lengths) -- 1 < 2: 2 is clipped
    contigs = ["A" * 40, "C" * 8, "G" * 8, "T" * 6]
    links = [[[[1, "+"], [2, "+"]], []], [[], [[0, "-"]]], [[], [[0, "-"]]], [[], []]]
    assert tips_model.clipped_of(contigs, links, k) == [2]
    # a longer sibling clips the shorter; beyond max_tip_len nothing is a candidate
    contigs[1] = "C" * 9
    assert tips_model.clipped_of(contigs, links, k) == [2]
    assert tips_model.clipped_of(contigs, links, k, max_tip_len=7) == []
    assert tips_model.clipped_of(contigs, links, k, max_tip_len=8) == [2]
    # the stem 0 short as well: it is linked on one side only, its siblings at the fork are none
    # (1 and 2 see each other and the stem's other side is empty), so only the fork's loser goes
    contigs[0] = "A" * 7
    assert tips_model.clipped_of(contigs, links, k) == [2]


@pytest.mark.skipif(not os.path.exists(LIB), reason="libeulerhip.so not built")
def test_symbol_exported_and_bound():
    import eulerhip

    assert hasattr(ctypes.CDLL(LIB), "ec_clip_tips")
    assert "ec_clip_tips" in eulerhip._SIGS
    assert ctypes.sizeof(eulerhip.ClipInfo) == 24
    assert eulerhip.lib().ec_version() >= 200


@pytest.mark.skipif(not os.path.exists(LIB), reason="libeulerhip.so not built")
def test_null_session_is_an_argument_error():
    import eulerhip

    L = eulerhip.lib()
    ci = eulerhip.ClipInfo()
    assert L.ec_clip_tips(None, 0, 4, ctypes.byref(ci)) == eulerhip.EC_ERR_ARG
    assert L.ec_last_error()
