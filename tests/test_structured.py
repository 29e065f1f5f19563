"""The structured read sets (tests/structured.py) have the properties they exist for, judged on
the reference's output alone (the C oracle), so that a later change of seed or generator cannot
make the GPU parity tests of test_structured_gpu.py vacuous; and the oracle's two restatements
of the reference (2-bit keys, refasm.c; string keys, refasm_str.c) agree on these topologies,
which the reference-generated goldens reach only below 600 bp.

Measured at the committed seed (SEED = 1); contigs / self-linked / branched are counted on the
oracle's links (self-linked: a contig that links to itself, i.e. a cycle; branched: more than
one link on a side), top count is the largest dict count:

  family           k   reads   n_dict  contigs  self-linked  branched
  replicons        22  61 402  306 926     170          168         0   (168 circular replicons)
  replicons        24  61 460  307 208     170          168         0
  replicons        31  61 652  308 098     170          168         0
  replicons        32  61 678  308 240     170          168         0
  replicons        33  61 706  308 362     170          168         0
  replicons        51  62 192  310 730     170          168         0
  replicons        63  62 514  312 306     170          168         0
  repeat_families  24  28 943  130 766     434            0       252
  repeat_families  31  29 926  137 002     401            0       217
  repeat_families  32  29 983  137 438     400            0       224
  repeat_families  33  30 039  138 020     403            0       215
  repeat_families  51  30 502  142 946     374            0       198
  diploid          24  26 666  106 714   1 346            0       452
  diploid          31  26 666  112 604   1 201            0       423
  diploid          32  26 666  113 390   1 182            0       410
  diploid          33  26 666  114 166   1 167            0       405
  diploid          51  26 666  126 170     853            0       307
  tandem_hairpin   24  24 706  129 370     345            0       118
  tandem_hairpin   31  25 369  128 438     347            9       119
  tandem_hairpin   32  26 900  137 456     347            0       118
  tandem_hairpin   33  26 963  132 714     347            9       119
  tandem_hairpin   51  33 683  153 026     345           11       118

  heavy            k   reads   n_dict  contigs  top count
  shuffled, L=100  21  11 500  39 944        6    120 000
  shuffled, L=100  31  11 500  39 924        6    105 000
  shuffled, L=100  32  11 500  39 922        6    103 500
  shuffled, L=100  51  11 500  39 882        7     75 000
  shuffled, L=100  52  11 500  39 878        7     73 500
  aligned, L=k+289 31   5 280  39 924        6     74 240
  aligned, L=k+289 32   5 280  39 922        6     74 240
  aligned, L=k+289 51   5 280  39 884        6     74 240
"""
import numpy as np
import pytest

import oracle
import structured

SEED = structured.SEED
GRAPH_KS = {"replicons": (22, 24, 31, 32, 33, 51, 63), "repeat_families": (24, 31, 32, 33, 51),
            "diploid": (24, 31, 32, 33, 51), "tandem_hairpin": (24, 31, 32, 33, 51)}
GRAPH_CASES = [(f, k) for f, ks in GRAPH_KS.items() for k in ks]
HEAVY_KS = (21, 31, 32, 51, 52)
HEAVY_ALIGNED_KS = (31, 32, 51)

reads_of, oracle_of = structured.reads_of, structured.oracle_of


def self_linked(links):
    return sum(any(j == i for side in sides for j, _ in side) for i, sides in enumerate(links))


def branched(links):
    return sum(any(len(side) > 1 for side in sides) for sides in links)


def test_one_length_no_n():
    """every family: reads of one length over A/C/G/T only (the default super-k-mer and
    minimizer-run count paths apply), offsets consistent with the buffer"""
    for family, k in [(f, 31) for f in GRAPH_KS] + [("heavy", 31), ("heavy_aligned", 31)]:
        buf, off = reads_of(family, k)
        assert buf.dtype == np.uint8 and off.dtype == np.uint64
        lens = np.diff(off)
        assert len(set(lens.tolist())) == 1 and int(off[-1]) == len(buf), family
        assert set(np.unique(buf).tolist()) <= set(b"ACGT"), family


def test_generators_are_seeded():
    a = structured.repeat_families(31, 5)
    b = structured.repeat_families(31, 5)
    c = structured.repeat_families(31, 6)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert not np.array_equal(a[0][:10_000], c[0][:10_000])


@pytest.mark.parametrize("family,k", GRAPH_CASES)
def test_graph_family_property(family, k):
    links = oracle_of(family, k)["links_unpacked"]
    if family == "replicons":
        ncirc = len(structured.replicon_sizes(k, SEED)[0])
        assert ncirc >= 150
        assert self_linked(links) >= 0.95 * ncirc
    elif family == "repeat_families":
        assert branched(links) >= 100
    elif family == "diploid":
        assert branched(links) >= 150
    else:
        assert branched(links) >= 60


def test_replicon_sizes_sit_on_the_ranking_strides():
    """cycle lengths on and beside RT_STEP_SEG = 512, RT_STEP = 768, RT_TN / 2 = 1024 canonical ids
    and twice that, and small ones down to k + 2"""
    circ, lin = structured.replicon_sizes(31, SEED)
    for n in (511, 512, 513, 767, 768, 769, 1023, 1024, 1025, 2047, 2048, 2049):
        assert n in circ
    assert min(circ) < 60 and lin == [700, 4000]


@pytest.mark.parametrize("k", HEAVY_KS)
def test_heavy_counts_pass_16_bits(k):
    assert max(c for _, c in oracle_of("heavy", k)["d"]) > 65_535


@pytest.mark.parametrize("k", HEAVY_ALIGNED_KS)
def test_heavy_aligned_blocks(k):
    """one 256-read tile holds 256 * 290 windows of one canonical key: the block's reads are
    byte-identical (unit A: half poly-A, half poly-T) and start at a multiple of 256"""
    assert max(c for _, c in oracle_of("heavy_aligned", k)["d"]) > 65_535
    buf, off = reads_of("heavy_aligned", k)
    L = k + 289
    assert 256 * (L - k + 1) > 65_535
    rows = buf.reshape(-1, L)
    for unit, a in zip(structured.HEAVY_UNITS, structured.heavy_blocks()):
        assert a % 256 == 0
        blk = rows[a:a + 256]
        if unit == "A":
            assert (blk[:128] == ord("A")).all() and (blk[128:] == ord("T")).all()
        else:
            assert (blk == blk[0]).all()
            assert bytes(blk[0][:len(unit)]) == unit.encode()


@pytest.mark.parametrize("family,k", [("replicons", 31), ("repeat_families", 33), ("diploid", 24),
                                      ("tandem_hairpin", 51), ("heavy", 32), ("heavy_aligned", 31)])
def test_string_oracle_equals_2bit_oracle(family, k):
    """refasm_str.c (string keys, the reference's own dict order by construction) against
    refasm.c (2-bit keys) on one input per family: dict, contigs and links"""
    buf, off = reads_of(family, k)
    ref = oracle_of(family, k)
    alt = oracle.assemble_packed(buf, off, k, 1, True, string=True)
    assert alt["n_positions"] == ref["n_positions"] and alt["n_dict"] == ref["n_dict"]
    assert alt["d"] == ref["d"]
    assert alt["contig_chars"] == ref["contig_chars"]
    assert np.array_equal(alt["contig_offsets"], ref["contig_offsets"])
    assert np.array_equal(alt["link_offsets"], ref["link_offsets"])
    assert np.array_equal(alt["links"], ref["links"])
