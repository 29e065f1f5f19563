"""k_skpart_w's entry count and store cursor (count_sk2.h): the wave's buffered entries are counted
on the scalar side -- one popcount of the closing lanes' ballot per window -- and an entry's LDS
address is the scalar cursor plus the lane's rank in that ballot.  What such a counter can get
wrong is its carry: across the rounds of a tile, across a flush, past the clamp of a full buffer,
out of a last partial round, and through windows whose ballot is full or empty.

Every case is compared with the oracle (ordered dict, contig bytes and offsets, links); where the
call stays on super-k-mer records its record count is also the numpy partition model's
(test_sk2_full_runs_gpu.model_runs).

Shapes (k, read length) -- every exit of the round loop:
  (31, 100) M = 70: four whole rounds and a last one of 2 windows      (31, 98) M = 68: whole rounds only
  (31, 47)  M = 17: exactly one block     (31, 40) M = 10 < W     (21, 100) W = 7
  (32, 100) W = 18, 8 first-window bits, runs cut at 16
  (31, 158), (31, 159): M = 128 and 129, the two sides of the 17-window entry's limit
Read sets of 4 099 reads (the last tile has idle lanes): a random 20 kbp genome; homopolymers and
period-2 / period-3 reads, where every lane of a wave closes a run in the same window or none does
for whole rounds (full and empty ballots); and the two interleaved, so the lanes of a wave disagree.
EULERHIP_SK2_ELIM: 128 and 192 put the clamp and the overflow flag inside a round (the call is then
redone on window records), 768 flushes in the middle of a tile.

The last test is for the bucket kernels' record loads: so few reads of so small a genome that most
final buckets are empty and the others hold fewer records than a workgroup has threads (a clamped
prefetch index on r1 == r0 and r1 - r0 < 512).
"""
import numpy as np
import pytest

import eulerhip
import oracle
from synth import make_reads
from test_sk2_full_runs_gpu import model_runs, nmax_of, window_minima, _codes

pytestmark = pytest.mark.gpu

N_READS = 4_099
SHAPES = [(31, 100), (31, 98), (31, 47), (31, 40), (21, 100), (32, 100), (31, 158), (31, 159)]
SETS = ["random", "lowcx", "mixed"]
ELIMS = [None, "128", "192", "768"]


def _low_complexity(n, L, seed):
    """homopolymers, period-2 and period-3 reads in turn, the unit and its phase drawn per read"""
    rng = np.random.default_rng(seed)
    out = np.empty((n, L), np.uint8)
    lut = np.frombuffer(b"ACGT", np.uint8)
    for i in range(n):
        period = 1 + i % 3
        while True:
            unit = rng.integers(0, 4, period)
            if period == 1 or len(set(unit.tolist())) > 1:  # (a period-2 / -3 unit of one base is a homopolymer)
                break
        out[i] = lut[np.resize(np.roll(unit, int(rng.integers(0, period))), L)]
    return out


_INPUTS = {}


def _inputs(kind, k, L):
    """(buf, off, oracle result), built once per (set, shape) and shared by the ELIM cases"""
    key = (kind, k, L)
    if key not in _INPUTS:
        seed = 8100 + 7 * k + L
        rnd, off = make_reads(20_000, N_READS, L, seed)  # half of them reverse-complemented
        if kind == "random":
            buf = rnd
        else:
            low = _low_complexity(N_READS, L, seed + 1)
            if kind == "mixed":  # alternate lanes, so every wave holds both kinds
                low[0::2] = rnd.reshape(N_READS, L)[0::2]
            buf = low.reshape(-1)
        _INPUTS[key] = (buf, off, oracle.assemble_packed(buf, off, k, 1, True))
    return _INPUTS[key]


@pytest.mark.parametrize("elim", ELIMS)
@pytest.mark.parametrize("kind", SETS)
@pytest.mark.parametrize("k,L", SHAPES)
def test_entry_cursor_vs_oracle(gpu_session, monkeypatch, k, L, kind, elim):
    if elim is None:
        monkeypatch.delenv("EULERHIP_SK2_ELIM", raising=False)
    else:
        monkeypatch.setenv("EULERHIP_SK2_ELIM", elim)
    buf, off, ref = _inputs(kind, k, L)
    gpu_session.run_host(buf, off, k, 1, eulerhip.EC_FLAG_WANT_DICT)
    res = gpu_session.fetch(k, True)
    on_sk = res.stats.count_variant == 3 and res.stats.record_bytes == 16
    print("k %d L %d %s elim %s: super-k-mer records %s, records %d" % (k, L, kind, elim, on_sk, res.stats.n_records))
    assert res.stats.n_positions == ref["n_positions"] and res.stats.n_dict == ref["n_dict"]
    assert [[x, c] for x, c in res.dict_items] == ref["d"]
    assert res.contig_bytes == ref["contig_chars"] and np.array_equal(res.contig_offsets, ref["contig_offsets"])
    assert res.links == oracle.unpack_links(ref)
    if on_sk:
        assert res.stats.n_records == model_runs(buf, L, k, nmax_of(k, L))[0]


def _min_remix(x):
    """superkmer.h min_remix on a uint32 array"""
    return (x >> np.uint32(14)) | (x << np.uint32(18))


SPARSE = (150, 160, 100, 8999)  # genome, reads, read length, seed


def _bucket_fill(buf, L, k, B):
    """records per final bucket, B = 2^b buckets: one record per run of equal window minimum, cut
    every sk2_nmax windows (model_runs' runs), in the bucket of its minimizer -- the top b bits
    of min_remix"""
    v = window_minima(_codes(buf, L), k)
    n, M = v.shape
    start = np.ones((n, M), bool)
    start[:, 1:] = v[:, 1:] != v[:, :-1]
    j = np.broadcast_to(np.arange(M), (n, M))
    pos = j - np.maximum.accumulate(np.where(start, j, 0), axis=1)
    rec = pos % nmax_of(k, L) == 0
    bucket = _min_remix(v[rec]) >> np.uint32(32 - (B.bit_length() - 1))
    return np.bincount(bucket.astype(np.int64), minlength=B)


def test_sparse_buckets_vs_oracle(gpu_session, monkeypatch):
    """160 reads of a 150-base genome (a call this small has 64 final buckets, and the genome
    ~15 minimizers): most final buckets are empty and no other holds a workgroup's 512 records --
    checked on the partition model with the call's own bucket count"""
    monkeypatch.delenv("EULERHIP_SK2_ELIM", raising=False)
    g, n, L, seed = SPARSE
    k = 31
    buf, off = make_reads(g, n, L, seed)
    ref = oracle.assemble_packed(buf, off, k, 1, True)
    gpu_session.run_host(buf, off, k, 1, eulerhip.EC_FLAG_WANT_DICT)
    res = gpu_session.fetch(k, True)
    assert res.stats.count_variant == 3 and res.stats.record_bytes == 16
    B = int(res.stats.n_buckets)
    assert B >= 2 and B & (B - 1) == 0
    fill = _bucket_fill(buf, L, k, B)
    print("buckets %d: empty %d, fullest %d records" % (B, int((fill == 0).sum()), int(fill.max())))
    assert (fill == 0).sum() > B // 2 and 0 < fill.max() < 512
    assert res.stats.n_records == fill.sum() == model_runs(buf, L, k, nmax_of(k, L))[0]
    assert res.stats.n_positions == ref["n_positions"] and res.stats.n_dict == ref["n_dict"]
    assert [[x, c] for x, c in res.dict_items] == ref["d"]
    assert res.contig_bytes == ref["contig_chars"] and np.array_equal(res.contig_offsets, ref["contig_offsets"])
    assert res.links == oracle.unpack_links(ref)
