"""Parity of the HIP paths with the oracle on structured genomes (tests/structured.py): many
cycles in one ranking call, repeat junctions with up to 4 successors, solid bubbles, inverted
repeats, and k-mers seen more than 65 535 times -- at sizes that cross the ranking tiles, the
count buckets and the rank segments (test_structured.py pins the properties of the inputs).

Everything is bit-exact against oracle.assemble_packed(..., want_dict=True): dict items in
order, contig bytes and offsets, links, n_positions and n_dict.
  A  the default path, every family over k
  B  forced stages (ranking variants, link joins, starts, filter buckets, count paths)
  C  the sharded flow (simulated ranks), both finishes and link modes, junction-table knobs,
     the streaming count
  D  heavy keys: counts past 2^16 on every count path, in one prescan group, summed across
     shards and chunks
  E  one session, inputs of very different chain statistics in turn
"""
import ctypes

import numpy as np
import pytest

import eulerhip
from structured import oracle_of, reads_of, reference
from synth import make_genome, make_reads

pytestmark = pytest.mark.gpu

GRAPH = ("replicons", "repeat_families", "diploid", "tandem_hairpin")


def _dict_raw(session, k, nd):
    """the call's dict as ec_copy_dict writes it: nd k-mers in order as one byte string, their
    counts as uint32 (Session.fetch(k, True) turns the same two buffers into a list of pairs)"""
    km = ctypes.create_string_buffer(max(nd * k, 1))
    cnt = np.zeros(max(nd, 1), dtype=np.uint32)
    eulerhip.check(eulerhip.lib().ec_copy_dict(session._h, km, cnt.ctypes.data))
    return km.raw[: nd * k], cnt[:nd]


def _check(session, k, ref):
    """the finished call of `session` against the oracle: positions, dict size, dict items in
    order (k-mers and counts), contig bytes and offsets, links"""
    res = session.fetch(k)
    assert res.stats.n_positions == ref["n_positions"]
    assert res.stats.n_dict == ref["n_dict"]
    kmers, counts = _dict_raw(session, k, res.stats.n_dict)
    assert kmers == ref["d_kmers"]
    assert np.array_equal(counts, ref["d_counts"])
    assert res.contig_bytes == ref["contig_chars"]
    assert np.array_equal(res.contig_offsets, ref["contig_offsets"])
    assert res.links == ref["links_unpacked"]
    res.dict_counts = counts
    return res


def _run(session, family, k, flags=0):
    buf, off = reads_of(family, k)
    session.run_host(buf, off, k, 1, flags | eulerhip.EC_FLAG_WANT_DICT)
    return _check(session, k, oracle_of(family, k))


# ---- A. default path ---------------------------------------------------------------------------
A_CASES = [(f, k) for f in GRAPH for k in (24, 31, 32, 33, 51)] + [("replicons", 22), ("replicons", 63)]


@pytest.mark.parametrize("family,k", A_CASES)
def test_default_path(gpu_session, family, k):
    """bit-exact on the path a caller gets, and for 21 <= k <= 32 that path is the super-k-mer
    count (count_variant 3).

    repeat_families at k = 31 and 32 is the case that needs phase_count_sk2's second refine: a
    final bucket holds whole minimizers and is planned for twice the mean plus 1024 records
    (fcap 4383 at k = 31), a minimizer inside the 300-base family is met by 40 copies x ~35 reads,
    ~1 400 records, and a bucket that draws a few of them outgrows the plan.  The call used to
    leave the super-k-mer path there (count_variant 1, table_retries 1, at every seed tried); it
    now refines once more with the capacity the first refine measured."""
    res = _run(gpu_session, family, k)
    if 21 <= k <= 32:
        assert res.stats.count_variant == 3  # super-k-mer records (count_sk2.h): the headline path
    else:
        assert res.stats.count_path == eulerhip.EC_PATH_PARTITIONED


# ---- B. forced stages --------------------------------------------------------------------------
B_MODES = [  # id, knobs, flags, k (None: 31 and 51)
    ("rank1_async", {"EULERHIP_RANK": "1", "EULERHIP_RANK_SYNC": "0"}, 0, None),
    ("rank1_sync", {"EULERHIP_RANK": "1", "EULERHIP_RANK_SYNC": "1"}, 0, None),
    ("rank2_async", {"EULERHIP_RANK": "2", "EULERHIP_RANK_SYNC": "0"}, 0, None),
    ("rank2_sync", {"EULERHIP_RANK": "2", "EULERHIP_RANK_SYNC": "1"}, 0, None),
    ("join_local", {"EULERHIP_JOIN_LINKS": "1", "EULERHIP_JOIN_LOCAL": "1"}, 0, None),
    ("join_global", {"EULERHIP_JOIN_LINKS": "1", "EULERHIP_JOIN_LOCAL": "0"}, 0, None),
    ("probe_links", {"EULERHIP_JOIN_LINKS": "0"}, 0, None),
    ("radix_starts", {"EULERHIP_NO_SMALL_STARTS": "1"}, 0, None),
    ("force_filter", {"EULERHIP_FORCE_FILTER": "1"}, 0, None),
    ("general", {}, eulerhip.EC_FLAG_GENERAL, None),
    ("window_records", {}, eulerhip.EC_FLAG_WINDOW_RECORDS, None),
    ("exact_count", {}, eulerhip.EC_FLAG_EXACT_COUNT, None),
    ("wide_l3", {"EULERHIP_WIDE_L3": "2"}, 0, 51),
    ("wide_mb0", {"EULERHIP_WIDE_MB": "0"}, 0, 51),
]
B_CASES = [(f, k, m) for f in GRAPH for k in (31, 51) for m in B_MODES if m[3] in (None, k)]


@pytest.mark.parametrize("family,k,mode", B_CASES, ids=["%s-%d-%s" % (f, k, m[0]) for f, k, m in B_CASES])
def test_forced_stage(gpu_session, monkeypatch, family, k, mode):
    name, knobs, flags, _ = mode
    for n, v in knobs.items():
        monkeypatch.setenv(n, v)
    res = _run(gpu_session, family, k, flags)
    if name == "general":
        assert res.stats.count_path == eulerhip.EC_PATH_GENERAL
    if name == "exact_count" and k <= 32:
        assert res.stats.count_variant == 0
    if name == "wide_l3":
        assert res.stats.n_buckets == (1 << 14) << 2


# ---- C. sharded flow ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def engines():
    import distributed

    es = [distributed.HipEngine(0) for _ in range(4)]
    yield es
    for e in es:
        e.sess.close()


def _check_sharded(res, P, ref, what):
    assert P == ref["n_positions"], what
    assert res.stats.n_dict == ref["n_dict"], what
    assert res.contig_bytes == ref["contig_chars"], what
    assert np.array_equal(res.contig_offsets, ref["contig_offsets"]), what
    assert res.links == ref["links_unpacked"], what


C_INPUTS = [(f, k) for f in ("replicons", "repeat_families", "diploid") for k in (31, 51)]


@pytest.mark.parametrize("world", [1, 3, 4])
@pytest.mark.parametrize("family,k", C_INPUTS)
def test_sharded_finishes(engines, family, k, world):
    """the partitioned finish (every rank ranks and emits its own segment: many cycles and
    junction-rich chains across the rank segments) and the replicated one"""
    import distributed

    buf, off = reads_of(family, k)
    for finish in ("partitioned", "replicated"):
        res, P = distributed.local_sharded_assemble(engines[:world], buf, off, k, 1, finish=finish)
        _check_sharded(res, P, oracle_of(family, k), finish)


@pytest.mark.parametrize("world", [1, 3, 4])
@pytest.mark.parametrize("family,k", C_INPUTS)
def test_sharded_links(engines, family, k, world):
    """the links computed per owner segment (partitioned) and on the gathered set"""
    import distributed

    buf, off = reads_of(family, k)
    for partitioned in (True, False):
        res, P = distributed.local_sharded_assemble(engines[:world], buf, off, k, 1, partitioned=partitioned)
        _check_sharded(res, P, oracle_of(family, k), partitioned)


@pytest.mark.parametrize("knobs", [{"EULERHIP_JUNCTION_BT": "2", "EULERHIP_JUNCTION_SB": "3"},
                                   {"EULERHIP_JUNCTION_RADIX": "1"}], ids=["split", "radix"])
@pytest.mark.parametrize("family,k", [(f, k) for f in ("repeat_families", "diploid") for k in (31, 51)])
def test_sharded_junction_tables(engines, monkeypatch, family, k, knobs):
    """the junction join with its buckets split into sub-buckets / ordered by the radix sort, on
    junction-dense inputs (the claim cap is left alone: near it the overflow is timing-dependent)"""
    import distributed

    for n, v in knobs.items():
        monkeypatch.setenv(n, v)
    buf, off = reads_of(family, k)
    res, P = distributed.local_sharded_assemble(engines[:2], buf, off, k, 1, finish="partitioned")
    _check_sharded(res, P, oracle_of(family, k), knobs)


@pytest.mark.parametrize("family", GRAPH)
def test_streaming(engines, family):
    """the reads counted in seven chunks, folded every two"""
    import distributed

    k = 31
    buf, off = reads_of(family, k)
    n = len(off) - 1
    chunk = n // 7 + 1
    stats = {}
    res, P = distributed.streaming_assemble(engines[0], buf, off, k, 1, chunk_reads=chunk, fold=2, stats=stats)
    assert stats["chunks"] == 7 and stats["folds"] == 3
    _check_sharded(res, P, oracle_of(family, k), family)


# ---- D. heavy keys -----------------------------------------------------------------------------
D_MODES = [("default", {}, 0), ("window_records", {}, eulerhip.EC_FLAG_WINDOW_RECORDS),
           ("no_sk2", {"EULERHIP_NO_SK2": "1"}, 0), ("exact_count", {}, eulerhip.EC_FLAG_EXACT_COUNT)]


@pytest.mark.parametrize("mode", D_MODES, ids=[m[0] for m in D_MODES])
@pytest.mark.parametrize("k", [21, 31, 32, 51, 52])
def test_heavy_counts(gpu_session, monkeypatch, k, mode):
    """dict counts of 73 500 .. 120 000 (past 16 bits; even k: palindromic keys, which add 2 per
    window) out of every count path"""
    for n, v in mode[1].items():
        monkeypatch.setenv(n, v)
    res = _run(gpu_session, "heavy", k, mode[2])
    assert int(res.dict_counts.max()) > 65_535


@pytest.mark.parametrize("k", [31, 32, 51])
def test_heavy_one_prescan_group(gpu_session, k):
    """256 identical reads of k + 289 bases in one 256-read tile: 74 240 windows of one canonical
    key in one prescan group wrap a 16-bit histogram bin; the prescan's check (its bin sum against
    the windows it placed) must set `skew`, which sends the call to the general path"""
    res = _run(gpu_session, "heavy_aligned", k)
    print("heavy_aligned k=%d: count_path %d count_variant %d table_retries %d"
          % (k, res.stats.count_path, res.stats.count_variant, res.stats.table_retries))
    assert res.stats.count_path == eulerhip.EC_PATH_GENERAL


def _heavy_limits(k):
    """limit 1; the count of every AAC rotation (500 reads a phase, L - k + 1 windows a read, a
    third of them each rotation: dropped at count > limit, kept if over-counted by one); and one
    below the count of the keys of A, AT and CG (kept; dropped if under-counted by one or held
    in 16 bits)"""
    w = 100 - k + 1
    return (1, 500 * w, 1500 * w - 1)


_HEAVY_REF = {}


def _heavy_ref(k, limit):
    if (k, limit) not in _HEAVY_REF:
        buf, off = reads_of("heavy", k)
        _HEAVY_REF[(k, limit)] = reference(buf, off, k, limit)
    return _HEAVY_REF[(k, limit)]


@pytest.mark.parametrize("k", [31, 51])
def test_heavy_limits_at_the_counts(gpu_session, k):
    """the solid filter count > limit at the heavy keys' own counts, on one GPU: the same limits as
    the sharded and streaming tests below, here with the dict"""
    buf, off = reads_of("heavy", k)
    for limit in _heavy_limits(k):
        ref = _heavy_ref(k, limit)
        assert 0 < ref["n_dict"] and (limit == 1 or ref["n_dict"] < 100)
        gpu_session.run_host(buf, off, k, limit, eulerhip.EC_FLAG_WANT_DICT)
        _check(gpu_session, k, ref)


@pytest.mark.parametrize("compact", [True, False])
@pytest.mark.parametrize("k", [31, 51])
def test_heavy_sharded(engines, k, compact):
    """counts summed across three shards' records (compact and full exchange records), both
    finishes; the results carry no dict, so the sums are checked through the solid filter at
    limits on either side of the heavy keys' counts"""
    import distributed

    buf, off = reads_of("heavy", k)
    n = len(off) - 1
    world = 3
    parts = []
    for r in range(world):
        lo, hi = distributed.shard_range(n, r, world)
        parts.append((buf[int(off[lo]):int(off[hi])], off[lo:hi + 1] - off[lo], lo))
    for limit in _heavy_limits(k):
        for finish in ("partitioned", "replicated"):
            res, P = distributed.local_sharded_assemble_shards(engines[:world], parts, k, limit, finish=finish,
                                                               compact=compact)
            _check_sharded(res, P, _heavy_ref(k, limit), (limit, finish))


@pytest.mark.parametrize("k", [31, 51])
def test_sharded_rank_without_solid_keys(engines, k):
    """reduced from test_heavy_sharded[51] at the limit that keeps three canonical keys on three
    ranks: the only solid key (poly-A, seen 30 * (100 - k + 1) times; every other k-mer once) has
    one owner, the other ranks' segments are empty.  ec_graph_starts_part counted an empty segment's
    starts (none) without holding the count for ec_graph_starts_copy, which then refused the
    call (EC_ERR_STATE) and with it the partitioned finish"""
    import distributed

    L = 100
    rnd = np.frombuffer(make_genome(30 * L, 8820 + k), np.uint8)  # cut into 30 reads: no shared k-mer
    rows = np.concatenate([rnd.reshape(30, L), np.full((30, L), ord("A"), np.uint8)])
    rows = rows[np.random.Generator(np.random.PCG64(8830)).permutation(60)]
    buf, off = rows.reshape(-1).copy(), np.arange(61, dtype=np.uint64) * np.uint64(L)
    ref = reference(buf, off, k, 1)
    assert ref["n_dict"] == 2 and [c for _, c in ref["d"]] == [30 * (L - k + 1)] * 2
    for finish in ("partitioned", "replicated"):
        res, P = distributed.local_sharded_assemble(engines[:3], buf, off, k, 1, finish=finish)
        _check_sharded(res, P, ref, finish)


@pytest.mark.parametrize("k", [31, 51])
def test_heavy_streaming(engines, k):
    """counts summed across seven chunks and three folds"""
    import distributed

    buf, off = reads_of("heavy", k)
    chunk = (len(off) - 1) // 7 + 1
    for limit in _heavy_limits(k):
        res, P = distributed.streaming_assemble(engines[0], buf, off, k, limit, chunk_reads=chunk, fold=2)
        _check_sharded(res, P, _heavy_ref(k, limit), limit)


# ---- E. one session, alternating inputs --------------------------------------------------------
def test_alternating_inputs_in_one_session():
    """iid -> replicons -> iid -> diploid -> replicons at k = 31 in one fresh session: the
    speculative refine plan and the queued ranking rounds carried over from the previous call meet
    a graph of 170 short chains and cycles after one long chain, and back"""
    k = 31
    iid = make_reads(40_000, 12_000, 150, 8801)
    iid_ref = reference(iid[0], iid[1], k, 1)
    s = eulerhip.Session(0)
    try:
        for i, name in enumerate(("iid", "replicons", "iid", "diploid", "replicons")):
            (buf, off), ref = (iid, iid_ref) if name == "iid" else (reads_of(name, k), oracle_of(name, k))
            s.run_host(buf, off, k, 1, eulerhip.EC_FLAG_WANT_DICT)
            res = _check(s, k, ref)
            assert res.stats.count_variant == 3, (i, name)
    finally:
        s.close()
