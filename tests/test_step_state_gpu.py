"""The stepwise graph ABI's call-order contract (include/eulerhip.h, "CALL ORDER" and "Exact-size
outputs"): ec_count_shard -> ec_merge_owned -> ec_graph_load / ec_graph_place / ec_graph_join ->
ec_graph_chains_part .. ec_graph_collect*, driven call by call through the C ABI on one rank.

Every step whose state was released, replaced or never made (a new session, ec_session_trim, a
new count, a fused assembly, ec_graph_load, ec_graph_place) is refused with the code the header
names, before it touches the device, and the session then runs a complete stepwise assembly
bit-exact against the oracle.  Every input is synth.make_reads, every expected result
oracle.assemble_packed on the same reads."""
import ctypes

import numpy as np
import pytest

import eulerhip
import oracle
from synth import make_reads

pytestmark = pytest.mark.gpu

ARG, STATE = eulerhip.EC_ERR_ARG, eulerhip.EC_ERR_STATE
U64 = ctypes.c_uint64
TRIM_LARGE = 64 << 20  # the value HipEngine.trim_if_large and streaming_assemble pass

# the matrix's reads per k: (genome, reads, read length, seed); err = 0.002
READS = {31: (20_000, 6_000, 100, 8801), 51: (20_000, 6_000, 150, 8802)}


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


@pytest.fixture(scope="module")
def data():
    """(buf, off, oracle result) per k, computed once and never changed"""
    cache = {}

    def get(k):
        if k not in cache:
            g, n, L, seed = READS[k]
            buf, off = make_reads(g, n, L, seed, err=0.002)
            buf.setflags(write=False)
            cache[k] = (buf, off, oracle.assemble_packed(buf, off, k, 1))
        return cache[k]

    return get


def assert_oracle(res, ref):
    assert res.contig_bytes == ref["contig_chars"]
    assert np.array_equal(res.contig_offsets, ref["contig_offsets"])
    assert np.array_equal(res.link_offsets, ref["link_offsets"])
    assert np.array_equal(res.link_codes, ref["links"])
    assert res.stats.n_dict == ref["n_dict"]


class Flow:
    """One rank's stepwise assembly, one C call per method.  Each method takes its arguments from
    what the earlier steps left on the object, keeps what later steps need and returns the call's
    status, so the same method serves as a step of a legitimate sequence (run) and as the late
    call of a refusal test."""

    # the junction-partitioned graph and the partitioned finish, as distributed.streaming_assemble
    # and local_sharded_assemble(finish="partitioned") run them on one rank
    JUNCTION = ["count", "export", "merge", "place", "place_copy", "join", "apply", "chains", "chains_copy", "rank",
                "starts", "starts_copy", "layout"]
    RUNS = JUNCTION + ["emit_runs", "copy_runs", "collect_runs"]
    PART = JUNCTION + ["emit_part", "collect"]  # the job-sized character / end buffers instead
    # the loaded set with partitioned links and the one-GPU finish
    LOAD = ["count", "export", "merge", "export_dense", "load", "links_part", "finish"]

    def __init__(self, eng, buf, off, k):
        import torch

        import distributed

        self.D = distributed
        self.k = int(k)
        self.buf, self.off = buf, off
        self.d_reads = torch.from_numpy(np.array(buf)).to(eng.device)
        self.d_off = torch.from_numpy(off.astype(np.int64)).to(eng.device)
        self.nreads = len(off) - 1
        self.rb = distributed.rec_bytes(k)
        self.jb = distributed.junction_bytes(k)
        self.loaded = False
        self.bind(eng)

    def bind(self, eng):
        self.e, self.L, self.h = eng, eng.L, eng._h()
        eng.k = self.k

    def run(self, steps):
        for name in steps:
            eulerhip.check(getattr(self, name)())
        return self

    def result(self):
        return self.e.sess.fetch(self.k)

    def dense(self):
        return int(self.L.ec_dense_count(self.h))

    # -- count and owner merge
    def count(self):
        rc = self.L.ec_count_shard(self.h, ptr(self.d_reads), ptr(self.d_off), self.nreads, 0, self.k, 0)
        self.n_count = self.dense()
        return rc

    def export(self):
        counts = (U64 * 1)()
        out = self.e.empty(self.n_count * self.rb)
        rc = self.L.ec_export_by_owner(self.h, 1, ptr(out), counts)
        self.recs = out[: self.n_count * self.rb]
        return rc

    def merge(self):
        rc = self.L.ec_merge_owned(self.h, ptr(self.recs), self.n_count, self.k, 1, 0)
        self.ur = self.dense()
        return rc

    def export_dense(self):
        out = self.e.empty(self.ur * self.rb)
        rc = self.L.ec_export_dense(self.h, ptr(out))
        self.solid = out[: self.ur * self.rb]
        return rc

    # -- loaded set
    def load(self):
        rc = self.L.ec_graph_load(self.h, ptr(self.solid), self.solid.numel() // self.rb, self.k, 0)
        self.ur = self.dense()
        self.loaded = True
        return rc

    def links_part(self):
        self.succ = self.e.empty(8 * self.ur)
        return self.L.ec_graph_links_part(self.h, 0, self.ur, ptr(self.succ))

    def finish(self):
        return self.L.ec_graph_finish(self.h, ptr(self.succ), 0)

    # -- placed segment
    def place(self, out=None, nowners=1):
        counts = (U64 * nowners)()
        npal = U64(0)
        rc = self.L.ec_graph_place(self.h, 0, self.ur, nowners, None if out is None else ptr(out), counts,
                                   ctypes.byref(npal))
        self.owner_counts = [int(c) for c in counts]
        self.njrec = sum(self.owner_counts)
        self.npal = int(npal.value)
        self.loaded = False
        if out is not None:
            self.jrecs = out[: self.njrec * self.jb]
        return rc

    def place_out(self, nowners=1):
        """ec_graph_place with an output buffer of the documented bound (4 Ur records)"""
        self.ur = self.dense()
        return self.place(self.e.empty(4 * self.ur * self.jb), nowners)

    def place_copy(self):
        out = self.e.empty(self.njrec * self.jb)
        rc = self.L.ec_graph_place_copy(self.h, ptr(out))
        self.jrecs = out[: self.njrec * self.jb]
        return rc

    def join(self):
        out = self.e.empty(self.njrec * self.D.LINK_BYTES)
        counts = (U64 * 1)()
        rc = self.L.ec_graph_join(self.h, ptr(self.jrecs), self.njrec, 1, (U64 * 2)(0, self.ur), ptr(out), counts)
        self.links = out[: int(counts[0]) * self.D.LINK_BYTES]
        return rc

    def apply(self):
        return self.L.ec_graph_links_apply(self.h, ptr(self.links), self.links.numel() // self.D.LINK_BYTES)

    # -- partitioned finish
    def chains(self, out=None):
        n = U64(0)
        succ = ptr(self.succ) if self.loaded else None  # (a placed segment holds its links)
        rc = self.L.ec_graph_chains_part(self.h, 0, self.ur, succ, None if out is None else ptr(out), ctypes.byref(n))
        self.M = int(n.value)
        if out is not None:
            self.supers = out[: self.M * self.D.SUPER_BYTES]
        return rc

    def chains_copy(self):
        out = self.e.empty(self.M * self.D.SUPER_BYTES)
        rc = self.L.ec_graph_chains_copy(self.h, ptr(out))
        self.supers = out[: self.M * self.D.SUPER_BYTES]
        return rc

    def rank(self):
        return self.L.ec_graph_rank_supers(self.h, ptr(self.supers), self.M)

    def starts(self, out=None):
        n = U64(0)
        rc = self.L.ec_graph_starts_part(self.h, 1 if self.M else 0, None if out is None else ptr(out), ctypes.byref(n))
        self.nst = int(n.value)
        if out is not None:
            self.start_recs = out[: self.nst * self.D.START_BYTES]
        return rc

    def starts_copy(self):
        out = self.e.empty(self.nst * self.D.START_BYTES)
        rc = self.L.ec_graph_starts_copy(self.h, ptr(out))
        self.start_recs = out[: self.nst * self.D.START_BYTES]
        return rc

    def layout(self):
        n = U64(0)
        rc = self.L.ec_graph_layout(self.h, ptr(self.start_recs), self.nst, ctypes.byref(n))
        self.nchars = int(n.value)
        return rc

    def emit_runs(self):
        n = U64(0)
        rc = self.L.ec_graph_emit_runs(self.h, ctypes.byref(n))
        self.nbytes = int(n.value)
        return rc

    def copy_runs(self):
        out = self.e.empty(self.nbytes)
        rc = self.L.ec_graph_copy_runs(self.h, ptr(out))
        self.runs = out[: self.nbytes]
        return rc

    def collect_runs(self):
        return self.L.ec_graph_collect_runs(self.h, ptr(self.runs), 1, (U64 * 1)(self.nbytes), self.npal)

    def emit_part(self):
        self.chars = self.e.zeros(self.nchars)
        self.ends = self.e.zeros(max(2 * self.nst * self.D.end_bytes(self.k), 8))
        return self.L.ec_graph_emit_part(self.h, ptr(self.chars), ptr(self.ends))

    def collect(self):
        return self.L.ec_graph_collect(self.h, ptr(self.chars), ptr(self.ends), self.npal)


def prefix(seq, step):
    return seq[: seq.index(step)]


def suffix(seq, step):
    return seq[seq.index(step) + 1:]


@pytest.fixture
def engine():
    import distributed

    made = []

    def make():
        made.append(distributed.HipEngine(0))
        return made[-1]

    yield make
    for e in made:
        e.sess.close()


@pytest.fixture(scope="module")
def solid(data):
    """per k: the job's solid records as ec_graph_load takes them (device tensor) and its
    palindrome count, made once on a session of their own"""
    import distributed

    cache = {}

    def get(k):
        if k not in cache:
            e = distributed.HipEngine(0)
            try:
                buf, off, _ = data(k)
                f = Flow(e, buf, off, k).run(["count", "export", "merge", "export_dense", "place"])
                cache[k] = (f.solid.clone(), f.npal)
            finally:
                e.sess.close()
        return cache[k]

    return get


# ---- a. refusal matrix ------------------------------------------------------------------------
# consumer (its C entry point) -> (the legitimate sequence it belongs to, its step, the code the
# header gives a late call).  The guard of every cell, in csrc/session.h and csrc/assemble.hip:
# each invalidator clears the session flags the consumers test before their first HIP call --
#   a new session       every flag at its default
#   ec_session_trim     drop_device_state: drop_step_state (hold, runs_ready, chain_scr,
#                       part_stage) + graph_loaded, placed, dense_ok; then n_dense, whatever
#                       min_bytes released
#   ec_count_shard, ec_assemble_*   begin_call: the same drop_device_state
#                       (the count sets dense_ok again)
#   ec_graph_load       begin_call, then graph_loaded alone
#   ec_graph_place      graph_place: drop_step_state + dense_ok, then graph_loaded and placed
# -- and the consumers test
#   the three *_copy    take_pending: hold.kind is the step's          EC_ERR_STATE
#   ec_graph_copy_runs  runs_ready and graph_loaded                    EC_ERR_STATE
#   ec_export_*         dense_ok                                       EC_ERR_STATE
#   links_part, finish  graph_loaded and not placed                    EC_ERR_ARG
#   chains_part         graph_loaded                                   EC_ERR_ARG
#   rank_supers .. collect_runs   graph_loaded and part_stage >= 1 / 2 / 3 / 4   EC_ERR_ARG
#   join, links_apply   placed                                         EC_ERR_ARG
CONSUMERS = {
    "ec_graph_place_copy": (Flow.RUNS, "place_copy", STATE),
    "ec_graph_chains_copy": (Flow.RUNS, "chains_copy", STATE),
    "ec_graph_starts_copy": (Flow.RUNS, "starts_copy", STATE),
    "ec_graph_copy_runs": (Flow.RUNS, "copy_runs", STATE),
    "ec_graph_links_part": (Flow.LOAD, "links_part", ARG),
    "ec_graph_finish": (Flow.LOAD, "finish", ARG),
    "ec_graph_chains_part": (Flow.RUNS, "chains", ARG),
    "ec_graph_rank_supers": (Flow.RUNS, "rank", ARG),
    "ec_graph_starts_part": (Flow.RUNS, "starts", ARG),
    "ec_graph_layout": (Flow.RUNS, "layout", ARG),
    "ec_graph_emit_part": (Flow.PART, "emit_part", ARG),
    "ec_graph_emit_runs": (Flow.RUNS, "emit_runs", ARG),
    "ec_graph_collect": (Flow.PART, "collect", ARG),
    "ec_graph_collect_runs": (Flow.RUNS, "collect_runs", ARG),
    "ec_graph_join": (Flow.RUNS, "join", ARG),
    "ec_graph_links_apply": (Flow.RUNS, "apply", ARG),
    "ec_export_by_owner": (Flow.RUNS, "export", STATE),
    "ec_export_dense": (Flow.LOAD, "export_dense", STATE),
}
INVALIDATORS = ["fresh", "trim0", "trim_large", "count", "run_host", "load", "place_out"]
# the pairs that are no refusal: the invalidator is the very call that makes the consumer's state
POSITIVE = {
    # a new count leaves new dense records: both exports deliver them
    ("ec_export_by_owner", "count"), ("ec_export_dense", "count"),
    # ec_graph_load loads a set: its links, the one-GPU finish and the chains of its segments
    ("ec_graph_links_part", "load"), ("ec_graph_finish", "load"), ("ec_graph_chains_part", "load"),
    # ec_graph_place places a segment: the join, the received links and (its links held by the
    # session) the chains step are valid on it
    ("ec_graph_join", "place_out"), ("ec_graph_links_apply", "place_out"), ("ec_graph_chains_part", "place_out"),
}
K51_CONSUMERS = ["ec_graph_place_copy", "ec_graph_chains_copy", "ec_graph_starts_copy", "ec_graph_copy_runs",
                 "ec_graph_join"]
CELLS = [(31, c, i) for c in CONSUMERS for i in INVALIDATORS] + [(51, c, i) for c in K51_CONSUMERS for i in INVALIDATORS]


def invalidate(f, inv, make_engine, solid_k):
    """apply one invalidator to the flow's session (each a legitimate, successful call)"""
    if inv == "fresh":  # the same arguments on a session that never ran a step
        f.bind(make_engine())
    elif inv == "trim0":
        f.e.sess.trim(0)
        assert f.e.sess.device_bytes() <= 4096  # (all but the scalars)
    elif inv == "trim_large":
        # the harmless trim: every buffer of these inputs is below 64 MiB, none is released --
        # the header's choice is that the state is dropped all the same
        held = f.e.sess.device_bytes()
        f.e.sess.trim(TRIM_LARGE)
        assert f.e.sess.device_bytes() == held > 0
    elif inv == "count":
        f.run(["count"])
    elif inv == "run_host":
        f.e.sess.run_host(f.buf, f.off, f.k, 1, 0)
    elif inv == "load":
        f.solid = solid_k[0]
        f.run(["load"])
    elif inv == "place_out":
        f.run(["place_out"])
    else:
        raise AssertionError(inv)


@pytest.mark.parametrize("k,consumer,inv", [pytest.param(k, c, i, id="k%d-%s-%s" % (k, c, i)) for k, c, i in CELLS
                                            if (c, i) not in POSITIVE])
def test_late_call_is_refused(engine, data, solid, k, consumer, inv):
    """the consumer, brought to where it would be valid, then cut off by the invalidator: the code
    of the header's contract, a message, and a session that still assembles bit-exact"""
    buf, off, ref = data(k)
    seq, step, code = CONSUMERS[consumer]
    f = Flow(engine(), buf, off, k).run(prefix(seq, step))
    invalidate(f, inv, engine, solid(k))
    rc = getattr(f, step)()
    assert rc == code and rc != 0
    assert f.L.ec_last_error()
    f.loaded = False
    assert_oracle(f.run(Flow.RUNS).result(), ref)


@pytest.mark.parametrize("k,consumer,inv", [pytest.param(k, c, i, id="k%d-%s-%s" % (k, c, i)) for k, c, i in CELLS
                                            if (c, i) in POSITIVE])
def test_call_on_reestablished_state(engine, data, solid, k, consumer, inv):
    """the pairs of the matrix where the invalidator makes the consumer's state anew: the
    consumer succeeds and the sequence it belongs to ends at the oracle's result"""
    buf, off, ref = data(k)
    seq, step, _ = CONSUMERS[consumer]
    f = Flow(engine(), buf, off, k).run(prefix(seq, step))
    invalidate(f, inv, engine, solid(k))
    if inv == "count":
        if step == "export_dense":  # the count's records, exactly those the owner export delivers
            f.ur = f.n_count
            f.run(["export_dense", "export"])
            rows = lambda t: np.sort(t.cpu().numpy().view(np.dtype((np.void, f.rb))))
            assert np.array_equal(rows(f.solid), rows(f.recs))
        f.run(suffix(Flow.RUNS, "count"))
    elif inv == "load":
        f.npal = solid(k)[1]
        if step == "chains":  # the partitioned finish of the loaded set's one segment
            f.run(["links_part"] + suffix(Flow.RUNS, "apply"))
        else:
            f.run(["links_part", "finish"])
    else:  # place_out: its records joined, the links applied, the chains ranked
        f.run(suffix(Flow.RUNS, "place_copy"))
    assert_oracle(f.result(), ref)


# ---- b. both orders of the shared junction-record buffer ----------------------------------------
@pytest.mark.parametrize("k", [31, 51])
def test_place_drops_held_chain_records(engine, data, k):
    """ec_graph_chains_part keeps a placed segment's chain records in the junction-record buffer
    (tests/test_distributed_gpu.py::test_chains_drop_held_place_records has place -> chains ->
    place_copy); the reverse, chains_part(NULL) -> place(out) -> chains_copy, is refused instead of
    compacting records the place overwrote, and chains_part(NULL) -> chains_copy -> place(out)
    -> ... is an ordinary sequence"""
    buf, off, ref = data(k)
    f = Flow(engine(), buf, off, k).run(prefix(Flow.RUNS, "chains_copy"))
    assert f.M > 0
    eulerhip.check(f.place_out())
    assert f.chains_copy() == STATE
    assert f.L.ec_last_error()
    # copied first, the records are delivered; a place after that starts the graph steps over
    f.run(suffix(Flow.RUNS, "place_copy")[:3])  # join, apply, chains
    eulerhip.check(f.chains_copy())
    first = f.supers.clone()
    eulerhip.check(f.place_out())
    f.run(suffix(Flow.RUNS, "place_copy"))
    import torch

    assert torch.equal(first, f.supers)  # (the same segment and links: the same chains)
    assert_oracle(f.result(), ref)


# ---- c. two-phase equals one-phase --------------------------------------------------------------
@pytest.mark.parametrize("k", [31, 51])
def test_count_then_copy_equals_direct(engine, data, k):
    """place, chains and starts: the records of a NULL-output count plus the copy equal the records
    of the direct call on the same session state, with equal counts (owner_counts, n_pal).  Chain
    and start records byte for byte: both are placed by ballot ranks and scans in node order
    (k_tile_chains, k_tile_compact, k_starts_write).  Junction records as sorted records per
    owner segment: ec_graph_place orders them by owner with a counting sort whose cursors are
    atomics (shard.h k_cs_scatter: "the order inside a bin is not deterministic")"""
    import torch

    buf, off, ref = data(k)
    f = Flow(engine(), buf, off, k).run(prefix(Flow.RUNS, "place"))
    nown = 3  # (one session places [0, Ur) of Ur ids; the owners only group the records)
    eulerhip.check(f.place_out(nown))
    direct, counts, npal = f.jrecs.cpu().numpy(), f.owner_counts, f.npal
    eulerhip.check(f.place(None, nown))
    assert (f.owner_counts, f.npal) == (counts, npal)
    assert min(counts) > 0
    eulerhip.check(f.place_copy())
    copied = f.jrecs.cpu().numpy()
    assert copied.size == direct.size == sum(counts) * f.jb
    rows = lambda a: np.sort(a.view(np.dtype((np.void, f.jb))))
    o = 0
    for c in counts:
        assert np.array_equal(rows(direct[o * f.jb:(o + c) * f.jb]), rows(copied[o * f.jb:(o + c) * f.jb]))
        o += c
    f.run(["place", "place_copy", "join", "apply"])  # (one owner again: the join of this rank)
    # chains
    eulerhip.check(f.chains(f.e.empty(2 * f.ur * f.D.SUPER_BYTES)))
    direct, M = f.supers.clone(), f.M
    assert M > 0
    f.run(["chains", "chains_copy"])
    assert f.M == M and torch.equal(f.supers, direct)
    f.run(["rank"])
    # starts
    eulerhip.check(f.starts(f.e.empty(2 * f.ur * f.D.START_BYTES)))
    direct, nst = f.start_recs.clone(), f.nst
    assert nst > 0
    f.run(["starts", "starts_copy"])
    assert f.nst == nst and torch.equal(f.start_recs, direct)
    f.run(suffix(Flow.RUNS, "starts_copy"))
    assert_oracle(f.result(), ref)


# ---- d. one session across paths and sizes ------------------------------------------------------
@pytest.mark.parametrize("k,L", [(31, 60), (51, 150)])
def test_session_reuse_across_paths_and_sizes(k, L):
    """one HipEngine through: a partitioned step with few chains, one with many (the chain-sized
    ranking buffers of ec_graph_rank_supers grow past their spare), the one-GPU ec_graph_finish
    (whose buffers the partitioned finish sized by chains must hold every node), a fused assembly
    larger than both, the small step again, and after a trim the large one -- each bit-exact"""
    import distributed

    small = make_reads(3_000, 1_500, L, 8900 + k, err=0.0)
    large = make_reads(60_000, 40_000, 100 if k <= 32 else 150, 8910 + k, err=0.01)
    fused = make_reads(100_000, 60_000, 100 if k <= 32 else 150, 8920 + k, err=0.002)
    refs = [oracle.assemble_packed(b, o, k, 1) for b, o in (small, large, fused)]
    e = distributed.HipEngine(0)
    chains = []
    inner = e.graph_chains_part

    def spy(lo, hi, succ_part=None):
        sup, m = inner(lo, hi, succ_part)
        chains.append(m)
        return sup, m

    e.graph_chains_part = spy

    def partitioned(reads, ref):
        before = len(chains)
        assert distributed.finish_mode("partitioned", k, distributed.OWNER_MINIMIZER) == "partitioned"
        res, P = distributed.local_sharded_assemble([e], reads[0], reads[1], k, 1, finish="partitioned")
        assert len(chains) == before + 1  # the partitioned finish ran: ec_graph_chains_part was called
        assert P == ref["n_positions"]
        assert_oracle(res, ref)
        return chains[-1]

    try:
        m1 = partitioned(small, refs[0])
        m2 = partitioned(large, refs[1])
        # the growth this test is for: past the spare ec_graph_rank_supers leaves (4096 + 1/16)
        assert m2 > m1 + 4096 + m1 // 16, (m1, m2)
        before = len(chains)
        res, _ = distributed.local_sharded_assemble([e], large[0], large[1], k, 1, finish="replicated")
        assert len(chains) == before  # (ec_graph_load / links_part / ec_graph_finish)
        assert_oracle(res, refs[1])
        e.sess.run_host(fused[0], fused[1], k, 1, 0)
        assert_oracle(e.sess.fetch(k), refs[2])
        # (a step's chain count follows its tile cuts, so it may differ a little between runs of one
        # input; the growth past the small step's spare is what has to happen again)
        m3 = partitioned(small, refs[0])
        e.sess.trim(0)
        assert partitioned(large, refs[1]) > m3 + 4096 + m3 // 16
    finally:
        e.sess.close()


# ---- e. what outlives a trim ----------------------------------------------------------------------
def test_results_outlive_trim(data):
    """ec_session_trim's promise: results already copied to host memory stay fetchable"""
    buf, off, ref = data(31)
    with eulerhip.Session(0) as s:
        s.run_host(buf, off, 31, 1, 0)
        s.trim(0)
        assert s.device_bytes() <= 4096
        assert_oracle(s.fetch(31), ref)


def test_staged_batch_outlives_trim(data):
    """a batch staged with ec_stage_packed_host stays staged across a trim (its device copies are
    the slot's own buffers, not among those a trim releases) and assembles to the oracle's result"""
    buf, off, ref = data(31)
    pr = eulerhip.pack_2bit(buf, off)
    with eulerhip.Session(0) as s:
        s.stage_packed(pr)
        s.trim(0)
        s.assemble_staged(31, 1, 0)
        assert_oracle(s.fetch(31), ref)
        assert s.stats().n_positions == ref["n_positions"]
