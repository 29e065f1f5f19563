"""The solid limit chosen on the sharded path (distributed.sharded_assemble(auto_limit=True),
ec_dense_spectrum / ec_dense_refilter, euler_run --limit auto), the part that needs no GPU: the
symbols, the command line's argument check, and the orchestration itself over gloo at world 2 and
3 with tests/fake_auto_engine.py -- the owner merge at limit 1, the ranks' spectra all-reduced,
the threshold rule on the sum, every rank re-filtering its segment.  Rows of spectrum_model.FIXED
(k <= 32; 256 bins): auto_info must equal the row, and contigs and links must equal the oracle's
build(limit = the row's) + all_contigs -- limit 1 for the row where no limit is found."""
import ctypes
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch.multiprocessing as mp

import oracle
import spectrum_model
from conftest import PKG, ROOT
from spectrum_model import FIXED, info_of
from synth import make_reads

LIB = os.path.join(PKG, "libeulerhip.so")
needs_lib = pytest.mark.skipif(not os.path.exists(LIB), reason="libeulerhip.so not built")
NBINS = 256  # the bins FIXED was computed with

# k = 15 (key-hash owners), k = 21 (minimizer owners), and the row where the rule finds no limit
ROWS = [FIXED[2], FIXED[0], FIXED[5]]
assert all(c[5] <= 32 for c, _ in ROWS) and ROWS[2][1][0] == 0 and ROWS[0][1][0] == ROWS[1][1][0] == 1
ROW_IDS = ["-".join(str(x) for x in c) for c, _ in ROWS]


@needs_lib
def test_symbols_bound_and_version():
    import eulerhip

    L = eulerhip.lib()
    for name in ("ec_dense_spectrum", "ec_dense_refilter"):
        assert name in eulerhip._SIGS and hasattr(L, name)
    assert L.ec_version() == 500
    # argument errors need no device: NULLs and bins out of range
    hist = (ctypes.c_uint64 * 8)()
    ri = eulerhip.RefilterInfo()
    assert L.ec_dense_spectrum(None, 8, hist) == eulerhip.EC_ERR_ARG
    assert L.ec_dense_refilter(None, 1, ctypes.byref(ri)) == eulerhip.EC_ERR_ARG
    import distributed

    for m in distributed.AUTO_METHODS:
        assert hasattr(distributed.HipEngine, m)


def test_cli_rejects_a_limit_that_is_no_number():
    """argparse refuses it (status 2) before torch is imported"""
    code = ("import sys; sys.argv = ['euler_run.py', '-i', 'x.fa', '--limit', 'banana']\n"
            "import runpy\n"
            "try:\n"
            "    runpy.run_path(%r, run_name='__main__')\n"
            "except SystemExit as e:\n"
            "    print('status', e.code, 'torch' in sys.modules)\n" % os.path.join(PKG, "euler_run.py"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.stdout.split() == ["status", "2", "False"], (r.stdout, r.stderr[-2000:])
    assert "banana" in r.stderr


def test_cli_limit_argument():
    import euler_run

    assert euler_run.limit_arg("auto") is None and euler_run.limit_arg("7") == 7 and euler_run.limit_arg("-1") == -1
    # the refusals that need neither torch nor a GPU
    assert euler_run.main(["-i", "x", "--limit", "auto", "--spectrum-bins", "1"]) == 2
    assert euler_run.main(["-i", "x", "--spectrum-out", "s.tsv"]) == 2
    assert euler_run.main(["-i", "x", "--auto-limit", "--sharded"]) == 2


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, reads, k, q, finish, partitioned, plain):
    """puts exactly one tuple on q, whatever happens: (rank, info, calls, contigs, links), or
    (rank, "RuntimeError" | "error", message, None, None)"""
    try:
        import torch
        import torch.distributed as dist

        for p in (PKG, os.path.join(ROOT, "oracle"), os.path.dirname(os.path.abspath(__file__))):
            if p not in sys.path:
                sys.path.insert(0, p)
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        try:
            import distributed
            from fake_auto_engine import FakeAutoEngine
            from fake_engine import FakeEngine

            lo, hi = distributed.shard_range(len(reads), rank, world)
            mine = reads[lo:hi]
            buf = "".join(mine).encode()
            off = np.zeros(len(mine) + 1, np.int64)
            off[1:] = np.cumsum([len(r) for r in mine])
            eng = FakeEngine(k) if plain else FakeAutoEngine(k)
            info = {}
            try:
                res, P = distributed.sharded_assemble(eng, distributed.TorchComm(),
                                                      torch.frombuffer(bytearray(buf or b"\0"), dtype=torch.uint8),
                                                      torch.from_numpy(off), len(mine), lo, k, 1, finish=finish,
                                                      partitioned=partitioned, auto_limit=True, spectrum_bins=NBINS,
                                                      auto_info=info)
            except RuntimeError as e:
                q.put((rank, "RuntimeError", str(e), None, None))
                return
            q.put((rank, info, getattr(eng, "auto_calls", None), res.contigs if res else None,
                   res.links if res else None))
        finally:
            dist.destroy_process_group()
    except Exception as e:  # (anything else: reported, so that the test fails at once instead of waiting)
        q.put((rank, "error", "%s: %s" % (type(e).__name__, e), None, None))


def _run(reads, k, world, finish="partitioned", partitioned=None, plain=False):
    """every rank's tuple in rank order.  A rank that reports an error, or dies without reporting,
    ends the run at once: the other ranks may be waiting for it in a collective, so they are
    stopped, and the test fails with what was reported."""
    import queue

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, reads, k, q, finish, partitioned, plain))
             for r in range(world)]
    for p in procs:
        p.start()
    out, failed = [], None
    try:
        while len(out) < world and failed is None:
            try:
                o = q.get(timeout=0.2)
            except queue.Empty:
                dead = [p for p in procs if p.exitcode not in (None, 0)]
                if dead:
                    failed = "a rank died with exit code %s" % dead[0].exitcode
                elif all(p.exitcode == 0 for p in procs) and q.empty():
                    failed = "ranks ended without a result"
                continue
            if o[1] == "error":
                failed = "rank %d: %s" % (o[0], o[2])
            out.append(o)
    finally:
        for p in procs:
            if failed is not None and p.is_alive():
                p.terminate()
            p.join(60)
    assert failed is None, failed
    assert all(p.exitcode == 0 for p in procs)
    return sorted(out, key=lambda o: o[0])


_cache = {}


def _row(case):
    """reads, the oracle's limit-1 dict spectrum, and the oracle's result at each limit: computed once"""
    if case not in _cache:
        G, n, L, seed, err, k = case
        buf, off = make_reads(G, n, L, seed, err=err)
        s = buf.tobytes().decode()
        reads = [s[int(off[i]):int(off[i + 1])] for i in range(len(off) - 1)]
        d = oracle.assemble_packed(buf, off, k, 1, want_dict=True)["d"]
        _cache[case] = (reads, spectrum_model.spectrum(d, NBINS), {})
    return _cache[case]


def _oracle_at(case, limit):
    reads, _, refs = _row(case)
    if limit not in refs:
        _, rc, rl = oracle.assemble(reads, case[5], limit, want_dict=False)
        refs[limit] = (rc, rl)
    return refs[limit]


def _want_info(want, h):
    found, lo, d, p, floor, limit, n_solid, kept = want
    w = info_of(found, lo, d, p, floor, limit)
    w["spectrum"] = {c: v for c, v in enumerate(h) if v}
    w["n_solid_before"], w["n_solid_after"] = n_solid, kept
    return w


@pytest.mark.parametrize("case,want", ROWS, ids=ROW_IDS)
def test_fixed_rows_hold_on_the_oracles_dict(case, want):
    """the expectations themselves, before any engine runs"""
    _, h, _ = _row(case)
    assert spectrum_model.threshold(h) == info_of(*want[:6])
    assert sum(h) == want[6]
    assert sum(h[want[5] + 1:]) == want[7] if want[0] else want[7] == want[6]


@needs_lib
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("case,want", ROWS, ids=ROW_IDS)
def test_sharded_auto_limit_matches_oracle(case, want, world):
    reads, h, _ = _row(case)
    k = case[5]
    L = want[5] if want[0] else 1
    rc, rl = _oracle_at(case, L)
    out = _run(reads, k, world)
    assert len(out) == world
    for rank, info, calls, contigs, links in out:
        assert info == _want_info(want, h), rank  # every rank: the same histogram, the same answer
        assert calls == [("dense_spectrum", NBINS)] + ([("dense_refilter", want[5])] if want[0] else []), rank
    assert out[0][3] == rc and out[0][4] == rl
    assert all(o[3] is None for o in out[1:])  # (the partitioned finish: rank 0 holds the result)


@needs_lib
@pytest.mark.parametrize("partitioned", [True, False])
def test_sharded_auto_limit_all_gather_paths(partitioned):
    """the replicated finish and the unpartitioned graph continue from export_dense()"""
    case, want = ROWS[0]
    reads, h, _ = _row(case)
    rc, rl = _oracle_at(case, want[5])
    for rank, info, calls, contigs, links in _run(reads, case[5], 2, finish="replicated", partitioned=partitioned):
        assert info == _want_info(want, h)
        assert calls == [("dense_spectrum", NBINS), ("dense_refilter", want[5]), ("export_dense",)]
        assert contigs == rc and links == rl


def test_auto_limit_needs_the_engines_calls():
    """a plain FakeEngine has none of them: a RuntimeError that names the engine, on every rank,
    before any collective"""
    case, _ = ROWS[0]
    reads, _, _ = _row(case)
    for rank, kind, msg, _, _ in _run(reads[:40], case[5], 2, plain=True):
        assert kind == "RuntimeError" and "FakeEngine" in msg and "dense_spectrum" in msg


def test_auto_limit_off_calls_nothing_new():
    """auto_limit = False: a FakeAutoEngine sees none of its three calls (today's call sequence)"""
    import torch

    import distributed
    from fake_auto_engine import FakeAutoEngine

    class OneRank:
        rank, world = 0, 1

        def __init__(self):
            self.torch = torch

        def alltoallv(self, send, counts_bytes, tag=0, meta=None):
            n = sum(counts_bytes)
            return (send[:n], tag, [n], [list(meta)]) if meta is not None else (send[:n], tag)

        def allgatherv(self, t, fill=0, with_sizes=False, sizes=None):
            return (t, [t.numel()]) if with_sizes else t

        def allgather_int(self, v):
            return [int(v)]

        def allreduce_vec(self, vals):
            return [int(v) for v in vals]

        def reduce_sum(self, t, dst=0):
            return t

    case, want = ROWS[0]
    reads, h, _ = _row(case)
    k = case[5]
    reads = reads[:300]
    buf = "".join(reads).encode()
    off = np.zeros(len(reads) + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in reads])
    args = (torch.frombuffer(bytearray(buf), dtype=torch.uint8), torch.from_numpy(off), len(reads), 0, k, 1)
    eng = FakeAutoEngine(k)
    res, _ = distributed.sharded_assemble(eng, OneRank(), *args)
    assert eng.auto_calls == []
    _, rc, rl = oracle.assemble(reads, k, 1, want_dict=False)
    assert res.contigs == rc and res.links == rl
