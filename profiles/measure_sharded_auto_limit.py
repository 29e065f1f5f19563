"""One measured run of the solid limit chosen on the sharded path (ec_dense_spectrum,
ec_dense_refilter, distributed.*_assemble(auto_limit=True)) on a bench.py configuration (default:
ecoli10m_err, the error-rich 10 M x 100 bp reads, k = 31), outside the test suite and outside
bench.py.

    python profiles/measure_sharded_auto_limit.py --ranks 1 --legs limit1,auto,given,filter
    EULERHIP_LIB=/path/to/parent/libeulerhip.so python profiles/measure_sharded_auto_limit.py --legs limit1

A leg is --steps timed steps after --warmup untimed ones, timed with events on the stream the
engines run on.  --ranks 1: the sharded step of one rank (distributed.sharded_assemble with a
one-rank communicator, reads resident in device memory); --ranks N > 1: N simulated ranks on the one
GPU (distributed.local_sharded_assemble: host reads, so every step of every leg also copies the
shards to the device).
  limit1   the sharded step at limit = 1 (any library: the parent's against this tree's)
  auto     auto_limit = True: the merge at limit 1, spectrum, threshold, ec_dense_refilter, graph
  given    the sharded step at limit = --given (5: what the rule picks on ecoli10m_err)
  filter   on rank 0's owner segment after the limit-1 merge (restored before every timed step,
           untimed): ec_dense_refilter(--given) alone, against the route a library without it
           allows, ec_export_dense -> ec_merge_owned(limit = --given) on the same records
Prints one JSON line a leg: the times, and for the whole-step legs the result's contigs / N50 /
solid k-mers and the auto_info.  --cache DIR keeps the generated reads there as .npy files (several
processes of one measurement read them instead of generating them again)."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "pycuda-euler_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

NEW = ("ec_dense_spectrum", "ec_dense_refilter")


def n50(offsets):
    ls = np.sort(np.diff(offsets.astype(np.int64)))[::-1]
    if not len(ls):
        return 0
    return int(ls[np.searchsorted(np.cumsum(ls), ls.sum() / 2.0)])


def shape(res):
    ls = np.diff(res.contig_offsets.astype(np.int64))
    return {"contigs": int(res.stats.n_contigs), "n50": n50(res.contig_offsets), "n_solid": int(res.stats.n_solid),
            "chars": int(res.stats.n_contig_chars), "longest": int(ls.max()) if len(ls) else 0}


class OneRank:
    """the collectives of a one-rank job (distributed.TorchComm's interface, nothing to exchange)"""
    rank, world = 0, 1

    def __init__(self, torch):
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


def load_reads(cfg, cache):
    from synth import make_reads

    if cache:
        fb, fo = (os.path.join(cache, "%s_%s.npy" % (cfg["name"], x)) for x in ("buf", "off"))
        if os.path.exists(fb) and os.path.exists(fo):
            return np.load(fb), np.load(fo)
    buf, off = make_reads(cfg["genome"], cfg["reads"], cfg["read_len"], cfg["seed"], err=cfg.get("err", 0.0))
    if cache:
        os.makedirs(cache, exist_ok=True)
        np.save(fb, buf)
        np.save(fo, off)
    return buf, off


def stat(v):
    return {"mean": round(float(np.mean(v)), 3), "min": round(float(np.min(v)), 3), "max": round(float(np.max(v)), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="ecoli10m_err")
    ap.add_argument("--legs", default="limit1,auto,given,filter")
    ap.add_argument("--ranks", type=int, default=1)
    ap.add_argument("--given", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--bins", type=int, default=1024)
    ap.add_argument("--cache", default="")
    a = ap.parse_args()

    import torch

    import bench
    import distributed as D
    import eulerhip

    cfg = dict(bench.CONFIGS[a.config], name=a.config)
    k = cfg["k"]
    buf, off = load_reads(cfg, a.cache)
    nreads = len(off) - 1
    have = ctypes.CDLL(eulerhip.LIB_PATH)
    for name in NEW:  # an older library: the limit1 and given legs, and the filter leg's merge route
        if not hasattr(have, name):
            eulerhip._SIGS.pop(name, None)
    has_new = all(n in eulerhip._SIGS for n in NEW)
    engines = [D.HipEngine(0) for _ in range(a.ranks)]
    if a.ranks == 1:
        d_buf = torch.from_numpy(buf).cuda()
        d_off = torch.from_numpy(off.astype(np.int64)).cuda()
        comm = OneRank(torch)
    torch.cuda.synchronize()

    def step(limit, auto, info):
        kw = dict(auto_limit=True, spectrum_bins=a.bins, auto_info=info) if auto else {}
        if a.ranks == 1:
            return D.sharded_assemble(engines[0], comm, d_buf, d_off, nreads, 0, k, limit, **kw)[0]
        return D.local_sharded_assemble(engines, buf, off, k, limit, **kw)[0]

    base = {"config": a.config, "k": k, "ranks": a.ranks, "steps": a.steps, "warmup": a.warmup,
            "lib": os.path.basename(os.path.dirname(eulerhip.LIB_PATH)) + "/" + os.path.basename(eulerhip.LIB_PATH),
            "lib_version": int(eulerhip.lib().ec_version())}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    for leg in a.legs.split(","):
        if leg == "auto" and not has_new:
            raise SystemExit("this library has no ec_dense_spectrum / ec_dense_refilter")
        if leg in ("limit1", "auto", "given"):
            limit = a.given if leg == "given" else 1
            t, info, res = [], {}, None
            for i in range(a.warmup + a.steps):
                info = {}
                ev[0].record()
                res = step(limit, leg == "auto", info)
                ev[1].record()
                torch.cuda.synchronize()
                if i >= a.warmup:
                    t.append(ev[0].elapsed_time(ev[1]))
            info.pop("spectrum", None)
            print(json.dumps(dict(base, leg=leg, limit=limit, step_ms=stat(t), result=shape(res),
                                  auto_info=info or None)), flush=True)
            continue
        if leg != "filter":
            raise SystemExit("unknown leg %r" % leg)
        # rank 0's owner segment: count, export by owner, exchange (as local_sharded_assemble_shards)
        sends, bases = [], []
        for r, eng in enumerate(engines):
            lo, hi = D.shard_range(nreads, r, a.ranks)
            b = torch.from_numpy(np.ascontiguousarray(buf[int(off[lo]):int(off[hi])])).cuda()
            o = torch.from_numpy((off[lo:hi + 1] - off[lo]).astype(np.int64)).cuda()
            eng.set_owner_rule(D.OWNER_MINIMIZER)
            eng.count_shard(b, o, hi - lo, lo, k, 0)
            recs, counts, lfb = eng.export_by_owner(a.ranks, compact=True)
            rb = D.compact_bytes(k) if lfb >= 0 else D.rec_bytes(k)
            sends.append((recs[: counts[0] * rb].clone(), lfb))
            bases.append(lo)
            del recs, b, o
            eng.sess.trim(0)
        got = torch.cat([s[0] for s in sends]) if a.ranks > 1 else sends[0][0]
        margs = ([s[0].numel() for s in sends], bases, [s[1] for s in sends])
        eng = engines[0]
        t_f, t_x, t_m, n0 = [], [], [], 0
        kept_f = kept_m = None
        for i in range(a.warmup + a.steps):
            if has_new:
                n0 = eng.merge_owned_from(got, *margs, k, 1, 0, export=False)
                ev[0].record()
                kept_f, _ = eng.dense_refilter(a.given)
                ev[1].record()
                torch.cuda.synchronize()
                if i >= a.warmup:
                    t_f.append(ev[0].elapsed_time(ev[1]))
            n0 = eng.merge_owned_from(got, *margs, k, 1, 0, export=False)
            ev[0].record()
            seg = eng.export_dense()
            ev[1].record()
            kept_m = eng.merge_owned(seg, k, a.given, 0, export=False)
            ev[2].record()
            torch.cuda.synchronize()
            if i >= a.warmup:
                t_x.append(ev[0].elapsed_time(ev[1]))
                t_m.append(ev[1].elapsed_time(ev[2]))
        rbk = 28 if k <= 32 else 36  # key, count and two first events of a record (no padding)
        out = dict(base, leg=leg, limit=a.given, segment_records=n0, kept_refilter=kept_f, kept_merge=kept_m,
                   refilter_ms=stat(t_f) if t_f else None, export_dense_ms=stat(t_x), merge_owned_ms=stat(t_m),
                   # what the filter must move: the counts twice (both passes), the kept records read, written to
                   # scratch, read there and written back
                   refilter_bytes=2 * 4 * n0 + 4 * rbk * (kept_f or 0) if has_new else None)
        if t_f:
            out["refilter_GBps_of_min"] = round(out["refilter_bytes"] / (out["refilter_ms"]["min"] * 1e6), 1)
        print(json.dumps(out), flush=True)
    for eng in engines:
        eng.sess.close()


if __name__ == "__main__":
    main()
