"""One measured run of bubble popping and of the per-contig k-mer sums on a bench.py
configuration (default: ecoli10m_err, the error-rich 10 M x 100 bp reads), outside the test suite
and outside bench.py.

    python profiles/measure_pop_bubbles.py --legs plain               # the plain step
    python profiles/measure_pop_bubbles.py --legs clip,clippop,sums   # tips; tips + bubbles; sums
    python profiles/measure_pop_bubbles.py --config ecoli10m --legs sums
    EULERHIP_LIB=/path/to/other/libeulerhip.so python profiles/measure_pop_bubbles.py --legs plain,plain

A leg is --steps timed steps after --warmup untimed ones on reads resident in device memory; a
step is ec_assemble_device (+ ec_clip_tips (+ ec_pop_bubbles)), timed with events on the
session's stream as a whole and around each clean-up alone.  The sums leg times
ec_copy_contig_kmer_sums (tile table, k_contig_ksum, the copy to the host) after the plain step.
Prints one JSON line a leg: step, clip, pop and sums times, per-round time, contigs and N50 before
/ between / after, the ClipInfo and PopInfo, what kinds of contigs a clip + pop leaves, the
session's peak device bytes."""
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


def n50(offsets):
    ls = np.sort(np.diff(offsets.astype(np.int64)))[::-1]
    if not len(ls):
        return 0
    return int(ls[np.searchsorted(np.cumsum(ls), ls.sum() / 2.0)])


def shape(res):
    return {"contigs": int(res.stats.n_contigs), "n50": n50(res.contig_offsets), "n_solid": int(res.stats.n_solid),
            "chars": int(res.stats.n_contig_chars)}


def remainder(res, k):
    """what the clean-ups left: contigs by link degrees, and the short (1, 1) contigs -- branches by
    everything but a partner -- by whether another one shares their pair of ports"""
    lo, lk = res.link_offsets.astype(np.int64), res.link_codes.astype(np.int64)
    deg = np.diff(lo)
    d0, d1 = deg[0::2], deg[1::2]
    short = np.diff(res.contig_offsets.astype(np.int64)) <= 2 * k
    b = (d0 == 1) & (d1 == 1)
    i = np.nonzero(b & short)[0]
    p0, p1 = lk[lo[2 * i]] ^ 1, lk[lo[2 * i + 1]] ^ 1
    _, c = np.unique(np.minimum(p0, p1) * (1 << 32) + np.maximum(p0, p1), return_counts=True)
    return {"isolated": int(((d0 == 0) & (d1 == 0)).sum()), "one_sided": int(((d0 == 0) != (d1 == 0)).sum()),
            "one_link_a_side": int(b.sum()), "one_link_a_side_short": int((b & short).sum()),
            "more_links": int(((d0 > 0) & (d1 > 0) & ~b).sum()),
            "more_links_short": int(((d0 > 0) & (d1 > 0) & ~b & short).sum()),
            "short": int(short.sum()), "short_pairs_of_ports_shared": int((c > 1).sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="ecoli10m_err")
    ap.add_argument("--legs", default="plain,clip,clippop,sums",
                    help="plain: no clean-up; clip: tips at defaults; clippop: tips, then bubbles at defaults; "
                         "sums: the plain step, then ec_copy_contig_kmer_sums")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()

    import torch

    import bench
    import eulerhip
    from synth import make_reads

    cfg = bench.CONFIGS[a.config]
    k = cfg["k"]
    buf, off = make_reads(cfg["genome"], cfg["reads"], cfg["read_len"], cfg["seed"], err=cfg.get("err", 0.0))
    d_buf = torch.from_numpy(buf).cuda()
    d_off = torch.from_numpy(off.astype(np.int64)).cuda()
    torch.cuda.synchronize()
    have = ctypes.CDLL(eulerhip.LIB_PATH)
    for name in ("ec_clip_tips", "ec_pop_bubbles", "ec_copy_contig_kmer_sums"):  # an older library: the plain leg only
        if not hasattr(have, name):
            eulerhip._SIGS.pop(name, None)
    for leg in a.legs.split(","):
        clip, pop, sums = leg in ("clip", "clippop"), leg == "clippop", leg == "sums"
        for need, name in ((clip, "ec_clip_tips"), (pop, "ec_pop_bubbles"), (sums, "ec_copy_contig_kmer_sums")):
            if need and name not in eulerhip._SIGS:
                raise SystemExit("this library has no " + name)
        eulerhip.mem_stats(reset=True)
        sess = eulerhip.Session(0, stream=torch.cuda.current_stream().cuda_stream)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        step_ms, clip_ms, pop_ms, sums_ms = [], [], [], []
        cinfo = pinfo = before = between = None
        total = None
        for i in range(a.warmup + a.steps):
            ev[0].record()
            sess.run_device(d_buf.data_ptr(), d_off.data_ptr(), cfg["reads"], k, 1, 0)
            ev[1].record()
            if i == 0:
                before = shape(sess.fetch(k))
                ev[1].record()
            if clip:
                ci = eulerhip.ClipInfo()
                eulerhip.check(eulerhip.lib().ec_clip_tips(sess._h, 0, 4, ci))
                cinfo = ci.as_dict()
            if sums:
                total = int(sess.contig_kmer_sums().sum())
            ev[2].record()
            if pop:
                if i == 0:
                    between = shape(sess.fetch(k))
                    ev[2].record()
                pi = eulerhip.PopInfo()
                eulerhip.check(eulerhip.lib().ec_pop_bubbles(sess._h, 0, 4, pi))
                pinfo = pi.as_dict()
            ev[3].record()
            torch.cuda.synchronize()
            if i >= a.warmup:
                step_ms.append(ev[0].elapsed_time(ev[1]) + ev[1].elapsed_time(ev[2]) + ev[2].elapsed_time(ev[3]))
                (sums_ms if sums else clip_ms).append(ev[1].elapsed_time(ev[2]))
                pop_ms.append(ev[2].elapsed_time(ev[3]))
        res = sess.fetch(k)
        mean = lambda v: round(float(np.mean(v)), 3)  # noqa: E731
        out = {"leg": leg, "config": cfg["name"], "k": k, "steps": a.steps, "warmup": a.warmup,
               "lib_version": int(eulerhip.lib().ec_version()),
               "step_ms": mean(step_ms), "step_ms_min": round(float(np.min(step_ms)), 3),
               "step_ms_max": round(float(np.max(step_ms)), 3),
               "clip_ms": mean(clip_ms) if clip else None, "clip_info": cinfo,
               "pop_ms": mean(pop_ms) if pop else None,
               # (a pop of r rounds evaluates r + 1 times when it converges)
               "pop_round_ms": round(float(np.mean(pop_ms)) / max(pinfo["rounds"], 1), 3) if pop else None,
               "pop_info": pinfo,
               "sums_ms": mean(sums_ms) if sums else None,
               "sums_ms_min": round(float(np.min(sums_ms)), 3) if sums else None,
               "sums_total": total,
               "before": before, "between": between, "after": shape(res),
               "remainder": remainder(res, k) if pop else None,
               "peak_session_bytes": eulerhip.mem_stats()[1]}
        print(json.dumps(out), flush=True)
        sess.close()


if __name__ == "__main__":
    main()
