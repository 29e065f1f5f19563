"""One measured run of tip clipping on a bench.py configuration (default: ecoli10m_err, the
error-rich 10 M x 100 bp reads), outside the test suite and outside bench.py.

    python profiles/measure_clip_tips.py --legs plain            # the unclipped step
    python profiles/measure_clip_tips.py --legs clip,clip1       # default settings, max_rounds = 1
    EULERHIP_LIB=/path/to/other/libeulerhip.so python profiles/measure_clip_tips.py --legs plain

A leg is --steps timed steps after --warmup untimed ones on reads resident in device memory; a
step is ec_assemble_device (+ ec_clip_tips), timed with events on the session's stream as a whole
and around the clip alone.  Prints one JSON line a leg: step and clip times, per-round time,
contigs and N50 before / after, the ClipInfo, the session's peak device bytes."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="ecoli10m_err")
    ap.add_argument("--legs", default="plain,clip,clip1", help="plain: no clip; clip: defaults; clip1: max_rounds = 1")
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
    if not hasattr(ctypes.CDLL(eulerhip.LIB_PATH), "ec_clip_tips"):  # an older library: the plain leg only
        eulerhip._SIGS.pop("ec_clip_tips", None)
    can_clip = "ec_clip_tips" in eulerhip._SIGS
    for leg in a.legs.split(","):
        rounds = {"plain": 0, "clip": 4, "clip1": 1}[leg]
        if rounds and not can_clip:
            raise SystemExit("this library has no ec_clip_tips")
        eulerhip.mem_stats(reset=True)
        sess = eulerhip.Session(0, stream=torch.cuda.current_stream().cuda_stream)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        step_ms, clip_ms, info, before = [], [], None, None
        for i in range(a.warmup + a.steps):
            ev[0].record()
            sess.run_device(d_buf.data_ptr(), d_off.data_ptr(), cfg["reads"], k, 1, 0)
            ev[1].record()
            if i == 0:
                r0 = sess.fetch(k)
                before = {"contigs": int(r0.stats.n_contigs), "n50": n50(r0.contig_offsets),
                          "n_solid": int(r0.stats.n_solid), "chars": int(r0.stats.n_contig_chars)}
                ev[1].record()
            if rounds:
                ci = eulerhip.ClipInfo()
                eulerhip.check(eulerhip.lib().ec_clip_tips(sess._h, 0, rounds, ci))
                info = ci.as_dict()
            ev[2].record()
            torch.cuda.synchronize()
            if i >= a.warmup:
                step_ms.append(ev[0].elapsed_time(ev[1]) + ev[1].elapsed_time(ev[2]))
                clip_ms.append(ev[1].elapsed_time(ev[2]))
        res = sess.fetch(k)
        out = {"leg": leg, "config": cfg["name"], "k": k, "steps": a.steps, "warmup": a.warmup,
               "lib_version": int(eulerhip.lib().ec_version()),
               "step_ms": round(float(np.mean(step_ms)), 3), "step_ms_min": round(float(np.min(step_ms)), 3),
               "step_ms_max": round(float(np.max(step_ms)), 3),
               "clip_ms": round(float(np.mean(clip_ms)), 3) if rounds else None,
               "round_ms": round(float(np.mean(clip_ms)) / max(info["rounds"], 1), 3) if rounds else None,
               "clip_info": info, "before": before,
               "after": {"contigs": int(res.stats.n_contigs), "n50": n50(res.contig_offsets),
                         "n_solid": int(res.stats.n_solid), "chars": int(res.stats.n_contig_chars)},
               "peak_session_bytes": eulerhip.mem_stats()[1]}
        print(json.dumps(out), flush=True)
        sess.close()


if __name__ == "__main__":
    main()
