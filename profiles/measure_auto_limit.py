"""One measured run of the coverage-aware solid threshold (ec_kmer_spectrum, ec_spectrum_threshold,
ec_refilter) on a bench.py configuration (default: ecoli10m_err, the error-rich 10 M x 100 bp
reads), outside the test suite and outside bench.py.

    python profiles/measure_auto_limit.py --legs plain                       # the plain step
    python profiles/measure_auto_limit.py --legs auto,autoclippop,clippop,fresh
    EULERHIP_LIB=/path/to/other/libeulerhip.so python profiles/measure_auto_limit.py --legs plain,plain

A leg is --steps timed steps after --warmup untimed ones on reads resident in device memory; a
step is ec_assemble_device(limit = 1) (+ ec_kmer_spectrum + ec_spectrum_threshold + ec_refilter)
(+ ec_clip_tips + ec_pop_bubbles), timed with events on the session's stream as a whole and around
the spectrum, the re-filter and the clean-ups alone.  The fresh leg is ec_assemble_device(limit =
v) with the v the rule picks on the limit-1 spectrum: what the re-filter saves is that step.
Prints one JSON line a leg: the times, contigs / N50 / n_solid before and after, the spectrum's
non-zero bins (--bins of them), the ec_spectrum_info and ec_refilter_info, the ClipInfo and
PopInfo, the session's peak device bytes."""
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

NEW = ("ec_kmer_spectrum", "ec_spectrum_threshold", "ec_refilter")


def n50(offsets):
    ls = np.sort(np.diff(offsets.astype(np.int64)))[::-1]
    if not len(ls):
        return 0
    return int(ls[np.searchsorted(np.cumsum(ls), ls.sum() / 2.0)])


def shape(res):
    ls = np.diff(res.contig_offsets.astype(np.int64))
    return {"contigs": int(res.stats.n_contigs), "n50": n50(res.contig_offsets), "n_solid": int(res.stats.n_solid),
            "chars": int(res.stats.n_contig_chars), "longest": int(ls.max()) if len(ls) else 0,
            "contigs_1000": int((ls >= 1000).sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="ecoli10m_err")
    ap.add_argument("--legs", default="plain,auto,autoclippop,clippop,fresh",
                    help="plain: no clean-up; auto: spectrum, threshold, re-filter; autoclippop: the same, then tips "
                         "and bubbles at defaults; clippop: tips and bubbles alone; fresh: a step at the limit the "
                         "rule picks")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--bins", type=int, default=1024)
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
    for name in NEW:  # an older library: the plain and clippop legs only
        if not hasattr(have, name):
            eulerhip._SIGS.pop(name, None)
    picked = None  # the limit of the first leg that ran the rule (the fresh leg's)
    for leg in a.legs.split(","):
        auto, clean, fresh = leg in ("auto", "autoclippop"), leg in ("autoclippop", "clippop"), leg == "fresh"
        if (auto or fresh) and any(n not in eulerhip._SIGS for n in NEW):
            raise SystemExit("this library has no ec_kmer_spectrum / ec_refilter")
        eulerhip.mem_stats(reset=True)
        sess = eulerhip.Session(0, stream=torch.cuda.current_stream().cuda_stream)
        if fresh and picked is None:
            sess.run_device(d_buf.data_ptr(), d_off.data_ptr(), cfg["reads"], k, 1, 0)
            si0 = eulerhip.spectrum_threshold(sess.kmer_spectrum(a.bins))
            picked = si0["limit"] if si0["found"] else 1
        limit = picked if fresh else 1
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
        t = {"step": [], "spectrum": [], "refilter": [], "clean": []}
        hist = si = ri = cinfo = pinfo = before = between = None
        for i in range(a.warmup + a.steps):
            ev[0].record()
            sess.run_device(d_buf.data_ptr(), d_off.data_ptr(), cfg["reads"], k, limit, 0)
            ev[1].record()
            if i == 0:
                before = shape(sess.fetch(k))
                ev[1].record()
            if auto:
                hist = sess.kmer_spectrum(a.bins)
                si = eulerhip.spectrum_threshold(hist)
            ev[2].record()
            if auto and si["found"]:
                r = eulerhip.RefilterInfo()
                eulerhip.check(eulerhip.lib().ec_refilter(sess._h, si["limit"], r))
                ri = r.as_dict()
                picked = si["limit"]
            ev[3].record()
            if clean:
                if i == 0 and auto:
                    between = shape(sess.fetch(k))
                    ev[3].record()
                ci, pi = eulerhip.ClipInfo(), eulerhip.PopInfo()
                eulerhip.check(eulerhip.lib().ec_clip_tips(sess._h, 0, 4, ci))
                eulerhip.check(eulerhip.lib().ec_pop_bubbles(sess._h, 0, 4, pi))
                cinfo, pinfo = ci.as_dict(), pi.as_dict()
            ev[4].record()
            torch.cuda.synchronize()
            if i >= a.warmup:
                parts = [ev[j].elapsed_time(ev[j + 1]) for j in range(4)]
                t["step"].append(sum(parts))
                t["spectrum"].append(parts[1])
                t["refilter"].append(parts[2])
                t["clean"].append(parts[3])
        res = sess.fetch(k)
        mean = lambda v: round(float(np.mean(v)), 3)  # noqa: E731
        out = {"leg": leg, "config": cfg["name"], "k": k, "limit": limit, "steps": a.steps, "warmup": a.warmup,
               "lib_version": int(eulerhip.lib().ec_version()),
               "step_ms": mean(t["step"]), "step_ms_min": round(float(np.min(t["step"])), 3),
               "step_ms_max": round(float(np.max(t["step"])), 3),
               "spectrum_ms": mean(t["spectrum"]) if auto else None,
               "spectrum_ms_min": round(float(np.min(t["spectrum"])), 3) if auto else None,
               "refilter_ms": mean(t["refilter"]) if auto else None,
               "refilter_ms_min": round(float(np.min(t["refilter"])), 3) if auto else None,
               "clean_ms": mean(t["clean"]) if clean else None,
               "spectrum_info": si, "refilter_info": ri, "clip_info": cinfo, "pop_info": pinfo,
               "spectrum_bins": a.bins if auto else None,
               "spectrum": [[int(c), int(hist[c])] for c in np.flatnonzero(hist)] if auto else None,
               "before": before, "between": between, "after": shape(res),
               "peak_session_bytes": eulerhip.mem_stats()[1]}
        print(json.dumps(out), flush=True)
        sess.close()


if __name__ == "__main__":
    main()
