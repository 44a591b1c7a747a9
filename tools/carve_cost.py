#!/usr/bin/env python3
"""What carving the dense voxel map costs, measured on one GPU.

  python tools/carve_cost.py                          -> profiles/carve_cost.json
  python tools/carve_cost.py --ab NAME=OTHER_LIB.so   -> profiles/carve_ahead_ab.json

Kernels: a stream of C4 (128 x 2048) scans integrated stand-alone at their poses into one
growing map of 0.2 m voxels with carving on and profiling on (HIP events around each
launch).  The "carve" profile id holds both launches of a carve (mark, rays); the tool
reports their time per integration, the rays and the steps per ray from the launches' own
counts, and the byte model of DESIGN.md §Dense map, Carving (16 B per ray's point, 8 B per
step, + 8 B where the voxel is present, + 8 B per point for the mark) against the HBM peak.
Twice: with the default parameters (every ray, margin 1, the dense gate) and with
ray_stride 4.

Stream: --scans C4 scans through fmx_register_scan with the dense map on in both arms and
carving off / on (every integration carved, the default parameters), the two arms alternated
over --rounds rounds on fresh contexts in this one process on this one GPU; the median
per-scan host time of each arm and their ratio (reported, not asserted).

--ab (repeatable): the kernel figures of this library and of other builds (FMX_LIB) in
alternating child processes on the same GPU, e.g. the plain form of the ray walk (make
BUILD=build_a1 OUT=../ab/libfmx_ahead1.so EXTRA=-DFMX_CARVE_AHEAD=1).
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from form_amd import fmx, synth  # noqa: E402
import provenance  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E peak (spec), as bench.py
VOXEL_W = 0.2
MAX_VOXELS = 1 << 25


def new_ctx(geo, carve=None):
    p = synth.default_params(geo)
    ctx = fmx.Context(fmx.EstimatorParams(extraction=fmx.KeypointExtractionParams(**p)))
    ctx.dense_configure(True, VOXEL_W, MAX_VOXELS)
    if carve is not None:
        ctx.carve_configure(**carve)
    return ctx


def kernels(geo, scans, poses, carve):
    ctx = new_ctx(geo, carve)
    for k in range(3):  # code objects, buffers
        ctx.dense_integrate(scans[k], poses[k], k)
    ctx.dense_clear()
    ctx.profile(True)
    ctx.profile_reset()
    tot = dict(rays=0, steps=0, misses=0, exempt=0)
    for k in range(len(scans)):
        ctx.dense_integrate(scans[k], poses[k], k)
        c, carved = ctx.carve_last()
        assert carved == 1
        for f in tot:
            tot[f] += c[f]
    prof = ctx.profile_read()
    ctx.profile(False)
    n, pts = len(scans), int(scans[0].shape[0])
    ms = prof["carve"]["ms"] / n
    by = (pts * 8.0 * n + tot["rays"] * 16.0 + tot["steps"] * 8.0 + (tot["misses"] + tot["exempt"]) * 8.0) / n
    out = dict(parameters=carve, integrations=n, launches=prof["carve"]["launches"], points_per_scan=pts,
               mark_plus_rays_us_per_integration=round(ms * 1e3, 2),
               claim_plus_fill_us_per_integration=round(prof["dense"]["ms"] / n * 1e3, 2),
               rays_per_integration=round(tot["rays"] / n, 1), steps_per_ray=round(tot["steps"] / max(tot["rays"], 1), 2),
               steps_per_integration=round(tot["steps"] / n, 1),
               present_per_step=round((tot["misses"] + tot["exempt"]) / max(tot["steps"], 1), 4),
               misses_per_integration=round(tot["misses"] / n, 1), exempt_per_integration=round(tot["exempt"] / n, 1),
               lookups_per_us=round(tot["steps"] / n / (ms * 1e3), 1) if ms > 0 else None,
               model_bytes_per_integration=by, gbs=round(by / (ms * 1e-3) / 1e9, 1) if ms > 0 else None,
               frac_of_hbm_peak=round(by / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4) if ms > 0 else None,
               voxels_after_stream=ctx.dense_stats()["voxels"], slots=ctx.dense_stats()["slots"])
    ctx.close()
    return out


def run_stream(ctx, items, skip):
    marks = []
    for k, it in enumerate(items):
        if k == skip:
            ctx.sync()
            marks.append(time.perf_counter())
        ctx.register_scan(it)
        if k >= skip:
            marks.append(time.perf_counter())
    ctx.sync()
    return np.diff(marks)


def stream(a, geo, scans):
    per = {False: [], True: []}
    pose, last = {}, None
    for r in range(a.rounds + 1):  # round 0 warms both arms up
        for carve in (False, True) if r % 2 == 0 else (True, False):
            ctx = new_ctx(geo, dict() if carve else None)
            dt = run_stream(ctx, scans, a.skip)
            pose[carve] = np.asarray(ctx.current_pose()).copy()
            if carve:
                last = (ctx.carve_last()[0], ctx.dense_stats())
            ctx.close()
            if r:
                per[carve].append(float(np.median(dt)) * 1e3)
    off_ms, on_ms = float(np.median(per[False])), float(np.median(per[True]))
    return {
        "scans": len(scans), "skipped": a.skip, "rounds": a.rounds, "dense_map": "on in both arms, every scan integrated",
        "carve_off_ms_median": round(off_ms, 4), "carve_on_ms_median": round(on_ms, 4),
        "carve_off_ms_rounds": [round(x, 4) for x in per[False]], "carve_on_ms_rounds": [round(x, 4) for x in per[True]],
        "on_over_off": round(on_ms / off_ms, 4), "added_us_per_scan": round((on_ms - off_ms) * 1e3, 2),
        "last_scan_carve_counts": last[0], "voxels_after_stream": last[1]["voxels"],
        "same_final_pose": bool(np.array_equal(pose[False], pose[True])),
    }


def ab(a):
    """This library and other builds, kernels only, in alternating fresh processes on this GPU."""
    libs = {"this": fmx.LIB_PATH}
    for spec in a.ab:
        name, path = spec.split("=", 1)
        libs[name] = os.path.abspath(path)
    names = list(libs)
    runs = {k: [] for k in names}
    for r in range(a.rounds):
        for name in names if r % 2 == 0 else names[::-1]:
            env = dict(os.environ, FMX_LIB=libs[name])
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--kernels-only", "--scans", str(a.scans)],
                                 env=env, check=True, capture_output=True, text=True, timeout=300)
            runs[name].append(json.loads(res.stdout.strip().splitlines()[-1]))
    out = {"workload": "c4 (128 x 2048) stand-alone integrations with carving on, 0.2 m voxels", "rounds": a.rounds,
           "scans": a.scans, "this_build": a.ab_this, "other_builds": {k: os.path.basename(libs[k]) for k in names[1:]}}
    first = runs["this"][0]
    for case in ("kernels_default", "kernels_ray_stride_4"):
        t = {k: [x[case]["mark_plus_rays_us_per_integration"] for x in v] for k, v in runs.items()}
        med = {k: float(np.median(v)) for k, v in t.items()}
        out[case] = {"us_per_integration_rounds": t, "us_per_integration_median": med,
                     "over_this": {k: round(med[k] / med["this"], 4) for k in names[1:]},
                     "steps_per_integration": first[case]["steps_per_integration"]}
    same = ("rays_per_integration", "steps_per_integration", "misses_per_integration", "exempt_per_integration",
            "voxels_after_stream")
    out["same_counts_all_builds"] = all(x[c][f] == first[c][f] for v in runs.values() for x in v
                                        for c in ("kernels_default", "kernels_ray_stride_4") for f in same)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ab", action="append", default=None, metavar="NAME=LIB.so",
                    help="other libfmx builds to compare the kernel figures with -> profiles/carve_ahead_ab.json")
    ap.add_argument("--ab-this", default="FMX_CARVE_AHEAD=4 (the default)")
    ap.add_argument("--scans", type=int, default=60)
    ap.add_argument("--skip", type=int, default=20, help="scans before the timed ones (the window fills)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--kernels-only", action="store_true", help="print the kernel figures, write nothing")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("carve_cost.py needs a GPU")
    if a.ab:
        out = provenance.stamp(dict(ab(a), device=torch.cuda.get_device_name(0)))
        os.makedirs(a.out_dir, exist_ok=True)
        with open(os.path.join(a.out_dir, "carve_ahead_ab.json"), "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
        print(json.dumps(out), flush=True)
        return
    geo = synth.GEOMETRIES["c4"]
    world = synth.World()
    scans = [synth.make_scan("c4", k, device="cuda:0", world=world)[0] for k in range(a.scans)]
    poses = [synth.trajectory_pose(k) for k in range(a.scans)]
    torch.cuda.synchronize()
    out = {"workload": "c4 (128 x 2048), smoothing mode, dense map of 0.2 m voxels on", "hbm_peak_gbs": HBM_PEAK_GBS,
           "device": torch.cuda.get_device_name(0), "voxel_width": VOXEL_W, "max_voxels": MAX_VOXELS,
           "kernels_default": kernels(geo, scans, poses, dict(margin=1, ray_stride=1)),
           "kernels_ray_stride_4": kernels(geo, scans, poses, dict(margin=1, ray_stride=4))}
    if a.kernels_only:
        print(json.dumps(out), flush=True)
        return
    out["stream_sequential"] = stream(a, geo, scans)
    provenance.stamp(out)
    os.makedirs(a.out_dir, exist_ok=True)
    with open(os.path.join(a.out_dir, "carve_cost.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
