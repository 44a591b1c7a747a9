#!/usr/bin/env python3
"""What probing the dense voxel map costs, measured on one GPU.

  python tools/probe_cost.py [--ab NAME=OTHER_LIB.so]   -> profiles/probe_cost.json

The map: tools/carve_cost.py's, a stream of C4 (128 x 2048) scans integrated stand-alone at
their poses into one map of 0.2 m voxels (max_voxels 2^25) with carving on (the default
parameters).  Then, with profiling on (HIP events around each launch; the probe launches are
the only ones under the "dense" id while they are timed), --reps repetitions each of

  probe_points   one scan's points at its pose
  probe_rays     the same scan from its pose, skip 0: with no filter, and with a miss-ratio
                 filter (max_miss_ratio 0.5)
  carve_rays     the same scan in the same process, margin 0: the yardstick (it walks the same
                 rays up to the voxel before the end, and exists without this tool's subject)

and reports the time per call, lookups per ns (the call's own `steps` over its time), the
byte model of DESIGN.md §Dense map, Probing against the HBM peak, and the ratio to the carve.
Nothing is asserted about any of these figures.

--ab (repeatable): the probe figures of this library and of other builds (FMX_LIB) in
alternating child processes on the same GPU, e.g. the plain form of the ray walk (make
BUILD=build_pa1 OUT=../ab/libfmx_probe_ahead1.so EXTRA=-DFMX_PROBE_AHEAD=1); the builds must
agree on every count.
"""
import argparse
import json
import os
import subprocess
import sys

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
MISS_RATIO = 0.5
OUT_BYTES_POINT = 1 + 24 + 8 + 4 + 4     # state, point, tag, hits, misses: what Context.probe_points asks for
OUT_BYTES_RAY = OUT_BYTES_POINT + 4 + 8  # ... and step, t


def timed(ctx, name, reps, call):
    """`reps` calls after one warm-up; the profile id's ms and launches per call, the last result."""
    call()
    ctx.profile_reset()
    for _ in range(reps):
        out = call()
    prof = ctx.profile_read()[name]
    return prof["ms"] / reps, prof["launches"] / reps, out


def figures(ms, n, steps, present, out_bytes, per_present):
    """Time, rate and the byte model of one call: the point (16), its outputs, 8 B per lookup
    (the home slot's key word; chains past it not counted), per_present where a voxel is there."""
    by = n * (16.0 + out_bytes) + steps * 8.0 + present * per_present
    return dict(us_per_call=round(ms * 1e3, 2), lookups=int(steps), lookups_per_ns=round(steps / (ms * 1e6), 3) if ms > 0 else None,
                lookups_per_point=round(steps / max(n, 1), 2), model_bytes=by,
                gbs=round(by / (ms * 1e-3) / 1e9, 1) if ms > 0 else None,
                frac_of_hbm_peak=round(by / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4) if ms > 0 else None)


def measure(a):
    geo = synth.GEOMETRIES["c4"]
    world = synth.World()
    scans = [synth.make_scan("c4", k, device="cuda:0", world=world)[0] for k in range(a.scans)]
    poses = [synth.trajectory_pose(k) for k in range(a.scans)]
    torch.cuda.synchronize()
    p = synth.default_params(geo)
    ctx = fmx.Context(fmx.EstimatorParams(extraction=fmx.KeypointExtractionParams(**p)))
    ctx.dense_configure(True, VOXEL_W, MAX_VOXELS)
    ctx.carve_configure(margin=1, ray_stride=1)
    for k in range(a.scans):
        ctx.dense_integrate(scans[k], poses[k], k)
    k = a.scans - 1 if a.probe_scan < 0 else a.probe_scan
    pts, T, n = scans[k], poses[k], int(scans[k].shape[0])
    stats = ctx.dense_stats()
    ctx.profile(True)
    out = {"map": dict(scans=a.scans, voxels=stats["voxels"], slots=stats["slots"], carve="margin 1, every ray"),
           "probed_scan": k, "points": n, "reps": a.reps}

    ms, la, r = timed(ctx, "dense", a.reps, lambda: ctx.probe_points(pts, T))
    c = r["counts"]
    valid = n - c["invalid"] - c["out_of_range"]
    out["probe_points"] = dict(figures(ms, n, valid, c["filtered"] + c["solid"], OUT_BYTES_POINT, 40.0), launches_per_call=la,
                               counts=c)
    for key, ratio in (("probe_rays", None), ("probe_rays_miss_ratio", MISS_RATIO)):
        ms, la, r = timed(ctx, "dense", a.reps, lambda: ctx.probe_rays(pts, T, max_miss_ratio=ratio))
        c = r["counts"]
        # a present voxel costs its hit count, and its miss count under a ratio; the hit's fields once per ray
        out[key] = dict(figures(ms, n, c["steps"], c["hit"], OUT_BYTES_RAY, 40.0), launches_per_call=la, counts=c,
                        max_miss_ratio=ratio, mean_range_fraction_of_hits=float(np.mean(r["t"][r["state"] == fmx.PROBE_SOLID]))
                        if c["hit"] else None)
    if not a.kernels_only:
        ctx.carve_configure(margin=0, ray_stride=1)  # (it counts misses: the yardstick comes last)
        ms, la, r = timed(ctx, "carve", a.reps, lambda: ctx.carve_rays(pts, T))
        by = r["rays"] * 16.0 + r["steps"] * 8.0 + (r["misses"] + r["exempt"]) * 8.0
        out["carve_rays_margin_0"] = dict(us_per_call=round(ms * 1e3, 2), launches_per_call=la, counts=r,
                                          lookups_per_ns=round(r["steps"] / (ms * 1e6), 3) if ms > 0 else None,
                                          lookups_per_ray=round(r["steps"] / max(r["rays"], 1), 2), model_bytes=by,
                                          gbs=round(by / (ms * 1e-3) / 1e9, 1) if ms > 0 else None)
        cu = out["carve_rays_margin_0"]["us_per_call"]
        out["over_carve"] = {key: round(out[key]["us_per_call"] / cu, 4) if cu > 0 else None
                             for key in ("probe_points", "probe_rays", "probe_rays_miss_ratio")}
    ctx.profile(False)
    ctx.close()
    return out


def ab(a):
    """This library and other builds, the probe figures only, in alternating fresh processes on this GPU."""
    libs = {"this": fmx.LIB_PATH}
    for spec in a.ab:
        name, path = spec.split("=", 1)
        libs[name] = os.path.abspath(path)
    names = list(libs)
    runs = {k: [] for k in names}
    for r in range(a.rounds):
        for name in names if r % 2 == 0 else names[::-1]:
            env = dict(os.environ, FMX_LIB=libs[name])
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--kernels-only", "--scans", str(a.scans), "--reps",
                                  str(a.reps), "--probe-scan", str(a.probe_scan)],
                                 env=env, check=True, capture_output=True, text=True, timeout=300)
            runs[name].append(json.loads(res.stdout.strip().splitlines()[-1]))
            print(f"round {r} {name}: probe_rays {runs[name][-1]['probe_rays']['us_per_call']} us", file=sys.stderr, flush=True)
    out = {"rounds": a.rounds, "this_build": a.ab_this, "other_builds": {k: os.path.basename(libs[k]) for k in names[1:]}}
    first = runs["this"][0]
    cases = ("probe_points", "probe_rays", "probe_rays_miss_ratio")
    for case in cases:
        t = {k: [x[case]["us_per_call"] for x in v] for k, v in runs.items()}
        med = {k: float(np.median(v)) for k, v in t.items()}
        out[case] = {"us_per_call_rounds": t, "us_per_call_median": med,
                     "over_this": {k: round(med[k] / med["this"], 4) for k in names[1:]}}
    out["same_counts_all_builds"] = all(x[c]["counts"] == first[c]["counts"] for v in runs.values() for x in v for c in cases)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ab", action="append", default=None, metavar="NAME=LIB.so",
                    help="other libfmx builds to compare the probe figures with, in alternating child processes")
    ap.add_argument("--ab-this", default="FMX_PROBE_AHEAD=4 (the default)")
    ap.add_argument("--scans", type=int, default=60)
    ap.add_argument("--probe-scan", type=int, default=-1, help="the scan that is probed (default: the last one integrated)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--kernels-only", action="store_true", help="print the probe figures, write nothing")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("probe_cost.py needs a GPU")
    out = {"workload": "c4 (128 x 2048) scans integrated stand-alone with carving, 0.2 m voxels; one scan probed at its pose",
           "hbm_peak_gbs": HBM_PEAK_GBS, "device": torch.cuda.get_device_name(0), "voxel_width": VOXEL_W,
           "max_voxels": MAX_VOXELS}
    out.update(measure(a))
    if a.kernels_only:
        print(json.dumps(out), flush=True)
        return
    if a.ab:
        out["ahead_ab"] = ab(a)
    provenance.stamp(out)
    os.makedirs(a.out_dir, exist_ok=True)
    with open(os.path.join(a.out_dir, "probe_cost.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
