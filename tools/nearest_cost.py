#!/usr/bin/env python3
"""What the nearest-voxel search of the dense map costs, measured on one GPU.

  python tools/nearest_cost.py [--ab NAME=OTHER_LIB.so]   -> profiles/nearest_cost.json

The map: tools/carve_cost.py's, a stream of C4 (128 x 2048) scans integrated stand-alone at
their poses into one map of 0.2 m voxels (max_voxels 2^25) with carving on (the default
parameters).  Then, with profiling on (HIP events around each launch; the timed launches are the
only ones under the "dense" id), --reps repetitions each of

  nearest_voxels   the last scan's points at their own pose, and a 4096-point subset of them
                   (every 64th): reach 1, 2 and 4, with no limit and with max_dist2 =
                   (reach * voxel_width)^2
  probe_points     the same scan: the yardstick of one lookup per point
  probe_rays       the same scan from its pose, skip 0: the yardstick of a chain of lookups

and reports the time per call, the call's own `lookups`, lookups per ns and the byte model of
DESIGN.md §Dense map, Nearest against the HBM peak.  The kernel does not count the present and
the solid voxels it met, so the model's "+ 4 B per present, + 24 B per solid voxel" is entered
with its floor, one of each per found point.  Nothing is asserted about any of these figures.

--ab (repeatable): the same figures of this library and of other builds (FMX_LIB) in
alternating child processes on the same GPU, each child under its own time limit and the run
ended by the first that fails, e.g. one lane per point (make BUILD=build_nl1
OUT=../ab/libfmx_nl1.so EXTRA=-DFMX_NEAREST_LANES=1); the builds must agree on the four class
counts of every case (`lookups` may differ: it is what the variants change).
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
REACHES = (1, 2, 4)
SUBSET = 4096
OUT_BYTES = 1 + 8 + 24 + 8 + 4 + 4  # state, dist2, point, tag, hits, misses: what Context.nearest_voxels asks for
# written down before the first run: at the ray walks' measured ~100 lookups per ns, reach 1 on
# a full scan without an early stop is 27 x 262144 = 7.1 M lookups, some 70 us plus the fields
EXPECTED = dict(case="full_reach1_nolimit", lookups_without_stop=27 * 128 * 2048, lookups_per_ns=100.0, us=70.0)


def timed(ctx, name, reps, call):
    """`reps` calls after one warm-up; the profile id's ms and launches per call, the last result."""
    call()
    ctx.profile_reset()
    for _ in range(reps):
        out = call()
    prof = ctx.profile_read()[name]
    return prof["ms"] / reps, prof["launches"] / reps, out


def figures(ms, n, lookups, found, ratio=False):
    by = n * (16.0 + OUT_BYTES) + lookups * 8.0 + found * ((8.0 if ratio else 4.0) + 24.0)
    return dict(us_per_call=round(ms * 1e3, 2), lookups=int(lookups), lookups_per_ns=round(lookups / (ms * 1e6), 3) if ms > 0 else None,
                lookups_per_point=round(lookups / max(n, 1), 2), model_bytes_floor=by,
                gbs=round(by / (ms * 1e-3) / 1e9, 1) if ms > 0 else None,
                frac_of_hbm_peak=round(by / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 5) if ms > 0 else None)


def case_name(which, reach, limit):
    return f"{which}_reach{reach}_{'limit' if limit else 'nolimit'}"


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
    k = a.scans - 1
    full, T = scans[k], poses[k]
    sets = {"full": full, "subset": full[::max(int(full.shape[0]) // SUBSET, 1)].contiguous()}
    stats = ctx.dense_stats()
    ctx.profile(True)
    out = {"map": dict(scans=a.scans, voxels=stats["voxels"], slots=stats["slots"], carve="margin 1, every ray"),
           "probed_scan": k, "points": {name: int(v.shape[0]) for name, v in sets.items()}, "reps": a.reps, "cases": {}}
    for which, pts in sets.items():
        n = int(pts.shape[0])
        for reach in REACHES:
            for limit in (False, True):
                md = reach * VOXEL_W if limit else None
                ms, la, r = timed(ctx, "dense", a.reps, lambda: ctx.nearest_voxels(pts, T, reach=reach, max_dist=md))
                c = r["counts"]
                d2 = r["dist2"][r["state"] == fmx.PROBE_SOLID]
                out["cases"][case_name(which, reach, limit)] = dict(
                    figures(ms, n, c["lookups"], c["found"]), launches_per_call=la, counts=c, reach=reach, max_dist=md,
                    cube_cells=(2 * reach + 1) ** 3, mean_dist_found=float(np.sqrt(d2).mean()) if len(d2) else None)
    ms, la, r = timed(ctx, "dense", a.reps, lambda: ctx.probe_points(full, T))
    out["probe_points"] = dict(us_per_call=round(ms * 1e3, 2), launches_per_call=la, counts=r["counts"])
    ms, la, r = timed(ctx, "dense", a.reps, lambda: ctx.probe_rays(full, T))
    out["probe_rays"] = dict(us_per_call=round(ms * 1e3, 2), launches_per_call=la, counts=r["counts"],
                             lookups_per_ns=round(r["counts"]["steps"] / (ms * 1e6), 3) if ms > 0 else None)
    e = out["cases"][EXPECTED["case"]]
    out["expectation"] = dict(EXPECTED, measured_us=e["us_per_call"], measured_lookups=e["lookups"],
                              measured_lookups_per_ns=e["lookups_per_ns"])
    ctx.profile(False)
    ctx.close()
    return out


def ab(a):
    """This library and other builds in alternating fresh processes on this GPU."""
    libs = {"this": fmx.LIB_PATH}
    for spec in a.ab:
        name, path = spec.split("=", 1)
        libs[name] = os.path.abspath(path)
    names = list(libs)
    runs = {k: [] for k in names}
    for r in range(a.rounds):
        for name in names if r % 2 == 0 else names[::-1]:
            env = dict(os.environ, FMX_LIB=libs[name])
            # (check: a child that fails or runs out of its time ends the whole run)
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--kernels-only", "--scans", str(a.scans), "--reps",
                                  str(a.reps)], env=env, check=True, capture_output=True, text=True, timeout=300)
            runs[name].append(json.loads(res.stdout.strip().splitlines()[-1]))
            print(f"round {r} {name}: full reach 1 {runs[name][-1]['cases']['full_reach1_nolimit']['us_per_call']} us",
                  file=sys.stderr, flush=True)
    out = {"rounds": a.rounds, "this_build": a.ab_this, "other_builds": {k: os.path.basename(libs[k]) for k in names[1:]}}
    first = runs["this"][0]["cases"]
    classes = lambda c: {k: v for k, v in c.items() if k != "lookups"}  # noqa: E731
    for case in first:
        t = {k: [x["cases"][case]["us_per_call"] for x in v] for k, v in runs.items()}
        med = {k: float(np.median(v)) for k, v in t.items()}
        out[case] = {"us_per_call_rounds": t, "us_per_call_median": med,
                     "lookups": {k: v[0]["cases"][case]["lookups"] for k, v in runs.items()},
                     "over_this": {k: round(med[k] / med["this"], 4) for k in names[1:]}}
    out["same_class_counts_all_builds"] = all(classes(x["cases"][c]["counts"]) == classes(first[c]["counts"])
                                              for v in runs.values() for x in v for c in first)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ab", action="append", default=None, metavar="NAME=LIB.so",
                    help="other libfmx builds to compare with, in alternating child processes")
    ap.add_argument("--ab-this", default="FMX_NEAREST_LANES=4 FMX_NEAREST_AHEAD=4 FMX_NEAREST_STOP=1 (the defaults)")
    ap.add_argument("--scans", type=int, default=60)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--kernels-only", action="store_true", help="print the figures, write nothing")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("nearest_cost.py needs a GPU")
    out = {"workload": "c4 (128 x 2048) scans integrated stand-alone with carving, 0.2 m voxels; the last scan's points searched "
                       "at their own pose",
           "hbm_peak_gbs": HBM_PEAK_GBS, "device": torch.cuda.get_device_name(0), "voxel_width": VOXEL_W,
           "max_voxels": MAX_VOXELS}
    out.update(measure(a))
    if a.kernels_only:
        print(json.dumps(out), flush=True)
        return
    if a.ab:
        out["variants_ab"] = ab(a)
    provenance.stamp(out)
    os.makedirs(a.out_dir, exist_ok=True)
    with open(os.path.join(a.out_dir, "nearest_cost.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
