#!/usr/bin/env python3
"""What aligning a scan to the dense map costs, and how well it localizes, measured on one GPU.

  python tools/align_cost.py [--ab NAME=OTHER_LIB.so]   -> profiles/align_cost.json
                                                          (+ profiles/align_lanes_ab.json with --ab)

The map and the scan are tools/nearest_cost.py's: a stream of C4 (128 x 2048) scans integrated
stand-alone at their poses into one map of 0.2 m voxels (max_voxels 2^25) with carving on, and
the last integrated scan's points at their own pose.  Then, with profiling on (HIP events around
each launch; the timed launches are the only ones under the "dense" id), --reps repetitions each of

  align_system     the scan at stride 1, 4 and 16: reach 1, max_dist = voxel_width, sigma 0.1
  nearest_voxels   the same points (the scan, every 4th, every 16th point) in the same process
                   with all its outputs: the yardstick
  dense_align      a whole alignment of the scan from a perturbed pose (stride 1 and 4): wall
                   time per call, systems evaluated, the launches' share

and, for accuracy, the scan that FOLLOWS the stream (never integrated) localized from a
perturbed guess against the stream's map: the pose error against the synthetic truth, with
the voxels' representatives being first points and not centroids.

The expectation, written down before the first run: the system costs no more than the nearest
call on the same points (it looks up the same cells and writes 29 doubles where that writes 49 B
per point).  Nothing is asserted about any of these figures; DESIGN.md §Dense map, Aligning
reads them.

--ab (repeatable): this library and other builds (FMX_LIB) in alternating child processes on the
same GPU, each child under its own time limit and the run ended by the first that fails, e.g.
four lanes per point (make BUILD=build_al4 OUT=../ab/libfmx_al4.so EXTRA=-DFMX_ALIGN_LANES=4);
the builds must agree on the class counts and the lookups of every case.
"""
import argparse
import json
import math
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
STRIDES = (1, 4, 16)
REACH, SIGMA = 1, 0.1
NEAREST_OUT_BYTES = 1 + 8 + 24 + 8 + 4 + 4  # what Context.nearest_voxels writes per point
# written down before the first run
EXPECTED = dict(claim="align_system costs no more than nearest_voxels (all outputs) on the same points",
                ratio_at_most=1.0)
PERTURB = (0.004, -0.003, 0.005, 0.03, -0.02, 0.025)  # [w; v], right perturbation of the true pose


def timed(ctx, reps, call):
    """`reps` calls after one warm-up: the dense id's ms and launches per call, the last result."""
    call()
    ctx.profile_reset()
    for _ in range(reps):
        out = call()
    prof = ctx.profile_read()["dense"]
    return prof["ms"] / reps, prof["launches"] / reps, out


def expmap(xi):
    w, v = np.array(xi[:3], np.float64), np.array(xi[3:], np.float64)
    th = float(np.linalg.norm(w))
    W = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-9:
        A, B, Cc = 1.0, 0.5, 1.0 / 6.0
    else:
        A, B, Cc = math.sin(th) / th, (1 - math.cos(th)) / th ** 2, (th - math.sin(th)) / th ** 3
    T = np.zeros((3, 4))
    T[:, :3] = np.eye(3) + A * W + B * (W @ W)
    T[:, 3] = (np.eye(3) + B * W + Cc * (W @ W)) @ v
    return T


def compose(a, b):
    a, b = np.asarray(a, np.float64).reshape(-1, 4)[:3], np.asarray(b, np.float64).reshape(-1, 4)[:3]
    T = np.zeros((3, 4))
    T[:, :3] = a[:, :3] @ b[:, :3]
    T[:, 3] = a[:, :3] @ b[:, 3] + a[:, 3]
    return T


def pose_error(T, truth):
    T, truth = np.asarray(T, np.float64).reshape(-1, 4)[:3], np.asarray(truth, np.float64).reshape(-1, 4)[:3]
    dR = truth[:, :3].T @ T[:, :3]
    ang = math.acos(max(-1.0, min(1.0, (np.trace(dR) - 1.0) / 2.0)))
    return dict(translation_m=float(np.linalg.norm(T[:, 3] - truth[:, 3])), rotation_rad=float(ang))


def measure(a):
    geo = synth.GEOMETRIES["c4"]
    world = synth.World()
    scans = [synth.make_scan("c4", k, device="cuda:0", world=world)[0] for k in range(a.scans + 1)]
    poses = [np.asarray(synth.trajectory_pose(k), np.float64).reshape(-1, 4)[:3] for k in range(a.scans + 1)]
    torch.cuda.synchronize()
    p = synth.default_params(geo)
    ctx = fmx.Context(fmx.EstimatorParams(extraction=fmx.KeypointExtractionParams(**p)))
    ctx.dense_configure(True, VOXEL_W, MAX_VOXELS)
    ctx.carve_configure(margin=1, ray_stride=1)
    for k in range(a.scans):
        ctx.dense_integrate(scans[k], poses[k], k)
    k = a.scans - 1
    full, T = scans[k], poses[k]
    n = int(full.shape[0])
    stats = ctx.dense_stats()
    ctx.profile(True)
    out = {"map": dict(scans=a.scans, voxels=stats["voxels"], slots=stats["slots"], carve="margin 1, every ray"),
           "scan": k, "points": n, "reps": a.reps, "reach": REACH, "max_dist": VOXEL_W, "sigma": SIGMA, "cases": {}}
    for stride in STRIDES:
        sub = full[::stride].contiguous()
        m = int(sub.shape[0])
        ms, la, r = timed(ctx, a.reps, lambda: ctx.align_system(full, T, REACH, VOXEL_W, SIGMA, stride=stride))
        cnt = r[1]
        nms, nla, nr = timed(ctx, a.reps, lambda: ctx.nearest_voxels(sub, T, reach=REACH, max_dist=VOXEL_W))
        blocks = min((m + 255) // 256, 2048)  # at one lane per point; the partials are a bound, not the cost
        by = m * 24.0 + cnt["lookups"] * 8.0 + cnt["found"] * (4.0 + 24.0) + blocks * 2 * 28 * 8.0
        out["cases"][f"stride{stride}"] = dict(
            kept_points=m, align_us=round(ms * 1e3, 2), align_launches_per_call=la, counts=cnt,
            nearest_us=round(nms * 1e3, 2), nearest_launches_per_call=nla, nearest_counts=nr["counts"],
            align_over_nearest=round(ms / nms, 4) if nms > 0 else None,
            lookups_per_ns=round(cnt["lookups"] / (ms * 1e6), 3) if ms > 0 else None, model_bytes_floor=by,
            frac_of_hbm_peak=round(by / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 5) if ms > 0 else None,
            nearest_output_bytes=m * NEAREST_OUT_BYTES, error=float(r[0][28]))
    out["expectation"] = dict(EXPECTED, measured={s: out["cases"][s]["align_over_nearest"] for s in out["cases"]},
                              holds=all(c["align_over_nearest"] <= EXPECTED["ratio_at_most"] for c in out["cases"].values()))
    # a whole alignment from a perturbed pose: the integrated scan (its own points are in the map)
    guess = compose(T, expmap(PERTURB))
    out["dense_align"] = {}
    for stride in (1, 4):
        call = lambda: ctx.dense_align(full, guess, REACH, VOXEL_W, SIGMA, stride=stride, max_iters=30, threshold=1e-6)  # noqa: E731
        call()
        ctx.profile_reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            got = call()
        wall = (time.perf_counter() - t0) / a.reps
        prof = ctx.profile_read()["dense"]
        out["dense_align"][f"stride{stride}"] = dict(
            wall_us_per_call=round(wall * 1e6, 1), iters=got["iters"], converged=got["converged"], last_step=got["last_step"],
            kernel_us_per_call=round(prof["ms"] * 1e3 / a.reps, 2), launches_per_call=prof["launches"] / a.reps,
            wall_us_per_iter=round(wall * 1e6 / max(got["iters"], 1), 1), counts=got["counts"],
            guess_error=pose_error(guess, T), pose_error=pose_error(got["pose"], T),
            note="wall time under profiling (HIP events around each launch)")
    # accuracy: the scan after the stream, never integrated, against first-point representatives
    fresh, truth = scans[a.scans], poses[a.scans]
    fguess = compose(truth, expmap(PERTURB))
    out["accuracy_fresh_scan"] = {}
    for stride in (1, 4):
        got = ctx.dense_align(fresh, fguess, REACH, VOXEL_W, SIGMA, stride=stride, max_iters=30, threshold=1e-6)
        S, cnt = ctx.align_system(fresh, got["pose"], REACH, VOXEL_W, SIGMA, stride=stride)
        valid = cnt["found"] + cnt["none"]
        out["accuracy_fresh_scan"][f"stride{stride}"] = dict(
            scan=a.scans, iters=got["iters"], converged=got["converged"], guess_error=pose_error(fguess, truth),
            pose_error=pose_error(got["pose"], truth), fitness=cnt["found"] / valid if valid else 0.0,
            rmse_m=math.sqrt(2.0 * float(S[28]) * SIGMA * SIGMA / cnt["found"]) if cnt["found"] else 0.0, counts=cnt)
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
            print(f"round {r} {name}: stride 1 {runs[name][-1]['cases']['stride1']['align_us']} us", file=sys.stderr, flush=True)
    out = {"rounds": a.rounds, "this_build": a.ab_this, "other_builds": {k: os.path.basename(libs[k]) for k in names[1:]},
           "device": torch.cuda.get_device_name(0)}
    first = runs["this"][0]
    for case in first["cases"]:
        t = {k: [x["cases"][case]["align_us"] for x in v] for k, v in runs.items()}
        med = {k: float(np.median(v)) for k, v in t.items()}
        out[case] = {"align_us_rounds": t, "align_us_median": med,
                     "nearest_us_rounds": {k: [x["cases"][case]["nearest_us"] for x in v] for k, v in runs.items()},
                     "over_this": {k: round(med[k] / med["this"], 4) for k in names[1:]}}
    for case in first["dense_align"]:
        t = {k: [x["dense_align"][case]["wall_us_per_call"] for x in v] for k, v in runs.items()}
        med = {k: float(np.median(v)) for k, v in t.items()}
        out["dense_align_" + case] = {"wall_us_rounds": t, "wall_us_median": med,
                                      "over_this": {k: round(med[k] / med["this"], 4) for k in names[1:]}}
    out["same_counts_all_builds"] = all(x["cases"][c]["counts"] == first["cases"][c]["counts"]
                                        for v in runs.values() for x in v for c in first["cases"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ab", action="append", default=None, metavar="NAME=LIB.so",
                    help="other libfmx builds to compare with, in alternating child processes")
    ap.add_argument("--ab-this", default="FMX_ALIGN_LANES=1 (the default)")
    ap.add_argument("--scans", type=int, default=60)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--kernels-only", action="store_true", help="print the figures, write nothing")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("align_cost.py needs a GPU")
    out = {"workload": "c4 (128 x 2048) scans integrated stand-alone with carving, 0.2 m voxels; the last integrated scan "
                       "aligned at and near its own pose, the following scan localized",
           "hbm_peak_gbs": HBM_PEAK_GBS, "device": torch.cuda.get_device_name(0), "voxel_width": VOXEL_W,
           "max_voxels": MAX_VOXELS}
    out.update(measure(a))
    if a.kernels_only:
        print(json.dumps(out), flush=True)
        return
    provenance.stamp(out)
    os.makedirs(a.out_dir, exist_ok=True)
    with open(os.path.join(a.out_dir, "align_cost.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)
    if a.ab:
        lanes = ab(a)
        provenance.stamp(lanes)
        with open(os.path.join(a.out_dir, "align_lanes_ab.json"), "w") as f:
            json.dump(lanes, f, indent=1)
            f.write("\n")
        print(json.dumps(lanes), flush=True)


if __name__ == "__main__":
    main()
