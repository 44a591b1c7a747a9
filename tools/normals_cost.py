#!/usr/bin/env python3
"""What the dense map's normals and the point-to-plane alignment cost, and whether the plane
form contracts where point-to-point does not, measured on one GPU.

  python tools/normals_cost.py   -> profiles/normals_cost.json

The map and the scan are tools/align_cost.py's (its helpers are imported): a stream of C4 (128 x
2048) scans integrated stand-alone at their poses into one map of 0.2 m voxels with carving on,
the last integrated scan at its own pose, and the scan that follows the stream.  With profiling
on (HIP events around each launch; the timed launches are the only ones under the "dense" id),
medians over --reps repetitions after a warm-up.

Three expectations, written down before the first run (EXPECTED below); the outcome is recorded
whichever way it falls, and nothing is asserted:

  1. build        normals_build at reach 1 looks up 27 cells per voxel.  nearest_voxels does
                  24.6 lookups per ns on this map (profiles/nearest_cost.json, 49 B of output
                  per point); the build reads every slot's key, writes 20 B per voxel and runs a
                  Jacobi per voxel with most of its lanes idle: expected within 3 x nearest's
                  time per lookup.
  2. plane_system against align_system on the same points in the same process at strides 1, 4
                  and 16: one row instead of three, 16 B more per found point, the same
                  reduction: expected no slower than align_system beyond its run-to-run spread
                  (two passes of align_system, the larger relative difference of the three
                  strides, and at least 5 %).
  3. contraction  DESIGN.md §Aligning's two scenarios (the integrated scan from 4.4 cm and 7 mrad
                  off; the never-integrated next scan from the same perturbation of its
                  synthetic true pose), plane=True beside plane=False: expected fewer
                  iterations, a last step below 1e-6, and an end no farther from the truth than
                  the 2.2 mm / 0.13 mrad recorded for point-to-point.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from form_amd import fmx, synth  # noqa: E402
import align_cost as AC  # noqa: E402
import provenance  # noqa: E402

NEAREST_LOOKUPS_PER_NS = 24.6  # profiles/nearest_cost.json, full_reach1_nolimit
BUILD = dict(reach=1, max_dist=None, min_support=5, max_flatness=0.1)  # fmx.NORMALS_DEFAULTS
# written down before the first run
EXPECTED = {
    "build": dict(claim="a reach-1 build takes at most 3 x nearest_voxels' time per lookup", times_nearest_per_lookup_at_most=3.0,
                  nearest_lookups_per_ns=NEAREST_LOOKUPS_PER_NS),
    "plane_system": dict(claim="plane_system is no slower than align_system beyond its run-to-run spread",
                         spread_floor=0.05),
    "contraction": dict(claim="plane=True needs fewer iterations than plane=False, its last step is below 1e-6, and it ends "
                              "no farther from the truth than point-to-point's recorded 2.2 mm / 0.13 mrad",
                        translation_m_at_most=2.2e-3, rotation_rad_at_most=0.13e-3),
}


def medians(ctx, reps, call):
    """Per repetition the dense id's ms (one launch each): the median and the spread."""
    call()
    ms = []
    for _ in range(reps):
        ctx.profile_reset()
        out = call()
        prof = ctx.profile_read()["dense"]
        ms.append(prof["ms"] / max(prof["launches"], 1))
    return statistics.median(ms), (min(ms), max(ms)), out


def measure(a):
    geo = synth.GEOMETRIES["c4"]
    world = synth.World()
    scans = [synth.make_scan("c4", k, device="cuda:0", world=world)[0] for k in range(a.scans + 1)]
    poses = [np.asarray(synth.trajectory_pose(k), np.float64).reshape(-1, 4)[:3] for k in range(a.scans + 1)]
    torch.cuda.synchronize()
    ctx = fmx.Context(fmx.EstimatorParams(extraction=fmx.KeypointExtractionParams(**synth.default_params(geo))))
    ctx.dense_configure(True, AC.VOXEL_W, AC.MAX_VOXELS)
    ctx.carve_configure(margin=1, ray_stride=1)
    for k in range(a.scans):
        ctx.dense_integrate(scans[k], poses[k], k)
    k = a.scans - 1
    full, T = scans[k], poses[k]
    stats = ctx.dense_stats()
    ctx.profile(True)
    out = {"map": dict(scans=a.scans, voxels=stats["voxels"], slots=stats["slots"], carve="margin 1, every ray"),
           "scan": k, "points": int(full.shape[0]), "reps": a.reps, "reach": AC.REACH, "max_dist": AC.VOXEL_W,
           "sigma": AC.SIGMA, "build_params": {k_: (v if v is not None else "inf") for k_, v in BUILD.items()}}
    # 1. the build
    ms, (lo, hi), cnt = medians(ctx, a.reps, lambda: ctx.normals_build(**BUILD))
    per_ns = cnt["lookups"] / (ms * 1e6)
    by = stats["slots"] * 8.0 + stats["voxels"] * 56.0 + cnt["lookups"] * 8.0
    e = EXPECTED["build"]
    out["build"] = dict(us=round(ms * 1e3, 2), us_min_max=[round(lo * 1e3, 2), round(hi * 1e3, 2)], counts=cnt,
                        lookups_per_ns=round(per_ns, 3), nearest_lookups_per_ns=NEAREST_LOOKUPS_PER_NS,
                        model_bytes_floor=by, frac_of_hbm_peak=round(by / (ms * 1e-3) / 1e9 / AC.HBM_PEAK_GBS, 5),
                        expectation=dict(e, measured_times_nearest_per_lookup=round(NEAREST_LOOKUPS_PER_NS / per_ns, 3),
                                         holds=bool(NEAREST_LOOKUPS_PER_NS / per_ns <= e["times_nearest_per_lookup_at_most"])))
    ms2, _, cnt2 = medians(ctx, max(a.reps // 4, 3), lambda: ctx.normals_build(**dict(BUILD, reach=2)))
    out["build_reach2"] = dict(us=round(ms2 * 1e3, 2), counts=cnt2, lookups_per_ns=round(cnt2["lookups"] / (ms2 * 1e6), 3))
    ctx.normals_build(**BUILD)
    # 2. plane_system against align_system, the same points, the same process
    out["systems"] = {}
    spread, worst = EXPECTED["plane_system"]["spread_floor"], 0.0
    for stride in AC.STRIDES:
        args = (full, T, AC.REACH, AC.VOXEL_W, AC.SIGMA)
        a1, _, ra = medians(ctx, a.reps, lambda: ctx.align_system(*args, stride=stride))
        pl, (plo, phi), rp = medians(ctx, a.reps, lambda: ctx.plane_system(*args, stride=stride))
        a2, _, _ = medians(ctx, a.reps, lambda: ctx.align_system(*args, stride=stride))
        al = 0.5 * (a1 + a2)
        spread = max(spread, abs(a1 - a2) / al)
        worst = max(worst, pl / al)
        out["systems"][f"stride{stride}"] = dict(
            kept_points=int(full[::stride].shape[0]), align_us=[round(a1 * 1e3, 2), round(a2 * 1e3, 2)],
            plane_us=round(pl * 1e3, 2), plane_us_min_max=[round(plo * 1e3, 2), round(phi * 1e3, 2)],
            plane_over_align=round(pl / al, 4), align_counts=ra[1], plane_counts=rp[1],
            unoriented_share=round(rp[1]["unoriented"] / max(rp[1]["found"] + rp[1]["unoriented"], 1), 4))
    out["systems"]["expectation"] = dict(EXPECTED["plane_system"], align_spread=round(spread, 4),
                                         worst_plane_over_align=round(worst, 4), holds=bool(worst <= 1.0 + spread))
    # 3. the two scenarios of DESIGN.md §Aligning, plane beside point
    out["alignment"] = {}
    e = EXPECTED["contraction"]
    holds = True
    for name, scan, truth in (("integrated_scan", full, T), ("fresh_scan", scans[a.scans], poses[a.scans])):
        guess = AC.compose(truth, AC.expmap(AC.PERTURB))
        rec = dict(guess_error=AC.pose_error(guess, truth))
        for plane in (False, True):
            got = ctx.dense_align(scan, guess, AC.REACH, AC.VOXEL_W, AC.SIGMA, max_iters=30, threshold=1e-6, plane=plane)
            c = got["counts"]
            rec["plane" if plane else "point"] = dict(
                iters=got["iters"], converged=got["converged"], last_step=got["last_step"],
                pose_error=AC.pose_error(got["pose"], truth), counts=c,
                unoriented_share=round(c["unoriented"] / max(c["found"] + c["unoriented"], 1), 4) if plane else None)
        pe = rec["plane"]["pose_error"]
        rec["holds"] = bool(rec["plane"]["iters"] < rec["point"]["iters"] and rec["plane"]["last_step"] < 1e-6 and
                            pe["translation_m"] <= e["translation_m_at_most"] and pe["rotation_rad"] <= e["rotation_rad_at_most"])
        holds = holds and rec["holds"]
        out["alignment"][name] = rec
    out["alignment"]["expectation"] = dict(e, holds=holds)
    ctx.profile(False)
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=60)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("normals_cost.py needs a GPU")
    out = {"workload": "c4 (128 x 2048) scans integrated stand-alone with carving, 0.2 m voxels (tools/align_cost.py's map); "
                       "the normals built, the last integrated scan's systems, both scans aligned with and without plane",
           "hbm_peak_gbs": AC.HBM_PEAK_GBS, "device": torch.cuda.get_device_name(0), "voxel_width": AC.VOXEL_W,
           "max_voxels": AC.MAX_VOXELS}
    out.update(measure(a))
    provenance.stamp(out)
    os.makedirs(a.out_dir, exist_ok=True)
    with open(os.path.join(a.out_dir, "normals_cost.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
