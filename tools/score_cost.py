#!/usr/bin/env python3
"""What scoring many candidate poses of a scan against the dense map costs, measured on one GPU.

  python tools/score_cost.py [--ab NAME=OTHER_LIB.so]   -> profiles/score_cost.json
                                                          (+ profiles/score_order_ab.json with --ab)

The map is tools/align_cost.py's: a stream of C4 (128 x 2048) scans integrated stand-alone at
their poses into one map of 0.2 m voxels (max_voxels 2^25) with carving on, 220 of them here.
The scan is the last integrated one at stride 64, 4096 kept points.  The candidates come from
fmx.pose_grid around the scan's true pose (0.5 m steps in x and y out to 8 m, 2 degree steps
in yaw out to 16 degrees: 18 513 poses), the K nearest the centre taken for K = 1, 64, 1024 and
16384, so K = 1 is the true pose alone.  Two searches: reach 1 with max_dist 0.2 m, and reach 6
with max_dist 1 m.  Per case, medians of --reps repetitions after a warm-up:

  ms per call          a host clock around Context.score_poses, which ends in a stream
                       synchronise, profiling off
  ns per (pose, point) that over K x 4096
  lookups per (pose, point)   from the records
  device time          of the two launches of a call (HIP events around each launch, the
                       "dense" profile id, in repetitions of their own)

The baseline is the capability as it was before fmx_score_poses: K sequential fmx_align_system
calls on the same points and stride (through ctypes with prebuilt arguments, so that the loop
costs as little as Python allows), for K <= 1024, timed in the same process before and after
the batched call.  A case whose single call takes longer than a second is repeated fewer times;
the count used is recorded.

Expectations, written down before the first run (EXPECTED below); each is reported as held or
not held, nothing is asserted:
  1. at K = 1024 the batch takes less time than the 1024 sequential calls;
  2. the device time per lookup of the batch (K = 1024) is no higher than k_nearest's on the same
     4096 points at the true pose and the same search, beyond the run-to-run spread of the two
     that this tool records (max over min of the repetitions);
  3. candidates off the true pose stop later: more lookups per point than at the true pose
     (K = 1); by how much is recorded.

--ab (repeatable): this library and other builds (FMX_LIB) in alternating child processes on
the same GPU, each child under its own time limit and the run ended by the first that fails,
e.g. the pose-major item order (make BUILD=build_pm OUT=../ab/libfmx_pm.so
EXTRA=-DFMX_SCORE_TILE_MAJOR=0); the builds must agree on every record, bit for bit.
"""
import argparse
import ctypes as C
import hashlib
import json
import math
import os
import statistics
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

VOXEL_W = 0.2
MAX_VOXELS = 1 << 25
STRIDE = 64
KS = (1, 64, 1024, 16384)
SEARCHES = (dict(reach=1, max_dist=0.2), dict(reach=6, max_dist=1.0))
GRID = dict(half_xyz=(8.0, 8.0, 0.0), step_xyz=(0.5, 0.5, 1.0), half_yaw=math.radians(16.0), step_yaw=math.radians(2.0))
BASELINE_MAX_K = 1024
SIGMA = 0.1
SLOW_CALL_S = 1.0
# written down before the first run
EXPECTED = {
    "batch_beats_sequential": dict(claim="at K = 1024 one score_poses call takes less time than 1024 sequential "
                                         "fmx_align_system calls on the same points and stride"),
    "cost_per_lookup": dict(claim="device time per lookup at K = 1024 is no higher than k_nearest's on the same points, map "
                                  "and search, beyond the run-to-run spread recorded here"),
    "off_pose_stops_later": dict(claim="candidates off the true pose cost more lookups per point than the true pose alone "
                                       "(K = 1); the ratio is recorded"),
}


def key(search):
    return f"reach{search['reach']}_max{search['max_dist']}"


def candidates(T):
    """The grid's poses, nearest the centre first (ties by grid index): K = 1 is the centre."""
    g = fmx.pose_grid(T, **GRID)
    d = np.linalg.norm(g[:, :, 3] - T[:, 3], axis=1)
    rel = np.einsum("kij,lj->kil", g[:, :, :3], T[:, :3])  # R_k R_c^T = Rz(psi)
    yaw = np.abs(np.arctan2(rel[:, 1, 0], rel[:, 0, 0]))
    order = np.lexsort((np.arange(len(g)), np.round(d * d + (10.0 * yaw) ** 2, 9)))
    assert g[order[0]].tobytes() == np.ascontiguousarray(T).tobytes()
    return np.ascontiguousarray(g[order])


def clocked(reps, call):
    """Wall seconds of each of `reps` calls after one warm-up (fewer when a call is slow)."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = call()
    first = time.perf_counter() - t0
    if first > SLOW_CALL_S:
        reps = max(3, min(reps, int(20.0 / first)))
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = call()
        ts.append(time.perf_counter() - t0)
    return ts, out


def device_ms(ctx, reps, call):
    """The dense id's ms and launches per call, per repetition, profiling on for these alone."""
    ctx.profile(True)
    call()
    ms, la = [], 0.0
    for _ in range(reps):
        ctx.profile_reset()
        call()
        prof = ctx.profile_read()["dense"]
        ms.append(prof["ms"])
        la = prof["launches"]
    ctx.profile(False)
    return ms, la


def sequential(ctx, pts, n, poses, search):
    """K raw fmx_align_system calls, arguments built once: a callable and its (K, 4) counts."""
    L = fmx.lib()
    prm = fmx._AlignParams(1, 0, 0, search["reach"], search["max_dist"] ** 2, SIGMA, STRIDE)
    P = np.ascontiguousarray(poses, np.float64).reshape(-1, 12)
    ptrs = [C.c_void_p(P[k].ctypes.data) for k in range(len(P))]
    out, cnt = np.zeros(29), fmx._AlignCounts()
    po, pp, pc, h, nn = fmx._p(out), C.byref(prm), C.byref(cnt), ctx.h, C.c_size_t(n)
    ptr = C.c_void_p(pts.data_ptr())
    counts = np.zeros((len(P), 4), np.int64)

    def run():
        for k, q in enumerate(ptrs):
            st = L.fmx_align_system(h, ptr, nn, 1, q, pp, po, pc)
            if st:
                raise RuntimeError(f"fmx_align_system: {st}")
            counts[k] = (cnt.found, cnt.none, cnt.out_of_range, cnt.invalid)
        return counts
    return run


def measure(a):
    geo = synth.GEOMETRIES["c4"]
    world = synth.World()
    p = synth.default_params(geo)
    ctx = fmx.Context(fmx.EstimatorParams(extraction=fmx.KeypointExtractionParams(**p)))
    ctx.dense_configure(True, VOXEL_W, MAX_VOXELS)
    ctx.carve_configure(margin=1, ray_stride=1)
    full = T = None
    for k in range(a.scans):  # one scan at a time: the stream is not kept
        full = synth.make_scan("c4", k, device="cuda:0", world=world)[0]
        T = np.asarray(synth.trajectory_pose(k), np.float64).reshape(-1, 4)[:3]
        ctx.dense_integrate(full, T, k)
        if k % 20 == 0:
            print(f"integrated {k + 1} / {a.scans}", file=sys.stderr, flush=True)
    T = np.ascontiguousarray(T)
    n = int(full.shape[0])
    kept = len(range(0, n, STRIDE))
    stats = ctx.dense_stats()
    cands = candidates(T)
    plan = fmx.score_plan(n, STRIDE, max(k for k in KS if k <= a.max_k))
    out = {"map": dict(scans=a.scans, voxels=stats["voxels"], slots=stats["slots"], carve="margin 1, every ray"),
           "scan": a.scans - 1, "points": n, "stride": STRIDE, "kept_points": kept, "reps": a.reps,
           "grid": {k: list(v) if isinstance(v, tuple) else v for k, v in GRID.items()}, "grid_poses": len(cands),
           "plan": plan, "cases": {}, "nearest": {}}
    sub = full[::STRIDE].contiguous()
    digest = hashlib.sha256()
    for search in SEARCHES:
        sk = key(search)
        # the yardstick per lookup: k_nearest on the kept points at the true pose, all outputs
        nms, _ = device_ms(ctx, a.reps, lambda: ctx.nearest_voxels(sub, T, **search))
        near = ctx.nearest_voxels(sub, T, **search)["counts"]
        out["nearest"][sk] = dict(device_us=round(statistics.median(nms) * 1e3, 2),
                                  device_us_min_max=[round(min(nms) * 1e3, 2), round(max(nms) * 1e3, 2)], counts=near,
                                  ns_per_lookup=round(statistics.median(nms) * 1e6 / near["lookups"], 5))
        for K in KS:
            if K > a.max_k:
                continue
            P = cands[:K]
            call = lambda: ctx.score_poses(full, P, stride=STRIDE, **search)  # noqa: E731
            base = None
            if K <= BASELINE_MAX_K:
                seq = sequential(ctx, full, n, P, search)
                before, counts = clocked(a.reps, seq)
                counts = counts.copy()
            ts, got = clocked(a.reps, call)
            if K <= BASELINE_MAX_K:
                after, _ = clocked(a.reps, seq)
                same = bool(all(np.array_equal(got[c], counts[:, i]) for i, c in enumerate(("found", "none", "out_of_range",
                                                                                             "invalid"))))
                base = dict(sequential_ms_before=round(statistics.median(before) * 1e3, 4),
                            sequential_ms_after=round(statistics.median(after) * 1e3, 4),
                            sequential_us_per_call=round(statistics.median(before + after) * 1e6 / K, 3),
                            same_counts_as_sequential=same,
                            batch_over_sequential=round(statistics.median(ts) / statistics.median(before + after), 5))
            dms, launches = device_ms(ctx, min(a.reps, len(ts)), call)
            for f in fmx.SCORE_FIELDS:
                digest.update(got[f].tobytes())
            look = float(got["lookups"].sum())
            med = statistics.median(ts)
            out["cases"][f"{sk}_K{K}"] = dict(
                poses=K, reps_used=len(ts), ms_per_call=round(med * 1e3, 4),
                ms_min_max=[round(min(ts) * 1e3, 4), round(max(ts) * 1e3, 4)],
                ns_per_pose_point=round(med * 1e9 / (K * kept), 4), lookups_per_pose_point=round(look / (K * kept), 3),
                device_ms_two_launches=round(statistics.median(dms), 4),
                device_ms_min_max=[round(min(dms), 4), round(max(dms), 4)], launches_per_call=launches,
                device_ns_per_lookup=round(statistics.median(dms) * 1e6 / look, 5) if look else None,
                found_at_centre=int(got["found"][0]), found_mean=round(float(got["found"].mean()), 2),
                found_best_off_centre=int(got["found"][1:].max()) if K > 1 else None,
                centre_ranks_first=bool(fmx.rank_scores(got)[0] == 0), baseline=base)
            print(f"{sk} K={K}: {med * 1e3:.3f} ms", file=sys.stderr, flush=True)
    out["records_sha256"] = digest.hexdigest()
    # the expectations
    exp = {}
    kmax = max(k for k in KS if k <= min(a.max_k, BASELINE_MAX_K))
    r = {key(s): out["cases"][f"{key(s)}_K{kmax}"]["baseline"]["batch_over_sequential"] for s in SEARCHES}
    exp["batch_beats_sequential"] = dict(EXPECTED["batch_beats_sequential"], at_K=kmax, batch_over_sequential=r,
                                         held=all(v < 1.0 for v in r.values()))
    per = {}
    for s in SEARCHES:
        c, nr = out["cases"][f"{key(s)}_K{kmax}"], out["nearest"][key(s)]
        spread = max(c["device_ms_min_max"][1] / c["device_ms_min_max"][0], nr["device_us_min_max"][1] / nr["device_us_min_max"][0])
        per[key(s)] = dict(score_ns_per_lookup=c["device_ns_per_lookup"], nearest_ns_per_lookup=nr["ns_per_lookup"],
                           spread=round(spread, 4), held=bool(c["device_ns_per_lookup"] <= nr["ns_per_lookup"] * spread))
    exp["cost_per_lookup"] = dict(EXPECTED["cost_per_lookup"], at_K=kmax, measured=per, held=all(v["held"] for v in per.values()))
    off = {}
    for s in SEARCHES:
        on, away = out["cases"][f"{key(s)}_K1"]["lookups_per_pose_point"], out["cases"][f"{key(s)}_K{kmax}"]["lookups_per_pose_point"]
        off[key(s)] = dict(on_pose=on, off_pose=away, ratio=round(away / on, 3) if on else None)
    exp["off_pose_stops_later"] = dict(EXPECTED["off_pose_stops_later"], at_K=kmax, measured=off,
                                       held=all(v["off_pose"] > v["on_pose"] for v in off.values()))
    out["expectations"] = exp
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
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--kernels-only", "--scans", str(a.ab_scans),
                                  "--reps", str(a.reps), "--max-k", "1024"], env=env, check=True, capture_output=True,
                                 text=True, timeout=300)
            runs[name].append(json.loads(res.stdout.strip().splitlines()[-1]))
            print(f"round {r} {name} done", file=sys.stderr, flush=True)
    out = {"rounds": a.rounds, "map_scans": a.ab_scans, "this_build": a.ab_this,
           "other_builds": {k: os.path.basename(libs[k]) for k in names[1:]}, "device": torch.cuda.get_device_name(0)}
    first = runs["this"][0]
    for case in first["cases"]:
        for fig in ("ms_per_call", "device_ms_two_launches"):
            t = {k: [x["cases"][case][fig] for x in v] for k, v in runs.items()}
            med = {k: float(np.median(v)) for k, v in t.items()}
            out.setdefault(case, {})[fig] = {"rounds": t, "median": med,
                                             "over_this": {k: round(med[k] / med["this"], 4) for k in names[1:]}}
    out["same_records_all_builds"] = len({x["records_sha256"] for v in runs.values() for x in v}) == 1
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ab", action="append", default=None, metavar="NAME=LIB.so",
                    help="other libfmx builds to compare with, in alternating child processes")
    ap.add_argument("--ab-this", default="tile-major items (the default)")
    ap.add_argument("--ab-scans", type=int, default=60, help="the map of the --ab children (each builds its own)")
    ap.add_argument("--scans", type=int, default=220)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--max-k", type=int, default=max(KS))
    ap.add_argument("--kernels-only", action="store_true", help="print the figures, write nothing")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("score_cost.py needs a GPU")
    out = {"workload": "c4 (128 x 2048) scans integrated stand-alone with carving, 0.2 m voxels; the last integrated scan at "
                       "stride 64 scored at the K grid poses nearest its own",
           "device": torch.cuda.get_device_name(0), "voxel_width": VOXEL_W, "max_voxels": MAX_VOXELS}
    out.update(measure(a))
    if a.kernels_only:
        print(json.dumps(out), flush=True)
        return
    provenance.stamp(out)
    os.makedirs(a.out_dir, exist_ok=True)
    with open(os.path.join(a.out_dir, "score_cost.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)
    if a.ab:
        order = ab(a)
        provenance.stamp(order)
        with open(os.path.join(a.out_dir, "score_order_ab.json"), "w") as f:
            json.dump(order, f, indent=1)
            f.write("\n")
        print(json.dumps(order), flush=True)


if __name__ == "__main__":
    main()
