#!/usr/bin/env python3
"""What refining many candidate poses of a scan against the dense map costs, measured on one GPU.

  python tools/refine_cost.py [--ab NAME=OTHER_LIB.so]   -> profiles/refine_cost.json
                                                           (+ profiles/refine_tile_ab.json with --ab)

The recipe, the map and the scan are tools/score_cost.py's: 220 C4 (128 x 2048) scans integrated
stand-alone at their poses into one map of 0.2 m voxels (max_voxels 2^25) with carving on, the
last integrated scan at stride 64 (4096 kept points) and whole (stride 1), reach 1 with max_dist
0.2 m, both row kinds (the plane form against a snapshot built with FORM's defaults).  The
candidates are score_cost's grid poses, the K nearest the scan's own pose.  Per case, medians of
--reps repetitions after a warm-up, a host clock around the call, profiling off.

  1. systems  Context.refine_systems at K = 1, 8, 64, 1024 against K sequential
              fmx_align_system / fmx_plane_system calls on the same points (raw ctypes calls
              with prebuilt arguments), timed in the same process before and after the batched
              call: what the capability cost before.  The ratio, and the ns per (pose, point)
              beside Context.score_poses' on the same inputs: the difference is what the rows
              and the 28-entry reduction cost.
  2. loop     Context.refine_poses from K = 1, 3, 8, 64 starts a few centimetres and
              milliradians off the scan's pose against K sequential fmx_align_dense /
              fmx_plane_align calls from the same starts: wall time, iterations per pose, and
              how far the final poses differ (a measured figure, not a bound).
  3. tile     --ab (repeatable): this library and other builds (FMX_LIB) in alternating child
              processes on the same GPU, each child under its own time limit and the run ended
              by the first that fails, e.g. a 1024-point tile (make BUILD=build_t1024
              OUT=../ab/libfmx_t1024.so EXTRA=-DFMX_REFINE_TILE=1024).  The builds' sums differ in
              order: their counts must agree, their systems to rounding.

Expectations, written down before the first run (EXPECTED below); each is reported as held or
not held, nothing is asserted.
"""
import argparse
import ctypes as C
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
import score_cost  # noqa: E402  (the grid and its ordering)

VOXEL_W = 0.2
MAX_VOXELS = 1 << 25
STRIDES = (64, 1)  # 4096 kept points, and the whole scan
SYSTEM_KS = (1, 8, 64, 1024)
LOOP_KS = (1, 3, 8, 64)
SEARCH = dict(reach=1, max_dist=0.2)
SIGMA = 0.1
LOOP = dict(max_iters=30, threshold=1e-6)
SLOW_CALL_S = 1.0
# written down before the first run
EXPECTED = {
    "batch_beats_sequential": dict(claim="at K = 1024 one refine_systems call takes less time than 1024 sequential "
                                         "fmx_align_system / fmx_plane_system calls, for both row kinds and both strides"),
    "rows_cost_less_than_the_search": dict(claim="at K = 1024 and 4096 kept points refine_systems costs more per (pose, point) "
                                                 "than score_poses on the same inputs, and less than twice as much"),
    "loop_k1_slower_k64_faster": dict(claim="refine_poses at K = 1 is slower than the one fmx_align_dense / fmx_plane_align "
                                            "call (two launches and a copy against one launch and a completion word), and "
                                            "at K = 64 faster than the 64 sequential calls"),
    "loops_agree": dict(claim="the final poses of the batched and the sequential loops differ by less than 1e-6 in every "
                              "entry (the sums' order differs, the iteration is the same)"),
    "tile": dict(claim="with --ab: the 1024-point tile is no slower than the 256-point tile at K = 1024 and 4096 kept "
                       "points (one reduction per 1024 points instead of four); the smaller K are recorded beside it and "
                       "the default is picked from the whole table"),
}


def clocked(reps, call):
    """Wall seconds of each of `reps` calls after one warm-up (fewer when a call is slow)."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = call()
    first = time.perf_counter() - t0
    if first > SLOW_CALL_S:
        reps = max(2, min(reps, int(6.0 / first)))
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = call()
        ts.append(time.perf_counter() - t0)
    return ts, out


def _params(stride):
    return fmx._AlignParams(1, 0, 0, SEARCH["reach"], SEARCH["max_dist"] ** 2, SIGMA, stride)


def sequential_systems(ctx, pts, n, poses, stride, plane):
    """K raw fmx_align_system / fmx_plane_system calls, arguments built once."""
    L = fmx.lib()
    prm = _params(stride)
    P = np.ascontiguousarray(poses, np.float64).reshape(-1, 12)
    ptrs = [C.c_void_p(P[k].ctypes.data) for k in range(len(P))]
    out, cnt = np.zeros(29), (fmx._PlaneCounts() if plane else fmx._AlignCounts())
    call = L.fmx_plane_system if plane else L.fmx_align_system
    po, pp, pc, h, nn = fmx._p(out), C.byref(prm), C.byref(cnt), ctx.h, C.c_size_t(n)
    ptr = C.c_void_p(pts.data_ptr())
    counts = np.zeros((len(P), 5), np.int64)
    systems = np.zeros((len(P), 29))

    def run():
        for k, q in enumerate(ptrs):
            st = call(h, ptr, nn, 1, q, pp, po, pc)
            if st:
                raise RuntimeError(f"sequential system: {st}")
            counts[k] = (cnt.found, cnt.none, cnt.out_of_range, cnt.invalid, cnt.unoriented if plane else 0)
            systems[k] = out
        return counts, systems
    return run


def sequential_loops(ctx, pts, n, starts, stride, plane):
    """K raw fmx_align_dense / fmx_plane_align calls, arguments built once; a singular start
    (FMX_E_STATE) keeps its start and is counted."""
    L = fmx.lib()
    prm = _params(stride)
    P = np.ascontiguousarray(starts, np.float64).reshape(-1, 12)
    ptrs = [C.c_void_p(P[k].ctypes.data) for k in range(len(P))]
    out, res = np.zeros(12), (fmx._PlaneResult() if plane else fmx._AlignResult())
    call = L.fmx_plane_align if plane else L.fmx_align_dense
    po, pp, pr, h, nn = fmx._p(out), C.byref(prm), C.byref(res), ctx.h, C.c_size_t(n)
    ptr = C.c_void_p(pts.data_ptr())
    mi, th = C.c_uint32(LOOP["max_iters"]), C.c_double(LOOP["threshold"])
    poses = np.zeros((len(P), 12))
    iters = np.zeros(len(P), np.int64)

    def run():
        singular = 0
        for k, q in enumerate(ptrs):
            st = call(h, ptr, nn, 1, q, pp, mi, th, po, pr)
            if st == 5:
                singular += 1
                poses[k], iters[k] = P[k], 0
                continue
            if st:
                raise RuntimeError(f"sequential loop: {st}")
            poses[k], iters[k] = out, res.iters
        return poses, iters, singular
    return run


def _exp(xi):
    """Exp of a tangent [w; v] as a 3 x 4 pose (Rodrigues; small-angle series below 1e-8)."""
    w, v = np.asarray(xi[:3], np.float64), np.asarray(xi[3:], np.float64)
    th = float(np.linalg.norm(w))
    W = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if th < 1e-8:
        A, B, Cc = 1.0, 0.5, 1.0 / 6.0
    else:
        A, B, Cc = math.sin(th) / th, (1.0 - math.cos(th)) / th ** 2, (th - math.sin(th)) / th ** 3
    out = np.zeros((3, 4))
    out[:, :3] = np.eye(3) + A * W + B * (W @ W)
    out[:, 3] = (np.eye(3) + B * W + Cc * (W @ W)) @ v
    return out


def starts_around(T, K, seed=17):
    """K starts T Exp(xi), xi up to 5 mrad and 5 cm per axis."""
    g = np.random.default_rng(seed)
    out = []
    for _ in range(K):
        xi = np.concatenate([g.uniform(-5e-3, 5e-3, 3), g.uniform(-0.05, 0.05, 3)])
        out.append(T @ np.vstack([_exp(xi), [0.0, 0.0, 0.0, 1.0]]))
    return np.ascontiguousarray(out)


def med_ms(ts):
    return round(statistics.median(ts) * 1e3, 4)


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
    normals = ctx.normals_build(**fmx.NORMALS_DEFAULTS)
    stats = ctx.dense_stats()
    cands = score_cost.candidates(T)
    out = {"map": dict(scans=a.scans, voxels=stats["voxels"], slots=stats["slots"], carve="margin 1, every ray",
                       normals={k: normals[k] for k in ("oriented", "flat_rejected", "sparse", "filtered")}),
           "scan": a.scans - 1, "points": n, "search": SEARCH, "sigma": SIGMA, "reps": a.reps,
           "plan": {f"stride{s}": fmx.refine_plan(n, s, max(SYSTEM_KS)) for s in STRIDES}, "systems": {}, "loop": {}}
    strides = [s for s in STRIDES if s in a.strides]
    # ---- 1. systems
    for stride in strides:
        kept = len(range(0, n, stride))
        for plane in (False, True):
            form = "plane" if plane else "point"
            for K in SYSTEM_KS:
                if K > a.max_k:
                    continue
                P = cands[:K]
                call = lambda: ctx.refine_systems(full, P, sigma=SIGMA, stride=stride, plane=plane, **SEARCH)  # noqa: E731
                seq = sequential_systems(ctx, full, n, P, stride, plane)
                before, (counts, systems) = clocked(a.reps, seq)
                counts, systems = counts.copy(), systems.copy()
                ts, got = clocked(a.reps, call)
                after, _ = clocked(a.reps, seq)
                sc, _ = clocked(a.reps, lambda: ctx.score_poses(full, P, stride=stride, **SEARCH))
                same = bool(all(np.array_equal(got[c], counts[:, i]) for i, c in
                                enumerate(("found", "none", "out_of_range", "invalid", "unoriented"))))
                scale = np.abs(systems[:, :28]).max(axis=1, keepdims=True) + 1e-300
                off = float((np.abs(got["system"][:, :28] - systems[:, :28]) / scale).max())
                med, base = statistics.median(ts), statistics.median(before + after)
                out["systems"][f"{form}_stride{stride}_K{K}"] = dict(
                    poses=K, kept_points=kept, reps_used=len(ts), ms_per_call=med_ms(ts),
                    ms_min_max=[round(min(ts) * 1e3, 4), round(max(ts) * 1e3, 4)],
                    ns_per_pose_point=round(med * 1e9 / (K * kept), 4),
                    score_ms_per_call=med_ms(sc), score_ns_per_pose_point=round(statistics.median(sc) * 1e9 / (K * kept), 4),
                    refine_over_score=round(med / statistics.median(sc), 4),
                    sequential_ms_before=med_ms(before), sequential_ms_after=med_ms(after),
                    sequential_us_per_call=round(base * 1e6 / K, 3), batch_over_sequential=round(med / base, 5),
                    same_counts_as_sequential=same, systems_off_by_relative=off,
                    found_at_centre=int(got["found"][0]), found_mean=round(float(got["found"].mean()), 2),
                    lookups_per_pose_point=round(float(got["lookups"].sum()) / (K * kept), 3))
                print(f"systems {form} stride {stride} K={K}: {med * 1e3:.3f} ms, sequential {base * 1e3:.3f} ms", file=sys.stderr,
                      flush=True)
    # ---- 2. the loop
    for stride in strides:
        for plane in (False, True):
            form = "plane" if plane else "point"
            for K in LOOP_KS:
                S = starts_around(T, K)
                kw = dict(sigma=SIGMA, stride=stride, plane=plane, **SEARCH, **LOOP)
                seq = sequential_loops(ctx, full, n, S, stride, plane)
                before, (sp, si, ssing) = clocked(a.reps, seq)
                sp, si = sp.copy(), si.copy()
                ts, got = clocked(a.reps, lambda: ctx.refine_poses(full, S, **kw))
                after, _ = clocked(a.reps, seq)
                ok = ~got["singular"]
                med, base = statistics.median(ts), statistics.median(before + after)
                out["loop"][f"{form}_stride{stride}_K{K}"] = dict(
                    poses=K, reps_used=len(ts), ms_per_call=med_ms(ts), sequential_ms_before=med_ms(before),
                    sequential_ms_after=med_ms(after), batch_over_sequential=round(med / base, 5),
                    iters_batched=[int(x) for x in got["iters"]], iters_sequential=[int(x) for x in si],
                    converged=int(got["converged"].sum()), singular_batched=int(got["singular"].sum()), singular_sequential=ssing,
                    final_poses_differ_by=float(np.abs(got["pose"].reshape(-1, 12)[ok] - sp[ok]).max()) if ok.any() else None,
                    final_off_the_scans_pose=float(np.abs(got["pose"][ok] - T).max()) if ok.any() else None)
                print(f"loop {form} stride {stride} K={K}: {med * 1e3:.3f} ms, sequential {base * 1e3:.3f} ms", file=sys.stderr,
                      flush=True)
    # ---- the expectations
    exp = {}
    kmax = max(k for k in SYSTEM_KS if k <= a.max_k)
    r = {k: v["batch_over_sequential"] for k, v in out["systems"].items() if k.endswith(f"_K{kmax}")}
    exp["batch_beats_sequential"] = dict(EXPECTED["batch_beats_sequential"], at_K=kmax, batch_over_sequential=r,
                                         held=all(v < 1.0 for v in r.values()))
    r = {k: v["refine_over_score"] for k, v in out["systems"].items() if k.endswith(f"_stride64_K{kmax}")}
    exp["rows_cost_less_than_the_search"] = dict(EXPECTED["rows_cost_less_than_the_search"], at_K=kmax, refine_over_score=r,
                                                 held=all(1.0 < v < 2.0 for v in r.values()) if r else None)
    r1 = {k: v["batch_over_sequential"] for k, v in out["loop"].items() if k.endswith("_K1")}
    r64 = {k: v["batch_over_sequential"] for k, v in out["loop"].items() if k.endswith("_K64")}
    exp["loop_k1_slower_k64_faster"] = dict(EXPECTED["loop_k1_slower_k64_faster"], K1=r1, K64=r64,
                                            held=all(v > 1.0 for v in r1.values()) and all(v < 1.0 for v in r64.values()))
    d = {k: v["final_poses_differ_by"] for k, v in out["loop"].items()}
    exp["loops_agree"] = dict(EXPECTED["loops_agree"], final_poses_differ_by=d,
                              held=all(v is not None and v < 1e-6 for v in d.values()))
    exp["tile"] = dict(EXPECTED["tile"], held=None, see="profiles/refine_tile_ab.json")
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
                                  "--reps", str(a.reps), "--max-k", "1024", "--strides", *map(str, a.strides)], env=env,
                                 check=True, capture_output=True, text=True, timeout=300)
            runs[name].append(json.loads(res.stdout.strip().splitlines()[-1]))
            print(f"round {r} {name} done", file=sys.stderr, flush=True)
    out = {"rounds": a.rounds, "map_scans": a.ab_scans, "this_build": a.ab_this,
           "other_builds": {k: os.path.basename(libs[k]) for k in names[1:]}, "device": torch.cuda.get_device_name(0),
           "tiles": {k: v[0]["plan"]["stride64"]["tile"] for k, v in runs.items()}}
    first = runs["this"][0]
    for part, fig in (("systems", "ms_per_call"), ("loop", "ms_per_call")):
        for case in first[part]:
            t = {k: [x[part][case][fig] for x in v] for k, v in runs.items()}
            med = {k: float(np.median(v)) for k, v in t.items()}
            out.setdefault(part, {})[case] = {"rounds": t, "median": med,
                                              "over_this": {k: round(med[k] / med["this"], 4) for k in names[1:]}}
    out["same_counts_as_sequential_all_builds"] = all(c["same_counts_as_sequential"] for v in runs.values() for x in v
                                                      for c in x["systems"].values())
    out["systems_off_by_relative_max"] = max(c["systems_off_by_relative"] for v in runs.values() for x in v
                                             for c in x["systems"].values())
    by_tile = {t: k for k, t in out["tiles"].items()}
    if 256 in by_tile and 1024 in by_tile:
        r = {}
        for form in ("point", "plane"):
            med = out["systems"].get(f"{form}_stride64_K1024", {}).get("median")
            if med:
                r[form] = round(med[by_tile[1024]] / med[by_tile[256]], 4)
        out["expectation"] = dict(EXPECTED["tile"], tile1024_over_tile256=r, held=all(v <= 1.0 for v in r.values()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ab", action="append", default=None, metavar="NAME=LIB.so",
                    help="other libfmx builds to compare with, in alternating child processes")
    ap.add_argument("--ab-this", default="FMX_REFINE_TILE=256 (the default)")
    ap.add_argument("--ab-scans", type=int, default=60, help="the map of the --ab children (each builds its own)")
    ap.add_argument("--ab-only", action="store_true", help="skip the main measurement")
    ap.add_argument("--scans", type=int, default=220)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--max-k", type=int, default=max(SYSTEM_KS))
    ap.add_argument("--strides", type=int, nargs="*", default=list(STRIDES))
    ap.add_argument("--kernels-only", action="store_true", help="print the figures, write nothing")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("refine_cost.py needs a GPU")
    os.makedirs(a.out_dir, exist_ok=True)
    if not a.ab_only:
        out = {"workload": "c4 (128 x 2048) scans integrated stand-alone with carving, 0.2 m voxels; the last integrated scan "
                           "at stride 64 and whole, refined at the K grid poses nearest its own",
               "device": torch.cuda.get_device_name(0), "voxel_width": VOXEL_W, "max_voxels": MAX_VOXELS}
        out.update(measure(a))
        if a.kernels_only:
            print(json.dumps(out), flush=True)
            return
        provenance.stamp(out)
        with open(os.path.join(a.out_dir, "refine_cost.json"), "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
        print(json.dumps(out["expectations"]), flush=True)
    if a.ab:
        tile = ab(a)
        provenance.stamp(tile)
        with open(os.path.join(a.out_dir, "refine_tile_ab.json"), "w") as f:
            json.dump(tile, f, indent=1)
            f.write("\n")
        print(json.dumps(tile.get("expectation")), flush=True)


if __name__ == "__main__":
    main()
