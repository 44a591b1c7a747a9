#!/usr/bin/env python3
"""What the dense voxel map costs, measured on one GPU.

  python tools/dense_cost.py                     -> profiles/dense_cost.json
  python tools/dense_cost.py --ab OTHER_LIB.so   -> profiles/dense_merge_ab.json
  python tools/dense_cost.py --roll --scans 220  -> profiles/roll_cost.json

Kernels: C4 (128 x 2048) scans integrated stand-alone with profiling on (HIP events around
each launch).  The "dense" profile id holds both launches of an integration (claim, fill), so
the tool reports their mean per launch and their sum per scan, against the byte model at the
HBM peak, for three cases: a scan into an empty map (cleared before each one: every voxel is
inserted), the same scan again (every point merges), and a stream of different scans at their
poses into one growing map.  The download's launches are timed the same way: the count pass
alone (the sizing call), and count + compact (the filling call, less one count).

Stream: --scans C4 scans through fmx_register_scan with the map off and on (every scan
integrated), the two arms alternated over --rounds rounds on fresh contexts, once fed one at
a time and once announced through fmx_next_scan; the median per-scan host time of each arm
and their ratio (reported, not asserted).

--roll: the launches of a roll (fmx_roll_evict) on a map of --scans C4 scans, about half of it
evicted, and the register_scan median of the same stream with the map on and rolling off and on
(a 50 m box, a 2 m step, spill kept), the arms alternated round by round in fresh child
processes; the ratio is reported, not asserted.

--ab: the kernel figures of this library and of another build (FMX_LIB) in alternating child
processes on the same GPU, e.g. the FMX_DENSE_MERGE=0 build of densemap.hip (make BUILD=build_plain OUT=../ab/libfmx_plain.so
EXTRA=-DFMX_DENSE_MERGE=0).
"""
import argparse
import ctypes as C
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


def new_ctx(geo, dense):
    p = synth.default_params(geo)
    ctx = fmx.Context(fmx.EstimatorParams(extraction=fmx.KeypointExtractionParams(**p)))
    if dense:
        ctx.dense_configure(True, VOXEL_W, MAX_VOXELS)
    return ctx


def per_launch(prof, per_call):
    la = max(prof["launches"], 1)
    ms, by = prof["ms"] / la, prof["bytes"] / la
    return dict(launches=prof["launches"], us_per_launch=round(ms * 1e3, 3), bytes_per_launch=by,
                us_per_call=round(ms * 1e3 * per_call, 3),
                gbs=round(by / (ms * 1e-3) / 1e9, 1) if ms > 0 else None,
                frac_of_hbm_peak=round(by / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4) if ms > 0 else None)


def kernels(a, geo, scans, poses):
    ctx = new_ctx(geo, True)
    out = {"points": int(scans[0].shape[0]), "voxel_width": VOXEL_W, "max_voxels": MAX_VOXELS,
           "slots": ctx.dense_stats()["slots"]}
    for _ in range(3):  # code objects, buffers
        ctx.dense_integrate(scans[0], poses[0], 0)
    ctx.dense_clear()

    def profiled(fn, reps, before=None):
        ctx.profile(True)
        ctx.profile_reset()
        for k in range(reps):
            if before:
                before()
            fn(k)
        r = ctx.profile_read()["dense"]
        ctx.profile(False)
        return r

    r = per_launch(profiled(lambda k: ctx.dense_integrate(scans[0], poses[0], k), a.reps, ctx.dense_clear), 2)
    out["integrate_into_empty_map"] = r
    ctx.dense_clear()
    out["counts_first_scan"] = ctx.dense_integrate(scans[0], poses[0], 0)
    out["integrate_same_scan_again"] = per_launch(profiled(lambda k: ctx.dense_integrate(scans[0], poses[0], k), a.reps), 2)
    ctx.dense_clear()
    out["integrate_stream_of_scans"] = per_launch(
        profiled(lambda k: ctx.dense_integrate(scans[k], poses[k], k), len(scans)), 2)
    out["voxels_after_stream"] = ctx.dense_stats()["voxels"]
    # the download: the sizing call is one count pass; the filling call counts again and appends
    n = C.c_uint32(0)

    def size_only(_):
        ctx._chk(ctx._L.fmx_dense_download(ctx.h, C.c_uint32(1), None, None, None, None, C.byref(n)))

    size_only(0)
    cnt = per_launch(profiled(size_only, a.reps // 4 + 1), 1)
    hits = np.zeros(n.value, np.uint32)

    def fill_only(_):
        cap = C.c_uint32(n.value)
        ctx._chk(ctx._L.fmx_dense_download(ctx.h, C.c_uint32(1), None, None, None, fmx._p(hits), C.byref(cap)))

    fill_only(0)
    both = profiled(fill_only, a.reps // 4 + 1)
    calls = both["launches"] // 2
    out["download_count_pass"] = cnt
    comp_ms = both["ms"] / calls - cnt["us_per_launch"] * 1e-3
    comp_by = both["bytes"] / calls - cnt["bytes_per_launch"]
    out["download_compact_pass"] = dict(
        launches=calls, us_per_launch=round(comp_ms * 1e3, 3), bytes_per_launch=comp_by,
        gbs=round(comp_by / (comp_ms * 1e-3) / 1e9, 1), frac_of_hbm_peak=round(comp_by / (comp_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
        voxels=int(n.value))
    ctx.close()
    return out


def run_stream(ctx, items, skip, announced, poses=None):
    marks = []
    for k, it in enumerate(items):
        if k == skip:
            ctx.sync()
            marks.append(time.perf_counter())
        if announced and k + 1 < len(items):
            ctx.next_scan(items[k + 1])
        ctx.register_scan(it)
        if k >= skip:
            marks.append(time.perf_counter())
        if poses is not None:  # the untimed round only
            poses.append(ctx.current_pose())
    ctx.sync()
    return np.diff(marks)


def stream(a, geo, scans, announced):
    per = {False: [], True: []}
    poses = {False: [], True: []}
    last = None
    for r in range(a.rounds + 1):  # round 0 warms both arms up (and records every pose)
        for dense in (False, True):
            ctx = new_ctx(geo, dense)
            dt = run_stream(ctx, scans, a.skip, announced, poses[dense] if r == 0 else None)
            if dense:
                last = ctx.dense_stats()
            ctx.close()
            if r:
                per[dense].append(float(np.median(dt)) * 1e3)
    off_ms, on_ms = float(np.median(per[False])), float(np.median(per[True]))
    first = next((k for k in range(len(scans)) if not np.array_equal(poses[False][k], poses[True][k])), None)
    return {
        "scans": len(scans), "skipped": a.skip, "rounds": a.rounds, "announced": announced,
        "map_off_ms_median": round(off_ms, 4), "map_on_ms_median": round(on_ms, 4),
        "map_off_ms_rounds": [round(x, 4) for x in per[False]], "map_on_ms_rounds": [round(x, 4) for x in per[True]],
        "on_over_off": round(on_ms / off_ms, 4), "added_us_per_scan": round((on_ms - off_ms) * 1e3, 2),
        "voxels_after_stream": last["voxels"], "integrations": last["integrations"],
        "first_scan_with_another_pose": first,
    }


def ab(a):
    """This library and another build, kernels only, in alternating fresh processes."""
    libs = {"this": fmx.LIB_PATH, "other": os.path.abspath(a.ab)}
    runs = {"this": [], "other": []}
    for r in range(a.rounds):
        for name in ("this", "other") if r % 2 == 0 else ("other", "this"):
            env = dict(os.environ, FMX_LIB=libs[name])
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--kernels-only", "--reps", str(a.reps),
                                  "--scans", str(a.scans)], env=env, check=True, capture_output=True, text=True, timeout=300)
            runs[name].append(json.loads(res.stdout.strip().splitlines()[-1])["kernels"])
    out = {"workload": "c4 (128 x 2048) stand-alone integrations", "other_build": a.ab_label, "rounds": a.rounds}
    for case in ("integrate_into_empty_map", "integrate_same_scan_again", "integrate_stream_of_scans"):
        t = {k: [x[case]["us_per_call"] for x in v] for k, v in runs.items()}
        out[case] = {"this_us_per_scan_rounds": t["this"], "other_us_per_scan_rounds": t["other"],
                     "this_us_per_scan_median": float(np.median(t["this"])),
                     "other_us_per_scan_median": float(np.median(t["other"])),
                     "other_over_this": round(float(np.median(t["other"])) / float(np.median(t["this"])), 4)}
    out["counts_first_scan"] = runs["this"][0]["counts_first_scan"]
    out["same_counts_both_builds"] = all(x["counts_first_scan"] == out["counts_first_scan"] and
                                         x["voxels_after_stream"] == runs["this"][0]["voxels_after_stream"]
                                         for v in runs.values() for x in v)
    return out


ROLL_BOX_M, ROLL_STEP_M = 50.0, 2.0  # the register path's box half-extent and step in the --roll stream


def roll_kernels(a, geo, scans, poses):
    """The three launches of a roll (all under the "dense" profile id).  The map of the scans
    is rebuilt with profiling off before every roll; the figures come from three kinds of roll:
    nothing outside (the count alone), everything outside (count + split) and about half
    outside (count + split + reinsert).  The split's time is that of the second kind less the
    count (its two walks over the keys do not depend on where a voxel goes), the reinsert's
    the third kind less the second."""
    ctx = new_ctx(geo, True)
    slots = ctx.dense_stats()["slots"]
    full = (1 << 21,) * 3
    centre = np.array(poses[len(scans) - 1])[:3, 3].copy()

    def rebuild():
        ctx.dense_clear()
        for k in range(len(scans)):
            ctx.dense_integrate(scans[k], poses[k], k)

    rebuild()
    voxels = ctx.dense_stats()["voxels"]
    lo, hi = 0, 4096  # the cube about the last pose that evicts closest to half
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if ctx.roll_count(centre, (mid,) * 3)[0] * 2 <= voxels:
            lo = mid
        else:
            hi = mid
    kept, evicted = ctx.roll_count(centre, (hi,) * 3)
    far = centre + 10000.0  # no voxel there
    ctx.roll_evict(centre, (hi,) * 3, discard=True)  # code objects, buffers

    def timed(box_centre, half, reps):
        ms, by, la = [], 0.0, 0
        for _ in range(reps):
            ctx.profile(False)
            rebuild()
            ctx.profile(True)
            ctx.profile_reset()
            ctx.roll_evict(box_centre, half, discard=True)
            r = ctx.profile_read()["dense"]
            ms.append(r["ms"])
            by, la = r["bytes"], r["launches"]
        ctx.profile(False)
        return float(np.median(ms)), by, la

    reps = max(a.reps // 20, 5)
    t_count, b_count, l1 = timed(centre, full, reps)
    t_all, b_all, l2 = timed(far, (0, 0, 0), reps)
    t_half, b_half, l3 = timed(centre, (hi,) * 3, reps)
    assert (l1, l2, l3) == (1, 2, 3), (l1, l2, l3)

    def fig(ms, by):
        return dict(us_per_launch=round(ms * 1e3, 3), bytes_per_launch=by,
                    gbs=round(by / (ms * 1e-3) / 1e9, 1) if ms > 0 else None,
                    frac_of_hbm_peak=round(by / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4) if ms > 0 else None)

    out = {"points": int(scans[0].shape[0]), "voxel_width": VOXEL_W, "max_voxels": MAX_VOXELS, "slots": slots,
           "scans_in_map": len(scans), "voxels": voxels, "box_half_voxels": hi, "kept": kept, "evicted": evicted,
           "rolls_per_figure": reps,
           "count": fig(t_count, b_count),
           "split_everything_evicted": fig(t_all - t_count, b_all - b_count),
           "reinsert": fig(t_half - t_all, 88.0 * kept),
           "roll_nothing_outside_us": round(t_count * 1e3, 3), "roll_everything_outside_us": round(t_all * 1e3, 3),
           "roll_half_outside_us": round(t_half * 1e3, 3), "roll_half_outside_bytes": b_half}
    ctx.close()
    return out


def roll_stream_arm(a, geo, scans, rolling):
    """One fresh process's stream: the dense map on, rolling on or off; per-scan host times."""
    ctx = new_ctx(geo, True)
    if rolling:
        half = int(np.ceil(ROLL_BOX_M / VOXEL_W))
        ctx.roll_configure(True, (half,) * 3, ROLL_STEP_M, True)
    dt, rolled, seen = [], [], 0
    for k, it in enumerate(scans):  # as run_stream, and which scans rolled (asked in both arms)
        if k == a.skip:
            ctx.sync()
        t0 = time.perf_counter()
        ctx.register_scan(it)
        t1 = time.perf_counter()
        r = ctx.roll_stats()["rolls"]
        if k >= a.skip:
            dt.append(t1 - t0)
            rolled.append(r != seen)
        seen = r
    ctx.sync()
    dt, rolled = np.array(dt), np.array(rolled)
    out = dict(rolling=rolling, ms_median=float(np.median(dt)) * 1e3, ms_mean=float(np.mean(dt)) * 1e3,
               ms_max=float(np.max(dt)) * 1e3, ms_median_scans_without_a_roll=float(np.median(dt[~rolled])) * 1e3,
               ms_median_scans_with_a_roll=float(np.median(dt[rolled])) * 1e3 if rolled.any() else None,
               timed_scans_with_a_roll=int(rolled.sum()), ms_scans_with_a_roll=(dt[rolled] * 1e3).round(4).tolist(),
               dense=ctx.dense_stats(), roll=ctx.roll_stats(),
               pose=np.asarray(ctx.current_pose()).reshape(-1).tolist())
    ctx.close()
    return out


def roll_stream(a):
    """The two arms alternated round by round, each run in a fresh child process."""
    runs = {"off": [], "on": []}
    for r in range(a.rounds + 1):  # round 0 is not used
        for arm in ("off", "on") if r % 2 == 0 else ("on", "off"):
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--roll-arm", arm, "--scans", str(a.scans),
                                  "--skip", str(a.skip)], check=True, capture_output=True, text=True, timeout=600)
            if r:
                runs[arm].append(json.loads(res.stdout.strip().splitlines()[-1]))
    off = float(np.median([x["ms_median"] for x in runs["off"]]))
    on = float(np.median([x["ms_median"] for x in runs["on"]]))
    off_mean = float(np.median([x["ms_mean"] for x in runs["off"]]))
    on_mean = float(np.median([x["ms_mean"] for x in runs["on"]]))
    return {"scans": a.scans, "skipped": a.skip, "rounds": a.rounds, "box_half_m": ROLL_BOX_M, "step_m": ROLL_STEP_M,
            "spill": True, "rolling_off_ms_median": round(off, 4), "rolling_on_ms_median": round(on, 4),
            "rolling_off_ms_rounds": [round(x["ms_median"], 4) for x in runs["off"]],
            "rolling_on_ms_rounds": [round(x["ms_median"], 4) for x in runs["on"]],
            "on_over_off": round(on / off, 4),
            "rolling_off_ms_mean": round(off_mean, 4), "rolling_on_ms_mean": round(on_mean, 4),
            "on_over_off_mean": round(on_mean / off_mean, 4),
            "rolling_on_ms_median_scans_without_a_roll_rounds":
                [round(x["ms_median_scans_without_a_roll"], 4) for x in runs["on"]],
            "rolling_on_ms_median_scans_with_a_roll_rounds":
                [round(x["ms_median_scans_with_a_roll"], 4) for x in runs["on"]],
            "timed_scans_with_a_roll": runs["on"][0]["timed_scans_with_a_roll"],
            "rolling_on_ms_scans_with_a_roll_last_round": runs["on"][-1]["ms_scans_with_a_roll"],
            "rolling_on_ms_max_rounds": [round(x["ms_max"], 4) for x in runs["on"]],
            "rolling_off_ms_max_rounds": [round(x["ms_max"], 4) for x in runs["off"]],
            "rolls": runs["on"][0]["roll"], "voxels_after_stream_on": runs["on"][0]["dense"]["voxels"],
            "voxels_after_stream_off": runs["off"][0]["dense"]["voxels"],
            "same_final_pose": all(x["pose"] == runs["off"][0]["pose"] for v in runs.values() for x in v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--roll", action="store_true", help="the cost of rolling the map -> profiles/roll_cost.json")
    ap.add_argument("--roll-arm", choices=["off", "on"], default=None, help="(child of --roll) one stream, one JSON line")
    ap.add_argument("--scans", type=int, default=120)
    ap.add_argument("--skip", type=int, default=20, help="scans before the timed ones (the window fills)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=200, help="profiled calls per kernel figure")
    ap.add_argument("--kernels-only", action="store_true", help="print the kernel figures, write nothing")
    ap.add_argument("--ab", default=None, help="another libfmx build to compare the kernel figures with")
    ap.add_argument("--ab-label", default="FMX_DENSE_MERGE=0 (no in-wave merge of equal adjacent keys)")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dense_cost.py needs a GPU")
    os.makedirs(a.out_dir, exist_ok=True)
    if a.ab:
        out = provenance.stamp(dict(ab(a), device=torch.cuda.get_device_name(0)))
        with open(os.path.join(a.out_dir, "dense_merge_ab.json"), "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
        print(json.dumps(out), flush=True)
        return
    geo = synth.GEOMETRIES["c4"]
    world = synth.World()
    scans = [synth.make_scan("c4", k, device="cuda:0", world=world)[0] for k in range(a.scans)]
    poses = [synth.trajectory_pose(k) for k in range(a.scans)]
    torch.cuda.synchronize()
    if a.roll_arm:
        print(json.dumps(roll_stream_arm(a, geo, scans, a.roll_arm == "on")), flush=True)
        return
    if a.roll:
        out = {"workload": "c4 (128 x 2048), smoothing mode, dense map on", "hbm_peak_gbs": HBM_PEAK_GBS,
               "device": torch.cuda.get_device_name(0), "kernels": roll_kernels(a, geo, scans, poses)}
        if a.kernels_only:
            print(json.dumps(out), flush=True)
            return
        out["stream_sequential"] = roll_stream(a)
        provenance.stamp(out)
        with open(os.path.join(a.out_dir, "roll_cost.json"), "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
        print(json.dumps(out), flush=True)
        return
    out = {"workload": "c4 (128 x 2048), smoothing mode", "hbm_peak_gbs": HBM_PEAK_GBS,
           "device": torch.cuda.get_device_name(0), "kernels": kernels(a, geo, scans, poses)}
    if a.kernels_only:
        print(json.dumps(out), flush=True)
        return
    out["stream_sequential"] = stream(a, geo, scans, False)
    out["stream_announced"] = stream(a, geo, scans, True)
    provenance.stamp(out)
    with open(os.path.join(a.out_dir, "dense_cost.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
