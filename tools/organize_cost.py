#!/usr/bin/env python3
"""What accepting unorganized clouds costs, measured on one GPU in one process.

  python tools/organize_cost.py            -> profiles/organize_cost.json

Kernels: a C4 (128 x 2048) scan as a shuffled cloud (synth.to_cloud: the ~257k returns
of the 262k cells) organized --reps times with profiling on (HIP events around each
launch), with and without sweep fractions: the "organize" profile id holds both launches
(claim, gather) of each call, so the tool reports their mean per launch and their sum per
cloud, against the byte model at the HBM peak.  The per-point deskew (k_deskew_cells) and
the per-column one (k_deskew) are timed the same way on the organized scan, from the
"deskew" id.

Stream: --scans C4 scans registered sequentially (no fmx_next_scan: clouds cannot be
announced) through fmx_register_scan and, as clouds, through fmx_register_cloud, the two
arms interleaved over --rounds rounds on fresh contexts; the median per-scan host time of
each and their ratio.  Scans and clouds are device-resident in both arms.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from form_amd import fmx, synth  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E peak (spec), as bench.py


def new_ctx(geo, organize):
    p = synth.default_params(geo)
    ctx = fmx.Context(fmx.EstimatorParams(extraction=fmx.KeypointExtractionParams(**p)))
    if organize:
        ctx.organize_configure(True)
    return ctx


def dev_cloud(scan, geo, seed):
    xyzw, ring, frac = synth.to_cloud(scan, geo, seed)
    return (torch.from_numpy(xyzw).to("cuda:0"), torch.from_numpy(ring.view(np.int16)).to("cuda:0"),
            torch.from_numpy(frac).to("cuda:0"))


def per_launch(prof):
    la = max(prof["launches"], 1)
    ms, by = prof["ms"] / la, prof["bytes"] / la
    return dict(launches=prof["launches"], us_per_launch=round(ms * 1e3, 3), bytes_per_launch=by,
                gbs=round(by / (ms * 1e-3) / 1e9, 1) if ms > 0 else None,
                frac_of_hbm_peak=round(by / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4) if ms > 0 else None)


def kernels(a, geo, scan):
    ctx = new_ctx(geo, True)
    cloud = dev_cloud(scan, geo, 1)
    out = {"cloud_points": int(cloud[0].shape[0]), "cells": geo.rows * geo.cols}
    for name, args in (("organize_with_fractions", cloud), ("organize_without_fractions", (cloud[0], cloud[1], None))):
        for _ in range(5):  # code objects, buffers
            ctx.organize(*args)
        ctx.profile(True)
        ctx.profile_reset()
        for _ in range(a.reps):
            ctx.organize(*args)
        r = per_launch(ctx.profile_read()["organize"])
        ctx.profile(False)
        r["us_per_cloud_claim_plus_gather"] = round(2 * r["us_per_launch"], 3)
        out[name] = r
    d = torch.from_numpy(np.ascontiguousarray(scan)).to("cuda:0")
    cols = (np.arange(geo.cols, dtype=np.float64) / geo.cols).astype(np.float32)
    frac = torch.from_numpy(np.tile(cols, geo.rows)).to("cuda:0")
    res = torch.empty_like(d)
    xi = np.array([0.004, -0.003, 0.02, 0.3, 0.02, -0.01])
    for name, fn in (("k_deskew", lambda: ctx.deskew(d, xi, out=res)),
                     ("k_deskew_cells", lambda: ctx.deskew_cells(d, frac, xi, out=res))):
        for _ in range(5):
            fn()
        ctx.profile(True)
        ctx.profile_reset()
        for _ in range(a.reps):
            fn()
        out[name] = per_launch(ctx.profile_read()["deskew"])
        ctx.profile(False)
    ctx.close()
    return out


def run_stream(ctx, items, skip, cloud, poses=None):
    marks = []
    for k, it in enumerate(items):
        if k == skip:
            ctx.sync()
            marks.append(time.perf_counter())
        if cloud:
            ctx.register_cloud(*it)
        else:
            ctx.register_scan(it)
        if k >= skip:
            marks.append(time.perf_counter())
        if poses is not None:  # the untimed round only
            poses.append(ctx.current_pose())
    ctx.sync()
    return np.diff(marks)


def stream(a, geo):
    world = synth.World()
    scans = [synth.make_scan("c4", k, device="cuda:0", world=world)[0] for k in range(a.scans)]
    clouds = [dev_cloud(s, geo, 100 + k) for k, s in enumerate(scans)]
    torch.cuda.synchronize()
    # which scans the organizer does not give back bit for bit (a return at negative range,
    # noise larger than the range, lies behind the sensor: its azimuth is off by pi)
    ctx = new_ctx(geo, True)
    differ = [k for k in range(a.scans)
              if not torch.equal(ctx.organize(*clouds[k])[0].view(torch.int32), scans[k].view(torch.int32))]
    ctx.close()
    per = {False: [], True: []}
    poses = {False: [], True: []}
    for r in range(a.rounds + 1):  # round 0 warms both arms up (and records every pose)
        for cloud in (False, True):
            ctx = new_ctx(geo, cloud)
            dt = run_stream(ctx, clouds if cloud else scans, a.skip, cloud, poses[cloud] if r == 0 else None)
            ctx.close()
            if r:
                per[cloud].append(float(np.median(dt)) * 1e3)
    scan_ms, cloud_ms = float(np.median(per[False])), float(np.median(per[True]))
    first = next((k for k in range(a.scans) if not np.array_equal(poses[False][k], poses[True][k])), None)
    return {
        "scans": a.scans, "skipped": a.skip, "rounds": a.rounds,
        "register_scan_ms_median": round(scan_ms, 4), "register_cloud_ms_median": round(cloud_ms, 4),
        "register_scan_ms_rounds": [round(x, 4) for x in per[False]],
        "register_cloud_ms_rounds": [round(x, 4) for x in per[True]],
        "cloud_over_scan": round(cloud_ms / scan_ms, 4),
        "scans_not_organized_back_bit_for_bit": differ, "first_scan_with_another_pose": first,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=120)
    ap.add_argument("--skip", type=int, default=20, help="scans before the timed ones (the window fills)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=200, help="profiled calls per kernel figure")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("organize_cost.py needs a GPU")
    geo = synth.GEOMETRIES["c4"]
    scan = synth.make_scan("c4", 0)[0].numpy()
    out = {"workload": "c4 (128 x 2048), smoothing mode, sequential", "hbm_peak_gbs": HBM_PEAK_GBS,
           "device": torch.cuda.get_device_name(0), "kernels": kernels(a, geo, scan), "stream": stream(a, geo)}
    os.makedirs(a.out_dir, exist_ok=True)
    with open(os.path.join(a.out_dir, "organize_cost.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
