#!/usr/bin/env python3
"""What scan deskewing costs and what it buys, measured on one GPU in one process.

  python tools/deskew_cost.py            -> profiles/deskew_cost.json
  python tools/deskew_cost.py --ate      -> profiles/deskew_ate.json

Cost: C4 (128 x 2048) skewed streams of --scans scans registered with deskewing off and
on, interleaved over --rounds rounds (pipelined, as bench.py's default line, and
sequential), the median
per-scan host time of each, and the deskew kernel's own time from a profiled pass (HIP
events around each launch) against its 32 B / point byte model at the HBM peak.  The
streams are the same skewed scans in both arms, so the arms differ in the deskew step and
in whatever the ICP loop makes of a compensated scan (its iteration counts are recorded).

ATE (--ate): tests/test_gpu_deskew.py::test_deskew_improves_ate's inputs (C2, 30 skewed
scans, ground truth the mid-sweep poses) on the GPU path and on the CPU oracle, raw and
deskewed.  The oracle's deskewed arm registers the scans fmx_deskew gives with the twists
of its OWN two previous poses (the initial twist for scans 0 and 1), i.e. it closes the
loop itself, as the GPU path does.
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
sys.path.insert(0, os.path.join(ROOT, "oracle"))

from form_amd import fmx, metrics, synth  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E peak (spec), as bench.py


def new_ctx(geo, deskew, xi0):
    p = synth.default_params(geo)
    ctx = fmx.Context(fmx.EstimatorParams(extraction=fmx.KeypointExtractionParams(**p)))
    if deskew:
        ctx.deskew_configure(True, initial_twist=xi0)
    return ctx


def run_stream(ctx, scans, skip, pipeline=True, stats=False):
    """Registration of the stream (pipelined: each scan announced one call ahead); per-scan host times (s) after `skip` scans
    and, with stats (untimed rounds), the ICP iterations of each of those scans."""
    marks, icp = [], []
    for k in range(len(scans)):
        if k == skip:
            ctx.sync()
            marks.append(time.perf_counter())
        if pipeline and k + 1 < len(scans):
            ctx.next_scan(scans[k + 1])
        ctx.register_scan(scans[k])
        if k >= skip:
            marks.append(time.perf_counter())
            if stats:
                icp.append(ctx.last_stats()["icp_iters"])
    ctx.sync()
    return np.diff(marks), icp


def gt_twist(O, k):
    T0, T1 = synth.trajectory_pose(k), synth.trajectory_pose(k + 1)
    inv = np.zeros((3, 4))
    inv[:, :3] = T0[:, :3].T
    inv[:, 3] = -T0[:, :3].T @ T0[:, 3]
    return O.logmap(O.compose(inv, T1))


def cost(a):
    import oracle_py as O
    geo = synth.GEOMETRIES["c4"]
    world = synth.World()
    scans = [synth.make_scan_skewed("c4", k, device="cuda:0", world=world)[0] for k in range(a.scans)]
    torch.cuda.synchronize()
    xi0 = gt_twist(O, 0)
    arms = [(pipe, on) for pipe in (True, False) for on in (False, True)]
    per = {arm: [] for arm in arms}
    icp = {}
    for r in range(a.rounds + 1):  # round 0 warms every arm up (code objects, buffers)
        for pipe, on in arms:
            ctx = new_ctx(geo, on, xi0)
            dt, it = run_stream(ctx, scans, a.skip, pipeline=pipe, stats=(r == 0))
            ctx.close()
            if r:
                per[(pipe, on)].append(float(np.median(dt)) * 1e3)
            elif pipe:
                icp[on] = round(float(np.mean(it)), 3)
    # profiled pass, deskew on, sequential (every launch on the context stream)
    ctx = new_ctx(geo, True, xi0)
    for k in range(a.skip):
        ctx.register_scan(scans[k])
    ctx.profile(True)
    ctx.profile_reset()
    for k in range(a.skip, a.scans):
        ctx.register_scan(scans[k])
    prof = ctx.profile_read()["deskew"]
    ctx.profile(False)
    ctx.close()
    ms = prof["ms"] / max(prof["launches"], 1)
    by = prof["bytes"] / max(prof["launches"], 1)
    out = {
        "workload": "c4 skewed stream, smoothing mode, pipelined", "scans": a.scans, "skipped": a.skip,
        "rounds": a.rounds,
        "scan_ms_median_off": round(float(np.median(per[(True, False)])), 4),
        "scan_ms_median_on": round(float(np.median(per[(True, True)])), 4),
        "scan_ms_rounds_off": [round(x, 4) for x in per[(True, False)]],
        "scan_ms_rounds_on": [round(x, 4) for x in per[(True, True)]],
        # every scan extracted inside its own register_scan (no fmx_next_scan): what is left
        # of the difference here is the deskew step itself
        "sequential_scan_ms_median_off": round(float(np.median(per[(False, False)])), 4),
        "sequential_scan_ms_median_on": round(float(np.median(per[(False, True)])), 4),
        "sequential_scan_ms_rounds_off": [round(x, 4) for x in per[(False, False)]],
        "sequential_scan_ms_rounds_on": [round(x, 4) for x in per[(False, True)]],
        "icp_iters_mean_off": icp[False], "icp_iters_mean_on": icp[True],
        "deskew_kernel_ms_per_launch": round(ms, 5), "deskew_launches": prof["launches"],
        "deskew_bytes_per_launch": by,
        "deskew_gbs": round(by / (ms * 1e-3) / 1e9, 1) if ms > 0 else None,
        "deskew_frac_of_hbm_peak": round(by / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4) if ms > 0 else None,
        "hbm_peak_gbs": HBM_PEAK_GBS,
        "device": torch.cuda.get_device_name(0),
    }
    return "deskew_cost.json", out


def ate(a):
    import oracle_py as O
    n = 30
    geo = synth.GEOMETRIES["c2"]
    world = synth.World()
    scans = [synth.make_scan_skewed("c2", k, device="cuda:0", world=world)[0] for k in range(n)]
    host = [s.cpu().numpy() for s in scans]
    gt = [synth.trajectory_pose(k + 0.5) for k in range(n)]
    xi0 = gt_twist(O, 0)
    out = {"workload": "c2, 30 skewed scans, ground truth trajectory_pose(k + 0.5)", "unit": "mm"}
    for on in (False, True):
        ctx = new_ctx(geo, on, xi0)
        est = []
        for k in range(n):
            ctx.register_scan(scans[k])
            est.append(ctx.current_pose())
        out["gpu_deskew_on" if on else "gpu_raw"] = round(metrics.ate_rmse(est, gt) * 1e3, 3)
        ctx.close()
    tool = new_ctx(geo, False, xi0)  # fmx_deskew as a stand-alone kernel
    prm = O.default_params(synth.default_params(geo))
    for on in (False, True):
        oest = O.Estimator(prm)
        est = []
        for k in range(n):
            s = host[k]
            if on:
                xi = xi0
                if k >= 2:
                    inv = np.zeros((3, 4))
                    inv[:, :3] = est[k - 2][:, :3].T
                    inv[:, 3] = -est[k - 2][:, :3].T @ est[k - 2][:, 3]
                    xi = O.logmap(O.compose(inv, est[k - 1]))
                s = tool.deskew(s, xi)
            est.append(oest.register_scan(s)[0].copy())
        out["oracle_deskew_on" if on else "oracle_raw"] = round(metrics.ate_rmse(est, gt) * 1e3, 3)
    out["gpu_ratio"] = round(out["gpu_deskew_on"] / out["gpu_raw"], 4)
    out["oracle_ratio"] = round(out["oracle_deskew_on"] / out["oracle_raw"], 4)
    return "deskew_ate.json", out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ate", action="store_true")
    ap.add_argument("--scans", type=int, default=120)
    ap.add_argument("--skip", type=int, default=20, help="scans before the timed ones (the window fills)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("deskew_cost.py needs a GPU")
    name, out = ate(a) if a.ate else cost(a)
    os.makedirs(a.out_dir, exist_ok=True)
    with open(os.path.join(a.out_dir, name), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
