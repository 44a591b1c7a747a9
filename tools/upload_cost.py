#!/usr/bin/env python3
"""What loading voxels back into the dense voxel map costs, measured on one GPU.

  python tools/upload_cost.py [--scans 220]   -> profiles/upload_cost.json

The map: tools/dense_cost.py --roll's, a stream of C4 (128 x 2048) scans integrated
stand-alone at their poses into one map of 0.2 m voxels (max_voxels 2^25).  It is downloaded
once; then, with profiling on (HIP events around each launch; the upload's three launches are
the only ones under the "dense" id while they are timed), --reps repetitions each of

  whole_into_empty   the whole download into the cleared table: every entry opens a voxel
  half_back          the voxels a roll about the last pose evicted (about half), put back
                     while the other half is resident
  all_merge          the whole download again into the full table: every entry merges

and, in the same process on the same box, the yardstick: k_roll_reinsert of the kept half, as
tools/dense_cost.py takes it (a roll with half outside less a roll with everything outside).
Per case: the device time of the three launches together (the profile keeps one sum per id),
the wall time of the call, which adds the owner numbering on the host, the host-to-device
copies (44 B per entry) and the wait, and both per entry.  Nothing is asserted about any of
these figures.
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from form_amd import fmx, synth  # noqa: E402
import provenance  # noqa: E402

VOXEL_W = 0.2
MAX_VOXELS = 1 << 25


def spread(v):
    return dict(median=round(float(np.median(v)), 3), min=round(float(np.min(v)), 3), max=round(float(np.max(v)), 3))


def measure(a):
    geo = synth.GEOMETRIES["c4"]
    world = synth.World()
    scans = [synth.make_scan("c4", k, device="cuda:0", world=world)[0] for k in range(a.scans)]
    poses = [synth.trajectory_pose(k) for k in range(a.scans)]
    torch.cuda.synchronize()
    ctx = fmx.Context(fmx.EstimatorParams(extraction=fmx.KeypointExtractionParams(**synth.default_params(geo))))
    ctx.dense_configure(True, VOXEL_W, MAX_VOXELS)
    for k in range(a.scans):
        ctx.dense_integrate(scans[k], poses[k], k)
    del scans
    whole = ctx.dense_download()
    voxels = len(whole["hits"])
    centre = np.array(poses[-1])[:3, 3].copy()
    lo, hi = 0, 4096  # the cube about the last pose that evicts closest to half (tools/dense_cost.py's)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if ctx.roll_count(centre, (mid,) * 3)[0] * 2 <= voxels:
            lo = mid
        else:
            hi = mid
    half = (hi,) * 3
    far = centre + 10000.0  # no voxel there

    def rebuild():
        ctx.profile(False)
        ctx.dense_clear()
        ctx.dense_upload(**whole)

    def timed(prepare, call):
        """--reps times: prepare() unprofiled, then call() profiled.  (device us, wall us, launches, last result)."""
        dev, wall, la, out = [], [], 0, None
        for _ in range(a.reps + 1):  # the first one warms up: code objects, buffers
            arg = prepare()
            ctx.profile(True)
            ctx.profile_reset()
            t0 = time.perf_counter()
            out = call(arg)
            wall.append((time.perf_counter() - t0) * 1e6)
            r = ctx.profile_read()["dense"]
            dev.append(r["ms"] * 1e3)
            la = r["launches"]
            ctx.profile(False)
        return dev[1:], wall[1:], la, out

    def case(n, dev, wall, la, counts):
        d, w = spread(dev), spread(wall)
        return dict(entries=n, counts=counts, launches_per_call=la, device_us=d, wall_us=w,
                    device_ns_per_entry=round(d["median"] * 1e3 / max(n, 1), 3),
                    wall_ns_per_entry=round(w["median"] * 1e3 / max(n, 1), 3))

    out = {"map": dict(scans=a.scans, voxels=voxels, slots=ctx.dense_stats()["slots"]), "reps": a.reps,
           "box_half_voxels": hi}

    def empty():
        ctx.profile(False)
        ctx.dense_clear()

    dev, wall, la, c = timed(empty, lambda _: ctx.dense_upload(**whole))
    out["whole_into_empty"] = case(voxels, dev, wall, la, c)

    def evicted_half():
        rebuild()
        return ctx.roll_evict(centre, half)

    got = {}
    dev, wall, la, c = timed(evicted_half, lambda ev: (got.update(n=len(ev["hits"])), ctx.dense_upload(**ev))[1])
    out["half_back"] = case(got["n"], dev, wall, la, c)

    dev, wall, la, c = timed(rebuild, lambda _: ctx.dense_upload(**whole))
    out["all_merge"] = case(voxels, dev, wall, la, c)

    # the yardstick, as tools/dense_cost.py takes it: count + split + reinsert less count + split
    rebuild()
    kept = ctx.roll_count(centre, half)[0]
    d_half, _, l3, _ = timed(rebuild, lambda _: ctx.roll_evict(centre, half, discard=True))
    d_all, _, l2, _ = timed(rebuild, lambda _: ctx.roll_evict(far, (0, 0, 0), discard=True))
    assert (l2, l3) == (2, 3), (l2, l3)
    t = float(np.median(d_half)) - float(np.median(d_all))
    out["roll_reinsert"] = dict(kept=kept, us=round(t, 3), ns_per_voxel=round(t * 1e3 / max(kept, 1), 3),
                                roll_half_outside_us=spread(d_half), roll_everything_outside_us=spread(d_all))
    r = out["roll_reinsert"]["ns_per_voxel"]
    out["device_ns_per_entry_over_reinsert"] = {k: round(out[k]["device_ns_per_entry"] / r, 3) if r > 0 else None
                                                for k in ("whole_into_empty", "half_back", "all_merge")}
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=220)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("upload_cost.py needs a GPU")
    out = {"workload": "c4 (128 x 2048) scans integrated stand-alone, 0.2 m voxels; the map's own download uploaded",
           "device": torch.cuda.get_device_name(0), "voxel_width": VOXEL_W, "max_voxels": MAX_VOXELS}
    out.update(measure(a))
    provenance.stamp(out)
    os.makedirs(a.out_dir, exist_ok=True)
    with open(os.path.join(a.out_dir, "upload_cost.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
