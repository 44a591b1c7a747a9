"""bench.py — scan-to-submap registration throughput on MI355X (driver contract).

  python bench.py [--gpus N] [--steps K] [--warmup W] [--workload c4|c2|c3|c5]
                  [--dump-outputs DIR] [--full]
  (N > 1: launched by torch.distributed.run, one rank per GPU)

A plain run does what the headline figure needs and no more: ray-cast the scans,
prefill, warm up, time the K steps, write the last step's outputs (--dump-outputs) and
print the line.  --full adds every secondary measurement described below (the other
mode and the sequential-extraction line, the profiled pass with its roofline blocks and
counters, concurrent streams, host input, the sharded C5 lines, the C2 / C3 sub-lines,
the CPU baseline and the ATE block); the --no-* switches take single ones out again.

A step = Estimator::register_scan of one synthetic organized scan (form/form.cpp:40-114):
feature extraction, voxel-map build of the window keyscans, the ICP loop (match + LM
whose linearizations and error evaluations run on the GPU) and map insertion.  Scans
are ray-cast on the GPU before the timed region (inputs resident in HBM); --prefill
untimed scans run first so the timed steps see the window in steady state.
Multi-GPU: a 128-beam scan does not shard, so every rank registers
its own independent stream ("replicas", weak scaling); value = all ranks' scans /
max-over-ranks time.  Beside it, `sharded_c5` times the north star's scaling config
on the same ranks: one 2M-point scan registered against a replicated 50M-voxel
submap, its points sharded over the ranks, the normal equations all-reduced over
RCCL each ICP iteration (strong scaling).

Prints ONE JSON line (rank 0) with the contract fields; with --full also `roofline`
(dominant kernel, HIP-event timed), `cpu_baseline` (the C++ oracle on the host cores,
bounded sample of the same stream) and `sharded_c5`.

--dump-outputs DIR: after the timed steps, what the last timed register_scan handed its
caller (Estimator.register_scan's features and current_lidar_estimate's pose) is written
as DIR/pose.npy (3x4 float64), DIR/planar.npy (F x 6 float32: xyz + normal) and
DIR/point.npy (F x 3 float32); --workload c5: DIR/pose.npy (and pose_wholemap.npy), the
pose of the last timed registration.  The scans are seeded, so equal arguments give
equal inputs in every run.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from form_amd import fmx, metrics, synth  # noqa: E402

METRIC = "scans/sec + Mpts/sec scan-to-submap ICP (128-beam); ATE delta vs reference"
HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8.0 TB/s peak (spec)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--workload", default="c4", choices=["c2", "c3", "c4", "c5"])
    ap.add_argument("--full", action="store_true",
                    help="also run the secondary measurements beside the headline (other mode, sequential "
                         "extraction, profiled pass / roofline, concurrent streams, host input, sharded C5, "
                         "C2 / C3 sub-lines, CPU baseline, ATE); a plain run times the headline only")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="write what the last timed step returned to its caller as DIR/<name>.npy (rank 0)")
    ap.add_argument("--c5-side", type=int, default=7071, help="C5 terrain grid side (7071^2 = 50M voxels)")
    ap.add_argument("--c5-queries", type=int, default=2097152, help="C5 query points (2M)")
    ap.add_argument("--prefill", type=int, default=90,
                    help="untimed scans registered before the warmup so the timed region runs with the "
                         "window in steady state (10 recent scans + keyscans), not while it fills")
    ap.add_argument("--c5-dist", default="both", choices=["both", "local", "wholemap"],
                    help="C5 query sets: the 240 m terrain scan, 2M distinct features across the whole map, or both")
    ap.add_argument("--c5-comm", action="store_true",
                    help="attach the RCCL communicator even on one rank (the exchange step's own overhead)")
    ap.add_argument("--c5-steps", type=int, default=5, help="sharded C5 registrations timed beside the C4 line")
    ap.add_argument("--c5-warmup", type=int, default=1)
    ap.add_argument("--no-c5", action="store_true", help="skip the sharded C5 measurement beside the C4 line")
    ap.add_argument("--sub-workloads", default="c2,c3",
                    help="other scan configs timed beside the headline (BASELINE configs 2 and 3), each with "
                         "prefill, roofline and a CPU-baseline sample; '' = skip")
    ap.add_argument("--rehearse-ranks", action="store_true",
                    help="TEST ONLY (tests/test_gpu_bench_ranks.py): run the --gpus N orchestration on a box with "
                         "fewer GPUs — every rank on cuda:0, gloo for the control collectives, the C5 exchange "
                         "as a host all-reduce in place of the RCCL communicator (RCCL refuses two ranks on one "
                         "GPU).  Prints a rehearsal record, never a driver line.")
    ap.add_argument("--no-host-input", action="store_true",
                    help="skip the host_input block (the same stream fed from host memory, as the reference's "
                         "std::vector<PointXYZf> boundary passes it)")
    ap.add_argument("--cpu-sample-s", type=float, default=15.0, help="budget of the CPU-baseline sample")
    ap.add_argument("--profile-steps", type=int, default=None,
                    help="extra steps, after the timed ones, with per-kernel HIP-event timing (roofline); "
                         "default = --steps.  The timed region itself runs without event overhead.")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--streams", default="2,4",
                    help="also time S independent register_scan streams sharing each GPU (one context and one "
                         "host thread each; a serving figure beside the single-stream headline); '' = skip")
    ap.add_argument("--mode", default="smooth", choices=["smooth", "single"],
                    help="ConstraintManager mode: smooth = the reference default (window smoother), "
                         "single = the disable_smoothing ablation (single-pose LM)")
    ap.add_argument("--no-ablation", action="store_true", help="skip the other mode's secondary measurement")
    ap.add_argument("--no-pipeline", action="store_true",
                    help="register without announcing the next scan (fmx_next_scan): each register_scan "
                         "extracts its own scan first instead of during the previous registration")
    ap.add_argument("--no-pin", action="store_true",
                    help="leave the registering thread unpinned (default: bound to the CPU it runs on for the "
                         "GPU measurements, released before the CPU baseline)")
    ap.add_argument("--subdiv", type=int, default=None, help="override voxel_subdivision (device map cells per voxel edge)")
    ap.add_argument("--traffic-json", default=None,
                    help="PMC-derived HBM bytes per launch (tools/pmc_traffic.py output); default "
                         "profiles/traffic_latest.json (c4) or profiles/traffic_<workload>.json")
    return ap.parse_args()


def spawn_ranks(n):
    """--gpus N without a launcher (WORLD_SIZE unset): start N ranks as child processes
    (torch.distributed.run, one per GPU, rendezvous on 127.0.0.1) and exit with their
    status.  Runs before anything touches the GPU (torch.cuda.device_count() does not
    initialise it); N larger than the visible devices is an error, never a smaller run."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__), *sys.argv[1:]]
    sys.exit(subprocess.call(cmd))


_CTRL = {"gloo": False}  # rehearsal: the control collectives run on gloo (CPU tensors)


def dist_setup(n, rehearse=False):
    if "WORLD_SIZE" not in os.environ:
        ndev = torch.cuda.device_count()
        if n > ndev and not rehearse:
            print(f"bench.py: --gpus {n} but {ndev} HIP device(s) visible", file=sys.stderr)
            sys.exit(2)
        if n > 1:
            spawn_ranks(n)
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != n:
        print(f"bench.py: --gpus {n} but WORLD_SIZE={world}", file=sys.stderr)
        sys.exit(2)
    if rehearse:
        local = 0  # every rank on the one GPU
    if world > 1:
        import torch.distributed as dist
        torch.cuda.set_device(local)
        if rehearse:
            dist.init_process_group("gloo")
            _CTRL["gloo"] = True
        else:
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    return rank, world, local


def barrier(world):
    if world > 1:
        import torch.distributed as dist
        dist.barrier()


def _over_ranks(x, world, local, op):
    if world == 1:
        return x
    import torch.distributed as dist
    t = torch.tensor([x], dtype=torch.float64, device="cpu" if _CTRL["gloo"] else f"cuda:{local}")
    dist.all_reduce(t, op=op)
    return float(t.item())


def max_over_ranks(x, world, local):
    import torch.distributed as dist
    return _over_ranks(x, world, local, dist.ReduceOp.MAX)


def sum_over_ranks(x, world, local):
    import torch.distributed as dist
    return _over_ranks(x, world, local, dist.ReduceOp.SUM)


sys.path.insert(0, os.path.join(ROOT, "tools"))
import provenance  # noqa: E402  (source hashes of the committed profiles: tools/provenance.py)


def pmc_traffic(a, name, workload=None, with_source=False):
    """HBM bytes per launch of kernel class `name` from the committed PMC summary of this
    workload (tools/gpu_pmc.sh, tools/gpu_c5pmc.sh), or None; with_source: also
    {file, measured_at (the commit of the measured code, tools/tag_profile.py)}."""
    workload = workload or a.workload
    path = (a.traffic_json if workload == a.workload else None) or os.path.join(
        ROOT, "profiles", "traffic_latest.json" if workload == "c4" else f"traffic_{workload}.json")
    val, src = None, None
    try:
        with open(path) as f:
            tj = json.load(f)
        if tj.get("workload") == workload and name in tj.get("kernels", {}):
            val = tj["kernels"][name]["hbm_bytes_per_launch"]
            src = {"file": os.path.relpath(path, ROOT), "measured_at": tj.get("measured_at"),
                   **provenance.staleness(tj, "kernels")}
    except (OSError, ValueError, KeyError):
        pass
    return (val, src) if with_source else val


def pin_thread(world, local):
    """Bind the calling (registering) thread to one CPU; returns the previous affinity.
    register_scan is a host-GPU latency chain (~15 host<->GPU round trips per scan): a
    thread migrating between cores mid-chain measured up to 12 % slower on some boxes
    (tools/step_times.py), never faster unpinned.  One rank: the CPU it runs on.  Several
    ranks: distinct CPUs from each GPU's NUMA-local list (sysfs local_cpulist)."""
    old = os.sched_getaffinity(0)
    cpu = None
    if world > 1:
        try:
            pr = torch.cuda.get_device_properties(local)
            bdf = f"{pr.pci_domain_id:04x}:{pr.pci_bus_id:02x}:{pr.pci_device_id:02x}.0"
            cpus = []
            for part in open(f"/sys/bus/pci/devices/{bdf}/local_cpulist").read().strip().split(","):
                lo, _, hi = part.partition("-")
                cpus += list(range(int(lo), int(hi or lo) + 1))
            cands = [c for c in cpus if c in old]
            cpu = cands[(4 * local) % len(cands)] if cands else None
        except (OSError, ValueError, AttributeError):
            cpu = None
        if cpu is None:
            return None
    else:
        with open("/proc/thread-self/stat") as f:
            cpu = int(f.read().rsplit(")", 1)[1].split()[36])
    os.sched_setaffinity(0, {cpu})
    return old


def host_info():
    """The host the CPU baseline runs on: logical CPUs, this job's affinity, CPU model."""
    model = "unknown"
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                model = line.split(":", 1)[1].strip()
                break
    except OSError:
        pass
    return {"host_cpus": os.cpu_count(), "affinity_cpus": len(os.sched_getaffinity(0)), "cpu_model": model}


def cpu_threads():
    """The job's CPU share: OMP_NUM_THREADS when the launcher sets it (the GPU box allots
    16 CPUs per GPU, exports 16 and asks worker pools to stay within it: its other CPUs
    belong to other jobs), else every CPU in this process's affinity mask (the
    reference's TBB default: all host cores)."""
    return int(os.environ.get("OMP_NUM_THREADS", "0")) or host_info()["affinity_cpus"]


def cpu_baseline(scans_host, params, budget_s, single, threads):
    """Oracle register_scan on `threads` host threads (a persistent pool at the
    reference's TBB sites) over the first scans of the same stream."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle_py as O  # CPU baseline only (test infrastructure)
    hi = host_info()
    prm = O.default_params(params)
    prm.disable_smoothing = int(single)
    est = O.Estimator(prm, threads)
    times = []
    t_all = time.perf_counter()
    poses = []
    for s in scans_host:
        t0 = time.perf_counter()
        T, _, _ = est.register_scan(s)
        times.append(time.perf_counter() - t0)
        poses.append(T)
        if time.perf_counter() - t_all > budget_s:
            break
    # steady state: skip the first (empty-map) scan when there is more than one
    steady = times[1:] if len(times) > 2 else times
    per = float(np.median(steady))
    return dict(value=1.0 / per, unit="scans/s", cores=threads, kind="port",
                sample=f"oracle register_scan ({'single-pose' if single else 'smoothing'} mode; C++ restatement, "
                       f"a persistent {threads}-thread pool at the reference's TBB sites (normals, match queries) "
                       f"and over the factors of a linearization (GTSAM's TBB-parallel "
                       f"NonlinearFactorGraph::linearize)) over the first "
                       f"{len(times)} scans of the same synthetic stream; median of {len(steady)} steady-state "
                       f"scans = {per * 1e3:.1f} ms/scan",
                ms_per_scan=per * 1e3, **hi), poses


def register(ctx, scans, k, pipeline):
    """register_scan(scans[k]); pipelined: announce scans[k + 1] first, so this call
    extracts it while registering scans[k] (fmx_next_scan)."""
    if pipeline and k + 1 < len(scans):
        ctx.next_scan(scans[k + 1])
    ctx.register_scan(scans[k])


def host_input_block(a, new_ctx, dscans, single, start, steps):
    """The headline stream fed from HOST memory, as the reference's boundary takes it
    (form.hpp:82-83: a host std::vector<PointXYZf>, filled per measurement by
    bindings.cpp:150-159): (a) pageable arrays — staged into pinned memory by libfmx's
    helper threads and DMA'd, sequential and pipelined (fmx_next_scan of the host array);
    (b) the caller assembling each scan in an fmx_scan_buffer (pinned: DMA'd directly),
    sequential and pipelined.  Timed: the fmx calls (the caller's assembly of a scan is
    outside, for the pageable arrays as for the pinned buffers).  Same scans and prefill as the
    headline; the raw 4-MiB H2D copy times are reported beside."""
    hscans = [s.cpu().numpy().copy() for s in dscans[: start + steps + 1]]
    out = {}
    for mode in ("pageable_sequential", "pageable_pipelined", "pinned_sequential", "pinned_pipelined"):
        ctx = new_ctx(single)
        pipe = mode.endswith("pipelined")
        pinned = mode.startswith("pinned")
        bufs = {}

        def get(k):
            if not pinned:
                return hscans[k]
            if k not in bufs:  # the caller's assembly of scan k, straight into pinned memory
                b = ctx.scan_buffer()
                np.copyto(b, hscans[k])
                bufs[k] = b
            return bufs[k]
        for k in range(start - 1):  # prefill from the device copies
            register(ctx, dscans[: start - 1], k, True)
        if pipe:  # as in the headline, the first timed scan's extraction runs before the timed region
            ctx.next_scan(get(start))
        ctx.register_scan(dscans[start - 1])
        ctx.sync()
        # timed: the fmx calls only (a pinned scan's assembly is the caller's own copy, as
        # the pageable arrays' is: bindings.cpp:150-156 builds its vector either way)
        dt = 0.0
        per = []
        for k in range(start, start + steps):
            nxt = get(k + 1) if pipe else None
            cur = get(k)
            t0 = time.perf_counter()
            if pipe:
                ctx.next_scan(nxt)
            ctx.register_scan(cur)
            per.append(time.perf_counter() - t0)
            dt += per[-1]
            bufs.pop(k - 1, None)
        t0 = time.perf_counter()
        ctx.sync()
        dt += time.perf_counter() - t0
        out[mode] = {"scans_per_s": round(steps / dt, 3), "ms_per_step": round(dt / steps * 1e3, 3),
                     "ms_per_step_p50": round(float(np.median(per)) * 1e3, 3),
                     "pipelined_scans": ctx.last_stats()["pipelined"]}
        ctx.close()
    # raw copies of one scan (median of 10): what the staging has to hide
    dst = torch.empty_like(dscans[0])
    pin = torch.empty(dscans[0].shape, dtype=torch.float32).pin_memory()
    times = {}
    for name, fn in (("pageable_h2d_us", lambda h: dst.copy_(torch.from_numpy(h))),
                     ("pinned_h2d_us", lambda h: dst.copy_(pin, non_blocking=True))):
        ts = []
        for k in range(12):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(hscans[k])
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        times[name] = round(float(np.median(ts[2:])) * 1e6, 1)
    out["copy_per_scan"] = {**times, "bytes": int(hscans[0].nbytes)}
    return out


def concurrent_streams(S, new_ctx, scans, start, steps, pipeline, single, aff):
    """S independent estimators on this GPU, each registering the same scans [start,
    start + steps) from its own host thread (ctypes drops the GIL inside each fmx
    call), after an untimed prefill of [0, start).  Returns aggregate and per-stream
    scans/s (time = the slowest stream's)."""
    import threading
    ctxs = [new_ctx(single) for _ in range(S)]
    for c in ctxs:
        for k in range(start):
            register(c, scans, k, pipeline)
        c.sync()
    cpus = sorted(aff) if aff else []
    ready = threading.Barrier(S + 1)
    times = [0.0] * S

    def run(i):
        if cpus:
            os.sched_setaffinity(0, {cpus[(4 * i + 1) % len(cpus)]})  # this thread only (Linux)
        ready.wait()
        t0 = time.perf_counter()
        for k in range(start, start + steps):
            register(ctxs[i], scans, k, pipeline)
        ctxs[i].sync()
        times[i] = time.perf_counter() - t0

    th = [threading.Thread(target=run, args=(i,)) for i in range(S)]
    for t in th:
        t.start()
    ready.wait()
    for t in th:
        t.join()
    for c in ctxs:
        c.close()
    tm = max(times)
    return {"streams": S, "scans_per_s": round(S * steps / tm, 3), "per_stream_scans_per_s": round(steps / tm, 3)}


def ate_block(scans_host, oracle_poses, params, k0, device, single, pipeline):
    """ATE of the GPU path and of the CPU oracle path over the same scans against the
    synthetic ground truth (the newer_college ATE is unavailable
    offline).  Untimed; a fresh context replays the sample (from device copies, in the
    bench's pipelined mode)."""
    n = len(oracle_poses)
    ctx = fmx.Context(fmx.EstimatorParams(extraction=fmx.KeypointExtractionParams(**params),
                                          disable_smoothing=single), device=device)
    dscans = [torch.from_numpy(s).to(f"cuda:{device}") for s in scans_host[:n]]
    gpu = []
    for k in range(n):
        register(ctx, dscans, k, pipeline)
        gpu.append(ctx.current_pose())
    gt = [synth.trajectory_pose(k0 + k) for k in range(n)]
    a_gpu, a_cpu = metrics.ate_rmse(gpu, gt), metrics.ate_rmse(oracle_poses, gt)
    return {"gpu_m": round(a_gpu, 6), "cpu_port_m": round(a_cpu, 6), "delta_m": round(a_gpu - a_cpu, 9),
            "max_pose_diff_m": round(float(max(np.abs(np.asarray(g)[:, 3] - np.asarray(o)[:, 3]).max()
                                               for g, o in zip(gpu, oracle_poses))), 9),
            "scans": n, "truth": "synthetic trajectory (synth.trajectory_pose)"}


def c5_setup(a, rank, world, local):
    """The sharded C5 problem on this rank: the replicated 50M-voxel terrain map and an
    RCCL communicator over all ranks (queries: c5_queries)."""
    from form_amd import shard
    w = 0.8
    pos4, nrm4 = shard.terrain_map(a.c5_side, w, synth.SEED, f"cuda:{local}")
    n_map = pos4.shape[0]
    prm = fmx.EstimatorParams(keypoint_pool_capacity=n_map + 1024, voxel_subdivision=a.subdiv or 1)
    ctx = fmx.Context(prm, device=local)
    if world > 1 and a.rehearse_ranks:
        pass  # rehearsal: the exchange is a host all-reduce (c5_register), no communicator
    elif world > 1:  # RCCL communicator of the exchange step (fmx_comm_init)
        import torch.distributed as dist
        uid = [fmx.comm_unique_id() if rank == 0 else None]
        dist.broadcast_object_list(uid, src=0)
        ctx.comm_init(uid[0], world, rank)
    elif a.c5_comm:  # a one-rank communicator: the all-reduce + publish path without peers
        ctx.comm_init(fmx.comm_unique_id(), 1, 0)
    ctx.keypoints_add_device(0, pos4, nrm4)
    I34 = np.hstack([np.eye(3), np.zeros((3, 1))])
    ctx.map_build([0], I34[None], w)
    torch.cuda.synchronize()
    return ctx, pos4, nrm4, n_map, w


def c5_build_line(a, ctx, n_map, w, reps=3):
    """The C5 map build (a9, map.tpp:128-146: the reference's serial to_voxel_map) of the
    50M-record terrain map, `reps` rebuilds with HIP events (profiled: the four build
    kernels as one class), with its roofline against §8(d)'s B_build."""
    I34 = np.hstack([np.eye(3), np.zeros((3, 1))])
    ctx.profile(True)
    ctx.profile_reset()
    for _ in range(reps):
        ctx.map_build([0], I34[None], w)
    ctx.sync()
    prof = ctx.profile_read()
    ctx.profile(False)
    d = prof.get("map_build")
    if not d or not d["launches"]:
        return None
    return {"records": n_map, "builds": int(d["launches"]), "ms_per_build": round(d["ms"] / d["launches"], 4),
            "records_per_s": round(n_map * d["launches"] / (d["ms"] * 1e-3), 1),
            "roofline": roofline(a, "map_build", d, "c5_build")}


C5_DISTS = {
    # a 240 m scan of the terrain (drawn with replacement, grid order): the round-1/2 line
    "local": "2M samples (with replacement) of the terrain within 240 m of the sensor, grid order",
    # 2M distinct features across the whole map, ring/azimuth order
    "wholemap": "2M distinct features drawn across the whole map, 128 range rings in azimuth order",
}


def c5_queries(a, dist_name, pos4, nrm4, rank, world):
    """This rank's contiguous shard of the C5 query set `dist_name` and the true offset."""
    from form_amd import shard
    if dist_name == "local":
        Ttrue = shard.c5_offset()
        q4, n4 = shard.make_queries(pos4, nrm4, a.c5_queries, Ttrue, 0.03, synth.SEED + 1)
    else:
        Ttrue = shard.c5_offset(shard.C5_WHOLEMAP_ROT_SCALE)
        q4, n4 = shard.make_queries_wholemap(pos4, nrm4, a.c5_queries, Ttrue, 0.03, synth.SEED + 2)
    b, e = shard.shard_bounds(a.c5_queries, rank, world)
    return q4[b:e].contiguous(), n4[b:e].contiguous(), Ttrue


def c5_register_host_exchange(ctx, w, max_iters=30, thr=1e-4):
    """Rehearsal only: the same ICP loop driven from Python, the shard systems summed by a
    host all-reduce (gloo) instead of libfmx's RCCL exchange."""
    from form_amd import shard
    T = np.hstack([np.eye(3), np.zeros((3, 1))])
    it = 0
    while it < max_iters:
        ctx.match(T, w, counts=False)
        S, e = ctx.linearize_matched(T, 0.1)
        S = shard.allreduce_sum(np.append(S, e))[:28]
        dx = shard.gauss_newton_step(S)
        T = shard.compose(T, shard.expmap(dx))
        it += 1
        if np.linalg.norm(dx) < thr:
            break
    return T, it


def c5_register(ctx, w, max_iters=30, thr=1e-4):
    """One registration of the 2M-point scan: ICP iterations of match
    (this rank's shard) -> the shard's single-pose 7x7 normal equations, all-reduced
    over the ranks on the device (RCCL) -> the identical Gauss-Newton step on every
    rank, from the identity to convergence (form.cpp:83-88's 1e-4 threshold on the
    increment).  The loop runs inside libfmx (fmx_register_points): one fused match +
    linearization launch and one completion-word wait per iteration, no Python in
    between.  Returns (pose, ICP iterations)."""
    return ctx.register_points(np.hstack([np.eye(3), np.zeros((3, 1))]), w, 0.1, max_iters, thr)


def c5_line(a, ctx, dist_name, Ttrue, n_map, w, rank, world, local, steps, warmup, profile):
    """Time `steps` registrations of the current query set (max over ranks)."""
    from form_amd import shard
    reg = c5_register_host_exchange if (world > 1 and a.rehearse_ranks) else c5_register
    for _ in range(warmup):
        T, iters = reg(ctx, w)
    barrier(world)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    it_total = 0
    for _ in range(steps):
        T, iters = reg(ctx, w)
        it_total += iters
    torch.cuda.synchronize()
    barrier(world)
    t_local = time.perf_counter() - t0
    prof, work = {}, {}
    nprof = max(steps // 2, 1)
    if profile:
        ctx.profile(True)
        ctx.profile_reset()
        for _ in range(nprof):
            reg(ctx, w)
        ctx.sync()
        prof = ctx.profile_read()
        work = ctx.profile_match_work()  # every profiled launch's own counters
        ctx.profile(False)
    t_max = max_over_ranks(t_local, world, local)
    if rank != 0:
        return None
    value = steps / t_max
    et, er = shard.pose_error(T, Ttrue)
    e0t, e0r = shard.pose_error(np.hstack([np.eye(3), np.zeros((3, 1))]), Ttrue)
    out = {
        "metric": "C5 registrations/s + Mpts/s (2M-point scan vs 50M-voxel submap, points sharded, RCCL all-reduce)",
        "value": round(value, 3), "unit": "registrations/s (2M-point scans)", "n_gpus": world,
        "steps": steps, "warmup": warmup, "ms_per_step": round(t_max / steps * 1e3, 3), "higher_is_better": True,
        "scaling": "strong",
        "icp_iters_per_registration": round(it_total / steps, 3),
        "icp_iters_per_s": round(it_total / t_max, 3),
        "mpts_per_s": round(value * a.c5_queries / 1e6, 3),
        "config": {"workload": f"c5/{dist_name}: {a.c5_queries} points vs a {n_map}-voxel terrain submap "
                               f"({C5_DISTS[dist_name]}); points sharded contiguously, map replicated; match + "
                               "single-pose 7x7 normal equations fused in one launch, all-reduced (RCCL, device "
                               "buffers, context stream) per ICP iteration", "points_per_scan": a.c5_queries,
                   "query_distribution": dist_name, "parallelism": f"point shards x{world} + all_reduce",
                   "rccl_communicator": world > 1 or bool(a.c5_comm)},
        "pose_error": {"initial_m": round(e0t, 6), "initial_rad": round(e0r, 8), "final_m": round(et, 6),
                       "final_rad": round(er, 8)},
        "pose": np.asarray(T).reshape(-1).tolist(),
    }
    if prof:
        name, d = max(prof.items(), key=lambda kv: kv[1]["ms"])
        out["roofline"] = roofline(a, name, d, "c5" if dist_name == "local" else "c5_wholemap")
        out["kernels_ms_per_step"] = {k: round(v["ms"] / nprof, 4) for k, v in prof.items() if v["ms"] > 0}
        q = sum(v["queries"] for v in work.values())
        out["match_work_per_query"] = {k: round(sum(v[k] for v in work.values()) / max(q, 1.0), 3)
                                       for k in ("probes", "candidates")}
        out["match_work_split"] = match_work_split({k: v for k, v in work.items() if v["launches"]})
    return out


def run_c5(a, rank, world, local, steps, warmup, profile=True, dists=("local", "wholemap")):
    """C5: a 2M-point scan vs a 50M-voxel terrain submap, the scan's
    points sharded over the ranks, the map replicated (built once, both query sets run
    against it).  A step = one registration (c5_register); strong scaling: the total
    work per step is fixed.  Returns {dist: line} on rank 0."""
    ctx, pos4, nrm4, n_map, w = c5_setup(a, rank, world, local)
    out = {}
    if profile and rank == 0:
        out["map_build"] = c5_build_line(a, ctx, n_map, w)
    for dn in dists:
        q4, n4, Ttrue = c5_queries(a, dn, pos4, nrm4, rank, world)
        ctx.set_queries_device(q4, n4)
        torch.cuda.synchronize()
        del q4, n4
        out[dn] = c5_line(a, ctx, dn, Ttrue, n_map, w, rank, world, local, steps, warmup, profile)
    del pos4, nrm4
    ctx.close()
    return out if rank == 0 else None


def sub_stream_line(a, wl, rank, world, local, single, pipe):
    """Another BASELINE scan config (c2: 64x1024 OS1-64, c3: 64x2048 HDL-64E stand-in with
    8 % dropouts) timed like the headline: prefill to the steady state, warmup, `steps`
    timed register_scans (max over ranks), then a profiled pass for the roofline and
    the per-scan counters.  Returns (line or None on ranks > 0, host copies of the
    first scans for the CPU baseline)."""
    dev = f"cuda:{local}"
    geo = synth.GEOMETRIES[wl]
    params = synth.default_params(geo)
    n_pts = geo.rows * geo.cols
    pre, steps, warmup = a.prefill, a.steps, a.warmup
    psteps = max(steps // 2, 5)
    total = pre + warmup + steps + psteps
    world_obj = synth.World()
    k0 = 1000 * rank
    scans = [synth.raycast(world_obj, synth.trajectory_pose(k0 + k), geo, synth.SEED + 7919 * (k0 + k + 1), dev)
             for k in range(total)]
    torch.cuda.synchronize()
    ctx = fmx.Context(fmx.EstimatorParams(extraction=fmx.KeypointExtractionParams(**params),
                                          voxel_subdivision=a.subdiv or 0, disable_smoothing=single), device=local)
    for k in range(pre + warmup):
        register(ctx, scans, k, pipe)
    ctx.sync()
    barrier(world)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    marks = [t0]
    for k in range(pre + warmup, pre + warmup + steps):
        register(ctx, scans, k, pipe)
        marks.append(time.perf_counter())
    ctx.sync()
    torch.cuda.synchronize()
    barrier(world)
    t_local = time.perf_counter() - t0
    ctx.profile(True)
    ctx.profile_reset()
    stats = []
    for k in range(pre + warmup + steps, total):
        register(ctx, scans, k, pipe)
        stats.append(ctx.last_stats())
    ctx.sync()
    prof = ctx.profile_read()
    mwork = ctx.profile_match_work()
    ctx.close()
    t_max = max_over_ranks(t_local, world, local)
    scans_total = sum_over_ranks(float(steps), world, local)
    host = [s.cpu().numpy() for s in scans[:40]] if rank == 0 and world == 1 else None
    del scans
    if rank != 0:
        return None, None
    value = scans_total / t_max
    ms = t_max / steps * 1e3
    name, d = max(prof.items(), key=lambda kv: kv[1]["ms"])
    kern_ms = {k: round(v["ms"] / psteps, 4) for k, v in prof.items() if v["ms"] > 0}
    side = {"map_build"} | ({"extract_rows", "closest", "fit", "compact"} if pipe else set())
    main_ms = sum(v for k, v in kern_ms.items() if k not in side)
    st_mean = {k: float(np.mean([s_[k] for s_ in stats])) for k in stats[0]}
    line = {
        "metric": f"scans/sec + Mpts/sec scan-to-submap ICP ({wl}: {geo.rows}-beam)", "value": round(value, 3),
        "unit": "scans/s", "n_gpus": world, "steps": steps, "warmup": warmup, "ms_per_step": round(ms, 3),
        "higher_is_better": True, "scaling": "weak",
        "config": {"workload": f"{wl}: {geo.rows}x{geo.cols} organized scan stream ({n_pts} pts/scan, "
                               f"{geo.dropout:.0%} dropouts), register_scan, "
                               f"{'single-pose ablation' if single else 'smoothing mode (ConstraintManager default)'}",
                   "points_per_scan": n_pts, "prefill": pre, "timed_scans": [pre + warmup, pre + warmup + steps],
                   "pipelined_extraction": pipe, "parallelism": f"replicas x{world}"},
        "mpts_per_s": round(value * n_pts / 1e6, 3),
        "ms_per_step_p50": round(float(np.median(np.diff(marks))) * 1e3, 3),
        "roofline": roofline(a, name, d, wl),
        "kernels_ms_per_step": kern_ms,
        "main_stream_busy_frac": round(min(main_ms / ms, 1.0), 4),
        "host_round_trips_per_scan": round(st_mean.get("host_waits", 0.0), 2),
        "counters": st_mean,
        "match_work_per_query": match_work_split(mwork),
    }
    return line, (host, params, k0)


# What a launch's algorithmic bytes count: the work the launch
# did, from the kernel's own probe / candidate counters.
ALG_BYTES_MODEL = {
    "match": "per query 16 B read + 45 B result (+32 B planar normal) + warm state 20 B written, 52 B read; "
             "64 B per brick probe, 32 B per candidate record tested (64 B when the map interleaves normals); "
             "a query the warm certificate settles probes and tests nothing (round 4: 87-92 % of warm queries)",
    "match_linearize": "per query 16 B read (+32 B planar normal of the winner unless the map interleaves it "
                       "with the position); 64 B per brick probe; per candidate record its line: 32 B, or 64 B "
                       "interleaved (maps of >= 4M records: C5); 256 B of block partials per block",
    "map_build": "SURVEY.md §8(d) B_build = 2 (32 M_pl + 16 M_pt) + 16 S: the local records read and the "
                 "world-sorted records written at the local size, 16 B per hash slot, S = 2 M (load 0.5)",
    "window": "72 B per plane row (p_i, n_i, p_j as fp64) + 48 B per point pair + 92 doubles of G per pair",
    "moments": "72 B per plane row (p_i, n_i, p_j as fp64) + 48 B per point pair + 2 x 136 doubles of moments "
               "per pair",
}


def match_work_split(mw):
    """fmx_profile_match_work -> per class: launches, and per query probes / candidates /
    certified (the fraction of the class's queries)."""
    out = {}
    for k, v in mw.items():
        q = max(v["queries"], 1.0)
        out[k] = {"launches": int(v["launches"]), "queries_per_launch": round(v["queries"] / max(v["launches"], 1), 1),
                  "probes": round(v["probes"] / q, 3), "candidates": round(v["candidates"] / q, 3),
                  "certified": round(v["certified"] / q, 3), "warm": round(v["warm"] / q, 3)}
    return out


def roofline(a, name, d, workload):
    """The roofline block of the dominant kernel class `name` (profile entry d): the §8(d)
    algorithmic bytes per launch over the HIP-event average launch time (frac), and the
    PMC-measured HBM bytes per launch (traffic, profiles/traffic_<workload>.json) over
    the same time (hbm_frac): what the memory system actually moved."""
    avg_ms = d["ms"] / max(d["launches"], 1)
    bytes_per = d["bytes"] / max(d["launches"], 1)
    achieved = bytes_per / (avg_ms * 1e-3) / 1e9 if avg_ms > 0 else 0.0
    traffic, tsrc = pmc_traffic(a, name, workload, with_source=True)
    roof = dict(bound="hbm", kernel=name, achieved=round(achieved, 3), peak=HBM_PEAK_GBS, unit="GB/s",
                frac=round(achieved / HBM_PEAK_GBS, 6), traffic=traffic, avg_launch_us=round(avg_ms * 1e3, 3),
                alg_bytes_per_launch=bytes_per)
    if name in ALG_BYTES_MODEL:
        roof["alg_bytes_model"] = ALG_BYTES_MODEL[name]
    if tsrc:
        roof["traffic_source"] = tsrc
    if traffic and avg_ms > 0:
        hbm = traffic / (avg_ms * 1e-3) / 1e9
        roof["hbm_achieved"] = round(hbm, 3)
        roof["hbm_frac"] = round(hbm / HBM_PEAK_GBS, 6)
    # where the kernel's waves spend their cycles (SQ wave-state PMC of the same kernel,
    # tools/gpu_sqpmc.sh, committed per workload): far below the HBM roof, the match is
    # a chain of dependent memory rounds with the VALU issue sharing the SIMD
    sq = os.path.join(ROOT, "profiles", f"sq_wavestate_{workload}.json")
    try:
        sqd = json.load(open(sq))
        c = sqd["kernels"][name]["counters_per_launch"]
        wc = max(c["SQ_WAVE_CYCLES"], 1.0)
        roof["wave_cycles"] = dict(valu_active=round(c["SQ_ACTIVE_INST_VALU"] / wc, 3),
                                   memory_wait=round(c["SQ_WAIT_ANY"] / wc, 3),
                                   issue_wait=round(c["SQ_WAIT_INST_ANY"] / wc, 3),
                                   source=os.path.relpath(sq, ROOT),
                                   measured_at=sqd.get("measured_at"), **provenance.staleness(sqd, "kernels"))
    except (OSError, KeyError, ValueError):
        pass
    return roof


def dump_outputs(path, arrays):
    """--dump-outputs: one <name>.npy per output array of the last timed step (float32 or
    float64 as the caller receives them; a few hundred KB in all)."""
    os.makedirs(path, exist_ok=True)
    for name, arr in arrays.items():
        arr = np.ascontiguousarray(arr)
        assert arr.dtype in (np.float32, np.float64), (name, arr.dtype)
        np.save(os.path.join(path, name + ".npy"), arr)


def rehearsal_record(out, a, world):
    """--rehearse-ranks: what the N-rank path produced, marked so no driver takes it for
    a measurement (the ranks shared one GPU)."""
    keep = {k: out[k] for k in ("n_gpus", "steps", "warmup", "scaling") if k in out}
    rec = {"rehearsal": True, "metric": "rehearsal of the --gpus N orchestration on one GPU (not a measurement)",
           "value": None, "ranks": world, **keep, "c4_scans_per_s_all_ranks": out.get("value")}
    for k in ("sharded_c5", "sharded_c5_wholemap"):
        if k in out:
            rec[k] = {"pose": out[k]["pose"], "icp_iters_per_registration": out[k]["icp_iters_per_registration"],
                      "registrations_per_s": out[k]["value"]}
    return rec


def main():
    a = parse()
    rank, world, local = dist_setup(a.gpus, a.rehearse_ranks)
    if a.workload == "c5":
        torch.cuda.set_device(local)
        dists = ("local", "wholemap") if a.c5_dist == "both" else (a.c5_dist,)
        res = run_c5(a, rank, world, local, a.steps, a.warmup, profile=a.full, dists=dists)
        if res is not None:
            out = res[dists[0]]
            if a.dump_outputs:
                dump_outputs(a.dump_outputs, {"pose" if dn == dists[0] else f"pose_{dn}":
                                              np.array(res[dn]["pose"], np.float64).reshape(3, 4) for dn in dists})
            if len(dists) > 1:
                out["wholemap"] = res["wholemap"]
            if res.get("map_build"):
                out["map_build"] = res["map_build"]
            if a.rehearse_ranks:
                out = {"rehearsal": True, "value": None, "ranks": world, "sharded_c5": {"pose": out["pose"]}}
            print(json.dumps(out), flush=True)
        if world > 1:
            import torch.distributed as dist
            dist.destroy_process_group()
        return
    dev = f"cuda:{local}"
    torch.cuda.set_device(local)
    geo = synth.GEOMETRIES[a.workload]
    params = synth.default_params(geo)
    n_pts = geo.rows * geo.cols
    # independent stream per rank (replicas): different trajectory phase
    world_obj = synth.World()
    k0 = 1000 * rank
    full = a.full
    psteps = (a.steps if a.profile_steps is None else a.profile_steps) if full else 0
    pre = a.prefill
    total = pre + a.warmup + a.steps + psteps
    # at least one scan past the timed ones: the last timed register_scan extracts it
    scans = [synth.raycast(world_obj, synth.trajectory_pose(k0 + k), geo, synth.SEED + 7919 * (k0 + k + 1), dev)
             for k in range(max(total, pre + a.warmup + a.steps + 1))]
    torch.cuda.synchronize()
    single = a.mode == "single"

    def new_ctx(single_pose):
        return fmx.Context(fmx.EstimatorParams(extraction=fmx.KeypointExtractionParams(**params),
                                               voxel_subdivision=a.subdiv or 0, disable_smoothing=single_pose),
                           device=local)

    prev_aff = None if a.no_pin else pin_thread(world, local)
    pipe = not a.no_pipeline

    def secondary(single_pose, pipeline):  # another mode over the same scans (untimed by the driver)
        actx = new_ctx(single_pose)
        for k in range(pre + a.warmup):
            register(actx, scans, k, pipeline)
        actx.sync()
        ta = time.perf_counter()
        mk = [ta]
        for k in range(pre + a.warmup, pre + a.warmup + a.steps):
            register(actx, scans, k, pipeline)
            mk.append(time.perf_counter())
        actx.sync()
        ta = time.perf_counter() - ta
        actx.close()
        return {"scans_per_s": round(a.steps / ta, 3), "ms_per_step": round(ta / a.steps * 1e3, 3),
                "ms_per_step_p50": round(float(np.median(np.diff(mk))) * 1e3, 3)}

    ablation = None
    if full and not a.no_ablation:
        ablation = {"mode": "single-pose (disable_smoothing)" if not single else "smoothing (default)",
                    **secondary(not single, pipe)}
    # the same mode with every scan extracted inside its own register_scan (no fmx_next_scan)
    sequential = secondary(single, False) if full and pipe else None
    ctx = new_ctx(single)
    for k in range(pre + a.warmup):
        register(ctx, scans, k, pipe)
    ctx.sync()
    stats = []
    barrier(world)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    marks = [t0]  # per-scan host marks (register_scan returns with the scan's pose)
    for k in range(pre + a.warmup, pre + a.warmup + a.steps):
        register(ctx, scans, k, pipe)
        marks.append(time.perf_counter())
    ctx.sync()
    torch.cuda.synchronize()
    barrier(world)
    t_local = time.perf_counter() - t0
    if a.dump_outputs and rank == 0:
        # what the last timed register_scan returned to its caller (fmx.Estimator): the
        # scan's features, and its pose (current_lidar_estimate)
        feats = ctx.extract_download()
        dump_outputs(a.dump_outputs, {"pose": ctx.current_pose(), "planar": feats["planar"],
                                      "point": feats["point"]})
    prof, mwork = {}, {}
    if full:
        # roofline pass: same stream continued, per-kernel HIP events on the context stream;
        # the per-scan counters (ICP / LM iterations, round trips, ...) are read here too, so
        # the timed loop above runs register_scan alone
        ctx.profile(True)
        ctx.profile_reset()
        for k in range(pre + a.warmup + a.steps, total):
            register(ctx, scans, k, pipe)
            stats.append(ctx.last_stats())
        ctx.sync()
        prof = ctx.profile_read()
        work = ctx.match_work()
        mwork = ctx.profile_match_work()
        ctx.profile(False)
    ctx.close()
    multi = {}
    for S in ([int(x) for x in a.streams.split(",") if x.strip()] if full and world == 1 else []):  # a per-GPU figure
        multi[str(S)] = concurrent_streams(S, new_ctx, scans, pre + a.warmup, a.steps, pipe, single, prev_aff)
    host_in = None
    if full and world == 1 and not a.no_host_input:
        host_in = host_input_block(a, new_ctx, scans, single, pre + a.warmup, a.steps)
    t_max = max_over_ranks(t_local, world, local)
    scans_total = sum_over_ranks(float(a.steps), world, local)
    # the sharded C5 registration beside the replica line: every rank takes part
    c5 = None
    if full and not a.no_c5:  # each C5 line ends with a short profiled pass (its roofline block)
        c5 = run_c5(a, rank, world, local, a.c5_steps, a.c5_warmup, profile=True)
    # BASELINE's other scan configs beside the headline (every rank takes part)
    subs = {}
    host = ([s_.cpu().numpy() for s_ in scans[: min(total, 60)]]
            if full and not a.no_cpu_baseline and world == 1 else None)
    del scans
    for wl in [w_.strip() for w_ in a.sub_workloads.split(",")
               if full and w_.strip() and w_.strip() != a.workload]:
        subs[wl] = sub_stream_line(a, wl, rank, world, local, single, pipe)
    c5_build = None
    if rank == 0 and c5 is not None:
        c5_whole = c5["wholemap"]
        c5_build = c5.get("map_build")
        c5 = c5["local"]
    if rank != 0:
        if world > 1:
            import torch.distributed as dist
            dist.destroy_process_group()
        return
    value = scans_total / t_max
    ms_per_step = t_max / a.steps * 1e3
    out = {
        "metric": METRIC,
        "value": round(value, 3),
        "unit": "scans/s",
        "n_gpus": world,
        "steps": a.steps,
        "warmup": a.warmup,
        "ms_per_step": round(ms_per_step, 3),
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "fp32 points / fp64 map, residuals and normal equations",
        "data": "synthetic (ray-cast organized scans, seed 0x464F524D; no datasets offline)",
        "config": {"workload": f"{a.workload}: {geo.rows}x{geo.cols} organized scan stream ({n_pts} pts/scan), "
                               f"register_scan, {'single-pose ablation (disable_smoothing)' if single else 'smoothing mode (ConstraintManager default)'}",
                   "points_per_scan": n_pts, "parallelism": f"replicas x{world}",
                   "timed_scans": [pre + a.warmup, pre + a.warmup + a.steps],
                   "prefill": pre,
                   # pipelined: each register_scan also extracts the next scan (announced with
                   # fmx_next_scan) on a side stream; the timed region runs as many extractions
                   # as scans (the first timed scan's ran in the warmup, the scan after the last
                   # timed one's runs inside)
                   "pipelined_extraction": pipe},
        "mpts_per_s": round(value * n_pts / 1e6, 3),
        # this rank's median per-scan wall time (host noise shows in the mean, not here)
        "ms_per_step_p50": round(float(np.median(np.diff(marks))) * 1e3, 3),
    }
    if full:  # the profiled pass's figures
        # dominant kernel by device time in the timed region
        name, d = max(prof.items(), key=lambda kv: kv[1]["ms"])
        roof = roofline(a, name, d, a.workload)
        # the runner-up kernel class too (C4: match and the window linearization are within a
        # few % of each other per scan)
        ranked = sorted(prof.items(), key=lambda kv: -kv[1]["ms"])
        roof_next = (roofline(a, ranked[1][0], ranked[1][1], a.workload)
                     if len(ranked) > 1 and ranked[1][1]["ms"] > 0 else None)
        st_mean = {k: float(np.mean([s[k] for s in stats])) for k in stats[0]} if stats else {}
        kern_ms = {k: round(v["ms"] / max(psteps, 1), 4) for k, v in prof.items()}
        kern_sum = sum(kern_ms.values())
        side = {"map_build"} | ({"extract_rows", "closest", "fit", "compact"} if pipe else set())
        main_ms = sum(v for k, v in kern_ms.items() if k not in side)
        out.update({
            "roofline": roof,
            "roofline_next": roof_next,
            "kernels_ms_per_step": kern_ms,
            "profile_steps": psteps,
            # the context (critical-path) stream's kernel time per scan (profile pass, HIP
            # events; its kernels never overlap each other) over the timed wall time per
            # scan; side-stream work (pipelined extraction, map build) is excluded.  The
            # rocprofv3 trace's own figure: profiles/critical_path_c4.json (tools/critical_path.py)
            "main_stream_busy_frac": round(min(main_ms / ms_per_step, 1.0), 4) if ms_per_step > 0 else None,
            "all_streams_kernel_ms_per_step": round(kern_sum, 4),
            "host_round_trips_per_scan": round(st_mean.get("host_waits", 0.0), 2),
            "counters": st_mean,
            # every profiled match launch, each charged its own counters, cold (a scan's first
            # match on its map) and warm (the ICP iterations after it) apart; certified: the
            # warm queries the certificate settled without a search (fmx_match_cert)
            "match_work_per_query": match_work_split(mwork),
        })
    if multi:
        # S independent streams on one GPU (per rank), each its own context, stream and
        # host thread: aggregate scans/s and the per-stream rate.  Not the headline (a
        # single stream's rate bounds one robot's odometry); what one MI355X serves.
        out["concurrent_streams"] = multi
    if ablation is not None:
        out["ablation"] = ablation
    if sequential is not None:
        out["sequential_extraction"] = sequential
    if host_in is not None:
        out["host_input"] = host_in
        out["host_input"]["vs_device"] = {
            "pipelined": round(host_in["pageable_pipelined"]["scans_per_s"] / value, 4),
            "sequential": round(host_in["pageable_sequential"]["scans_per_s"] / sequential["scans_per_s"], 4)
            if sequential else None,
            "pinned_pipelined": round(host_in["pinned_pipelined"]["scans_per_s"] / value, 4),
            "pinned_sequential": round(host_in["pinned_sequential"]["scans_per_s"] / sequential["scans_per_s"], 4)
            if sequential else None}
        # the same ratios from median scan times (robust to the host hiccups that move
        # the means between runs on one box): device median / host-input median
        p50_dev = out.get("ms_per_step_p50")
        p50_seq = sequential.get("ms_per_step_p50") if sequential else None
        out["host_input"]["vs_device_p50"] = {
            "pipelined": round(p50_dev / host_in["pageable_pipelined"]["ms_per_step_p50"], 4) if p50_dev else None,
            "sequential": round(p50_seq / host_in["pageable_sequential"]["ms_per_step_p50"], 4) if p50_seq else None,
            "pinned_pipelined": round(p50_dev / host_in["pinned_pipelined"]["ms_per_step_p50"], 4) if p50_dev else None,
            "pinned_sequential": round(p50_seq / host_in["pinned_sequential"]["ms_per_step_p50"], 4)
            if p50_seq else None}
    if c5 is not None:
        out["sharded_c5"] = c5
        out["sharded_c5_wholemap"] = c5_whole
        if c5_build:
            out["c5_map_build"] = c5_build
    cp = os.path.join(ROOT, "profiles", f"critical_path_{a.workload}.json")
    if full and os.path.exists(cp):  # a committed rocprofv3-trace figure, not measured by this run
        with open(cp) as f:
            out["critical_path_trace"] = json.load(f)
        out["critical_path_trace"]["source"] = os.path.relpath(cp, ROOT)
        out["critical_path_trace"].update(provenance.staleness(out["critical_path_trace"], "all"))
    if prev_aff is not None:
        os.sched_setaffinity(0, prev_aff)  # the CPU baseline's threads use every host core
    if host is not None:
        out["cpu_baseline"], opos = cpu_baseline(host, params, a.cpu_sample_s, single, cpu_threads())
        # one thread over the same scans: the pool's scaling (and a per-core figure)
        one, _ = cpu_baseline(host[:12], params, a.cpu_sample_s / 2, single, 1)
        out["cpu_baseline"]["single_thread"] = {"value": one["value"], "ms_per_scan": one["ms_per_scan"],
                                                "sample": one["sample"]}
        out["ate"] = ate_block(host, opos, params, k0, local, single, pipe)
    for wl, (line, cpu_in) in subs.items():
        if line is None:
            continue
        if cpu_in is not None and cpu_in[0] is not None and not a.no_cpu_baseline:
            sh, sp, sk0 = cpu_in
            line["cpu_baseline"], sop = cpu_baseline(sh, sp, a.cpu_sample_s / 3, single, cpu_threads())
            line["ate"] = ate_block(sh, sop, sp, sk0, local, single, pipe)
        out[wl] = line
    if a.rehearse_ranks:
        out = rehearsal_record(out, a, world)
    print(json.dumps(out), flush=True)
    if world > 1:
        import torch.distributed as dist
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
