"""Context teardown (fmx_destroy): closing a context right behind its last call, with the
announced next scan's work still in flight, and repeated create / use / close cycles
giving their device memory back.  Tiny geometry (16 x 256), smoothing mode; ordinary use
throughout."""
import functools

import numpy as np
import pytest
import torch

from form_amd import synth

pytestmark = pytest.mark.gpu

N = 3  # scans registered; scan N is only ever announced
VARIANTS = ["device", "pageable_host", "device_deskew"]


def _ctx(fmx, deskew=False):
    p = synth.default_params(synth.GEOMETRIES["tiny"])
    ctx = fmx.Context(fmx.EstimatorParams(extraction=fmx.KeypointExtractionParams(**p)))
    if deskew:
        ctx.deskew_configure(True)
    return ctx


@functools.lru_cache(maxsize=None)
def _host_scans():
    world = synth.World()
    out = []
    for k in range(N + 1):
        s = synth.make_scan("tiny", k, world=world)[0].numpy().copy()
        s.setflags(write=False)
        out.append(s)
    return out


def _scans(variant):
    if variant == "pageable_host":
        return [np.array(s) for s in _host_scans()]
    return [torch.from_numpy(np.array(s)).to("cuda:0") for s in _host_scans()]


@functools.lru_cache(maxsize=None)
def _oracle_poses():
    """The oracle's poses of the three registered scans as they are (no deskewing)."""
    import oracle_py
    p = synth.default_params(synth.GEOMETRIES["tiny"])
    oest = oracle_py.Estimator(oracle_py.default_params(p))
    out = []
    for s in _host_scans()[:N]:
        T = np.array(oest.register_scan(np.array(s))[0])
        T.setflags(write=False)
        out.append(T)
    return out


def _announce_and_register(ctx, scans, after=None):
    """Announce scan k + 1, register scan k, k = 0..N-1; no sync().  The last announcement
    (scan N, never registered) is what is still in flight when the caller closes: its
    extraction queued on the side stream (device), its staging copy by the helper threads
    into the pinned buffer (pageable host), its deskew + extraction launched at the end
    of the last register_scan (deskewing)."""
    for k in range(N):
        ctx.next_scan(scans[k + 1])
        ctx.register_scan(scans[k])
        if after:
            after(k)


@pytest.mark.parametrize("variant", VARIANTS)
def test_close_with_work_in_flight(fmx_mod, oracle, variant):
    """close() at once behind the last register_scan, the announced fourth scan's work in
    flight: the destructor has to wait for every stream and stop the staging helpers
    before anything is freed.  A fresh context, used the same way, then matches the oracle
    to 1e-6 on the three registered scans.  With deskewing the oracle is fed the scans that
    the context's own fmx_deskew gives with the twists it reports: that checks the
    registration after a teardown, not the deskewing (tests/test_gpu_deskew.py does)."""
    deskew = variant == "device_deskew"
    scans = _scans(variant)
    ctx = _ctx(fmx_mod, deskew)
    _announce_and_register(ctx, scans)
    ctx.close()
    assert ctx.h is None
    ctx.close()  # closing twice is a no-op

    fresh = _ctx(fmx_mod, deskew)
    oest = None
    if deskew:
        p = synth.default_params(synth.GEOMETRIES["tiny"])
        oest = oracle.Estimator(oracle.default_params(p))

    def check(k):
        assert fresh.last_stats()["pipelined"] == (1 if k > 0 else 0)
        if deskew:
            xi, src = fresh.deskew_last()
            assert src == (1 if k < 2 else 2)
            To = oest.register_scan(fresh.deskew(scans[k], xi).cpu().numpy())[0]
        else:
            To = _oracle_poses()[k]
        d = np.abs(fresh.current_pose() - To).max()
        print(f"{variant} scan {k}: |pose - oracle| max {d:.3e}")
        assert d < 1e-6, k

    _announce_and_register(fresh, scans, after=check)
    fresh.close()


def test_repeated_cycles_return_device_memory(fmx_mod):
    """16 cycles of create, announce + register three scans, close must not lower the free
    device memory by 2 MiB or more.  The smallest device buffer is 1 << 18 one-byte
    elements = 256 KiB, so one buffer leaked per context costs at least 4 MiB over 16
    cycles; the bound is half of that.  Pinned host memory is not visible to this test:
    what guards it is that the owning buffer types cannot be copied."""
    scans = _scans("device")

    def cycle():
        ctx = _ctx(fmx_mod)
        _announce_and_register(ctx, scans)
        ctx.close()

    cycle()  # warm-up: the runtime's own pools and code objects
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(16):
        cycle()
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info()[0]
    drop = free0 - free1
    print(f"free device memory: {free0} -> {free1} B, drop {drop} B ({drop / 2**20:.3f} MiB)")
    assert drop < 2 * 2**20
