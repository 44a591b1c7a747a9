"""The keypoint pool and the window store across compaction and growth, on the device.

Both stores move their contents (fmx_api.cpp: compact_pool; window.hip: win_reserve) only
after minutes of streaming at their production sizes.  FMX_TEST_STORE_LIMITS (read when a
context is created) shrinks them so that short streams reach every such event; the event
counts at the end of Context.last_stats() prove that they did — every test asserts them.

* seam API: random keypoints_add / keypoints_remove / map_insert against the restatement
  (tests/store_ref.py); after every compaction, map_build + match over the live scans is
  bit-exact to oracle.VoxelMap (the comparison of tests/test_gpu_map.py).
* registration streams: a context with tight limits gives, scan by scan, the same pose,
  features, counts and map, bit for bit, as a roomy one, which in turn lies within 1e-6 of
  oracle.Estimator.  All limits are sized from the oracle's per-scan counts of that stream.
"""
import functools

import numpy as np
import pytest

import store_ref as SR
from form_amd import synth

pytestmark = pytest.mark.gpu

I34 = np.hstack([np.eye(3), np.zeros((3, 1))])
OOM = 3
WINDOW = (4, 3)  # max_num_recent_scans, max_num_keyscans: marginalizations start at scan 5
N_SCANS = 40
STORE_KEYS = ("pool_compactions_planar", "pool_compactions_point", "win_compactions", "win_growths_plane",
              "win_growths_point")


def _limits(monkeypatch, pool=0, win_pl=0, win_pt=0):
    if pool or win_pl or win_pt:
        monkeypatch.setenv("FMX_TEST_STORE_LIMITS", f"{int(pool)},{int(win_pl)},{int(win_pt)}")
    else:
        monkeypatch.delenv("FMX_TEST_STORE_LIMITS", raising=False)


def _events(ctx):
    s = ctx.last_stats()
    return {k: s[k] for k in STORE_KEYS}


# ================================================================== seam API: the pool alone
def _planar(g, n, centre):
    xyz = g.uniform(-3, 3, (n, 3)) + centre
    nrm = g.normal(size=(n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return np.ascontiguousarray(np.hstack([xyz, nrm]), np.float32)


def _point(g, n, centre):
    return np.ascontiguousarray(g.uniform(-3, 3, (n, 3)) + centre, np.float32)


def _check_live(ctx, oracle, refs, feats, poses, qpl, qpt, qid, w=0.8, max_dist=0.8):
    """map_build + match over the restatement's live scans against oracle.VoxelMap: accepted
    set, scan, d^2, p_i, n_i and per-pair counts bit for bit (tests/test_gpu_map.py, _check),
    so positions, normals, scan ids and the order inside a voxel are those of the restatement."""
    ids = sorted(set(refs[0].scans()) | set(refs[1].scans()))
    omaps = [oracle.VoxelMap(w, 0), oracle.VoxelMap(w, 1)]
    for s in ids:
        for t in range(2):
            recs = refs[t].records(s)
            if recs:
                omaps[t].add_scan(s, poses[s], feats[t][recs])
    ctx.map_build(ids, np.stack([poses[s] for s in ids]), w)
    ctx.set_queries(qpl, qpt, qid)
    Tj = I34.copy()
    Tj[:, 3] = [0.003, -0.002, 0.001]
    cpl, cpt = ctx.match(Tj, max_dist)
    got = ctx.match_download()
    npl = len(qpl)
    idarr = np.asarray(ids, np.uint64)
    found_any = 0
    for t, (om, Q) in enumerate(zip(omaps, (qpl, qpt))):
        ref = om.match(Q, Tj)
        sl = slice(0, npl) if t == 0 else slice(npl, None)
        acc = ref["found"] & (ref["d2"] < max_dist * max_dist)
        pair = got["pair"][sl]
        assert np.array_equal(pair >= 0, acc)
        assert np.array_equal(idarr[pair[acc]], ref["scan"][acc])
        assert np.array_equal(got["d2"][sl][acc], ref["d2"][acc])
        assert np.array_equal(got["pi"][sl][acc], ref["pi"][acc])
        if t == 0:
            assert np.array_equal(got["ni"][acc], ref["ni"][acc])
        assert np.array_equal(got["d2"][sl] > 0.01, ~ref["found"] | (ref["d2"] > 0.01))
        counts = np.array([np.count_nonzero(ref["scan"][acc] == s) for s in ids])
        assert np.array_equal(cpl if t == 0 else cpt, counts)
        found_any += int(acc.sum())
    assert found_any > 100  # the comparison is about matches, not about an empty map
    return got


def test_seam_pool_compactions_match_restatement(fmx_mod, oracle, monkeypatch):
    """Pool limit 4000 records.  Feature values live in two big arrays; the restatement stores
    their row numbers.  fmx_map_download reads its poses from the estimator and refuses a
    context without a registered scan, so here the pool is read back through map_build +
    match alone (every record's position, normal, scan id and order enters that comparison);
    the registration tests below compare map_download."""
    LIMIT = 4000
    _limits(monkeypatch, pool=LIMIT)
    p = synth.default_params(synth.GEOMETRIES["tiny"])
    ctx = fmx_mod.Context(fmx_mod.EstimatorParams(extraction=fmx_mod.KeypointExtractionParams(**p)))
    assert _events(ctx) == dict.fromkeys(STORE_KEYS, 0)
    g = np.random.default_rng(7)
    feats = [np.zeros((0, 6), np.float32), np.zeros((0, 3), np.float32)]
    refs = [SR.PoolRef(LIMIT), SR.PoolRef(LIMIT)]
    poses = {}
    qpl, qpt = _planar(g, 700, 0.0), _point(g, 400, 0.0)
    checks = []

    def add(scan, npl, npt, expect="ok"):
        """keypoints_add of fresh random features; -> compacted (planar, point)"""
        centre = g.uniform(-1.5, 1.5, 3)
        new = [_planar(g, npl, centre), _point(g, npt, centre)]
        if scan not in poses:
            T = I34.copy()
            T[:, 3] = g.normal(0, 0.05, 3)
            poses[scan] = T
        before = _events(ctx)
        want = []
        for t in range(2):  # the planar pool first, as fmx_keypoints_add does
            rows = list(range(len(feats[t]), len(feats[t]) + len(new[t])))
            feats[t] = np.vstack([feats[t], new[t]])
            want.append(refs[t].add(scan, rows))
            if want[-1][0] != "ok":
                break
        status = want[-1][0]
        assert status == expect, (scan, npl, npt, want)
        if status == "ok":
            ctx.keypoints_add(scan, new[0], new[1])
        else:
            with pytest.raises(fmx_mod.FmxError) as e:
                ctx.keypoints_add(scan, new[0], new[1])
            assert e.value.status == OOM and "keypoint pool capacity exceeded" in str(e.value)
            if scan not in refs[0].scans() + refs[1].scans():
                poses.pop(scan)
        after = _events(ctx)
        comp = [w[1] for w in want] + [False] * (2 - len(want))
        assert after["pool_compactions_planar"] - before["pool_compactions_planar"] == comp[0], (scan, want)
        assert after["pool_compactions_point"] - before["pool_compactions_point"] == comp[1], (scan, want)
        if any(comp):
            checks.append(scan)
            _check_live(ctx, oracle, refs, feats, poses, qpl, qpt, 10 ** 6)
        return comp

    def remove(scan):
        ctx.keypoints_remove(scan)
        for r in refs:
            r.remove(scan)
        poses.pop(scan)

    add(0, 1500, 900)
    add(1, 1200, 0)                       # planar features only
    add(2, 0, 1100)                       # point features only
    add(3, LIMIT - refs[0].tail, LIMIT - refs[1].tail)  # fits exactly: no compaction
    assert refs[0].tail == refs[1].tail == LIMIT and _events(ctx)["pool_compactions_planar"] == 0
    remove(1)
    remove(2)
    assert add(4, 1000, 1000) == [True, True]   # fits only after compaction
    # an add that fits not even after compaction: refused, the held scans unchanged
    ev = _events(ctx)
    add(5, LIMIT - refs[0].live + 1, 10, expect="oom")
    assert _events(ctx)["pool_compactions_planar"] == ev["pool_compactions_planar"] + 1
    _check_live(ctx, oracle, refs, feats, poses, qpl, qpt, 10 ** 6)
    add(6, 10, LIMIT + 1, expect="oom")         # larger than the whole pool (the planar part is kept)
    _check_live(ctx, oracle, refs, feats, poses, qpl, qpt, 10 ** 6)
    # a map_insert that triggers the compaction: the queries as scan 7, inserted where no
    # record lies within min_dist_map
    remove(0)
    for t in range(2):
        assert refs[t].tail + len((qpl, qpt)[t]) > LIMIT >= refs[t].live + len((qpl, qpt)[t])
    got = _check_live(ctx, oracle, refs, feats, poses, qpl, qpt, 7)
    before = _events(ctx)
    n_ins = ctx.map_insert()
    after = _events(ctx)
    assert after["pool_compactions_planar"] == before["pool_compactions_planar"] + 1
    assert after["pool_compactions_point"] == before["pool_compactions_point"] + 1
    ins = got["d2"] > ctx.params.min_dist_map ** 2
    poses[7] = I34.copy()
    poses[7][:, 3] = [0.003, -0.002, 0.001]
    for t, (Q, m) in enumerate(((qpl, ins[:len(qpl)]), (qpt, ins[len(qpl):]))):
        rows = list(range(len(feats[t]), len(feats[t]) + int(m.sum())))
        feats[t] = np.vstack([feats[t], Q[m]])
        assert refs[t].add(7, rows, need=len(Q)) == ("ok", True)
    assert n_ins == (int(ins[:len(qpl)].sum()), int(ins[len(qpl):].sum())) and min(n_ins) > 50
    q2pl, q2pt = _planar(g, 500, 0.2), _point(g, 300, 0.2)
    _check_live(ctx, oracle, refs, feats, poses, q2pl, q2pt, 10 ** 6)
    # random adds and removes until each pool has compacted three more times
    scan = 8
    start = _events(ctx)
    for step in range(60):
        live = sorted(poses)
        if len(live) > 2 and g.random() < 0.45:
            remove(int(g.choice(live)))
            continue
        npl, npt = (int(x) for x in g.integers(300, 1500, 2))
        fits = all(refs[t].live + n <= LIMIT for t, n in ((0, npl), (1, npt)))
        if not fits:
            remove(int(g.choice(live)))
            continue
        add(scan, npl, npt)
        scan += 1
        ev = _events(ctx)
        if all(ev[k] - start[k] >= 3 for k in STORE_KEYS[:2]):
            break
    ev = _events(ctx)
    assert all(ev[k] - start[k] >= 3 for k in STORE_KEYS[:2]), (ev, start)
    assert ev["pool_compactions_planar"] == refs[0].compactions and ev["pool_compactions_point"] == refs[1].compactions
    assert ev["win_compactions"] == 0 and len(checks) >= 6


# ================================================================== registration streams
def _geo(name):
    return synth.GEOMETRIES["tiny"] if name == "tiny" else synth.ScanGeometry(5, 200, 15.0, 0.01, 0.02)


@functools.lru_cache(maxsize=None)
def _scans(name):
    """The stream as read-only host arrays: the tiny stream, or the 5 x 200 shape of the dense-map
    tests (rows and columns that are no multiple of any tile)."""
    world = synth.World()
    geo = _geo(name)
    out = []
    for k in range(N_SCANS):
        s = synth.make_scan("tiny", k, world=world)[0] if name == "tiny" else \
            synth.raycast(world, synth.trajectory_pose(k), geo, 4242 + k)
        a = np.ascontiguousarray(s.numpy(), np.float32)
        a.setflags(write=False)
        out.append(a)
    return out


_ORACLE = {}


def _oracle_trace(oracle, name, single):
    """oracle.Estimator over the stream, once: per scan the pose, the feature counts, the
    match counts (= the window store's rows of that scan) and the map's size afterwards."""
    key = (name, single)
    if key not in _ORACLE:
        p = synth.default_params(_geo(name))
        prm = oracle.default_params(p)
        prm.disable_smoothing = int(single)
        prm.max_num_recent_scans, prm.max_num_keyscans = WINDOW
        est = oracle.Estimator(prm, nthreads=4)  # (a few hundred features per scan)
        tr = dict(pose=[], feat=[], match=[], live=[])
        for s in _scans(name):
            T, st, _ = est.register_scan(s)
            m = est.map()
            tr["pose"].append(T)
            tr["feat"].append((int(st[0]), int(st[1])))
            tr["match"].append((int(st[4]), int(st[5])))
            tr["live"].append((len(m["planar"][0]), len(m["point"][0])))
        _ORACLE[key] = tr
    return _ORACLE[key]


def _sizes(tr):
    """The limits, from the oracle's counts alone.  pool: the largest of (map before a scan +
    that scan's features) over both feature types: what insert_matches asks room for, so the
    tightest limit that never refuses.  rows: the largest per-scan match count of each type."""
    pool = max(tr["live"][k - 1][t] + tr["feat"][k][t] for k in range(1, N_SCANS) for t in range(2))
    pool = max(pool, max(tr["feat"][0]))
    rows = [max(m[t] for m in tr["match"]) for t in range(2)]
    return pool, rows


def _ctx(fmx, name, single=False):
    p = synth.default_params(_geo(name))
    return fmx.Context(fmx.EstimatorParams(extraction=fmx.KeypointExtractionParams(**p), disable_smoothing=single,
                                           max_num_recent_scans=WINDOW[0], max_num_keyscans=WINDOW[1]))


COUNT_KEYS = ("icp_iters", "lm_iters", "matched_planar", "matched_point", "map_planar", "map_point", "map_scans",
              "window_poses")


def _run(ctx, name, feed, every_map=False, map_after=None):
    """Register the stream; per scan the pose, the features, the counts, the store events and
    the map (every scan, or where map_after(events before, events after, k) says so)."""
    import torch
    host = _scans(name)
    scans = [np.array(s) for s in host] if feed == "pipe_host" else [torch.from_numpy(np.array(s)).to("cuda:0") for s in host]
    out = []
    ev = _events(ctx)
    for k in range(N_SCANS):
        if feed != "seq" and k + 1 < N_SCANS:
            ctx.next_scan(scans[k + 1])
        ctx.register_scan(scans[k])
        st = ctx.last_stats()
        if feed != "seq":
            assert st["pipelined"] == (1 if k > 0 else 0), k
        nev = {key: st[key] for key in STORE_KEYS}
        rec = dict(pose=ctx.current_pose(), feat=ctx.extract_download(), counts={key: st[key] for key in COUNT_KEYS},
                   events=nev, map=None)
        if every_map or (map_after and map_after(ev, nev, k)):
            rec["map"] = ctx.map_download(0.1)
        ev = nev
        out.append(rec)
    return out


_ROOMY = {}


def _roomy(fmx, oracle, monkeypatch, name, single):
    """Context A: no limits, sequential, once per stream and mode; anchored to the oracle
    (1e-6 on every pose); its store events read 0."""
    key = (name, single)
    if key not in _ROOMY:
        _limits(monkeypatch)
        a = _run(_ctx(fmx, name, single), name, "seq", every_map=True)
        tr = _oracle_trace(oracle, name, single)
        for k, rec in enumerate(a):
            assert np.abs(rec["pose"] - tr["pose"][k]).max() < 1e-6, k
            assert (rec["counts"]["matched_planar"], rec["counts"]["matched_point"]) == tr["match"][k], k
            # (the map a scan is matched against is the one the scan before left)
            assert (rec["counts"]["map_planar"], rec["counts"]["map_point"]) == (tr["live"][k - 1] if k else (0, 0)), k
        assert a[-1]["events"] == dict.fromkeys(STORE_KEYS, 0)
        _ROOMY[key] = a
    return _ROOMY[key]


def _same_map(a, b, where):
    for kind in ("planar", "point"):
        for x, y in zip(a[kind], b[kind]):
            if x is None:
                assert y is None
            else:
                assert np.array_equal(x, y), (where, kind)


def _compare(a, b, need_maps):
    """Tight run b against roomy run a, scan by scan, bit for bit."""
    maps = 0
    for k, (ra, rb) in enumerate(zip(a, b)):
        assert np.array_equal(ra["pose"], rb["pose"]), (k, np.abs(ra["pose"] - rb["pose"]).max(), rb["events"])
        for key in ("planar_index", "point_index", "planar", "point"):
            assert np.array_equal(ra["feat"][key], rb["feat"][key]), (k, key)
        assert ra["counts"] == rb["counts"], (k, ra["counts"], rb["counts"], rb["events"])
        if rb["map"] is not None:
            _same_map(ra["map"], rb["map"], k)
            maps += 1
    assert maps >= need_maps, maps


def _after_events(before, after, k):
    """The map is compared right after the first compaction of either pool, right after the
    first compaction of the window store, and after the last scan."""
    first_pool = sum(before[x] for x in STORE_KEYS[:2]) == 0 < sum(after[x] for x in STORE_KEYS[:2])
    first_win = before["win_compactions"] == 0 < after["win_compactions"]
    return first_pool or first_win or k == N_SCANS - 1


@pytest.mark.parametrize("feed", ["seq", "pipe_dev", "pipe_host"])
@pytest.mark.parametrize("name", ["tiny", "odd"])
def test_tight_stream_equals_roomy(fmx_mod, oracle, monkeypatch, name, feed):
    """Context B: the pool at its tightest limit, both arenas starting at one scan's rows."""
    a = _roomy(fmx_mod, oracle, monkeypatch, name, False)
    pool, rows = _sizes(_oracle_trace(oracle, name, False))
    _limits(monkeypatch, pool, rows[0], rows[1])
    b = _run(_ctx(fmx_mod, name), name, feed, map_after=_after_events)
    ev = b[-1]["events"]
    print(name, feed, "limits", pool, rows, "events", ev)
    assert ev["pool_compactions_planar"] + ev["pool_compactions_point"] >= 3, ev
    assert ev["win_compactions"] >= 3 and ev["win_growths_plane"] >= 1 and ev["win_growths_point"] >= 1, ev
    _compare(a, b, 2)


@pytest.mark.parametrize("name", ["tiny", "odd"])
def test_tight_pool_single_pose_mode(fmx_mod, oracle, monkeypatch, name):
    """disable_smoothing: no window store; the pool compacts under a pipelined device feed."""
    a = _roomy(fmx_mod, oracle, monkeypatch, name, True)
    pool, rows = _sizes(_oracle_trace(oracle, name, True))
    _limits(monkeypatch, pool)
    b = _run(_ctx(fmx_mod, name, True), name, "pipe_dev", map_after=_after_events)
    ev = b[-1]["events"]
    print(name, "single limits", pool, "events", ev)
    assert ev["pool_compactions_planar"] + ev["pool_compactions_point"] >= 3, ev
    assert ev["win_compactions"] == 0, ev
    _compare(a, b, 2)


@pytest.mark.parametrize("grows", ["point", "plane"])
@pytest.mark.parametrize("name", ["tiny", "odd"])
def test_one_arena_grows_the_other_compacts(fmx_mod, oracle, monkeypatch, name, grows):
    """The growing arena starts at half the rows of the first scan that has any (growth from
    an empty store); the other at 4 x (window + 3) scans' rows, more than twice what the
    window can hold, so it only ever compacts.  No pool limit."""
    a = _roomy(fmx_mod, oracle, monkeypatch, name, False)
    tr = _oracle_trace(oracle, name, False)
    _, rows = _sizes(tr)
    t = 0 if grows == "plane" else 1
    first = next(m[t] for m in tr["match"] if m[t] > 0)
    caps = [4 * (sum(WINDOW) + 3) * rows[0], 4 * (sum(WINDOW) + 3) * rows[1]]
    caps[t] = max(first // 2, 1)
    _limits(monkeypatch, 0, caps[0], caps[1])
    b = _run(_ctx(fmx_mod, name), name, "seq", map_after=_after_events)
    ev = b[-1]["events"]
    print(name, grows, "caps", caps, "events", ev)
    first_k = next(k for k, m in enumerate(tr["match"]) if m[t] > 0)
    e1 = b[first_k]["events"]
    assert e1["win_compactions"] == 1 and e1[STORE_KEYS[3 + t]] == 1, e1  # the first segment did not fit
    assert ev[STORE_KEYS[3 + t]] >= 1 and ev[STORE_KEYS[4 - t]] == 0 and ev["win_compactions"] >= 2, ev
    assert ev["pool_compactions_planar"] + ev["pool_compactions_point"] == 0, ev
    _compare(a, b, 2)
