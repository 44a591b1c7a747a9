"""The pair sort bit for bit in every dispatch form (form_amd/csrc/pair_sort_plan.hpp):
fmx_corr_download() after a sorted match against the numpy reference (tests/pairsort_ref.py)
on the same match's query-order results.  The sort moves data and widens float32 exactly, so
every comparison is np.array_equal; the match itself (checked against the oracle elsewhere)
is the trusted input.  Scenes fix every query's pair by construction
(tests/pairsort_cases.py), so a scene cannot silently match nothing.

tests/test_gpu_parity.py::test_match_sort_then_linearize runs two of these shapes against
the oracle's G blocks: its K = 5 is case A, the scatter-scanned form (its docstring's "scanned
by the match's last block" describes the tail-scanned form, case C here); its K = 300 is D2."""
import ctypes as C
import time

import numpy as np
import pytest

import pairsort_cases as PC
import pairsort_ref as PR

pytestmark = pytest.mark.gpu

MIN_D2 = PC.MIN_DIST_MAP * PC.MIN_DIST_MAP

_SCENES = {}


def _scene(cid):
    """Built once per case and shared (never modified)."""
    if cid not in _SCENES:
        _SCENES[cid] = PC.case_scene(PC.BY_ID[cid])
    return _SCENES[cid]


class Rig:
    """One context; the scans of every K used on it are stored once (a scene's map depends
    on K alone) and the map is rebuilt where K changes."""

    def __init__(self, fmx):
        self.fmx = fmx
        self.ctx = fmx.Context(fmx.EstimatorParams(min_dist_map=PC.MIN_DIST_MAP))
        self.bases = {}
        self.K = None
        self.next_scan = 0

    def use_map(self, scene):
        K = scene["K"]
        if K not in self.bases:
            self.bases[K] = self.next_scan
            self.next_scan += K
            for k, (pl, pt) in enumerate(scene["scans"]):
                self.ctx.keypoints_add(self.bases[K] + k, pl, pt)
        if self.K != K:
            self.ctx.map_build(self.bases[K] + np.arange(K), scene["poses"], PC.VOXEL)
            self.K = K

    def set_queries(self, scene):
        self.ctx.set_queries(scene["q_pl"], scene["q_pt"], 1 << 20 | self.next_scan)
        self.next_scan += 1  # (a query scan of its own: map_insert appends under it)

    def check(self, cid, fresh_queries=True, deferred=None):
        """One sorted match of the case, every table and row against the reference; returns
        the download.  deferred: None (counts requested), "download" (match without counts,
        then the download launches the scatter) or "linearize" (a linearization first)."""
        case, scene, ctx = PC.BY_ID[cid], _scene(cid), self.ctx
        K, npl = case.K, case.npl
        self.use_map(scene)
        if fresh_queries:
            self.set_queries(scene)
        plan = self.fmx.pair_sort_plan(case.npl, case.npt, K)
        assert (plan["group"], plan["form"], plan["scan_launches"]) == (case.group, case.form, case.scan_launches)
        want_pl, want_pt = PC.design_counts(K, scene["pair_pl"], scene["pair_pt"])
        if deferred is None:
            cpl, cpt = ctx.match(scene["Tj"], PC.MAX_DIST)
            assert np.array_equal(cpl, want_pl) and np.array_equal(cpt, want_pt), f"{cid}: counts"
        else:
            assert ctx.match(scene["Tj"], PC.MAX_DIST, counts=False) is None
            if deferred == "linearize":
                ctx.linearize(scene["poses"].reshape(K, 12), np.tile(scene["Tj"].reshape(12), (K, 1)), 0.1)
        got = ctx.corr_download()
        m = ctx.match_download()
        # the scene realizes its design: every query's pair, hence the per-pair counts
        assert np.array_equal(m["pair"], np.concatenate([scene["pair_pl"], scene["pair_pt"]])), f"{cid}: pairs"
        assert np.array_equal(got["counts_plane"], want_pl) and np.array_equal(got["counts_point"], want_pt)
        ref = PR.pair_sort_ref(m["pair"], m["pi"], m["ni"], scene["q_pl"], scene["q_pt"], K)
        PR.assert_same(got, ref, cid)
        # the insert offsets come from the same tail / meta pass
        ins = ctx.map_insert()
        assert ins == (int((m["d2"][:npl] > MIN_D2).sum()), int((m["d2"][npl:] > MIN_D2).sum())), f"{cid}: inserts"
        return got


@pytest.fixture
def rig(fmx_mod):
    r = Rig(fmx_mod)
    yield r
    r.ctx.close()


def _same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in PR.KEYS)


@pytest.mark.parametrize("cid", [c.id for c in PC.CASES])
def test_case(rig, cid):
    """Each table row on a fresh context: counts, first rows, chunk table, every row."""
    _scene(cid)
    t0 = time.perf_counter()
    got = rig.check(cid)
    case = PC.BY_ID[cid]
    if not case.reach:
        assert got["n_chunks"] == 0 and not got["counts_plane"].any() and not got["counts_point"].any()
        assert len(got["plane_pi"]) == 0 and len(got["point_pi"]) == 0
    else:
        assert got["n_chunks"] > 0
    print(f"{cid}: {case.form}, group {case.group}, scans {case.scan_launches}: {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("cid", ["A", "C", "D2", "F64", "F256"])
def test_repeatable(rig, cid):
    """Twice on one context: new queries, then the same queries again (a warm match)."""
    a = rig.check(cid)
    b = rig.check(cid, fresh_queries=False)
    c = rig.check(cid)
    assert _same(a, b) and _same(a, c)


def test_form_changes_on_one_context(rig):
    """The count table's two halves, its clear and its regrowth: scatter-scanned with a full
    table, nothing matched, scatter-scanned, tail-scanned (a larger table), per-block,
    scatter-scanned twice."""
    seen = {}
    for cid in ("B", "A3", "A", "C", "D", "A", "A"):
        got = rig.check(cid)
        if cid in seen:
            assert _same(got, seen[cid])
        seen[cid] = got


def test_form_changes_across_builds(rig):
    """... and between the one-lane and the eight-lane build of the match."""
    seen = {}
    for cid in ("E'", "A", "F64", "A"):
        got = rig.check(cid)
        if cid in seen:
            assert _same(got, seen[cid])
        seen[cid] = got


def test_deferred_scatter_small(rig):
    """fmx_match without counts defers the row scatter (and, scatter-scanned, the counts):
    the download launches it and returns the same bits as the immediate form."""
    assert _same(rig.check("A", deferred="download"), rig.check("A"))


def test_deferred_match_large(rig):
    """On the one-lane build the match itself is deferred: a linearization launches match
    and scatter, the download then reads the same bits."""
    assert _same(rig.check("E'", deferred="linearize"), rig.check("E'"))


def test_no_queries_after_a_match(rig):
    """A match without queries launches nothing: its tables are empty, not the words the
    previous match (case A, same context) left on the device."""
    rig.check("A")
    ctx = rig.ctx
    ctx.set_queries(np.zeros((0, 6), np.float32), np.zeros((0, 3), np.float32), 1 << 21)
    cpl, cpt = ctx.match(_scene("A")["Tj"], PC.MAX_DIST)
    assert not cpl.any() and not cpt.any()
    got = ctx.corr_download()
    empty = np.zeros((0, 3))
    ref = PR.pair_sort_ref(np.zeros(0, np.int32), empty, empty, np.zeros((0, 6), np.float32),
                           np.zeros((0, 3), np.float32), 5)
    PR.assert_same(got, ref, "no queries")
    assert got["n_chunks"] == 0 and ctx.map_insert() == (0, 0)


def test_one_more_query_changes_build_not_rows(fmx_mod):
    """E' is E with one more point query: the one-lane build sorts it, and every row but
    that query's equals the eight-lane build's."""
    r1, r2 = Rig(fmx_mod), Rig(fmx_mod)
    e, ep = r1.check("E"), r2.check("E'")
    r1.ctx.close()
    r2.ctx.close()
    for k in ("plane_pi", "plane_ni", "plane_pj", "counts_plane", "base_plane"):
        assert np.array_equal(e[k], ep[k]), k
    extra = int(_scene("E'")["pair_pt"][-1])
    row = int(ep["base_point"][extra] + ep["counts_point"][extra] - 1)  # the last query is its pair's last row
    assert np.array_equal(np.delete(ep["point_pi"], row, 0), e["point_pi"])
    assert np.array_equal(np.delete(ep["point_pj"], row, 0), e["point_pj"])
    assert np.array_equal(ep["point_pj"][row], _scene("E'")["q_pt"][-1].astype(np.float64))


def _corr(rng, n_plane, n_point):
    Np, Nt = int(sum(n_plane)), int(sum(n_point))
    return dict(n_plane=np.array(n_plane, np.uint32), n_point=np.array(n_point, np.uint32),
                plane_pi=rng.normal(size=(Np, 3)), plane_ni=rng.normal(size=(Np, 3)), plane_pj=rng.normal(size=(Np, 3)),
                point_pi=rng.normal(size=(Nt, 3)), point_pj=rng.normal(size=(Nt, 3)))


def test_corr_set_round_trip(fmx_mod):
    """corr_set(x) then corr_download() is x, with the chunk table upload_corr builds: empty
    pairs, and pairs of 256 and 257 rows."""
    ctx = fmx_mod.Context()
    x = _corr(np.random.default_rng(3), [0, 256, 257, 3, 0, 100, 0], [5, 0, 0, 300, 0, 256, 0])
    ctx.corr_set(x["n_plane"], x["plane_pi"], x["plane_ni"], x["plane_pj"], x["n_point"], x["point_pi"], x["point_pj"])
    got = ctx.corr_download()
    ref = dict(x, counts_plane=x["n_plane"], counts_point=x["n_point"],
               base_plane=(np.cumsum(x["n_plane"]) - x["n_plane"]).astype(np.uint32),
               base_point=(np.cumsum(x["n_point"]) - x["n_point"]).astype(np.uint32),
               **PR.chunk_table(x["n_plane"], x["n_point"]))
    PR.assert_same(got, ref, "round trip")
    assert got["n_chunks"] == (1 + 2 + 1 + 1) + (1 + 2 + 1)  # plane 256, 257, 3, 100; point 5, 300, 256
    ctx.close()


def _raw_download(fmx, ctx, bufs, caps):
    return fmx.lib().fmx_corr_download(
        ctx.h, fmx._p(bufs["sizes"]), fmx._p(bufs["counts"]), fmx._p(bufs["base"]), fmx._p(bufs["chunk_range"]),
        C.c_uint32(caps[0]), fmx._p(bufs["chunks"]), C.c_uint32(caps[1]), fmx._p(bufs["pl"][0]), fmx._p(bufs["pl"][1]),
        fmx._p(bufs["pl"][2]), C.c_uint32(caps[2]), fmx._p(bufs["pt"][0]), fmx._p(bufs["pt"][1]), C.c_uint32(caps[3]))


def test_corr_download_state_and_capacity(fmx_mod):
    """Before any match: FMX_E_STATE.  A capacity one short: FMX_E_INVAL, outputs untouched."""
    ctx = fmx_mod.Context()
    with pytest.raises(fmx_mod.FmxError) as e:
        ctx.corr_download()
    assert e.value.status == 5  # FMX_E_STATE
    x = _corr(np.random.default_rng(4), [10, 0, 300], [0, 7, 2])
    ctx.corr_set(x["n_plane"], x["plane_pi"], x["plane_ni"], x["plane_pj"], x["n_point"], x["point_pi"], x["point_pj"])
    full = (3, int(ctx.corr_download()["n_chunks"]), 310, 9)
    for short in range(4):
        caps = tuple(c - (i == short) for i, c in enumerate(full))
        bufs = dict(sizes=np.full(4, 77, np.uint32), counts=np.full(6, 77, np.uint32), base=np.full(6, 77, np.uint32),
                    chunk_range=np.full(4, 77, np.uint32), chunks=np.full((full[1], 4), 77, np.uint32),
                    pl=[np.full((310, 3), 77.0) for _ in range(3)], pt=[np.full((9, 3), 77.0) for _ in range(2)])
        assert _raw_download(fmx_mod, ctx, bufs, caps) == 1  # FMX_E_INVAL
        for v in list(bufs.values()):
            for a in (v if isinstance(v, list) else [v]):
                assert np.all(a == 77)
    # with the capacities it asked for, and with NULL outputs whose capacities are then ignored
    bufs["pl"] = [None, None, None]
    assert _raw_download(fmx_mod, ctx, bufs, (full[0], full[1], 0, full[3])) == 0
    assert list(bufs["sizes"]) == [3, full[1], 310, 9] and np.array_equal(bufs["pt"][1], x["point_pj"])
    ctx.close()
