"""Plain numpy reference of the pair sort (form_amd/csrc/voxelmap.hip): query-order match
results -> pair-major rows, per-pair counts and first rows, and the chunk table.  Uses
nothing from the library."""
import numpy as np

CHUNK_ROWS = 256  # rows per chunk of either type (the window kernel's block)


def pair_sort_ref(pair, pi, ni, q_pl, q_pt, K):
    """pair: [npl + npt] int32 (planar queries first, -1 = not accepted); pi: [npl + npt, 3]
    and ni: [npl, 3] float64 as match_download() gives them; q_pl / q_pt: float32 query
    positions ([n, >= 3]: further columns are ignored)."""
    pair = np.asarray(pair)
    q_pl = np.asarray(q_pl, np.float32).reshape(len(q_pl), -1) if len(q_pl) else np.zeros((0, 3), np.float32)
    q_pt = np.asarray(q_pt, np.float32).reshape(len(q_pt), -1) if len(q_pt) else np.zeros((0, 3), np.float32)
    npl = len(q_pl)
    out = {}
    for name, pr, p_i, q in (("plane", pair[:npl], pi[:npl], q_pl), ("point", pair[npl:], pi[npl:], q_pt)):
        acc = np.flatnonzero(pr >= 0)
        cnt = np.bincount(pr[acc], minlength=K).astype(np.uint32)
        order = acc[np.argsort(pr[acc], kind="stable")]  # a stable partition by pair
        out["counts_" + name] = cnt
        out["base_" + name] = (np.cumsum(cnt) - cnt).astype(np.uint32)
        out[name + "_pi"] = p_i[order].astype(np.float64).reshape(-1, 3)
        out[name + "_pj"] = q[order, :3].astype(np.float64).reshape(-1, 3)  # float32 widens exactly
        if name == "plane":
            out["plane_ni"] = np.asarray(ni)[order].astype(np.float64).reshape(-1, 3)
    out.update(chunk_table(out["counts_plane"], out["counts_point"]))
    return out


def chunk_table(n_plane, n_point):
    """Per pair its plane chunks then its point chunks, CHUNK_ROWS rows each; a descriptor
    is (type, pair, first row, end row) with rows counted per type."""
    K = len(n_plane)
    chunks, cr = [], np.zeros(K + 1, np.uint32)
    op = ot = 0
    for k in range(K):
        cr[k] = len(chunks)
        for r in range(0, int(n_plane[k]), CHUNK_ROWS):
            chunks.append((0, k, op + r, op + min(int(n_plane[k]), r + CHUNK_ROWS)))
        for r in range(0, int(n_point[k]), CHUNK_ROWS):
            chunks.append((1, k, ot + r, ot + min(int(n_point[k]), r + CHUNK_ROWS)))
        op += int(n_plane[k])
        ot += int(n_point[k])
    cr[K] = len(chunks)
    return dict(chunk_range=cr, n_chunks=len(chunks), chunks=np.array(chunks, np.uint32).reshape(-1, 4))


KEYS = ("counts_plane", "counts_point", "base_plane", "base_point", "chunk_range", "n_chunks", "chunks",
        "plane_pi", "plane_ni", "plane_pj", "point_pi", "point_pj")


def assert_same(got, ref, what=""):
    """Every item bit for bit (the sort moves data and widens float32 exactly)."""
    for k in KEYS:
        g, r = got[k], ref[k]
        if k == "n_chunks":
            assert int(g) == int(r), f"{what} n_chunks: {g} != {r}"
            continue
        assert g.shape == r.shape, f"{what} {k}: shape {g.shape} != {r.shape}"
        if not np.array_equal(g, r):
            bad = np.flatnonzero((g != r).any(axis=1) if g.ndim > 1 else g != r)
            raise AssertionError(f"{what} {k}: {len(bad)} of {len(g)} entries differ, first at {bad[:5]}")
