"""numpy restatement of the cloud organizer (include/fmx/fmx.h, fmx_organize) and of the
per-point deskew (fmx_deskew_cells), plus the jittered cloud both test files use.

Organizer, all in fp64 on the fp32 coordinates: a point with a non-finite coordinate or
x = y = z = 0 is invalid; u = (atan2(y, x) - azimuth_offset) * cols / 2pi, negated when
clockwise; col = floor(u + 0.5) mod cols; row = ring_to_row[ring] (identity without a
table; past the table or -1: off-grid) or the elevation table's entry nearest to
atan2(z, sqrt(x x + y y)) (a tie to the lower row; beyond an outermost entry by more than
half the spacing to its neighbour: off-grid).  A cell keeps the point with the smallest
r2 = (x x + y y) + z z (fp32), the lowest index among equal r2."""
import numpy as np

EMPTY = 0xFFFFFFFF


def cells_of(xyzw, ring, rows, cols, elevation=None, ring_to_row=None, azimuth_offset=0.0, clockwise=False):
    """(row, col, valid, on_grid, column offset from the cell centre in columns, row offset
    in spacings (elevation mode, else 0)) of every point."""
    p = np.ascontiguousarray(xyzw, np.float32)[:, :3]
    valid = np.isfinite(p).all(1) & p.any(1)
    x, y, z = (np.where(valid, p[:, k], 1.0).astype(np.float64) for k in range(3))
    u = (np.arctan2(y, x) - azimuth_offset) * cols / (2 * np.pi)
    if clockwise:
        u = -u
    f = np.floor(u + 0.5)
    col = np.mod(f, cols).astype(np.int64)
    if elevation is not None:
        tab = np.asarray(elevation, np.float64)
        el = np.arctan2(z, np.sqrt(x * x + y * y))
        row = np.abs(tab[None, :] - el[:, None]).argmin(1)  # the first minimum: a tie goes to the lower row
        gap = np.abs(np.diff(tab))
        out0 = np.abs(el - tab[0]) > 0.5 * gap[0]
        out1 = np.abs(el - tab[-1]) > 0.5 * gap[-1]
        on = ~((row == 0) & out0) & ~((row == rows - 1) & out1)
        near = np.where(row == 0, gap[0], gap[np.maximum(row, 1) - 1])
        drow = np.abs(el - tab[row]) / near
    else:
        g = np.asarray(ring).astype(np.int64)
        t = np.arange(rows) if ring_to_row is None else np.asarray(ring_to_row, np.int64)
        row = np.where(g < len(t), t[np.minimum(g, len(t) - 1)], -1)
        on = (row >= 0) & (row < rows)
        row = np.where(on, row, 0)
        drow = np.zeros(len(p))
    return row, col, valid, on & valid, np.abs(u - f), drow


def organize(xyzw, ring, rows, cols, fraction=None, **cfg):
    """(scan (rows * cols, 4) float32, index (rows * cols,) uint32, fraction plane or None,
    counts dict)."""
    xyzw = np.ascontiguousarray(xyzw, np.float32).reshape(-1, 4)
    n = len(xyzw)
    row, col, valid, on, _, _ = cells_of(xyzw, ring, rows, cols, **cfg)
    x, y, z = xyzw[:, 0], xyzw[:, 1], xyzw[:, 2]
    with np.errstate(all="ignore"):
        r2 = ((x * x + y * y) + z * z).astype(np.float32)
    key = (r2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(n, dtype=np.uint64)
    best = np.full(rows * cols, np.iinfo(np.uint64).max, np.uint64)
    np.minimum.at(best, (row * cols + col)[on], key[on])
    filled = best != np.iinfo(np.uint64).max
    index = np.where(filled, best & np.uint64(EMPTY), EMPTY).astype(np.uint32)
    scan = np.zeros((rows * cols, 4), np.float32)
    scan[filled, :3] = xyzw[index[filled], :3]
    plane = None
    if fraction is not None:
        plane = np.zeros(rows * cols, np.float32)
        plane[filled] = np.clip(np.asarray(fraction, np.float32), 0.0, 1.0)[index[filled]]
    placed = int(filled.sum())
    counts = dict(placed=placed, displaced=int(on.sum()) - placed, off_grid=int((valid & ~on).sum()),
                  invalid=int((~valid).sum()))
    return scan, index, plane, counts


def deskew_cells(oracle, scan, fraction, xi):
    """deskew_ref.deskew's per-column formula evaluated per point: p' = Exp((s - 0.5) xi) p
    with the point's own fraction s (float32), fp64, ((R0 x + R1 y) + R2 z) + t, rounded
    once; a dropout stays 0 and a point whose scaled twist is exactly 0 is copied."""
    scan = np.ascontiguousarray(scan, np.float32).reshape(-1, 4)
    xi = np.asarray(xi, np.float64).reshape(6)
    s = np.asarray(fraction, np.float32).astype(np.float64) - 0.5
    out = scan.copy()
    uniq, inv = np.unique(s, return_inverse=True)
    moves = np.array([bool(np.any(v * xi)) for v in uniq])
    Ts = np.stack([np.asarray(oracle.expmap(v * xi), np.float64).reshape(3, 4) if mv else np.eye(3, 4)
                   for v, mv in zip(uniq, moves)])
    M = Ts[inv]
    x, y, z = (scan[:, k].astype(np.float64) for k in range(3))
    q = np.stack([((M[:, k, 0] * x + M[:, k, 1] * y) + M[:, k, 2] * z) + M[:, k, 3] for k in range(3)], 1)
    live = scan[:, :3].any(1) & moves[inv]
    out[live, :3] = q[live].astype(np.float32)
    return out


def jittered_cloud(rows, cols, elev_deg=15.0, seed=11, azimuth_offset=0.3, clockwise=True, sprinkle=True):
    """The collision test's cloud: 0-3 points per cell (default_rng(seed).integers(0, 4)), azimuth
    at (c + U(-0.4, 0.4)) columns, elevation at tab[r] + U(-0.4, 0.4) spacings, range
    U(1, 80), 5 % of the points appended again as exact duplicates, all shuffled; with
    sprinkle a few all-zero, NaN and Inf points and rings >= rows are mixed in.  Returns
    dict(xyzw, ring, fraction, elevation (the table), cfg (the organizer's settings))."""
    g = np.random.default_rng(seed)
    tab = np.linspace(np.radians(elev_deg), -np.radians(elev_deg), rows)
    per = g.integers(0, 4, rows * cols)
    cell = np.repeat(np.arange(rows * cols), per)
    r, c = cell // cols, cell % cols
    m = len(cell)
    u = c + g.uniform(-0.4, 0.4, m)
    az = u * (2 * np.pi / cols)
    az = (-az if clockwise else az) + azimuth_offset
    spacing = abs(tab[1] - tab[0])
    el = tab[r] + g.uniform(-0.4, 0.4, m) * spacing
    rng = g.uniform(1.0, 80.0, m)
    xyz = np.stack([rng * np.cos(el) * np.cos(az), rng * np.cos(el) * np.sin(az), rng * np.sin(el)], 1)
    xyzw = np.zeros((m, 4), np.float32)
    xyzw[:, :3] = xyz.astype(np.float32)
    ring = r.astype(np.uint16)
    frac = g.uniform(0.0, 1.0, m).astype(np.float32)
    dup = g.choice(m, m // 20, replace=False)
    xyzw, ring, frac = (np.concatenate([a, a[dup]]) for a in (xyzw, ring, frac))
    if sprinkle:
        k = 12
        bad = np.zeros((k, 4), np.float32)
        bad[4:8, 0] = np.nan
        bad[4:8, 1] = 1.0
        bad[8:10, 2] = np.inf
        bad[10:12] = xyzw[:2]  # fine points (copies of the first two), but on rings the sensor does not have
        bring = np.zeros(k, np.uint16)
        bring[10:12] = (rows, 65535)
        xyzw = np.concatenate([xyzw, bad])
        ring = np.concatenate([ring, bring])
        frac = np.concatenate([frac, np.full(k, 0.5, np.float32)])
    perm = g.permutation(len(xyzw))
    out = dict(xyzw=xyzw[perm], ring=ring[perm], fraction=frac[perm], elevation=tab,
               cfg=dict(azimuth_offset=azimuth_offset, clockwise=clockwise))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out
