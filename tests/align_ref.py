"""Aligning a scan to the dense map restated (include/fmx/fmx.h, fmx_align_system and
fmx_align_dense; DESIGN.md §Dense map, Aligning).  Given the points, the pose and a nearest
result (`state`, `points`: from tests/nearest_ref.py's NearestRef, from the device's
nearest_voxels, or from anywhere else) it builds the per-point rows in numpy fp64, one rounding
per written operation, and sums each of the 29 entries with math.fsum, so the sums are the
exactly rounded ones whatever order a kernel adds in.  The Gauss-Newton loop is restated in
plain Python with pose.hpp's expmap, compose and Cholesky."""
import math

import numpy as np

import probe_ref as PR

CLASSES = ("found", "none", "out_of_range", "invalid")


def pack_index(r, q):
    return r * 7 - r * (r - 1) // 2 + (q - r)


def kept(n, stride):
    """The indices i % stride == 0 (stride 0 reads 1)."""
    return np.arange(0, n, max(int(stride), 1))


def rows(xyzw, pose34, state, q, sigma):
    """(3 F, 7) whitened rows [H_a * inv, -r_a * inv] of the F found points, a fastest."""
    p = np.ascontiguousarray(xyzw, np.float32).reshape(-1, 4)[:, :3].astype(np.float64)
    T = np.ascontiguousarray(pose34, np.float64).reshape(3, 4)
    found = np.asarray(state) == PR.SOLID
    p, q = p[found], np.ascontiguousarray(q, np.float64).reshape(-1, 3)[found]
    inv = 1.0 / float(sigma)
    out = np.zeros((len(p), 3, 7))
    for a in range(3):
        R0, R1, R2, t = T[a, 0], T[a, 1], T[a, 2], T[a, 3]
        w = ((R0 * p[:, 0] + R1 * p[:, 1]) + R2 * p[:, 2]) + t  # the integration's expression
        r = w - q[:, a]
        out[:, a, 0] = (R2 * p[:, 1] - R1 * p[:, 2]) * inv
        out[:, a, 1] = (R0 * p[:, 2] - R2 * p[:, 0]) * inv
        out[:, a, 2] = (R1 * p[:, 0] - R0 * p[:, 1]) * inv
        out[:, a, 3], out[:, a, 4], out[:, a, 5] = R0 * inv, R1 * inv, R2 * inv
        out[:, a, 6] = -r * inv
    return out.reshape(-1, 7)


def system(xyzw, pose34, state, q, sigma):
    """The 29 doubles of fmx_align_system over the given points (already strided)."""
    v = rows(xyzw, pose34, state, q, sigma)
    S = np.zeros(29)
    for r in range(7):
        for c in range(r, 7):
            S[pack_index(r, c)] = math.fsum((v[:, r] * v[:, c]).tolist())
    S[28] = 0.5 * S[27]
    return S


def counts_of(state, n, stride):
    st = np.asarray(state)
    return dict(found=int((st == PR.SOLID).sum()), none=int((st == PR.ABSENT).sum()),
                out_of_range=int((st == PR.OUT_OF_RANGE).sum()), invalid=int((st == PR.INVALID).sum()),
                skipped=int(n - len(st)))


def system_from(nearest, xyzw, pose34, sigma=1.0, stride=1, **kw):
    """nearest(points, pose34, **kw) -> a nearest result; the system, the counts and the
    result's lookups_bounds (None where it has none) over the points i % stride == 0."""
    p = np.ascontiguousarray(xyzw, np.float32).reshape(-1, 4)
    sub = p[kept(len(p), stride)]
    got = nearest(sub, pose34, **kw)
    return system(sub, pose34, got["state"], got["points"], sigma), counts_of(got["state"], len(p), stride), \
        got.get("lookups_bounds")


def unpack(S):
    H, g = np.zeros((6, 6)), np.zeros(6)
    for r in range(7):
        for c in range(r, 7):
            v = float(S[pack_index(r, c)])
            if c < 6:
                H[r, c] = H[c, r] = v
            elif r < 6:
                g[r] = v
    return H, g


# ---- pose.hpp, operation for operation
def compose(a, b):
    a, b = np.asarray(a, np.float64).reshape(3, 4).tolist(), np.asarray(b, np.float64).reshape(3, 4).tolist()
    c = [[0.0] * 4 for _ in range(3)]
    for i in range(3):
        for j in range(3):
            c[i][j] = (a[i][0] * b[0][j] + a[i][1] * b[1][j]) + a[i][2] * b[2][j]
        c[i][3] = ((a[i][0] * b[0][3] + a[i][1] * b[1][3]) + a[i][2] * b[2][3]) + a[i][3]
    return np.array(c)


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def expmap(xi):
    w, v = [float(x) for x in xi[:3]], [float(x) for x in xi[3:6]]
    th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2]
    if th2 <= np.finfo(np.float64).eps:
        A, B, a, b = 1.0, 0.5, 0.5, 1.0 / 6.0
    else:
        th = math.sqrt(th2)
        A = math.sin(th) / th
        B = (1.0 - math.cos(th)) / th2
        a = B
        b = (th - math.sin(th)) / (th2 * th)
    W = [[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]]
    T = [[0.0] * 4 for _ in range(3)]
    for i in range(3):
        for j in range(3):
            w2 = W[i][0] * W[0][j] + W[i][1] * W[1][j] + W[i][2] * W[2][j]
            T[i][j] = (1.0 if i == j else 0.0) + A * W[i][j] + B * w2
    wxv = _cross(w, v)
    wxwxv = _cross(w, wxv)
    for i in range(3):
        T[i][3] = v[i] + a * wxv[i] + b * wxwxv[i]
    return np.array(T)


def chol_solve6(H, g):
    """x with H x = g, or None where a pivot is not positive."""
    H, g = np.asarray(H, np.float64).tolist(), [float(x) for x in g]
    L = [[0.0] * 6 for _ in range(6)]
    for i in range(6):
        for j in range(i + 1):
            s = H[i][j]
            for k in range(j):
                s -= L[i][k] * L[j][k]
            if i == j:
                if s <= 0:
                    return None
                L[i][i] = math.sqrt(s)
            else:
                L[i][j] = s / L[j][j]
    y, x = [0.0] * 6, [0.0] * 6
    for i in range(6):
        s = g[i]
        for k in range(i):
            s -= L[i][k] * y[k]
        y[i] = s / L[i][i]
    for i in range(5, -1, -1):
        s = y[i]
        for k in range(i + 1, 6):
            s -= L[k][i] * x[k]
        x[i] = s / L[i][i]
    return np.array(x)


def gn_step(S, pose34):
    """(the pose after one step, ||dx||), or None for a singular system."""
    H, g = unpack(S)
    dx = chol_solve6(H, g)
    if dx is None:
        return None
    n2 = 0.0
    for x in dx.tolist():
        n2 += x * x
    return compose(pose34, expmap(dx)), math.sqrt(n2)


def align(system_at, pose_init34, max_iters=30, threshold=1e-6):
    """fmx_align_dense's loop over system_at(pose34) -> (S, counts).  Returns dict(pose, iters,
    converged, last_step, error, counts, steps: every step's norm), or None when a system is
    singular."""
    T = np.array(pose_init34, np.float64).reshape(3, 4)
    out = dict(iters=0, converged=False, last_step=0.0, error=0.0, counts=None, steps=[])
    while out["iters"] < max_iters:
        S, cnt = system_at(T)
        out["iters"] += 1
        out["error"], out["counts"] = float(S[28]), cnt
        step = gn_step(S, T)
        if step is None:
            return None
        T, out["last_step"] = step
        out["steps"].append(out["last_step"])
        out["converged"] = out["last_step"] < threshold
        if out["converged"]:
            break
    out["pose"] = T
    return out


# ---- the zero-residual problem shared by tests/test_align_cpu.py and tests/test_gpu_align.py
ZERO_W = 1.0
ZERO_THRESHOLD = 1e-6
ZERO_XI = (0.02, -0.015, 0.025, 0.06, -0.04, 0.05)  # the initial pose is Exp(ZERO_XI)


def zero_residual_cloud(seed=3):
    """48 fp32 points, one per voxel of a 4 x 4 x 3 block of width ZERO_W (each at least 0.25
    inside its cell), and Exp(ZERO_XI): a scan that is the map itself, seen from a perturbed pose."""
    g = np.random.default_rng(seed)
    cells = np.array([(x, y, z) for x in range(-2, 2) for y in range(-2, 2) for z in range(-1, 2)], np.float64)
    p = np.zeros((len(cells), 4), np.float32)
    p[:, :3] = (cells + 0.5 + g.uniform(-0.25, 0.25, cells.shape)) * ZERO_W
    return p, expmap(ZERO_XI)
