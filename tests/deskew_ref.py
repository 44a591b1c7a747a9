"""numpy restatement of scan deskewing (include/fmx/fmx.h, fmx_deskew): column c of an
organized rows x cols scan, sampled at sweep fraction s_c, moves to mid-sweep by
Exp((s_c - 0.5) xi) (oracle_py.expmap, the reference's Pose3::Expmap), applied in fp64 in
the expression order ((R0 x + R1 y) + R2 z) + t and rounded once to fp32.  A dropout
(x = y = z = 0) stays 0, the pad is copied, and a column whose scaled twist is exactly 0
is copied (Exp(0) is the identity)."""
import numpy as np


def fractions(cols: int, table=None) -> np.ndarray:
    if table is None:
        return np.arange(cols, dtype=np.float64) / float(cols)
    return np.asarray(table, np.float32).astype(np.float64)


def deskew(oracle, scan: np.ndarray, rows: int, cols: int, xi, table=None) -> np.ndarray:
    scan = np.ascontiguousarray(scan, np.float32).reshape(rows, cols, 4)
    xi = np.asarray(xi, np.float64).reshape(6)
    out = scan.copy()
    s = fractions(cols, table)
    for c in range(cols):
        x6 = (s[c] - 0.5) * xi
        if not np.any(x6):
            continue
        T = oracle.expmap(x6)
        p = scan[:, c, :3].astype(np.float64)
        x, y, z = p[:, 0], p[:, 1], p[:, 2]
        q = np.stack([((T[i, 0] * x + T[i, 1] * y) + T[i, 2] * z) + T[i, 3] for i in range(3)], 1).astype(np.float32)
        drop = (scan[:, c, 0] == 0) & (scan[:, c, 1] == 0) & (scan[:, c, 2] == 0)
        q[drop] = 0.0
        out[:, c, :3] = q
    return out.reshape(rows * cols, 4)


def ulp_diff(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """Distance in fp32 units in the last place between two float32 arrays."""
    def key(v):
        i = np.ascontiguousarray(v, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


def room_plane_distance(world, pts_world: np.ndarray) -> np.ndarray:
    """Distance of each world point to its nearest room plane (walls, floor, ceiling)."""
    room = np.asarray(world.room, np.float64)
    d = np.concatenate([np.abs(pts_world - room[:, 0]), np.abs(pts_world - room[:, 1])], 1)
    return d.min(1)


def se3(oracle, T34, xi):
    """T * Exp(xi) as 3x4."""
    return oracle.compose(np.asarray(T34, np.float64), oracle.expmap(np.asarray(xi, np.float64)))


def to_world(T34, pts: np.ndarray) -> np.ndarray:
    T34 = np.asarray(T34, np.float64).reshape(3, 4)
    return pts.astype(np.float64) @ T34[:, :3].T + T34[:, 3]

