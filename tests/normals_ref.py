"""The dense map's surface normals restated (include/fmx/fmx.h, fmx_normals_build; DESIGN.md
§Dense map, Normals) over tests/nearest_ref.py's map, which it does not change.  Support, the
moments and the covariance are plain Python floats (IEEE double, one rounding per operation),
the neighbours added in ascending key order: the kernel adds them in the offset list's order,
so the moments agree to rounding, not to the bit, and only `support` and the classes are
compared with equality.  The eigen decomposition is numpy.linalg.eigh."""
import math

import numpy as np

import carve_ref as CR
import dense_ref as R
import nearest_ref as NR

INF = float("inf")
CLASSES = ("oriented", "flat_rejected", "sparse", "filtered")


def cell_of(key):
    return ((key >> 42) & 0x1FFFFF) - R.BIAS, ((key >> 21) & 0x1FFFFF) - R.BIAS, (key & 0x1FFFFF) - R.BIAS


def sign_rule(n):
    """The component of largest magnitude positive, the lowest axis among equal magnitudes."""
    a = np.abs(n)
    k = 0
    for j in (1, 2):
        if a[j] > a[k]:
            k = j
    return -n if n[k] < 0 else n


def covariance(q0, neighbours, max_dist2):
    """(support, C) of a voxel with representative q0 over the candidate representatives."""
    k, S1, S2 = 0, [0.0] * 3, [[0.0] * 3 for _ in range(3)]
    for q in neighbours:
        e = [float(q[a]) - float(q0[a]) for a in range(3)]
        d2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
        if d2 <= max_dist2:
            k += 1
            for a in range(3):
                S1[a] += e[a]
                for b in range(3):
                    S2[a][b] += e[a] * e[b]
    m = [S1[a] / k for a in range(3)]
    return k, np.array([[S2[a][b] / k - m[a] * m[b] for b in range(3)] for a in range(3)])


def classify(k, C, min_support, max_flatness):
    """(class, normal (zeros unless oriented), flatness, (l0, l1, l2)) from support and covariance."""
    lam, vec = np.linalg.eigh(C)
    l0, l1, l2 = max(float(lam[0]), 0.0), float(lam[1]), float(lam[2])
    flat = l0 / l1 if l1 > 0.0 else INF
    if k < max(int(min_support), 3):
        cls = "sparse"
    elif l1 > 0.0 and l0 <= max_flatness * l1:
        cls = "oriented"
    else:
        cls = "flat_rejected"
    n = sign_rule(vec[:, 0]) if cls == "oriented" else np.zeros(3)
    return cls, n, flat, (l0, l1, l2)


def build(ref, reach=1, max_dist=None, min_support=5, max_flatness=0.1, min_hits=1, max_miss_ratio=None, max_dist2=None,
          brute=False):
    """Every stored voxel of `ref` (a NearestRef): key -> dict(cls, support, normal, flatness,
    lams, point).  brute: the candidates are all voxels whose cell lies within `reach` on every
    axis, found by a loop over the whole map instead of over the cube."""
    num, den = CR.miss_fraction(max_miss_ratio)
    if max_dist2 is None:
        md = INF if max_dist is None else float(max_dist)
        max_dist2 = md * md
    reach = int(reach)
    if not 1 <= reach <= NR.MAX_REACH or not max_dist2 >= 0.0 or not 0.0 <= max_flatness <= 1.0:
        raise ValueError("FMX_E_INVAL")
    solid = sorted(k for k in ref.vox if ref._solid(k, min_hits, num, den))
    cells = {k: cell_of(k) for k in solid}
    out = {}
    for key, v in ref.vox.items():
        q0 = v[3]
        if key not in cells:
            out[key] = dict(cls="filtered", support=0, normal=np.zeros(3), flatness=0.0, lams=None, point=q0)
            continue
        c = cells[key]
        if brute:
            near = [k for k in solid if all(abs(cells[k][a] - c[a]) <= reach for a in range(3))]
        else:
            span = range(-reach, reach + 1)
            near = sorted(R.pack_key(c[0] + dx, c[1] + dy, c[2] + dz) for dx in span for dy in span for dz in span
                          if NR.storable((c[0] + dx, c[1] + dy, c[2] + dz)))
            near = [k for k in near if k in cells]
        k, C = covariance(q0, [ref.vox[j][3] for j in near], float(max_dist2))
        cls, n, flat, lams = classify(k, C, min_support, float(max_flatness))
        out[key] = dict(cls=cls, support=k, normal=n, flatness=flat, lams=lams, point=q0, cov=C)
    return out


def counts_of(built):
    c = dict.fromkeys(CLASSES, 0)
    for v in built.values():
        c[v["cls"]] += 1
    return c


def fixture(seed=41):
    """The issue's map at voxel width 1: three mutually orthogonal 12 x 12 patches with in-plane
    jitter and 0.02 of noise across, six isolated voxels 3 apart and an exact line of ten, (N, 4)
    float32, to be integrated at the identity."""
    g = np.random.default_rng(seed)
    rows = []
    for a in range(3):
        for i in range(12):
            for j in range(12):
                u, v = i + 1.5 + g.uniform(-0.3, 0.3), j + 1.5 + g.uniform(-0.3, 0.3)
                h = 0.5 + float(np.clip(g.normal(0.0, 0.02), -0.2, 0.2))
                p = [u, v]
                p.insert(a, h)
                rows.append(p)
    rows += [(20.5 + 3 * i, 20.5, 20.5) for i in range(6)]
    rows += [(20.5 + i, 30.5, 30.5) for i in range(10)]
    p = np.zeros((len(rows), 4), np.float32)
    p[:, :3] = np.asarray(rows, np.float32)
    return p


def flatness_bound(flat, lams):
    """|device - restated| for a flatness stored as fp32: the storage rounding (2^-22 relative;
    2^-24 for the rounding itself, the rest for the quotient's own) plus the eigenvalues'
    backward error over l1 (64 eps l2 / l1)."""
    eps = float(np.finfo(np.float64).eps)
    return 2.0 ** -22 * flat + 64.0 * eps * lams[2] / lams[1]
