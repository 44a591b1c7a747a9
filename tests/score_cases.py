"""The ranking fixture of the score tests (tests/test_score_cpu.py checks its design on the
restatement, tests/test_gpu_score.py runs FORM.dense_relocalize on it).  A scene with no
symmetry under the candidates' moves: an L-shaped wall (one arm along x, one along y, five
voxels high) plus a box near the corner's inside, every surface point at a voxel centre of a
1.0-wide grid, so every point is its voxel's representative.  The scan is the scene in the
frame of the true pose, rounded to fp32; the candidates are the true pose, the poses 2 voxels
from it along +-x and +-y, and the poses turned +-90 degrees about z."""
import functools
import math

import numpy as np

WIDTH, CAPACITY, RADIUS = 1.0, 2048, 0.4  # reach = floor(0.4 / 1.0) + 1 = 1


def _rz(a):
    c, s = math.cos(a), math.sin(a)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


@functools.lru_cache(maxsize=None)
def ranking_fixture():
    """(world points (N, 4) fp32, scan (N, 4) fp32, candidates (7, 3, 4), the truth's index)."""
    cells = set()
    for z in range(5):
        for x in range(0, 21):
            cells.add((x, 10, z))       # the arm along x
        for y in range(-10, 11):
            cells.add((20, y, z))       # the arm along y
    for x in range(5, 8):
        for y in range(0, 3):
            for z in range(0, 3):
                if x in (5, 7) or y in (0, 2) or z == 2:
                    cells.add((x, y, z))  # the box: its walls and its lid
    world = np.zeros((len(cells), 4), np.float32)
    world[:, :3] = np.array(sorted(cells), np.float64) + 0.5
    truth = np.zeros((3, 4))
    truth[:, :3] = _rz(0.3)
    truth[:, 3] = (8.2, 3.1, 1.4)
    scan = np.zeros_like(world)
    scan[:, :3] = ((world[:, :3].astype(np.float64) - truth[:, 3]) @ truth[:, :3]).astype(np.float32)
    cands = [truth.copy()]
    for d in ((2.0, 0, 0), (-2.0, 0, 0), (0, 2.0, 0), (0, -2.0, 0)):
        T = truth.copy()
        T[:, 3] += np.array(d) * WIDTH
        cands.append(T)
    for a in (math.pi / 2, -math.pi / 2):
        T = truth.copy()
        T[:, :3] = _rz(a) @ truth[:, :3]
        cands.append(T)
    order = [3, 5, 0, 1, 6, 2, 4]  # the truth is not first in the list
    cands = np.ascontiguousarray(np.array(cands)[order])
    for a in (world, scan, cands):
        a.setflags(write=False)
    return world, scan, cands, order.index(0)
