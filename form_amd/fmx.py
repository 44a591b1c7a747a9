"""ctypes host layer over libfmx.so (include/fmx/fmx.h).

Mirrors the reference's Python-facing surface for this path:
  * ``KeypointExtractionParams`` / ``extract_keypoints`` — form._core
    (python/bindings.cpp:194-240): returns (planar_points, normals, point_points).
  * ``Estimator`` — form::Estimator (form/form.hpp:40-84): ``register_scan(scan)``
    returns the (planar, point) features, ``current_lidar_estimate()`` the pose.
  * ``Context`` — the stage-level seams (extract / map_build / match /
    linearize / error / insert) used by the parity tests.

There is no CPU fallback: if libfmx.so is missing or no HIP device is visible the
import or the constructor raises.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from dataclasses import dataclass, fields

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FMX_LIB", os.path.join(_HERE, "libfmx.so"))  # FMX_LIB: A/B of two builds
_LIB = None

FMX_OK = 0
_STATUS = {1: "FMX_E_INVAL", 2: "FMX_E_SIZE", 3: "FMX_E_OOM", 4: "FMX_E_HIP", 5: "FMX_E_STATE",
           6: "FMX_E_RANGE", 7: "FMX_E_RCCL"}


class FmxError(RuntimeError):
    def __init__(self, status: int, msg: str):
        super().__init__(f"{_STATUS.get(status, status)}: {msg}")
        self.status = status


class _ExtractParams(C.Structure):
    _fields_ = [
        ("neighbor_points", C.c_uint32), ("num_sectors", C.c_uint32),
        ("planar_threshold", C.c_double), ("planar_feats_per_sector", C.c_uint32),
        ("point_feats_per_sector", C.c_uint32), ("radius", C.c_double),
        ("min_points", C.c_uint32), ("min_norm_squared", C.c_double),
        ("max_norm_squared", C.c_double), ("num_columns", C.c_int32), ("num_rows", C.c_int32),
    ]


class _Params(C.Structure):
    _fields_ = [
        ("extraction", _ExtractParams), ("max_dist_matching", C.c_double),
        ("new_pose_threshold", C.c_double), ("max_num_rematches", C.c_uint32),
        ("planar_constraint_sigma", C.c_double), ("disable_smoothing", C.c_int32),
        ("max_num_keyscans", C.c_int64), ("max_steps_unused_keyscan", C.c_int64),
        ("max_num_recent_scans", C.c_uint32), ("keyscan_match_ratio", C.c_double),
        ("min_dist_map", C.c_double), ("keypoint_pool_capacity", C.c_uint64),
        ("max_pairs", C.c_uint32), ("voxel_subdivision", C.c_uint32),
    ]


class _DeskewParams(C.Structure):
    _fields_ = [("enable", C.c_int32), ("initial_twist", C.c_double * 6), ("column_fraction", C.c_void_p)]


class _OrganizeParams(C.Structure):
    _fields_ = [("enable", C.c_int32), ("row_source", C.c_int32), ("elevation", C.c_void_p),
                ("ring_to_row", C.c_void_p), ("n_rings", C.c_uint32), ("azimuth_offset", C.c_double),
                ("clockwise", C.c_int32)]


class _Cloud(C.Structure):
    _fields_ = [("xyzw", C.c_void_p), ("n", C.c_size_t), ("ring", C.c_void_p), ("sweep_fraction", C.c_void_p),
                ("on_device", C.c_int32)]


class _OrganizeCounts(C.Structure):
    _fields_ = [("placed", C.c_uint32), ("displaced", C.c_uint32), ("off_grid", C.c_uint32), ("invalid", C.c_uint32)]

    def as_dict(self):
        return dict(placed=self.placed, displaced=self.displaced, off_grid=self.off_grid, invalid=self.invalid)


class _DenseParams(C.Structure):
    _fields_ = [("enable", C.c_int32), ("voxel_width", C.c_double), ("max_voxels", C.c_uint64),
                ("min_norm_squared", C.c_double), ("max_norm_squared", C.c_double), ("every", C.c_uint32)]


class _DenseCounts(C.Structure):
    _fields_ = [("added", C.c_uint32), ("merged", C.c_uint32), ("gated", C.c_uint32), ("out_of_range", C.c_uint32),
                ("invalid", C.c_uint32)]

    def as_dict(self):
        return dict(added=self.added, merged=self.merged, gated=self.gated, out_of_range=self.out_of_range,
                    invalid=self.invalid)


class _RollParams(C.Structure):
    _fields_ = [("enable", C.c_int32), ("half", C.c_uint32 * 3), ("step", C.c_double), ("spill", C.c_int32)]


class _CarveParams(C.Structure):
    _fields_ = [("enable", C.c_int32), ("max_norm_squared", C.c_double), ("margin", C.c_uint32),
                ("ray_stride", C.c_uint32), ("every", C.c_uint32)]


class _CarveCounts(C.Structure):
    _fields_ = [("rays", C.c_uint32), ("steps", C.c_uint64), ("misses", C.c_uint64), ("exempt", C.c_uint64)]

    def as_dict(self):
        return dict(rays=int(self.rays), steps=int(self.steps), misses=int(self.misses), exempt=int(self.exempt))


class _VoxelArrays(C.Structure):
    _fields_ = [("xyz", C.c_void_p), ("scan", C.c_void_p), ("index", C.c_void_p), ("hits", C.c_void_p),
                ("misses", C.c_void_p)]


class _VoxelInput(C.Structure):
    _fields_ = [("xyz", C.c_void_p), ("scan", C.c_void_p), ("index", C.c_void_p), ("hits", C.c_void_p),
                ("misses", C.c_void_p)]


class _UploadCounts(C.Structure):
    _fields_ = [("added", C.c_uint32), ("merged", C.c_uint32), ("out_of_range", C.c_uint32), ("invalid", C.c_uint32)]

    def as_dict(self):
        return dict(added=int(self.added), merged=int(self.merged), out_of_range=int(self.out_of_range),
                    invalid=int(self.invalid))


class _ProbePointCounts(C.Structure):
    _fields_ = [("absent", C.c_uint32), ("filtered", C.c_uint32), ("solid", C.c_uint32), ("out_of_range", C.c_uint32),
                ("invalid", C.c_uint32)]

    def as_dict(self):
        return dict(absent=int(self.absent), filtered=int(self.filtered), solid=int(self.solid),
                    out_of_range=int(self.out_of_range), invalid=int(self.invalid))


class _ProbeRayCounts(C.Structure):
    _fields_ = [("hit", C.c_uint32), ("clear", C.c_uint32), ("out_of_range", C.c_uint32), ("invalid", C.c_uint32),
                ("steps", C.c_uint64)]

    def as_dict(self):
        return dict(hit=int(self.hit), clear=int(self.clear), out_of_range=int(self.out_of_range),
                    invalid=int(self.invalid), steps=int(self.steps))


class _NearestCounts(C.Structure):
    _fields_ = [("found", C.c_uint32), ("none", C.c_uint32), ("out_of_range", C.c_uint32), ("invalid", C.c_uint32),
                ("lookups", C.c_uint64)]

    def as_dict(self):
        return dict(found=int(self.found), none=int(self.none), out_of_range=int(self.out_of_range),
                    invalid=int(self.invalid), lookups=int(self.lookups))


NEAREST_MAX_REACH = 8  # FMX_NEAREST_MAX_REACH


class _AlignParams(C.Structure):
    _fields_ = [("min_hits", C.c_uint32), ("miss_num", C.c_uint32), ("miss_den", C.c_uint32), ("reach", C.c_uint32),
                ("max_dist2", C.c_double), ("sigma", C.c_double), ("stride", C.c_uint32)]


class _AlignCounts(C.Structure):
    _fields_ = [("found", C.c_uint32), ("none", C.c_uint32), ("out_of_range", C.c_uint32), ("invalid", C.c_uint32),
                ("skipped", C.c_uint32), ("lookups", C.c_uint64)]

    def as_dict(self):
        return dict(found=int(self.found), none=int(self.none), out_of_range=int(self.out_of_range),
                    invalid=int(self.invalid), skipped=int(self.skipped), lookups=int(self.lookups))


class _AlignResult(C.Structure):
    _fields_ = [("iters", C.c_uint32), ("converged", C.c_int32), ("last_step", C.c_double), ("error", C.c_double),
                ("counts", _AlignCounts)]


class _NormalsParams(C.Structure):
    _fields_ = [("min_hits", C.c_uint32), ("miss_num", C.c_uint32), ("miss_den", C.c_uint32), ("reach", C.c_uint32),
                ("max_dist2", C.c_double), ("min_support", C.c_uint32), ("max_flatness", C.c_double)]


class _NormalsCounts(C.Structure):
    _fields_ = [("oriented", C.c_uint32), ("flat_rejected", C.c_uint32), ("sparse", C.c_uint32), ("filtered", C.c_uint32),
                ("lookups", C.c_uint64)]

    def as_dict(self):
        return dict(oriented=int(self.oriented), flat_rejected=int(self.flat_rejected), sparse=int(self.sparse),
                    filtered=int(self.filtered), lookups=int(self.lookups))


class _PlaneCounts(C.Structure):
    _fields_ = [("found", C.c_uint32), ("none", C.c_uint32), ("out_of_range", C.c_uint32), ("invalid", C.c_uint32),
                ("skipped", C.c_uint32), ("unoriented", C.c_uint32), ("lookups", C.c_uint64)]

    def as_dict(self):
        return dict(found=int(self.found), none=int(self.none), out_of_range=int(self.out_of_range),
                    invalid=int(self.invalid), skipped=int(self.skipped), unoriented=int(self.unoriented),
                    lookups=int(self.lookups))


class _PlaneResult(C.Structure):
    _fields_ = [("iters", C.c_uint32), ("converged", C.c_int32), ("last_step", C.c_double), ("error", C.c_double),
                ("counts", _PlaneCounts)]


SCORE_MAX_POSES = 65536  # FMX_SCORE_MAX_POSES


class _PoseScore(C.Structure):
    _fields_ = [("found", C.c_uint32), ("none", C.c_uint32), ("out_of_range", C.c_uint32), ("invalid", C.c_uint32),
                ("sum_d2", C.c_double), ("lookups", C.c_uint64)]


# the same record as a numpy dtype: Context.score_poses hands the call an array of these
SCORE_DTYPE = np.dtype([("found", np.uint32), ("none", np.uint32), ("out_of_range", np.uint32), ("invalid", np.uint32),
                        ("sum_d2", np.float64), ("lookups", np.uint64)])
SCORE_FIELDS = SCORE_DTYPE.names


REFINE_MAX_POSES = 65536  # FMX_REFINE_MAX_POSES


class _RefineSystem(C.Structure):
    _fields_ = [("S", C.c_double * 29), ("found", C.c_uint32), ("none", C.c_uint32), ("out_of_range", C.c_uint32),
                ("invalid", C.c_uint32), ("unoriented", C.c_uint32), ("reserved", C.c_uint32), ("lookups", C.c_uint64)]


class _RefineResult(C.Structure):
    _fields_ = [("iters", C.c_uint32), ("converged", C.c_int32), ("singular", C.c_int32), ("reserved", C.c_uint32),
                ("last_step", C.c_double), ("error", C.c_double), ("found", C.c_uint32), ("none", C.c_uint32),
                ("out_of_range", C.c_uint32), ("invalid", C.c_uint32), ("unoriented", C.c_uint32),
                ("reserved2", C.c_uint32), ("lookups", C.c_uint64)]


# the same records as numpy dtypes: Context.refine_systems / refine_poses hand the calls arrays of these
REFINE_SYSTEM_DTYPE = np.dtype([("system", np.float64, (29,)), ("found", np.uint32), ("none", np.uint32),
                                ("out_of_range", np.uint32), ("invalid", np.uint32), ("unoriented", np.uint32),
                                ("reserved", np.uint32), ("lookups", np.uint64)])
REFINE_RESULT_DTYPE = np.dtype([("iters", np.uint32), ("converged", np.int32), ("singular", np.int32),
                                ("reserved", np.uint32), ("last_step", np.float64), ("error", np.float64),
                                ("found", np.uint32), ("none", np.uint32), ("out_of_range", np.uint32),
                                ("invalid", np.uint32), ("unoriented", np.uint32), ("reserved2", np.uint32),
                                ("lookups", np.uint64)])
REFINE_SYSTEM_FIELDS = tuple(k for k in REFINE_SYSTEM_DTYPE.names if k != "reserved")
REFINE_RESULT_FIELDS = tuple(k for k in REFINE_RESULT_DTYPE.names if not k.startswith("reserved"))


# FORM.dense_localize(plane=True) and FORM.dense_normals build the snapshot with these when it is
# not current: the 3 x 3 x 3 cells around a voxel, at least 5 neighbours, l0 <= 0.1 l1
NORMALS_DEFAULTS = dict(reach=1, max_dist=None, min_support=5, max_flatness=0.1)


# fmx_probe_points / fmx_probe_rays: the per-point state
PROBE_ABSENT, PROBE_FILTERED, PROBE_SOLID, PROBE_OUT_OF_RANGE, PROBE_INVALID = range(5)
PROBE_NO_STEP = 0xFFFFFFFF


def fitness_of(state, dist2) -> dict:
    """FORM.dense_fitness's figures from a nearest_voxels result's state and dist2."""
    state = np.asarray(state)
    found = state == PROBE_SOLID
    n_valid = int(found.sum() + (state == PROBE_ABSENT).sum())
    n_found = int(found.sum())
    total = math.fsum(float(d) for d in np.asarray(dist2, np.float64)[found])  # in index order
    return dict(n_valid=n_valid, n_found=n_found, fitness=n_found / n_valid if n_valid else 0.0,
                rmse=math.sqrt(total / n_found) if n_found else 0.0)


def miss_fraction(max_miss_ratio):
    """(miss_num, miss_den) of a download's miss filter misses * miss_den <= hits * miss_num:
    (0, 0), no filter, for None; else the ratio in 1/65536ths, rounded to nearest (0.5 is
    32768 / 65536), at most 65535."""
    if max_miss_ratio is None:
        return 0, 0
    r = float(max_miss_ratio)
    if not (r >= 0.0):
        raise ValueError("max_miss_ratio must be a number >= 0")
    return int(min(math.floor(r * 65536.0 + 0.5), float((1 << 32) - 1))), 1 << 16


class _Counts(C.Structure):
    _fields_ = [("planar", C.c_uint32), ("point", C.c_uint32), ("planar_selected", C.c_uint32)]


def lib():
    """Load libfmx.so (raises if it has not been built)."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} missing: run __graft_entry__.build() (make -C form_amd/csrc)")
        L = C.CDLL(LIB_PATH)
        L.fmx_last_error.restype = C.c_char_p
        L.fmx_profile_name.restype = C.c_char_p
        _LIB = L
    return _LIB


EXPORTED = [
    "fmx_abi_version", "fmx_default_params", "fmx_create", "fmx_destroy", "fmx_last_error",
    "fmx_extract", "fmx_extract_download", "fmx_set_queries", "fmx_set_queries_device", "fmx_keypoints_add",
    "fmx_keypoints_add_device",
    "fmx_keypoints_remove", "fmx_map_build", "fmx_match", "fmx_match_download", "fmx_map_insert",
    "fmx_corr_set", "fmx_linearize", "fmx_error", "fmx_linearize_matched", "fmx_register_scan", "fmx_next_scan",
    "fmx_current_pose",
    "fmx_last_stats", "fmx_match_work", "fmx_profile_enable", "fmx_profile_reset", "fmx_profile_count",
    "fmx_profile_name", "fmx_profile_read", "fmx_sync", "fmx_comm_unique_id", "fmx_comm_init",
    "fmx_map_download", "fmx_register_points", "fmx_scan_buffer", "fmx_match_cert", "fmx_profile_match_work",
    "fmx_corr_generation", "fmx_moments", "fmx_moments_contract",
    "fmx_deskew_configure", "fmx_deskew_set_twist", "fmx_deskew_last", "fmx_deskew",
    "fmx_organize_configure", "fmx_organize", "fmx_register_cloud", "fmx_deskew_cells",
    "fmx_corr_download", "fmx_pair_sort_plan",
    "fmx_dense_configure", "fmx_dense_integrate", "fmx_dense_last", "fmx_dense_stats", "fmx_dense_download",
    "fmx_dense_clear",
    "fmx_roll_configure", "fmx_roll_count", "fmx_roll_evict", "fmx_roll_drain", "fmx_roll_stats",
    "fmx_carve_configure", "fmx_carve_rays", "fmx_carve_last", "fmx_carve_download", "fmx_carve_evict",
    "fmx_carve_drain",
    "fmx_probe_points", "fmx_probe_rays",
    "fmx_upload_voxels",
    "fmx_nearest_voxels",
    "fmx_align_system", "fmx_align_dense",
    "fmx_normals_build", "fmx_normals_stats", "fmx_normals_download",
    "fmx_plane_system", "fmx_plane_align",
    "fmx_score_poses", "fmx_score_plan",
    "fmx_refine_systems", "fmx_refine_poses", "fmx_refine_plan",
]

PAIR_SORT_FORMS = ("none", "per-block", "tail-scanned", "scatter-scanned")


def pair_sort_plan(n_planar: int, n_point: int, K: int, sorted: bool = True) -> dict:
    """fmx_pair_sort_plan (host only, no context): the form the pair sort of such a match
    takes (form_amd/csrc/pair_sort_plan.hpp)."""
    out = np.zeros(8, np.uint32)
    st = lib().fmx_pair_sort_plan(C.c_uint32(n_planar), C.c_uint32(n_point), C.c_uint32(K), C.c_int(int(sorted)),
                                  _p(out))
    if st != FMX_OK:
        raise FmxError(st, "fmx_pair_sort_plan")
    keys = ("group", "form", "nb_pl", "nb_pt", "ntl_pl", "ntl_pt", "hist_words", "scan_launches")
    plan = {k: int(v) for k, v in zip(keys, out)}
    plan["form"] = PAIR_SORT_FORMS[plan["form"]]
    return plan


def score_plan(n_points: int, stride: int = 1, n_poses: int = 1) -> dict:
    """fmx_score_plan (host only, no context): the tiling and chunking of such a
    Context.score_poses call (form_amd/csrc/score_host.hpp): kept (points), tile (points per
    tile), tiles (per pose), chunk (poses per chunk), chunks (of this call), cap (the grid's,
    in blocks)."""
    out = np.zeros(6, np.uint32)
    st = lib().fmx_score_plan(C.c_uint64(n_points), C.c_uint32(stride), C.c_uint32(n_poses), _p(out))
    if st != FMX_OK:
        raise FmxError(st, "fmx_score_plan")
    return {k: int(v) for k, v in zip(("kept", "tile", "tiles", "chunk", "chunks", "cap"), out)}


def refine_plan(n_points: int, stride: int = 1, n_poses: int = 1) -> dict:
    """fmx_refine_plan (host only, no context): the tiling and chunking of such a
    Context.refine_systems call (form_amd/csrc/refine_host.hpp), score_plan's six figures."""
    out = np.zeros(6, np.uint32)
    st = lib().fmx_refine_plan(C.c_uint64(n_points), C.c_uint32(stride), C.c_uint32(n_poses), _p(out))
    if st != FMX_OK:
        raise FmxError(st, "fmx_refine_plan")
    return {k: int(v) for k, v in zip(("kept", "tile", "tiles", "chunk", "chunks", "cap"), out)}


def rank_scores(scores) -> np.ndarray:
    """The candidates of a Context.score_poses result by rank: found descending, then sum_d2
    ascending, then the index ascending (integers and doubles compared, nothing computed;
    score_host.hpp restates it).  Returns the indices, (K,) int64."""
    found = np.asarray(scores["found"], np.int64)
    d2 = np.asarray(scores["sum_d2"], np.float64)
    return np.lexsort((np.arange(len(found)), d2, -found)).astype(np.int64)


def pose_grid(centre34, half_xyz=(0.0, 0.0, 0.0), step_xyz=(1.0, 1.0, 1.0), half_yaw: float = 0.0,
              step_yaw: float = 1.0) -> np.ndarray:
    """Candidate poses on a grid around a centre pose [R_c | t_c] (3 x 4 or 4 x 4), on the
    host: [Rz(psi) R_c | t_c + d] for psi = j * step_yaw, |j| <= floor(half_yaw / step_yaw),
    and d_k = i_k * step_xyz[k], |i_k| <= floor(half_xyz[k] / step_xyz[k]) (a half of 0, or a
    step that is not positive: that axis stays at the centre).  Nesting, outermost first: yaw,
    x, y, z, each ascending; the centre is always among the candidates (every index 0).
    Returns (K, 3, 4) float64; ValueError past SCORE_MAX_POSES."""
    Tc = np.asarray(centre34, np.float64).reshape(-1, 4)[:3]

    def steps(half, step):
        half, step = float(half), float(step)
        if not (half >= 0.0) or math.isinf(half):
            raise ValueError("a half-extent must be a finite number >= 0")
        m = int(math.floor(half / step + 1e-9)) if step > 0.0 and half > 0.0 else 0
        return [i * step for i in range(-m, m + 1)]

    yaws = steps(half_yaw, step_yaw)
    dx, dy, dz = (steps(h, s) for h, s in zip(half_xyz, step_xyz))
    total = len(yaws) * len(dx) * len(dy) * len(dz)
    if total > SCORE_MAX_POSES:
        raise ValueError(f"{total} candidates: more than SCORE_MAX_POSES ({SCORE_MAX_POSES})")
    out = np.empty((total, 3, 4), np.float64)
    k = 0
    for psi in yaws:
        c, sn = math.cos(psi), math.sin(psi)
        Rm = np.array([[c, -sn, 0.0], [sn, c, 0.0], [0.0, 0.0, 1.0]]) @ Tc[:, :3] if psi != 0.0 else Tc[:, :3]
        for x in dx:
            for y in dy:
                for z in dz:
                    out[k, :, :3] = Rm
                    out[k, :, 3] = Tc[:, 3] + np.array([x, y, z]) if (x, y, z) != (0.0, 0.0, 0.0) else Tc[:, 3]
                    k += 1
    return out


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


_NO_ENTRIES = np.zeros(1, np.uint64)  # a non-NULL address for an array of no entries (never read)


def _host(a):
    """A host array of a numpy array or CPU tensor."""
    return a.numpy() if hasattr(a, "numpy") and not isinstance(a, np.ndarray) else a


def _ready(*tensors):
    """Device tensors handed to a context's stream: wait for the torch stream that
    produced them (fmx copies them on its own stream, unordered with torch's)."""
    import torch
    for t in tensors:
        if t is not None and t.is_cuda:
            torch.cuda.current_stream(t.device).synchronize()
            return


@dataclass
class KeypointExtractionParams:
    """form::FeatureExtractor::Params (extraction.hpp:59-88); same names as the
    nanobind class KeypointExtractionParams (bindings.cpp:194-211)."""
    neighbor_points: int = 5
    num_sectors: int = 6
    planar_threshold: float = 1.0
    planar_feats_per_sector: int = 50
    point_feats_per_sector: int = 3
    radius: float = 1.0
    min_points: int = 5
    min_norm_squared: float = 1.0
    max_norm_squared: float = 100.0 * 100.0
    num_columns: int = 1024
    num_rows: int = 64

    def as_dict(self):
        return {f.name: getattr(self, f.name) for f in fields(self)}


@dataclass
class EstimatorParams:
    """form::Estimator::Params (form.hpp:42-56), flattened like the evalio YAML keys
    (bindings.cpp:66-88)."""
    extraction: KeypointExtractionParams = None
    max_dist_matching: float = 0.8
    new_pose_threshold: float = 1e-4
    max_num_rematches: int = 30
    planar_constraint_sigma: float = 0.1
    disable_smoothing: bool = False  # constraints.hpp:56 (True: single-pose ablation)
    max_num_keyscans: int = 50
    max_steps_unused_keyscan: int = 10
    max_num_recent_scans: int = 10
    keyscan_match_ratio: float = 0.1
    min_dist_map: float = 0.1
    keypoint_pool_capacity: int = 4 << 20
    max_pairs: int = 1024
    voxel_subdivision: int = 1

    def __post_init__(self):
        if self.extraction is None:
            self.extraction = KeypointExtractionParams()

    def to_c(self) -> _Params:
        p = _Params()
        lib().fmx_default_params(C.byref(p))
        for k, v in self.extraction.as_dict().items():
            setattr(p.extraction, k, v)
        for f in fields(self):
            if f.name != "extraction":
                setattr(p, f.name, int(getattr(self, f.name)) if isinstance(getattr(self, f.name), bool)
                        else getattr(self, f.name))
        return p


class Context:
    """One fmx context (one HIP device + stream).  Thin, stage-level API."""

    def __init__(self, params: EstimatorParams | None = None, device: int = 0):
        self.params = params or EstimatorParams()
        self._L = lib()
        h = C.c_void_p()
        st = self._L.fmx_create(C.byref(self.params.to_c()), C.c_int(device), C.byref(h))
        if st != FMX_OK:
            raise FmxError(st, "fmx_create failed (is a HIP device visible?)")
        self.h = h
        self.K = 0
        self.n_planar = 0
        self.n_point = 0

    def close(self):
        if getattr(self, "h", None):
            self._L.fmx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, st: int):
        if st != FMX_OK:
            raise FmxError(st, self._L.fmx_last_error(self.h).decode())

    # ---------------------------------------------------------------- stage 1
    def extract(self, scan, scan_idx: int = 0):
        """scan: (N, 4) float32 numpy array (host) or torch tensor (host or device)."""
        on_dev, ptr, n, keep = _scan_ptr(scan)
        c = _Counts()
        self._chk(self._L.fmx_extract(self.h, ptr, C.c_size_t(n), C.c_uint64(scan_idx),
                                      C.c_int(on_dev), C.byref(c)))
        del keep
        self.n_planar, self.n_point = c.planar, c.point
        return c.planar, c.point, c.planar_selected

    def extract_download(self, with_mask: bool = False):
        npl, npt = self.n_planar, self.n_point
        planar = np.zeros((npl, 6), np.float32)
        pidx = np.zeros(npl, np.uint32)
        point = np.zeros((npt, 3), np.float32)
        tidx = np.zeros(npt, np.uint32)
        e = self.params.extraction
        mask = np.zeros(e.num_rows * e.num_columns, np.uint8) if with_mask else None
        self._chk(self._L.fmx_extract_download(self.h, _p(planar), _p(pidx), _p(point), _p(tidx), _p(mask)))
        out = dict(planar=planar, planar_index=pidx, point=point, point_index=tidx)
        if with_mask:
            out["planar_mask"] = mask.astype(bool)
        return out

    def set_queries(self, planar: np.ndarray, point: np.ndarray, scan_idx: int = 0):
        planar = np.ascontiguousarray(planar, np.float32).reshape(-1, 6)
        point = np.ascontiguousarray(point, np.float32).reshape(-1, 3)
        self._chk(self._L.fmx_set_queries(self.h, C.c_uint64(scan_idx), _p(planar), C.c_uint32(len(planar)),
                                          _p(point), C.c_uint32(len(point))))
        self.n_planar, self.n_point = len(planar), len(point)

    def set_queries_device(self, planar_pos4, planar_nrm4, point_pos4=None, scan_idx: int = 0):
        """Device-resident queries: (N,4) float32 CUDA tensors."""
        npt = 0 if point_pos4 is None else point_pos4.shape[0]
        pp = C.c_void_p(point_pos4.data_ptr()) if npt else None
        _ready(planar_pos4, planar_nrm4, point_pos4)
        self._chk(self._L.fmx_set_queries_device(self.h, C.c_uint64(scan_idx), C.c_void_p(planar_pos4.data_ptr()),
                                                 C.c_void_p(planar_nrm4.data_ptr()), C.c_uint32(planar_pos4.shape[0]),
                                                 pp, C.c_uint32(npt)))
        self.n_planar, self.n_point = planar_pos4.shape[0], npt

    # ---------------------------------------------------------------- stage 2
    def keypoints_add_device(self, scan_idx: int, planar_pos4, planar_nrm4, point_pos4=None):
        npt = 0 if point_pos4 is None else point_pos4.shape[0]
        pp = C.c_void_p(point_pos4.data_ptr()) if npt else None
        _ready(planar_pos4, planar_nrm4, point_pos4)
        self._chk(self._L.fmx_keypoints_add_device(self.h, C.c_uint64(scan_idx), C.c_void_p(planar_pos4.data_ptr()),
                                                   C.c_void_p(planar_nrm4.data_ptr()), C.c_uint32(planar_pos4.shape[0]),
                                                   pp, C.c_uint32(npt)))

    def keypoints_add(self, scan_idx: int, planar: np.ndarray, point: np.ndarray):
        planar = np.ascontiguousarray(planar, np.float32).reshape(-1, 6)
        point = np.ascontiguousarray(point, np.float32).reshape(-1, 3)
        self._chk(self._L.fmx_keypoints_add(self.h, C.c_uint64(scan_idx), _p(planar), C.c_uint32(len(planar)),
                                            _p(point), C.c_uint32(len(point))))

    def keypoints_remove(self, scan_idx: int):
        self._chk(self._L.fmx_keypoints_remove(self.h, C.c_uint64(scan_idx)))

    def map_build(self, scans, poses34, voxel_width: float):
        scans = np.ascontiguousarray(scans, np.uint64)
        poses = np.ascontiguousarray(poses34, np.float64).reshape(-1, 12)
        self._chk(self._L.fmx_map_build(self.h, _p(scans), _p(poses), C.c_uint32(len(scans)),
                                        C.c_double(voxel_width)))
        self.K = len(scans)

    def match(self, pose_j34, max_dist: float, counts: bool = True):
        """fmx_match; counts=False returns None without waiting for the kernel."""
        pose = np.ascontiguousarray(pose_j34, np.float64).reshape(12)
        if not counts:
            self._chk(self._L.fmx_match(self.h, _p(pose), C.c_double(max_dist), None, None))
            return None
        cpl = np.zeros(max(self.K, 1), np.uint32)
        cpt = np.zeros(max(self.K, 1), np.uint32)
        self._chk(self._L.fmx_match(self.h, _p(pose), C.c_double(max_dist), _p(cpl), _p(cpt)))
        return cpl[:self.K], cpt[:self.K]

    def match_download(self):
        nq = self.n_planar + self.n_point
        pair = np.zeros(nq, np.int32)
        d2 = np.zeros(nq, np.float64)
        pi = np.zeros((nq, 3), np.float64)
        ni = np.zeros((self.n_planar, 3), np.float64)
        self._chk(self._L.fmx_match_download(self.h, _p(pair), _p(d2), _p(pi), _p(ni)))
        return dict(pair=pair, d2=d2, pi=pi, ni=ni)

    def map_insert(self, min_dist_map: float | None = None):
        n = np.zeros(2, np.uint32)
        md = self.params.min_dist_map if min_dist_map is None else min_dist_map
        self._chk(self._L.fmx_map_insert(self.h, C.c_double(md), _p(n)))
        return int(n[0]), int(n[1])

    # ---------------------------------------------------------------- stage 3
    def corr_set(self, n_plane, plane_pi, plane_ni, plane_pj, n_point, point_pi, point_pj):
        n_plane = np.ascontiguousarray(n_plane, np.uint32)
        n_point = np.ascontiguousarray(n_point, np.uint32)
        arrs = [np.ascontiguousarray(a, np.float64).reshape(-1, 3) for a in
                (plane_pi, plane_ni, plane_pj, point_pi, point_pj)]
        self._chk(self._L.fmx_corr_set(self.h, C.c_uint32(len(n_plane)), _p(n_plane), _p(arrs[0]), _p(arrs[1]),
                                       _p(arrs[2]), _p(n_point), _p(arrs[3]), _p(arrs[4])))
        self.K = len(n_plane)

    def corr_download(self):
        """fmx_corr_download: the pair-major correspondences as the device holds them (after
        a sorted match or corr_set): per-pair counts and first rows per type, the chunk table
        and the rows in device order."""
        f = self._L.fmx_corr_download
        z = C.c_uint32(0)
        sizes = np.zeros(4, np.uint32)
        self._chk(f(self.h, _p(sizes), None, None, None, z, None, z, None, None, None, z, None, None, z))
        K, nch, n_pl, n_pt = (int(v) for v in sizes)
        counts = np.zeros(2 * K, np.uint32)
        base = np.zeros(2 * K, np.uint32)
        chunk_range = np.zeros(K + 1, np.uint32)
        chunks = np.zeros((nch, 4), np.uint32)
        pl = [np.zeros((n_pl, 3), np.float64) for _ in range(3)]
        pt = [np.zeros((n_pt, 3), np.float64) for _ in range(2)]
        self._chk(f(self.h, _p(sizes), _p(counts), _p(base), _p(chunk_range), C.c_uint32(K), _p(chunks),
                    C.c_uint32(nch), _p(pl[0]), _p(pl[1]), _p(pl[2]), C.c_uint32(n_pl), _p(pt[0]), _p(pt[1]),
                    C.c_uint32(n_pt)))
        return dict(counts_plane=counts[:K], counts_point=counts[K:], base_plane=base[:K], base_point=base[K:],
                    chunk_range=chunk_range, n_chunks=int(sizes[1]), chunks=chunks, plane_pi=pl[0], plane_ni=pl[1],
                    plane_pj=pl[2], point_pi=pt[0], point_pj=pt[1])

    def linearize(self, poses_i, poses_j, sigma: float = 0.1, single: bool = False):
        pi_ = np.ascontiguousarray(poses_i, np.float64).reshape(-1, 12)
        pj_ = np.ascontiguousarray(poses_j, np.float64).reshape(-1, 12)
        G = np.zeros((max(self.K, 1), 28 if single else 91))
        err = np.zeros(max(self.K, 1))
        self._chk(self._L.fmx_linearize(self.h, _p(pi_), _p(pj_), C.c_double(sigma), C.c_int(int(single)),
                                        _p(G), _p(err)))
        return G[:self.K], err[:self.K]

    def error(self, poses_i, poses_j, sigma: float = 0.1):
        pi_ = np.ascontiguousarray(poses_i, np.float64).reshape(-1, 12)
        pj_ = np.ascontiguousarray(poses_j, np.float64).reshape(-1, 12)
        err = np.zeros(max(self.K, 1))
        self._chk(self._L.fmx_error(self.h, _p(pi_), _p(pj_), C.c_double(sigma), _p(err)))
        return err[:self.K]

    def linearize_matched(self, pose_j34, sigma: float = 0.1):
        """Single-pose 7x7 system (28 packed) summed over every accepted match of the
        last match at pose_j, and its error."""
        pose = np.ascontiguousarray(pose_j34, np.float64).reshape(12)
        out = np.zeros(29)
        self._chk(self._L.fmx_linearize_matched(self.h, _p(pose), C.c_double(sigma), _p(out)))
        return out[:28].copy(), float(out[28])

    def register_points(self, pose_init34, max_dist: float, sigma: float = 0.1, max_iters: int = 30,
                        threshold: float = 1e-4):
        """fmx_register_points: Gauss-Newton ICP of the query set against the built map
        (match + summed 7x7 + solve per iteration, all in libfmx).  Returns (pose 3x4,
        iterations)."""
        T0 = np.ascontiguousarray(pose_init34, np.float64).reshape(12)
        T = np.zeros(12)
        it = C.c_uint32(0)
        self._chk(self._L.fmx_register_points(self.h, _p(T0), C.c_double(max_dist), C.c_double(sigma),
                                              C.c_uint32(max_iters), C.c_double(threshold), _p(T), C.byref(it)))
        return T.reshape(3, 4), int(it.value)

    # ---------------------------------------------------------------- multi-GPU
    def comm_init(self, unique_id: bytes, nranks: int, rank: int):
        """Attach an RCCL communicator (see comm_unique_id): linearization sums are then
        all-reduced over the ranks on the device, on this context's stream."""
        buf = (C.c_uint8 * 128).from_buffer_copy(unique_id)
        self._chk(self._L.fmx_comm_init(self.h, buf, C.c_int(nranks), C.c_int(rank)))

    # ---------------------------------------------------------------- estimator
    def register_scan(self, scan):
        on_dev, ptr, n, keep = _scan_ptr(scan)
        c = _Counts()
        self._chk(self._L.fmx_register_scan(self.h, ptr, C.c_size_t(n), C.c_int(on_dev), C.byref(c)))
        del keep
        self.n_planar, self.n_point = c.planar, c.point
        return c.planar, c.point

    def scan_buffer(self, n: int | None = None) -> np.ndarray:
        """fmx_scan_buffer: a context-owned page-locked (n, 4) float32 buffer (default:
        rows * cols points) to assemble a scan in; registered or announced as a host scan
        it is DMA'd without a staging copy.  Buffers rotate over three: the array
        returned here aliases the one returned by the third next call."""
        e = self.params.extraction
        n = n or e.num_rows * e.num_columns
        p = C.c_void_p()
        self._chk(self._L.fmx_scan_buffer(self.h, C.c_size_t(n), C.byref(p)))
        a = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_float)), shape=(n, 4))
        # the memory belongs to the context: the array keeps the Context alive (a view
        # whose base holds it).  It is invalid after close() and after a later
        # scan_buffer call that asks for more points than this buffer holds.
        return np.asarray(_CtxBuffer(a, self))

    def next_scan(self, scan):
        """fmx_next_scan: announce the scan that follows the one the next register_scan
        receives — a contiguous (N, 4) float32 CUDA tensor, or a host array / tensor (its
        staging copy then starts at once, in the background) — left unchanged until its
        own register_scan; that call extracts it while registering.  None withdraws."""
        if scan is None:
            self._chk(self._L.fmx_next_scan(self.h, None, C.c_size_t(0), C.c_int(0)))
            return
        on_dev, ptr, n, keep = _scan_ptr(scan)
        # a converted copy would not be the memory later registered
        same = (keep is scan) if not isinstance(scan, np.ndarray) else (
            keep.__array_interface__["data"][0] == scan.__array_interface__["data"][0])
        if not same:
            raise ValueError("next_scan needs a contiguous (N, 4) float32 array or tensor")
        self._chk(self._L.fmx_next_scan(self.h, ptr, C.c_size_t(n), C.c_int(on_dev)))
        # the tensor must outlive the extraction queued for it
        self._pf_keep = (getattr(self, "_pf_keep", (None, None))[1], scan)

    # ---------------------------------------------------------------- deskewing
    def deskew_configure(self, enable: bool = True, initial_twist=None, column_fraction=None):
        """fmx_deskew_configure (before the first register_scan): constant-velocity
        deskewing of every registered scan to mid-sweep.  initial_twist: [w; v] per scan
        period for the scans without two predecessors (default 0); column_fraction:
        per-column sweep fractions in [0, 1] (default c / cols)."""
        p = _DeskewParams()
        p.enable = int(bool(enable))
        xi = np.zeros(6) if initial_twist is None else np.ascontiguousarray(initial_twist, np.float64).reshape(6)
        for k in range(6):
            p.initial_twist[k] = float(xi[k])
        frac = None
        if column_fraction is not None:
            frac = np.ascontiguousarray(column_fraction, np.float32).reshape(-1)
            if len(frac) != self.params.extraction.num_columns:
                raise ValueError("column_fraction needs one value per scan column")
            p.column_fraction = frac.ctypes.data
        self._chk(self._L.fmx_deskew_configure(self.h, C.byref(p)))
        del frac

    def deskew_set_twist(self, twist):
        """fmx_deskew_set_twist: the twist ([w; v] per scan period, e.g. integrated IMU /
        wheel odometry) the next register_scan deskews with, once."""
        xi = np.ascontiguousarray(twist, np.float64).reshape(6)
        self._chk(self._L.fmx_deskew_set_twist(self.h, _p(xi)))

    def deskew_last(self):
        """fmx_deskew_last: (twist (6,), source) of the last register_scan; source 0
        none/off, 1 initial, 2 constant velocity, 3 caller."""
        xi = np.zeros(6)
        src = C.c_int(0)
        self._chk(self._L.fmx_deskew_last(self.h, _p(xi), C.byref(src)))
        return xi, int(src.value)

    def deskew(self, scan, twist, out=None):
        """fmx_deskew: one rows * cols scan moved to mid-sweep by `twist` with the
        registration's kernel.  A CUDA tensor gives a new CUDA tensor (or fills `out`, a
        CUDA tensor of the same shape); host input gives a numpy array."""
        on_dev, ptr, n, keep = _scan_ptr(scan)
        xi = np.ascontiguousarray(twist, np.float64).reshape(6)
        if on_dev:
            import torch
            res = torch.empty_like(keep) if out is None else out
            if not (res.is_cuda and res.is_contiguous() and res.dtype == keep.dtype and res.shape == keep.shape):
                raise ValueError("out must be a contiguous (N, 4) float32 CUDA tensor")
            _ready(keep, res)
            optr = C.c_void_p(res.data_ptr())
        else:
            res = np.empty((n, 4), np.float32) if out is None else out
            if not (isinstance(res, np.ndarray) and res.dtype == np.float32 and res.shape == (n, 4)
                    and res.flags.c_contiguous):
                raise ValueError("out must be a contiguous (N, 4) float32 array")
            optr = _p(res)
        self._chk(self._L.fmx_deskew(self.h, ptr, C.c_size_t(n), C.c_int(on_dev), _p(xi), optr, C.c_int(on_dev)))
        del keep
        return res

    def deskew_cells(self, scan, fraction, twist, out=None):
        """fmx_deskew_cells: as deskew, with one sweep fraction per point of the rows * cols
        scan ((N,) float32, host or device like the scan) instead of one per column."""
        on_dev, ptr, n, keep = _scan_ptr(scan)
        xi = np.ascontiguousarray(twist, np.float64).reshape(6)
        if on_dev:
            import torch
            fr = torch.as_tensor(fraction, dtype=torch.float32, device=keep.device).reshape(-1).contiguous()
            res = torch.empty_like(keep) if out is None else out
            if not (res.is_cuda and res.is_contiguous() and res.dtype == keep.dtype and res.shape == keep.shape):
                raise ValueError("out must be a contiguous (N, 4) float32 CUDA tensor")
            _ready(keep, fr, res)
            fptr, optr = C.c_void_p(fr.data_ptr()), C.c_void_p(res.data_ptr())
        else:
            fr = np.ascontiguousarray(_host(fraction), np.float32).reshape(-1)
            res = np.empty((n, 4), np.float32) if out is None else out
            if not (isinstance(res, np.ndarray) and res.dtype == np.float32 and res.shape == (n, 4)
                    and res.flags.c_contiguous):
                raise ValueError("out must be a contiguous (N, 4) float32 array")
            fptr, optr = _p(fr), _p(res)
        if len(fr) != n:
            raise ValueError("deskew_cells needs one fraction per point")
        self._chk(self._L.fmx_deskew_cells(self.h, ptr, C.c_size_t(n), C.c_int(on_dev), fptr, _p(xi), optr,
                                           C.c_int(on_dev)))
        del keep, fr
        return res

    # ---------------------------------------------------------------- unorganized clouds
    def organize_configure(self, enable: bool = True, elevation=None, ring_to_row=None,
                           azimuth_offset: float = 0.0, clockwise: bool = False):
        """fmx_organize_configure (before the first registration): accept unordered clouds.
        elevation: rows angles in radians, strictly monotonic -> elevation mode; else ring
        mode with row = ring_to_row[ring] (None: identity).  azimuth_offset: the azimuth of
        the centre of column 0."""
        p = _OrganizeParams()
        p.enable = int(bool(enable))
        p.azimuth_offset = float(azimuth_offset)
        p.clockwise = int(bool(clockwise))
        el = r2r = None
        if elevation is not None:
            el = np.ascontiguousarray(elevation, np.float64).reshape(-1)
            if len(el) != self.params.extraction.num_rows:
                raise ValueError("elevation needs one angle per scan row")
            p.row_source = 1
            p.elevation = el.ctypes.data
        elif ring_to_row is not None:
            r2r = np.ascontiguousarray(ring_to_row, np.int32).reshape(-1)
            p.ring_to_row = r2r.ctypes.data
            p.n_rings = len(r2r)
        self._chk(self._L.fmx_organize_configure(self.h, C.byref(p)))
        del el, r2r

    def _cloud(self, xyzw, ring, sweep_fraction):
        """(fmx_cloud, keepalive) of numpy arrays or torch tensors: (N, 4) float32 points,
        (N,) uint16 rings and (N,) float32 sweep fractions (either may be None), all host
        or all device like the points."""
        on_dev, ptr, n, keep = _scan_ptr(xyzw)
        cl = _Cloud()
        cl.n = n
        cl.on_device = on_dev
        keeps = [keep]
        if n == 0:  # an empty cloud carries no arrays
            return cl, keeps
        cl.xyzw = ptr
        if on_dev:
            import torch
            if ring is not None:
                # 16-bit rings travel as int16 (the same bits): torch's uint16 support is thin
                if isinstance(ring, np.ndarray):
                    ring = torch.from_numpy(np.ascontiguousarray(ring, np.uint16).view(np.int16))
                r = ring if ring.dtype in (torch.int16, torch.uint16) else ring.to(torch.int16)
                r = r.to(keep.device).reshape(-1).contiguous()
                keeps.append(r)
                cl.ring = r.data_ptr()
            if sweep_fraction is not None:
                f = torch.as_tensor(sweep_fraction, dtype=torch.float32, device=keep.device).reshape(-1).contiguous()
                keeps.append(f)
                cl.sweep_fraction = f.data_ptr()
            _ready(*keeps)
        else:
            if ring is not None:
                r = np.ascontiguousarray(_host(ring), np.uint16).reshape(-1)
                keeps.append(r)
                cl.ring = r.ctypes.data
            if sweep_fraction is not None:
                f = np.ascontiguousarray(_host(sweep_fraction), np.float32).reshape(-1)
                keeps.append(f)
                cl.sweep_fraction = f.ctypes.data
        if any(len(k) != n for k in keeps[1:]):
            raise ValueError("ring and sweep_fraction need one value per point")
        return cl, keeps

    def organize(self, xyzw, ring=None, sweep_fraction=None):
        """fmx_organize: (scan (rows * cols, 4) float32, index (rows * cols,) uint32,
        fraction (rows * cols,) float32 or None without sweep fractions, counts dict) of
        one cloud.  Device tensors give device tensors (the index as int64), host input
        gives numpy arrays."""
        cl, keeps = self._cloud(xyzw, ring, sweep_fraction)
        e = self.params.extraction
        cells = e.num_rows * e.num_columns
        have_f = sweep_fraction is not None and cl.n > 0
        cnt = _OrganizeCounts()
        if cl.on_device:
            import torch
            dev = keeps[0].device
            scan = torch.empty((cells, 4), dtype=torch.float32, device=dev)
            idx = torch.empty(cells, dtype=torch.int32, device=dev)
            fr = torch.empty(cells, dtype=torch.float32, device=dev) if have_f else None
            ptrs = [C.c_void_p(t.data_ptr()) if t is not None else None for t in (scan, idx, fr)]
        else:
            scan = np.empty((cells, 4), np.float32)
            idx = np.empty(cells, np.uint32)
            fr = np.empty(cells, np.float32) if have_f else None
            ptrs = [_p(scan), _p(idx), _p(fr)]
        self._chk(self._L.fmx_organize(self.h, C.byref(cl), ptrs[0], C.c_int(cl.on_device), ptrs[1], ptrs[2],
                                       C.byref(cnt)))
        del keeps
        if cl.on_device:
            idx = idx.to(torch.int64) & 0xFFFFFFFF
        return scan, idx, fr, cnt.as_dict()

    def register_cloud(self, xyzw, ring=None, sweep_fraction=None):
        """fmx_register_cloud: organize the cloud on the device and register it.  Returns
        (planar, point, organize counts dict)."""
        cl, keeps = self._cloud(xyzw, ring, sweep_fraction)
        c = _Counts()
        cnt = _OrganizeCounts()
        self._chk(self._L.fmx_register_cloud(self.h, C.byref(cl), C.byref(c), C.byref(cnt)))
        del keeps
        self.n_planar, self.n_point = c.planar, c.point
        return c.planar, c.point, cnt.as_dict()

    # ---------------------------------------------------------------- dense voxel map
    def dense_configure(self, enable: bool = True, voxel_width: float = 0.2, max_voxels: int = 1 << 22,
                        min_norm_squared: float = 0.0, max_norm_squared: float = 0.0, every: int = 1):
        """fmx_dense_configure (before the first registration or integration): a dense voxel
        map of the registered scans, `max_voxels` voxels of width `voxel_width` at the most.
        The gate defaults (both 0) to the extraction's range limits; `every`: the register
        path integrates scans 0, every, 2 every, ..."""
        p = _DenseParams()
        p.enable = int(bool(enable))
        p.voxel_width = float(voxel_width)
        p.max_voxels = int(max_voxels)
        p.min_norm_squared = float(min_norm_squared)
        p.max_norm_squared = float(max_norm_squared)
        p.every = int(every)
        self._chk(self._L.fmx_dense_configure(self.h, C.byref(p)))
        self._dense = True  # profile_read reports the "dense" id from here on

    def dense_integrate(self, points, pose34, scan_idx: int = 0) -> dict:
        """fmx_dense_integrate: (N, 4) float32 points (numpy, or a torch tensor on the host
        or the device) into the map at pose34 (3 x 4).  Returns the counts (added, merged,
        gated, out_of_range, invalid; they sum to N)."""
        on_dev, ptr, n, keep = _scan_ptr(points)
        pose = np.ascontiguousarray(pose34, np.float64).reshape(12)
        if on_dev:
            _ready(keep)
        cnt = _DenseCounts()
        self._chk(self._L.fmx_dense_integrate(self.h, ptr if n else None, C.c_size_t(n), C.c_int(on_dev), _p(pose),
                                              C.c_uint64(scan_idx), C.byref(cnt)))
        del keep
        return cnt.as_dict()

    def dense_last(self):
        """fmx_dense_last: (counts dict, integrated) of the last register_scan /
        register_cloud; integrated 1 done, 0 skipped by `every` (or the map is off), -1
        refused for capacity."""
        cnt = _DenseCounts()
        flag = C.c_int(0)
        self._chk(self._L.fmx_dense_last(self.h, C.byref(cnt), C.byref(flag)))
        return cnt.as_dict(), int(flag.value)

    def dense_stats(self) -> dict:
        s = np.zeros(4, np.uint64)
        self._chk(self._L.fmx_dense_stats(self.h, _p(s)))
        return dict(voxels=int(s[0]), max_voxels=int(s[1]), integrations=int(s[2]), slots=int(s[3]))

    def _voxel_arrays(self, m: int, misses: bool):
        """Arrays for m voxels, the fmx_voxel_arrays over them and the dict a caller gets."""
        out = dict(points=np.zeros((m, 3), np.float64), scan=np.zeros(m, np.uint64), index=np.zeros(m, np.uint32),
                   hits=np.zeros(m, np.uint32))
        if misses:
            out["misses"] = np.zeros(m, np.uint32)
        A = _VoxelArrays()
        A.xyz, A.scan, A.index, A.hits = (out[k].ctypes.data for k in ("points", "scan", "index", "hits"))
        A.misses = out["misses"].ctypes.data if misses else None
        return A, out

    def _with_misses(self, misses, filtered=False) -> bool:
        return bool(getattr(self, "_carve", False) or filtered) if misses is None else bool(misses)

    def dense_download(self, min_hits: int = 1, max_miss_ratio=None, misses=None) -> dict:
        """fmx_carve_download: the voxels with at least min_hits points, in no particular
        order: points (N, 3) float64 in the world, scan (N,) uint64 and index (N,) uint32 of
        each voxel's representative, hits (N,) uint32.  With max_miss_ratio only the voxels
        with misses <= max_miss_ratio * hits (the integer rule of miss_fraction).  misses (N,)
        uint32 is returned as well once carve_configure has been called on this context, with
        a max_miss_ratio, or with misses=True; a context that never carves reads as before."""
        num, den = miss_fraction(max_miss_ratio)
        args = (C.c_uint32(min_hits), C.c_uint32(num), C.c_uint32(den))
        n = C.c_uint32(0)
        self._chk(self._L.fmx_carve_download(self.h, *args, None, C.byref(n)))
        m = int(n.value)
        A, out = self._voxel_arrays(m, self._with_misses(misses, max_miss_ratio is not None))
        if m:
            self._chk(self._L.fmx_carve_download(self.h, *args, C.byref(A), C.byref(n)))
        return {k: v[:n.value] for k, v in out.items()}

    def dense_clear(self):
        self._chk(self._L.fmx_dense_clear(self.h))

    # ---------------------------------------------------------------- rolling the dense map
    @staticmethod
    def _roll_box(centre, half):
        return (np.ascontiguousarray(centre, np.float64).reshape(3),
                np.ascontiguousarray([int(h) for h in half], np.uint32).reshape(3))

    def roll_configure(self, enable: bool = True, half=(0, 0, 0), step: float = 0.0, spill: bool = True):
        """fmx_roll_configure: the register path rolls the dense map about the previous
        scan's pose once it has moved `step` metres on an axis (or when the next integration
        would not fit), keeping the voxels within `half` (three voxel counts) of it."""
        p = _RollParams()
        p.enable = int(bool(enable))
        for k in range(3):
            p.half[k] = int(half[k])
        p.step = float(step)
        p.spill = int(bool(spill))
        self._chk(self._L.fmx_roll_configure(self.h, C.byref(p)))

    def roll_count(self, centre, half):
        """fmx_roll_count: (inside, outside) of the box; changes nothing."""
        c, h = self._roll_box(centre, half)
        out = np.zeros(2, np.uint64)
        self._chk(self._L.fmx_roll_count(self.h, _p(c), _p(h), _p(out)))
        return int(out[0]), int(out[1])

    def roll_evict(self, centre, half, discard: bool = False, misses=None) -> dict:
        """fmx_carve_evict: the voxels outside the box leave the map and are returned like
        dense_download's (empty arrays with discard=True; misses as there)."""
        c, h = self._roll_box(centre, half)
        m = 0 if discard else self.roll_count(c, h)[1]
        A, out = self._voxel_arrays(m, self._with_misses(misses))
        n = C.c_uint32(m)
        if discard:
            self._chk(self._L.fmx_carve_evict(self.h, _p(c), _p(h), None, C.byref(n)))
        elif m:
            self._chk(self._L.fmx_carve_evict(self.h, _p(c), _p(h), C.byref(A), C.byref(n)))
        return {k: v[:m] for k, v in out.items()}

    def roll_drain(self, misses=None) -> dict:
        """fmx_carve_drain: the voxels the register path's rolls evicted since the last drain
        (misses as in dense_download)."""
        n = C.c_uint32(0)
        self._chk(self._L.fmx_carve_drain(self.h, None, C.byref(n)))
        m = int(n.value)
        A, out = self._voxel_arrays(m, self._with_misses(misses))
        if m:
            self._chk(self._L.fmx_carve_drain(self.h, C.byref(A), C.byref(n)))
        return {k: v[:n.value] for k, v in out.items()}

    # ---------------------------------------------------------------- carving the dense map
    def carve_configure(self, enable: bool = True, max_norm_squared: float = 0.0, margin: int = 1,
                        ray_stride: int = 1, every: int = 1):
        """fmx_carve_configure (any time once the dense map is on): integrations also cast a
        ray from the sensor to every point they took (within max_norm_squared, 0 = the dense
        gate's; every ray_stride-th input index; every `every`-th integration) and each stored
        voxel counts the rays that passed through it, except in the last `margin` voxels
        before the return."""
        p = _CarveParams()
        p.enable = int(bool(enable))
        p.max_norm_squared = float(max_norm_squared)
        p.margin = int(margin)
        p.ray_stride = int(ray_stride)
        p.every = int(every)
        self._chk(self._L.fmx_carve_configure(self.h, C.byref(p)))
        self._carve = True  # profile_read lists the "carve" id, the downloads carry misses, from here on

    def carve_rays(self, points, pose34) -> dict:
        """fmx_carve_rays: the rays of (N, 4) float32 points at pose34 against the map as it
        stands; integrates nothing, exempts nothing.  Returns rays, steps, misses, exempt."""
        on_dev, ptr, n, keep = _scan_ptr(points)
        pose = np.ascontiguousarray(pose34, np.float64).reshape(12)
        if on_dev:
            _ready(keep)
        cnt = _CarveCounts()
        self._chk(self._L.fmx_carve_rays(self.h, ptr if n else None, C.c_size_t(n), C.c_int(on_dev), _p(pose),
                                         C.byref(cnt)))
        del keep
        return cnt.as_dict()

    def carve_last(self):
        """fmx_carve_last: (counts dict, carved) of the last dense_integrate / register_scan /
        register_cloud."""
        cnt = _CarveCounts()
        flag = C.c_int(0)
        self._chk(self._L.fmx_carve_last(self.h, C.byref(cnt), C.byref(flag)))
        return cnt.as_dict(), int(flag.value)

    # ---------------------------------------------------------------- probing the dense map
    def probe_points(self, points, pose34, min_hits: int = 1, max_miss_ratio=None) -> dict:
        """fmx_probe_points: one lookup per (N, 4) float32 point (numpy, or a torch tensor on
        the host or the device) at pose34, on the device; changes nothing.  Returns state (N,)
        uint8 (PROBE_ABSENT, _FILTERED: present but not solid under min_hits and
        max_miss_ratio (miss_fraction's integer rule), _SOLID, _OUT_OF_RANGE, _INVALID), the
        voxel's points, scan, index, hits and misses where the state is FILTERED or SOLID
        (zeros elsewhere), and counts (absent, filtered, solid, out_of_range, invalid)."""
        num, den = miss_fraction(max_miss_ratio)
        on_dev, ptr, n, keep = _scan_ptr(points)
        pose = np.ascontiguousarray(pose34, np.float64).reshape(12)
        if on_dev:
            _ready(keep)
        A, out = self._voxel_arrays(n, True)
        state = np.zeros(n, np.uint8)
        cnt = _ProbePointCounts()
        self._chk(self._L.fmx_probe_points(self.h, ptr if n else None, C.c_size_t(n), C.c_int(on_dev), _p(pose),
                                           C.c_uint32(min_hits), C.c_uint32(num), C.c_uint32(den), _p(state),
                                           C.byref(A), C.byref(cnt)))
        del keep
        return dict(out, state=state, counts=cnt.as_dict())

    def probe_rays(self, points, pose34, min_hits: int = 1, max_miss_ratio=None, skip: int = 0) -> dict:
        """fmx_probe_rays: one segment cast per (N, 4) float32 point, from pose34's translation
        to the point's world point through the voxels of the map, the first `skip` voxels of
        the path left out and the end voxel included; changes nothing.  Returns state (N,)
        uint8 (PROBE_SOLID: the ray ended in a solid voxel; PROBE_ABSENT: clear;
        _OUT_OF_RANGE, _INVALID), step (N,) uint32 (the hit voxel's place on the path,
        PROBE_NO_STEP without a hit), t (N,) float64 (where the ray entered it as a fraction
        of the segment, +inf without a hit), the hit voxel's points, scan, index, hits and
        misses, and counts (hit, clear, out_of_range, invalid, steps: the voxels examined)."""
        num, den = miss_fraction(max_miss_ratio)
        on_dev, ptr, n, keep = _scan_ptr(points)
        pose = np.ascontiguousarray(pose34, np.float64).reshape(12)
        if on_dev:
            _ready(keep)
        A, out = self._voxel_arrays(n, True)
        state, step, t = np.zeros(n, np.uint8), np.zeros(n, np.uint32), np.zeros(n, np.float64)
        cnt = _ProbeRayCounts()
        self._chk(self._L.fmx_probe_rays(self.h, ptr if n else None, C.c_size_t(n), C.c_int(on_dev), _p(pose),
                                         C.c_uint32(min_hits), C.c_uint32(num), C.c_uint32(den), C.c_uint32(skip),
                                         _p(state), _p(step), _p(t), C.byref(A), C.byref(cnt)))
        del keep
        return dict(out, state=state, step=step, t=t, counts=cnt.as_dict())

    # ---------------------------------------------------------------- the nearest solid voxel
    def nearest_voxels(self, points, pose34, reach: int = 1, max_dist=None, min_hits: int = 1,
                       max_miss_ratio=None) -> dict:
        """fmx_nearest_voxels: per (N, 4) float32 point (numpy, or a torch tensor on the host or
        the device) at pose34 the nearest solid representative among the cells within `reach`
        (at most NEAREST_MAX_REACH) of its own voxel, no farther than max_dist (None: no
        limit; max_dist2 = max_dist * max_dist); changes nothing.  Returns state (N,) uint8
        (PROBE_SOLID: found; PROBE_ABSENT: none; _OUT_OF_RANGE, _INVALID), dist2 (N,) float64
        (the squared distance, +inf unless found), the winner's points, scan, index, hits and
        misses (zeros unless found) and counts (found, none, out_of_range, invalid, lookups:
        the cells the kernel looked up).  With reach = floor(max_dist / voxel_width) + 1 it is
        an exact radius search."""
        num, den = miss_fraction(max_miss_ratio)
        md = math.inf if max_dist is None else float(max_dist)
        on_dev, ptr, n, keep = _scan_ptr(points)
        pose = np.ascontiguousarray(pose34, np.float64).reshape(12)
        if on_dev:
            _ready(keep)
        A, out = self._voxel_arrays(n, True)
        state, dist2 = np.zeros(n, np.uint8), np.zeros(n, np.float64)
        cnt = _NearestCounts()
        self._chk(self._L.fmx_nearest_voxels(self.h, ptr if n else None, C.c_size_t(n), C.c_int(on_dev), _p(pose),
                                             C.c_uint32(min_hits), C.c_uint32(num), C.c_uint32(den), C.c_uint32(reach),
                                             C.c_double(md * md), _p(state), _p(dist2), C.byref(A), C.byref(cnt)))
        del keep
        return dict(out, state=state, dist2=dist2, counts=cnt.as_dict())

    # ---------------------------------------------------------------- aligning a scan to the map
    @staticmethod
    def _align_params(reach, max_dist, sigma, min_hits, max_miss_ratio, stride) -> "_AlignParams":
        num, den = miss_fraction(max_miss_ratio)
        md = math.inf if max_dist is None else float(max_dist)
        return _AlignParams(min_hits, num, den, reach, md * md, float(sigma), stride)

    def align_system(self, points, pose34, reach: int = 1, max_dist=None, sigma: float = 1.0, min_hits: int = 1,
                     max_miss_ratio=None, stride: int = 1):
        """fmx_align_system: the point-to-point Gauss-Newton system of the (N, 4) float32 points
        (numpy, or a torch tensor on the host or the device) at pose34 against their nearest
        solid representatives (the search of nearest_voxels: reach, max_dist, min_hits,
        max_miss_ratio), over the points i % stride == 0, whitened by sigma; changes nothing.
        Returns (system, counts): the packed upper 7 x 7 [H g]^T [H g] and the error, (29,)
        float64, and the counts found, none, out_of_range, invalid, skipped, lookups."""
        prm = self._align_params(reach, max_dist, sigma, min_hits, max_miss_ratio, stride)
        on_dev, ptr, n, keep = _scan_ptr(points)
        pose = np.ascontiguousarray(pose34, np.float64).reshape(12)
        if on_dev:
            _ready(keep)
        out = np.zeros(29, np.float64)
        cnt = _AlignCounts()
        self._chk(self._L.fmx_align_system(self.h, ptr if n else None, C.c_size_t(n), C.c_int(on_dev), _p(pose),
                                           C.byref(prm), _p(out), C.byref(cnt)))
        del keep
        return out, cnt.as_dict()

    def plane_system(self, points, pose34, reach: int = 1, max_dist=None, sigma: float = 1.0, min_hits: int = 1,
                     max_miss_ratio=None, stride: int = 1):
        """fmx_plane_system: align_system with the point-to-plane row against the winner's
        normal of the current snapshot (normals_build); a winner without a normal makes the
        point unoriented and adds nothing.  Returns (system, counts) as align_system, the
        counts with unoriented."""
        prm = self._align_params(reach, max_dist, sigma, min_hits, max_miss_ratio, stride)
        on_dev, ptr, n, keep = _scan_ptr(points)
        pose = np.ascontiguousarray(pose34, np.float64).reshape(12)
        if on_dev:
            _ready(keep)
        out = np.zeros(29, np.float64)
        cnt = _PlaneCounts()
        self._chk(self._L.fmx_plane_system(self.h, ptr if n else None, C.c_size_t(n), C.c_int(on_dev), _p(pose),
                                           C.byref(prm), _p(out), C.byref(cnt)))
        del keep
        return out, cnt.as_dict()

    def dense_align(self, points, pose_init34, reach: int = 1, max_dist=None, sigma: float = 1.0, min_hits: int = 1,
                    max_miss_ratio=None, stride: int = 1, max_iters: int = 30, threshold: float = 1e-6,
                    plane: bool = False) -> dict:
        """fmx_align_dense: Gauss-Newton on align_system's system from pose_init34 (arguments as
        align_system), at most max_iters systems, until a step's norm is below threshold;
        changes nothing.  Returns pose (3, 4), iters, converged, last_step, error and counts
        (the last system's).  plane=True: fmx_plane_align, the same loop on plane_system's
        system (needs a current normals_build)."""
        prm = self._align_params(reach, max_dist, sigma, min_hits, max_miss_ratio, stride)
        on_dev, ptr, n, keep = _scan_ptr(points)
        pose = np.ascontiguousarray(pose_init34, np.float64).reshape(12)
        if on_dev:
            _ready(keep)
        out = np.zeros(12, np.float64)
        res = _PlaneResult() if plane else _AlignResult()
        call = self._L.fmx_plane_align if plane else self._L.fmx_align_dense
        self._chk(call(self.h, ptr if n else None, C.c_size_t(n), C.c_int(on_dev), _p(pose), C.byref(prm),
                       C.c_uint32(max_iters), C.c_double(threshold), _p(out), C.byref(res)))
        del keep
        return dict(pose=out.reshape(3, 4), iters=int(res.iters), converged=bool(res.converged),
                    last_step=float(res.last_step), error=float(res.error), counts=res.counts.as_dict())

    # ---------------------------------------------------------------- scoring candidate poses
    def score_poses(self, points, poses, reach: int = 1, max_dist=None, min_hits: int = 1, max_miss_ratio=None,
                    stride: int = 1) -> dict:
        """fmx_score_poses: the (N, 4) float32 points (numpy, or a torch tensor on the host or
        the device) judged at each of the K poses (K x 3 x 4, or K x 12) in one call: per pose
        the class counts of nearest_voxels over the points i % stride == 0 (reach, max_dist,
        min_hits, max_miss_ratio as there) and the sum of the found points' squared distances;
        changes nothing.  Returns a dict of (K,) arrays: found, none, out_of_range, invalid
        (uint32), sum_d2 (float64), lookups (uint64).  At most SCORE_MAX_POSES poses."""
        prm = self._align_params(reach, max_dist, 1.0, min_hits, max_miss_ratio, stride)
        on_dev, ptr, n, keep = _scan_ptr(points)
        P = np.ascontiguousarray(poses, np.float64).reshape(-1, 12)
        if on_dev:
            _ready(keep)
        rec = np.zeros(len(P), SCORE_DTYPE)
        self._chk(self._L.fmx_score_poses(self.h, ptr if n else None, C.c_size_t(n), C.c_int(on_dev),
                                          _p(P) if len(P) else None, C.c_uint32(len(P)), C.byref(prm),
                                          _p(rec) if len(P) else None))
        del keep
        return {k: np.ascontiguousarray(rec[k]) for k in SCORE_FIELDS}

    # ---------------------------------------------------------------- refining candidate poses
    def refine_systems(self, points, poses, reach: int = 1, max_dist=None, sigma: float = 1.0, min_hits: int = 1,
                       max_miss_ratio=None, stride: int = 1, plane: bool = False) -> dict:
        """fmx_refine_systems: align_system's (plane=True: plane_system's) system of the (N, 4)
        float32 points at each of the K poses (K x 3 x 4, or K x 12) in one call; arguments as
        align_system; changes nothing.  Returns a dict of arrays: system (K, 29) float64, found,
        none, out_of_range, invalid, unoriented (uint32, unoriented 0 unless plane), lookups
        (uint64).  At most REFINE_MAX_POSES poses."""
        prm = self._align_params(reach, max_dist, sigma, min_hits, max_miss_ratio, stride)
        on_dev, ptr, n, keep = _scan_ptr(points)
        P = np.ascontiguousarray(poses, np.float64).reshape(-1, 12)
        if on_dev:
            _ready(keep)
        rec = np.zeros(len(P), REFINE_SYSTEM_DTYPE)
        self._chk(self._L.fmx_refine_systems(self.h, ptr if n else None, C.c_size_t(n), C.c_int(on_dev),
                                             _p(P) if len(P) else None, C.c_uint32(len(P)), C.byref(prm),
                                             C.c_int(int(bool(plane))), _p(rec) if len(P) else None))
        del keep
        return {k: np.ascontiguousarray(rec[k]) for k in REFINE_SYSTEM_FIELDS}

    def refine_poses(self, points, poses_init, reach: int = 1, max_dist=None, sigma: float = 1.0, min_hits: int = 1,
                     max_miss_ratio=None, stride: int = 1, max_iters: int = 30, threshold: float = 1e-6,
                     plane: bool = False) -> dict:
        """fmx_refine_poses: dense_align's loop from each of the K poses_init at once, all poses
        that are still running evaluated together per iteration (arguments as dense_align);
        changes nothing.  Returns a dict of arrays: pose (K, 3, 4), iters, converged, singular
        (bool; such a pose is returned as it came), last_step, error and the last system's
        found, none, out_of_range, invalid, unoriented and lookups."""
        prm = self._align_params(reach, max_dist, sigma, min_hits, max_miss_ratio, stride)
        on_dev, ptr, n, keep = _scan_ptr(points)
        P = np.ascontiguousarray(poses_init, np.float64).reshape(-1, 12)
        if on_dev:
            _ready(keep)
        out = np.zeros((len(P), 12), np.float64)
        res = np.zeros(len(P), REFINE_RESULT_DTYPE)
        self._chk(self._L.fmx_refine_poses(self.h, ptr if n else None, C.c_size_t(n), C.c_int(on_dev),
                                           _p(P) if len(P) else None, C.c_uint32(len(P)), C.byref(prm),
                                           C.c_int(int(bool(plane))), C.c_uint32(max_iters), C.c_double(threshold),
                                           _p(out) if len(P) else None, _p(res) if len(P) else None))
        del keep
        got = {k: np.ascontiguousarray(res[k]) for k in REFINE_RESULT_FIELDS}
        got["converged"], got["singular"] = got["converged"] != 0, got["singular"] != 0
        return dict(got, pose=out.reshape(-1, 3, 4))

    # ---------------------------------------------------------------- surface normals of the map
    def normals_build(self, reach: int = 1, max_dist=None, min_support: int = 5, max_flatness: float = 0.1,
                      min_hits: int = 1, max_miss_ratio=None) -> dict:
        """fmx_normals_build: one normal record per voxel of the map as it stands, from the
        solid representatives (min_hits, max_miss_ratio) of the cells within `reach` of the
        voxel's own, no farther than max_dist (None: the whole cube): the covariance's smallest
        eigenvector where at least min_support were admitted and l0 <= max_flatness * l1.  The
        snapshot is current until the table changes.  Returns the counts oriented,
        flat_rejected, sparse, filtered (they sum to the voxels) and lookups."""
        num, den = miss_fraction(max_miss_ratio)
        md = math.inf if max_dist is None else float(max_dist)
        prm = _NormalsParams(min_hits, num, den, reach, md * md, min_support, float(max_flatness))
        cnt = _NormalsCounts()
        self._chk(self._L.fmx_normals_build(self.h, C.byref(prm), C.byref(cnt)))
        return cnt.as_dict()

    def normals_stats(self) -> dict:
        """fmx_normals_stats: built, current, and the voxels and the oriented ones at the build."""
        s = np.zeros(4, np.uint64)
        self._chk(self._L.fmx_normals_stats(self.h, _p(s)))
        return dict(built=bool(s[0]), current=bool(s[1]), voxels=int(s[2]), oriented=int(s[3]))

    def normals_download(self, oriented_only: bool = True, misses=None) -> dict:
        """fmx_normals_download: dense_download's arrays for the voxels that were solid under
        the build's filter (oriented_only: those with a normal), in no particular order, with
        normals (N, 3) float32 (zeros unless oriented), flatness (N,) float32 and support (N,)
        uint32.  The snapshot must be current."""
        flag = C.c_int(int(bool(oriented_only)))
        n = C.c_uint32(0)
        self._chk(self._L.fmx_normals_download(self.h, flag, None, None, None, None, C.byref(n)))
        m = int(n.value)
        A, out = self._voxel_arrays(m, self._with_misses(misses))
        out.update(normals=np.zeros((m, 3), np.float32), flatness=np.zeros(m, np.float32), support=np.zeros(m, np.uint32))
        if m:
            self._chk(self._L.fmx_normals_download(self.h, flag, C.byref(A), _p(out["normals"]), _p(out["flatness"]),
                                                   _p(out["support"]), C.byref(n)))
        return {k: v[:n.value] for k, v in out.items()}

    # ---------------------------------------------------------------- loading voxels back
    def dense_upload(self, points, scan=None, index=None, hits=None, misses=None) -> dict:
        """fmx_upload_voxels: voxel records back into the map, under the keys dense_download,
        roll_evict and roll_drain return them with (ctx.dense_upload(**ctx.roll_drain())):
        points (N, 3) float64 in the world, scan (N,) uint64, index, hits and misses (N,)
        uint32; None: 0, 0, 1 and 0 for every entry.  A resident voxel keeps its
        representative and adds the hits and misses; an absent one is opened with the first
        entry that names it.  misses needs carve_configure to have been called on this map.
        Returns the counts (added, merged, out_of_range, invalid; they sum to N)."""
        pts = np.ascontiguousarray(_host(points), np.float64)
        if pts.size % 3 or (pts.ndim == 2 and pts.shape[1] != 3):
            raise ValueError("points must be (N, 3)")
        pts = pts.reshape(-1, 3)
        n = len(pts)
        keep = [pts]
        A = _VoxelInput()
        A.xyz = pts.ctypes.data if n else None
        for name, a, dt in (("scan", scan, np.uint64), ("index", index, np.uint32), ("hits", hits, np.uint32),
                            ("misses", misses, np.uint32)):
            if a is None:
                continue
            a = np.ascontiguousarray(_host(a), dt).reshape(-1)
            if len(a) != n:
                raise ValueError(f"{name} must hold one value per point ({len(a)} != {n})")
            keep.append(a)
            # (an empty array still says that the field is given: misses on a map without carving is refused)
            setattr(A, name, a.ctypes.data if n else _NO_ENTRIES.ctypes.data)
        cnt = _UploadCounts()
        self._chk(self._L.fmx_upload_voxels(self.h, C.byref(A), C.c_uint32(n), C.byref(cnt)))
        del keep
        return cnt.as_dict()

    def roll_stats(self) -> dict:
        s = np.zeros(6, np.uint64)
        self._chk(self._L.fmx_roll_stats(self.h, _p(s)))
        return dict(rolls=int(s[0]), evicted=int(s[1]), spilled=int(s[2]), last_kept=int(s[3]), last_evicted=int(s[4]),
                    last_scan=int(s[5]))

    def current_pose(self) -> np.ndarray:
        T = np.zeros(12)
        self._chk(self._L.fmx_current_pose(self.h, _p(T)))
        return T.reshape(3, 4)

    def map_download(self, voxel_width: float):
        """fmx_map_download: FORM::map()'s to_voxel_map of both feature types at the
        current estimates (bindings.cpp:96-119), voxel by voxel.  Returns {"planar":
        (xyz (M,3), normals (M,3), scans (M,)), "point": (xyz, None, scans)}."""
        npl, npt = C.c_uint32(0), C.c_uint32(0)
        self._chk(self._L.fmx_map_download(self.h, C.c_double(voxel_width), None, None, C.byref(npl), None, None,
                                           C.byref(npt)))
        pl = np.zeros((npl.value, 6))
        spl = np.zeros(npl.value, np.uint64)
        pt = np.zeros((npt.value, 3))
        spt = np.zeros(npt.value, np.uint64)
        self._chk(self._L.fmx_map_download(self.h, C.c_double(voxel_width), _p(pl), _p(spl), C.byref(npl), _p(pt),
                                           _p(spt), C.byref(npt)))
        return {"planar": (pl[:npl.value, :3].copy(), pl[:npl.value, 3:].copy(), spl[:npl.value]),
                "point": (pt[:npt.value], None, spt[:npt.value])}

    def last_stats(self) -> dict:
        keys = ["icp_iters", "lm_iters", "matched_planar", "matched_point", "map_planar", "map_point",
                "linearizations", "map_scans", "host_waits", "spec_matches", "spec_hits", "spec_map",
                "pipelined", "window_poses",
                # cumulative since the context was created (every entry point counts)
                "pool_compactions_planar", "pool_compactions_point", "win_compactions", "win_growths_plane",
                "win_growths_point"]
        s = np.zeros(len(keys), np.uint64)
        self._chk(self._L.fmx_last_stats(self.h, _p(s), C.c_int(len(keys))))
        return {k: int(v) for k, v in zip(keys, s)}

    def match_work(self) -> dict:
        w = np.zeros(3)
        self._chk(self._L.fmx_match_work(self.h, _p(w)))
        return dict(queries=float(w[0]), probes=float(w[1]), candidates=float(w[2]))

    # ---------------------------------------------------------------- profiling
    def moments(self, ref_i, ref_j) -> np.ndarray:
        """fmx_moments: the (K, 272) pair moments of the context's correspondences at
        reference poses ref_i[k], ref_j[k] (K x 3 x 4); evaluate them at any poses with
        moments_contract (no device round trip)."""
        ri = np.ascontiguousarray(ref_i, np.float64).reshape(-1, 12)
        rj = np.ascontiguousarray(ref_j, np.float64).reshape(-1, 12)
        out = np.zeros((max(self.K, 1), 272))
        self._chk(self._L.fmx_moments(self.h, _p(ri), _p(rj), _p(out)))
        return out[:self.K]

    def match_cert(self, per_query: bool = False):
        """fmx_match_cert: the warm certificate of the last match — (certified, warm)
        query counts, and with per_query a uint8 array (planar then point queries, 1 =
        settled by the certificate without a search)."""
        cnt = np.zeros(2, np.uint64)
        flags = np.zeros(self.n_planar + self.n_point if per_query else 0, np.uint8)
        self._chk(self._L.fmx_match_cert(self.h, _p(cnt), _p(flags) if per_query else None))
        out = dict(certified=int(cnt[0]), warm=int(cnt[1]))
        if per_query:
            out["flags"] = flags
        return out

    def profile_match_work(self) -> dict:
        """fmx_profile_match_work: the profiled match launches' work since the last
        reset, split into cold (first match on a map / query set) and warm launches."""
        w = np.zeros(12)
        self._chk(self._L.fmx_profile_match_work(self.h, _p(w)))
        return {k: dict(launches=w[6 * i], queries=w[6 * i + 1], probes=w[6 * i + 2], candidates=w[6 * i + 3],
                        certified=w[6 * i + 4], warm=w[6 * i + 5])
                for i, k in enumerate(("cold", "warm"))}

    def corr_generation(self) -> int:
        g = C.c_uint64()
        self._chk(self._L.fmx_corr_generation(self.h, C.byref(g)))
        return int(g.value)

    def profile(self, on: bool = True):
        self._chk(self._L.fmx_profile_enable(self.h, C.c_int(int(on))))

    def profile_reset(self):
        self._chk(self._L.fmx_profile_reset(self.h))

    def profile_read(self) -> dict:
        """Per kernel id: ms, launches, bytes since the last reset.  The "dense" id is
        listed once dense_configure has been called, the "carve" id once carve_configure has:
        a context that never configures them reads exactly as before."""
        n = self._L.fmx_profile_count()
        for name, flag in ((b"carve", "_carve"), (b"dense", "_dense")):  # the last ids, in this order
            if not getattr(self, flag, False) and self._L.fmx_profile_name(n - 1) == name:
                n -= 1
        ms = np.zeros(n)
        la = np.zeros(n, np.uint64)
        by = np.zeros(n)
        self._chk(self._L.fmx_profile_read(self.h, _p(ms), _p(la), _p(by), C.c_int(n)))
        return {self._L.fmx_profile_name(k).decode(): dict(ms=float(ms[k]), launches=int(la[k]), bytes=float(by[k]))
                for k in range(n)}

    def sync(self):
        self._chk(self._L.fmx_sync(self.h))


class _CtxBuffer:
    """Buffer protocol over a context-owned pinned array that also holds the context."""

    def __init__(self, arr, ctx):
        self._arr = arr
        self._ctx = ctx
        self.__array_interface__ = arr.__array_interface__


def _scan_ptr(scan):
    """(on_device, pointer, n_points, keepalive) for a numpy array or torch tensor."""
    try:
        import torch
        if isinstance(scan, torch.Tensor):
            if scan.dtype != torch.float32 or scan.dim() != 2 or scan.shape[1] != 4:
                raise ValueError("scan tensor must be (N, 4) float32")
            t = scan.contiguous()
            return (1 if t.is_cuda else 0), C.c_void_p(t.data_ptr()), t.shape[0], t
    except ImportError:
        pass
    a = np.ascontiguousarray(scan, np.float32)
    if a.ndim != 2 or a.shape[1] != 4:
        raise ValueError("scan must be (N, 4) float32 (PointXYZf layout)")
    return 0, _p(a), a.shape[0], a


def moments_contract(mom, ref_i, ref_j, poses_i, poses_j, sigma: float):
    """fmx_moments_contract (host only): packed 13 x 13 G (K, 91) and errors (K,) of K
    pairs at poses (poses_i[k], poses_j[k]) from their moments taken at (ref_i, ref_j)."""
    m = np.ascontiguousarray(mom, np.float64).reshape(-1, 272)
    K = m.shape[0]
    a = [np.ascontiguousarray(x, np.float64).reshape(K, 12) for x in (ref_i, ref_j, poses_i, poses_j)]
    G = np.zeros((max(K, 1), 91))
    err = np.zeros(max(K, 1))
    st = lib().fmx_moments_contract(C.c_uint32(K), _p(m), _p(a[0]), _p(a[1]), _p(a[2]), _p(a[3]),
                                    C.c_double(sigma), _p(G), _p(err))
    if st != FMX_OK:
        raise FmxError(st, "fmx_moments_contract failed")
    return G[:K], err[:K]


def comm_unique_id() -> bytes:
    """fmx_comm_unique_id: the 128-byte RCCL id one rank creates and shares."""
    buf = (C.c_uint8 * 128)()
    st = lib().fmx_comm_unique_id(buf)
    if st != FMX_OK:
        raise FmxError(st, "fmx_comm_unique_id failed (RCCL missing?)")
    return bytes(buf)


class Estimator:
    """form::Estimator (form/form.hpp:40-84) backed by the MI355X path."""

    def __init__(self, params: EstimatorParams | None = None, device: int = 0):
        self.ctx = Context(params, device)

    def register_scan(self, scan):
        """Returns (planar (F,6) xyz+normal, point (F,3)) like register_scan's tuple."""
        self.ctx.register_scan(scan)
        d = self.ctx.extract_download()
        return d["planar"], d["point"]

    def current_lidar_estimate(self) -> np.ndarray:
        return self.ctx.current_pose()


def extract_keypoints(points, params: KeypointExtractionParams, lidar_params=None):
    """form._core.extract_keypoints (bindings.cpp:214-240): (planar_points, normals,
    point_points).  lidar_params is accepted and ignored, as in the reference."""
    pts = np.asarray(points, np.float64).reshape(-1, 3)
    scan = np.zeros((len(pts), 4), np.float32)
    scan[:, :3] = pts.astype(np.float32)
    ctx = Context(EstimatorParams(extraction=params))
    try:
        ctx.extract(scan, 0)
        d = ctx.extract_download()
    finally:
        ctx.close()
    planar = d["planar"].astype(np.float64)
    return planar[:, :3].copy(), planar[:, 3:].copy(), d["point"].astype(np.float64)


# ---------------------------------------------------------------------------- evalio
# The evalio pipeline surface of form._core.FORM (python/bindings.cpp:48-180), backed by
# fmx.  evalio itself is not needed: lidar parameters, measurements and poses are
# duck-typed (attributes / numpy arrays), and results are numpy arrays.

# EVALIO_SETUP_PARAMS (bindings.cpp:66-88): YAML key -> (type, default, where it lands).
# Note the reference's key `max_dist_map` sets KeypointMapParams::min_dist_map (:85),
# and `num_threads` sizes the reference's TBB pool (no role on the GPU path).
PIPELINE_PARAMS = {
    "neighbor_points": (int, 5, "extraction.neighbor_points"),
    "num_sectors": (int, 6, "extraction.num_sectors"),
    "planar_threshold": (float, 1.0, "extraction.planar_threshold"),
    "planar_feats_per_sector": (int, 50, "extraction.planar_feats_per_sector"),
    "point_feats_per_sector": (int, 3, "extraction.point_feats_per_sector"),
    "radius": (float, 1.0, "extraction.radius"),
    "min_points": (int, 5, "extraction.min_points"),
    "max_dist_matching": (float, 0.8, "max_dist_matching"),
    "new_pose_threshold": (float, 1e-4, "new_pose_threshold"),
    "max_num_rematches": (int, 30, "max_num_rematches"),
    "disable_smoothing": (bool, False, "disable_smoothing"),
    "max_num_keyscans": (int, 50, "max_num_keyscans"),
    "max_num_recent_scans": (int, 10, "max_num_recent_scans"),
    "max_steps_unused_keyscan": (int, 10, "max_steps_unused_keyscan"),
    "keyscan_match_ratio": (float, 0.1, "keyscan_match_ratio"),
    "max_dist_map": (float, 0.1, "min_dist_map"),
    "num_threads": (int, 0, None),
}
# keys of an evalio config's pipeline entry that are not pipeline parameters
CONFIG_KEYS = ("pipeline", "name")


def _pose44(T) -> np.ndarray:
    T = np.asarray(T, np.float64)
    if T.shape == (4, 4):
        return T.copy()
    out = np.eye(4)
    out[:3, :] = T.reshape(3, 4)
    return out


def _points_xyz(mm) -> np.ndarray:
    """A LidarMeasurement's points as (N, 3): an (N, >=3) array, a measurement with a
    `points` attribute, or a sequence of objects with x, y, z (evalio.Point)."""
    pts = getattr(mm, "points", mm)
    try:
        a = np.asarray(pts, np.float64)
        if a.ndim == 2 and a.shape[1] >= 3:
            return a[:, :3]
    except (TypeError, ValueError):
        pass
    return np.array([[p.x, p.y, p.z] for p in pts], np.float64).reshape(-1, 3)


def _seconds(t) -> float:
    """A time as float seconds: a number or an evalio Duration (to_sec)."""
    return float(t.to_sec()) if hasattr(t, "to_sec") else float(t)


def _cloud_fields(mm):
    """A LidarMeasurement's points as an unordered cloud: ((N, 3) xyz, (N,) ring or None,
    (N,) time in seconds or None) from an (N, >= 5) array (columns 3 and 4: ring, time),
    an (N, 3..4) array (no ring, no time), or evalio-style points (x, y, z, row, t)."""
    pts = getattr(mm, "points", mm)
    try:
        a = np.asarray(pts, np.float64)
        if a.ndim == 2 and a.shape[1] >= 3:
            if a.shape[1] >= 5:
                return a[:, :3], a[:, 3].astype(np.uint16), a[:, 4]
            return a[:, :3], None, None
    except (TypeError, ValueError):
        pass
    pts = list(pts)
    xyz = np.array([[p.x, p.y, p.z] for p in pts], np.float64).reshape(-1, 3)
    ring = np.array([p.row for p in pts], np.uint16) if pts and hasattr(pts[0], "row") else None
    t = np.array([_seconds(p.t) for p in pts], np.float64) if pts and hasattr(pts[0], "t") else None
    return xyz, ring, t


class FORM:
    """form._core.FORM (bindings.cpp:48-180) on the MI355X path.

    Same call sequence as evalio drives the reference: ``set_params`` (YAML keys),
    ``set_lidar_params``, ``set_imu_T_lidar``, ``initialize``, then ``add_lidar`` per
    scan, ``pose()`` and ``map()``.  ``add_lidar`` returns {"planar", "point"} as
    (F, 4) arrays of (x, y, z, scan) in the scan's frame — the reference's evalio
    Points carry the scan index in `col` as a uint16 (bindings.cpp:31-41, so it wraps
    modulo 65536); ``map()`` the same in the
    world frame, voxel by voxel (bindings.cpp:96-119)."""

    def __init__(self, device: int = 0):
        self.params = EstimatorParams()
        self.num_threads = 0
        self.device = device
        self.lidar_T_imu = np.eye(4)
        self._est = None
        self._scan = -1
        self._pose = np.eye(4)
        self._deskew = None  # set_deskew's arguments, applied by initialize()
        self._organize = None  # set_organize's arguments, applied by initialize()
        self._dense = None  # set_dense_map's arguments, applied by initialize()
        self._roll = None  # set_dense_roll's arguments, applied by initialize() after the dense map
        self._carve = None  # set_dense_carve's arguments, applied by initialize() after the dense map
        self._scan_period = None  # seconds, from set_lidar_params when the parameters carry one

    @staticmethod
    def name() -> str:
        return "form"

    @staticmethod
    def url() -> str:
        return "https://github.com/rpl-cmu/form"

    @staticmethod
    def default_params() -> dict:
        return {k: d for k, (_, d, _) in PIPELINE_PARAMS.items()}

    def set_params(self, params: dict) -> dict:
        """Apply YAML parameter overrides (EVALIO_SETUP_PARAMS keys, bindings.cpp:66-88);
        an evalio config entry's own keys (pipeline, name) are skipped.  Unknown keys
        raise KeyError.  Returns the full parameter dict now in effect."""
        for k, v in params.items():
            if k in CONFIG_KEYS:
                continue
            if k not in PIPELINE_PARAMS:
                raise KeyError(f"unknown FORM parameter {k!r}")
            typ, _, dest = PIPELINE_PARAMS[k]
            v = typ(v)
            if dest is None:
                self.num_threads = v
            elif dest.startswith("extraction."):
                setattr(self.params.extraction, dest.split(".", 1)[1], v)
            else:
                setattr(self.params, dest, v)
        return self.get_params()

    def get_params(self) -> dict:
        out = {}
        for k, (_, _, dest) in PIPELINE_PARAMS.items():
            if dest is None:
                out[k] = self.num_threads
            elif dest.startswith("extraction."):
                out[k] = getattr(self.params.extraction, dest.split(".", 1)[1])
            else:
                out[k] = getattr(self.params, dest)
        return out

    def set_imu_params(self, params) -> None:  # bindings.cpp:123 (unused)
        pass

    def set_lidar_params(self, params) -> None:
        """bindings.cpp:126-132: range limits (squared) and the organized geometry."""
        e = self.params.extraction
        e.min_norm_squared = float(params.min_range) * float(params.min_range)
        e.max_norm_squared = float(params.max_range) * float(params.max_range)
        e.num_columns = int(params.num_columns)
        e.num_rows = int(params.num_rows)
        # bindings.cpp:131: delta_time_ = params.delta_time() (evalio: 1 / rate)
        if hasattr(params, "delta_time"):
            dt = params.delta_time
            self._scan_period = _seconds(dt() if callable(dt) else dt)
        elif getattr(params, "rate", None):
            self._scan_period = 1.0 / float(params.rate)

    def set_imu_T_lidar(self, T) -> None:
        """bindings.cpp:135-137: lidar_T_imu = (imu_T_lidar)^-1."""
        self.lidar_T_imu = np.linalg.inv(_pose44(T))

    def initialize(self) -> None:
        """bindings.cpp:141: a fresh estimator with the current parameters."""
        if self._est is not None:
            self._est.close()
        self._est = Context(self.params, self.device)
        if self._deskew is not None:
            self._est.deskew_configure(*self._deskew)
        if self._organize is not None:
            self._est.organize_configure(**self._organize)
        if self._dense is not None:
            self._est.dense_configure(**self._dense)
        if self._roll is not None:
            if self._dense is None:
                raise ValueError("set_dense_roll needs set_dense_map")
            w = self._dense["voxel_width"]
            half = [int(math.ceil(h / w)) for h in self._roll["half_extent_m"]]
            self._est.roll_configure(self._roll["enable"], half, self._roll["step_m"], self._roll["spill"])
        if self._carve is not None:
            if self._dense is None:
                raise ValueError("set_dense_carve needs set_dense_map")
            c = self._carve
            self._est.carve_configure(c["enable"], c["max_range_m"] ** 2, c["margin"], c["ray_stride"], c["every"])
        self._scan = -1
        self._pose = np.eye(4)

    def set_deskew(self, enable: bool = True, initial_twist=None, column_fraction=None) -> None:
        """Constant-velocity deskewing of every scan to mid-sweep (fmx_deskew_configure;
        no reference counterpart, so not a pipeline YAML key).  Applied by initialize().
        initial_twist: [w; v] per scan period for the first two scans (default: at rest);
        column_fraction: per-column sweep fractions in [0, 1] (default c / cols)."""
        self._deskew = (bool(enable),
                        None if initial_twist is None else np.array(initial_twist, np.float64).reshape(6),
                        None if column_fraction is None else np.array(column_fraction, np.float32).reshape(-1))

    def set_organize(self, enable: bool = True, elevation=None, ring_to_row=None, azimuth_offset: float = 0.0,
                     clockwise: bool = False) -> None:
        """Accept unordered clouds of any length in add_lidar (fmx_organize_configure; no
        reference counterpart, so not a pipeline YAML key).  Applied by initialize().
        elevation: rows angles in radians (elevation mode); else the points' ring picks the
        row, through ring_to_row if given."""
        self._organize = dict(enable=bool(enable),
                              elevation=None if elevation is None else np.array(elevation, np.float64).reshape(-1),
                              ring_to_row=None if ring_to_row is None else np.array(ring_to_row, np.int32).reshape(-1),
                              azimuth_offset=float(azimuth_offset), clockwise=bool(clockwise))

    def set_dense_map(self, enable: bool = True, voxel_width: float = 0.2, max_voxels: int = 1 << 22, every: int = 1,
                      min_norm_squared: float = 0.0, max_norm_squared: float = 0.0) -> None:
        """A dense voxel map of the registered scans, kept on the device (fmx_dense_configure;
        the reference's users build one on the host with scripts/rerun_map.py, so not a
        pipeline YAML key).  Applied by initialize().  Every `every`-th scan is integrated at
        its pose as add_lidar leaves it; the gate defaults to set_lidar_params' range limits."""
        self._dense = dict(enable=bool(enable), voxel_width=float(voxel_width), max_voxels=int(max_voxels),
                           every=int(every), min_norm_squared=float(min_norm_squared),
                           max_norm_squared=float(max_norm_squared))

    def set_dense_roll(self, enable: bool = True, half_extent_m=50.0, step_m: float = 2.0, spill: bool = True) -> None:
        """Roll the dense map with the sensor (fmx_roll_configure): once the pose has moved
        step_m on an axis, the voxels farther than half_extent_m (one number, or one per axis;
        ceil(half_extent_m / voxel_width) voxels) from it leave the device.  With spill they
        wait for dense_evicted(), else they are dropped.  Applied by initialize()."""
        h = np.broadcast_to(np.asarray(half_extent_m, np.float64), (3,))
        self._roll = dict(enable=bool(enable), half_extent_m=[float(v) for v in h], step_m=float(step_m),
                          spill=bool(spill))

    def set_dense_carve(self, enable: bool = True, max_range_m: float = 0.0, margin: int = 1, ray_stride: int = 1,
                        every: int = 1) -> None:
        """Count, per voxel of the dense map, the rays of later scans that passed through it
        (fmx_carve_configure), so that dense_map(max_miss_ratio=...) can leave out what moved
        while the map was built.  max_range_m: only returns nearer than this cast a ray (0: the
        dense gate's); margin: voxels in front of a return that are left alone; ray_stride,
        every: cast every n-th point's ray, carve every n-th integration.  Applied by
        initialize()."""
        self._carve = dict(enable=bool(enable), max_range_m=float(max_range_m), margin=int(margin),
                           ray_stride=int(ray_stride), every=int(every))

    def add_imu(self, mm) -> None:  # bindings.cpp:144 (unused)
        pass

    def add_lidar(self, mm) -> dict:
        """bindings.cpp:147-179: register the scan, update the pose
        (current_lidar_estimate * lidar_T_imu) and return its features."""
        if self._est is None:
            raise RuntimeError("FORM.add_lidar before initialize()")
        if self._organize is not None and self._organize["enable"]:
            return self._add_cloud(mm)
        xyz = _points_xyz(mm)
        # point_to_form: PointXYZf(x, y, z) (bindings.cpp:43-45), assembled straight into
        # a pinned fmx_scan_buffer: the registration then DMAs it with no staging copy
        scan = self._est.scan_buffer(len(xyz))
        scan[:, :3] = xyz
        scan[:, 3] = 0.0
        self._est.register_scan(scan)
        return self._scan_done()

    def _add_cloud(self, mm) -> dict:
        """add_lidar with set_organize: a measurement of any length, organized on the
        device.  Ring and time come from an (N, >= 5) array (columns 3 and 4) or from
        evalio-style points (row, t); times become sweep fractions with the scan period of
        set_lidar_params (without one they are taken as fractions already)."""
        xyz, ring, t = _cloud_fields(mm)
        cloud = np.zeros((len(xyz), 4), np.float32)
        cloud[:, :3] = xyz
        frac = None
        if t is not None:
            frac = (t / self._scan_period if self._scan_period else t).astype(np.float32)
        self._est.register_cloud(cloud, ring, frac)
        return self._scan_done()

    def _scan_done(self) -> dict:
        self._scan += 1
        self._pose = _pose44(self._est.current_pose()) @ self.lidar_T_imu
        d = self._est.extract_download()
        # point_to_evalio stores the scan id as static_cast<uint16_t>(scan) in the
        # point's col (bindings.cpp:31-41): it wraps past 65535 scans
        sid = self._scan % 65536
        planar = np.zeros((len(d["planar"]), 4))
        planar[:, :3] = d["planar"][:, :3]
        planar[:, 3] = sid
        point = np.zeros((len(d["point"]), 4))
        point[:, :3] = d["point"]
        point[:, 3] = sid
        return {"planar": planar, "point": point}

    def pose(self) -> np.ndarray:
        """bindings.cpp:93: the latest pose (4 x 4).  With deskewing on (set_deskew) it is
        the pose at the middle of the last sweep, and add_lidar's features are in that
        frame."""
        return self._pose.copy()

    def map(self) -> dict:
        """bindings.cpp:96-119: the window's keypoints in the world frame, to_voxel_map
        at voxel width min_dist_map, as (M, 4) arrays of (x, y, z, scan)."""
        if self._est is None or self._scan < 0:
            return {"planar": np.zeros((0, 4)), "point": np.zeros((0, 4))}
        m = self._est.map_download(self.params.min_dist_map)
        out = {}
        for name, (xyz, _, sc) in m.items():
            a = np.zeros((len(xyz), 4))
            a[:, :3] = xyz
            a[:, 3] = sc % 65536  # uint16 col, as add_lidar (map_download keeps the raw id)
            out[name] = a
        return out

    def dense_map(self, min_hits: int = 1, max_miss_ratio=None) -> dict:
        """The dense voxel map (set_dense_map): one point per voxel with at least min_hits
        points, as dense_download gives it: points (N, 3) in the world (lidar poses, as
        map()), scan, index and hits; empty before initialize() or with the map off.  With
        set_dense_carve also misses, and max_miss_ratio leaves out the voxels that more than
        that fraction of their hits' worth of rays passed through."""
        if self._est is None or self._dense is None or not self._dense["enable"]:
            out = dict(points=np.zeros((0, 3)), scan=np.zeros(0, np.uint64), index=np.zeros(0, np.uint32),
                       hits=np.zeros(0, np.uint32))
            if self._carve is not None or max_miss_ratio is not None:
                out["misses"] = np.zeros(0, np.uint32)
            return out
        return self._est.dense_download(min_hits, max_miss_ratio)

    def dense_normals(self, min_hits: int = 1, max_miss_ratio=None, reach_m=None, viewpoint=None) -> dict:
        """The dense map's oriented voxels with their surface normals (Context.normals_build,
        then normals_download): dense_map's arrays plus normals (N, 3) float32, flatness and
        support.  The snapshot is rebuilt with this filter, NORMALS_DEFAULTS and reach =
        ceil(reach_m / voxel_width) (None: one cell; ValueError past NEAREST_MAX_REACH), which
        also bounds the neighbours' distance.  A normal's sign is the build's (its largest
        component positive) unless a viewpoint (3,) is given: each is then flipped, here on
        the host, to face it."""
        self._need_dense()
        kw = dict(NORMALS_DEFAULTS)
        if reach_m is not None:
            r = float(reach_m)
            if not (r > 0.0) or math.isinf(r):
                raise ValueError("reach_m must be a finite number > 0")
            kw["reach"] = max(1, math.ceil(r / float(self._dense["voxel_width"])))
            kw["max_dist"] = r
            if kw["reach"] > NEAREST_MAX_REACH:
                raise ValueError(f"reach_m spans more than {NEAREST_MAX_REACH} voxels: reach {kw['reach']}")
        self._est.normals_build(min_hits=min_hits, max_miss_ratio=max_miss_ratio, **kw)
        out = self._est.normals_download(True)
        if viewpoint is not None:
            to_eye = np.asarray(viewpoint, np.float64).reshape(1, 3) - out["points"]
            away = np.einsum("ij,ij->i", to_eye, out["normals"].astype(np.float64)) < 0.0
            out["normals"][away] *= -1.0
        return out

    def _probe_args(self, points, pose):
        if self._est is None or self._dense is None or not self._dense["enable"]:
            raise RuntimeError("the dense map is off (set_dense_map, then initialize())")
        if isinstance(points, np.ndarray) and points.ndim == 2 and points.shape[1] == 3:
            p4 = np.zeros((len(points), 4), np.float32)
            p4[:, :3] = points
            points = p4
        T = self._est.current_pose() if pose is None else np.asarray(pose, np.float64).reshape(-1, 4)[:3]
        return points, T

    def dense_lookup(self, points, pose=None, min_hits: int = 1, max_miss_ratio=None) -> dict:
        """Look points of the sensor frame up in the dense map (Context.probe_points): (N, 3)
        or (N, 4) float32 points at the lidar pose `pose` (3 x 4 or 4 x 4; None: the current
        one, where the last scan was integrated)."""
        points, T = self._probe_args(points, pose)
        return self._est.probe_points(points, T, min_hits, max_miss_ratio)

    def dense_cast(self, points, pose=None, min_hits: int = 1, max_miss_ratio=None, skip: int = 0) -> dict:
        """Cast the segments from the sensor at `pose` to the points through the dense map
        (Context.probe_rays; arguments as dense_lookup): the first solid voxel on each."""
        points, T = self._probe_args(points, pose)
        return self._est.probe_rays(points, T, min_hits, max_miss_ratio, skip)

    def dense_nearest(self, points, radius_m: float, pose=None, min_hits: int = 1, max_miss_ratio=None) -> dict:
        """The exact radius search of the dense map (Context.nearest_voxels; points and pose as
        dense_lookup): per point the nearest solid voxel no farther than radius_m, or none.
        reach = floor(radius_m / voxel_width) + 1; ValueError when that passes
        NEAREST_MAX_REACH."""
        points, T = self._probe_args(points, pose)
        r = float(radius_m)
        if not (r >= 0.0) or math.isinf(r):
            raise ValueError("radius_m must be a finite number >= 0")
        reach = math.floor(r / float(self._dense["voxel_width"])) + 1
        if reach > NEAREST_MAX_REACH:
            raise ValueError(f"radius_m spans more than {NEAREST_MAX_REACH} voxels: reach {reach}")
        return self._est.nearest_voxels(points, T, reach, r, min_hits, max_miss_ratio)

    def dense_fitness(self, points, radius_m: float, pose=None, min_hits: int = 1, max_miss_ratio=None) -> dict:
        """A scan judged against the dense map, from dense_nearest on the host: n_valid (points
        neither invalid nor out of range), n_found (those with a solid voxel within radius_m),
        fitness = n_found / n_valid (0.0 when there are none) and rmse = sqrt(sum(dist2 of the
        found) / n_found) (0.0 when there are none), summed in index order with math.fsum."""
        got = self.dense_nearest(points, radius_m, pose, min_hits, max_miss_ratio)
        return fitness_of(got["state"], got["dist2"])

    def dense_localize(self, points, radius_m: float, pose_guess=None, sigma: float = 0.1, max_iters: int = 30,
                       threshold: float = 1e-6, stride: int = 1, min_hits: int = 1, max_miss_ratio=None,
                       plane: bool = False) -> dict:
        """Register a scan against the dense map (Context.dense_align; points as dense_lookup,
        pose_guess None: the current pose): point-to-point Gauss-Newton on the nearest solid
        voxels within radius_m (reach as dense_nearest, ValueError past NEAREST_MAX_REACH).
        Nothing is changed, the estimator included.  Returns pose (3, 4), iters, converged
        and, from one more system at that pose, n_valid, n_found, fitness = n_found / n_valid
        and rmse = sqrt(2 error sigma^2 / n_found) (0.0 where the divisor is 0): dense_fitness's
        figures over the points i % stride == 0, without a per-point download.
        plane=True: point-to-plane against the map's normals (Context.plane_system); the
        snapshot is built first with NORMALS_DEFAULTS and this call's filter when
        normals_stats() says it is not current.  n_found then counts the points with an
        oriented winner, n_valid those and the unoriented and the ones without a winner, rmse
        is the point-to-plane one, and n_unoriented is returned as well."""
        points, T = self._probe_args(points, pose_guess)
        r = float(radius_m)
        if not (r >= 0.0) or math.isinf(r):
            raise ValueError("radius_m must be a finite number >= 0")
        reach = math.floor(r / float(self._dense["voxel_width"])) + 1
        if reach > NEAREST_MAX_REACH:
            raise ValueError(f"radius_m spans more than {NEAREST_MAX_REACH} voxels: reach {reach}")
        if plane:
            if not self._est.normals_stats()["current"]:
                self._est.normals_build(min_hits=min_hits, max_miss_ratio=max_miss_ratio, **NORMALS_DEFAULTS)
            got = self._est.dense_align(points, T, reach, r, sigma, min_hits, max_miss_ratio, stride, max_iters, threshold,
                                        plane=True)
            S, cnt = self._est.plane_system(points, got["pose"], reach, r, sigma, min_hits, max_miss_ratio, stride)
            n_found, n_valid = cnt["found"], cnt["found"] + cnt["unoriented"] + cnt["none"]
            return dict(pose=got["pose"], iters=got["iters"], converged=got["converged"], n_valid=n_valid,
                        n_found=n_found, n_unoriented=cnt["unoriented"], fitness=n_found / n_valid if n_valid else 0.0,
                        rmse=math.sqrt(2.0 * float(S[28]) * float(sigma) * float(sigma) / n_found) if n_found else 0.0)
        got = self._est.dense_align(points, T, reach, r, sigma, min_hits, max_miss_ratio, stride, max_iters, threshold)
        S, cnt = self._est.align_system(points, got["pose"], reach, r, sigma, min_hits, max_miss_ratio, stride)
        n_found, n_valid = cnt["found"], cnt["found"] + cnt["none"]
        return dict(pose=got["pose"], iters=got["iters"], converged=got["converged"], n_valid=n_valid, n_found=n_found,
                    fitness=n_found / n_valid if n_valid else 0.0,
                    rmse=math.sqrt(2.0 * float(S[28]) * float(sigma) * float(sigma) / n_found) if n_found else 0.0)

    def dense_localize_many(self, points, radius_m: float, pose_guesses, sigma: float = 0.1, max_iters: int = 30,
                            threshold: float = 1e-6, stride: int = 1, min_hits: int = 1, max_miss_ratio=None,
                            plane: bool = False) -> dict:
        """dense_localize from K guesses at once (Context.refine_poses; pose_guesses K x 3 x 4,
        K x 4 x 4 or K x 12, the other arguments as dense_localize): the batched Gauss-Newton
        loop, then one more batched system evaluation at the final poses.  Returns a dict of
        (K, ...) arrays: pose, iters, converged, singular (such a guess is reported, not
        raised, and its pose is the guess) and, by dense_localize's formulas from that
        evaluation, n_valid, n_found, fitness, rmse (and n_unoriented with plane=True).  Nothing
        is changed, the estimator included."""
        P = np.asarray(pose_guesses, np.float64)
        P = P.reshape(-1, 12) if P.ndim == 2 and P.shape[1] == 12 else P.reshape(-1, P.shape[-2], 4)[:, :3]
        P = np.ascontiguousarray(P).reshape(-1, 12)
        points, _ = self._probe_args(points, P[0].reshape(3, 4) if len(P) else np.eye(3, 4))
        r = float(radius_m)
        if not (r >= 0.0) or math.isinf(r):
            raise ValueError("radius_m must be a finite number >= 0")
        reach = math.floor(r / float(self._dense["voxel_width"])) + 1
        if reach > NEAREST_MAX_REACH:
            raise ValueError(f"radius_m spans more than {NEAREST_MAX_REACH} voxels: reach {reach}")
        if plane and not self._est.normals_stats()["current"]:
            self._est.normals_build(min_hits=min_hits, max_miss_ratio=max_miss_ratio, **NORMALS_DEFAULTS)
        got = self._est.refine_poses(points, P, reach, r, sigma, min_hits, max_miss_ratio, stride, max_iters, threshold, plane)
        last = self._est.refine_systems(points, got["pose"], reach, r, sigma, min_hits, max_miss_ratio, stride, plane)
        n_found = last["found"].astype(np.int64)
        n_valid = n_found + last["none"].astype(np.int64) + last["unoriented"].astype(np.int64)
        s2 = float(sigma) * float(sigma)
        fitness = np.array([int(f) / int(v) if v else 0.0 for f, v in zip(n_found, n_valid)], np.float64)
        rmse = np.array([math.sqrt(2.0 * float(e) * s2 / int(f)) if f else 0.0 for e, f in zip(last["system"][:, 28], n_found)],
                        np.float64)
        out = dict(pose=got["pose"], iters=got["iters"], converged=got["converged"], singular=got["singular"],
                   n_valid=n_valid, n_found=n_found, fitness=fitness, rmse=rmse)
        if plane:
            out["n_unoriented"] = last["unoriented"].astype(np.int64)
        return out

    def dense_score(self, points, poses, radius_m: float, stride: int = 1, min_hits: int = 1,
                    max_miss_ratio=None) -> dict:
        """Judge a scan at many candidate poses in one call (Context.score_poses; points as
        dense_lookup, poses K x 3 x 4 or K x 4 x 4): per pose the counts of the radius search of
        dense_nearest (reach from radius_m as there) over the points i % stride == 0, sum_d2,
        and dense_fitness's figures from them: n_valid = found + none, fitness = found /
        n_valid and rmse = sqrt(sum_d2 / found) (0.0 where the divisor is 0).  Nothing is
        changed."""
        P = np.asarray(poses, np.float64)
        P = P.reshape(-1, 12) if P.ndim == 2 and P.shape[1] == 12 else P.reshape(-1, P.shape[-2], 4)[:, :3]
        points, _ = self._probe_args(points, P[0] if len(P) else np.eye(3, 4))
        r = float(radius_m)
        if not (r >= 0.0) or math.isinf(r):
            raise ValueError("radius_m must be a finite number >= 0")
        reach = math.floor(r / float(self._dense["voxel_width"])) + 1
        if reach > NEAREST_MAX_REACH:
            raise ValueError(f"radius_m spans more than {NEAREST_MAX_REACH} voxels: reach {reach}")
        got = self._est.score_poses(points, P, reach, r, min_hits, max_miss_ratio, stride)
        found = got["found"].astype(np.float64)
        n_valid = got["found"].astype(np.int64) + got["none"].astype(np.int64)
        with np.errstate(divide="ignore", invalid="ignore"):
            got["n_valid"] = n_valid
            got["fitness"] = np.where(n_valid > 0, found / np.maximum(n_valid, 1), 0.0)
            got["rmse"] = np.where(found > 0, np.sqrt(got["sum_d2"] / np.maximum(found, 1.0)), 0.0)
        return got

    def dense_relocalize(self, points, radius_m: float, candidates, top: int = 3, score_stride=None,
                         plane: bool = False, batched: bool = False, **localize_kw) -> dict:
        """Find the sensor in the dense map without a guess inside the search radius: score
        every candidate pose (dense_score at score_stride; None: max(1, N // 4096)), rank them
        (rank_scores), run dense_localize (radius_m, plane and localize_kw: sigma, max_iters,
        threshold, stride, min_hits, max_miss_ratio) from each of the first `top`, and return
        the result with the largest n_found, then the smallest rmse, then the earliest rank,
        with candidate (its index), ranking (all indices by rank) and scores (dense_score's).
        A candidate whose system is singular (too few found points) drops out; FmxError when
        all of them do.  Nothing is changed, the estimator included.
        batched=True refines the first `top` in one dense_localize_many call instead (one pair
        of launches per iteration however many are still running) and picks by the same rule;
        the result's entries are those of dense_localize, from that call."""
        P = np.asarray(candidates, np.float64)
        P = P.reshape(-1, 12) if P.ndim == 2 and P.shape[1] == 12 else P.reshape(-1, P.shape[-2], 4)[:, :3]
        P = np.ascontiguousarray(P).reshape(-1, 3, 4)
        if not len(P):
            raise ValueError("no candidates")
        n = len(points)
        stride = max(1, n // 4096) if score_stride is None else int(score_stride)
        scores = self.dense_score(points, P, radius_m, stride, localize_kw.get("min_hits", 1),
                                  localize_kw.get("max_miss_ratio"))
        ranking = rank_scores(scores)
        if batched:
            first = ranking[:max(int(top), 1)]
            many = self.dense_localize_many(points, radius_m, P[first], plane=plane, **localize_kw)
            best = None
            for rank, k in enumerate(first):
                if many["singular"][rank]:
                    continue
                key = (-int(many["n_found"][rank]), float(many["rmse"][rank]), rank)
                if best is None or key < best[0]:
                    best = (key, rank, int(k))
            if best is None:
                raise FmxError(5, "dense_relocalize: every candidate's system is singular (too few found points)")
            j = best[1]
            got = dict(pose=many["pose"][j].copy(), iters=int(many["iters"][j]), converged=bool(many["converged"][j]),
                       n_valid=int(many["n_valid"][j]), n_found=int(many["n_found"][j]))
            if plane:
                got["n_unoriented"] = int(many["n_unoriented"][j])
            got.update(fitness=float(many["fitness"][j]), rmse=float(many["rmse"][j]))
            return dict(got, candidate=best[2], ranking=ranking, scores=scores)
        best, last = None, None
        for rank, k in enumerate(ranking[:max(int(top), 1)]):
            try:
                got = self.dense_localize(points, radius_m, P[k], plane=plane, **localize_kw)
            except FmxError as e:
                if e.status != 5:  # FMX_E_STATE: a singular system
                    raise
                last = e
                continue
            key = (-got["n_found"], got["rmse"], rank)
            if best is None or key < best[0]:
                best = (key, got, int(k))
        if best is None:
            raise last
        return dict(best[1], candidate=best[2], ranking=ranking, scores=scores)

    def _need_dense(self):
        if self._est is None or self._dense is None or not self._dense["enable"]:
            raise RuntimeError("the dense map is off (set_dense_map, then initialize())")

    def dense_restore(self, voxels: dict) -> dict:
        """Put voxels back into the dense map (Context.dense_upload): what dense_map() and
        dense_evicted() return, e.g. the evicted voxels of a place the sensor comes back to.
        Returns the counts (added, merged, out_of_range, invalid)."""
        self._need_dense()
        v = dict(voxels)
        return self._est.dense_upload(v["points"], v.get("scan"), v.get("index"), v.get("hits"), v.get("misses"))

    def dense_save(self, path, min_hits: int = 1) -> None:
        """Write the dense map to a numpy .npz: dense_map(min_hits)'s arrays (misses all 0
        without set_dense_carve) and voxel_width."""
        self._need_dense()
        d = self.dense_map(min_hits)
        misses = d["misses"] if "misses" in d else np.zeros(len(d["hits"]), np.uint32)
        with open(path, "wb") as f:  # (np.savez would append .npz to a bare name)
            np.savez(f, points=d["points"], scan=d["scan"], index=d["index"], hits=d["hits"], misses=misses,
                     voxel_width=np.float64(self._dense["voxel_width"]))

    def dense_load(self, path, drop_misses: bool = False) -> dict:
        """Read a dense_save file into the map (dense_restore).  ValueError when the file's
        voxel width is not, bit for bit, the configured one (the round trip promises
        exactness), or when it holds non-zero misses and set_dense_carve is not on, unless
        drop_misses.  Returns dense_restore's counts."""
        self._need_dense()
        with np.load(path) as z:
            d = {k: z[k] for k in ("points", "scan", "index", "hits", "misses", "voxel_width")}
        w = np.float64(d.pop("voxel_width"))
        if w.tobytes() != np.float64(self._dense["voxel_width"]).tobytes():
            raise ValueError(f"dense_load: the file's voxel width {float(w)!r} is not the configured "
                             f"{self._dense['voxel_width']!r}")
        carving = self._carve is not None and self._carve["enable"]
        if not carving:
            if d["misses"].any() and not drop_misses:
                raise ValueError("dense_load: the file holds misses and carving is off (set_dense_carve, or drop_misses=True)")
            del d["misses"]
        elif drop_misses:
            del d["misses"]
        return self.dense_restore(d)

    def dense_evicted(self) -> dict:
        """The voxels the rolling map (set_dense_roll) has evicted since the last call, as
        dense_map gives them; empty before initialize() or with rolling off."""
        if self._est is None or self._dense is None or not self._dense["enable"] or self._roll is None:
            return dict(points=np.zeros((0, 3)), scan=np.zeros(0, np.uint64), index=np.zeros(0, np.uint32),
                        hits=np.zeros(0, np.uint32))
        return self._est.roll_drain()
