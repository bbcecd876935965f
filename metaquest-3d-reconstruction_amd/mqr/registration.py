"""Fragment registration on the GPU, mirroring the Open3D calls of the reference
(scripts/processing/reconstruction/depth_optimization/refine_fragment_poses.py:122-193):

    o3d.t.pipelines.registration.evaluate_registration(source, target, max_correspondence_distance, transformation)
    o3d.t.pipelines.registration.multi_scale_icp(source, target, voxel_sizes, criteria_list,
                                                 max_correspondence_distances, init_source_to_target)
    o3d.t.pipelines.registration.get_information_matrix(source, target, max_correspondence_distance, transformation)

Point-to-point estimation only (what the reference passes).  The single-pair functions build a
two-cloud :class:`CloudSet`; the batched forms on a CloudSet register many pairs of N clouds per
launch, with every cloud down-sampled and indexed once (csrc/registration.hip).  Clouds that live in
HBM (an extraction's ``pcd.point.positions``) are taken in place.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import numpy as np

from . import _lib
from .geometry import DeviceArray, PointCloud, Tensor, device_ptr


@dataclass
class ICPConvergenceCriteria:
    """o3d.t.pipelines.registration.ICPConvergenceCriteria"""
    relative_fitness: float = 1e-6
    relative_rmse: float = 1e-6
    max_iteration: int = 30


@dataclass
class RegistrationResult:
    """o3d.t.pipelines.registration.RegistrationResult (plus the passes run per level)."""
    transformation: np.ndarray = field(default_factory=lambda: np.eye(4))
    fitness: float = 0.0
    inlier_rmse: float = 0.0
    num_iterations: List[int] = field(default_factory=list)
    correspondences: int = 0


def _positions(cloud):
    """The xyz Tensor / array behind a PointCloud, Tensor, DeviceArray or array-like."""
    if isinstance(cloud, PointCloud):
        return cloud.point.positions
    return cloud


def _i32(a):
    return np.ascontiguousarray(a, np.int32)


def _f64(a):
    return np.ascontiguousarray(a, np.float64)


def _transforms(T, n):
    T = np.eye(4) if T is None else np.asarray(T.numpy() if hasattr(T, "numpy") else T, np.float64)
    if T.ndim == 2:
        T = np.broadcast_to(T, (n, 4, 4))
    if T.shape != (n, 4, 4):
        raise ValueError(f"transformations must be (4, 4) or ({n}, 4, 4), got {T.shape}")
    return np.ascontiguousarray(T)


class CloudSet:
    """N point clouds resident in HBM with their cached down-sampled views and grid indices
    (mqr_cloudset).  ``clouds``: PointClouds, Tensors, DeviceArrays or (n, 3) arrays -- either all in
    HBM on ``device_id`` (used in place and kept alive by the set) or all on the host (copied once)."""

    def __init__(self, clouds: Sequence, device_id: int = 0):
        pos = [_positions(c) for c in clouds]
        if not pos:
            raise ValueError("a CloudSet needs at least one cloud")
        dev = [device_ptr(p, device_id) if isinstance(p, (Tensor, DeviceArray)) else None for p in pos]
        self.device_id = int(device_id)
        self._keep = []
        n = len(pos)
        ptrs = (ctypes.c_void_p * n)()
        counts = np.zeros(n, np.int64)
        if all(d is not None for d in dev):
            loc = _lib.MQR_DEVICE
            for i, (p, d) in enumerate(zip(pos, dev)):
                if len(p.shape) != 2 or p.shape[1] != 3 or np.dtype(p.dtype) != np.float32:
                    raise ValueError("device clouds must be (n, 3) float32")
                ptrs[i] = d[0] or None
                counts[i] = p.shape[0]
                self._keep.append(p)
        else:
            loc = _lib.MQR_HOST
            for i, p in enumerate(pos):
                a = np.ascontiguousarray(p.numpy() if hasattr(p, "numpy") else p, np.float32).reshape(-1, 3)
                self._keep.append(a)
                ptrs[i] = a.ctypes.data if len(a) else None
                counts[i] = len(a)
        self.counts = [int(c) for c in counts]
        h = ctypes.c_void_p()
        _lib.call("mqr_cloudset_create", self.device_id, n, ptrs, _lib.ptr(counts, _lib._i64p), loc, ctypes.byref(h))
        self._h = h
        if loc == _lib.MQR_HOST:
            self._keep = []  # copied

    def __len__(self):
        return len(self.counts)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value and _lib._lib is not None:
            _lib._lib.mqr_cloudset_destroy(self._h)
        self._h = None
        self._keep = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- views
    def voxel_down_sample(self, cloud: int, voxel_size: float) -> np.ndarray:
        """The voxel down-sampled view of one cloud as an (m, 3) float32 host array."""
        n = ctypes.c_int64()
        _lib.call("mqr_cloudset_voxel_down", self._h, int(cloud), float(voxel_size), ctypes.byref(n), None,
                  _lib.MQR_HOST)
        out = np.empty((n.value, 3), np.float32)
        _lib.call("mqr_cloudset_voxel_down", self._h, int(cloud), float(voxel_size), ctypes.byref(n), _lib.ptr(out),
                  _lib.MQR_HOST)
        return out

    # ---- batched pair operations
    def evaluate_pairs(self, src, tgt, max_correspondence_distance, transformations=None, every_k: int = 1):
        src, tgt = _i32(src), _i32(tgt)
        n = len(src)
        if n == 0:
            return []
        T = _transforms(transformations, n)
        fit, rmse, cnt = np.zeros(n), np.zeros(n), np.zeros(n, np.int64)
        _lib.call("mqr_evaluate_pairs", self._h, n, _lib.ptr(src, _lib._i32p), _lib.ptr(tgt, _lib._i32p), int(every_k),
                  float(max_correspondence_distance), _lib.ptr(T, _lib._f64p), _lib.ptr(fit, _lib._f64p),
                  _lib.ptr(rmse, _lib._f64p), _lib.ptr(cnt, _lib._i64p))
        return [RegistrationResult(T[i].copy(), float(fit[i]), float(rmse[i]), [1], int(cnt[i])) for i in range(n)]

    def icp_pairs(self, src, tgt, voxel_sizes, criteria_list, max_correspondence_distances, init_source_to_target=None):
        src, tgt = _i32(src), _i32(tgt)
        n = len(src)
        if n == 0:
            return []
        L = len(voxel_sizes)
        if not (len(criteria_list) == L == len(max_correspondence_distances)):
            raise ValueError("voxel_sizes, criteria_list and max_correspondence_distances differ in length")
        vs, md = _f64(list(voxel_sizes)), _f64(list(max_correspondence_distances))
        mi = _i32([c.max_iteration for c in criteria_list])
        rf, rr = _f64([c.relative_fitness for c in criteria_list]), _f64([c.relative_rmse for c in criteria_list])
        T0 = _transforms(init_source_to_target, n)
        T = np.zeros((n, 4, 4))
        fit, rmse, its = np.zeros(n), np.zeros(n), np.zeros((n, L), np.int32)
        _lib.call("mqr_icp_pairs", self._h, n, _lib.ptr(src, _lib._i32p), _lib.ptr(tgt, _lib._i32p), L,
                  _lib.ptr(vs, _lib._f64p), _lib.ptr(md, _lib._f64p), _lib.ptr(mi, _lib._i32p),
                  _lib.ptr(rf, _lib._f64p), _lib.ptr(rr, _lib._f64p), _lib.ptr(T0, _lib._f64p),
                  _lib.ptr(T, _lib._f64p), _lib.ptr(fit, _lib._f64p), _lib.ptr(rmse, _lib._f64p),
                  _lib.ptr(its, _lib._i32p))
        return [RegistrationResult(T[i].copy(), float(fit[i]), float(rmse[i]), [int(x) for x in its[i]])
                for i in range(n)]

    def information_pairs(self, src, tgt, max_correspondence_distance, transformations=None) -> np.ndarray:
        src, tgt = _i32(src), _i32(tgt)
        n = len(src)
        if n == 0:
            return np.zeros((0, 6, 6))
        T = _transforms(transformations, n)
        info = np.zeros((n, 6, 6))
        _lib.call("mqr_information_pairs", self._h, n, _lib.ptr(src, _lib._i32p), _lib.ptr(tgt, _lib._i32p),
                  float(max_correspondence_distance), _lib.ptr(T, _lib._f64p), _lib.ptr(info, _lib._f64p))
        return info


def _pair_set(source, target, device_id: Optional[int] = None):
    if device_id is None:
        d = device_ptr(_positions(source)) if isinstance(_positions(source), (Tensor, DeviceArray)) else None
        device_id = d[1] if d else 0
    return CloudSet([source, target], device_id)


def evaluate_registration(source, target, max_correspondence_distance, transformation=None) -> RegistrationResult:
    cs = _pair_set(source, target)
    try:
        return cs.evaluate_pairs([0], [1], max_correspondence_distance, transformation)[0]
    finally:
        cs.close()


def multi_scale_icp(source, target, voxel_sizes, criteria_list, max_correspondence_distances,
                    init_source_to_target=None, estimation_method=None) -> RegistrationResult:
    """Point-to-point multi-scale ICP (``estimation_method`` is accepted for call compatibility; the
    reference passes TransformationEstimationPointToPoint)."""
    cs = _pair_set(source, target)
    try:
        return cs.icp_pairs([0], [1], voxel_sizes, criteria_list, max_correspondence_distances,
                            init_source_to_target)[0]
    finally:
        cs.close()


def get_information_matrix(source, target, max_correspondence_distance, transformation=None) -> np.ndarray:
    cs = _pair_set(source, target)
    try:
        return cs.information_pairs([0], [1], max_correspondence_distance, transformation)[0]
    finally:
        cs.close()
