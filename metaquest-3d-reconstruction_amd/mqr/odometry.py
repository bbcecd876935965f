"""Odometry information matrices on the GPU, mirroring the Open3D call of the reference
(scripts/processing/reconstruction/depth_optimization/make_fragments.py:142-150, 229-233):

    o3d.t.pipelines.odometry.compute_odometry_information_matrix(source_depth, target_depth, intrinsic,
                                                                 source_to_target, dist_threshold,
                                                                 depth_scale, depth_max)

``odometry_information_pairs`` runs every image pair of one stack of depth frames in one launch
(csrc/odometry.hip); the single-pair form stacks its two images and takes the batched call's entry.
The rules are written out in DESIGN "odometry information rules": they restate Open3D's kernel from
memory and are not pinned against it.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from .geometry import DeviceArray, Image, Tensor, device_ptr
from .ingest import ctypes_ptr


def _frames(depths, device):
    """(pointer argument, loc, N, H, W, keep-alive) of a frame stack: a (N, H, W) host array, a
    device-backed Tensor / DeviceArray of that shape, or (device buffer or pointer, N, H, W)."""
    if isinstance(depths, tuple):
        buf, N, H, W = depths
        return ctypes_ptr(buf), _lib.MQR_DEVICE, int(N), int(H), int(W), buf
    if isinstance(depths, (Tensor, DeviceArray)):
        d = device_ptr(depths, device)
        if d is not None:
            if len(depths.shape) != 3 or np.dtype(depths.dtype) != np.float32:
                raise ValueError("device frames must be (N, H, W) float32")
            N, H, W = depths.shape
            return ctypes_ptr(d[0]), _lib.MQR_DEVICE, int(N), int(H), int(W), depths
        if device_ptr(depths) is not None:
            raise ValueError(f"the frames live on another device than {device}")
        depths = depths.numpy()
    a = np.ascontiguousarray(depths, dtype=np.float32)
    if a.ndim != 3:
        raise ValueError(f"depths must be (N, H, W), got {a.shape}")
    return _lib.ptr(a), _lib.MQR_HOST, a.shape[0], a.shape[1], a.shape[2], a


def odometry_information_pairs(depths, K, src, tgt, T, dist_threshold, depth_scale=1.0, depth_max=3.0, device=0):
    """Information matrices of the pairs (src[p], tgt[p]) of a stack of depth frames.

    depths: (N, H, W) float32 frames -- a host array, a device-backed Tensor / DeviceArray, or
    (DeviceBuffer, N, H, W); K: the (3, 3) intrinsic matrix of all frames; T: (P, 4, 4) or (4, 4)
    source camera -> target camera.  Returns (info (P, 6, 6) float64 in the order rx, ry, rz, tx, ty,
    tz; counts (P,) int64, the accepted pixels of each pair)."""
    src = np.ascontiguousarray(src, np.int32).reshape(-1)
    tgt = np.ascontiguousarray(tgt, np.int32).reshape(-1)
    P = len(src)
    if len(tgt) != P:
        raise ValueError("src and tgt differ in length")
    info, counts = np.zeros((P, 6, 6)), np.zeros(P, np.int64)
    if P == 0:
        return info, counts
    K = np.ascontiguousarray(np.asarray(K.numpy() if hasattr(K, "numpy") else K, np.float64).reshape(3, 3))
    T = np.asarray(T.numpy() if hasattr(T, "numpy") else T, np.float64)
    if T.ndim == 2:
        T = np.broadcast_to(T, (P, 4, 4))
    if T.shape != (P, 4, 4):
        raise ValueError(f"T must be (4, 4) or ({P}, 4, 4), got {T.shape}")
    T = np.ascontiguousarray(T)
    dptr, loc, N, H, W, keep = _frames(depths, int(device))
    _lib.call("mqr_odometry_information_pairs", int(device), dptr, loc, N, H, W, _lib.ptr(K, _lib._f64p), P,
              _lib.ptr(src, _lib._i32p), _lib.ptr(tgt, _lib._i32p), _lib.ptr(T, _lib._f64p), float(dist_threshold),
              float(depth_scale), float(depth_max), _lib.ptr(info, _lib._f64p), _lib.ptr(counts, _lib._i64p))
    del keep
    return info, counts


def _image_array(img):
    if isinstance(img, Image):
        return img.numpy()
    a = np.asarray(img.numpy() if hasattr(img, "numpy") else img, np.float32)
    return a[:, :, 0] if a.ndim == 3 and a.shape[2] == 1 else a


def compute_odometry_information_matrix(source_depth, target_depth, intrinsic, source_to_target, dist_threshold=0.07,
                                        depth_scale=1.0, depth_max=3.0, device=0) -> np.ndarray:
    """o3d.t.pipelines.odometry.compute_odometry_information_matrix for one pair of depth images
    (``mqr.geometry.Image`` or (H, W) arrays): the 6x6 float64 matrix, bit for bit the batched call's."""
    s, t = _image_array(source_depth), _image_array(target_depth)
    if s.shape != t.shape or s.ndim != 2:
        raise ValueError(f"source and target depth must be (H, W) images of one size, got {s.shape} and {t.shape}")
    info, _ = odometry_information_pairs(np.stack([s, t]), intrinsic, [0], [1], source_to_target, dist_threshold,
                                         depth_scale, depth_max, device)
    return info[0]
