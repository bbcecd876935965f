"""Triangle-mesh ray casting on the GPU.

Stands in for ``o3d.t.geometry.RaycastingScene`` as the reference uses it for colour-aligned
depth (reconstruct_scene.py:197-201; o3d_utils.py:324-341; optimize_color_pose.py:24-47):

    scene = RaycastingScene(device=...)
    scene.add_triangles(mesh)                       # or (vertex_positions, triangle_indices)
    rays = RaycastingScene.create_rays_pinhole(K, T_wc, width_px, height_px)
    depth = scene.cast_rays(rays)['t_hit'].cpu().numpy()

``raycast_in_color_view`` also takes a ``VoxelBlockGrid`` (the volume marched directly, no mesh), and
``render_color_aligned_depth`` drives either over a capture (reconstruct_scene.py:181-225).

The BVH is built on the device (libmqr_hip.so, csrc/raycast.hip) at the first query after the
geometry changed.  ``cast_pinhole`` is the fused path (rays generated on the device, identical
to create_rays_pinhole + cast_rays).  t_hit is inf where a ray hits nothing; ids are
0xFFFFFFFF (``INVALID_ID``) there.  A mesh already in HBM (this package's extraction or mesh filter)
is added in place, and the cast results stay in HBM as Open3D's do on a CUDA device (copied to the
host on the first ``.numpy()``), so ``color_map`` can take them without a round trip.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from ._lib import MQR_HOST, call, ptr
from .geometry import DeviceArray, Tensor, device_mesh, host_rows, mesh_fields

INVALID_ID = 0xFFFFFFFF


def _pinhole_params(K, T):
    """float32(R^T K^-1) and float32(-R^T t), as Open3D's CreateRaysPinhole forms them."""
    K = np.asarray(K, np.float64).reshape(3, 3)
    T = np.asarray(T, np.float64).reshape(4, 4)
    if K[0, 1] == 0 and K[1, 0] == 0 and K[2, 0] == 0 and K[2, 1] == 0 and K[2, 2] == 1:
        inv = np.array([[1.0 / K[0, 0], 0.0, -K[0, 2] / K[0, 0]],
                        [0.0, 1.0 / K[1, 1], -K[1, 2] / K[1, 1]],
                        [0.0, 0.0, 1.0]])
    else:  # the adjugate over the determinant, operation by operation as csrc/raycast.hip's pinhole()
        a, b, c, d, e, f, g, h, i = (float(x) for x in K.reshape(9))
        A, B, C = e * i - f * h, -(d * i - f * g), d * h - e * g
        det = a * A + b * B + c * C
        inv = np.array([[A, -(b * i - c * h), b * f - c * e],
                        [B, a * i - c * g, -(a * f - c * d)],
                        [C, -(a * h - b * g), a * e - b * d]]) / det
    RT = T[:3, :3].T
    m = np.empty((3, 3))
    for r in range(3):
        for k in range(3):
            m[r, k] = (RT[r, 0] * inv[0, k] + RT[r, 1] * inv[1, k]) + RT[r, 2] * inv[2, k]
    c = -((RT[:, 0] * T[0, 3] + RT[:, 1] * T[1, 3]) + RT[:, 2] * T[2, 3])
    return m.astype(np.float32), c.astype(np.float32)


class RaycastingScene:
    def __init__(self, nthreads: int = 0, device=None):
        from .vbg import parse_device
        self.device_id = parse_device(device)
        h = ctypes.c_void_p()
        call("mqr_scene_create", self.device_id, ctypes.byref(h))
        self._h = h
        self._ngeom = 0

    def __del__(self):
        try:
            if getattr(self, "_h", None) is not None and self._h.value:
                call("mqr_scene_destroy", self._h)
                self._h = None
        except Exception:
            pass

    def add_triangles(self, vertex_positions, triangle_indices=None) -> int:
        gid = ctypes.c_uint32()
        f = mesh_fields(vertex_positions, triangle_indices)
        d = device_mesh(f, self.device_id)
        if d is not None:  # the mesh is in HBM on this scene's device: no host round trip
            call("mqr_scene_add_triangles", self._h, ctypes.c_void_p(d.positions), d.nv, ctypes.c_void_p(d.triangles),
                 d.nt, _lib.MQR_DEVICE, ctypes.byref(gid))
        else:
            v, t = host_rows(f.positions, np.float32), host_rows(f.triangles, np.int32)
            call("mqr_scene_add_triangles", self._h, ptr(v), v.shape[0], ptr(t), t.shape[0], MQR_HOST,
                 ctypes.byref(gid))
        self._ngeom += 1
        return int(gid.value)

    def triangle_count(self) -> int:
        n = ctypes.c_int64()
        call("mqr_scene_triangle_count", self._h, ctypes.byref(n))
        return int(n.value)

    @staticmethod
    def create_rays_pinhole(intrinsic_matrix, extrinsic_matrix, width_px: int, height_px: int) -> Tensor:
        """(H, W, 6) float32 rays: origin = camera centre, direction = R^T K^-1 (x+0.5, y+0.5, 1)."""
        K = intrinsic_matrix.numpy() if hasattr(intrinsic_matrix, "numpy") else intrinsic_matrix
        T = extrinsic_matrix.numpy() if hasattr(extrinsic_matrix, "numpy") else extrinsic_matrix
        m, c = _pinhole_params(K, T)
        px = np.arange(width_px, dtype=np.float32) + np.float32(0.5)
        py = np.arange(height_px, dtype=np.float32) + np.float32(0.5)
        px, py = np.meshgrid(px, py)
        rays = np.empty((height_px, width_px, 6), np.float32)
        rays[..., :3] = c
        for r in range(3):
            rays[..., 3 + r] = (m[r, 0] * px + m[r, 1] * py) + m[r, 2]
        return Tensor(rays)

    def _outputs(self, n, full):
        """Device buffers for the cast's results: (t_hit, geometry ids, primitive ids, uvs, normals)."""
        from ._lib import DeviceBuffer
        specs = [(np.float32, ())] + ([(np.uint32, ()), (np.uint32, ()), (np.float32, (2,)), (np.float32, (3,))]
                                      if full else [])
        out = [(DeviceBuffer(max(4, n * np.dtype(dt).itemsize * int(np.prod(k, dtype=np.int64))), self.device_id),
                dt, k) for dt, k in specs]
        return out + [None] * (5 - len(out))

    @staticmethod
    def _p(o):
        return None if o is None else o[0].ptr

    def _tensors(self, outs, shape, full):
        """The results as Tensors over their device buffers (host copies on first access)."""
        names = ["t_hit"] + (["geometry_ids", "primitive_ids", "primitive_uvs", "primitive_normals"] if full else [])
        return {nm: Tensor(DeviceArray(buf, buf.ptr.value, shape + k, dt, self.device_id))
                for nm, (buf, dt, k) in zip(names, outs)}

    def cast_rays(self, rays, nthreads: int = 0, full: bool = True) -> dict:
        r = rays.numpy() if hasattr(rays, "numpy") else np.asarray(rays)
        shape = r.shape[:-1]
        r = np.ascontiguousarray(r, dtype=np.float32).reshape(-1, 6)
        n = r.shape[0]
        outs = self._outputs(n, full)
        t, g, p, uv, nr = outs
        call("mqr_scene_cast_rays", self._h, ptr(r), n, MQR_HOST, self._p(t), self._p(g), self._p(p), self._p(uv),
             self._p(nr), _lib.MQR_DEVICE)
        return self._tensors([o for o in outs if o is not None], tuple(shape), full)

    def cast_pinhole(self, intrinsics, extrinsics, width_px: int, height_px: int, full: bool = False) -> dict:
        """Fused create_rays_pinhole + cast_rays for one camera (K (3,3), T_wc (4,4)) or a stack
        (n,3,3) / (n,4,4) of same-size cameras; outputs shaped (n, H, W[, k]) or (H, W[, k])."""
        K = np.ascontiguousarray(intrinsics, dtype=np.float64)
        T = np.ascontiguousarray(extrinsics, dtype=np.float64)
        single = K.ndim == 2
        K = K.reshape(-1, 3, 3)
        T = T.reshape(-1, 4, 4)
        nf = K.shape[0]
        n = nf * height_px * width_px
        outs = self._outputs(n, full)
        t, g, p, uv, nr = outs
        call("mqr_scene_cast_pinhole", self._h, ptr(K, _lib._f64p), ptr(T, _lib._f64p), nf, int(height_px),
             int(width_px), self._p(t), self._p(g), self._p(p), self._p(uv), self._p(nr), _lib.MQR_DEVICE)
        shape = (height_px, width_px) if single else (nf, height_px, width_px)
        return self._tensors([o for o in outs if o is not None], shape, full)


def raycast_in_color_view(scene, dataset, batch: int = 16, **cast_kw):
    """Generator of colour-aligned depth maps, one (H, W) float32 per dataset frame in order
    (reference o3d_utils.py:324-341); consecutive same-size frames are cast together.  `scene` is a
    RaycastingScene (the mesh cast) or a VoxelBlockGrid: the volume itself is then marched
    (``ray_cast_frames`` at the pixel centres, refined crossings, metric depth; `cast_kw` passes its
    thresholds through) and its misses (0) become inf, the mesh cast's t_hit convention."""
    from .o3d_utils import compute_o3d_intrinsic_matrices
    from .vbg import VoxelBlockGrid
    K = compute_o3d_intrinsic_matrices(dataset).astype(np.float32).astype(np.float64)
    T = dataset.transforms.extrinsics_wc.astype(np.float32).astype(np.float64)
    volume = isinstance(scene, VoxelBlockGrid)
    if cast_kw and not volume:
        raise TypeError(f"raycast_in_color_view: {sorted(cast_kw)} are the volume cast's arguments; a "
                        "RaycastingScene takes none")
    n = len(dataset)
    i = 0
    while i < n:
        w, h = int(dataset.widths[i]), int(dataset.heights[i])
        j = i + 1
        while j < n and j - i < batch and int(dataset.widths[j]) == w and int(dataset.heights[j]) == h:
            j += 1
        if volume:
            depth = scene.ray_cast_frames(K[i:j], T[i:j], w, h, **{**cast_kw, "render_attributes": ("depth",),
                                                                   "depth_scale": 1.0, "pixel_offset": 0.5,
                                                                   "refine": True})["depth"].numpy()
            depth[depth == 0] = np.inf
        else:
            depth = scene.cast_pinhole(K[i:j], T[i:j], w, h)["t_hit"].numpy()
        for k in range(j - i):
            yield depth[k]
        i = j


def render_color_aligned_depth(scene_or_vbg, data_io, optimized_color_dataset_map=None,
                               only_use_optimized_dataset: bool = False, sides=None, batch: int = 16, **cast_kw):
    """The reference's colour-aligned-depth stage (reconstruct_scene.py:200-225): per side, one depth map per
    colour frame through ``data_io.rgbd.save_color_aligned_depth`` -- the unoptimised frames whose timestamps
    are not in the optimised set, then the optimised ones; without an optimised map, every frame unless
    only_use_optimized_dataset.  The saves run on the I/O pool, so they overlap the next batch's cast.
    Returns the number of maps written."""
    from collections import deque
    from ._io import io_pool
    from .models import Side
    pending = deque()  # saves in flight, oldest first: at most two batches' worth, so a slow disk holds the
    written = 0        # casts back instead of letting the maps (4.9 MB each at 1280 x 960) pile up in memory

    def render(dataset, side):
        nonlocal written
        maps = raycast_in_color_view(scene_or_vbg, dataset, batch=batch, **cast_kw)
        for i in range(len(dataset)):
            while len(pending) >= 2 * batch:  # before the next batch's cast: the batch before last is on disk
                pending.popleft().result()
            timestamp = dataset.timestamps[i]
            depth_map = next(maps)
            pending.append(io_pool().submit(data_io.rgbd.save_color_aligned_depth, depth_map=depth_map, side=side,
                                            timestamp=timestamp))
            written += 1

    for side in (Side if sides is None else sides):
        color_dataset = data_io.color.load_color_dataset(side=side, use_cache=True)
        if optimized_color_dataset_map is not None:
            optimized = optimized_color_dataset_map[side]
            if not only_use_optimized_dataset:
                optimized_timestamps = set(optimized.timestamps)
                render(color_dataset[[i for i in range(len(color_dataset))
                                      if color_dataset.timestamps[i] not in optimized_timestamps]], side)
            render(optimized, side)
        elif not only_use_optimized_dataset:
            render(color_dataset, side)
    while pending:
        pending.popleft().result()
    return written
