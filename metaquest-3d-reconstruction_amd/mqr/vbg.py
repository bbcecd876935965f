"""``VoxelBlockGrid`` -- HBM-resident voxel-block TSDF volume on one MI355X.

Drop-in for the ``o3d.t.geometry.VoxelBlockGrid`` surface the reference uses
(scripts/processing/reconstruction/utils/o3d_utils.py:170-229, reconstruct_scene.py:90-108,
refine_fragment_poses.py:39, reconstruction_data_io.py:42-55):

    VoxelBlockGrid(attr_names=('tsdf','weight'), attr_dtypes=(f32,f32), attr_channels=((1),(1)),
                   voxel_size, block_resolution, block_count, device)
    VoxelBlockGrid(attr_names=('tsdf','weight','color'), attr_dtypes=(f32,f32,f32), attr_channels=((1),(1),(3)), ...)
                                      the coloured volume: ``integrate`` takes Open3D's colour
                                      overload, ``integrate_frames`` takes ``colors=``, the extractions return
                                      coloured geometry and the ray cast renders "color"
    .compute_unique_block_coordinates(depth, intrinsic, extrinsic, depth_scale, depth_max,
                                      trunc_voxel_multiplier) -> (N,3) int32 block keys
    .integrate(block_coords, depth, intrinsic, extrinsic, depth_scale, depth_max, trunc_voxel_multiplier)
    .extract_point_cloud(weight_threshold=3.0, estimated_point_number=-1)
    .extract_triangle_mesh(weight_threshold=3.0, estimated_vertex_number=-1)
    .save(path) / VoxelBlockGrid.load(path)
    .ray_cast(block_coords, intrinsic, extrinsic, width, height, render_attributes, depth_scale, depth_min,
              depth_max, weight_threshold, trunc_voxel_multiplier, range_map_down_factor)
                                      -> {"depth" (H,W,1), "vertex" (H,W,3), "normal" (H,W,3)}  (Open3D's
                                      method, which the reference does not call; ``ray_cast_frames`` is its
                                      batched form)

plus ``integrate_frames`` (the batched whole-loop entry used by ``mqr.o3d_utils.integrate``).
Every call goes through libmqr_hip.so; there is no CPU path.
"""
from __future__ import annotations

import ctypes
import threading

import numpy as np

from . import _lib
from ._lib import MQR_DEVICE, MQR_DEVICE_RESIDENT, MQR_HOST, MqrStats, call, ptr
from .geometry import Image, PointCloud, Tensor, TriangleMesh

# Open3D defaults for the keyword arguments the reference relies on.
_O3D_DEPTH_SCALE = 1000.0
_O3D_DEPTH_MAX = 3.0
_O3D_TRUNC = 8.0


def parse_device(device) -> int:
    """'CUDA:0' / 'HIP:0' / 'cuda:1' / 0 / o3d.core.Device -> HIP device index.

    The reference's default is 'CPU:0' (config/pipeline_config.yml:14); this framework always
    runs the fusion path on the GPU, so 'CPU:n' maps to HIP device 0."""
    if device is None:
        return 0
    if isinstance(device, (int, np.integer)):
        return int(device)
    s = str(device).strip()
    if hasattr(device, "get_id") and hasattr(device, "get_type"):
        s = f"{device.get_type()}:{device.get_id()}"
    s = s.replace("Device(", "").replace(")", "")
    if ":" in s:
        kind, idx = s.rsplit(":", 1)
        if kind.strip().upper().endswith("CPU"):
            return 0
        try:
            return int(idx)
        except ValueError:
            return 0
    return 0


def _depth_array(depth) -> np.ndarray:
    if isinstance(depth, Image):
        return depth.numpy()
    if hasattr(depth, "as_tensor"):
        depth = depth.as_tensor()
    if hasattr(depth, "numpy"):
        depth = depth.numpy()
    a = np.ascontiguousarray(depth, dtype=np.float32)
    if a.ndim == 3 and a.shape[2] == 1:
        a = np.ascontiguousarray(a[:, :, 0])
    if a.ndim != 2:
        raise ValueError(f"depth must be H x W, got shape {a.shape}")
    return a


def _plain_array(x):
    """x as a numpy array or an object with ``shape`` / ``dtype``, nothing converted."""
    if hasattr(x, "as_tensor"):
        x = x.as_tensor()
    if hasattr(x, "numpy") and not getattr(x, "is_cuda", False):  # (a host tensor; one on the GPU stays as it is)
        x = x.numpy()
    return x if hasattr(x, "shape") and hasattr(x, "dtype") else np.asarray(x)


def _is_color_image(x) -> bool:
    """An H x W x 3 image (what tells Open3D's colour overload of ``integrate`` from the depth-only one)."""
    try:
        shape = tuple(_plain_array(x).shape)
    except Exception:  # noqa: BLE001
        return False
    return len(shape) == 3 and shape[2] == 3


def _color_array(color, ndim=3) -> np.ndarray:
    """A host colour image (H, W, 3) or stack (B, H, W, 3): uint8 only, anything else is a ValueError."""
    a = _plain_array(color)
    if getattr(a, "is_cuda", False):
        raise ValueError("a host colour image is expected here (device frames go through integrate_frames)")
    if np.dtype(a.dtype) != np.uint8:
        raise ValueError(f"colour images must be uint8, got {a.dtype}")
    a = np.ascontiguousarray(a)
    if a.ndim != ndim or a.shape[-1] != 3:
        raise ValueError(f"colour must be {'B x ' if ndim == 4 else ''}H x W x 3, got shape {a.shape}")
    return a


def _device_colors(colors):
    """(pointer, B, H, W, keep-alive) of a uint8 (B, H, W, 3) colour stack held in HBM -- a ``(buffer, B, H, W)``
    tuple (a DeviceBuffer, a DeviceArray or a raw pointer), a device-backed Tensor / DeviceArray, or a torch
    tensor on the GPU -- else None."""
    if isinstance(colors, tuple):
        buf, B, H, W = colors
        return getattr(buf, "ptr", buf), int(B), int(H), int(W), buf
    d = colors.device_array() if isinstance(colors, Tensor) else colors
    if hasattr(d, "device_id") and hasattr(d, "ptr") and hasattr(d, "shape"):
        shape, dtype, p = d.shape, d.dtype, d.ptr
    elif hasattr(colors, "data_ptr") and getattr(colors, "is_cuda", False):
        if not colors.is_contiguous():
            raise ValueError("device colour frames must be contiguous")
        shape, dtype, p = tuple(colors.shape), np.dtype(str(colors.dtype).replace("torch.", "")), colors.data_ptr()
    else:
        return None
    if np.dtype(dtype) != np.uint8:
        raise ValueError(f"colour images must be uint8, got {dtype}")
    if len(shape) != 4 or shape[3] != 3:
        raise ValueError(f"colour must be B x H x W x 3, got shape {tuple(shape)}")
    return p, int(shape[0]), int(shape[1]), int(shape[2]), colors


def _is_float32(d) -> bool:
    if d is None:
        return True
    try:
        return np.dtype(d) == np.float32
    except TypeError:
        return str(d).lower().replace("_", "").endswith("float32")


def _wants_color(names, dtypes, channels) -> bool:
    """True for the coloured layout ('tsdf','weight','color') with float32 attributes and channels ((1),(1),(3))
    (or None); False for ('tsdf','weight'); any other combination is not supported."""
    err = NotImplementedError(f"only attr_names=('tsdf','weight') (the reference's o3d_utils.py:172 layout) and "
                              f"('tsdf','weight','color') with float32 attributes and channels ((1),(1),(3)) are "
                              f"supported, got {names}, dtypes {dtypes}, channels {channels}")
    if names == ("tsdf", "weight"):
        return False
    if names != ("tsdf", "weight", "color"):
        raise err
    if dtypes is not None and (len(tuple(dtypes)) != 3 or not all(_is_float32(d) for d in dtypes)):
        raise err
    if channels is not None:
        try:
            ch = [[int(v) for v in np.asarray(c).reshape(-1)] for c in channels]
        except (TypeError, ValueError):
            raise err from None
        if ch != [[1], [1], [3]]:
            raise err
    return True


def _mat(m, shape) -> np.ndarray:
    if hasattr(m, "numpy"):
        m = m.numpy()
    a = np.ascontiguousarray(m, dtype=np.float64)
    if a.shape != shape:
        raise ValueError(f"expected matrix of shape {shape}, got {a.shape}")
    return a


# Released grids kept for reuse: creating and destroying a grid (its HBM pool and hash table, its streams)
# cost ~2.6 ms per fresh volume, which the fragment path pays once per 100 frames (tools/fragment_probe.py).
# A released grid that never grew is reset (the state of a new grid, mqr_vbg_reset) and handed to the next
# VoxelBlockGrid of the same voxel size, resolution, block count and device.  Budget per process: at most
# SPARE_GRIDS kept in total, only grids whose pool is at most SPARE_MAX_BYTES (the reference's default
# 50 000-block grid at R = 16 is 1.64 GB; a large volume's HBM is not held back), and only while at least
# SPARE_MIN_FREE of the device's HBM stays free (hipMemGetInfo).  A create that fails while spares are
# held releases them and tries once more.  A 4-process fragment pool on one GPU thus holds <= 8 GiB.
SPARE_GRIDS = 1
SPARE_MAX_BYTES = 2 << 30
SPARE_MIN_FREE = 0.25
_spares = []  # [(key, handle)]
_spares_lock = threading.Lock()


def _hbm_headroom(device) -> bool:
    """At least SPARE_MIN_FREE of `device`'s HBM is free (a spare grid is kept only then)."""
    free, total = ctypes.c_int64(), ctypes.c_int64()
    if _lib._lib.mqr_device_mem_info(int(device), ctypes.byref(free), ctypes.byref(total)) != 0 or total.value <= 0:
        return False
    return free.value >= SPARE_MIN_FREE * total.value


def release_spare_grids():
    """Destroy the kept released grids (their HBM is freed)."""
    with _spares_lock:
        hs = [h for _, h in _spares]
        _spares.clear()
    for h in hs:
        _lib._lib.mqr_vbg_destroy(h)


class VoxelBlockGrid:
    def __init__(self, attr_names=("tsdf", "weight"), attr_dtypes=None, attr_channels=None, voxel_size=0.01,
                 block_resolution=16, block_count=50_000, device=None):
        self._color = _wants_color(tuple(attr_names), attr_dtypes, attr_channels)
        self.voxel_size = float(voxel_size)
        self.block_resolution = int(block_resolution)
        self.device = device
        self.device_id = parse_device(device)
        # (a coloured grid is never kept or handed out as a spare: no key)
        self._key = None if self._color else (self.voxel_size, self.block_resolution, int(block_count),
                                              self.device_id)
        create = "mqr_vbg_create_color" if self._color else "mqr_vbg_create"
        with _spares_lock:
            i = next((j for j, (k, _) in enumerate(_spares) if k == self._key), None) if self._key else None
            h = _spares.pop(i)[1] if i is not None else None
        if h is None:
            h = ctypes.c_void_p()
            try:
                call(create, self.voxel_size, self.block_resolution, int(block_count), self.device_id,
                     ctypes.byref(h))
            except _lib.MqrError:
                with _spares_lock:
                    held = bool(_spares)
                if not held:
                    raise
                release_spare_grids()  # their HBM may be what the new grid lacks
                h = ctypes.c_void_p()
                call(create, self.voxel_size, self.block_resolution, int(block_count), self.device_id,
                     ctypes.byref(h))
        self._h = h

    # -- lifetime -----------------------------------------------------------------------------
    def __del__(self):
        h = getattr(self, "_h", None)
        if h is None or not h.value or _lib._lib is None:
            return
        self._h = None
        try:  # (at interpreter exit the module's globals may already be gone: then just destroy)
            key = None if getattr(self, "_profiled", False) else getattr(self, "_key", None)
            cap = ctypes.c_int64(-1)
            # (the integrate configuration back to a new grid's default, then emptied)
            if (key is not None and SPARE_GRIDS > 0 and key[2] * key[1] ** 3 * 8 <= SPARE_MAX_BYTES
                    and _hbm_headroom(key[3])
                    and _lib._lib.mqr_vbg_capacity(h, ctypes.byref(cap)) == 0
                    and cap.value == key[2] and _lib._lib.mqr_vbg_set_variant(h, 0) == 0
                    and _lib._lib.mqr_vbg_reset(h) == 0):
                with _spares_lock:
                    if len(_spares) < SPARE_GRIDS:
                        _spares.append((key, h))
                        return
        except Exception:  # noqa: BLE001
            pass
        _lib._lib.mqr_vbg_destroy(h)

    @property
    def handle(self):
        return self._h

    @property
    def has_color(self) -> bool:
        """The volume carries the 'color' attribute (three float32 channels per voxel, 0..255)."""
        return self._color

    def reset(self):
        """Empty the grid in place (same state as a new grid, allocations kept)."""
        call("mqr_vbg_reset", self._h)

    def export_keys(self) -> np.ndarray:
        n = self.size()
        keys = np.empty((n, 3), np.int32)
        if n:
            call("mqr_vbg_export", self._h, ptr(keys), None, None, MQR_HOST)
        return keys

    def pack_weighted(self, union_keys_dev_ptr, U, out_dev_ptr):
        """[U][R^3][2] (w*tsdf, w) float32 into device memory, zeros for absent blocks."""
        call("mqr_vbg_pack_weighted", self._h, ctypes.c_void_p(union_keys_dev_ptr), int(U),
             ctypes.c_void_p(out_dev_ptr))

    def unpack_weighted(self, union_keys_dev_ptr, U, in_dev_ptr):
        """Activate the union keys and set tsdf = sum(w*tsdf)/sum(w), weight = sum(w)."""
        call("mqr_vbg_unpack_weighted", self._h, ctypes.c_void_p(union_keys_dev_ptr), int(U),
             ctypes.c_void_p(in_dev_ptr))

    def size(self) -> int:
        n = ctypes.c_int64()
        call("mqr_vbg_size", self._h, ctypes.byref(n))
        return n.value

    def capacity(self) -> int:
        n = ctypes.c_int64()
        call("mqr_vbg_capacity", self._h, ctypes.byref(n))
        return n.value

    # -- per-frame Open3D API -------------------------------------------------------------------
    def compute_unique_block_coordinates(self, depth, intrinsic, extrinsic, depth_scale=_O3D_DEPTH_SCALE,
                                         depth_max=_O3D_DEPTH_MAX, trunc_voxel_multiplier=_O3D_TRUNC):
        d = _depth_array(depth)
        H, W = d.shape
        K = _mat(intrinsic, (3, 3))
        T = _mat(extrinsic, (4, 4))
        out = np.empty((max(4 * (H // 4) * (W // 4), 1), 3), np.int32)
        n = ctypes.c_int64()
        call("mqr_touch", self._h, ptr(d), MQR_HOST, H, W, ptr(K, _lib._f64p), ptr(T, _lib._f64p),
             float(depth_scale), float(depth_max), float(trunc_voxel_multiplier), ptr(out, _lib._i32p),
             ctypes.byref(n))
        return Tensor(out[: n.value].copy())

    def integrate(self, block_coords, depth, *args, **kwargs):
        """Open3D's three overloads, told apart by the third argument being an H x W x 3 image:

            integrate(block_coords, depth, intrinsic, extrinsic, depth_scale, depth_max, trunc_voxel_multiplier)
            integrate(block_coords, depth, color, intrinsic, extrinsic, ...)
            integrate(block_coords, depth, color, depth_intrinsic, color_intrinsic, extrinsic, ...)

        The colour ones need a coloured volume and a uint8 image (anything else is a ValueError); the depth-only
        one stays legal on a coloured volume and leaves its colours alone."""
        if "color" in kwargs or (args and _is_color_image(args[0])):
            return self._integrate_color(block_coords, depth, *args, **kwargs)
        return self._integrate_depth(block_coords, depth, *args, **kwargs)

    def _integrate_color(self, block_coords, depth, color, *mats, depth_intrinsic=None, color_intrinsic=None,
                         intrinsic=None, extrinsic=None, depth_scale=_O3D_DEPTH_SCALE, depth_max=_O3D_DEPTH_MAX,
                         trunc_voxel_multiplier=_O3D_TRUNC):
        mats = list(mats)
        # positional tail: (intrinsic, extrinsic, ...) or (depth_intrinsic, color_intrinsic, extrinsic, ...)
        two_k = len(mats) >= 2 and tuple(np.shape(_plain_array(mats[1]))) == (3, 3)
        order = (["depth_intrinsic", "color_intrinsic", "extrinsic"] if two_k or len(mats) == 0 else
                 ["intrinsic", "extrinsic"]) + ["depth_scale", "depth_max", "trunc_voxel_multiplier"]
        if len(mats) > len(order):
            raise TypeError("integrate: too many positional arguments")
        given = dict(depth_intrinsic=depth_intrinsic, color_intrinsic=color_intrinsic, intrinsic=intrinsic,
                     extrinsic=extrinsic, depth_scale=depth_scale, depth_max=depth_max,
                     trunc_voxel_multiplier=trunc_voxel_multiplier)
        given.update(zip(order, mats))
        kd = given["depth_intrinsic"] if given["depth_intrinsic"] is not None else given["intrinsic"]
        kc = given["color_intrinsic"] if given["color_intrinsic"] is not None else given["intrinsic"]
        if kd is None or kc is None or given["extrinsic"] is None:
            raise TypeError("integrate: intrinsics and extrinsic are required")
        c = _color_array(color)
        if not self._color:
            raise ValueError("integrate: the volume carries no colour (attr_names=('tsdf','weight','color'))")
        keys = np.ascontiguousarray(block_coords.numpy() if hasattr(block_coords, "numpy") else block_coords,
                                    dtype=np.int32).reshape(-1, 3)
        d = _depth_array(depth)
        H, W = d.shape
        Kd, Kc, T = _mat(kd, (3, 3)), _mat(kc, (3, 3)), _mat(given["extrinsic"], (4, 4))
        call("mqr_integrate_color", self._h, ptr(keys, _lib._i32p), keys.shape[0], ptr(d), MQR_HOST, H, W, ptr(c),
             MQR_HOST, c.shape[0], c.shape[1], ptr(Kd, _lib._f64p), ptr(Kc, _lib._f64p), ptr(T, _lib._f64p),
             float(given["depth_scale"]), float(given["depth_max"]), float(given["trunc_voxel_multiplier"]))

    def _integrate_depth(self, block_coords, depth, intrinsic, extrinsic=None, depth_scale=_O3D_DEPTH_SCALE,
                         depth_max=_O3D_DEPTH_MAX, trunc_voxel_multiplier=_O3D_TRUNC):
        keys = np.ascontiguousarray(block_coords.numpy() if hasattr(block_coords, "numpy") else block_coords,
                                    dtype=np.int32).reshape(-1, 3)
        d = _depth_array(depth)
        H, W = d.shape
        K = _mat(intrinsic, (3, 3))
        T = _mat(extrinsic, (4, 4))
        call("mqr_integrate", self._h, ptr(keys, _lib._i32p), keys.shape[0], ptr(d), MQR_HOST, H, W,
             ptr(K, _lib._f64p), ptr(T, _lib._f64p), float(depth_scale), float(depth_max),
             float(trunc_voxel_multiplier))

    # -- batched whole-sequence entry ---------------------------------------------------------------
    def integrate_frames(self, depths, intrinsics, extrinsics, frame_ok=None, depth_scale=1.0, depth_max=3.0,
                         trunc_voxel_multiplier=8.0, resident=False, colors=None, color_intrinsics=None):
        """touch + integrate for every frame in order (== sequential per-frame calls, bit for bit).

        depths: (B,H,W) float32 host array, or an ``_lib.DeviceBuffer`` holding B*H*W floats (then
        pass ``depths=(buffer, B, H, W)``); intrinsics (B,3,3), extrinsics (B,4,4) world->camera.
        resident=True (device frames only): the caller keeps the frames allocated and unchanged until it
        synchronizes the device (MQR_DEVICE_RESIDENT, include/mqr.h), so its stream does not wait for the
        call's integrates and the next call's first touch can overlap them.
        colors (a coloured volume only): the frames' colour images, uint8 (B,Hc,Wc,3) -- a host array, or device
        frames as a ``(buffer, B, Hc, Wc)`` tuple, a device-backed Tensor or a torch tensor on the GPU (what
        ``decode_color_frames(out_ptr=)`` filled); color_intrinsics (B,3,3) defaults to the depth intrinsics, and
        the colour frames must then have the depth frames' size.  With depth and colour both in HBM the call
        returns with its last integrate queued, as the depth-only call does."""
        if isinstance(depths, tuple):
            buf, B, H, W = depths
            dptr, loc = buf.ptr, (MQR_DEVICE_RESIDENT if resident else MQR_DEVICE)
            keep = None
        else:
            keep = np.ascontiguousarray(depths, dtype=np.float32)
            B, H, W = keep.shape
            dptr, loc = ptr(keep), MQR_HOST
        K = np.ascontiguousarray(intrinsics, dtype=np.float64).reshape(B, 3, 3)
        T = np.ascontiguousarray(extrinsics, dtype=np.float64).reshape(B, 4, 4)
        ok = None if frame_ok is None else np.ascontiguousarray(frame_ok, dtype=np.uint8)
        if colors is None:
            if color_intrinsics is not None:
                raise ValueError("integrate_frames: color_intrinsics without colors")
            call("mqr_integrate_frames", self._h, dptr, loc, B, H, W, ptr(K, _lib._f64p), ptr(T, _lib._f64p),
                 None if ok is None else ptr(ok, _lib._u8p), float(depth_scale), float(depth_max),
                 float(trunc_voxel_multiplier))
            del keep
            return
        dev = _device_colors(colors)
        if dev is not None:
            cptr, Bc, Hc, Wc, ckeep = dev
            cloc = MQR_DEVICE
        else:
            ckeep = _color_array(colors, ndim=4)
            Bc, Hc, Wc = ckeep.shape[:3]
            cptr, cloc = ptr(ckeep), MQR_HOST
        if not self._color:
            raise ValueError("integrate_frames: the volume carries no colour (attr_names=('tsdf','weight','color'))")
        if resident:
            raise ValueError("integrate_frames: resident frames are not supported with colours")
        if Bc != B:
            raise ValueError(f"{Bc} colour frames for {B} depth frames")
        if color_intrinsics is None:
            if (Hc, Wc) != (H, W):
                raise ValueError(f"colour frames are {Hc} x {Wc}, depth frames {H} x {W}: give color_intrinsics")
            Kc = K
        else:
            Kc = np.ascontiguousarray(color_intrinsics, dtype=np.float64).reshape(B, 3, 3)
        call("mqr_integrate_frames_color", self._h, dptr, loc, B, H, W, cptr, cloc, Hc, Wc, ptr(K, _lib._f64p),
             ptr(Kc, _lib._f64p), ptr(T, _lib._f64p), None if ok is None else ptr(ok, _lib._u8p), float(depth_scale),
             float(depth_max), float(trunc_voxel_multiplier))
        del keep, ckeep

    # -- extraction --------------------------------------------------------------------------------
    def _geom(self, fn, thr):
        """The extraction's result, left in HBM (DeviceGeom): host arrays are copied on first access."""
        from .geometry import DeviceGeom
        g = ctypes.c_void_p()
        try:
            call(fn, self._h, float(thr), ctypes.byref(g))
        except _lib.MqrError:
            if g.value:  # a failed extraction may still have handed out its result object
                _lib._lib.mqr_geom_free(g)
            raise
        try:
            return DeviceGeom(g, self.device_id)
        except Exception:
            _lib._lib.mqr_geom_free(g)
            raise

    def extract_point_cloud(self, weight_threshold=3.0, estimated_point_number=-1):
        """Open3D returns the cloud on the volume's device; so does this (positions / normals in HBM,
        copied to the host on first host access)."""
        return PointCloud.from_device(self._geom("mqr_extract_points", weight_threshold), device=self.device)

    def extract_triangle_mesh(self, weight_threshold=3.0, estimated_vertex_number=-1):
        """The mesh on the volume's device, as Open3D returns it (arrays in HBM until a host access)."""
        return TriangleMesh.from_device(self._geom("mqr_extract_mesh", weight_threshold), device=self.device)

    # -- rendering ---------------------------------------------------------------------------------
    _RENDER_ATTRIBUTES = ("depth", "vertex", "normal", "color")

    def ray_cast_frames(self, intrinsics, extrinsics, width, height, render_attributes=("depth",),
                        depth_scale=_O3D_DEPTH_SCALE, depth_min=0.1, depth_max=_O3D_DEPTH_MAX, weight_threshold=3.0,
                        trunc_voxel_multiplier=_O3D_TRUNC, range_map_down_factor=8, block_coords=None,
                        pixel_offset=0.0, refine=False):
        """Depth / vertex / normal / colour maps of the fused surface for a stack of same-size cameras (intrinsics
        (n,3,3), extrinsics (n,4,4) world -> camera), marched through the volume itself (csrc/volumecast.hip,
        DESIGN.md §2.10): a dict of Tensors over device buffers, "depth" (n, H, W), "vertex" and "normal"
        (n, H, W, 3), 0 where a ray hits nothing; "color" (n, H, W, 3) in 0..1 on a coloured volume (§2.11), a
        ValueError on any other.  pixel_offset 0.5 casts the rays of
        ``RaycastingScene.create_rays_pinhole``; refine re-interpolates each crossing trilinearly."""
        from ._lib import DeviceBuffer
        from .geometry import DeviceArray
        attrs = tuple(render_attributes)
        bad = [a for a in attrs if a not in self._RENDER_ATTRIBUTES]
        if bad or not attrs:
            raise ValueError(f"render_attributes must be among {self._RENDER_ATTRIBUTES}, got {attrs}")
        if "color" in attrs and not self._color:
            raise ValueError(f"render_attributes {attrs}: the volume carries no colour "
                             f"(attr_names=('tsdf','weight','color'))")
        K = np.ascontiguousarray(intrinsics, dtype=np.float64).reshape(-1, 3, 3)
        T = np.ascontiguousarray(extrinsics, dtype=np.float64).reshape(-1, 4, 4)
        if len(K) != len(T):
            raise ValueError(f"{len(K)} intrinsics for {len(T)} extrinsics")
        n, H, W = len(K), int(height), int(width)
        keys, nk = None, 0
        if block_coords is not None:
            keys = np.ascontiguousarray(block_coords.numpy() if hasattr(block_coords, "numpy") else block_coords,
                                        dtype=np.int32).reshape(-1, 3)
            nk = keys.shape[0]
            if nk == 0:  # an empty list (a non-null pointer, no rows) bounds nothing: all misses
                keys = np.zeros((1, 3), np.int32)
        outs = {}
        for a in self._RENDER_ATTRIBUTES:
            if a in attrs:
                k = () if a == "depth" else (3,)
                outs[a] = (DeviceBuffer(max(4, 4 * max(n, 0) * max(H, 0) * max(W, 0) * (3 if k else 1)),
                                        self.device_id), k)
        p = {a: (outs[a][0].ptr if a in outs else None) for a in self._RENDER_ATTRIBUTES}
        head = (self._h, None if keys is None else ptr(keys), nk, MQR_HOST, ptr(K, _lib._f64p), ptr(T, _lib._f64p), n, H,
                W, float(depth_scale), float(depth_min), float(depth_max), float(weight_threshold),
                float(trunc_voxel_multiplier), int(range_map_down_factor), float(pixel_offset), 1 if refine else 0,
                p["depth"], p["vertex"], p["normal"])
        if p["color"] is None:
            call("mqr_vbg_ray_cast", *head, MQR_DEVICE)
        else:
            call("mqr_vbg_ray_cast_color", *head, p["color"], MQR_DEVICE)
        return {a: Tensor(DeviceArray(buf, buf.ptr.value, (n, H, W) + k, np.float32, self.device_id))
                for a, (buf, k) in outs.items()}

    def ray_cast(self, block_coords, intrinsic, extrinsic, width, height, render_attributes=("depth",),
                 depth_scale=_O3D_DEPTH_SCALE, depth_min=0.1, depth_max=_O3D_DEPTH_MAX, weight_threshold=3.0,
                 trunc_voxel_multiplier=_O3D_TRUNC, range_map_down_factor=8):
        """Open3D's ``VoxelBlockGrid.ray_cast`` (its argument order and defaults): a dict with "depth" (H, W, 1),
        "vertex", "normal" and (a coloured volume) "color" (H, W, 3) as asked for.  block_coords=None: every active
        block."""
        r = self.ray_cast_frames(_mat(intrinsic, (3, 3)), _mat(extrinsic, (4, 4)), width, height, render_attributes,
                                 depth_scale, depth_min, depth_max, weight_threshold, trunc_voxel_multiplier,
                                 range_map_down_factor, block_coords=block_coords)
        from .geometry import DeviceArray
        H, W = int(height), int(width)
        return {a: Tensor(DeviceArray(t.device_array().owner, t.device_array().ptr, (H, W, 1 if a == "depth" else 3),
                                      np.float32, self.device_id)) for a, t in r.items()}

    def ray_cast_last_ms(self):
        """(range map, march) device time of the last ray cast on this volume's device, ms."""
        a, b = ctypes.c_double(), ctypes.c_double()
        call("mqr_vbg_ray_cast_last_ms", self._h, ctypes.byref(a), ctypes.byref(b))
        return a.value, b.value

    # -- contents ----------------------------------------------------------------------------------
    def export(self):
        """(keys (N,3) int32, tsdf (N,R,R,R) f32, weight (N,R,R,R) f32) in buffer order; a coloured volume adds
        its colours (N,R,R,R,3) f32 in 0..255 as a fourth array."""
        n = self.size()
        R = self.block_resolution
        keys = np.empty((n, 3), np.int32)
        tsdf = np.empty((n, R, R, R), np.float32)
        wgt = np.empty((n, R, R, R), np.float32)
        if n:
            call("mqr_vbg_export", self._h, ptr(keys), ptr(tsdf), ptr(wgt), MQR_HOST)
        if self._color:
            col = np.empty((n, R, R, R, 3), np.float32)
            if n:
                call("mqr_vbg_export_color", self._h, ptr(col), MQR_HOST)
            return keys, tsdf, wgt, col
        return keys, tsdf, wgt

    def import_blocks(self, keys, tsdf, weight, color=None):
        """Add blocks; color (N,R,R,R,3) float32 in 0..255 for a coloured volume (left at zero when not given)."""
        keys = np.ascontiguousarray(keys, dtype=np.int32).reshape(-1, 3)
        tsdf = np.ascontiguousarray(tsdf, dtype=np.float32)
        weight = np.ascontiguousarray(weight, dtype=np.float32)
        if color is not None:
            if not self._color:
                raise ValueError("import_blocks: the volume carries no colour")
            color = np.ascontiguousarray(color, dtype=np.float32)
            if color.size != tsdf.size * 3:
                raise ValueError(f"color must hold 3 channels per voxel, got shape {color.shape}")
        call("mqr_vbg_import", self._h, ptr(keys), ptr(tsdf), ptr(weight), keys.shape[0], MQR_HOST)
        if color is not None and keys.shape[0]:
            call("mqr_vbg_import_color", self._h, ptr(keys), ptr(color), keys.shape[0], MQR_HOST)

    def save(self, file_name):
        """npz with Open3D's VoxelBlockGrid::Save keys: voxel_size, block_resolution, key, tsdf, weight, and
        color (N,R,R,R,3) for a coloured volume (a colourless file is byte for byte what it was)."""
        keys, tsdf, wgt, *col = self.export()
        R = self.block_resolution
        extra = {"color": col[0]} if col else {}
        np.savez(file_name, voxel_size=np.array([self.voxel_size], np.float32),
                 block_resolution=np.array([R], np.int64), key=keys,
                 tsdf=tsdf.reshape(-1, R, R, R, 1), weight=wgt.reshape(-1, R, R, R, 1), **extra)

    @staticmethod
    def load(file_name, device=None):
        data = np.load(file_name, allow_pickle=False)
        R = int(np.asarray(data["block_resolution"]).reshape(-1)[0])
        keys = np.asarray(data["key"], np.int32).reshape(-1, 3)
        colored = "color" in data.files  # a file with the key loads as a coloured volume
        vbg = VoxelBlockGrid(attr_names=("tsdf", "weight", "color") if colored else ("tsdf", "weight"),
                             voxel_size=float(np.asarray(data["voxel_size"]).reshape(-1)[0]), block_resolution=R,
                             block_count=max(len(keys), 1), device=device)
        if len(keys):
            vbg.import_blocks(keys, np.asarray(data["tsdf"]).reshape(-1, R, R, R),
                              np.asarray(data["weight"]).reshape(-1, R, R, R),
                              color=np.asarray(data["color"]).reshape(-1, R, R, R, 3) if colored else None)
        return vbg

    # -- profiling ---------------------------------------------------------------------------------
    def profile(self, enable=True, touch=False):
        """Per-launch timing events (stats()['integrate_ms']); touch=True also times the touch launches."""
        call("mqr_vbg_profile", self._h, (2 if touch else 1) if enable else 0)
        self._profiled = True  # (its timing state stays with it: not kept for reuse)

    def stats(self, reset=False) -> dict:
        s = MqrStats()
        call("mqr_vbg_stats", self._h, ctypes.byref(s), 1 if reset else 0)
        return {k: getattr(s, k) for k, _ in MqrStats._fields_}
