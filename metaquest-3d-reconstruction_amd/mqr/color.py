"""Per-vertex colour projection from colour keyframes.

The reference colours the extracted mesh with Open3D's colour-map pipeline
(processing/reconstruction/color_map_optimization/optimize_color_pose.py:24-73): the filtered
mesh goes into a RaycastingScene, every colour keyframe gets a colour-aligned depth map from
``raycast_in_color_view`` (utils/o3d_utils.py:324-341), and ``run_rigid_optimizer`` assigns vertex
colours by visibility-tested averaging (upstream ColorMapUtils.cpp) while it refines the poses.
This module is that stage on the GPU.  The colour assignment with the keyframe poses as given
(run_rigid_optimizer at maximum_iteration = 0):

    colors, counts = color_map(vertices, images, t_hit, K, T_wc)      # complete upstream semantics
    colors, counts = project_vertex_colors(mesh, images, K, T_wc)     # ray casts t_hit first
    colors, counts = color_vertices(vertices, images, depths, K, T_wc)  # visibility + average only

color_map adds what run_rigid_optimizer does around the averaging (upstream ColorMapUtils /
RigidOptimizer / Image.cpp, recalled -- VERIFY): the RGBD depth truncated at 3 m
(create_from_color_and_depth), depth-discontinuity masks (Sobel > 0.1, dilated by 3 px), float64
means, and the mean of the 3 nearest sampled vertices for vertices no keyframe samples.  All on the
GPU (libmqr_hip.so: color.hip; raycast.hip for the depths).

The pose refinement itself -- run_rigid_optimizer at maximum_iteration > 0 -- is device resident too
(colormap.hip; the rules are DESIGN §2.4's, restated from Open3D as recalled):

    colors, counts, T_wc, residuals = run_rigid_optimizer(mesh, images, t_hit, K, T_wc,
                                                          RigidOptimizerOption(maximum_iteration=100))
    with ColorMapOptimizer(vertices, images, t_hit, K, T_wc) as o:    # the handle, step by step
        o.pairs_per_keyframe; o.proxy(); o.systems(); o.optimize(10); o.poses; o.colors()
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from ._lib import MQR_HOST, call, ptr

# Open3D RigidOptimizerOption defaults (maximum_allowable_depth, depth_threshold_for_visibility_check,
# image_boundary_margin)
MAX_DEPTH = 2.5
VISIBILITY_THRESHOLD = 0.03
MARGIN = 10
# ... depth_threshold_for_discontinuity_check, half_dilation_kernel_size_for_discontinuity_map,
# invisible_vertex_color_knn; and RGBDImage.create_from_color_and_depth's default depth_trunc
DISCONTINUITY_THRESHOLD = 0.1
HALF_DILATION = 3
KNN = 3
DEPTH_TRUNC = 3.0


def _resident_images(images, t_hit, device, keep):
    """The (N,H,W,3) uint8 keyframes and their (N,H,W) float32 depths as one pair of pointers in one place
    (the C ABI takes a single location for both): images or t_hit already in HBM on `device` (detected
    with mqr.geometry.device_ptr) are used in place and the other goes up beside them; both on the host
    stay there.  -> (N, H, W, image pointer, depth pointer, location); `keep` collects what must outlive
    the call."""
    from .geometry import device_ptr
    from ._lib import MQR_DEVICE, DeviceBuffer
    di = device_ptr(images, device) if getattr(images, "dtype", None) == np.uint8 else None
    if di is not None:
        shape = tuple(images.shape)
        if len(shape) != 4 or shape[3] != 3:
            raise ValueError(f"images must be (N,H,W,3) uint8, got {shape}")
        im = None
    else:
        im = np.ascontiguousarray(images.numpy() if hasattr(images, "numpy") else images, dtype=np.uint8)
        if im.ndim != 4 or im.shape[3] != 3:
            raise ValueError(f"images must be (N,H,W,3) uint8, got {im.shape}")
        shape = im.shape
    N, H, W = (int(x) for x in shape[:3])
    dt = device_ptr(t_hit, device) if getattr(t_hit, "dtype", None) == np.float32 else None
    tshape = tuple(t_hit.shape) if hasattr(t_hit, "shape") else np.shape(t_hit)
    if int(np.prod(tshape)) != N * H * W:
        raise ValueError(f"t_hit must be ({N},{H},{W}) float32, got {tshape}")
    if N == 0 or (di is None and dt is None):
        if im is None:
            im = np.ascontiguousarray(images.numpy(), dtype=np.uint8)
        d = np.ascontiguousarray(t_hit.numpy() if dt is not None else t_hit, dtype=np.float32).reshape(N, H, W)
        keep += [im, d]
        return N, H, W, ptr(im), ptr(d), MQR_HOST
    if di is not None:
        keep.append(images)
        iptr = ctypes.c_void_p(di[0])
    else:  # images go up beside the resident depths
        buf = DeviceBuffer.from_array(im, int(device))
        keep.append(buf)
        iptr = buf.ptr
    if dt is not None:
        keep.append(t_hit)
        tptr = ctypes.c_void_p(dt[0])
    else:
        buf = DeviceBuffer.from_array(np.ascontiguousarray(t_hit, dtype=np.float32).reshape(N, H, W), int(device))
        keep.append(buf)
        tptr = buf.ptr
    return N, H, W, iptr, tptr, MQR_DEVICE


def color_vertices(vertices, images, depths, K, T_wc, max_depth=MAX_DEPTH,
                   visibility_threshold=VISIBILITY_THRESHOLD, margin=MARGIN, device=0):
    """vertices (V,3) float32; images (N,H,W,3) uint8 RGB; depths (N,H,W) float32 colour-aligned
    depth; K (N,3,3), T_wc (N,4,4) world->camera.  Returns (colours (V,3) float32 in [0,1],
    counts (V,) int32 = keyframes averaged)."""
    V = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
    im = np.ascontiguousarray(images, dtype=np.uint8)
    if im.ndim != 4 or im.shape[3] != 3:
        raise ValueError(f"images must be (N,H,W,3) uint8, got {im.shape}")
    N, H, W = im.shape[:3]
    d = np.ascontiguousarray(depths, dtype=np.float32).reshape(N, H, W)
    Kd = np.ascontiguousarray(K, dtype=np.float64).reshape(N, 9)
    Td = np.ascontiguousarray(T_wc, dtype=np.float64).reshape(N, 16)
    out = np.empty((len(V), 3), np.float32)
    cnt = np.empty(len(V), np.int32)
    call("mqr_color_vertices", int(device), ptr(V), len(V), MQR_HOST, ptr(im), ptr(d), MQR_HOST, N, H, W,
         ptr(Kd, _lib._f64p), ptr(Td, _lib._f64p), float(max_depth), float(visibility_threshold), int(margin),
         ptr(out), ptr(cnt), MQR_HOST)
    return out, cnt


def color_map(vertices, images, t_hit, K, T_wc, max_depth=MAX_DEPTH, visibility_threshold=VISIBILITY_THRESHOLD,
              margin=MARGIN, discontinuity_threshold=DISCONTINUITY_THRESHOLD, half_dilation=HALF_DILATION,
              depth_trunc=DEPTH_TRUNC, knn=KNN, device=0):
    """run_rigid_optimizer's vertex colours with the poses as given.  t_hit (N,H,W) float32: the
    keyframes' raycast_in_color_view depth (inf on a miss).  Returns (colours (V,3) float32,
    counts (V,) int32 = keyframes averaged; 0 where the colour comes from the knn fill).  Vertices and
    t_hit already in HBM on `device` (a mesh from this package's extraction, a cast's t_hit Tensor) are
    used in place, and so are images held there."""
    from .geometry import device_ptr
    from ._lib import MQR_DEVICE
    keep = []
    N, H, W, iptr, tptr, iloc = _resident_images(images, t_hit, device, keep)
    dv = device_ptr(vertices, device) if getattr(vertices, "dtype", None) == np.float32 else None
    if dv is not None and vertices.shape[-1:] == (3,):
        nv, vptr, vloc = int(np.prod(vertices.shape[:-1])), ctypes.c_void_p(dv[0]), MQR_DEVICE
    else:
        V = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
        nv, vptr, vloc = len(V), ptr(V), MQR_HOST
    Kd = np.ascontiguousarray(K, dtype=np.float64).reshape(N, 9)
    Td = np.ascontiguousarray(T_wc, dtype=np.float64).reshape(N, 16)
    out = np.empty((nv, 3), np.float32)
    cnt = np.empty(nv, np.int32)
    call("mqr_color_map", int(device), vptr, nv, vloc, iptr, tptr, iloc, N, H, W,
         ptr(Kd, _lib._f64p), ptr(Td, _lib._f64p), float(max_depth), float(visibility_threshold), int(margin),
         float(discontinuity_threshold), int(half_dilation), float(depth_trunc), int(knn), ptr(out), ptr(cnt), MQR_HOST)
    del keep
    return out, cnt


def project_vertex_colors(mesh, images, K, T_wc, device=0, complete=True, **kw):
    """Ray-cast each keyframe's colour-aligned depth from `mesh` (raycast_in_color_view), then colour
    the vertices: color_map (complete=True) or the visibility-and-average primitive color_vertices.
    Returns (colours, counts)."""
    from .geometry import device_mesh, host_rows, mesh_fields
    from .raycasting import RaycastingScene
    im = np.asarray(images)
    N, H, W = im.shape[:3]
    scene = RaycastingScene(device=device)
    f = mesh_fields(mesh)
    if device_mesh(f, device) is not None:  # the mesh stays in HBM from extraction to colours
        v = f.positions
        scene.add_triangles(mesh)
    else:
        v = host_rows(f.positions, np.float32)
        scene.add_triangles(v, host_rows(f.triangles, np.int32))
    depth = scene.cast_pinhole(np.asarray(K, np.float64).reshape(N, 3, 3), np.asarray(T_wc, np.float64).reshape(N, 4, 4),
                               W, H)["t_hit"]
    if complete:
        return color_map(v, im, depth, K, T_wc, device=device, **kw)
    return color_vertices(v, im, depth.numpy(), K, T_wc, device=device, **kw)


# ------------------------------------------------------------------ rigid colour-map optimisation
class RigidOptimizerOption:
    """o3d.pipelines.color_map.RigidOptimizerOption: the same field names and defaults."""

    def __init__(self, maximum_iteration=0, maximum_allowable_depth=MAX_DEPTH,
                 depth_threshold_for_visibility_check=VISIBILITY_THRESHOLD,
                 depth_threshold_for_discontinuity_check=DISCONTINUITY_THRESHOLD,
                 half_dilation_kernel_size_for_discontinuity_map=HALF_DILATION, image_boundary_margin=MARGIN,
                 invisible_vertex_color_knn=KNN):
        self.maximum_iteration = int(maximum_iteration)
        self.maximum_allowable_depth = float(maximum_allowable_depth)
        self.depth_threshold_for_visibility_check = float(depth_threshold_for_visibility_check)
        self.depth_threshold_for_discontinuity_check = float(depth_threshold_for_discontinuity_check)
        self.half_dilation_kernel_size_for_discontinuity_map = int(half_dilation_kernel_size_for_discontinuity_map)
        self.image_boundary_margin = int(image_boundary_margin)
        self.invisible_vertex_color_knn = int(invisible_vertex_color_knn)

    def __repr__(self):
        return "RigidOptimizerOption(" + ", ".join(f"{k}={v!r}" for k, v in vars(self).items()) + ")"


class ColorMapOptimizer:
    """The device-resident rigid colour-map optimiser (libmqr_hip.so: colormap.hip).

    vertices (V,3) float32 (or a device mesh's positions), images (N,H,W,3) uint8, t_hit (N,H,W) float32
    colour-aligned depth, K (N,3,3), T_wc (N,4,4) world->camera.  Builds the utility images, the
    depth-boundary masks and both visibility lists at T_wc; vertices / images / t_hit already in HBM on
    `device` (e.g. the images mqr.colorframes.decode_color_frames wrote through out_ptr, wrapped in a device
    Tensor) are used in place (the vertices must outlive the optimiser)."""

    def __init__(self, vertices, images, t_hit, K, T_wc, option=None, depth_trunc=DEPTH_TRUNC, device=0):
        from .geometry import device_ptr
        from ._lib import MQR_DEVICE
        opt = option if option is not None else RigidOptimizerOption()
        self.option, self.device, self._h = opt, int(device), None
        self._keep = [vertices]
        N, H, W, iptr, tptr, iloc = _resident_images(images, t_hit, device, self._keep)
        Kd = np.ascontiguousarray(K, dtype=np.float64)
        Td = np.ascontiguousarray(T_wc, dtype=np.float64)
        if Kd.size != 9 * N or Td.size != 16 * N:
            raise ValueError(f"K must be ({N},3,3) and T_wc ({N},4,4), got {Kd.shape} and {Td.shape}")
        Kd, Td = Kd.reshape(N, 9), Td.reshape(N, 16)
        dv = device_ptr(vertices, device) if getattr(vertices, "dtype", None) == np.float32 else None
        if dv is not None and vertices.shape[-1:] == (3,):
            nv, vptr, vloc = int(np.prod(vertices.shape[:-1])), ctypes.c_void_p(dv[0]), MQR_DEVICE
        else:
            V = np.ascontiguousarray(vertices, dtype=np.float32)
            if V.ndim != 2 or V.shape[1] != 3:
                raise ValueError(f"vertices must be (V,3) float32, got {V.shape}")
            nv, vptr, vloc = len(V), ptr(V), MQR_HOST
        self.nv, self.N, self.H, self.W = nv, N, H, W
        self._T0 = Td.reshape(N, 4, 4).copy()
        h = ctypes.c_void_p()
        call("mqr_colormap_create", int(device), vptr, nv, vloc, iptr, tptr, iloc, N, H, W, ptr(Kd, _lib._f64p),
             ptr(Td, _lib._f64p), opt.maximum_allowable_depth, opt.depth_threshold_for_visibility_check,
             opt.image_boundary_margin, opt.depth_threshold_for_discontinuity_check,
             opt.half_dilation_kernel_size_for_discontinuity_map, float(depth_trunc), ctypes.byref(h))
        self._h = h

    def _handle(self):
        if self._h is None:
            raise ValueError("the optimiser is closed")
        return self._h

    @property
    def pairs_per_keyframe(self):
        """(N,) int64: the visibility pairs of each keyframe (fixed at construction)."""
        out = np.zeros(self.N, np.int64)
        call("mqr_colormap_counts", self._handle(), ptr(out, _lib._i64p))
        return out

    @property
    def poses(self):
        """(N,4,4) float64 world->camera: the current poses."""
        if self.N == 0 or self.nv == 0:
            return self._T0.copy()
        out = np.empty((self.N, 4, 4), np.float64)
        call("mqr_colormap_get_poses", self._handle(), ptr(out, _lib._f64p))
        return out

    @poses.setter
    def poses(self, T_wc):
        T = np.ascontiguousarray(T_wc, dtype=np.float64)
        if T.size != 16 * self.N:
            raise ValueError(f"T_wc must be ({self.N},4,4), got {T.shape}")
        call("mqr_colormap_set_poses", self._handle(), ptr(T, _lib._f64p))
        self._T0 = T.reshape(self.N, 4, 4).copy()

    def proxy(self):
        """Recompute and return the vertices' proxy intensities (V,) float64 at the current poses."""
        out = np.zeros(self.nv, np.float64)
        call("mqr_colormap_proxy", self._handle(), ptr(out, _lib._f64p))
        return out

    def systems(self):
        """One evaluation at the current poses and proxies, no update ->
        (JTJ (N,6,6), JTr (N,6), r2 (N,), count (N,) int64)."""
        N = self.N
        JTJ, JTr = np.zeros((N, 6, 6)), np.zeros((N, 6))
        r2, cnt = np.zeros(N), np.zeros(N, np.int64)
        call("mqr_colormap_systems", self._handle(), ptr(JTJ, _lib._f64p), ptr(JTr, _lib._f64p), ptr(r2, _lib._f64p),
             ptr(cnt, _lib._i64p))
        return JTJ, JTr, r2, cnt

    def optimize(self, n):
        """n iterations -> (residuals (n,) float64, term counts (n,) int64), read once at the end."""
        n = int(n)
        if n < 0:
            raise ValueError("the iteration count must be >= 0")
        res, cnt = np.zeros(n), np.zeros(n, np.int64)
        call("mqr_colormap_optimize", self._handle(), n, ptr(res, _lib._f64p), ptr(cnt, _lib._i64p))
        return res, cnt

    @property
    def last_optimize_ms(self):
        """Device time of the last optimize's launches (events around the loop on the handle's stream)."""
        ms = ctypes.c_float(0)
        call("mqr_colormap_optimize_ms", self._handle(), ctypes.byref(ms))
        return float(ms.value)

    def colors(self, knn=None):
        """(colours (V,3) float32, counts (V,) int32) at the current poses."""
        knn = self.option.invisible_vertex_color_knn if knn is None else int(knn)
        out = np.zeros((self.nv, 3), np.float32)
        cnt = np.zeros(self.nv, np.int32)
        call("mqr_colormap_colors", self._handle(), knn, ptr(out), ptr(cnt), MQR_HOST)
        return out, cnt

    def close(self):
        if self._h is not None:
            h, self._h = self._h, None
            call("mqr_colormap_destroy", h)
        self._keep = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def colormap_build_tag() -> str:
    """Hash of the colour-map optimiser's sources compiled into the loaded library."""
    buf = ctypes.create_string_buffer(64)
    call("mqr_colormap_build_tag", buf, 64)
    return buf.value.decode()


def run_rigid_optimizer(mesh_or_vertices, images, t_hit, K, T_wc, option=None, device=0):
    """o3d.pipelines.color_map.run_rigid_optimizer on the GPU: refine the keyframe poses for
    option.maximum_iteration iterations, then colour the vertices.  mesh_or_vertices: a mesh of this
    package (its positions are used, in HBM when they live there) or (V,3) float32 vertices.
    Returns (colours (V,3) float32, counts (V,) int32, T_wc (N,4,4) float64, residuals (iters,) float64)."""
    v = mesh_or_vertices
    if hasattr(v, "vertex") and hasattr(v.vertex, "positions"):
        v = v.vertex.positions
    elif hasattr(v, "vertices"):
        v = v.vertices
    opt = option if option is not None else RigidOptimizerOption()
    with ColorMapOptimizer(v, images, t_hit, K, T_wc, opt, device=device) as o:
        res, _ = o.optimize(opt.maximum_iteration)
        colors, counts = o.colors()
        return colors, counts, o.poses, res
