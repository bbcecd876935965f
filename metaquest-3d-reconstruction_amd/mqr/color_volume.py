"""Fuse colour frames into a coloured TSDF volume: the quick way from a capture's colour
frames to a coloured mesh, cloud or rendered image -- no mesh, BVH, per-vertex projection or rigid optimiser.
Cruder than ``optimize_color_pose`` + ``color_map`` (one nearest pixel per voxel and frame, the colour poses
as given), which it complements and does not replace.

The chain stays in HBM: a geometry volume, depth rendered from it at the colour poses
(``VoxelBlockGrid.ray_cast_frames``), the colour integrate on those maps, then ``extract_triangle_mesh`` /
``extract_point_cloud`` / ``ray_cast(render_attributes=("color",))`` on the result.
"""
from __future__ import annotations

import numpy as np

from .vbg import VoxelBlockGrid, _device_colors

COLOR_ATTRS = ("tsdf", "weight", "color")


def _batches(n, batch):
    batch = max(1, int(batch))
    return [(i, min(i + batch, n)) for i in range(0, n, batch)]


def fuse_color_volume(images, intrinsics, extrinsics, depths=None, geometry=None, voxel_size=0.01,
                      block_resolution=16, block_count=50_000, depth_max=3.0, trunc_voxel_multiplier=8.0, device=None,
                      batch=32, weight_threshold=3.0, depth_min=0.1):
    """A coloured ``VoxelBlockGrid`` from colour frames and the depth seen from their poses.

    images: (N,H,W,3) uint8, a host array or device frames (what ``integrate_frames(colors=)`` takes);
    intrinsics (N,3,3) and extrinsics (N,4,4) world -> camera of the colour cameras.  Either ``depths``, the
    colour-aligned metric depth maps (N,H,W) float32 (0 or non-finite = nothing seen), or ``geometry``, a
    ``VoxelBlockGrid`` holding the surface: the maps are then rendered from it per batch of `batch` frames
    (``ray_cast_frames(depth_scale=1)``, its ``weight_threshold`` / ``depth_min``) and handed to the integrate
    without leaving HBM.  voxel_size, block_resolution, block_count, depth_max, trunc_voxel_multiplier and
    device are the coloured volume's and its integrate's."""
    if (depths is None) == (geometry is None):
        raise ValueError("fuse_color_volume: give either depths or geometry")
    K = np.ascontiguousarray(intrinsics, np.float64).reshape(-1, 3, 3)
    T = np.ascontiguousarray(extrinsics, np.float64).reshape(-1, 4, 4)
    dev = _device_colors(images)
    if dev is None:
        images = np.asarray(images)
        if images.dtype != np.uint8 or images.ndim != 4 or images.shape[3] != 3:
            raise ValueError(f"images must be uint8 (N,H,W,3), got {images.dtype} {images.shape}")
        N, H, W = images.shape[:3]
    else:
        N, H, W = dev[1:4]
    if len(K) != N or len(T) != N:
        raise ValueError(f"{N} images for {len(K)} intrinsics and {len(T)} extrinsics")
    if depths is not None:
        depths = np.asarray(depths, np.float32)
        if depths.shape != (N, H, W):
            raise ValueError(f"depths must be {(N, H, W)}, got {depths.shape}")
        depths = np.where(np.isfinite(depths), depths, np.float32(0))  # (a mesh cast marks a miss with inf)
    vbg = VoxelBlockGrid(attr_names=COLOR_ATTRS, voxel_size=voxel_size, block_resolution=block_resolution,
                         block_count=block_count, device=device)
    frame_bytes = H * W * 3
    for a, b in _batches(N, batch):
        if dev is None:
            colors = images[a:b]
        else:  # the batch's frames inside the device stack
            base = dev[0].value if hasattr(dev[0], "value") else int(dev[0])
            colors = (base + a * frame_bytes, b - a, H, W)
        if geometry is not None:
            d = geometry.ray_cast_frames(K[a:b], T[a:b], W, H, render_attributes=("depth",), depth_scale=1.0,
                                         depth_min=depth_min, depth_max=depth_max, weight_threshold=weight_threshold,
                                         trunc_voxel_multiplier=trunc_voxel_multiplier)["depth"]
            frames = (d.device_array(), b - a, H, W)
            ok = None
        else:
            frames = depths[a:b]
            ok = (frames > 0).reshape(b - a, -1).any(axis=1).astype(np.uint8)  # (an empty map is skipped, not an error)
            if not ok.any():
                continue
        vbg.integrate_frames(frames, K[a:b], T[a:b], frame_ok=ok, depth_scale=1.0, depth_max=depth_max,
                             trunc_voxel_multiplier=trunc_voxel_multiplier, colors=colors)
    return vbg


def build_color_volume(data_io, color_dataset_map, config=None, geometry=None, sides=None, **fuse_kw):
    """``fuse_color_volume`` over a capture: per side, the images through ``data_io.color.load_rgb_batch``, the
    poses through ``o3d_utils.dataset_intrinsics_extrinsics``, and -- without a `geometry` volume -- the
    colour-aligned depth maps ``render_color_aligned_depth`` wrote (``data_io.rgbd.load_color_aligned_depth``).
    config: an object or mapping with any of voxel_size, block_resolution, block_count, depth_max,
    trunc_voxel_multiplier, device, batch (`fuse_kw` overrides it).  Returns the coloured volume."""
    from .o3d_utils import dataset_intrinsics_extrinsics
    names = ("voxel_size", "block_resolution", "block_count", "depth_max", "trunc_voxel_multiplier", "device", "batch")
    kw = {}
    for n in names:
        v = config.get(n) if isinstance(config, dict) else getattr(config, n, None)
        if v is not None:
            kw[n] = v
    kw.update(fuse_kw)
    images, Ks, Ts, depths = [], [], [], []
    for side in (list(color_dataset_map) if sides is None else sides):
        ds = color_dataset_map[side]
        if len(ds) == 0:
            continue
        K, T = dataset_intrinsics_extrinsics(ds)
        images.append(data_io.color.load_rgb_batch(side, ds.timestamps, device=kw.get("device")
                                                   if isinstance(kw.get("device"), int) else None))
        Ks.append(K)
        Ts.append(T)
        if geometry is None:
            depths.append(np.stack([data_io.rgbd.load_color_aligned_depth(side=side, timestamp=int(t))
                                    for t in ds.timestamps]).astype(np.float32))
    if not images:
        raise ValueError("build_color_volume: no colour frames")
    if len({im.shape[1:] for im in images}) > 1:
        raise ValueError(f"colour frames of differing sizes: {sorted({im.shape[1:3] for im in images})}")
    return fuse_color_volume(np.concatenate(images), np.concatenate(Ks), np.concatenate(Ts),
                             depths=None if geometry is not None else np.concatenate(depths), geometry=geometry, **kw)
