"""Drop-in for the reference's colour-map stage
(processing/reconstruction/color_map_optimization/optimize_color_pose.py:11-100), without Open3D:

    from mqr.color_map_optimization import optimize_color_pose
    colored_mesh, color_dataset_map = optimize_color_pose(vbg, data_io, config)

Same order as the reference: extract the mesh, filter small components, ray-cast the colour-aligned
depth of every ``config.interval``-th colour frame of each side, run the rigid colour-map optimiser
(mqr.color.run_rigid_optimizer's device-resident loop) for ``config.max_iteration``
iterations, attach the vertex colours, filter again, and hand back the datasets with their transforms
replaced by the optimised poses.  The mesh stays in HBM from extraction to colours.
"""
from __future__ import annotations

import numpy as np

from .color import ColorMapOptimizer, RigidOptimizerOption
from .geometry import Tensor, device_mesh, mesh_fields
from .meshfilter import filter_mesh_components
from .models import CoordinateSystem, Side, Transforms
from .o3d_utils import dataset_intrinsics_extrinsics, extrinsics_to_transforms
from .raycasting import RaycastingScene
from .vbg import parse_device


def _colored(mesh, colors):
    mesh.vertex["colors"] = Tensor(np.ascontiguousarray(colors, dtype=np.float32))
    return mesh


def _filter_colored(mesh, colors, min_triangle_count):
    """filter_mesh_components of a coloured mesh: the colours follow their vertices."""
    nv = len(mesh.vertex.positions)
    out = filter_mesh_components(mesh, min_triangle_count=min_triangle_count)
    if out is mesh or len(out.vertex.positions) == nv:  # nothing dropped: the filter keeps the vertex order
        return _colored(out, colors)
    # vertices were dropped: a second pass carries the colours through the filter's per-vertex channel
    from .geometry import TriangleMesh
    carry = filter_mesh_components(TriangleMesh(mesh.vertices, colors, mesh.triangles, device=mesh.device),
                                   min_triangle_count=min_triangle_count)
    return _colored(out, carry.vertex_normals)


def optimize_color_pose(vbg, data_io, config, sides=None):
    """-> (colored_mesh, {side: color_dataset}).  `data_io.color` needs load_color_dataset(side=,
    use_cache=) and load_rgb(side=, timestamp=) (the reference's DataIO has both); where it also has
    load_rgb_batch(side, timestamps, device=) (mqr.dataio.ImageDataIO), each side's frames come from one
    call of that; `config` the fields of the reference's ColorOptimizationConfig.  `sides`: the Side members to walk (default: this package's
    Side enum, in order).  Keyframes of differing sizes raise ValueError."""
    mesh = vbg.extract_triangle_mesh(weight_threshold=config.weight_threshold,
                                     estimated_vertex_number=config.estimated_vertex_number)
    # Filter out small disconnected mesh components (e.g., floating body parts)
    mesh = filter_mesh_components(mesh, min_triangle_count=config.min_triangle_count)

    device = parse_device(getattr(mesh, "device", None) or getattr(config, "device", None))
    scene = RaycastingScene(device=device)
    on_device = device_mesh(mesh_fields(mesh), device) is not None
    if on_device:
        scene.add_triangles(mesh)
    else:
        scene.add_triangles(mesh.vertices, mesh.triangles)

    color_dataset_map = {}
    images, Ks, Ts = [], [], []
    for side in (Side if sides is None else sides):
        color_dataset = data_io.color.load_color_dataset(side=side, use_cache=config.use_dataset_cache)
        color_dataset = color_dataset[::config.interval]
        color_dataset_map[side] = color_dataset
        color_dataset.transforms = color_dataset.transforms.convert_coordinate_system(
            target_coordinate_system=CoordinateSystem.OPEN3D, is_camera=True)
        K, T = dataset_intrinsics_extrinsics(color_dataset)
        Ks.append(K)
        Ts.append(T)
        n = len(color_dataset.timestamps)
        if hasattr(data_io.color, "load_rgb_batch"):  # one batched read (raw frames decoded on the device)
            batch = np.asarray(data_io.color.load_rgb_batch(side, color_dataset.timestamps, device=device)) if n else ()
            if n and (batch.ndim != 4 or len(batch) != n):
                raise ValueError(f"load_rgb_batch must return ({n},H,W,3) uint8, got {batch.shape}")
        else:
            batch = (np.asarray(data_io.color.load_rgb(side=side, timestamp=color_dataset.timestamps[i]))
                     for i in range(n))
        for i, rgb in enumerate(batch):
            if rgb.ndim != 3 or rgb.shape[2] != 3:
                raise ValueError(f"load_rgb must return (H,W,3) uint8, got {rgb.shape}")
            if (rgb.shape[1], rgb.shape[0]) != (int(color_dataset.widths[i]), int(color_dataset.heights[i])):
                raise ValueError(f"colour frame {color_dataset.timestamps[i]} is {rgb.shape[1]}x{rgb.shape[0]}, its "
                                 f"dataset row says {color_dataset.widths[i]}x{color_dataset.heights[i]}")
            images.append(rgb)
    if len({im.shape for im in images}) > 1:
        raise ValueError(f"colour keyframes of differing sizes: {sorted({im.shape[:2] for im in images})}")

    N = len(images)
    K = np.concatenate(Ks) if Ks else np.zeros((0, 3, 3))
    T = np.concatenate(Ts) if Ts else np.zeros((0, 4, 4))
    option = RigidOptimizerOption(maximum_iteration=config.max_iteration)
    nv = len(mesh.vertex.positions)
    if N == 0 or nv == 0:
        colors, poses = np.zeros((nv, 3), np.float32), T
    else:
        H, W = images[0].shape[:2]
        t_hit = scene.cast_pinhole(K, T, W, H)["t_hit"]  # raycast_in_color_view, every keyframe in one cast
        v = mesh.vertex.positions if on_device else mesh.vertices
        with ColorMapOptimizer(v, np.stack(images), t_hit, K, T, option, device=device) as opt:
            opt.optimize(option.maximum_iteration)
            colors, _ = opt.colors()
            poses = opt.poses

    # Filter the colored mesh again after color optimization (the reference does, optimize_color_pose.py:75-84)
    print("[Info] Filtering colored mesh after color optimization...")
    colored_mesh = _filter_colored(mesh, colors, config.min_triangle_count)

    trajectory_transforms = extrinsics_to_transforms(poses)
    start_index = 0
    for side, color_dataset in color_dataset_map.items():
        end_index = start_index + len(color_dataset)
        color_dataset.transforms = Transforms(coordinate_system=trajectory_transforms.coordinate_system,
                                              positions=trajectory_transforms.positions[start_index:end_index],
                                              rotations=trajectory_transforms.rotations[start_index:end_index])
        start_index = end_index
    return colored_mesh, color_dataset_map
