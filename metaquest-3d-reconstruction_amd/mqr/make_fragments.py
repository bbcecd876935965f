"""Drop-in for the reference's fragment generation
(scripts/processing/reconstruction/depth_optimization/make_fragments.py:14-308):

    frustum_overlap_filter(extrinsic_cw_1, extrinsic_cw_2, intrinsic_1, intrinsic_2, ...)      :14-81
    build_pose_graph_for_fragment(frag_dataset, depth_data_io, side, config)                   :84-248
    optimize_dataset_pose(depth_data_io, frag_dataset, side, config)                           :251-275
    make_fragment_datasets(depth_data_io, config)                                              :278-308

The reference computes one odometry information matrix per image pair -- 99 odometry pairs and up to
45 key-frame pairs of a 100-frame fragment -- each call loading and uploading its two frames again.
Here a fragment's frames are read once, decoded into HBM once (mqr.ingest), the pair list is built on
the host in the reference's order (odometry pairs, then the key-frame pairs that pass the frustum
filter) and ONE batched launch gives every matrix (mqr.odometry).  The graph is then optimised on the
host (mqr.posegraph).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional

import numpy as np

from ._io import io_pool
from .models import CoordinateSystem, DepthDataset, Side
from .posegraph import (GlobalOptimizationConvergenceCriteria, GlobalOptimizationOption, PoseGraph, PoseGraphEdge,
                        global_optimization)


@dataclass
class FragmentGenerationConfig:
    """reconstruction_config.py:43-56."""
    device: object = "CUDA:0"
    fragment_size: int = 100
    use_confidence_filtered_depth: bool = True
    confidence_threshold: float = 0.05
    valid_count_threshold: int = 4
    depth_max: float = 3.0
    odometry_loop_interval: int = 10
    overlap_ratio_threshold: float = 0.1
    loop_yaw_info_density_threshold: float = 0.3
    dist_threshold: float = 0.07
    edge_prune_threshold: float = 0.25
    use_dataset_cache: bool = True
    use_multi_threading: bool = False


def _frustum_box(extrinsic_cw, intrinsic, image_size, z_near, z_far):
    """World-space axis-aligned box (lower corner, upper corner) around ten points of a camera's frustum:
    along the rays through the four corner pixels and the centre pixel (width // 2, height // 2), the
    points at distance z_near and at distance z_far from the camera centre.  The ray slopes are formed in
    the intrinsic matrix's own precision (float32 from compute_o3d_intrinsic_matrices, as the reference's
    scalar arithmetic leaves them), everything after that in float64."""
    intrinsic = np.asarray(intrinsic)
    width, height = image_size
    pixels = np.array([[0, 0], [width - 1, 0], [width - 1, height - 1], [0, height - 1],
                       [width // 2, height // 2]], intrinsic.dtype if intrinsic.dtype.kind == "f" else np.float64)
    rays = np.ones((5, 3))
    rays[:, 0] = (pixels[:, 0] - intrinsic[0, 2]) / intrinsic[0, 0]
    rays[:, 1] = (pixels[:, 1] - intrinsic[1, 2]) / intrinsic[1, 1]
    rays /= np.linalg.norm(rays, axis=1, keepdims=True)
    in_camera = np.concatenate([rays * z_near, rays * z_far])
    R, t = np.asarray(extrinsic_cw)[:3, :3], np.asarray(extrinsic_cw)[:3, 3]
    in_world = in_camera @ R.T + t
    return in_world.min(axis=0), in_world.max(axis=0)


def frustum_overlap_ratio(extrinsic_cw_1, extrinsic_cw_2, intrinsic_1, intrinsic_2, image_size_1, image_size_2,
                          z_near: float = 0.1, z_far: float = 3.0) -> float:
    """Volume shared by the two cameras' frustum boxes (_frustum_box) over the smaller box's volume; 0.0
    when the boxes do not meet."""
    lo1, hi1 = _frustum_box(extrinsic_cw_1, intrinsic_1, image_size_1, z_near, z_far)
    lo2, hi2 = _frustum_box(extrinsic_cw_2, intrinsic_2, image_size_2, z_near, z_far)
    shared = np.clip(np.minimum(hi1, hi2) - np.maximum(lo1, lo2), 0.0, None).prod()
    if shared == 0.0:
        return 0.0
    return float(shared / min((hi1 - lo1).prod(), (hi2 - lo2).prod()))


def frustum_overlap_filter(extrinsic_cw_1, extrinsic_cw_2, intrinsic_1, intrinsic_2, image_size_1, image_size_2,
                           z_near: float = 0.1, z_far: float = 3.0, overlap_ratio_threshold: float = 0.05) -> bool:
    """make_fragments.py:14-81: do the two cameras' frustum boxes overlap by more than the threshold?"""
    return frustum_overlap_ratio(extrinsic_cw_1, extrinsic_cw_2, intrinsic_1, intrinsic_2, image_size_1, image_size_2,
                                 z_near, z_far) > overlap_ratio_threshold


def _fragment_name(frag_dataset, side) -> str:
    ts = frag_dataset.timestamps
    span = f"timestamps {ts[0]}..{ts[-1]}" if len(ts) else "no frames"
    return f"{getattr(side, 'name', side)} fragment ({len(ts)} frames, {span})"


def load_fragment_frames(depth_data_io, frag_dataset, side, config):
    """The fragment's frames, read once and decoded into HBM once: (DeviceBuffer of N*H*W metric float32,
    loaded (N,) bool, H, W).  ``loaded[i]`` is False where the reference's load_depth_map gives None (a
    missing file or an invalid buffer); the confidence mask is applied as load_depth_map applies it
    (o3d_utils.py:109-150).  Frames of different sizes raise ValueError."""
    from ._lib import DeviceBuffer
    from .dataio import DepthDataIO
    from .ingest import decode_depth_frames
    from .o3d_utils import _masked_depth, _raw_reader
    from .vbg import parse_device
    N = len(frag_dataset.timestamps)
    sizes = {(int(h), int(w)) for h, w in zip(frag_dataset.heights, frag_dataset.widths)}
    if len(sizes) != 1:
        raise ValueError(f"{_fragment_name(frag_dataset, side)}: its frames differ in size {sorted(sizes)}; "
                         "one batched odometry call needs frames of one size")
    (H, W), = sizes
    device = parse_device(config.device)
    masked = bool(config.use_confidence_filtered_depth)
    read_raw = _raw_reader(depth_data_io, side)
    ts = frag_dataset.timestamps
    if read_raw is None:
        # a data IO without raw-buffer access: its own decode, frame by frame, uploaded once
        frames = np.zeros((N, H, W), np.float32)
        loaded = np.zeros(N, bool)

        def one_decoded(i):
            msgs = []
            d = _masked_depth(depth_data_io, side, i, frag_dataset, masked, config.confidence_threshold,
                              config.valid_count_threshold, warn=msgs.append)
            if d is not None:
                frames[i] = d
                loaded[i] = True
            return msgs
        for msgs in io_pool().map(one_decoded, range(N)):
            for m in msgs:
                print(m)
        return DeviceBuffer.from_array(frames, device), loaded, H, W
    raw = np.zeros((N, H, W), np.float32)
    mask = np.zeros((N, H, W), np.uint8) if masked else None
    has = np.zeros(N, bool)

    def one(i):  # -> warning or None
        r = read_raw(ts[i], W, H)
        if r is None:
            return None  # a zero buffer: the decode flags it invalid
        raw[i] = r
        if not masked or not DepthDataIO.is_depth_map_valid(r):
            return None
        cm = depth_data_io.load_confidence_map(side=side, timestamp=ts[i])
        if cm is None:
            return f"[Warning] Confidence map not found for timestamp {ts[i]}"
        m = mask[i].view(np.bool_)
        np.less(cm.confidence_map, config.confidence_threshold, out=m)
        m |= cm.valid_count < config.valid_count_threshold
        has[i] = True
        return None
    for msg in io_pool().map(one, range(N)):
        if msg:
            print(msg)
    buf = DeviceBuffer(4 * N * H * W, device)
    try:
        any_mask = bool(has.any())
        _, loaded = decode_depth_frames(raw, [frag_dataset.nears[i] for i in range(N)],
                                        [frag_dataset.fars[i] for i in range(N)], mask=mask if any_mask else None,
                                        has_mask=has if any_mask else None, device=device, out_ptr=buf.ptr)
    except Exception:
        buf.free()
        raise
    return buf, loaded, H, W


def fragment_pairs(frag_dataset, loaded, intrinsic_matrix, config):
    """The fragment's pair list in the reference's order (make_fragments.py:124-227): (source, target,
    uncertain, width * height) -- the odometry pairs (i, i + 1) of loaded frames, then every pair of
    loaded key frames (every odometry_loop_interval-th frame) that passes the frustum filter.  The image
    size of key pair (i, j) is the reference's: widths[i] / heights[i] with i the key frame's position
    in the key list, not its frame index."""
    N = len(frag_dataset.timestamps)
    extrinsics_cw = frag_dataset.transforms.extrinsics_cw
    pairs = [(i, i + 1, False, 0) for i in range(N - 1) if loaded[i] and loaded[i + 1]]
    key_indices = list(range(0, N, int(config.odometry_loop_interval)))
    for i, key_i in enumerate(key_indices):
        width, height = frag_dataset.widths[i], frag_dataset.heights[i]
        if not loaded[key_i]:
            continue
        for key_j in key_indices[i + 1:]:
            if not loaded[key_j]:
                continue
            if not frustum_overlap_filter(extrinsic_cw_1=extrinsics_cw[key_i], extrinsic_cw_2=extrinsics_cw[key_j],
                                          intrinsic_1=intrinsic_matrix, intrinsic_2=intrinsic_matrix,
                                          image_size_1=(width, height), image_size_2=(width, height), z_near=0.1,
                                          z_far=config.depth_max,
                                          overlap_ratio_threshold=config.overlap_ratio_threshold):
                continue
            pairs.append((key_i, key_j, True, int(width) * int(height)))
    return pairs


def build_pose_graph_for_fragment(frag_dataset, depth_data_io, side, config) -> PoseGraph:
    """make_fragments.py:84-248: nodes = the frames' camera->world poses; a certain edge per odometry
    pair, an uncertain one per key-frame pair whose information density info[5, 5] / (width * height)
    exceeds loop_yaw_info_density_threshold.  A frame that fails to load has no edge."""
    from .o3d_utils import compute_o3d_intrinsic_matrices, convert_transforms_to_pose_graph
    from .odometry import odometry_information_pairs
    from .vbg import parse_device
    transforms = frag_dataset.transforms
    pose_graph = convert_transforms_to_pose_graph(transforms=transforms)
    if len(frag_dataset.timestamps) == 0:
        return pose_graph
    intrinsic_matrix = compute_o3d_intrinsic_matrices(dataset=frag_dataset)[0]
    extrinsics_wc, extrinsics_cw = transforms.extrinsics_wc, transforms.extrinsics_cw
    buf, loaded, H, W = load_fragment_frames(depth_data_io, frag_dataset, side, config)
    try:
        pairs = fragment_pairs(frag_dataset, loaded, intrinsic_matrix, config)
        # float32 products, as the reference forms them, widened for the kernel
        rel = [extrinsics_wc[b] @ extrinsics_cw[a] for a, b, _, _ in pairs]
        info, _ = odometry_information_pairs((buf, len(loaded), H, W), intrinsic_matrix.astype(np.float64),
                                             [p[0] for p in pairs], [p[1] for p in pairs],
                                             np.array(rel, np.float64).reshape(-1, 4, 4), config.dist_threshold,
                                             depth_scale=1.0, depth_max=config.depth_max,
                                             device=parse_device(config.device))
    finally:
        buf.free()
    for (a, b, uncertain, area), T, m in zip(pairs, rel, info):
        if uncertain and not m[5, 5] / area > config.loop_yaw_info_density_threshold:
            continue
        pose_graph.edges.append(PoseGraphEdge(source_node_id=a, target_node_id=b, transformation=T, information=m,
                                              uncertain=uncertain, confidence=1.0))
    return pose_graph


def optimize_dataset_pose(depth_data_io, frag_dataset, side, config):
    """make_fragments.py:251-275: the fragment's graph, optimised with node 0 fixed; the node poses become
    the fragment's transforms."""
    from .o3d_utils import convert_pose_graph_to_transforms
    pose_graph = build_pose_graph_for_fragment(frag_dataset=frag_dataset, depth_data_io=depth_data_io, side=side,
                                               config=config)
    option = GlobalOptimizationOption(max_correspondence_distance=config.dist_threshold,
                                      edge_prune_threshold=config.edge_prune_threshold, reference_node=0)
    global_optimization(pose_graph, option, GlobalOptimizationConvergenceCriteria())
    frag_dataset.transforms = convert_pose_graph_to_transforms(pose_graph=pose_graph)


def make_fragment_datasets(depth_data_io, config, sides: Optional[List[Side]] = None) -> Dict[Side, List[DepthDataset]]:
    """make_fragments.py:278-308: every side's dataset in OPEN3D coordinates, split into fragments, each
    fragment's poses optimised.  A fragment whose optimisation raises keeps its poses and the error is
    printed, as the reference's parallel_map does (default_on_error=None).  The fragments run in this
    process one after the other whatever use_multi_threading says: each is one batched launch, and a
    worker process could not hand the poses it assigns back."""
    fragment_dataset_map: Dict[Side, List[DepthDataset]] = {}
    for side in (sides if sides is not None else list(Side)):
        depth_dataset = depth_data_io.load_depth_dataset(side=side, use_cache=config.use_dataset_cache)
        depth_dataset.transforms = depth_dataset.transforms.convert_coordinate_system(
            target_coordinate_system=CoordinateSystem.OPEN3D, is_camera=True)
        frag_datasets = depth_dataset.split(fragment_size=config.fragment_size)
        fragment_dataset_map[side] = frag_datasets
        for frag_dataset in frag_datasets:
            try:
                optimize_dataset_pose(depth_data_io, frag_dataset, side, config)
            except Exception as e:  # noqa: BLE001 -- the reference catches everything per fragment
                print(f"[Error] optimize_dataset_pose failed: {e}")
    return fragment_dataset_map
