"""Drop-in for the reference's fragment integration (the second caller of ``integrate``):

    integrate_fragment_point_cloud(depth_data_io, frag_dataset, side, config)
        scripts/processing/reconstruction/depth_optimization/refine_fragment_poses.py:14-58
    integrate_fragment_point_clouds(depth_data_io, fragment_dataset_map, config, workers)
        the parallel part of integrate_and_save_fragment_point_clouds (:61-119), without the saving
    compute_pcd_pair_edge(clouds, source_node, target_node, config, uncertain)            :122-193
    build_pose_graph_for_scene(fragment_clouds_by_side, config)                           :196-271
        the pose-graph edges of every fragment pair, registered on the GPU (mqr.registration)
    refine_fragment_poses(depth_data_io, fragment_dataset_map, config, workers)           :274-321
        integrate, register, optimise the scene graph (mqr.posegraph), move the fragments

Each fragment (``fragment_size`` = 100 frames, pipeline_config.yml:38) is integrated into a FRESH
volume (``vbg_opt=None``) and its point cloud extracted with the default weight threshold 3.0; a
failure or an empty cloud gives ``None`` with the reference's messages.  With
``use_multi_threading`` the reference runs the fragments on a spawn Pool of cpu_count - 1 workers
(utils/paralell_utils.py:55-67): here every worker process opens its own HIP context on the same
GPU (one HIP runtime per process, mqr._lib), so several fragments integrate concurrently on one
MI355X.  Worker results cross the process boundary as (side, positions, normals) arrays.
"""
from __future__ import annotations

import itertools
import multiprocessing
import os
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

from .models import Side
from .posegraph import PoseGraph, PoseGraphEdge, PoseGraphNode  # noqa: F401  (re-exported)


@dataclass
class FragmentPoseRefinementConfig:
    """reconstruction_config.py:60-84 (defaults; the pipeline's values are in
    config/pipeline_config.yml:50-58): the integration fields, then the registration fields."""
    device: object = "CUDA:0"
    use_confidence_filtered_depth: bool = True
    confidence_threshold: float = 0.05
    valid_count_threshold: int = 4
    voxel_size: float = 0.01
    block_resolution: int = 16
    block_count: int = 50_000
    depth_max: float = 1.5
    trunc_voxel_multiplier: float = 8.0
    use_multi_threading: bool = False
    use_pre_filtering: bool = True
    pre_filter_every_k_points: float = 30
    pre_filter_max_corr_dist: float = 0.1
    pre_filter_inlier_rmse_threshold: float = 0.05
    pre_filter_fitness_threshold: float = 0.2
    icp_voxel_sizes: List[float] = field(default_factory=lambda: [0.05, 0.025, 0.0125])
    max_corr_dists: List[float] = field(default_factory=lambda: [0.1, 0.05, 0.025])
    max_iterations: List[int] = field(default_factory=lambda: [50, 31, 14])
    relative_fitnesses: List[float] = field(default_factory=lambda: [1e-6, 1e-6, 1e-6])
    relative_rmses: List[float] = field(default_factory=lambda: [1e-6, 1e-6, 1e-6])
    icp_fitness_threshold: float = 0.2
    icp_inlier_rmse_threshold: float = 0.05
    dist_threshold: float = 0.07
    edge_prune_threshold: float = 0.25

    @property
    def icp_criteria_list(self):
        from .registration import ICPConvergenceCriteria
        return [ICPConvergenceCriteria(relative_fitness=f, relative_rmse=r, max_iteration=i)
                for f, r, i in zip(self.relative_fitnesses, self.relative_rmses, self.max_iterations)]


def integrate_fragment_point_cloud(depth_data_io, frag_dataset, side: Side, config: FragmentPoseRefinementConfig):
    """refine_fragment_poses.py:14-58: fresh volume, integrate, extract_point_cloud(); None on an
    empty cloud or an error (printed as the reference prints it)."""
    from .o3d_utils import integrate
    try:
        vbg = integrate(dataset=frag_dataset, depth_data_io=depth_data_io, side=side,
                        use_confidence_filtered_depth=config.use_confidence_filtered_depth,
                        confidence_threshold=config.confidence_threshold,
                        valid_count_threshold=config.valid_count_threshold, voxel_size=config.voxel_size,
                        block_resolution=config.block_resolution, block_count=config.block_count,
                        depth_max=config.depth_max, trunc_voxel_multiplier=config.trunc_voxel_multiplier,
                        device=config.device, show_progress=False, desc=None, vbg_opt=None)
        pcd = vbg.extract_point_cloud()
        del vbg
        if pcd.point.positions.shape[0] == 0:
            print(f"[Warning] Fragment point cloud for {side.name} is empty (no valid points). "
                  f"Dataset has {len(frag_dataset.timestamps)} frames. "
                  f"This may indicate insufficient depth data or overly strict filtering.")
            return None
        return side, pcd
    except Exception as e:  # noqa: BLE001 -- the reference catches everything per fragment
        ts = frag_dataset.timestamps
        print(f"[Error] integrate_fragment_point_cloud failed for {side.name}: {e}")
        print(f"[Error] Fragment dataset info: {len(ts)} frames, "
              f"timestamps range: {ts.min() if len(ts) > 0 else 'N/A'} - {ts.max() if len(ts) > 0 else 'N/A'}")
        return None


def _worker(args):
    """Pool task: (index, depth_data_io, frag_dataset, side, config) -> (index, result arrays, seconds)."""
    import time
    i, io, ds, side, config = args
    t0 = time.perf_counter()
    # the reference's ParallelWorker (paralell_utils.py:11-19) turns ANY failure of a task into None
    # for that task: library load / HIP context creation in a spawned worker or reading the cloud
    # back must not abort the other fragments
    try:
        r = integrate_fragment_point_cloud(io, ds, side, config)
        if r is None:
            return i, None, time.perf_counter() - t0
        side, pcd = r
        return i, (side, pcd.points, pcd.normals), time.perf_counter() - t0
    except Exception as e:  # noqa: BLE001
        print(f"[Error] integrate_fragment_point_cloud failed for {getattr(side, 'name', side)}: {e}")
        return i, None, time.perf_counter() - t0


def _warm(_):
    """Pool warm-up task: load the library and open the HIP context in the worker."""
    from . import _lib
    _lib.load()
    return os.getpid()


def integrate_fragment_point_clouds(depth_data_io, fragment_dataset_map, config: FragmentPoseRefinementConfig,
                                    workers: Optional[int] = None, pool=None, keep_on_device: bool = False):
    """Every fragment of every side through integrate_fragment_point_cloud, in the reference's
    argument order (sides, then fragments).  With config.use_multi_threading: a spawn Pool of
    `workers` processes (default cpu_count - 1, at most 15: one GPU holds a bounded number of
    contexts), or the caller's `pool`.  Returns [(side, positions, normals) | None] in argument order.
    With keep_on_device (in-process only) the entries are (side, PointCloud) with the cloud left in
    HBM, ready for build_pose_graph_for_scene without a trip over PCIe."""
    args = [(i, depth_data_io, ds, side, config)
            for i, (side, ds) in enumerate((s, d) for s, dss in fragment_dataset_map.items() for d in dss)]
    if keep_on_device:
        if config.use_multi_threading or pool is not None:
            raise ValueError("keep_on_device needs the in-process path: device memory does not cross processes")
        return [integrate_fragment_point_cloud(io, ds, side, cfg) for _, io, ds, side, cfg in args]
    if not config.use_multi_threading:
        out = [_worker(a) for a in args]
    elif pool is not None:
        out = pool.map(_worker, args)
    else:
        n = workers or max(1, min(multiprocessing.cpu_count() - 1, 15, len(args)))
        os.environ["OMP_NUM_THREADS"] = "1"
        with multiprocessing.get_context("spawn").Pool(processes=n) as p:
            out = p.map(_worker, args)
    res = [None] * len(args)
    for i, r, _ in out:
        res[i] = r
    return res


def fragment_datasets(dataset, fragment_size: int = 100):
    """Consecutive fragment_size-frame slices of a dataset (make_fragments.py's fragment layout; the
    fragments' own pose graphs are mqr.make_fragments)."""
    n = len(dataset)
    return [dataset[list(range(a, min(n, a + fragment_size)))] for a in range(0, n, fragment_size)]


# ---- pose graph of the fragments (refine_fragment_poses.py:122-271) --------------------------------
# The containers (Open3D's attribute names) live in mqr.posegraph with the optimiser; they are imported
# above so that ``from mqr.fragments import PoseGraph`` keeps working.
def _pre_filter_rejects(result, config) -> bool:
    return (result.fitness < config.pre_filter_fitness_threshold
            or result.inlier_rmse > config.pre_filter_inlier_rmse_threshold)


def _icp_converged(result, config) -> bool:
    # the reference's stand-in for Open3D's always-false `converged` flag (refine_fragment_poses.py:163-172)
    return result.fitness >= config.icp_fitness_threshold or result.inlier_rmse <= config.icp_inlier_rmse_threshold


def compute_pcd_pair_edge(clouds, source_node: int, target_node: int, config: FragmentPoseRefinementConfig,
                          uncertain: bool) -> Optional[PoseGraphEdge]:
    """refine_fragment_poses.py:122-193 for one pair, through the single-pair registration functions.
    `clouds`: the fragment clouds by node index (PointClouds, device or host arrays)."""
    from . import registration as reg
    source, target = clouds[source_node], clouds[target_node]
    if config.use_pre_filtering and uncertain:
        cs = reg.CloudSet([source, target])
        try:
            pre = cs.evaluate_pairs([0], [1], config.pre_filter_max_corr_dist, np.eye(4),
                                    every_k=int(config.pre_filter_every_k_points))[0]
        finally:
            cs.close()
        if _pre_filter_rejects(pre, config):
            return None
    icp = reg.multi_scale_icp(source, target, config.icp_voxel_sizes, config.icp_criteria_list,
                              config.max_corr_dists, np.eye(4))
    if uncertain and not _icp_converged(icp, config):
        return None
    info = reg.get_information_matrix(source, target, config.max_corr_dists[-1], icp.transformation)
    return PoseGraphEdge(source_node, target_node, icp.transformation, info, uncertain, 1.0)


def pose_graph_pairs(fragment_counts):
    """(source node, target node, uncertain) in the reference's order (:226-254): the odometry pairs
    side by side, then every combination of two nodes as a loop closure."""
    pairs, base = [], 0
    for count in fragment_counts:
        pairs += [(base + i, base + i + 1, False) for i in range(count - 1)]
        base += count
    pairs += [(a, b, True) for a, b in itertools.combinations(range(base), 2)]
    return pairs


def build_pose_graph_for_scene(fragment_clouds_by_side, config: FragmentPoseRefinementConfig, batched: bool = True,
                               stats: Optional[dict] = None):
    """refine_fragment_poses.py:196-271 over fragment clouds in memory: {side: [cloud, ...]} ->
    (PoseGraph, [(side, index), ...]).  The same nodes (sides, then index) and pairs (odometry, then
    itertools.combinations) as the reference; batched, the pairs run as three calls on one CloudSet --
    pre-filter every uncertain pair, ICP the survivors and the odometry pairs, information for the
    edges kept.  ``batched=False`` runs compute_pcd_pair_edge pair by pair instead.  `stats` (a dict)
    receives the pair counts of each stage."""
    from . import registration as reg
    node_side_index_list = [(side, i) for side, cs in fragment_clouds_by_side.items() for i in range(len(cs))]
    clouds = [c for cs in fragment_clouds_by_side.values() for c in cs]
    graph = PoseGraph(nodes=[PoseGraphNode() for _ in clouds])
    pairs = pose_graph_pairs([len(cs) for cs in fragment_clouds_by_side.values()])
    edges: List[Optional[PoseGraphEdge]] = [None] * len(pairs)
    if not batched:
        edges = [compute_pcd_pair_edge(clouds, a, b, config, unc) for a, b, unc in pairs]
    elif pairs:
        cs = reg.CloudSet(clouds)
        try:
            alive = list(range(len(pairs)))
            if config.use_pre_filtering:
                unc = [i for i in alive if pairs[i][2]]
                pre = cs.evaluate_pairs([pairs[i][0] for i in unc], [pairs[i][1] for i in unc],
                                        config.pre_filter_max_corr_dist, np.eye(4),
                                        every_k=int(config.pre_filter_every_k_points))
                dropped = {i for i, r in zip(unc, pre) if _pre_filter_rejects(r, config)}
                alive = [i for i in alive if i not in dropped]
            icp = cs.icp_pairs([pairs[i][0] for i in alive], [pairs[i][1] for i in alive], config.icp_voxel_sizes,
                               config.icp_criteria_list, config.max_corr_dists, np.eye(4))
            kept = [(i, r) for i, r in zip(alive, icp) if not pairs[i][2] or _icp_converged(r, config)]
            info = cs.information_pairs([pairs[i][0] for i, _ in kept], [pairs[i][1] for i, _ in kept],
                                        config.max_corr_dists[-1],
                                        np.stack([r.transformation for _, r in kept]) if kept else None)
            for (i, r), m in zip(kept, info):
                a, b, u = pairs[i]
                edges[i] = PoseGraphEdge(a, b, r.transformation, m, u, 1.0)
            if stats is not None:
                stats.update(pairs=len(pairs), icp_pairs=len(alive), information_pairs=len(kept))
        finally:
            cs.close()
    valid_edges = [e for e in edges if e is not None]
    print(f"[Info] Valid edges: {len(valid_edges)} / {len(edges)}")
    graph.edges.extend(valid_edges)
    return graph, node_side_index_list


def refine_fragment_poses(depth_data_io, fragment_dataset_map, config: FragmentPoseRefinementConfig,
                          workers: Optional[int] = None):
    """refine_fragment_poses.py:274-321 in memory: integrate every fragment, register every pair of the
    fragments that gave a cloud (build_pose_graph_for_scene), optimise the scene graph with node 0 fixed
    and move each fragment by its node's pose.  Changes the fragments' transforms in place and returns
    (pose_graph, node_side_index_list).

    Fragments that fail to integrate are dropped the way the reference's fragment_counts drops them: the
    clouds of a side are numbered in order, so node (side, k) stands for the side's k-th SAVED cloud and
    moves ``fragment_dataset_map[side][k]`` (after a failure these differ, as in the reference).  Without
    use_multi_threading the clouds stay in HBM between integration and registration."""
    from .geometry import PointCloud
    from .o3d_utils import convert_pose_graph_to_transforms
    from .posegraph import GlobalOptimizationConvergenceCriteria, GlobalOptimizationOption, global_optimization
    in_process = not config.use_multi_threading
    results = integrate_fragment_point_clouds(depth_data_io, fragment_dataset_map, config, workers=workers,
                                              keep_on_device=in_process)
    valid = [r for r in results if r is not None]
    failed = len(results) - len(valid)
    if failed > 0:
        print(f"[Warning] {failed} out of {len(results)} fragment point clouds failed to integrate or were empty.")
    if not valid:
        raise Exception("Failed to integrate fragment point clouds: all fragments produced empty or invalid point clouds.")
    clouds_by_side = {}
    for r in valid:
        cloud = r[1] if in_process else PointCloud(r[1], r[2])
        clouds_by_side.setdefault(r[0], []).append(cloud)
    print(f"[Info] Successfully integrated {len(valid)} fragment point clouds.")
    pose_graph, node_side_index_list = build_pose_graph_for_scene(clouds_by_side, config)
    del clouds_by_side, valid, results
    option = GlobalOptimizationOption(max_correspondence_distance=config.dist_threshold,
                                      edge_prune_threshold=config.edge_prune_threshold, reference_node=0)
    global_optimization(pose_graph, option, GlobalOptimizationConvergenceCriteria())
    moves = convert_pose_graph_to_transforms(pose_graph)
    for (side, k), shift, turn in zip(node_side_index_list, moves.positions, moves.rotations):
        frag = fragment_dataset_map[side][k]
        frag.transforms = frag.transforms.apply_world_transform(delta_position=shift, delta_rotation=turn)
    return pose_graph, node_side_index_list
