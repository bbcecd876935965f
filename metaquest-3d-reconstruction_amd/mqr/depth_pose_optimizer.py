"""Drop-in for the reference's DepthPoseOptimizer
(scripts/processing/reconstruction/depth_optimization/depth_pose_optimizer.py:14-100), in memory:

    optimize_depth_poses(depth_data_io, config) -> {side: DepthDataset}
        make_fragment_datasets -> refine_fragment_poses -> DepthDataset.merge per side

The poses it returns are the ones every later ``integrate`` call of the pipeline uses.  The reference's
on-disk caches (fragment datasets, fragment point clouds, the optimised datasets; its
``use_fragment_dataset_cache`` / ``use_optimized_dataset_cache`` switches) are out of scope: nothing is
written, and a caller that wants them saves the returned datasets with ``DepthDataset.save``.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional

from .fragments import FragmentPoseRefinementConfig, refine_fragment_poses
from .make_fragments import FragmentGenerationConfig, make_fragment_datasets
from .models import DepthDataset, Side


@dataclass
class DepthPoseOptimizationConfig:
    """The two parts of the reference's ReconstructionConfig that DepthPoseOptimizer reads."""
    fragment_generation: FragmentGenerationConfig = field(default_factory=FragmentGenerationConfig)
    fragment_pose_refinement: FragmentPoseRefinementConfig = field(default_factory=FragmentPoseRefinementConfig)


def merge_fragment_datasets(frag_dataset_map: Dict[Side, List[DepthDataset]]) -> Dict[Side, DepthDataset]:
    """depth_pose_optimizer.py:14-20."""
    return {side: DepthDataset.merge(frags) for side, frags in frag_dataset_map.items()}


def optimize_depth_poses(depth_data_io, config, sides: Optional[List[Side]] = None,
                         workers: Optional[int] = None) -> Dict[Side, DepthDataset]:
    """Make fragments, refine their poses, merge: one optimised DepthDataset (OPEN3D coordinates) per
    side.  `config`: anything with ``fragment_generation`` and ``fragment_pose_refinement`` (the
    reference's ReconstructionConfig, or DepthPoseOptimizationConfig)."""
    frag_dataset_map = make_fragment_datasets(depth_data_io=depth_data_io, config=config.fragment_generation,
                                              sides=sides)
    refine_fragment_poses(depth_data_io=depth_data_io, fragment_dataset_map=frag_dataset_map,
                          config=config.fragment_pose_refinement, workers=workers)
    return merge_fragment_datasets(frag_dataset_map)
