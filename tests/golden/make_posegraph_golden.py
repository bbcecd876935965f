"""Generate tests/golden/posegraph_golden.npz by running the REFERENCE's own Python code.

Run where the reference checkout is available:
    python tests/golden/make_posegraph_golden.py <the reference's scripts directory>
It imports the reference's scripts (read-only) with ``open3d`` and ``cv2`` stubbed by MagicMock, as
make_golden.py does (neither is installed; the functions exercised never touch them), feeds them seeded
inputs and stores inputs + reference outputs as .npz data.  Nothing from the reference is copied.

Fixtures (posegraph_golden.npz, a few kilobytes):
  frustum_*   frustum_overlap_filter (make_fragments.py:14-81) for seeded camera pairs: the poses, the
              intrinsic matrix, image size, z range and threshold, the decisions, and the overlap ratios
              (found by bisection on the reference's own decision, so that cases within 1e-6 of the
              threshold can be left out)
  world_*     Transforms.apply_world_transform (transforms.py:242-258): inputs and outputs
  merge_*     DepthDataset.merge (camera_dataset.py:167-192) of three seeded datasets: every field
"""
from __future__ import annotations

import sys
from pathlib import Path
from unittest.mock import MagicMock

import numpy as np

HERE = Path(__file__).resolve().parent


def import_reference(ref_scripts):
    for m in ("open3d", "open3d.core", "cv2"):
        sys.modules[m] = MagicMock()
    sys.path.insert(0, str(Path(ref_scripts).resolve()))
    from models.camera_dataset import DepthDataset
    from models.transforms import CoordinateSystem, Transforms
    from processing.reconstruction.depth_optimization.make_fragments import frustum_overlap_filter
    return DepthDataset, CoordinateSystem, Transforms, frustum_overlap_filter


def random_pose(rng, spread):
    from scipy.spatial.transform import Rotation
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = Rotation.from_rotvec(rng.normal(0.0, 0.6, 3)).as_matrix()
    T[:3, 3] = rng.normal(0.0, spread, 3)
    return T


def ratio_of(filter_fn, args, lo=0.0, hi=1.0):
    """The overlap ratio behind the reference's decision, by bisection on its threshold argument (the
    decision is ratio > threshold, and ratio <= 1)."""
    if not filter_fn(*args, overlap_ratio_threshold=0.0):
        return 0.0
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        if filter_fn(*args, overlap_ratio_threshold=mid):
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    DepthDataset, CoordinateSystem, Transforms, frustum_overlap_filter = import_reference(sys.argv[1])
    rng = np.random.default_rng(20)
    out = {}

    # ---- frustum filter
    K = np.array([[70.0, 0, 39.5], [0, 70.0, 29.5], [0, 0, 1]], np.float32)
    size = (80, 60)
    thr, z_near, z_far = 0.1, 0.1, 3.0
    A, B, dec, ratios = [], [], [], []
    while len(dec) < 48:
        a, b = random_pose(rng, 0.3), random_pose(rng, [0.3, 1.0, 2.5][len(dec) % 3])
        args = (a, b, K, K, size, size, z_near, z_far)
        r = ratio_of(frustum_overlap_filter, args)
        if abs(r - thr) < 1e-6:
            continue
        A.append(a)
        B.append(b)
        dec.append(bool(frustum_overlap_filter(*args, overlap_ratio_threshold=thr)))
        ratios.append(r)
    assert any(dec) and not all(dec)
    out.update(frustum_cw_1=np.stack(A), frustum_cw_2=np.stack(B), frustum_K=K, frustum_size=np.array(size),
               frustum_z=np.array([z_near, z_far]), frustum_threshold=np.array(thr),
               frustum_decision=np.array(dec), frustum_ratio=np.array(ratios))

    # ---- apply_world_transform
    from scipy.spatial.transform import Rotation
    pos = rng.normal(0.0, 1.0, (9, 3))
    rot = Rotation.from_rotvec(rng.normal(0.0, 1.0, (9, 3))).as_quat()
    dpos = rng.normal(0.0, 0.5, (4, 3))
    drot = Rotation.from_rotvec(rng.normal(0.0, 0.8, (4, 3))).as_quat()
    t = Transforms(coordinate_system=CoordinateSystem.OPEN3D, positions=pos, rotations=rot)
    moved = [t.apply_world_transform(delta_position=dpos[i], delta_rotation=drot[i]) for i in range(4)]
    out.update(world_positions=pos, world_rotations=rot, world_delta_positions=dpos, world_delta_rotations=drot,
               world_out_positions=np.stack([m.positions for m in moved]),
               world_out_rotations=np.stack([m.rotations for m in moved]))

    # ---- DepthDataset.merge
    def dataset(n, t0):
        return DepthDataset(
            directory_relative_path="left_depth", image_file_names=np.array([f"{t0 + i}.raw" for i in range(n)]),
            timestamps=np.arange(t0, t0 + n), fx=rng.random(n), fy=rng.random(n), cx=rng.random(n), cy=rng.random(n),
            transforms=Transforms(coordinate_system=CoordinateSystem.OPEN3D, positions=rng.normal(size=(n, 3)),
                                  rotations=Rotation.from_rotvec(rng.normal(size=(n, 3))).as_quat()),
            widths=np.full(n, 80), heights=np.full(n, 60), nears=np.full(n, 0.1), fars=np.full(n, np.inf))
    parts = [dataset(4, 1000), dataset(3, 2000), dataset(5, 3000)]
    merged = DepthDataset.merge(parts)
    out["merge_lengths"] = np.array([len(p.timestamps) for p in parts])
    for k, v in merged.to_dict().items():
        out[f"merge_out_{k}"] = np.asarray(v)
    for k in parts[0].to_dict():
        vals = [np.asarray(p.to_dict()[k]) for p in parts]
        out[f"merge_in_{k}"] = np.concatenate(vals) if vals[0].ndim else vals[0]
    np.savez_compressed(HERE / "posegraph_golden.npz", **out)
    print("wrote", HERE / "posegraph_golden.npz", (HERE / "posegraph_golden.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
