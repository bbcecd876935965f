"""downsample_mesh on the GPU: the mesh reduction of the reference's ``scripts/downsample_fbx_mesh.py``.

``downsample_mesh(mesh, target_vertex_percent)`` mirrors the reference function (lines 129-283): the same
scalar rules (the percentage check, ``target = max(4, int(n * (percent / 100.0)))``, the input object returned
as it is when ``target >= n``, the bounding-box diagonal, ``v_ref = diagonal / target ** (1/3) * 1.2``), the
same messages, and the same point-cloud branch for a mesh without triangles.  What it reduces with is
``TriangleMesh.simplify_vertex_clustering`` (csrc/meshsimplify.hip), on a mesh held in HBM without
leaving it.

The reference tries ``simplify_quadric_decimation`` first and falls back to vertex clustering at ``v_ref``.
Quadric decimation is a serial priority queue with Open3D-internal tie breaking and is NOT implemented here
(DESIGN §7).  Two rules stand in for it:

* ``voxel_size_rule="reference"`` clusters at ``v_ref``: the reference's fallback branch as written.
* ``voxel_size_rule="fit"`` (the default) keeps what the quadric branch is for -- a result of about ``target``
  vertices.  ``v_ref`` does not give that: it assumes the vertices fill the box, while the occupied cells of a
  surface grow like ``target ** (2/3)``.  The fit is a deterministic search over ``C(v)``, the vertex count
  clustering at ``v`` gives (``mqr_mesh_cluster_count``), in Python float64:

  1. ``v_hi = v_ref``; while ``C(v_hi) > target`` double it (at most 32 times);
  2. ``v_lo = v_hi / 2``; while ``C(v_lo) < target`` and the grid limit (2^21 cells along an axis) is not hit,
     halve it (at most 32 times);
  3. 16 steps at ``v_mid = sqrt(v_lo * v_hi)``: ``C(v_mid) > target`` (or a grid past the limit) makes it the
     new ``v_lo``, anything else the new ``v_hi``;
  4. of every size whose count was evaluated, the one with the smallest ``|C - target|``; ties go to the
     larger size.

  A host mesh is uploaded once for the whole search.

Deviations from the reference, besides the above: ``compute_vertex_normals`` is not implemented, so
an input without normals gives zero normals (as ``filter_mesh_components`` does); the point-cloud branch's
``voxel_down_sample`` returns positions only, so colours are dropped there; FBX / Aspose file handling is out --
the command line reads and writes PLY:

    python -m mqr.downsample_mesh in.ply out.ply --vertex-percent 10 [--voxel-size-rule fit|reference]

with the reference script's ``--vertex-percent`` (default 50.0) and exit status 1 on any error.
"""
from __future__ import annotations

import argparse
import math
import sys
from pathlib import Path

import numpy as np

from .geometry import (GridTooFine, PointCloud, ResidentMesh, Tensor, TriangleMesh, _simplified_mesh, host_rows,
                       mesh_fields)

RULES = ("fit", "reference")


def target_vertex_count(n: int, target_vertex_percent: float) -> int:
    """The reference's target (lines 143-150); ValueError unless 0 < percent <= 100."""
    if target_vertex_percent <= 0 or target_vertex_percent > 100:
        raise ValueError(f"Target vertex percentage must be between 0 and 100, got: {target_vertex_percent}")
    return max(4, int(n * (target_vertex_percent / 100.0)))


def reference_voxel_size(diagonal: float, target: int) -> float:
    """``diagonal / target ** (1/3) * 1.2`` (lines 238, 262)."""
    return diagonal / (target ** (1 / 3)) * 1.2


def fit_voxel_size(count, v_ref: float, target: int):
    """The search of the module docstring over ``count(v)`` (which raises GridTooFine past the grid limit):
    (size, its count, [(size, count) of every evaluation, in order])."""
    seen = []

    def C(v):
        c = count(v)
        seen.append((v, c))
        return c

    v_hi = v_ref
    c = C(v_hi)
    for _ in range(32):
        if c <= target:
            break
        v_hi *= 2.0
        c = C(v_hi)
    v_lo = v_hi / 2.0
    for _ in range(32):
        try:
            if C(v_lo) >= target:
                break
        except GridTooFine:
            break
        v_lo /= 2.0
    for _ in range(16):
        v_mid = math.sqrt(v_lo * v_hi)
        try:
            above = C(v_mid) > target
        except GridTooFine:
            above = True
        if above:
            v_lo = v_mid
        else:
            v_hi = v_mid
    v, c = min(seen, key=lambda vc: (abs(vc[1] - target), -vc[0]))
    return v, c, seen


def _rows_of(x) -> int:
    """Rows of an (..., 3) field without bringing a device tensor to the host."""
    shape = x.shape if hasattr(x, "shape") else np.shape(x)
    return int(np.prod(shape[:-1], dtype=np.int64)) if len(shape) > 1 else int(shape[0]) // 3


def _point_cloud_branch(f, n, target, v_ref, device):
    """Lines 162-211: every k-th point, then a voxel down-sample at v_ref when that left more than 1.5 target
    (v_ref None: the bounding box is degenerate, every k-th point only)."""
    print("[Info] Mesh has no triangles (point cloud), using uniform downsampling")
    pos = host_rows(f.positions, np.float32)
    nrm = host_rows(f.normals, np.float32) if f.normals is not None else np.zeros_like(pos)
    col = None if f.colors is None else host_rows(f.colors, np.float32)
    pcd = PointCloud(pos, nrm if nrm.shape == pos.shape else np.zeros_like(pos), device=device,
                     colors=col if col is not None and col.shape == pos.shape else None)
    every_k = max(1, n // target)
    if v_ref is None:
        print("[Warning] Bounding box is invalid, using simple uniform downsampling")
        down = pcd.uniform_down_sample(every_k)
    else:
        print(f"[Info] Using voxel size: {v_ref:.6f} for uniform downsampling")
        down = pcd.uniform_down_sample(every_k)
        if len(down.points) > target * 1.5:
            print(f"[Info] Uniform downsampling resulted in {len(down.points)} points, using voxel downsampling")
            down = pcd.voxel_down_sample(v_ref)  # positions only: colours are dropped (module docstring)
    out = TriangleMesh(down.points, down.normals, np.zeros((0, 3), np.int32), device=device)
    if down.has_colors():
        out.vertex["colors"] = Tensor(down.colors)
    return out


def downsample_mesh(mesh, target_vertex_percent: float, voxel_size_rule: str = "fit"):
    """Drop-in for the reference's ``downsample_mesh`` (module docstring).  ``mesh``: anything
    ``mqr.geometry.mesh_fields`` unpacks; the result is a :class:`mqr.geometry.TriangleMesh` (in HBM when the
    input is), or the input object itself when the target is not below its vertex count."""
    if voxel_size_rule not in RULES:
        raise ValueError(f"voxel_size_rule must be one of {RULES}, got {voxel_size_rule!r}")
    f = mesh_fields(mesh)
    n = _rows_of(f.positions)
    target = target_vertex_count(n, target_vertex_percent)
    if target >= n:
        print(f"[Info] Target vertex count ({target}) >= original ({n}), returning original mesh")
        return mesh
    print(f"[Info] Downsampling mesh from {n} to {target} vertices ({target_vertex_percent:.1f}%)")
    r = ResidentMesh(mesh)
    try:
        lo, hi = r.bounds()
        diagonal = float(np.linalg.norm(hi - lo))
        if r.nt == 0:
            return _point_cloud_branch(f, n, target, reference_voxel_size(diagonal, target) if diagonal > 0 else None,
                                       f.device)
        if diagonal <= 0:
            raise ValueError("Mesh bounding box has zero size, cannot downsample")
        v_ref = reference_voxel_size(diagonal, target)
        if v_ref <= 0:
            raise ValueError(f"Calculated voxel size is invalid: {v_ref}")
        if voxel_size_rule == "reference":
            v = v_ref
        else:
            v = fit_voxel_size(r.cluster_count, v_ref, target)[0]
        print(f"[Info] Using voxel size: {v:.6f} for vertex clustering")
        out, stats = _simplified_mesh(r, v, f.device)
    finally:
        r.free()
    nv, nt = int(stats[1]), int(stats[5])
    print(f"[Info] Vertex clustering resulted in {nv} vertices")
    if f.colors is not None:
        print(f"[Info] Vertex colors preserved: {nv if out.has_vertex_colors() else 0} colors")
    print(f"[Info] Downsampling complete: {nv} vertices, {nt} faces")
    print(f"[Info] Reduction: {n - nv} vertices removed ({100 * (1 - nv / n):.1f}%)")
    return out


def parse_args(argv=None):
    parser = argparse.ArgumentParser(
        description="Downsample a PLY mesh file by reducing vertices to a specified percentage. "
                    "Preserves vertex colors and mesh topology.")
    parser.add_argument("input_ply", type=str, help="Path to the input PLY file")
    parser.add_argument("output_ply", type=str, help="Path to the output PLY file")
    parser.add_argument("--vertex-percent", type=float, default=50.0,
                        help="Percentage of vertices to keep (0-100). Default: 50.0 (keep 50%% of vertices)")
    parser.add_argument("--voxel-size-rule", choices=RULES, default="fit",
                        help="fit: search the voxel size that reaches the target count (default); "
                             "reference: the reference's diagonal / target^(1/3) * 1.2")
    return parser.parse_args(argv)


def main(argv=None) -> int:
    from .geometry import read_triangle_mesh, write_triangle_mesh
    args = parse_args(argv)
    try:
        input_path, output_path = Path(args.input_ply).resolve(), Path(args.output_ply).resolve()
        if args.vertex_percent <= 0 or args.vertex_percent > 100:
            print(f"[Error] Vertex percentage must be between 0 and 100, got: {args.vertex_percent}", file=sys.stderr)
            return 1
        if not input_path.exists():
            raise FileNotFoundError(f"PLY file not found: {input_path}")
        mesh = read_triangle_mesh(str(input_path))
        if len(mesh.vertices) == 0:
            raise ValueError("Loaded mesh has no vertices")
        print(f"[Info] Successfully loaded mesh: {len(mesh.vertices)} vertices, {len(mesh.triangles)} faces")
        out = downsample_mesh(mesh, args.vertex_percent, args.voxel_size_rule)
        output_path.parent.mkdir(parents=True, exist_ok=True)
        write_triangle_mesh(str(output_path), out)
        print("[Info] Downsampling complete!")
        print(f"[Info] Input:  {input_path} ({len(mesh.vertices)} vertices)")
        print(f"[Info] Output: {output_path} ({len(out.vertices)} vertices)")
    except (FileNotFoundError, ValueError) as e:
        print(f"[Error] {e}", file=sys.stderr)
        return 1
    except Exception as e:  # as the reference: anything else is reported with its traceback, status 1
        print(f"[Error] Unexpected error: {e}", file=sys.stderr)
        import traceback
        traceback.print_exc()
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
