"""Golden ground-truth comparison reports from the reference's own function.  Tests never run this.

Run where the reference checkout is available:
    python tests/golden/make_compare_golden.py <the reference's analysis directory>
It imports the reference's analysis/computation/compare_mesh_to_ground_truth.py (read-only) with ``open3d``,
``matplotlib`` and ``mesh_loader`` stubbed, points its ``load_mesh`` at the stand-in meshes below and its
``mesh_to_point_cloud`` at this project's sampler (seeds seed .. seed + 3 in the order the reference asks for
samples: scan, ground truth, overlap scan, overlap ground truth), calls its ``compare_meshes`` and stores the
meshes, the arguments and every returned metric in tests/golden/compare_golden.npz.  Nothing from the
reference is copied.

The stand-in geometry restates the Open3D calls the reference makes (the unpinned part):
  compute_point_cloud_distance   brute force, d2 = (dx dx + dy dy) + dz dz in float64, sqrt
  KDTreeFlann.search_knn_vector_3d   the k nearest by (d2, index)
  KDTreeFlann.search_radius_vector_3d   the points with d2 < r^2, strict
  get_volume   |sum p0 . (p1 x p2) / 6| when every edge lies on two triangles that traverse it in opposite
               directions, else an exception (the reference then uses 0.0)
  get_surface_area, get_axis_aligned_bounding_box (get_extent, get_center = (min + max) / 2), get_center (the
  mean point), translate, scale

Cases (ground truth: the octahedron subdivided 3 times, 258 / 512; all coordinates float32):
  identical       the octahedron against itself
  noisy_explicit  a noisy open 14 x 14 grid, threshold 0.05
  noisy_auto      the same, threshold None (1 % of the ground truth's diagonal)
  holes           the grid without a 3 x 3 block of cells and with one triangle replaced by a ring around a
                  pinhole (a hole above and one below the 1 % bar; the grid's rim is a third loop)
  touching        the grid without cells (4, 4) and (5, 5): two holes that meet in a vertex of degree 4
  degenerate      the grid plus a fin on an interior edge (multiplicity 3) and a triangle (a, a, b)
  cloud           700 points near the sphere, no triangles (500 samples: the vertex branch chooses)
  center          the noisy grid shifted by (0.3, -0.2, 0.1), align_method "center"
  scale           the same with scale_normalize

The generator fails if a sample's distance lies within relative 2^-30 of the threshold it is compared with
(F-score, overlap) -- for the moved samples of ``center`` and ``scale`` additionally within the float32
rounding bound sqrt(3) 2^-24 max|coordinate| -- or a hole perimeter within relative 2^-30 of its bar: every
count is then decided the same way by any implementation of the rules.
"""
import importlib.util
import os
import sys
import types
from pathlib import Path
from unittest import mock

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "metaquest-3d-reconstruction_amd"))
import compare_ref as cr  # noqa: E402

SAMPLES = 1000
MARGIN = 2.0 ** -30


def _d2(q, t):
    d = np.asarray(q, np.float64)[None, :] - np.asarray(t, np.float64)
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


class _Box:
    def __init__(self, p):
        self.lo, self.hi = p.min(0), p.max(0)

    def get_extent(self):
        return self.hi - self.lo

    def get_center(self):
        return (self.lo + self.hi) * 0.5


class StandInCloud:
    def __init__(self, other=None):
        self.points = np.zeros((0, 3)) if other is None else np.array(other.points, np.float64)

    def compute_point_cloud_distance(self, target):
        t = np.asarray(target.points, np.float64)
        return np.array([np.sqrt(_d2(p, t).min()) for p in np.asarray(self.points, np.float64)])

    def get_center(self):
        return np.asarray(self.points, np.float64).mean(0)

    def get_axis_aligned_bounding_box(self):
        return _Box(np.asarray(self.points, np.float64))

    def translate(self, t):
        self.points = np.asarray(self.points, np.float64) + np.asarray(t, np.float64)
        return self

    def scale(self, f, center):
        c = np.asarray(center, np.float64)
        self.points = (np.asarray(self.points, np.float64) - c) * f + c
        return self


class StandInMesh:
    def __init__(self, v, t):
        self.vertices = np.asarray(v, np.float32).astype(np.float64)
        self.triangles = np.asarray(t, np.int64).reshape(-1, 3)

    def get_axis_aligned_bounding_box(self):
        return _Box(self.vertices)

    def get_surface_area(self):
        return cr.surface_area(self.vertices, self.triangles)[0]

    def get_volume(self):
        if not cr.closed_oriented(self.triangles):
            raise RuntimeError("The mesh is not watertight, and the volume cannot be computed.")
        return cr.volume(self.vertices, self.triangles)[0]


class StandInTree:
    def __init__(self, geometry):
        self.p = np.asarray(geometry.points, np.float64)

    def search_knn_vector_3d(self, q, k):
        d2 = _d2(q, self.p)
        order = np.lexsort((np.arange(len(d2)), d2))[:k]
        return len(order), order.tolist(), d2[order].tolist()

    def search_radius_vector_3d(self, q, r):
        d2 = _d2(q, self.p)
        hit = np.nonzero(d2 < r * r)[0]
        return len(hit), hit.tolist(), d2[hit].tolist()


def import_reference(analysis_dir):
    path = os.path.join(analysis_dir, "computation", "compare_mesh_to_ground_truth.py")
    o3d = types.ModuleType("open3d")
    o3d.geometry = types.SimpleNamespace(PointCloud=StandInCloud, TriangleMesh=StandInMesh, KDTreeFlann=StandInTree)
    o3d.utility = types.SimpleNamespace(Vector3dVector=lambda a: np.asarray(a, np.float64))
    loader = types.ModuleType("mesh_loader")
    loader.load_mesh = lambda p: None
    loader.mesh_to_point_cloud = lambda m, num_points=None: None
    sys.modules.update({"open3d": o3d, "matplotlib": mock.MagicMock(), "matplotlib.pyplot": mock.MagicMock(),
                        "mesh_loader": loader})
    spec = importlib.util.spec_from_file_location("compare_mesh_to_ground_truth_reference", path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod  # @dataclass looks the module up while it executes
    spec.loader.exec_module(mod)
    return mod


# ---------------------------------------------------------------------------- cases
N = 14


def noisy_grid():
    return cr.grid(N, seed=11)


def case_holes():
    v, t = noisy_grid()
    t = cr.drop_cells(t, N, [(r, c) for r in (8, 9, 10) for c in (2, 3, 4)])
    return cr.pinhole(v, t, tri=20)


def case_touching():
    v, t = noisy_grid()
    return v, cr.drop_cells(t, N, [(4, 4), (5, 5)])


def case_degenerate():
    v, t = noisy_grid()
    a, b = 6 * N + 6, 6 * N + 7  # an interior edge: two grid triangles lie on it already
    v = np.concatenate([v, np.array([[0.05, 0.1, 1.0]], np.float32)])
    return v, np.concatenate([t, np.array([[a, b, len(v) - 1], [3, 3, 4]], np.int32)])


def case_cloud():
    rng = np.random.default_rng(5)
    p = rng.standard_normal((700, 3))
    p = p / np.linalg.norm(p, axis=1)[:, None] * (1.0 + 0.03 * rng.standard_normal((700, 1)))
    return p.astype(np.float32), np.zeros((0, 3), np.int32)


def case_shifted():
    v, t = noisy_grid()
    return (v + np.array([0.3, -0.2, 0.1], np.float32)).astype(np.float32), t


CASES = (
    ("identical", lambda: cr.octahedron(3), dict(threshold=None)),
    ("noisy_explicit", noisy_grid, dict(threshold=0.05)),
    ("noisy_auto", noisy_grid, dict(threshold=None)),
    ("holes", case_holes, dict(threshold=None)),
    ("touching", case_touching, dict(threshold=None)),
    ("degenerate", case_degenerate, dict(threshold=None)),
    ("cloud", case_cloud, dict(threshold=None, num_sample_points=500)),
    ("center", case_shifted, dict(threshold=None, align_method="center")),
    ("scale", case_shifted, dict(threshold=None, align_method="center", scale_normalize=True)),
)


def flatten(metrics):
    out = []
    for f in cr.FIELDS:
        out += list(np.atleast_1d(np.asarray(getattr(metrics, f), np.float64)))
    return np.array(out)


def check_margins(name, scan, gt, kw, thr):
    """The two conditions of the docstring, on the restatement's intermediate values."""
    sv, st = scan
    gv, gt_t = gt
    seed, n = kw.get("seed", 0), kw.get("num_sample_points", SAMPLES)
    sp = cr.sample(sv, st, n, seed).astype(np.float64)
    gp = cr.sample(gv, gt_t, n, seed + 1).astype(np.float64)
    slack = 0.0
    if kw.get("scale_normalize"):
        lo, hi = sp.min(0), sp.max(0)
        c = (lo + hi) * 0.5
        sp = (sp - c) * float(np.linalg.norm(gp.max(0) - gp.min(0)) / np.linalg.norm(hi - lo)) + c
    if kw.get("align_method", "none") == "center":
        sp = sp + (gp.mean(0) - sp.mean(0))
        slack = cr.lipschitz(max(np.abs(sp).max(), np.abs(gp).max()))
    for d in (cr.nearest(sp, gp)[0], cr.nearest(gp, sp)[0]):
        gap = np.abs(d - thr).min()
        assert gap > MARGIN * thr + slack, (name, "a distance too near the threshold", gap, thr)
    od = cr.nearest(cr.sample(sv, st, cr.OVERLAP_SAMPLES, seed + 2), cr.sample(gv, gt_t, cr.OVERLAP_SAMPLES, seed + 3))[0]
    assert np.abs(od - cr.OVERLAP_THRESHOLD).min() > MARGIN * cr.OVERLAP_THRESHOLD, (name, "overlap margin")
    for v, t in (scan, gt):
        _, per, bar = cr.count_holes(v, t)
        assert all(abs(p - bar) > MARGIN * bar for p in per), (name, "a hole perimeter too near its bar", per, bar)


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref = import_reference(sys.argv[1])
    from mqr.compare_mesh_to_ground_truth import mesh_to_point_cloud as project_sampler
    gt = cr.octahedron(3)
    out = {"gt_vertices": gt[0], "gt_triangles": gt[1], "cases": np.array([c[0] for c in CASES]),
           "fields": np.array(cr.FIELDS)}
    for name, make, kw in CASES:
        sv, st = make()
        meshes = {"scan": StandInMesh(sv, st), "gt": StandInMesh(*gt)}
        arrays = {id(meshes["scan"]): (sv, st), id(meshes["gt"]): gt}
        seed = kw.get("seed", 0)
        calls = []

        def sampler(mesh, num_points=None, _calls=calls, _arrays=arrays, _seed=seed):
            pc = StandInCloud()
            pc.points = project_sampler(_arrays[id(mesh)], num_points, _seed + len(_calls)).astype(np.float64)
            _calls.append(num_points)
            return pc

        ref.load_mesh = lambda p, _m=meshes: _m[str(p)]
        ref.mesh_to_point_cloud = sampler
        args = dict(num_sample_points=SAMPLES, align_method="none", scale_normalize=False)
        args.update(kw)
        rep = ref.compare_meshes(Path("scan"), Path("gt"), **args)
        assert len(calls) == 4, calls
        check_margins(name, (sv, st), gt, args, rep.threshold)
        out[name + "_vertices"], out[name + "_triangles"] = sv, st
        out[name + "_metrics"] = flatten(rep.metrics)
        out[name + "_threshold_used"] = np.float64(rep.threshold)
        out[name + "_threshold"] = np.float64(np.nan if args["threshold"] is None else args["threshold"])
        out[name + "_num_sample_points"] = np.int64(args["num_sample_points"])
        out[name + "_align_method"] = np.array(args["align_method"])
        out[name + "_scale_normalize"] = np.bool_(args["scale_normalize"])
        out[name + "_seed"] = np.int64(seed)
        print(name, len(sv), len(st), rep.threshold, {f: getattr(rep.metrics, f) for f in cr.FIELDS})
    np.savez_compressed(os.path.join(HERE, "compare_golden.npz"), **out)


if __name__ == "__main__":
    main()
