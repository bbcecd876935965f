"""Golden mesh-quality metrics from the reference's own function.  Tests never run this.

Run where the reference checkout is available:
    python tests/golden/make_quality_golden.py <the reference's scripts directory>
It imports the reference's scripts/evaluation/evaluate_fbx_quality.py (read-only) with ``open3d``,
``matplotlib``, ``matplotlib.pyplot`` and ``evaluation.mesh_loader`` stubbed, points its ``load_mesh`` at
the stand-in mesh class below, calls its ``compute_raw_metrics_for_mesh`` on five small meshes and its
``compute_quality_scores`` on the batch, and stores the meshes with every returned field in
tests/golden/quality_golden.npz.  Nothing from the reference is copied.

The stand-in mesh restates the two Open3D legacy routines the reference calls (the one unpinned piece,
DESIGN §2.5): triangle normal (p1 - p0) x (p2 - p0); vertex normal = the sum of the unnormalised
triangle normals of its corners, added triangle by triangle, corners 0, 1, 2; both divided by their
length, a zero vector staying zero.

Cases (all coordinates float32-representable: generated in float32 and widened):
  mixed          noisy 12x12 grid + a 4x4 grid 1 m above it + a fin triangle on an interior edge + (5,5,6)
                 + (0,0,0) + a collinear triangle on three vertices of its own + an unreferenced vertex,
                 random colours, default_rng(0)
  closed         octahedron subdivided 3x on the unit sphere, no colours (258 / 512, watertight)
  flat           exact 9x9 planar grid, steps 0.125 x 0.25, z = 0.5 (zero extent, vertices on cell faces)
  alldegenerate  (0,0,1), (0,1,2) collinear, (3,3,3): every default; edge (0,1) has multiplicity 3
  big            noisy 48x48 grid with colours, default_rng(7) (2304 / 4418)
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
from quality_ref import FIELDS, grid_mesh  # noqa: E402

SCORE_FIELDS = ("S_shape", "S_topology", "S_bonuses", "S_geom", "S_smooth", "S_complete", "S_color", "Q_raw",
                "Q_norm")


class _Box:
    def __init__(self, v):
        self.min_bound = v.min(0)
        self._ext = v.max(0) - v.min(0)

    def get_extent(self):
        return self._ext.copy()


class StandInMesh:
    """What the reference reads of an Open3D legacy TriangleMesh; TriangleMesh(mesh) copies."""

    def __init__(self, other=None):
        self.vertices = np.zeros((0, 3)) if other is None else other.vertices.copy()
        self.triangles = np.zeros((0, 3), int) if other is None else other.triangles.copy()
        self.vertex_colors = np.zeros((0, 3)) if other is None else other.vertex_colors.copy()
        self.vertex_normals = np.zeros((0, 3))
        self.triangle_normals = np.zeros((0, 3))

    def has_vertex_colors(self):
        return len(self.vertex_colors) > 0 and len(self.vertex_colors) == len(self.vertices)

    def get_axis_aligned_bounding_box(self):
        return _Box(self.vertices)

    @staticmethod
    def _normalize(n):
        for k in range(len(n)):
            z = (n[k, 0] * n[k, 0] + n[k, 1] * n[k, 1]) + n[k, 2] * n[k, 2]
            if z > 0:
                n[k] = n[k] / np.sqrt(z)
        return n

    def _raw_triangle_normals(self):
        v, t = self.vertices, self.triangles
        out = np.zeros((len(t), 3))
        for k, (i0, i1, i2) in enumerate(t):
            a, b = v[i1] - v[i0], v[i2] - v[i0]
            out[k] = (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])
        return out

    def compute_triangle_normals(self):
        self.triangle_normals = self._normalize(self._raw_triangle_normals())

    def compute_vertex_normals(self):
        tn = self._raw_triangle_normals()
        vn = np.zeros((len(self.vertices), 3))
        for k, tri in enumerate(self.triangles):
            for i in tri:
                vn[i] = vn[i] + tn[k]
        self.vertex_normals = self._normalize(vn)
        self.triangle_normals = self._normalize(tn)


def import_reference(ref_scripts):
    path = os.path.join(ref_scripts, "evaluation", "evaluate_fbx_quality.py")
    o3d = types.ModuleType("open3d")
    o3d.geometry = types.SimpleNamespace(TriangleMesh=StandInMesh)
    loader = types.ModuleType("evaluation.mesh_loader")
    loader.load_mesh = lambda p: None
    pkg = types.ModuleType("evaluation")
    pkg.__path__ = []
    stubs = {"open3d": o3d, "matplotlib": mock.MagicMock(), "matplotlib.pyplot": mock.MagicMock(), "evaluation": pkg,
             "evaluation.mesh_loader": loader}
    sys.modules.update(stubs)
    spec = importlib.util.spec_from_file_location("evaluate_fbx_quality", path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules["evaluate_fbx_quality"] = mod  # @dataclass looks the module up while it executes
    spec.loader.exec_module(mod)
    return mod


# ---------------------------------------------------------------------- the five meshes
def case_mixed():
    rng = np.random.default_rng(0)
    v, t = grid_mesh(12, 12, rng, noise=0.08)
    v2, t2 = grid_mesh(4, 4, rng, noise=0.02)
    v2 = (v2 + np.array([3.0, 3.0, 1.0], np.float32)).astype(np.float32)
    n0 = len(v)
    verts = [v, v2]
    tris = [t, t2 + n0]
    n = n0 + len(v2)
    # a fin on the interior edge (5*12+5, 5*12+6): a third triangle on it, to a vertex above the grid
    verts.append(np.array([[5.0, 5.5, 0.75]], np.float32))
    tris.append(np.array([[5 * 12 + 5, 5 * 12 + 6, n]], np.int32))
    n += 1
    tris.append(np.array([[5, 5, 6], [0, 0, 0]], np.int32))
    verts.append(np.array([[20.0, 0.0, 0.0], [20.5, 0.0, 0.0], [21.5, 0.0, 0.0]], np.float32))  # collinear
    tris.append(np.array([[n, n + 1, n + 2]], np.int32))
    n += 3
    verts.append(np.array([[-3.0, -3.0, 2.0]], np.float32))  # unreferenced
    v = np.concatenate(verts).astype(np.float32)
    return v, np.concatenate(tris).astype(np.int32), rng.random(v.shape).astype(np.float32)


def case_closed():
    v = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    v = [np.array(p, float) for p in v]
    t = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    for _ in range(3):
        mid, t2 = {}, []

        def midpoint(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[k] = len(v) - 1
            return mid[k]

        for a, b, c in t:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            t2 += [(a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca)]
        t = t2
    return np.array(v).astype(np.float32), np.array(t, np.int32), None


def case_flat():
    v, t = grid_mesh(9, 9, step=(0.125, 0.25), z=0.5)
    return v, t, None


def case_alldegenerate():
    v = np.array([[0, 0, 0], [1, 0, 0], [2.5, 0, 0], [0, 1, 0]], np.float32)
    return v, np.array([[0, 0, 1], [0, 1, 2], [3, 3, 3]], np.int32), None


def case_big():
    rng = np.random.default_rng(7)
    v, t = grid_mesh(48, 48, rng, noise=0.3)
    return v, t, rng.random(v.shape).astype(np.float32)


CASES = (("mixed", case_mixed), ("closed", case_closed), ("flat", case_flat), ("alldegenerate", case_alldegenerate),
         ("big", case_big))


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref = import_reference(sys.argv[1])
    out, raws = {}, []
    for name, make in CASES:
        v, t, c = make()
        mesh = StandInMesh()
        mesh.vertices = v.astype(np.float64)
        mesh.triangles = t.astype(int)
        if c is not None:
            mesh.vertex_colors = c.astype(np.float64)
        ref.load_mesh = lambda p, _m=mesh: _m
        raw = ref.compute_raw_metrics_for_mesh(Path(name + ".ply"), name)
        raws.append(raw)
        out[name + "_vertices"], out[name + "_triangles"] = v, t
        if c is not None:
            out[name + "_colors"] = c
        out[name + "_raw"] = np.array([float(getattr(raw, f)) for f in FIELDS], np.float64)
        print(name, len(v), len(t), {f: getattr(raw, f) for f in FIELDS})
    scores = ref.compute_quality_scores(raws)
    out["scores"] = np.array([[float(getattr(s, f)) for f in SCORE_FIELDS] for s in scores], np.float64)
    out["cases"] = np.array([n for n, _ in CASES])
    out["fields"] = np.array(FIELDS)
    out["score_fields"] = np.array(SCORE_FIELDS)
    np.savez_compressed(os.path.join(HERE, "quality_golden.npz"), **out)


if __name__ == "__main__":
    main()
