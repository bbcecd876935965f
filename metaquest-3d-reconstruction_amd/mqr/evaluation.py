"""The reference's intrinsic mesh quality score on the GPU.

Mirrors ``scripts/evaluation/evaluate_fbx_quality.py``: :class:`RawMeshMetrics` and
:class:`QualityScores` with its fields in its order, ``compute_raw_metrics_for_mesh``,
``compute_quality_scores`` and ``write_csv``.  The per-mesh metrics -- the reference's pure-Python
loops over every triangle and every edge -- run in libmqr_hip.so (csrc/meshquality.hip, rules in
DESIGN §2.5); the batch normalisation and the weights are a few dozen float64 operations on the host.

Positions and colours are float32 on the device, as everywhere in this package: a float64 input that
is not float32-representable is rounded to float32 first, then every metric is computed in float64.
"""
from __future__ import annotations

import csv
import ctypes
from dataclasses import asdict, dataclass, fields
from pathlib import Path
from typing import List, Optional

import numpy as np

from ._lib import MQR_DEVICE, MQR_HOST, call, ptr
from .geometry import device_mesh, host_array, mesh_fields


@dataclass
class RawMeshMetrics:
    """One mesh's metrics as the device returns them (fields and order of the reference's class)."""

    name: str
    path: Optional[Path]

    # triangle shape and edge topology
    mean_aspect_ratio: float
    mean_skewness: float
    degenerate_triangles: int
    non_manifold_edges: int
    boundary_edge_ratio: float
    component_count: int
    total_edges: int

    # normals across edges
    normal_deviation_avg_deg: float
    dihedral_min_deg: float
    dihedral_max_deg: float
    dihedral_penalty: float
    surface_roughness: float  # population std of the dihedral angles

    # coverage
    is_single_component: bool
    vertex_density_stddev: float

    # vertex colours
    has_color: bool
    uncolored_vertex_ratio: float
    color_gradient_stddev: float

    # from the counts above
    is_manifold: bool
    is_watertight: bool

    # mesh size
    num_vertices: int
    num_triangles: int


@dataclass
class QualityScores:
    """One mesh's sub-scores and total within its batch (fields and order of the reference's class)."""

    name: str
    path: Optional[Path]
    S_shape: float
    S_topology: float
    S_bonuses: float
    S_geom: float
    S_smooth: float
    S_complete: float
    S_color: float
    Q_raw: float
    Q_norm: float
    raw: RawMeshMetrics


_METRIC_FIELDS = [f for f in fields(RawMeshMetrics) if f.name not in ("name", "path")]


class _Metrics(ctypes.Structure):  # mqr_quality_metrics (include/mqr.h): RawMeshMetrics' order
    _fields_ = [(f.name, ctypes.c_double if f.type == "float" else ctypes.c_int64) for f in _METRIC_FIELDS]


def _host_mesh(vertices, triangles, colors):
    """Checked host arrays (float32 positions / colours, int32 triangles); ValueError before any launch."""
    v = np.asarray(vertices)
    t = np.asarray(triangles)
    if v.ndim != 2 or v.shape[1] != 3 or t.ndim != 2 or t.shape[1] != 3:
        raise ValueError(f"vertices must be (nv, 3) and triangles (nt, 3), got {v.shape} and {t.shape}")
    if v.shape[0] == 0 or t.shape[0] == 0:
        raise ValueError(f"Mesh has no geometry (vertices={v.shape[0]}, triangles={t.shape[0]})")
    if 3 * t.shape[0] >= 2 ** 31:
        raise ValueError("mesh too large (3 * triangles >= 2^31)")
    if not np.isfinite(v).all():
        raise ValueError("a vertex coordinate is not finite")
    if not np.issubdtype(t.dtype, np.integer):
        raise ValueError("triangle indices must be integers")
    if t.min() < 0 or t.max() >= v.shape[0]:
        raise ValueError(f"a triangle index is outside [0, {v.shape[0]})")
    c = None
    if colors is not None:
        c = np.asarray(colors)
        if c.shape != v.shape:
            raise ValueError(f"colors must be {v.shape}, got {c.shape}")
        if not np.isfinite(c).all():
            raise ValueError("a vertex colour is not finite")
        c = np.ascontiguousarray(c, dtype=np.float32)
    return np.ascontiguousarray(v, dtype=np.float32), np.ascontiguousarray(t, dtype=np.int32), c


def _run(device, pv, nv, pc, pt, nt, loc, name, path):
    m = _Metrics()
    call("mqr_mesh_quality", int(device), pv, int(nv), pc, pt, int(nt), loc, ctypes.byref(m))
    kw = {f.name: (bool if f.type == "bool" else float if f.type == "float" else int)(getattr(m, f.name))
          for f in _METRIC_FIELDS}
    return RawMeshMetrics(name=name, path=path, **kw)


def compute_raw_metrics(mesh, name: str = "", path=None, device: int = 0) -> RawMeshMetrics:
    """The reference's raw metrics of one mesh, computed on the GPU.

    ``mesh`` is anything ``geometry.mesh_fields`` unpacks; a tensor mesh held in HBM is read in place
    (``geometry.device_mesh``).  Host arrays are checked with numpy (shape, finite values, index range) and
    raise ``ValueError`` before anything is launched.  Positions and colours are float32 on the device:
    float64 inputs are rounded to float32, then all arithmetic is float64.
    """
    f = mesh_fields(mesh)
    d = device_mesh(f, colors=True, strict=True)
    if d is not None:
        if d.nv == 0 or d.nt == 0:
            raise ValueError(f"Mesh {path} has no geometry (vertices={d.nv}, triangles={d.nt})")
        pc = None if d.colors is None else ctypes.c_void_p(d.colors)
        return _run(d.device, ctypes.c_void_p(d.positions), d.nv, pc, ctypes.c_void_p(d.triangles), d.nt, MQR_DEVICE,
                    name, path)
    if f.kind == "tensor" and f.device is not None:
        from .vbg import parse_device
        device = parse_device(f.device)
    c = None if f.colors is None else host_array(f.colors)
    if c is not None and c.size == 0:
        c = None
    v, t, c = _host_mesh(host_array(f.positions), host_array(f.triangles), c)
    return _run(device, ptr(v), v.shape[0], None if c is None else ptr(c), ptr(t), t.shape[0], MQR_HOST, name, path)


def compute_raw_metrics_for_mesh(path, name: str, device: int = 0) -> RawMeshMetrics:
    """:func:`compute_raw_metrics` of a binary PLY file, under the reference's name and argument order; ``red`` /
    ``green`` / ``blue`` vertex properties, when the file has them, are divided by 255 and taken as colours."""
    from .geometry import read_ply
    path = Path(path)
    props, faces = read_ply(path)
    if not all(k in props for k in ("x", "y", "z")):
        raise ValueError(f"Mesh {path} has no vertex positions")
    v = np.stack([props["x"], props["y"], props["z"]], 1)
    t = faces if faces is not None else np.zeros((0, 3), np.int64)
    c = None
    if all(k in props for k in ("red", "green", "blue")):
        c = np.stack([props["red"], props["green"], props["blue"]], 1).astype(np.float64) / 255.0
    if v.shape[0] == 0 or t.shape[0] == 0:
        raise ValueError(f"Mesh {path} has no geometry (vertices={v.shape[0]}, triangles={t.shape[0]})")
    return compute_raw_metrics((v, t) if c is None else (v, t, c), name=name, path=path, device=device)


def min_max_normalize(values: np.ndarray) -> np.ndarray:
    """Min-max scaling to [0, 1]; a constant array (``np.isclose``) maps to 0.5 everywhere."""
    values = np.asarray(values, dtype=float)
    if values.size == 0:
        return np.zeros(values.shape)
    lo, hi = float(values.min()), float(values.max())
    if np.isclose(lo, hi):
        return np.full(values.shape, 0.5)
    return (values - lo) / (hi - lo)


def compute_quality_scores(raw_metrics: List[RawMeshMetrics]) -> List[QualityScores]:
    """Batch-normalised quality scores (the reference's weights), float64 on the host."""
    if len(raw_metrics) == 0:
        return []

    def norm(get):
        return min_max_normalize(np.array([get(m) for m in raw_metrics], dtype=float))

    ar = norm(lambda m: m.mean_aspect_ratio)
    skew = norm(lambda m: m.mean_skewness)
    deg = norm(lambda m: m.degenerate_triangles)
    nonman = norm(lambda m: m.non_manifold_edges)
    boundary = norm(lambda m: m.boundary_edge_ratio)
    comp = norm(lambda m: max(0, m.component_count - 1))
    normal_dev = norm(lambda m: m.normal_deviation_avg_deg)
    dihedral_pen = norm(lambda m: m.dihedral_penalty)
    rough = norm(lambda m: m.surface_roughness)
    density = norm(lambda m: m.vertex_density_stddev)
    uncolored = norm(lambda m: m.uncolored_vertex_ratio)
    color_grad = norm(lambda m: m.color_gradient_stddev)

    scores: List[QualityScores] = []
    for i, m in enumerate(raw_metrics):
        S_shape = 0.5 * (1.0 - ar[i]) + 0.5 * (1.0 - skew[i])
        S_topology = (0.4 * (1.0 - deg[i]) + 0.3 * (1.0 - nonman[i]) + 0.2 * (1.0 - boundary[i])
                      + 0.1 * (1.0 - comp[i]))
        S_bonuses = 0.5 * (1.0 if m.is_manifold else 0.0) + 0.5 * (1.0 if m.is_watertight else 0.0)
        S_geom = 0.25 * S_shape + 0.15 * S_topology + 0.10 * S_bonuses
        S_smooth = 0.48 * (1.0 - normal_dev[i]) + 0.32 * (1.0 - dihedral_pen[i]) + 0.20 * (1.0 - rough[i])
        S_complete = (0.50 * (1.0 - m.boundary_edge_ratio) + 0.30 * (1.0 if m.is_single_component else 0.0)
                      + 0.20 * (1.0 - density[i]))
        if m.has_color:
            S_color = 0.5 * (1.0 - uncolored[i]) + 0.5 * (1.0 - color_grad[i])
        else:
            S_color = 0.5  # neutral when the mesh has no colours
        Q_raw = 0.50 * S_geom + 0.25 * S_smooth + 0.15 * S_complete + 0.10 * S_color
        scores.append(QualityScores(name=m.name, path=m.path, S_shape=float(S_shape), S_topology=float(S_topology),
                                    S_bonuses=float(S_bonuses), S_geom=float(S_geom), S_smooth=float(S_smooth),
                                    S_complete=float(S_complete), S_color=float(S_color), Q_raw=float(Q_raw),
                                    Q_norm=0.0, raw=m))
    q_norm = min_max_normalize(np.array([s.Q_raw for s in scores], dtype=float))
    for i, s in enumerate(scores):
        s.Q_norm = float(q_norm[i])
    return scores


CSV_FIELDS = ["name", "path", "Q_raw", "Q_norm", "S_geom", "S_smooth", "S_complete", "S_color", "S_shape",
              "S_topology", "S_bonuses"] + [f.name for f in _METRIC_FIELDS]


def write_csv(scores: List[QualityScores], csv_path) -> None:
    """The reference's ``quality_scores.csv``: its columns in its order, one row per mesh."""
    csv_path = Path(csv_path)
    csv_path.parent.mkdir(parents=True, exist_ok=True)
    with csv_path.open("w", newline="") as f:
        writer = csv.DictWriter(f, fieldnames=CSV_FIELDS)
        writer.writeheader()
        for s in scores:
            row = {k: getattr(s, k) for k in CSV_FIELDS[2:11]}
            row["name"] = s.name
            row["path"] = str(s.path)
            row.update({k: v for k, v in asdict(s.raw).items() if k not in ("name", "path")})
            writer.writerow(row)
