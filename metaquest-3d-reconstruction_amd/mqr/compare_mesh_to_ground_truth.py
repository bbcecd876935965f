"""Accuracy of a reconstructed mesh against a ground-truth model, on the GPU.

Mirrors ``analysis/computation/compare_mesh_to_ground_truth.py``: :class:`ComparisonMetrics`,
:class:`ComparisonReport` and :class:`DualComparisonReport` with its fields in its order, ``compare_meshes``,
``compare_dual_scans`` and the metric functions under its names.  Every Open3D call of the reference comes
down to three device primitives of libmqr_hip.so (csrc/meshcompare.hip, rules in DESIGN §2.6): the exact
nearest neighbour of every query point, the statistics of a distance array (only a small struct comes back
to the host), and one measure pass per mesh (area, bounds, volume, boundary edges).

A mesh is a path to a binary PLY file or anything ``geometry.mesh_fields`` unpacks; a mesh held in HBM is
measured and searched in place.  A mesh without triangles -- also a ``PointCloud`` or a bare ``(n, 3)``
array -- is a point cloud.  A "point cloud" argument of the metric functions is an ``(n, 3)`` array.

Stated differences from the reference:

* Sampling.  Open3D's random stream cannot be matched, so :func:`mesh_to_point_cloud` has its own rule,
  seeded: triangle by ``searchsorted`` on the cumulative areas, barycentric weights
  ``(1 - sqrt(r1), sqrt(r1) (1 - r2), sqrt(r1) r2)``, all in float64 on the host, rounded to float32.
  ``compare_meshes`` uses seeds ``seed .. seed + 3`` for the scan sample, the ground-truth sample and the two
  10 000-point overlap samples.
* Positions are float32 on the device: samples moved by an alignment or a scale are rounded to float32
  before they are searched.
* Volume is reported for a mesh whose every edge lies on two triangles that traverse it in opposite
  directions; vertex-manifoldness and self-intersection, which Open3D also demands, are not tested.
* ``threshold=None`` with a ground truth of zero extent raises ``ValueError`` (the reference falls back to
  an unseeded random estimate).
"""
from __future__ import annotations

import ctypes
import json
from dataclasses import asdict, dataclass
from pathlib import Path
from typing import List, Optional, Tuple

import numpy as np

from ._lib import MQR_DEVICE, MQR_HOST, DeviceBuffer, call, ptr
from .geometry import PointCloud, device_mesh, host_array, mesh_fields, read_ply

OVERLAP_SAMPLES = 10000     # compute_volume_metrics' samples per mesh
OVERLAP_THRESHOLD = 0.01    # ... and its radius (1 cm)


@dataclass
class ComparisonMetrics:
    """Metrics of a scan against its ground truth (fields and order of the reference's class)."""

    chamfer_distance: float
    hausdorff_distance: float

    mean_point_to_surface: float
    median_point_to_surface: float
    std_point_to_surface: float
    max_point_to_surface: float

    precision: float  # share of scan samples within the threshold of the ground truth
    recall: float     # share of ground-truth samples within the threshold of the scan
    f_score: float

    volume_scan: float
    volume_gt: float
    volume_overlap: float
    volume_iou: float

    bounding_box_ratio: Tuple[float, float, float]  # scan / ground truth per axis
    center_offset: Tuple[float, float, float]       # scan box centre - ground-truth box centre

    num_scan_points: int
    num_gt_points: int

    surface_area_scan: float
    surface_area_gt: float
    num_holes_scan: int
    num_holes_gt: int


@dataclass
class ComparisonReport:
    scan_path: Optional[Path]
    ground_truth_path: Optional[Path]
    metrics: ComparisonMetrics
    threshold: float
    warnings: List[str]
    errors: List[str]


@dataclass
class DualComparisonReport:
    ground_truth_path: Optional[Path]
    no_fog_scan_path: Optional[Path]
    fog_scan_path: Optional[Path]
    no_fog_report: ComparisonReport
    fog_report: ComparisonReport
    improvement: dict  # fog - no_fog


# ---------------------------------------------------------------------------- the C ABI
class _Stats(ctypes.Structure):  # mqr_distance_stats_result
    _fields_ = [("mean", ctypes.c_double), ("std", ctypes.c_double), ("min", ctypes.c_double),
                ("max", ctypes.c_double), ("median", ctypes.c_double), ("count_below", ctypes.c_int64),
                ("count", ctypes.c_int64)]


class _Measure(ctypes.Structure):  # mqr_mesh_measure_result
    _fields_ = [("surface_area", ctypes.c_double), ("volume", ctypes.c_double), ("min_bound", ctypes.c_double * 3),
                ("max_bound", ctypes.c_double * 3), ("is_closed_oriented", ctypes.c_int64),
                ("boundary_edges", ctypes.c_int64), ("num_vertices", ctypes.c_int64),
                ("num_triangles", ctypes.c_int64)]


def _points(p) -> np.ndarray:
    """A point set as a contiguous (n, 3) float32 host array (float64 input is rounded)."""
    if isinstance(p, PointCloud):
        p = p.point.positions
    a = np.asarray(host_array(p))
    if a.ndim != 2 or a.shape[1] != 3:
        raise ValueError(f"points must be (n, 3), got {a.shape}")
    if not (np.abs(a) <= 1e18).all():  # (a NaN fails the comparison) the search's coordinate range, include/mqr.h
        raise ValueError("a point coordinate is not finite or beyond 1e18 in magnitude")
    return np.ascontiguousarray(a, dtype=np.float32)


class NearestNeighbour:
    """The exact nearest target of query points (mqr_nn): ``targets`` is an ``(n, 3)`` host array, or a
    ``(pointer, n)`` pair of float32 xyz already in HBM on ``device`` (read in place while the tree is built)."""

    def __init__(self, targets, device: int = 0):
        self.device = int(device)
        self._h = None
        h = ctypes.c_void_p()
        if isinstance(targets, tuple):
            p, n = targets
            call("mqr_nn_create", self.device, ctypes.c_void_p(p), int(n), MQR_DEVICE, ctypes.byref(h))
        else:
            a = _points(targets)
            if len(a) == 0:
                raise ValueError("the target point set is empty")
            call("mqr_nn_create", self.device, ptr(a), len(a), MQR_HOST, ctypes.byref(h))
        self._h = h

    def query(self, queries, indices: bool = False):
        """Distances (float64) of host queries to their nearest target, with ``indices`` also its index."""
        q = _points(queries)
        d = np.empty(len(q), np.float64)
        i = np.empty(len(q), np.int32) if indices else None
        call("mqr_nn_query", self._h, ptr(q), len(q), MQR_HOST, ptr(d), None if i is None else ptr(i), MQR_HOST)
        return (d, i) if indices else d

    def query_stats(self, queries: DeviceBuffer, nq: int, threshold: float) -> _Stats:
        """Statistics of the distances of ``nq`` queries in HBM; the distances never leave the device."""
        d = DeviceBuffer(8 * nq, self.device)
        try:
            call("mqr_nn_query", self._h, queries.ptr, int(nq), MQR_DEVICE, d.ptr, None, MQR_DEVICE)
            return _device_stats(self.device, d.ptr, nq, MQR_DEVICE, threshold)
        finally:
            d.free()

    def close(self):
        from . import _lib
        if self._h is not None and self._h.value and _lib._lib is not None:
            _lib._lib.mqr_nn_destroy(self._h)
        self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _device_stats(device, p, n, loc, threshold) -> _Stats:
    s = _Stats()
    call("mqr_distance_stats", int(device), p, int(n), loc, float(threshold), ctypes.byref(s))
    return s


def distance_stats(distances, threshold: float = 0.0, device: int = 0) -> dict:
    """mean, population std, min, max, median and the count of values ``< threshold`` of a non-negative
    float64 array, reduced on the device in a fixed order."""
    d = np.ascontiguousarray(distances, np.float64).reshape(-1)
    if len(d) == 0:
        raise ValueError("the distance array is empty")
    s = _device_stats(device, ptr(d), len(d), MQR_HOST, threshold)
    return {k: getattr(s, k) for k, _ in _Stats._fields_}


def point_cloud_distance(source, target, device: int = 0) -> np.ndarray:
    """For each source point the distance to its nearest target point (float64): the stand-in for Open3D's
    ``source.compute_point_cloud_distance(target)``."""
    source, target = _points(source), _points(target)  # both checked before anything is launched
    with NearestNeighbour(target, device) as nn:
        return nn.query(source)


# ---------------------------------------------------------------------------- meshes
class _Mesh:
    """A loaded mesh: host arrays (fetched once when the mesh lives in HBM) and, there, its device pointers."""

    def __init__(self, mesh):
        self.path, self.dm, self._v, self._t = None, None, None, None
        if isinstance(mesh, _Mesh):
            self.__dict__.update(mesh.__dict__)
            return
        if isinstance(mesh, (str, Path)):
            self.path = Path(mesh)
            props, faces = read_ply(self.path)
            if not all(k in props for k in ("x", "y", "z")):
                raise ValueError(f"Mesh {self.path} has no vertex positions")
            self._v = np.stack([props["x"], props["y"], props["z"]], 1)
            self._t = faces if faces is not None else np.zeros((0, 3), np.int32)
        elif isinstance(mesh, PointCloud) or (isinstance(mesh, np.ndarray) and mesh.ndim == 2):
            self._v = _points(mesh)
            self._t = np.zeros((0, 3), np.int32)
        else:
            f = mesh_fields(mesh)
            self.dm = device_mesh(f)
            self._f = f
        if self._v is not None:
            self._check()

    def _check(self):
        v, t = np.asarray(self._v), np.asarray(self._t)
        if v.ndim != 2 or v.shape[1] != 3 or v.shape[0] == 0:
            raise ValueError(f"vertices must be (nv, 3) with nv > 0, got {v.shape}")
        t = t.reshape(-1, 3)
        if 3 * t.shape[0] >= 2 ** 31:
            raise ValueError("mesh too large (3 * triangles >= 2^31)")
        if not np.isfinite(v).all():
            raise ValueError("a vertex coordinate is not finite")
        if len(t) and (not np.issubdtype(t.dtype, np.integer) or t.min() < 0 or t.max() >= v.shape[0]):
            raise ValueError(f"a triangle index is outside [0, {v.shape[0]})")
        self._v = np.ascontiguousarray(v, dtype=np.float32)
        self._t = np.ascontiguousarray(t, dtype=np.int32)

    def _host(self):
        if self._v is None:
            self._v = host_array(self._f.positions)
            t = self._f.triangles
            self._t = np.zeros((0, 3), np.int32) if t is None else host_array(t)
            self._v = np.asarray(self._v).reshape(-1, 3)
            self._check()

    @property
    def vertices(self) -> np.ndarray:
        self._host()
        return self._v

    @property
    def triangles(self) -> np.ndarray:
        self._host()
        return self._t

    def device_id(self, default):
        return self.dm.device if self.dm is not None else int(default)

    def vertex_tree(self, device) -> NearestNeighbour:
        if self.dm is not None:
            return NearestNeighbour((self.dm.positions, self.dm.nv), self.dm.device)
        return NearestNeighbour(self.vertices, device)


@dataclass
class MeshMeasure:
    """One mesh's measure pass (mqr_mesh_measure)."""
    surface_area: float
    volume: float
    min_bound: np.ndarray
    max_bound: np.ndarray
    is_closed_oriented: bool
    boundary: np.ndarray  # (n, 2) int32 (min, max) vertex pairs, ascending by slot 3 t + e
    num_vertices: int
    num_triangles: int

    @property
    def extent(self):
        return self.max_bound - self.min_bound

    @property
    def center(self):
        return (self.min_bound + self.max_bound) * 0.5


def measure_mesh(mesh, device: int = 0) -> MeshMeasure:
    """Surface area, bounds, volume and the ordered boundary-edge list of one mesh, on the device."""
    m = _Mesh(mesh)
    r, e = _Measure(), ctypes.c_void_p()
    if m.dm is not None:
        d = m.dm
        if d.nv == 0:
            raise ValueError("the mesh has no vertices")
        dev = d.device
        call("mqr_mesh_measure", dev, ctypes.c_void_p(d.positions), d.nv, ctypes.c_void_p(d.triangles), d.nt,
             MQR_DEVICE, ctypes.byref(r), ctypes.byref(e))
    else:
        dev = int(device)
        v, t = m.vertices, m.triangles
        call("mqr_mesh_measure", dev, ptr(v), len(v), ptr(t) if len(t) else None, len(t), MQR_HOST,
             ctypes.byref(r), ctypes.byref(e))
    boundary = np.zeros((int(r.boundary_edges), 2), np.int32)
    try:
        if e.value:
            call("mqr_edge_list_copy", e, ptr(boundary), MQR_HOST)
    finally:
        if e.value:
            call("mqr_edge_list_free", e)
    return MeshMeasure(float(r.surface_area), float(r.volume), np.array(r.min_bound[:]), np.array(r.max_bound[:]),
                       bool(r.is_closed_oriented), boundary, int(r.num_vertices), int(r.num_triangles))


# ---------------------------------------------------------------------------- sampling (host, float64)
def _sample_triangles(vertices, triangles, num_points: int, seed: int):
    """(points float64, triangle index) of ``num_points`` area-weighted samples: the rule of the module docstring."""
    v = np.asarray(vertices, np.float64)
    t = np.asarray(triangles).reshape(-1, 3)
    a, b, c = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    cum = np.cumsum(0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1))
    rng = np.random.default_rng(seed)
    k = np.searchsorted(cum, rng.random(num_points) * cum[-1], side="right")
    k = np.minimum(k, len(t) - 1)
    s = np.sqrt(rng.random(num_points))[:, None]
    r2 = rng.random(num_points)[:, None]
    return (1.0 - s) * a[k] + (s * (1.0 - r2)) * b[k] + (s * r2) * c[k], k


def mesh_to_point_cloud(mesh, num_points: Optional[int] = None, seed: int = 0) -> np.ndarray:
    """``num_points`` samples of the mesh's surface as an ``(n, 3)`` float32 array; ``None``: its vertices.  A mesh
    without triangles gives its vertices when there are at most ``num_points`` of them, else ``num_points`` of
    them chosen without replacement (the reference's vertex branch, seeded)."""
    m = _Mesh(mesh)
    v, t = m.vertices, m.triangles
    if num_points is None:
        return v.copy()
    if len(t) > 0:
        return np.ascontiguousarray(_sample_triangles(v, t, int(num_points), seed)[0], np.float32)
    if len(v) <= num_points:
        return v.copy()
    return np.ascontiguousarray(v[np.random.default_rng(seed).choice(len(v), size=int(num_points), replace=False)])


# ---------------------------------------------------------------------------- the reference's metric functions
def compute_chamfer_distance(scan_pcd, gt_pcd, device: int = 0):
    """(mean scan-to-GT distance + mean GT-to-scan distance, scan-to-GT distances, GT-to-scan distances)."""
    s2g = point_cloud_distance(scan_pcd, gt_pcd, device)
    g2s = point_cloud_distance(gt_pcd, scan_pcd, device)
    chamfer = distance_stats(s2g, device=device)["mean"] + distance_stats(g2s, device=device)["mean"]
    return float(chamfer), s2g, g2s


def compute_hausdorff_distance(scan_pcd, gt_pcd, device: int = 0) -> float:
    s2g = point_cloud_distance(scan_pcd, gt_pcd, device)
    g2s = point_cloud_distance(gt_pcd, scan_pcd, device)
    return float(max(distance_stats(s2g, device=device)["max"], distance_stats(g2s, device=device)["max"]))


def compute_point_to_surface_distance(scan_pcd, gt_mesh, device: int = 0) -> np.ndarray:
    """Distance of each scan point to the nearest ground-truth VERTEX (what the reference computes)."""
    m = _Mesh(gt_mesh)
    with m.vertex_tree(device) as nn:
        return nn.query(scan_pcd)


def _f_score(precision: float, recall: float) -> float:
    return float(2 * (precision * recall) / (precision + recall)) if precision + recall > 0 else 0.0


def compute_f_score(scan_pcd, gt_pcd, threshold: float, device: int = 0):
    """(precision, recall, F-score) at ``threshold`` (strict ``<``)."""
    s2g = distance_stats(point_cloud_distance(scan_pcd, gt_pcd, device), threshold, device)
    g2s = distance_stats(point_cloud_distance(gt_pcd, scan_pcd, device), threshold, device)
    precision, recall = s2g["count_below"] / s2g["count"], g2s["count_below"] / g2s["count"]
    return float(precision), float(recall), _f_score(precision, recall)


def _overlap_ratio(scan: _Mesh, gt: _Mesh, seed: int, device: int) -> float:
    sp = mesh_to_point_cloud(scan, OVERLAP_SAMPLES, seed + 2)
    gp = mesh_to_point_cloud(gt, OVERLAP_SAMPLES, seed + 3)
    with NearestNeighbour(gp, device) as nn:
        q = DeviceBuffer.from_array(sp, device)
        try:
            st = nn.query_stats(q, len(sp), OVERLAP_THRESHOLD)
        finally:
            q.free()
    return st.count_below / len(sp) if len(sp) else 0.0


def _volume_metrics(vol_scan, vol_gt, ratio):
    overlap = vol_scan * ratio
    union = vol_scan + vol_gt - overlap
    return float(vol_scan), float(vol_gt), float(overlap), float(overlap / union if union > 0 else 0.0)


def compute_volume_metrics(scan_mesh, gt_mesh, seed: int = 0, device: int = 0):
    """(scan volume, GT volume, overlap volume, IoU): the overlap is the scan volume times the share of 10 000
    scan samples (seed + 2) with a GT sample (seed + 3) nearer than 1 cm."""
    s, g = _Mesh(scan_mesh), _Mesh(gt_mesh)
    return _volume_metrics(measure_mesh(s, device).volume, measure_mesh(g, device).volume,
                           _overlap_ratio(s, g, seed, device))


def compute_surface_area(mesh, device: int = 0) -> float:
    return measure_mesh(mesh, device).surface_area


def hole_perimeters(boundary, vertices) -> List[float]:
    """The closed loops of the reference's boundary walk and their perimeters, in the order it finds them.

    ``boundary``: the (min, max) pairs in the order the reference's edge dictionary lists them.  Every vertex,
    in order of first appearance, starts a walk along its first neighbour whose edge is unvisited; each step
    takes the first unvisited neighbour, and a walk counts as a hole when it returns to its start after more
    than two edges."""
    boundary = [(int(a), int(b)) for a, b in np.asarray(boundary).reshape(-1, 2)]
    v = np.asarray(vertices, np.float64)
    adj = {}
    for a, b in boundary:
        adj.setdefault(a, [])
        adj.setdefault(b, [])
        adj[a].append(b)
        adj[b].append(a)

    def key(a, b):
        return (a, b) if a <= b else (b, a)

    visited, perimeters = set(), []
    for start in adj:
        nxt = next((w for w in adj[start] if key(start, w) not in visited), None)
        if nxt is None:
            continue
        cur, loop, length = start, [start], 0
        while key(cur, nxt) not in visited:
            visited.add(key(cur, nxt))
            length += 1
            cur = nxt
            loop.append(cur)
            if cur == start and length > 2:
                p = 0.0
                for i in range(len(loop) - 1):
                    p += float(np.linalg.norm(v[loop[i]] - v[loop[i + 1]]))
                perimeters.append(p)
                break
            nxt = next((w for w in adj[cur] if key(cur, w) not in visited), None)
            if nxt is None or length > len(boundary):
                break
    return perimeters


def _count_holes(measure: MeshMeasure, vertices, min_hole_size_ratio):
    if measure.num_triangles == 0 or len(measure.boundary) == 0:
        return 0
    bar = np.linalg.norm(measure.extent) * min_hole_size_ratio
    return sum(1 for p in hole_perimeters(measure.boundary, vertices) if p >= bar)


def count_holes(mesh, min_hole_size_ratio: float = 0.01, device: int = 0) -> int:
    """Boundary loops whose perimeter is at least ``min_hole_size_ratio`` of the bounding-box diagonal."""
    m = _Mesh(mesh)
    return _count_holes(measure_mesh(m, device), m.vertices, min_hole_size_ratio)


def _scale_and_alignment(ms: MeshMeasure, mg: MeshMeasure):
    se, ge = ms.extent, mg.extent
    ratios = tuple(float(se[a] / ge[a]) if ge[a] > 0 else 0.0 for a in range(3))
    off = ms.center - mg.center
    return ratios, (float(off[0]), float(off[1]), float(off[2]))


def compute_scale_and_alignment_metrics(scan_mesh, gt_mesh, device: int = 0):
    """(scan / GT extent ratio per axis, scan box centre - GT box centre)."""
    return _scale_and_alignment(measure_mesh(scan_mesh, device), measure_mesh(gt_mesh, device))


def align_point_clouds(source_pcd, target_pcd, method: str = "center", device: int = 0):
    """(aligned source as float64, 4x4 transform).  ``center``: the clouds' mean points coincide.  ``icp``: that
    shift, then one level of point-to-point ICP on the full clouds (distance 0.1, 50 iterations) from the
    identity (mqr.registration).  The caller rounds the result to float32.  The transform maps the source as it
    was given onto the aligned cloud: for ``icp`` it is ``T_icp @ shift``, where the reference returns ``T_icp``
    alone (its ``transform`` is still the identity when it multiplies); no metric reads it."""
    src = np.asarray(source_pcd, np.float64)
    if method == "none":
        return src, np.eye(4)
    if method not in ("center", "icp"):
        raise ValueError(f"unknown alignment method {method!r}")
    tgt = np.asarray(target_pcd, np.float64)
    transform = np.eye(4)
    transform[:3, 3] = tgt.mean(0) - src.mean(0)
    aligned = src + transform[:3, 3]
    if method == "icp":
        from .registration import CloudSet, ICPConvergenceCriteria
        cs = CloudSet([aligned.astype(np.float32), tgt.astype(np.float32)], device)
        try:
            res = cs.icp_pairs([0], [1], [-1.0], [ICPConvergenceCriteria(1e-6, 1e-6, 50)], [0.1])[0]
        finally:
            cs.close()
        T = res.transformation
        aligned = aligned @ T[:3, :3].T + T[:3, 3]
        transform = T @ transform
    return aligned, transform


def normalize_scale(pcd, target_scale: Optional[float] = None, reference_pcd=None):
    """(the cloud scaled about its box centre so that its box diagonal is the target's, the factor), float64."""
    p = np.asarray(pcd, np.float64)
    if target_scale is None and reference_pcd is None:
        return p, 1.0
    lo, hi = p.min(0), p.max(0)
    current = np.linalg.norm(hi - lo)
    if target_scale is None:
        r = np.asarray(reference_pcd, np.float64)
        target_scale = float(np.linalg.norm(r.max(0) - r.min(0)))
    if current == 0:
        return p, 1.0
    factor = float(target_scale / current)
    center = (lo + hi) * 0.5
    return (p - center) * factor + center, factor


# ---------------------------------------------------------------------------- the report
def compare_meshes(scan, ground_truth, threshold: Optional[float] = None, num_sample_points: int = 50000,
                   align_method: str = "none", scale_normalize: bool = False, seed: int = 0,
                   device: int = 0) -> ComparisonReport:
    """The reference's report of one scan against its ground truth (module docstring: inputs and differences)."""
    scan, gt = _Mesh(scan), _Mesh(ground_truth)
    device = gt.device_id(scan.device_id(device))
    ms, mg = measure_mesh(scan, device), measure_mesh(gt, device)

    scan_pts = mesh_to_point_cloud(scan, num_sample_points, seed)
    gt_pts = mesh_to_point_cloud(gt, num_sample_points, seed + 1)
    if scale_normalize or align_method != "none":
        moved = scan_pts.astype(np.float64)
        if scale_normalize:
            moved, _ = normalize_scale(moved, reference_pcd=gt_pts)
        moved, _ = align_point_clouds(moved, gt_pts, align_method, device)
        scan_pts = np.ascontiguousarray(moved, np.float32)

    if threshold is None:
        threshold_value = float(np.linalg.norm(mg.extent) * 0.01)
        if threshold_value == 0.0:
            raise ValueError("the ground truth has zero extent: pass an explicit threshold")
    else:
        threshold_value = float(threshold)

    ns, ng = len(scan_pts), len(gt_pts)
    sq, gq = DeviceBuffer.from_array(scan_pts, device), DeviceBuffer.from_array(gt_pts, device)
    try:
        with NearestNeighbour((gq.ptr.value, ng), device) as nn:
            s2g = nn.query_stats(sq, ns, threshold_value)
        with NearestNeighbour((sq.ptr.value, ns), device) as nn:
            g2s = nn.query_stats(gq, ng, threshold_value)
        with gt.vertex_tree(device) as nn:
            p2s = nn.query_stats(sq, ns, threshold_value)
    finally:
        sq.free()
        gq.free()

    precision, recall = s2g.count_below / ns, g2s.count_below / ng
    ratio = _overlap_ratio(scan, gt, seed, device)
    volume_scan, volume_gt, volume_overlap, volume_iou = _volume_metrics(ms.volume, mg.volume, ratio)
    bbox_ratio, center_offset = _scale_and_alignment(ms, mg)
    metrics = ComparisonMetrics(
        chamfer_distance=float(s2g.mean + g2s.mean),
        hausdorff_distance=float(max(s2g.max, g2s.max)),
        mean_point_to_surface=float(p2s.mean),
        median_point_to_surface=float(p2s.median),
        std_point_to_surface=float(p2s.std),
        max_point_to_surface=float(p2s.max),
        precision=float(precision),
        recall=float(recall),
        f_score=_f_score(precision, recall),
        volume_scan=volume_scan,
        volume_gt=volume_gt,
        volume_overlap=volume_overlap,
        volume_iou=volume_iou,
        bounding_box_ratio=bbox_ratio,
        center_offset=center_offset,
        num_scan_points=ns,
        num_gt_points=ng,
        surface_area_scan=ms.surface_area,
        surface_area_gt=mg.surface_area,
        num_holes_scan=_count_holes(ms, scan.vertices, 0.01),
        num_holes_gt=_count_holes(mg, gt.vertices, 0.01),
    )
    return ComparisonReport(scan_path=scan.path, ground_truth_path=gt.path, metrics=metrics,
                            threshold=threshold_value, warnings=[], errors=[])


IMPROVEMENT_KEYS = ("chamfer_distance", "hausdorff_distance", "mean_point_to_surface", "median_point_to_surface",
                    "max_point_to_surface", "f_score", "precision", "recall", "surface_area_scan", "num_holes_scan")


def compare_dual_scans(no_fog_scan, fog_scan, ground_truth, threshold: Optional[float] = None,
                       num_sample_points: int = 50000, align_method: str = "none", scale_normalize: bool = False,
                       seed: int = 0, device: int = 0) -> DualComparisonReport:
    """Both scans against one ground truth; ``improvement[k]`` = fog - no_fog (distances and holes: negative is
    better; scores and area: positive is better)."""
    gt = _Mesh(ground_truth)
    kw = dict(threshold=threshold, num_sample_points=num_sample_points, align_method=align_method,
              scale_normalize=scale_normalize, seed=seed, device=device)
    no_fog = compare_meshes(no_fog_scan, gt, **kw)
    fog = compare_meshes(fog_scan, gt, **kw)
    improvement = {k: getattr(fog.metrics, k) - getattr(no_fog.metrics, k) for k in IMPROVEMENT_KEYS}
    return DualComparisonReport(ground_truth_path=gt.path, no_fog_scan_path=no_fog.scan_path,
                                fog_scan_path=fog.scan_path, no_fog_report=no_fog, fog_report=fog,
                                improvement=improvement)


def report_to_dict(report: ComparisonReport) -> dict:
    """The reference's ``comparison_metrics.json`` as a dict: its keys in its order, tuples as lists."""
    metrics = asdict(report.metrics)
    metrics["bounding_box_ratio"] = list(metrics["bounding_box_ratio"])
    metrics["center_offset"] = list(metrics["center_offset"])
    return {"scan_path": str(report.scan_path), "ground_truth_path": str(report.ground_truth_path),
            "threshold": report.threshold, "metrics": metrics, "warnings": report.warnings, "errors": report.errors}


def write_metrics_json(report: ComparisonReport, path) -> None:
    path = Path(path)
    path.parent.mkdir(parents=True, exist_ok=True)
    with path.open("w") as f:
        json.dump(report_to_dict(report), f, indent=2)
