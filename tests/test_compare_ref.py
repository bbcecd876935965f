"""The numpy restatement of the ground-truth comparison (compare_ref) against the reference's own reports
(tests/golden/compare_golden.npz, made by tests/golden/make_compare_golden.py), and the host pieces of
mqr.compare_mesh_to_ground_truth that need no GPU: the sampler and the hole walk."""
import os
from dataclasses import fields

import numpy as np
import pytest

import compare_ref as cr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "compare_golden.npz")
CASES = ("identical", "noisy_explicit", "noisy_auto", "holes", "touching", "degenerate", "cloud", "center", "scale")


@pytest.fixture(scope="session")
def golden():
    with np.load(GOLDEN) as z:
        g = {k: z[k] for k in z.files}
    for a in g.values():
        a.setflags(write=False)
    return g


def golden_case(g, case):
    """(scan vertices, scan triangles, GT vertices, GT triangles, keyword arguments of compare_meshes)."""
    thr = float(g[case + "_threshold"])
    kw = dict(threshold=None if np.isnan(thr) else thr, num_sample_points=int(g[case + "_num_sample_points"]),
              align_method=str(g[case + "_align_method"]), scale_normalize=bool(g[case + "_scale_normalize"]),
              seed=int(g[case + "_seed"]))
    return g[case + "_vertices"], g[case + "_triangles"], g["gt_vertices"], g["gt_triangles"], kw


def golden_metrics(g, case):
    flat, out, i = g[case + "_metrics"], {}, 0
    for f in cr.FIELDS:
        if f in ("bounding_box_ratio", "center_offset"):
            out[f] = tuple(flat[i:i + 3])
            i += 3
        else:
            out[f] = flat[i]
            i += 1
    assert i == len(flat)
    out["threshold"] = float(g[case + "_threshold_used"])
    return out


_REPORTS = {}


def ref_report(g, case):
    """The restatement's report of a golden case, computed once per session (the device tests share it)."""
    if case not in _REPORTS:
        sv, st, gv, gt, kw = golden_case(g, case)
        _REPORTS[case] = cr.report(sv, st, gv, gt, **kw)
    return _REPORTS[case]


@pytest.mark.parametrize("case", CASES)
def test_restatement_matches_the_reference(golden, case):
    assert list(golden["cases"]) == list(CASES) and tuple(golden["fields"]) == cr.FIELDS
    got, tol = ref_report(golden, case)
    cr.compare(got, golden_metrics(golden, case), tol, case)


def test_golden_pins_every_branch(golden):
    m = {c: golden_metrics(golden, c) for c in CASES}
    assert m["identical"]["volume_scan"] == m["identical"]["volume_gt"] > 4.0  # reported (a sphere's is 4.19)
    assert m["identical"]["bounding_box_ratio"] == (1.0, 1.0, 1.0) and m["identical"]["center_offset"] == (0, 0, 0)
    assert m["noisy_auto"]["volume_scan"] == 0.0 and m["noisy_auto"]["volume_iou"] == 0.0  # open: not reported
    assert m["noisy_auto"]["num_holes_scan"] == 1  # the rim
    assert m["holes"]["num_holes_scan"] == 2  # rim and block; the pinhole is below the bar
    sv, st = golden["holes_vertices"], golden["holes_triangles"]
    _, per, bar = cr.count_holes(sv, st)
    assert len(per) == 3 and sorted(p >= bar for p in per) == [False, True, True]
    assert m["touching"]["num_holes_scan"] >= 2
    assert m["cloud"]["surface_area_scan"] == 0.0 and m["cloud"]["num_holes_scan"] == 0
    assert m["cloud"]["num_scan_points"] == 500 and len(golden["cloud_vertices"]) == 700
    assert m["noisy_explicit"]["threshold"] == 0.05 != m["noisy_auto"]["threshold"]
    assert m["noisy_explicit"]["precision"] != m["noisy_auto"]["precision"]
    assert m["center"]["chamfer_distance"] != m["scale"]["chamfer_distance"]
    keys, mult, _ = cr.edge_runs(golden["degenerate_triangles"])
    assert 3 in mult.values() and (3, 3) in mult
    assert all(m[c]["num_holes_gt"] == 0 for c in CASES)


def test_touching_holes_share_a_vertex_of_degree_four(golden):
    """The shared vertex has four boundary neighbours: which way a walk leaves it decides the loops, and the
    module's walk leaves it the way the restatement's does."""
    from mqr.compare_mesh_to_ground_truth import hole_perimeters
    sv, st = golden["touching_vertices"], golden["touching_triangles"]
    b = cr.boundary_edges(st)
    assert np.bincount(b.reshape(-1)).max() == 4
    per = cr.hole_perimeters(b, sv)
    assert len(per) >= 2 and hole_perimeters(b, sv) == per


# ---------------------------------------------------------------------------- the module's host pieces
def test_dataclasses_mirror_the_reference_order():
    from mqr import compare_mesh_to_ground_truth as cm
    assert tuple(f.name for f in fields(cm.ComparisonMetrics)) == cr.FIELDS
    assert [f.name for f in fields(cm.ComparisonReport)] == ["scan_path", "ground_truth_path", "metrics", "threshold",
                                                             "warnings", "errors"]
    assert [f.name for f in fields(cm.DualComparisonReport)] == ["ground_truth_path", "no_fog_scan_path",
                                                                 "fog_scan_path", "no_fog_report", "fog_report",
                                                                 "improvement"]
    import mqr
    assert mqr.compare_mesh_to_ground_truth is cm


def test_report_to_dict_has_the_reference_keys():
    from mqr import compare_mesh_to_ground_truth as cm
    vals = {f.name: (1.0, 2.0, 3.0) if f.name in ("bounding_box_ratio", "center_offset") else 1 for f in
            fields(cm.ComparisonMetrics)}
    rep = cm.ComparisonReport(None, None, cm.ComparisonMetrics(**vals), 0.5, [], [])
    d = cm.report_to_dict(rep)
    assert list(d) == ["scan_path", "ground_truth_path", "threshold", "metrics", "warnings", "errors"]
    assert tuple(d["metrics"]) == cr.FIELDS and d["metrics"]["center_offset"] == [1.0, 2.0, 3.0]


def test_sampler_is_deterministic_and_equals_the_restatement(golden):
    from mqr.compare_mesh_to_ground_truth import mesh_to_point_cloud
    v, t = golden["holes_vertices"], golden["holes_triangles"]
    a, b = mesh_to_point_cloud((v, t), 777, seed=5), mesh_to_point_cloud((v, t), 777, seed=5)
    assert a.dtype == np.float32 and a.shape == (777, 3) and np.array_equal(a, b)
    assert np.array_equal(a, cr.sample(v, t, 777, 5))
    assert not np.array_equal(a, mesh_to_point_cloud((v, t), 777, seed=6))
    assert np.array_equal(mesh_to_point_cloud((v, t)), v)  # num_points None: the vertices
    c = golden["cloud_vertices"]
    none = np.zeros((0, 3), np.int32)
    assert np.array_equal(mesh_to_point_cloud((c, none), 700), c)  # no triangles, few enough: all vertices
    pick = mesh_to_point_cloud((c, none), 100, seed=3)
    assert np.array_equal(pick, cr.sample(c, none, 100, 3)) and len(np.unique(pick, axis=0)) == 100


def test_sampled_points_lie_inside_their_triangles(golden):
    from mqr.compare_mesh_to_ground_truth import _sample_triangles
    v, t = golden["gt_vertices"], golden["gt_triangles"]
    p, k = _sample_triangles(v, t, 2000, seed=1)
    a, b, c = (v[t[k, j]].astype(np.float64) for j in range(3))
    # barycentric coordinates by least squares on the triangle's plane
    e0, e1, d = b - a, c - a, p - a
    d00, d01, d11 = (e0 * e0).sum(1), (e0 * e1).sum(1), (e1 * e1).sum(1)
    d20, d21 = (d * e0).sum(1), (d * e1).sum(1)
    den = d00 * d11 - d01 * d01
    w1, w2 = (d11 * d20 - d01 * d21) / den, (d00 * d21 - d01 * d20) / den
    assert (w1 >= -1e-9).all() and (w2 >= -1e-9).all() and (w1 + w2 <= 1 + 1e-9).all()
    assert np.abs(a + w1[:, None] * e0 + w2[:, None] * e1 - p).max() < 1e-12  # and in its plane


def test_sampler_area_shares():
    from mqr.compare_mesh_to_ground_truth import _sample_triangles
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [10, 0, 0], [13, 0, 0], [10, 2, 0]], np.float32)
    t = np.array([[0, 1, 2], [3, 4, 5]], np.int32)  # areas 0.5 and 3
    n = 20000
    _, k = _sample_triangles(v, t, n, seed=9)
    share = 0.5 / 3.5
    sigma = np.sqrt(n * share * (1 - share))
    assert abs(int((k == 0).sum()) - n * share) <= 4 * sigma


def test_hole_walk_on_hand_made_boundaries():
    from mqr.compare_mesh_to_ground_truth import hole_perimeters
    sq = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [2, 0, 0], [2, 1, 0], [3, 0, 0]], np.float64)
    for walk in (hole_perimeters, cr.hole_perimeters):
        assert walk(np.zeros((0, 2), np.int32), sq) == []
        assert walk([(0, 1), (1, 2), (2, 3), (0, 3)], sq) == [4.0]  # one square
        assert walk([(0, 1), (1, 2)], sq) == []  # an open chain closes nothing
        assert walk([(0, 1), (0, 1)], sq) == []  # back at the start after two edges: not a hole
        # a triangle and a separate open chain
        assert walk([(0, 1), (1, 3), (0, 3), (4, 5), (5, 6)], sq) == [2.0 + np.sqrt(2.0)]
        # two triangles, (0, 1, 3) and (1, 4, 2), that touch in vertex 1: the order of vertex 1's neighbours decides.
        # Listed triangle by triangle, the walk from 0 comes back through 3 and closes each triangle on its own;
        tri = 2.0 + np.sqrt(2.0)
        assert walk([(0, 1), (1, 3), (0, 3), (1, 4), (2, 4), (1, 2)], sq) == pytest.approx([tri, tri])
        # with (1, 4) listed before (1, 3), the walk from 0 turns into the second triangle at vertex 1 and
        # closes one loop of six edges around both
        assert walk([(0, 1), (1, 4), (1, 3), (0, 3), (2, 4), (1, 2)], sq) == pytest.approx([2 * tri])


def test_normalize_scale_and_center_alignment():
    from mqr.compare_mesh_to_ground_truth import align_point_clouds, normalize_scale
    rng = np.random.default_rng(3)
    p, ref = rng.uniform(-1, 2, (500, 3)), rng.uniform(0, 5, (400, 3))
    same, one = normalize_scale(p)
    assert one == 1.0 and np.array_equal(same, p)
    diag = float(np.linalg.norm(p.max(0) - p.min(0)))
    q, f = normalize_scale(p, target_scale=2.5)
    assert f == 2.5 / diag and abs(np.linalg.norm(q.max(0) - q.min(0)) - 2.5) < 1e-12
    assert np.abs((q.min(0) + q.max(0)) - (p.min(0) + p.max(0))).max() < 1e-12  # about the box centre
    r, g = normalize_scale(p, reference_pcd=ref)
    r2, g2 = normalize_scale(p, target_scale=float(np.linalg.norm(ref.max(0) - ref.min(0))))
    assert g == g2 and np.array_equal(r, r2)
    assert normalize_scale(np.zeros((4, 3)), target_scale=1.0)[1] == 1.0  # zero extent: unchanged
    a, T = align_point_clouds(p, ref, "center")
    assert np.abs(a.mean(0) - ref.mean(0)).max() < 1e-12 and np.array_equal(T[:3, :3], np.eye(3))
    assert np.array_equal(a, p + T[:3, 3])
    a, T = align_point_clouds(p, ref, "none")
    assert np.array_equal(a, p) and np.array_equal(T, np.eye(4))
    with pytest.raises(ValueError):
        align_point_clouds(p, ref, "nearest")


def test_zero_extent_ground_truth_needs_an_explicit_threshold(monkeypatch):
    from mqr import compare_mesh_to_ground_truth as cm
    flat = cm.MeshMeasure(0.0, 0.0, np.zeros(3), np.zeros(3), False, np.zeros((0, 2), np.int32), 3, 0)
    monkeypatch.setattr(cm, "measure_mesh", lambda mesh, device=0: flat)
    p = np.zeros((3, 3), np.float32)
    with pytest.raises(ValueError, match="zero extent"):
        cm.compare_meshes(p, p, num_sample_points=3)


def test_host_meshes_are_checked_before_any_library_call(monkeypatch):
    from mqr import _lib
    from mqr import compare_mesh_to_ground_truth as cm

    def no_call(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(cm, "call", no_call)
    monkeypatch.setattr(_lib, "call", no_call)
    v, t = cr.octahedron(1)
    bad = t.copy()
    bad[3, 1] = len(v)
    with pytest.raises(ValueError, match="outside"):
        cm.measure_mesh((v, bad))
    nan = v.copy()
    nan[2, 0] = np.nan
    with pytest.raises(ValueError, match="finite"):
        cm.compare_meshes((nan, t), (v, t))
    with pytest.raises(ValueError, match="finite"):
        cm.point_cloud_distance(nan, v)
    with pytest.raises(ValueError):
        cm.measure_mesh((np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)))


def test_c_entry_points_reject_bad_sizes_before_touching_a_device():
    import ctypes
    from mqr import _lib
    L = _lib.load()
    h, one = ctypes.c_void_p(), np.zeros(3, np.float32)
    assert L.mqr_nn_create(0, _lib.ptr(one), 0, _lib.MQR_HOST, ctypes.byref(h)) == 2 and not h.value
    assert b"empty" in L.mqr_last_error()
    assert L.mqr_nn_create(0, _lib.ptr(one), 2 ** 31, _lib.MQR_HOST, ctypes.byref(h)) == 2
    assert b"2^31" in L.mqr_last_error()
    out = (ctypes.c_double * 16)()
    assert L.mqr_distance_stats(0, _lib.ptr(one), 0, _lib.MQR_HOST, 0.0, out) == 2
    assert L.mqr_distance_stats(0, _lib.ptr(one), 2 ** 31, _lib.MQR_HOST, 0.0, out) == 2
    assert L.mqr_mesh_measure(0, _lib.ptr(one), 0, None, 0, _lib.MQR_HOST, out, None) == 2
    assert L.mqr_mesh_measure(0, _lib.ptr(one), 1, _lib.ptr(one), 2 ** 31 // 3, _lib.MQR_HOST, out, None) == 2
    assert L.mqr_nn_destroy(None) == 0 and L.mqr_edge_list_free(None) == 0
