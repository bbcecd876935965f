"""The ground-truth comparison on the device (csrc/meshcompare.hip through mqr.compare_mesh_to_ground_truth)
against the reference's own reports (golden), the numpy restatement (compare_ref) and, for the ICP alignment,
tests/registration_ref.py.  Counts are exact; float fields use compare_ref's derived tolerances."""
from dataclasses import asdict

import numpy as np
import pytest

import compare_ref as cr
import registration_ref as rr
from test_compare_ref import CASES, golden, golden_case, golden_metrics, ref_report  # noqa: F401  (golden: fixture)
from test_gpu_mesh_quality import room  # noqa: F401  (fixture: the extracted room mesh, left in HBM)

pytestmark = pytest.mark.gpu


def report_dict(rep):
    d = asdict(rep.metrics)
    d["threshold"] = rep.threshold
    return d


@pytest.mark.parametrize("case", CASES)
def test_golden_cases(golden, case):
    from mqr.compare_mesh_to_ground_truth import compare_meshes
    sv, st, gv, gt, kw = golden_case(golden, case)
    _, tol = ref_report(golden, case)
    scan = sv if len(st) == 0 else (sv, st)
    cr.compare(report_dict(compare_meshes(scan, (gv, gt), **kw)), golden_metrics(golden, case), tol, case)


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 10001])
def test_distance_stats_against_numpy(n):
    from mqr.compare_mesh_to_ground_truth import distance_stats
    x = np.abs(np.random.default_rng(n).standard_normal(n)) * 0.3
    thr = float(x[n // 2])  # a value equal to the threshold is not counted
    got, want = distance_stats(x, thr), cr.distance_stats(x, thr)
    print(n, got, want)
    for k in ("min", "max", "median", "count_below", "count"):  # picked values and counts: exact
        assert got[k] == want[k], k
    assert want["count_below"] == int((x < thr).sum()) < n
    assert abs(got["mean"] - want["mean"]) <= cr.tolerance("mean_point_to_surface", n, want["mean"])
    assert abs(got["std"] - want["std"]) <= cr.tolerance("std_point_to_surface", n, 3 * want["max"])
    assert distance_stats(x, thr) == got  # a repeated call is bit-identical


def test_distance_stats_of_equal_values():
    from mqr.compare_mesh_to_ground_truth import distance_stats
    for n in (2, 1000):
        got = distance_stats(np.full(n, 0.125), 0.125)
        assert got == dict(mean=0.125, std=0.0, min=0.125, max=0.125, median=0.125, count_below=0, count=n)
    assert distance_stats(np.zeros(5), 1.0)["count_below"] == 5
    even = distance_stats(np.array([4.0, 1.0, 3.0, 2.0]), 0.0)
    odd = distance_stats(np.array([4.0, 1.0, 3.0]), 0.0)
    assert even["median"] == 2.5 and odd["median"] == 3.0


def test_measure_of_the_octahedron():
    from mqr.compare_mesh_to_ground_truth import measure_mesh
    v, t = cr.octahedron(3)
    m = measure_mesh((v, t))
    vol, vol_scale = cr.volume(v, t)
    area, area_scale = cr.surface_area(v, t)
    print(m.volume, vol, m.surface_area, area)
    assert m.is_closed_oriented and len(m.boundary) == 0 and (m.num_vertices, m.num_triangles) == (258, 512)
    assert 4.0 < vol < 4.19 and abs(m.volume - vol) <= cr.tolerance("volume_gt", len(t), vol_scale)
    assert abs(m.surface_area - area) <= cr.tolerance("surface_area_gt", len(t), area_scale)
    assert np.array_equal(m.min_bound, v.min(0).astype(np.float64)) and np.array_equal(m.max_bound, v.max(0))
    flipped = t.copy()
    flipped[100] = flipped[100, ::-1]
    f = measure_mesh((v, flipped))
    assert not f.is_closed_oriented and f.volume == 0.0 and cr.volume(v, flipped)[0] == 0.0
    assert f.surface_area == m.surface_area and len(f.boundary) == 0
    again = measure_mesh((v, t))
    assert (again.volume, again.surface_area) == (m.volume, m.surface_area)  # a repeated call is bit-identical


@pytest.mark.parametrize("nt", [1, 255, 257])
def test_strip_boundary_in_slot_order(nt):
    from mqr.compare_mesh_to_ground_truth import measure_mesh
    v, t = cr.strip(nt, seed=nt)
    t = t[np.random.default_rng(nt).permutation(nt)]  # slot order is then not vertex order
    m = measure_mesh((v, t))
    want = cr.boundary_edges(t)
    assert len(want) == nt + 2 and np.array_equal(m.boundary, want)
    area, scale = cr.surface_area(v, t)
    assert abs(m.surface_area - area) <= cr.tolerance("surface_area_scan", nt, scale)
    assert m.volume == 0.0 and not m.is_closed_oriented


def test_point_cloud_measure_and_errors():
    from mqr import _lib
    from mqr.compare_mesh_to_ground_truth import measure_mesh
    p = np.random.default_rng(1).uniform(-3, 5, (1000, 3)).astype(np.float32)
    m = measure_mesh(p)
    assert (m.surface_area, m.volume, len(m.boundary), m.num_triangles) == (0.0, 0.0, 0, 0)
    assert np.array_equal(m.min_bound, p.min(0)) and np.array_equal(m.max_bound, p.max(0))
    # a mesh in HBM cannot be checked with numpy: the device passes reject it before any gather
    from mqr.geometry import DeviceArray, Tensor, TriangleMesh
    v, t = cr.octahedron(1)
    bad = t.copy()
    bad[5, 2] = len(v)
    bv, bt = _lib.DeviceBuffer.from_array(v), _lib.DeviceBuffer.from_array(bad)
    mesh = TriangleMesh(Tensor(DeviceArray(bv, bv.ptr.value, v.shape, np.float32, 0)), np.zeros_like(v),
                        Tensor(DeviceArray(bt, bt.ptr.value, t.shape, np.int32, 0)), device="HIP:0")
    with pytest.raises(_lib.MqrError, match="outside"):
        measure_mesh(mesh)
    assert measure_mesh((v, t)).is_closed_oriented  # and the library is fine afterwards


@pytest.mark.parametrize("nq", [1, 65])
def test_nn_distances_do_not_depend_on_where_the_outputs_go(nq):
    """mqr_nn_query stages its outputs only when they go to the host, and the index array only when asked for
    (optional pieces of its scratch block): the distances are the same bits in all four cases, and so are the
    indices where there are any."""
    import ctypes
    from mqr import _lib
    from mqr._lib import MQR_DEVICE, MQR_HOST, call, ptr
    from mqr.compare_mesh_to_ground_truth import NearestNeighbour
    rng = np.random.default_rng(nq)
    targets = rng.uniform(-1, 1, (300, 3)).astype(np.float32)
    q = rng.uniform(-1.2, 1.2, (nq, 3)).astype(np.float32)
    want = np.sqrt(((q[:, None, :].astype(np.float64) - targets[None].astype(np.float64)) ** 2).sum(-1)).min(1)
    with NearestNeighbour(targets) as nn:
        got = {}
        for host_out in (True, False):
            for with_idx in (False, True):
                if host_out:
                    d, i = np.empty(nq, np.float64), np.empty(nq, np.int32)
                    call("mqr_nn_query", nn._h, ptr(q), nq, MQR_HOST, ptr(d), ptr(i) if with_idx else None, MQR_HOST)
                else:
                    bd, bi = _lib.DeviceBuffer(8 * nq), _lib.DeviceBuffer(4 * nq)
                    call("mqr_nn_query", nn._h, ptr(q), nq, MQR_HOST, bd.ptr, bi.ptr if with_idx else None, MQR_DEVICE)
                    d, i = bd.to_array((nq,), np.float64), bi.to_array((nq,), np.int32)
                got[host_out, with_idx] = (d, i if with_idx else None)
    first = got[True, True]
    assert np.abs(first[0] - want).max() <= 1e-5  # float32-level agreement guards the setup (exactness: test_golden_cases)
    for key, (d, i) in got.items():
        assert np.array_equal(d.view(np.uint64), first[0].view(np.uint64)), key
        if i is not None:
            assert np.array_equal(i, first[1]), key


CLOUD_SWEEP = """
import numpy as np
from mqr import _lib
from mqr.compare_mesh_to_ground_truth import measure_mesh
from mqr.geometry import DeviceArray, Tensor, TriangleMesh, device_mesh, mesh_fields
p = np.random.default_rng(0).uniform(-1, 1, (262000, 3)).astype(np.float32)
for nv in range(65300, 65500):  # host clouds: al256(12 nv) + al256(4 nv) + 2 KiB (8 slots), 1 MiB at nv = 65408
    m = measure_mesh(p[:nv])
    assert m.num_vertices == nv and np.array_equal(m.max_bound, p[:nv].max(0))
buf = _lib.DeviceBuffer.from_array(p)
for nv in range(261400, 262000, 3):  # clouds in HBM: al256(4 nv) + 2 KiB, 1 MiB at nv = 261632
    mesh = TriangleMesh(Tensor(DeviceArray(buf, buf.ptr.value, (nv, 3), np.float32, 0)), np.zeros((nv, 3), np.float32),
                        Tensor(DeviceArray(buf, 0, (0, 3), np.int32, 0)), device="HIP:0")
    assert device_mesh(mesh_fields(mesh)) is not None  # measured in place
    m = measure_mesh(mesh)
    assert m.num_vertices == nv and m.num_triangles == 0
print("swept")
"""


def test_cloud_sizes_whose_scratch_request_ends_on_a_block_boundary():
    """Scratch blocks are whole MiB.  A fresh process holds no larger cached block, so a call that takes more
    than it asked for fails exactly where the request ends within its last KiB: point clouds (no triangles)
    once did.  This test is about the fresh process, hence the child."""
    import os
    import subprocess
    import sys
    env = dict(os.environ, PYTHONPATH=os.pathsep.join(sys.path))
    r = subprocess.run([sys.executable, "-c", CLOUD_SWEEP], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "swept" in r.stdout, r.stderr[-2000:]


def test_public_metric_functions_agree_with_the_report(golden):
    """compare_meshes goes through private helpers; the functions under the reference's names must give its fields."""
    from mqr import compare_mesh_to_ground_truth as cm
    sv, st, gv, gt, kw = golden_case(golden, "holes")
    scan, gtm = (sv, st), (gv, gt)
    rep = cm.compare_meshes(scan, gtm, **kw)
    m = rep.metrics
    sp = cm.mesh_to_point_cloud(scan, kw["num_sample_points"], kw["seed"])
    gp = cm.mesh_to_point_cloud(gtm, kw["num_sample_points"], kw["seed"] + 1)
    chamfer, s2g, g2s = cm.compute_chamfer_distance(sp, gp)
    assert chamfer == m.chamfer_distance and len(s2g) == len(sp) and len(g2s) == len(gp)
    assert np.array_equal(s2g, cr.nearest(sp, gp)[0]) and np.array_equal(g2s, cr.nearest(gp, sp)[0])
    assert cm.compute_hausdorff_distance(sp, gp) == m.hausdorff_distance
    assert cm.compute_f_score(sp, gp, rep.threshold) == (m.precision, m.recall, m.f_score)
    assert m.precision != m.recall  # the two directions are not interchangeable here
    p2s = cm.distance_stats(cm.compute_point_to_surface_distance(sp, gtm))
    assert (p2s["mean"], p2s["median"], p2s["std"], p2s["max"]) == (
        m.mean_point_to_surface, m.median_point_to_surface, m.std_point_to_surface, m.max_point_to_surface)
    assert cm.compute_surface_area(scan) == m.surface_area_scan and cm.compute_surface_area(gtm) == m.surface_area_gt
    assert cm.count_holes(scan) == m.num_holes_scan == 2 and cm.count_holes(gtm) == 0
    assert cm.count_holes(scan, min_hole_size_ratio=1e-6) == 3  # the pinhole counts under a lower bar
    assert cm.compute_scale_and_alignment_metrics(scan, gtm) == (m.bounding_box_ratio, m.center_offset)
    assert cm.compute_volume_metrics(scan, gtm, seed=kw["seed"]) == (m.volume_scan, m.volume_gt, m.volume_overlap,
                                                                       m.volume_iou)
    # a closed scan: volumes reported, and the overlap samples are seed + 2 and seed + 3
    ident = cm.compare_meshes(gtm, gtm, **golden_case(golden, "identical")[4]).metrics
    vols = cm.compute_volume_metrics(gtm, gtm, seed=0)
    assert vols == (ident.volume_scan, ident.volume_gt, ident.volume_overlap, ident.volume_iou) and vols[0] > 4.0
    ratio = np.mean(cr.nearest(cr.sample(gv, gt, 10000, 2), cr.sample(gv, gt, 10000, 3))[0] < 0.01)
    assert 0.0 < ratio < 1.0 and vols[2] == vols[0] * ratio
    assert cm.compute_volume_metrics(gtm, gtm, seed=5)[2] != vols[2]


def test_room_mesh_in_hbm_equals_its_host_copy(room):
    from mqr.compare_mesh_to_ground_truth import compare_meshes
    from mqr.geometry import device_ptr
    assert device_ptr(room.vertex.positions) is not None  # measured and searched in place
    on_device = compare_meshes(room, room, num_sample_points=4000)
    host = room.cpu()
    assert device_ptr(host.vertex.positions) is None
    on_host = compare_meshes((host.vertices, host.triangles), host, num_sample_points=4000)
    assert report_dict(on_device) == report_dict(on_host)
    m = on_device.metrics
    assert m.bounding_box_ratio == (1.0, 1.0, 1.0) and m.center_offset == (0.0, 0.0, 0.0)
    assert m.surface_area_scan == m.surface_area_gt > 1.0 and m.num_holes_scan == m.num_holes_gt
    assert m.num_scan_points == 4000 and 0.0 < m.chamfer_distance < 0.2


def test_ply_paths(golden, tmp_path):
    from mqr.compare_mesh_to_ground_truth import compare_meshes, write_metrics_json
    from mqr.geometry import _write_ply
    sv, st, gv, gt, kw = golden_case(golden, "noisy_auto")
    _write_ply(tmp_path / "scan.ply", sv, None, st)
    _write_ply(tmp_path / "gt.ply", gv, None, gt)
    rep = compare_meshes(tmp_path / "scan.ply", str(tmp_path / "gt.ply"), **kw)
    assert rep.scan_path == tmp_path / "scan.ply" and rep.ground_truth_path == tmp_path / "gt.ply"
    assert report_dict(rep) == report_dict(compare_meshes((sv, st), (gv, gt), **kw))
    write_metrics_json(rep, tmp_path / "out" / "comparison_metrics.json")
    import json
    d = json.loads((tmp_path / "out" / "comparison_metrics.json").read_text())
    assert d["metrics"]["chamfer_distance"] == rep.metrics.chamfer_distance and d["threshold"] == rep.threshold


def test_icp_alignment(golden):
    """The noisy scan rotated by 3 degrees and shifted by 2 cm: the transform against registration_ref's ICP
    within the registration tests' 1e-9, the metrics within the aligned tolerance."""
    from mqr.compare_mesh_to_ground_truth import align_point_clouds, compare_meshes
    sv, st, gv, gt, kw = golden_case(golden, "noisy_auto")
    M = rr.motion(3.0, 0.0, 0.0, (0.02, 0.0, 0.0))
    sv = rr.apply(M, sv)
    kw["align_method"] = "icp"
    seen = {}

    def icp(src, tgt):
        seen["T"] = rr.icp(src, tgt, [-1.0], [0.1], [50], [1e-6], [1e-6])["transformation"]
        return seen["T"]

    want, tol = cr.report(sv, st, gv, gt, icp=icp, icp_tol=1e-9, **kw)
    sp, gp = cr.sample(sv, st, kw["num_sample_points"], kw["seed"]), cr.sample(gv, gt, kw["num_sample_points"], kw["seed"] + 1)
    aligned, T = align_point_clouds(sp, gp, "icp")
    shift = np.eye(4)
    shift[:3, 3] = gp.astype(np.float64).mean(0) - sp.astype(np.float64).mean(0)
    err = np.abs(T - seen["T"] @ shift).max()
    print("icp transform |diff|", err)
    assert err <= 1e-9
    assert np.abs(aligned - (sp.astype(np.float64) @ T[:3, :3].T + T[:3, 3])).max() < 1e-12
    cr.compare(report_dict(compare_meshes((sv, st), (gv, gt), **kw)), want, tol, "icp")


def test_dual_scans_improvement_signs(golden):
    from mqr.compare_mesh_to_ground_truth import IMPROVEMENT_KEYS, compare_dual_scans
    gv, gt = golden["gt_vertices"], golden["gt_triangles"]
    rng = np.random.default_rng(8)
    fog = (gv + 0.002 * rng.standard_normal(gv.shape)).astype(np.float32), gt
    no_fog = (gv + 0.03 * rng.standard_normal(gv.shape)).astype(np.float32), gt[40:]  # noisier, and torn open
    dual = compare_dual_scans(no_fog, fog, (gv, gt), num_sample_points=2000)
    imp, a, b = dual.improvement, dual.no_fog_report.metrics, dual.fog_report.metrics
    assert tuple(imp) == IMPROVEMENT_KEYS == ("chamfer_distance", "hausdorff_distance", "mean_point_to_surface",
                                              "median_point_to_surface", "max_point_to_surface", "f_score",
                                              "precision", "recall", "surface_area_scan", "num_holes_scan")
    for k in IMPROVEMENT_KEYS:
        assert imp[k] == getattr(b, k) - getattr(a, k), k
    assert imp["chamfer_distance"] < 0 and imp["mean_point_to_surface"] < 0 and imp["hausdorff_distance"] < 0
    assert imp["f_score"] > 0 and imp["precision"] > 0 and imp["recall"] > 0
    assert imp["surface_area_scan"] != 0 and imp["num_holes_scan"] < 0 and b.num_holes_scan == 0
    assert b.volume_scan > 0 and a.volume_scan == 0.0
