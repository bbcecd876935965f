"""Fragment registration on the device (csrc/registration.hip through mqr.registration and
mqr.fragments) against the CPU restatement of the same rules (tests/registration_ref.py).

The comparisons are exact where the rules make them exact (voxel down-sample rows, inlier counts,
fitness, iteration counts, batch == single == repeat) and 1e-9 where only the summation order and the
3x3 solver differ (the reference's own summation-order noise is ~1e-14, test_registration_ref.py).
The margins test_registration_ref.py asserts (no tie and no distance within 1e-9 of the radius) are
what makes the exact part meaningful."""
import numpy as np
import pytest

import registration_ref as ref

pytestmark = pytest.mark.gpu

LEVELS = dict(voxel_sizes=[0.05, 0.025, 0.0125], max_dists=[0.1, 0.05, 0.025], max_iters=[50, 31, 14],
              rel_fitness=[1e-6] * 3, rel_rmse=[1e-6] * 3)


def _criteria(levels=LEVELS):
    from mqr.registration import ICPConvergenceCriteria
    return [ICPConvergenceCriteria(f, r, i)
            for f, r, i in zip(levels["rel_fitness"], levels["rel_rmse"], levels["max_iters"])]


def _cloud(n, seed, T=None):
    p = ref.surface(n + 3, seed)[:n]
    return p if T is None else ref.apply(T, p)


@pytest.fixture(scope="module")
def pair():
    src, tgt, T_true = ref.icp_pair()
    r = ref.icp(src, tgt, **LEVELS)
    for a in (src, tgt):
        a.setflags(write=False)
    return src, tgt, T_true, r


@pytest.fixture(scope="module")
def pair_set(pair):
    from mqr.registration import CloudSet
    cs = CloudSet([pair[0], pair[1]])
    yield cs
    cs.close()


def _planted_cloud():
    base = ref.surface(2100, 3)  # 2100 points, both signs
    rng = np.random.default_rng(5)
    dense = (np.array([0.30, -0.45, 0.10]) + rng.uniform(0.001, 0.049, (300, 3))).astype(np.float32)
    # on the faces of both voxel sizes (as far as float32 holds them), both signs, and the origin
    vals = np.array([0.0, 0.05, -0.05, 0.1, -0.1, 0.25, -0.25, 0.0125, -0.0125, -0.5], np.float32)
    grid = np.stack(np.meshgrid(vals, vals, vals[:2], indexing="ij"), -1).reshape(-1, 3)[:101]
    p = np.concatenate([base, dense, grid]).astype(np.float32)
    p = p[np.random.default_rng(6).permutation(len(p))]
    assert len(p) == 2501
    return np.ascontiguousarray(p)


@pytest.mark.parametrize("v", [0.05, 0.0125])
def test_voxel_down_sample_is_bit_exact(v):
    from mqr.geometry import PointCloud
    from mqr.registration import CloudSet
    p = _planted_cloud()
    exp = ref.voxel_down(p, v)
    key = np.floor(p.astype(np.float64) / v).astype(np.int64)
    assert np.unique(key, axis=0, return_counts=True)[1].max() >= (300 if v == 0.05 else 2)
    cs = CloudSet([p])
    got = cs.voxel_down_sample(0, v)
    again = cs.voxel_down_sample(0, v)
    cs.close()
    assert got.dtype == np.float32 and got.shape == exp.shape
    assert np.array_equal(got.view(np.uint32), exp.view(np.uint32))
    assert np.array_equal(got, again)
    pc = PointCloud(p, np.zeros_like(p)).voxel_down_sample(v)
    assert np.array_equal(pc.points, exp)
    assert np.array_equal(PointCloud(p, np.zeros_like(p)).uniform_down_sample(30).points, p[::30])


@pytest.mark.parametrize("every_k", [1, 30])
@pytest.mark.parametrize("at", ["identity", "true"])
def test_evaluate_registration_matches_reference(pair, pair_set, every_k, at):
    src, tgt, T_true, _ = pair
    T = np.eye(4) if at == "identity" else T_true
    exp = ref.evaluate(src, tgt, 0.1, T, every_k)
    got = pair_set.evaluate_pairs([0], [1], 0.1, T, every_k=every_k)[0]
    print("count", got.correspondences, exp["count"], "rmse", got.inlier_rmse, exp["inlier_rmse"])
    assert got.correspondences == exp["count"] and exp["count"] > 0
    assert got.fitness == exp["fitness"]
    assert abs(got.inlier_rmse - exp["inlier_rmse"]) <= 1e-12 * exp["inlier_rmse"]
    if every_k == 1:
        from mqr.registration import evaluate_registration
        one = evaluate_registration(src, tgt, 0.1, T)
        assert (one.fitness, one.inlier_rmse) == (got.fitness, got.inlier_rmse)


def test_multi_scale_icp_matches_reference(pair, pair_set):
    from mqr.registration import multi_scale_icp
    src, tgt, T_true, r = pair
    got = multi_scale_icp(src, tgt, LEVELS["voxel_sizes"], _criteria(), LEVELS["max_dists"], np.eye(4))
    dT = float(np.abs(got.transformation - r["transformation"]).max())
    print("iterations", got.num_iterations, r["num_iterations"], "max |T - T_ref|", dT, "fitness", got.fitness,
          r["fitness"], "rmse", got.inlier_rmse, r["inlier_rmse"])
    assert got.num_iterations == r["num_iterations"]
    assert got.fitness == r["fitness"]  # = inliers / points of the last pass: equal counts
    # inlier counts of the full clouds under each result, at every level's radius
    for radius in LEVELS["max_dists"]:
        a = pair_set.evaluate_pairs([0], [1], radius, got.transformation)[0].correspondences
        assert a == ref.evaluate(src, tgt, radius, r["transformation"])["count"]
    assert abs(got.inlier_rmse - r["inlier_rmse"]) <= 1e-9
    assert dT <= 1e-9
    assert np.array_equal(got.transformation[3], [0, 0, 0, 1])
    assert float(np.abs(got.transformation - T_true).max()) < 5e-3


def test_information_matrix_matches_reference(pair, pair_set):
    from mqr.registration import get_information_matrix
    src, tgt, _, r = pair
    T = r["transformation"]
    exp = ref.information(src, tgt, 0.025, T)
    got = get_information_matrix(src, tgt, 0.025, T)
    assert got.shape == (6, 6) and np.array_equal(got, got.T)
    rel = float(np.abs(got - exp).max() / np.abs(exp).max())
    print("information max rel diff", rel, "count", got[3, 3], exp[3, 3])
    assert got[3, 3] == exp[3, 3] == got[4, 4] == got[5, 5]
    assert rel <= 1e-9
    assert np.array_equal(pair_set.information_pairs([0], [1], 0.025, T)[0], got)


def test_batch_equals_single_pair_calls_and_repeats():
    import itertools
    from mqr.registration import CloudSet
    sizes = [1000, 2501, 4096, 6000, 64]
    clouds = [_cloud(n, 10 + i, ref.motion(0.4 * i, -0.3 * i, 0.5 * i, (0.004 * i, -0.003 * i, 0.002 * i)))
              for i, n in enumerate(sizes)]
    assert [len(c) for c in clouds] == sizes
    pairs = list(itertools.combinations(range(5), 2))
    s, t = [a for a, _ in pairs], [b for _, b in pairs]
    cs = CloudSet(clouds)

    def run(src, tgt):
        ev = cs.evaluate_pairs(src, tgt, 0.1, np.eye(4), every_k=7)
        icp = cs.icp_pairs(src, tgt, LEVELS["voxel_sizes"], _criteria(), LEVELS["max_dists"], np.eye(4))
        info = cs.information_pairs(src, tgt, 0.025, np.stack([r.transformation for r in icp]))
        return ([(r.fitness, r.inlier_rmse, r.correspondences) for r in ev],
                [(r.transformation.tobytes(), r.fitness, r.inlier_rmse, tuple(r.num_iterations)) for r in icp],
                [m.tobytes() for m in info])

    batch = run(s, t)
    again = run(s, t)
    assert batch == again
    for i, (a, b) in enumerate(pairs):
        one = run([a], [b])
        assert (one[0][0], one[1][0], one[2][0]) == (batch[0][i], batch[1][i], batch[2][i]), (a, b)
    cs.close()
    assert any(f > 0.3 for f, _, _ in batch[0])  # the batch did register something


def test_degenerate_pairs_give_clean_results():
    from mqr._lib import MqrError
    from mqr.fragments import FragmentPoseRefinementConfig, compute_pcd_pair_edge
    from mqr.registration import CloudSet
    a = _cloud(3000, 21)
    far = (a + np.float32(5.0)).astype(np.float32)
    two = np.ascontiguousarray(a[:2])
    T0 = ref.motion(1.0, 2.0, 3.0, (0.01, 0.02, 0.03))
    cs = CloudSet([a, far, two])
    for s, t in ((0, 1), (2, 0)):
        r = cs.icp_pairs([s], [t], LEVELS["voxel_sizes"], _criteria(), LEVELS["max_dists"], T0)[0]
        assert r.num_iterations == [1, 1, 1]
        assert np.array_equal(r.transformation, T0)
        assert np.isfinite([r.fitness, r.inlier_rmse]).all()
        info = cs.information_pairs([s], [t], 0.025, T0)[0]
        assert np.isfinite(info).all()
    r = cs.icp_pairs([0], [1], LEVELS["voxel_sizes"], _criteria(), LEVELS["max_dists"], T0)[0]
    assert (r.fitness, r.inlier_rmse) == (0.0, 0.0)
    e = cs.evaluate_pairs([0], [1], 0.1, np.eye(4))[0]
    assert (e.fitness, e.inlier_rmse, e.correspondences) == (0.0, 0.0, 0)
    assert not cs.information_pairs([0], [1], 0.025, np.eye(4)).any()
    with pytest.raises(MqrError, match="out of range"):
        cs.evaluate_pairs([0], [3], 0.1, np.eye(4))
    cs.close()
    assert compute_pcd_pair_edge([a, far], 0, 1, FragmentPoseRefinementConfig(), True) is None
    assert compute_pcd_pair_edge([a, far], 0, 1, FragmentPoseRefinementConfig(), False) is not None
    with pytest.raises(MqrError, match="empty"):
        CloudSet([a, np.zeros((0, 3), np.float32)])
    bad = a.copy()
    bad[17, 1] = np.nan
    with pytest.raises(MqrError, match="non-finite"):
        CloudSet([bad, a])
    huge = a.copy()
    huge[5, 0] = 1e6
    cs = CloudSet([huge, a])
    with pytest.raises(MqrError, match="cell index"):
        cs.voxel_down_sample(0, 0.0125)
    cs.close()


def test_pose_graph_from_the_fragment_path(tmp_path, capsys):
    from mqr import _lib, synthetic
    from mqr.dataio import DepthDataIO
    from mqr.fragments import (FragmentPoseRefinementConfig, build_pose_graph_for_scene, fragment_datasets,
                               integrate_fragment_point_clouds)
    from mqr.geometry import DeviceArray, PointCloud, Tensor
    from mqr.models import CoordinateSystem, Side
    _lib.load()
    seq = synthetic.make_sequence("room", n=120, height=240, width=320, f=262.5, noise=True, seed=17)
    synthetic.write_capture(tmp_path, seq)
    io = DepthDataIO(tmp_path)
    ds = io.load_depth_dataset(Side.LEFT)
    ds.transforms = ds.transforms.convert_coordinate_system(target_coordinate_system=CoordinateSystem.OPEN3D,
                                                            is_camera=True)
    frags = fragment_datasets(ds, 30)
    assert len(frags) == 4
    cfg = FragmentPoseRefinementConfig(device="CUDA:0", use_confidence_filtered_depth=False, voxel_size=0.02,
                                       block_count=20_000, depth_max=4.0, trunc_voxel_multiplier=8.0,
                                       pre_filter_every_k_points=POSE_GRAPH_EVERY_K,
                                       max_iterations=[20, 10, 5])
    res = integrate_fragment_point_clouds(io, {Side.LEFT: frags}, cfg, keep_on_device=True)
    assert all(r is not None and r[1].point.positions.is_cuda for r in res)
    clouds = [r[1] for r in res]
    host = [c.point.positions.device_array().host() for c in clouds]
    # two fragments moved by a known small motion (uploaded again: they stay in HBM like the others)
    moves = {1: ref.motion(0.8, -0.5, 0.6, (0.012, -0.008, 0.01)), 3: ref.motion(-0.6, 0.7, -0.4, (-0.01, 0.006, 0.009))}
    for i, M in moves.items():
        host[i] = ref.apply(M, host[i])
        buf = _lib.DeviceBuffer.from_array(host[i])
        clouds[i] = PointCloud(Tensor(DeviceArray(buf, buf.ptr.value, host[i].shape, np.float32, 0)),
                               np.zeros((0, 3), np.float32))
    stats = {}
    graph, nodes = build_pose_graph_for_scene({Side.LEFT: clouds}, cfg, stats=stats)
    out = capsys.readouterr().out
    exp_edges, why = ref.pose_graph({Side.LEFT: host}, cfg)
    print("points", [len(h) for h in host], "decisions", why, "stats", stats)
    assert nodes == [(Side.LEFT, i) for i in range(4)] and len(graph.nodes) == 4
    assert f"[Info] Valid edges: {len(exp_edges)} / 9" in out
    loop = why[3:]
    assert loop.count("kept") >= 1 and len(loop) - loop.count("kept") >= 1
    assert why[:3] == ["kept"] * 3
    assert [(e.source_node_id, e.target_node_id, e.uncertain) for e in graph.edges] == \
        [(e["source_node_id"], e["target_node_id"], e["uncertain"]) for e in exp_edges]
    assert stats["icp_pairs"] == 9 - why.count("pre_filter") and stats["information_pairs"] == len(exp_edges)
    for e, x in zip(graph.edges, exp_edges):
        d = float(np.abs(e.transformation - x["transformation"]).max())
        rel = float(np.abs(e.information - x["information"]).max() / np.abs(x["information"]).max())
        print((e.source_node_id, e.target_node_id), "max |T - T_ref|", d, "information rel", rel)
        assert d <= 1e-9 and rel <= 1e-9 and e.confidence == 1.0
    # (for the record: how close the odometry edges of the moved fragments come to the planted motion)
    print("odometry 0->1 vs planted", float(np.abs(graph.edges[0].transformation - moves[1]).max()),
          "2->3 vs planted", float(np.abs(graph.edges[2].transformation - moves[3]).max()))


# Every POSE_GRAPH_EVERY_K-th point for the pre-filter of the pose-graph test: chosen so that, on these
# four fragments, the reference keeps some loop closures and rejects others (asserted in the test).
POSE_GRAPH_EVERY_K = 30
