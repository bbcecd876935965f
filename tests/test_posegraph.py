"""The host pose-graph optimiser (mqr.posegraph, DESIGN "pose-graph rules"): the pose vector, a
consistent loop graph left alone, a drifted one recovered, a planted false loop closure pruned."""
import numpy as np
import pytest

from mqr.posegraph import (GlobalOptimizationConvergenceCriteria, GlobalOptimizationLevenbergMarquardt,
                           GlobalOptimizationOption, PoseGraph, PoseGraphEdge, PoseGraphNode, global_optimization,
                           mat4, vec6)

N = 12
LOOPS = [(0, 11), (0, 6), (2, 8), (3, 10)]
PRUNE = 0.25


def _truth():
    a = 2 * np.pi * np.arange(N) / N
    return mat4(np.stack([0.1 * np.sin(a), 0.9 * a, 0.05 * np.cos(a), np.cos(a), 0.1 * np.sin(2 * a), np.sin(a)], 1))


GT = _truth()
GT.setflags(write=False)


def _exact(i, j):
    return np.linalg.inv(GT[j]) @ GT[i]


def _graph(poses, extra=()):
    """12 nodes on a loop: exact odometry edges (certain) and exact loop edges (uncertain); the
    information is a count-scaled identity."""
    g = PoseGraph(nodes=[PoseGraphNode(np.array(p)) for p in poses])
    g.edges += [PoseGraphEdge(i, i + 1, _exact(i, i + 1), 4000.0 * np.eye(6), False, 1.0) for i in range(N - 1)]
    g.edges += [PoseGraphEdge(i, j, _exact(i, j), 3000.0 * np.eye(6), True, 1.0) for i, j in LOOPS]
    g.edges += list(extra)
    return g


def _drifted():
    rng = np.random.default_rng(3)
    d = np.array(GT)
    for i in range(1, N):
        d[i] = mat4(rng.normal(0.0, [0.01, 0.01, 0.01, 0.02, 0.02, 0.02])) @ d[i]
    return d


def _option(ref=0):
    return GlobalOptimizationOption(max_correspondence_distance=0.07, edge_prune_threshold=PRUNE, reference_node=ref)


def _max_pose_error(g):
    return max(float(np.abs(n.pose - t).max()) for n, t in zip(g.nodes, GT))


def test_vec6_mat4_round_trip():
    rng = np.random.default_rng(0)
    v = rng.uniform(-1.0, 1.0, (200, 6)) * [3.0, 1.5, 3.0, 2.0, 2.0, 2.0]
    T = mat4(v)
    assert np.abs(vec6(T) - v).max() <= 1e-12
    assert np.abs(mat4(vec6(T)) - T).max() <= 1e-12
    assert np.abs(T[:, :3, :3] @ np.swapaxes(T[:, :3, :3], 1, 2) - np.eye(3)).max() <= 1e-12
    # sy <= 1e-6: ry = +-pi/2; rz is reported as 0 and rx takes the whole in-plane angle
    for ry in (np.pi / 2, -np.pi / 2):
        w = v[:20].copy()
        w[:, 1] = ry
        Tg = mat4(w)
        assert (np.sqrt(Tg[:, 0, 0] ** 2 + Tg[:, 1, 0] ** 2) <= 1e-6).all()
        back = vec6(Tg)
        assert (back[:, 2] == 0.0).all()
        assert np.abs(mat4(back) - Tg).max() <= 1e-12
    assert np.array_equal(mat4(np.zeros(6)), np.eye(4))
    assert np.array_equal(vec6(np.eye(4)), np.zeros(6))


def test_consistent_graph_is_left_unchanged():
    g = _graph(GT)
    global_optimization(g, _option())
    assert _max_pose_error(g) <= 1e-9
    assert len(g.edges) == N - 1 + len(LOOPS)
    assert all(e.confidence > 0.9 for e in g.edges if e.uncertain)


def test_drifted_graph_recovers_ground_truth():
    start = _drifted()
    assert float(np.abs(start - GT).max()) > 1e-2
    g = _graph(start)
    reports = global_optimization(g, _option())
    assert _max_pose_error(g) <= 1e-6
    assert np.array_equal(g.nodes[0].pose, GT[0])  # the reference node, bit for bit
    for rep in reports:
        r = rep["residuals"]
        assert all(b <= a for a, b in zip(r, r[1:])), r
    assert reports[0]["residuals"][0] > 1.0 and reports[1]["residuals"][-1] < 1e-6
    assert len(g.edges) == N - 1 + len(LOOPS)


def test_open3d_argument_order_is_accepted():
    g = _graph(_drifted())
    global_optimization(g, GlobalOptimizationLevenbergMarquardt(), GlobalOptimizationConvergenceCriteria(), _option())
    assert _max_pose_error(g) <= 1e-6


def test_false_loop_edge_is_pruned():
    wrong = mat4(np.array([0.0, np.deg2rad(20.0), 0.0, 0.5, 0.0, 0.0])) @ _exact(1, 9)
    false = PoseGraphEdge(1, 9, wrong, 3000.0 * np.eye(6), True, 1.0)
    g = _graph(_drifted(), [false])
    reports = global_optimization(g, _option())
    assert reports[0]["pruned"] == 1
    assert all(e is not false for e in g.edges) and len(g.edges) == N - 1 + len(LOOPS)
    assert false.confidence < PRUNE
    loops = [e for e in g.edges if e.uncertain]
    assert len(loops) == len(LOOPS) and all(e.confidence > 0.9 for e in loops)
    assert _max_pose_error(g) <= 1e-6


def test_certain_edges_are_never_pruned():
    # the same wrong edge marked certain stays (and drags the solution), whatever it costs
    wrong = mat4(np.array([0.0, np.deg2rad(20.0), 0.0, 0.5, 0.0, 0.0])) @ _exact(1, 9)
    certain = PoseGraphEdge(1, 9, wrong, 3000.0 * np.eye(6), False, 1.0)
    g = _graph(GT, [certain])
    global_optimization(g, _option())
    assert any(e is certain for e in g.edges)
    assert sum(not e.uncertain for e in g.edges) == N
    assert certain.confidence == 1.0


def test_graph_without_edges_is_unchanged():
    start = _drifted()
    g = PoseGraph(nodes=[PoseGraphNode(np.array(p)) for p in start])
    global_optimization(g, _option())
    assert all(np.array_equal(n.pose, p) for n, p in zip(g.nodes, start)) and g.edges == []
    empty = PoseGraph()
    global_optimization(empty, _option())
    assert empty.nodes == [] and empty.edges == []


def test_reference_node_minus_one_is_node_zero():
    a, b = _graph(_drifted()), _graph(_drifted())
    global_optimization(a, _option(ref=-1))
    global_optimization(b, _option(ref=0))
    assert all(np.array_equal(x.pose, y.pose) for x, y in zip(a.nodes, b.nodes))
    assert np.array_equal(a.nodes[0].pose, GT[0])


def test_another_reference_node_is_held():
    start = _drifted()
    g = _graph(start)
    global_optimization(g, _option(ref=5))
    assert np.array_equal(g.nodes[5].pose, start[5])
    # the graph is consistent again: every edge's misalignment vanishes
    for e in g.edges:
        m = np.linalg.inv(e.transformation) @ np.linalg.inv(g.nodes[e.target_node_id].pose) @ g.nodes[e.source_node_id].pose
        assert np.abs(m - np.eye(4)).max() <= 1e-6


def test_containers_are_shared_with_fragments():
    from mqr import fragments
    assert fragments.PoseGraph is PoseGraph and fragments.PoseGraphEdge is PoseGraphEdge
    assert fragments.PoseGraphNode is PoseGraphNode


def test_bad_edge_index_raises():
    g = _graph(GT, [PoseGraphEdge(0, N, np.eye(4), np.eye(6), True, 1.0)])
    with pytest.raises(ValueError):
        global_optimization(g, _option())
