"""The edge list shared by the mesh filter and the mesh quality pass (csrc/mesh_edges.hpp), through both of its
users, against their CPU restatements: oracle/meshfilter_ref.py bit for bit, tests/quality_ref.py within its
tolerance (the fields asserted here are integers: exact)."""
from dataclasses import asdict

import numpy as np
import pytest

import meshfilter_ref as mf
import quality_ref as qr
from test_gpu_meshfilter import _cmp

pytestmark = pytest.mark.gpu


def gpu_filter(v, t, min_count):
    from mqr.meshfilter import filter_mesh_components_gpu
    return filter_mesh_components_gpu(v, None, t, min_count)


def gpu_metrics(v, t):
    from mqr.evaluation import compute_raw_metrics
    return asdict(compute_raw_metrics((v, t), name="m"))


@pytest.mark.parametrize("nt", [1, 85, 86, 341, 342])
def test_strips_through_the_filter_at_workgroup_and_slab_edges(nt):
    """3 nt crosses 256 (one workgroup of the edge kernels) between 85 and 86, and 1024 (one slab of the
    quality pass's reductions) between 341 and 342."""
    v, t, _ = qr.strip_mesh(nt, seed=nt)
    for min_count in (1, nt + 1):  # everything qualifies / nothing does: the largest cluster is kept
        _cmp(gpu_filter(v, t, min_count), mf.filter_mesh_components(v, None, t, min_count))


def test_loop_edge_is_adjacency_for_the_filter_and_no_edge_for_the_metrics():
    """Two triangles that share only the loop edge (0, 0), and one ordinary triangle elsewhere: the one intended
    difference between the two users of k_edge_keys."""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [5, 0, 0], [6, 0, 0], [5, 1, 0]], np.float32)
    t = np.array([[0, 0, 1], [0, 0, 2], [3, 4, 5]], np.int32)
    ref = mf.filter_mesh_components(v, None, t, 1)
    assert ref[3]["clusters"] == 2  # Open3D's rule: the first two triangles are one cluster
    got = gpu_filter(v, t, 1)
    assert got[3]["clusters"] == ref[3]["clusters"]
    _cmp(got, ref)
    want, _ = qr.raw_metrics(v, t, None)
    assert want["total_edges"] == 5 and want["component_count"] == 2  # (0,1), (0,2), three of the ordinary one
    m = gpu_metrics(v, t)
    assert m["total_edges"] == want["total_edges"] and m["component_count"] == want["component_count"]


def test_fan_of_four_on_one_edge_and_an_unreferenced_vertex():
    v = np.array([[0, 0, 0], [1, 0, 0], [0.5, 1.0, 0], [0.5, -2.0, 0], [0.5, 0, 3.0], [0.5, 0, -4.0], [9, 9, 9]],
                 np.float32)
    t = np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4], [1, 0, 5]], np.int32)
    ref = mf.filter_mesh_components(v, None, t, 1)
    assert ref[3]["non_manifold_removed"] == 2  # the two smallest of the four go
    got = gpu_filter(v, t, 1)
    assert got[3]["non_manifold_removed"] == ref[3]["non_manifold_removed"]
    _cmp(got, ref)
    want, _ = qr.raw_metrics(v, t, None)
    assert want["non_manifold_edges"] == 1 and want["component_count"] == 2  # the fan, and vertex 6 on its own
    m = gpu_metrics(v, t)
    assert m["non_manifold_edges"] == want["non_manifold_edges"]
    assert m["component_count"] == want["component_count"]
