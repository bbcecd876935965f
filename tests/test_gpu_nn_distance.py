"""mqr_nn_* (csrc/meshcompare.hip) through mqr.compare_mesh_to_ground_truth.NearestNeighbour: distances and
indices bit-equal to the float64 brute force of compare_ref.nearest (d2 = (dx dx + dy dy) + dz dz, lowest index
among equal d2, dist = sqrt(d2))."""
import ctypes

import numpy as np
import pytest

import compare_ref as cr

pytestmark = pytest.mark.gpu

N_TARGETS = (1, 15, 16, 17, 255, 256, 257, 4097)  # bucket (16) and tree-level edges
N_QUERIES = (1, 63, 64, 65, 257)                   # wave and workgroup edges


def search(targets, queries):
    from mqr.compare_mesh_to_ground_truth import NearestNeighbour
    with NearestNeighbour(targets) as nn:
        return nn.query(queries, indices=True)


def check(targets, queries, label=""):
    d, i = search(targets, queries)
    wd, wi = cr.nearest(queries, targets)
    assert d.dtype == np.float64 and i.dtype == np.int32
    assert np.array_equal(i, wi), (label, np.nonzero(i != wi)[0][:5])
    assert np.array_equal(d.view(np.uint64), wd.view(np.uint64)), (label, np.abs(d - wd).max())
    return d, i


@pytest.fixture(scope="module")
def clouds():
    rng = np.random.default_rng(2)
    return rng.uniform(-1, 1, (max(N_TARGETS), 3)).astype(np.float32), rng.uniform(-1.2, 1.2, (max(N_QUERIES), 3)).astype(np.float32)


@pytest.mark.parametrize("n", N_TARGETS)
def test_sizes_at_bucket_level_and_wave_edges(clouds, n):
    from mqr.compare_mesh_to_ground_truth import NearestNeighbour
    t, q = clouds
    wd, wi = cr.nearest(q, t[:n])
    with NearestNeighbour(t[:n]) as nn:  # one tree, every query count
        for nq in N_QUERIES:
            d, i = nn.query(q[:nq], indices=True)
            assert np.array_equal(i, wi[:nq]), (n, nq)
            assert np.array_equal(d.view(np.uint64), wd[:nq].view(np.uint64)), (n, nq)
            assert np.array_equal(nn.query(q[:nq]), d)  # idx NULL


def test_identical_targets_have_a_zero_extent_box(clouds):
    t = np.tile(np.array([[0.25, -0.5, 2.0]], np.float32), (100, 1))
    d, i = check(t, clouds[1], "identical")
    assert (i == 0).all()


def test_coplanar_targets(clouds):
    t = clouds[0][:1000].copy()
    t[:, 2] = 0.5
    check(t, clouds[1], "coplanar")


def test_duplicated_targets_lowest_index_wins(clouds):
    base = clouds[0][:300]
    t = np.concatenate([base, base[::-1], base])  # every point three times, far apart in index
    d, i = check(t, clouds[1], "duplicates")
    assert (i < 300).all()


def test_query_equal_to_a_target_has_distance_zero(clouds):
    t = clouds[0][:2000]
    q = t[::7].copy()
    d, i = check(t, q, "equal")
    assert (d == 0.0).all() and np.array_equal(i, np.arange(0, 2000, 7))


def test_queries_far_outside_the_box(clouds):
    t = clouds[0][:3000]
    rng = np.random.default_rng(4)
    q = (rng.uniform(-1, 1, (200, 3)) * np.array([1e3, 50.0, 1e4])).astype(np.float32)
    check(t, q, "far")


def test_everything_offset_by_a_kilometre(clouds):
    """At |coordinate| ~ 1000 a float32 difference of nearby points keeps few bits: the float32 bound's 2^-18
    margin has to cover it."""
    off = np.array([1000.0, -1000.0, 1000.0], np.float32)
    t = (clouds[0][:4097] * 0.05 + off).astype(np.float32)
    q = (clouds[1] * 0.05 + off).astype(np.float32)
    check(t, q, "offset")


def test_coordinate_range(clouds):
    """Up to 1e18 the float32 bounds cannot overflow and the search stays exact; beyond it a coordinate is
    rejected (an overflowed bound would be +inf and prune nearer points)."""
    from mqr import _lib
    from mqr.compare_mesh_to_ground_truth import NearestNeighbour
    t = (clouds[0][:2000] * np.float32(9e17)).astype(np.float32)
    q = (clouds[1] * np.float32(8e17)).astype(np.float32)
    check(t, q, "huge")
    mixed = np.concatenate([clouds[0][:500], t[:500]])  # a unit cluster inside a box 1e18 wide
    check(mixed, np.concatenate([clouds[1], q[:50]]), "mixed scales")
    far = clouds[0][:100].copy()
    far[7, 2] = 3e19
    buf = _lib.DeviceBuffer.from_array(far)
    h = ctypes.c_void_p()
    with pytest.raises(_lib.MqrError, match="beyond 1e18"):
        _lib.call("mqr_nn_create", 0, buf.ptr, len(far), _lib.MQR_DEVICE, ctypes.byref(h))
    with pytest.raises(ValueError, match="beyond 1e18"):
        NearestNeighbour(far)


def test_repeated_call_is_bit_identical(clouds):
    from mqr.compare_mesh_to_ground_truth import NearestNeighbour
    t, q = clouds
    with NearestNeighbour(t) as nn:
        a, b = nn.query(q, indices=True), nn.query(q, indices=True)
    assert np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64)) and np.array_equal(a[1], b[1])
    d, i = search(t, q[::-1])  # and the order of the queries does not matter
    assert np.array_equal(d[::-1], a[0]) and np.array_equal(i[::-1], a[1])


def test_device_resident_inputs_equal_host_inputs(clouds):
    from mqr import _lib
    from mqr.compare_mesh_to_ground_truth import NearestNeighbour
    t, q = clouds
    want = search(t, q)
    bt, bq = _lib.DeviceBuffer.from_array(t), _lib.DeviceBuffer.from_array(q)
    bd, bi = _lib.DeviceBuffer(8 * len(q)), _lib.DeviceBuffer(4 * len(q))
    with NearestNeighbour((bt.ptr.value, len(t))) as nn:
        bt.free()  # the tree keeps its own copy of the targets
        _lib.call("mqr_nn_query", nn._h, bq.ptr, len(q), _lib.MQR_DEVICE, bd.ptr, bi.ptr, _lib.MQR_DEVICE)
    assert np.array_equal(bd.to_array(len(q), np.float64), want[0])
    assert np.array_equal(bi.to_array(len(q), np.int32), want[1])


def test_nan_target_is_rejected_and_the_library_stays_usable(clouds):
    from mqr import _lib
    t, q = clouds
    bad = t[:500].copy()
    bad[123, 1] = np.nan
    buf = _lib.DeviceBuffer.from_array(bad)  # in HBM numpy cannot check it: the device pass must
    h = ctypes.c_void_p()
    with pytest.raises(_lib.MqrError, match="not finite"):
        _lib.call("mqr_nn_create", 0, buf.ptr, len(bad), _lib.MQR_DEVICE, ctypes.byref(h))
    assert not h.value
    inf = q[:10].copy()
    inf[3, 0] = np.inf
    qb = _lib.DeviceBuffer.from_array(inf)
    out = _lib.DeviceBuffer(80)
    from mqr.compare_mesh_to_ground_truth import NearestNeighbour
    with NearestNeighbour(t[:500]) as nn:
        with pytest.raises(_lib.MqrError, match="not finite"):
            _lib.call("mqr_nn_query", nn._h, qb.ptr, 10, _lib.MQR_DEVICE, out.ptr, None, _lib.MQR_DEVICE)
    check(t[:500], q, "after the errors")
