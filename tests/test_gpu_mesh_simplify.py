"""Vertex clustering on the device (csrc/meshsimplify.hip through the C ABI, TriangleMesh.simplify_vertex_clustering
and mqr.downsample_mesh) against tests/simplify_ref.py, the numpy restatement of the rule.
Positions, normals, colours, triangles and stats are compared bit for bit: the rule is float64 with a fixed
order of operations, so there is no tolerance to state.  The triples of a result with 2^21 or more vertices are
sorted in two passes (c, then (a, b)); below that they are one key: both paths are implemented, and
test_wide_triples reaches the first."""
import ctypes

import numpy as np
import pytest

import simplify_ref as sr
from test_gpu_mesh_quality import room  # noqa: F401  (fixture: the extracted room mesh, left in HBM)
from test_simplify_ref import boundary_case, cube_case, f32, isolated_case, negative_case, triangle_case

pytestmark = pytest.mark.gpu

NV = [1, 3, 63, 64, 65, 256, 257, 4097, 65537]   # wave, workgroup, scan-tile and sort-algorithm edges
NT_EDGES = [0, 1, 255, 256, 257]
HUGE, TINY = 1.0e3, 1.0e-5                         # everything in one cell / every vertex alone


def random_mesh(nv, nt=None, seed=0):
    """Random vertices and random index triples, as tests/test_gpu_mesh_sample.py builds them."""
    rng = np.random.default_rng(seed + 1000 * nv)
    nt = 2 * nv if nt is None else nt
    v = rng.standard_normal((nv, 3)).astype(np.float32)
    t = rng.integers(0, nv, (nt, 3)).astype(np.int32)
    return v, t


def fields(v, seed=0):
    rng = np.random.default_rng(seed + 7)
    return rng.standard_normal(v.shape).astype(np.float32), rng.random(v.shape).astype(np.float32)


def raw_simplify(v, t, voxel_size, normals=None, colors=None, in_device=False, nv=None, device=0):
    """One mqr_mesh_simplify_clustering call without error translation -> (status, handle, stats, held buffers)."""
    from mqr import _lib
    L = _lib.load()
    vp = ctypes.c_void_p
    held, ptrs = [], []
    for a in (v, normals, colors, t):
        if a is None or a.size == 0:
            ptrs.append(None)
        elif in_device:
            held.append(_lib.DeviceBuffer.from_array(a, device))
            ptrs.append(held[-1].ptr.value)
        else:
            ptrs.append(a.ctypes.data)
    g, stats = vp(), np.full(8, -1, np.int64)
    rc = L.mqr_mesh_simplify_clustering(device, vp(ptrs[0]), len(v) if nv is None else nv, vp(ptrs[1]), vp(ptrs[2]),
                                        vp(ptrs[3]), 0 if t is None else len(t),
                                        _lib.MQR_DEVICE if in_device else _lib.MQR_HOST, float(voxel_size),
                                        ctypes.byref(g), _lib.ptr(stats, _lib._i64p))
    return rc, g, stats, held


def device_simplify(v, t, voxel_size, normals=None, colors=None, in_device=False):
    """-> (positions, normals, colors or None, triangles, stats) as host arrays (normals are zeros without input)."""
    from mqr import _lib
    rc, g, stats, held = raw_simplify(v, t, voxel_size, normals, colors, in_device)
    try:
        assert rc == 0, _lib.load().mqr_last_error().decode()
        nv, nt = ctypes.c_int64(), ctypes.c_int64()
        _lib.call("mqr_geom_counts", g, ctypes.byref(nv), ctypes.byref(nt))
        pos, nrm = np.empty((nv.value, 3), np.float32), np.empty((nv.value, 3), np.float32)
        tri = np.empty((nt.value, 3), np.int32)
        _lib.call("mqr_geom_copy", g, _lib.ptr(pos), _lib.ptr(nrm), _lib.ptr(tri) if nt.value else None, _lib.MQR_HOST)
        col = None
        if colors is not None:
            col = np.empty((nv.value, 3), np.float32)
            _lib.call("mqr_geom_copy_colors", g, _lib.ptr(col), _lib.MQR_HOST)
        else:
            c = ctypes.c_void_p()
            _lib.call("mqr_geom_device_colors", g, ctypes.byref(c))
            assert not c.value
    finally:
        if g.value:
            _lib.call("mqr_geom_free", g)
        for b in held:
            b.free()
    return pos, nrm, col, tri, stats


def device_count(v, voxel_size, in_device=False):
    from mqr import _lib
    n = ctypes.c_int64(-1)
    buf = _lib.DeviceBuffer.from_array(v) if in_device else None
    try:
        _lib.call("mqr_mesh_cluster_count", 0, ctypes.c_void_p(buf.ptr.value if in_device else v.ctypes.data), len(v),
                  _lib.MQR_DEVICE if in_device else _lib.MQR_HOST, float(voxel_size), ctypes.byref(n))
    finally:
        if buf is not None:
            buf.free()
    return n.value


def same_bits(got, want, what=""):
    """got from device_simplify, want from sr.simplify."""
    gp, gn, gc, gt, gs = got
    wp, wn, wc, wt, ws = want
    assert np.array_equal(gs, ws), (what, gs.tolist(), ws.tolist())
    if wn is None:
        wn = np.zeros_like(wp)
    assert (gc is None) == (wc is None), what
    for name, g, w in (("positions", gp, wp), ("normals", gn, wn), ("colors", gc, wc)):
        if w is not None:
            assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape)
            assert np.array_equal(g.view(np.uint32), w.view(np.uint32)), (what, name)
    assert gt.shape == wt.shape and gt.dtype == wt.dtype and np.array_equal(gt, wt), (what, "triangles")


def check(v, t, voxel_size, normals=None, colors=None, what="", in_device=False):
    want = sr.simplify(v, t, voxel_size, normals, colors)
    same_bits(device_simplify(v, t, voxel_size, normals, colors, in_device), want, what)
    assert device_count(v, voxel_size) == want[4][1] == sr.cluster_count(v, voxel_size), what
    return want


@pytest.mark.parametrize("nv", NV)
def test_random_meshes_at_launch_edges(nv):
    v, t = random_mesh(nv)
    nrm, col = fields(v)
    for j, vs in enumerate((0.1, 0.25, HUGE, TINY)):
        with_n, with_c = bool((j + nv) & 1), bool((j + nv) & 2) or j == 0
        want = check(v, t, vs, nrm if with_n else None, col if with_c else None, f"nv={nv} vs={vs}")
        if vs == HUGE:
            assert want[4][1] == 1 and want[4][6] == nv and want[4][5] == 0
        if vs == TINY:
            assert want[4][1] == nv and want[4][6] == 1


@pytest.mark.parametrize("nt", NT_EDGES)
def test_triangle_count_edges(nt):
    v, t = random_mesh(257, nt, seed=1)
    nrm, col = fields(v)
    for vs in (0.25, TINY):
        check(v, t if nt else None, vs, nrm, col, f"nt={nt} vs={vs}")
    if nt:  # many duplicates and collapses: 257 triangles over 12 vertices
        t2 = np.random.default_rng(nt).integers(0, 12, (nt, 3)).astype(np.int32)
        want = check(v, t2, TINY, what=f"nt={nt} dense")
        assert nt < 255 or (want[4][3] > 0 and want[4][4] > 0)


@pytest.mark.parametrize("nrm_on,col_on", [(False, False), (True, False), (False, True), (True, True)])
def test_with_and_without_normals_and_colours(nrm_on, col_on):
    v, t = random_mesh(4097, seed=2)
    nrm, col = fields(v)
    check(v, t, 0.1, nrm if nrm_on else None, col if col_on else None, f"normals={nrm_on} colors={col_on}")


def clusters(pops, seed):
    """Cluster k holds pops[k] points x = k + u, u in [0, 0.4) (one point exactly 0), shuffled: with voxel_size 1
    the origin is -0.5 and cluster k is cell k."""
    rng = np.random.default_rng(seed)
    x = np.concatenate([k + 0.4 * rng.random(p) for k, p in enumerate(pops)])
    v = np.column_stack([x, 0.4 * rng.random(len(x)), 0.4 * rng.random(len(x))]).astype(np.float32)
    v[0] = 0.0
    return v[np.concatenate([[0], 1 + rng.permutation(len(v) - 1)])]


def test_a_cell_of_70000_members():
    v = clusters([70000, 3, 1], seed=3)
    nrm, col = fields(v)
    t = np.random.default_rng(4).integers(0, len(v), (1000, 3)).astype(np.int32)
    want = check(v, t, 1.0, nrm, col, "70000")
    assert want[4][1] == 3 and want[4][6] == 70000


def test_populations_side_by_side():
    pops = [1, 63, 64, 65, 257]
    v = clusters(pops, seed=5)
    nrm, col = fields(v)
    t = np.random.default_rng(6).integers(0, len(v), (2 * len(v), 3)).astype(np.int32)
    want = check(v, t, 1.0, nrm, col, "populations")
    assert want[4][1] == 5 and want[4][6] == 257
    mp, _ = sr.first_appearance(sr.cells(v, 1.0)[0])
    assert sorted(np.bincount(mp).tolist()) == pops


def test_hand_built_cases():
    v, t, vs = cube_case()
    got = device_simplify(v, t, vs, v * 2, v * 0.25)
    same_bits(got, sr.simplify(v, t, vs, v * 2, v * 0.25), "cube")
    assert got[0].tolist() == [[0.5, 0.5, 0.5]] and got[1].tolist() == [[1, 1, 1]] and got[4][3] == 12
    v, t, vs = isolated_case()
    got = check(v, t, vs, what="isolated")
    assert np.array_equal(got[0].view(np.uint32), v.view(np.uint32))
    v, vs, _ = boundary_case()
    want = check(v, None, vs, what="boundary")
    assert want[4][1] == 5 and want[0][1, 0] == np.float32(0.1875)  # 0.125 belongs to the upper cell, with 0.25
    v, vs, _ = negative_case()
    check(v, None, vs, what="negative")
    got = device_simplify(f32([[-0.0, -0.0, -0.0], [1, 1, 1]]), None, 0.25)
    assert not np.signbit(got[0][0]).any()
    v, t, vs, want_tri = triangle_case()
    got = device_simplify(v, t, vs)
    same_bits(got, sr.simplify(v, t, vs), "triangles")
    assert got[3].tolist() == want_tri.tolist() and got[4].tolist() == [10, 9, 11, 2, 5, 4, 2, 33]


def test_wide_triples():
    """2^21 + 1 isolated vertices on a 129 x 128 x 128 lattice: the output vertex count passes 2^21, so the triples
    are sorted in two passes.  Triangles: a pool of 24 vertices (low and high indices) gives duplicates in every
    rotation, opposite pairs, collapses and triples that share (a, b) and differ in c."""
    n = (1 << 21) + 1
    i = np.arange(n)
    v = np.column_stack([i // (128 * 128), (i // 128) % 128, i % 128]).astype(np.float32)
    rng = np.random.default_rng(8)
    pool = np.concatenate([rng.integers(0, 64, 8), rng.integers(n - 4096, n, 15), [n - 1]])
    t = pool[rng.integers(0, len(pool), (3000, 3))].astype(np.int32)
    t[10] = [n - 1, 5, n - 2]
    t[20] = [5, n - 2, n - 1]           # the same triple from another corner
    t[30] = [n - 2, 5, n - 1]           # the opposite orientation
    t[40] = [n - 1, n - 1, 3]           # collapsed
    t[50], t[60] = [7, n - 3, n - 5], [7, n - 3, n - 6]  # (a, b) shared, c differs
    want = sr.simplify(v, t, 0.25)
    assert want[4][1] == n >= 1 << 21 and want[4][3] > 0 and want[4][4] > 100 and want[4][5] > 1000
    got = device_simplify(v, t, 0.25, in_device=True)
    same_bits(got, want, "wide")
    assert device_count(v, 0.25, in_device=True) == n


def test_cluster_count_on_device_inputs():
    v, _ = random_mesh(4097, seed=9)
    for vs in (0.1, 0.25, HUGE, TINY):
        assert device_count(v, vs, in_device=True) == device_count(v, vs) == sr.cluster_count(v, vs)
    from mqr import _lib
    lo, hi = np.empty(3), np.empty(3)
    _lib.call("mqr_vertex_bounds", 0, _lib.ptr(v), len(v), _lib.MQR_HOST, _lib.ptr(lo, _lib._f64p),
              _lib.ptr(hi, _lib._f64p))
    assert np.array_equal(lo, v.min(0).astype(np.float64)) and np.array_equal(hi, v.max(0).astype(np.float64))


def test_errors_leave_the_handle_null():
    from mqr import _lib
    v, t = random_mesh(257, seed=10)
    nan_v = v.copy()
    nan_v[7, 1] = np.nan
    t_hi, t_neg = t.copy(), t.copy()
    t_hi[100, 2] = len(v)
    t_neg[5, 0] = -1
    two = f32([[0, 0, 0], [1, 0, 0]])
    cases = [("not finite", nan_v, t, 0.25, None), ("outside", v, t_hi, 0.25, None), ("outside", v, t_neg, 0.25, None),
             ("voxel_size", v, t, 0.0, None), ("voxel_size", v, t, float("nan"), None), ("no vertices", v, None, 0.25, 0),
             ("too fine", two, None, 1e-7, None)]
    for match, vv, tt, vs, nv in cases:
        for in_device in (False, True):
            rc, g, stats, held = raw_simplify(vv, tt, vs, in_device=in_device, nv=nv)
            for b in held:
                b.free()
            assert rc == 2 and not g.value, (match, rc)
            assert match in _lib.load().mqr_last_error().decode(), match
    n = ctypes.c_int64()
    with pytest.raises(_lib.MqrError, match="too fine"):
        _lib.call("mqr_mesh_cluster_count", 0, _lib.ptr(two), 2, _lib.MQR_HOST, 1e-7, ctypes.byref(n))
    with pytest.raises(_lib.MqrError, match="not finite"):
        _lib.call("mqr_mesh_cluster_count", 0, _lib.ptr(nan_v), len(v), _lib.MQR_HOST, 0.25, ctypes.byref(n))
    same_bits(device_simplify(v, t, 0.25), sr.simplify(v, t, 0.25), "after the errors")


def test_python_mirror_on_host_meshes():
    from mqr.geometry import GridTooFine, Tensor, TriangleMesh, device_ptr
    v, t = random_mesh(4097, seed=11)
    nrm, col = fields(v)
    mesh = TriangleMesh(v, nrm, t)
    out = mesh.simplify_vertex_clustering(0.25, contraction="Average")
    assert isinstance(out, TriangleMesh) and device_ptr(out.vertex.positions) is None and not out.has_vertex_colors()
    want = sr.simplify(v, t, 0.25, nrm)
    assert np.array_equal(out.vertices.view(np.uint32), want[0].view(np.uint32))
    assert np.array_equal(out.vertex_normals.view(np.uint32), want[1].view(np.uint32))
    assert np.array_equal(out.triangles, want[3])
    mesh.vertex["colors"] = Tensor(col)
    out = mesh.simplify_vertex_clustering(0.25)
    assert np.array_equal(out.vertex_colors.view(np.uint32), sr.simplify(v, t, 0.25, nrm, col)[2].view(np.uint32))
    bad_v = v.copy()
    bad_v[3, 0] = np.inf
    with pytest.raises(ValueError, match="not finite"):
        TriangleMesh(bad_v, nrm, t).simplify_vertex_clustering(0.25)
    bad_t = t.copy()
    bad_t[5, 0] = len(v)
    with pytest.raises(ValueError, match="outside"):
        TriangleMesh(v, nrm, bad_t).simplify_vertex_clustering(0.25)
    with pytest.raises(ValueError, match="normals must be"):
        TriangleMesh(v, nrm[:-1], t).simplify_vertex_clustering(0.25)
    with pytest.raises(GridTooFine):
        mesh.simplify_vertex_clustering(1e-7)
    assert issubclass(GridTooFine, RuntimeError)


def test_python_mirror_reports_device_input_errors_as_value_errors():
    from mqr import _lib
    from mqr.geometry import DeviceArray, Tensor, TriangleMesh
    v, t = random_mesh(257, seed=12)
    bad_t = t.copy()
    bad_t[5, 0] = len(v)
    bufs = [_lib.DeviceBuffer.from_array(a) for a in (v, np.zeros_like(v), bad_t)]
    dev = [Tensor(DeviceArray(b, b.ptr.value, a.shape, a.dtype, 0)) for b, a in zip(bufs, (v, v, bad_t))]
    with pytest.raises(ValueError, match="outside"):
        TriangleMesh(*dev, device="HIP:0").simplify_vertex_clustering(0.25)


def mesh_bits(m):
    c = m.vertex_colors
    return (m.vertices.view(np.uint32), m.vertex_normals.view(np.uint32), m.triangles,
            None if c is None else c.view(np.uint32))


def same_mesh(a, b, what=""):
    for x, y in zip(mesh_bits(a), mesh_bits(b)):
        assert (x is None) == (y is None) and (x is None or np.array_equal(x, y)), what


def test_room_in_place_and_from_host_copies(room):  # noqa: F811
    from mqr.geometry import Tensor, device_ptr
    dev = device_ptr(room.vertex.positions)
    assert dev is not None
    vs = 4 * 0.02
    on_device = room.simplify_vertex_clustering(vs)
    for field in (on_device.vertex.positions, on_device.vertex.normals, on_device.triangle.indices):
        assert device_ptr(field, dev[1]) is not None
    assert on_device.device == room.device and not on_device.has_vertex_colors()
    host = room.cpu()
    from_host = host.simplify_vertex_clustering(vs)
    assert device_ptr(from_host.vertex.positions) is None
    same_mesh(on_device, from_host, "in place vs host copies")
    same_mesh(room.simplify_vertex_clustering(vs), on_device, "repeated call")
    want = sr.simplify(host.vertices, host.triangles, vs, host.vertex_normals)
    assert len(on_device.vertices) == want[4][1] < len(host.vertices) and want[4][5] > 100
    assert np.array_equal(on_device.vertices.view(np.uint32), want[0].view(np.uint32))
    assert np.array_equal(on_device.vertex_normals.view(np.uint32), want[1].view(np.uint32))
    assert np.array_equal(on_device.triangles, want[3])


def test_room_downsample_feeds_the_downstream_stages(room):  # noqa: F811
    """downsample_mesh(room, 10) reaches the size and count of the restatement's search, and its coloured result,
    still in HBM, is an input of the quality metrics and the surface sampler like any other."""
    from mqr import _lib
    from mqr.downsample_mesh import downsample_mesh
    from mqr.evaluation import compute_raw_metrics
    from mqr.geometry import DeviceArray, Tensor, device_ptr
    host = room.cpu()
    v, t, nrm = host.vertices, host.triangles, host.vertex_normals
    col = np.random.default_rng(13).random(v.shape).astype(np.float32)
    buf = _lib.DeviceBuffer.from_array(col)
    dev = device_ptr(room.vertex.positions)[1]
    room.vertex["colors"] = Tensor(DeviceArray(buf, buf.ptr.value, col.shape, col.dtype, dev))
    try:
        out = downsample_mesh(room, 10)
        ref_out = downsample_mesh(room, 10, voxel_size_rule="reference")
    finally:
        del room.vertex["colors"]
    size, want = sr.downsample(v, t, 10, "fit", nrm, col)
    target = sr.target_count(len(v), 10)
    print(f"room: {len(v)} vertices, target {target}, fit size {size:.6f} -> {want[4][1]} vertices; "
          f"v_ref -> {len(ref_out.vertices)}")
    for field in (out.vertex.positions, out.vertex.normals, out.vertex["colors"], out.triangle.indices):
        assert device_ptr(field, dev) is not None
    assert len(out.vertices) == want[4][1]
    for got, w in zip(mesh_bits(out), (want[0], want[1], want[3], want[2])):
        assert np.array_equal(got, w.view(np.uint32) if w.dtype == np.float32 else w)
    assert abs(want[4][1] - target) <= abs(len(ref_out.vertices) - target)
    _, want_ref = sr.downsample(v, t, 10, "reference", nrm, col)
    assert np.array_equal(ref_out.vertices.view(np.uint32), want_ref[0].view(np.uint32))
    m = compute_raw_metrics(out, name="downsampled")
    assert m.num_vertices == want[4][1] and m.num_triangles == want[4][5] and m.has_color
    pc = out.sample_points_uniformly(1000, seed=1)
    assert device_ptr(pc.point.positions, dev) is not None and pc.has_colors() and len(pc.points) == 1000
    assert downsample_mesh(room, 100) is room


def test_existing_producers_report_no_colours(room):  # noqa: F811
    from mqr import _lib
    from mqr.geometry import DeviceGeom
    from mqr.meshfilter import filter_mesh_components
    for mesh in (room, filter_mesh_components(room, 50)):
        geom = mesh.vertex.positions.device_array().owner
        assert isinstance(geom, DeviceGeom) and geom.colors() is None
        out = np.zeros((geom.nv, 3), np.float32)
        with pytest.raises(_lib.MqrError, match="no colours"):
            _lib.call("mqr_geom_copy_colors", geom._h, _lib.ptr(out), _lib.MQR_HOST)
