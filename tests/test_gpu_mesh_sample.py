"""Surface sampling on the device (csrc/meshsample.hip through the C ABI and TriangleMesh.sample_points_uniformly)
against tests/sample_ref.py, the numpy restatement of the rule.  Positions, normals, colours and
triangle indices are compared bit for bit: the rule is integer arithmetic for the selection and float64 with a
fixed operation order for the point, so there is no tolerance to state."""
import ctypes

import numpy as np
import pytest

import sample_ref as sr
from test_gpu_mesh_quality import room  # noqa: F401  (fixture: the extracted room mesh, left in HBM)

pytestmark = pytest.mark.gpu

NT = [1, 2, 255, 256, 257, 4097, 65537]     # coarse-table segment (256) and scan-tile edges
N = [1, 63, 64, 65, 257, 100003]            # wave, workgroup and grid-stride edges
SEEDS = [0, 2 ** 64 - 1]


def random_mesh(nt, seed=0, scale=1.0):
    """Random vertices and random index triples (triangle order is random by construction)."""
    rng = np.random.default_rng(seed + 1000 * nt)
    nv = max(3, nt // 2 + 3)
    v = (rng.standard_normal((nv, 3)) * scale).astype(np.float32)
    t = rng.integers(0, nv, (nt, 3)).astype(np.int32)
    t[0] = [0, 1, 2]  # at least one triangle with distinct corners
    return v, t


def fields(v, seed=0):
    rng = np.random.default_rng(seed + 7)
    return rng.standard_normal(v.shape).astype(np.float32), rng.random(v.shape).astype(np.float32)


def device_sample(v, t, n, seed=0, normals=None, colors=None, use_triangle_normal=False, in_device=False,
                  out_device=False, want_normals=None, device=0):
    """mqr_mesh_sample_points -> (positions, normals or None, colors or None, triangle) as host arrays."""
    from mqr import _lib
    vp = ctypes.c_void_p
    want_normals = (normals is not None or use_triangle_normal) if want_normals is None else want_normals
    ins = {"v": v, "t": t, "n": normals, "c": colors}
    held, p_in = [], {}
    for k, a in ins.items():
        if a is None:
            p_in[k] = None
        elif in_device:
            held.append(_lib.DeviceBuffer.from_array(a, device))
            p_in[k] = held[-1].ptr.value
        else:
            p_in[k] = a.ctypes.data
    m = max(n, 0)
    shapes = {"p": ((m, 3), np.float32), "n": ((m, 3), np.float32) if want_normals else None,
              "c": ((m, 3), np.float32) if colors is not None else None, "t": ((m,), np.int32)}
    outs, p_out = {}, {}
    for k, sd in shapes.items():
        if sd is None:
            outs[k], p_out[k] = None, None
        elif out_device:
            outs[k] = _lib.DeviceBuffer(int(np.prod(sd[0])) * 4, device)
            p_out[k] = outs[k].ptr.value
        else:
            outs[k] = np.empty(*sd)
            p_out[k] = outs[k].ctypes.data
    try:
        _lib.call("mqr_mesh_sample_points", device, vp(p_in["v"]), len(v), vp(p_in["n"]), vp(p_in["c"]), vp(p_in["t"]),
                  len(t), _lib.MQR_DEVICE if in_device else _lib.MQR_HOST, n, seed, int(use_triangle_normal),
                  vp(p_out["p"]), vp(p_out["n"]), vp(p_out["c"]), vp(p_out["t"]),
                  _lib.MQR_DEVICE if out_device else _lib.MQR_HOST)
        if out_device:
            outs = {k: None if b is None else b.to_array(*shapes[k]) for k, b in outs.items()}
    finally:
        for b in held:
            b.free()
    return outs["p"], outs["n"], outs["c"], outs["t"]


def same_bits(got, want, what=""):
    for name, g, w in zip(("positions", "normals", "colors", "triangle"), got, want):
        assert (g is None) == (w is None), (what, name)
        if g is not None:
            assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape)
            assert np.array_equal(g.view(np.uint32), w.view(np.uint32)), (what, name)


@pytest.mark.parametrize("nt", NT)
def test_bit_equal_at_table_and_launch_edges(nt):
    v, t = random_mesh(nt)
    nrm, col = fields(v)
    assert sr.table(v, t)[-1] > 0
    for j, n in enumerate(N):
        seed = SEEDS[(j + nt) % 2]
        got = device_sample(v, t, n, seed, nrm, col)
        same_bits(got, sr.sample(v, t, n, seed, nrm, col), f"nt={nt} n={n} seed={seed}")
        assert got[3].min() >= 0 and got[3].max() < nt


def test_both_seeds_at_the_largest_case():
    v, t = random_mesh(65537)
    for seed in SEEDS:
        same_bits(device_sample(v, t, 100003, seed), sr.sample(v, t, 100003, seed), f"seed={seed}")


def degenerate_mesh():
    """513 random triangles whose first, last and several interior ones (segment edges included) are degenerate."""
    v, t = random_mesh(513, seed=3)
    bad = [0, 1, 100, 255, 256, 257, 400, 511, 512]
    for i, k in enumerate(bad):
        t[k] = [t[k, 0], t[k, 0], t[k, 2]] if i % 2 else [t[k, 0], t[k, 1], t[k, 1]]
    return v, t, np.array(bad)


def span_mesh():
    """Right triangles at the origin with legs 2^-j, j = 0 .. 29 (areas spanning 2^58), several of each,
    shuffled: those below 2^-32 of the largest have weight 0."""
    legs = 2.0 ** -np.repeat(np.arange(30), 9)
    v = [[0, 0, 0]]
    for s in legs:
        v += [[s, 0, 0], [0, s, 0]]
    t = np.array([[0, 2 * j + 1, 2 * j + 2] for j in range(len(legs))], np.int32)
    order = np.random.default_rng(9).permutation(len(t))
    return np.array(v, np.float32), t[order]


def test_degenerate_triangles_are_never_drawn():
    v, t, bad = degenerate_mesh()
    nrm, col = fields(v)
    assert (sr.weights(sr.areas(v, t))[bad] == 0).all()
    got = device_sample(v, t, 100003, 1, nrm, col)
    same_bits(got, sr.sample(v, t, 100003, 1, nrm, col))
    assert not np.isin(got[3], bad).any()


def test_areas_spanning_two_to_the_40_and_more():
    v, t = span_mesh()
    w = sr.weights(sr.areas(v, t))
    assert (w == 0).sum() >= 9 * 10 and w.max() == 2 ** 31 and (w > 0).sum() >= 9 * 16
    for tri_normal in (False, True):
        got = device_sample(v, t, 100003, 0, use_triangle_normal=tri_normal)
        same_bits(got, sr.sample(v, t, 100003, 0, use_triangle_normal=tri_normal))
        assert (w[got[3]] > 0).all()
    assert np.array_equal(got[1], np.tile(np.float32([0, 0, 1]), (100003, 1)))


def test_vertices_at_1e18_scale():
    v, t = random_mesh(4097, seed=5, scale=1e18)
    nrm, col = fields(v)
    assert np.isfinite(sr.areas(v, t)).all() and np.abs(v).max() > 1e18
    for tri_normal in (False, True):
        got = device_sample(v, t, 257, 2 ** 64 - 1, nrm, col, use_triangle_normal=tri_normal)
        same_bits(got, sr.sample(v, t, 257, 2 ** 64 - 1, nrm, col, use_triangle_normal=tri_normal))
        assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()


@pytest.mark.parametrize("with_normals", [False, True])
@pytest.mark.parametrize("with_colors", [False, True])
@pytest.mark.parametrize("tri_normal", [False, True])
def test_option_variants(with_normals, with_colors, tri_normal):
    v, t = random_mesh(257, seed=2)
    nrm, col = fields(v)
    nrm, col = nrm if with_normals else None, col if with_colors else None
    got = device_sample(v, t, 257, 3, nrm, col, use_triangle_normal=tri_normal)
    want = sr.sample(v, t, 257, 3, nrm, col, use_triangle_normal=tri_normal)
    same_bits(got, want, f"normals={with_normals} colors={with_colors} tri_normal={tri_normal}")
    assert (got[1] is not None) == (with_normals or tri_normal) and (got[2] is not None) == with_colors
    if tri_normal:
        assert np.abs(np.linalg.norm(got[1].astype(np.float64), axis=1) - 1.0).max() < 1e-6


def test_residency_and_repeatability():
    from mqr import _lib
    v, t = random_mesh(4097, seed=4)
    nrm, col = fields(v)
    base = device_sample(v, t, 257, 5, nrm, col)
    same_bits(base, sr.sample(v, t, 257, 5, nrm, col))
    same_bits(device_sample(v, t, 257, 5, nrm, col), base, "second call")
    same_bits(device_sample(v, t, 257, 5, nrm, col, in_device=True), base, "device inputs")
    same_bits(device_sample(v, t, 257, 5, nrm, col, out_device=True), base, "device outputs")
    same_bits(device_sample(v, t, 257, 5, nrm, col, in_device=True, out_device=True), base, "device both")
    short = device_sample(v, t, 64, 5, nrm, col)
    same_bits(short, tuple(a[:64] for a in base), "the first 64 samples of n = 257 are n = 64's")
    _lib.call("mqr_mesh_sample_set_flat_search", 1)
    try:
        flat = device_sample(v, t, 257, 5, nrm, col)
    finally:
        _lib.call("mqr_mesh_sample_set_flat_search", 0)
    same_bits(flat, base, "one-level search")
    ms = [ctypes.c_float() for _ in range(3)]
    _lib.call("mqr_mesh_sample_last_ms", 0, *[ctypes.byref(x) for x in ms])
    assert ms[1].value > 0.0 and ms[2].value > 0.0 and ms[0].value >= ms[1].value + ms[2].value - 1e-3


def test_errors_are_reported_before_any_gather():
    from mqr._lib import MqrError
    v, t = random_mesh(257, seed=6)
    with pytest.raises(MqrError, match="no triangles"):
        device_sample(v, t[:0], 10)
    with pytest.raises(MqrError, match="negative"):
        device_sample(v, t, -1)
    flat = t.copy()
    flat[:, 2] = flat[:, 1]
    with pytest.raises(MqrError, match="degenerate"):
        device_sample(v, flat, 10)
    bad_v = v.copy()
    bad_v[7, 1] = np.nan
    with pytest.raises(MqrError, match="not finite"):
        device_sample(bad_v, t, 10)
    bad_t = t.copy()
    bad_t[100, 2] = len(v)
    for in_device in (False, True):
        with pytest.raises(MqrError, match=r"outside \[0, nv\)"):
            device_sample(v, bad_t, 10, in_device=in_device)
    with pytest.raises(MqrError, match="has none"):
        device_sample(v, t, 10, want_normals=True)
    out = np.full((4, 3), 7.0, np.float32)  # n == 0: a successful no-op that writes nothing
    from mqr import _lib
    _lib.call("mqr_mesh_sample_points", 0, ctypes.c_void_p(v.ctypes.data), len(v), None, None,
              ctypes.c_void_p(t.ctypes.data), len(t), _lib.MQR_HOST, 0, 0, 0, ctypes.c_void_p(out.ctypes.data), None,
              None, None, _lib.MQR_HOST)
    assert (out == 7.0).all()


def test_python_mirror_on_host_meshes():
    from mqr.geometry import PointCloud, Tensor, TriangleMesh, device_ptr
    v, t = random_mesh(257, seed=8)
    nrm, col = fields(v)
    mesh = TriangleMesh(v, nrm, t)
    pc = mesh.sample_points_uniformly(300, seed=9)
    assert isinstance(pc, PointCloud) and device_ptr(pc.point.positions) is None and pc.colors is None
    want = sr.sample(v, t, 300, 9, nrm)
    same_bits((pc.points, pc.normals), want[:2])
    mesh.vertex["colors"] = Tensor(col)
    pc = mesh.sample_points_uniformly(300, use_triangle_normal=True, seed=9)
    want = sr.sample(v, t, 300, 9, nrm, col, use_triangle_normal=True)
    same_bits((pc.points, pc.normals, pc.point.colors.numpy()), want[:3])
    for n in (0, -3):
        with pytest.raises(RuntimeError, match="number_of_points"):
            mesh.sample_points_uniformly(n)
    with pytest.raises(RuntimeError, match="no triangles"):
        TriangleMesh(v, nrm, t[:0]).sample_points_uniformly(10)
    bad_v = v.copy()
    bad_v[3, 0] = np.inf
    with pytest.raises(ValueError, match="not finite"):
        TriangleMesh(bad_v, nrm, t).sample_points_uniformly(10)
    bad_t = t.copy()
    bad_t[5, 0] = -1
    with pytest.raises(ValueError, match="outside"):
        TriangleMesh(v, nrm, bad_t).sample_points_uniformly(10)
    flat = t.copy()
    flat[:, 2] = flat[:, 1]
    with pytest.raises(RuntimeError, match="degenerate"):
        TriangleMesh(v, nrm, flat).sample_points_uniformly(10)


def test_python_mirror_reports_device_input_errors_as_value_errors():
    from mqr import _lib
    from mqr.geometry import DeviceArray, Tensor, TriangleMesh
    v, t = random_mesh(257, seed=8)
    bad_t = t.copy()
    bad_t[5, 0] = len(v)  # rejected by the index check, before any gather
    bufs = [_lib.DeviceBuffer.from_array(a) for a in (v, np.zeros_like(v), bad_t)]
    dev = [Tensor(DeviceArray(b, b.ptr.value, a.shape, a.dtype, 0)) for b, a in zip(bufs, (v, v, bad_t))]
    with pytest.raises(ValueError, match="outside"):
        TriangleMesh(*dev, device="HIP:0").sample_points_uniformly(10)


def test_device_mesh_with_misshapen_host_fields_is_rejected_before_any_launch(room, monkeypatch):  # noqa: F811
    """A mesh in HBM whose colours (or normals) are a host tensor is sampled after an upload of that tensor; the
    kernel gathers nv rows from it, so a tensor of another shape is a ValueError and nothing is launched."""
    from mqr import _lib
    from mqr.geometry import Tensor, TriangleMesh, device_ptr
    nv = len(room.vertex.positions)
    assert device_ptr(room.vertex.positions) is not None
    launched = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (launched.append(name), real(name, *a))[1])
    for rows in (nv - 1, 1, nv + 1):
        room.vertex["colors"] = Tensor(np.zeros((rows, 3), np.float32))
        try:
            with pytest.raises(ValueError, match="colors must be"):
                room.sample_points_uniformly(64)
        finally:
            del room.vertex["colors"]
    short = TriangleMesh(room.vertex.positions, Tensor(np.zeros((nv - 1, 3), np.float32)), room.triangle.indices,
                         device=room.device)
    with pytest.raises(ValueError, match="normals must be"):
        short.sample_points_uniformly(64)
    assert "mqr_mesh_sample_points" not in launched and "mqr_memcpy" not in launched
    short.sample_points_uniformly(64, use_triangle_normal=True)  # the vertex normals are then not read
    assert launched.count("mqr_mesh_sample_points") == 1


def ulp32(x):
    return float(np.spacing(np.float32(x)))


def test_room_to_coloured_point_cloud_file(room, tmp_path):  # noqa: F811
    """extract -> colours -> sample_points_uniformly(2 nv) on the device -> color.ply -> read back."""
    from mqr.dataio import ReconstructionDataIO
    from mqr.geometry import Tensor, color_to_uint8, device_ptr, read_ply, read_point_cloud
    v, t, nrm = room.vertices, room.triangles, room.vertex_normals
    nv = len(v)
    assert device_ptr(room.vertex.positions) is not None and nv > 1000
    col = np.random.default_rng(12).random((nv, 3)).astype(np.float32)
    room.vertex["colors"] = Tensor(col)  # as optimize_color_pose attaches them: a host tensor on a device mesh
    try:
        pc = room.sample_points_uniformly(2 * nv, seed=1)
    finally:
        del room.vertex["colors"]
    for field in (pc.point.positions, pc.point.normals, pc.point.colors):  # the cloud stays in HBM
        assert device_ptr(field, device_ptr(room.vertex.positions)[1]) is not None
    assert pc.device == room.device
    want = sr.sample(v, t, 2 * nv, 1, nrm, col)
    same_bits((pc.points, pc.normals, pc.colors), want[:3])

    io = ReconstructionDataIO(tmp_path)
    io.save_colored_pcd_legacy(pc.to_legacy())
    path = tmp_path / "reconstruction" / "color.ply"
    props, faces = read_ply(path)
    assert faces is None and props["x"].dtype == np.float64
    assert np.array_equal(np.stack([props["x"], props["y"], props["z"]], 1), pc.points.astype(np.float64))
    back = read_point_cloud(str(path))
    assert np.array_equal(back.points, pc.points) and np.array_equal(back.normals, pc.normals)
    assert np.array_equal(np.stack([props["red"], props["green"], props["blue"]], 1), color_to_uint8(pc.colors))
    assert np.array_equal(back.colors, (color_to_uint8(pc.colors).astype(np.float64) / 255.0).astype(np.float32))

    # Every sample lies in its triangle's plane up to the float32 rounding of the stored point: the float64
    # blend (wa a + wb b) + wc c is in the plane to ~1e-15, and rounding each coordinate to float32 moves it by
    # at most half an ulp of the largest coordinate magnitude, so the distance is at most sqrt(3) / 2 ulp.
    k = want[3]
    extent = float(np.abs(v).max())
    tol = np.sqrt(3.0) * 0.5 * ulp32(extent) + 1e-12
    assert tol <= 1e-6, (extent, tol)
    V = v.astype(np.float64)
    a, b, c = V[t[k, 0]], V[t[k, 1]], V[t[k, 2]]
    nn = np.cross(b - a, c - a)
    nn /= np.linalg.norm(nn, axis=1)[:, None]
    dist = np.abs(np.einsum("ij,ij->i", pc.points.astype(np.float64) - a, nn))
    print(f"extent {extent:.3f} m, tolerance {tol:.3e}, max plane distance {dist.max():.3e}")
    assert dist.max() <= tol
