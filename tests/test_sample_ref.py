"""The surface-sampling rule itself (tests/sample_ref.py, the numpy restatement of csrc/meshsample.hip, DESIGN
§2.8): the integer pieces against Python integers, the properties the rule promises, and the distribution of
the drawn triangles against the binomial expectation.  No GPU."""
import numpy as np
import pytest

import sample_ref as sr

M64 = 2 ** 64 - 1


def py_splitmix(seed, k):
    z = (seed + k * sr.GOLDEN) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def spread_mesh(seed=5, nt=64, ratio=2700.0):
    """`nt` right triangles of their own vertices with areas 1 .. `ratio` (geometric), then two degenerate ones
    (collinear corners; a repeated corner), all in shuffled order.  -> vertices, triangles, degenerate mask."""
    rng = np.random.default_rng(seed)
    area = ratio ** (np.arange(nt) / (nt - 1))
    leg = np.sqrt(2.0 * area)
    v, t = [], []
    for j in range(nt):
        o = rng.uniform(-50, 50, 3)
        v += [o, o + [leg[j], 0, 0], o + [0, leg[j], 0]]
        t.append([3 * j, 3 * j + 1, 3 * j + 2])
    b = len(v)
    v += [[0, 0, 0], [1, 1, 1], [2, 2, 2], [5, 5, 5], [6, 5, 5]]
    t += [[b, b + 1, b + 2], [b + 3, b + 4, b + 3]]
    v, t = np.asarray(v, np.float32), np.asarray(t, np.int32)
    order = rng.permutation(len(t))
    return v, t[order], (order >= nt)


def test_arguments_are_rejected_before_any_device_is_touched():
    """What the product refuses from its arguments alone, on a machine without a GPU: the Python method's
    checks of a host mesh and the C entry's size checks come before the first device call."""
    import ctypes
    from mqr import _lib
    from mqr.geometry import Tensor, TriangleMesh
    v, t, _ = spread_mesh()
    nrm = np.zeros_like(v)
    mesh = TriangleMesh(v, nrm, t)
    for n in (0, -1):
        with pytest.raises(RuntimeError, match="number_of_points"):
            mesh.sample_points_uniformly(n)
    with pytest.raises(RuntimeError, match="no triangles"):
        TriangleMesh(v, nrm, t[:0]).sample_points_uniformly(10)
    bad = v.copy()
    bad[4, 2] = np.nan
    with pytest.raises(ValueError, match="not finite"):
        TriangleMesh(bad, nrm, t).sample_points_uniformly(10)
    far = t.copy()
    far[3, 1] = len(v)
    with pytest.raises(ValueError, match="outside"):
        TriangleMesh(v, nrm, far).sample_points_uniformly(10)
    mesh.vertex["colors"] = Tensor(np.zeros((len(v) - 1, 3), np.float32))  # one row short
    with pytest.raises(ValueError, match="colors must be"):
        mesh.sample_points_uniformly(10)
    with pytest.raises(ValueError, match="normals must be"):
        TriangleMesh(v, nrm[:5], t).sample_points_uniformly(10)

    vp, out = ctypes.c_void_p, np.empty((4, 3), np.float32)

    def c_call(nv, nt, n):
        _lib.call("mqr_mesh_sample_points", 0, vp(v.ctypes.data), nv, None, None, vp(t.ctypes.data), nt, _lib.MQR_HOST,
                  n, 0, 0, vp(out.ctypes.data), None, None, None, _lib.MQR_HOST)

    for args, msg in (((len(v), 0, 4), "no triangles"), ((len(v), len(t), -1), "negative"),
                      ((len(v), 2 ** 31, 4), "too large"), ((2 ** 31, len(t), 4), "too large")):
        with pytest.raises(_lib.MqrError, match=msg):
            c_call(*args)
    c_call(len(v), len(t), 0)  # n == 0: a successful no-op


def test_mulhi64_against_python_integers():
    rng = np.random.default_rng(0)
    a = rng.integers(0, 2 ** 64, 1000, dtype=np.uint64)
    b = rng.integers(0, 2 ** 64, 1000, dtype=np.uint64)
    a[:4] = [0, M64, M64, 1]
    b[:4] = [M64, M64, 1, 1]
    got = sr.mulhi64(a, b)
    assert [int(x) for x in got] == [(int(x) * int(y)) >> 64 for x, y in zip(a, b)]


def test_splitmix64_known_outputs():
    # the generator's published first outputs for seed 0
    known = [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    assert [int(x) for x in sr.splitmix64(0, np.arange(1, 4))] == known
    assert [py_splitmix(0, k) for k in (1, 2, 3)] == known
    for seed in (1, 7, M64, 0x0123456789ABCDEF):
        ks = [1, 2, 3, 1000, 3 * 100003 + 3]
        assert [int(x) for x in sr.splitmix64(seed, np.array(ks, np.uint64))] == [py_splitmix(seed, k) for k in ks]


def test_sample_is_independent_of_n():
    v, t, _ = spread_mesh()
    nrm = np.random.default_rng(1).standard_normal(v.shape).astype(np.float32)
    col = np.random.default_rng(2).random(v.shape).astype(np.float32)
    small = sr.sample(v, t, 100, 3, nrm, col)
    big = sr.sample(v, t, 1000, 3, nrm, col)
    for a, b in zip(small, big):
        assert np.array_equal(a.view(np.uint32), b[:100].view(np.uint32))
    assert not np.array_equal(small[3], sr.sample(v, t, 100, 4)[3])  # the seed matters


def test_zero_area_triangles_are_never_chosen():
    v, t, degenerate = spread_mesh()
    assert degenerate.sum() == 2 and (sr.weights(sr.areas(v, t))[degenerate] == 0).all()
    for seed in (0, 1, 7):
        k = sr.sample(v, t, 200000, seed)[3]
        assert not degenerate[k].any()
    # degenerate triangles first and last in the table: the search never lands on them either
    order = np.argsort(~degenerate, kind="stable")
    t2 = np.concatenate([t[order][:1], t[order][2:], t[order][1:2]])
    k = sr.sample(v, t2, 200000, 0)[3]
    assert k.min() >= 1 and k.max() <= len(t2) - 2


def test_barycentric_weights_of_a_single_triangle():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    t = np.array([[0, 1, 2]], np.int32)
    k, r1, r2 = sr.choose(sr.table(v, t), 100000, 11)
    assert (k == 0).all()
    wa, wb, wc = sr.barycentric(r1, r2)
    assert (wa >= 0).all() and (wb >= 0).all() and (wc >= 0).all()
    assert np.abs((wa + wb) + wc - 1.0).max() <= 2.0 ** -52  # one ulp of 1
    pos = sr.sample(v, t, 100000, 11)[0]
    assert (pos >= 0).all() and (pos[:, 0] + pos[:, 1] <= 1.0 + 2.0 ** -23).all() and (pos[:, 2] == 0).all()
    # extreme words: u = 0 gives corner a, u1 = u2 = 1 - 2^-53 stays inside
    wa, wb, wc = sr.barycentric(np.array([0, M64], np.uint64), np.array([0, M64], np.uint64))
    assert (wa[0], wb[0], wc[0]) == (1.0, 0.0, 0.0) and wa[1] >= 0 and wb[1] >= 0


@pytest.mark.parametrize("seed", [0, 1, 7])
def test_triangle_counts_are_binomial(seed):
    """Every non-degenerate triangle's count within 5 sigma of Binomial(n, w_t / total)."""
    v, t, degenerate = spread_mesh()
    area = sr.areas(v, t)
    assert area[~degenerate].max() / area[~degenerate].min() >= 1000
    n = 200000
    w = sr.weights(area).astype(np.float64)
    p = w / w.sum()
    k = sr.sample(v, t, n, seed)[3]
    count = np.bincount(k, minlength=len(t))
    sigma = np.sqrt(n * p * (1 - p))
    z = np.abs(count - n * p)[~degenerate] / sigma[~degenerate]
    print(f"seed {seed}: max |z| = {z.max():.2f}")
    assert (z <= 5.0).all()


def test_tiny_triangle_has_weight_zero():
    assert list(sr.weights(np.array([1.0, 2.0 ** -33, 2.0 ** -31, 2.0 ** -32]))) == [2 ** 31, 0, 1, 0]
    # as a mesh: legs 1 x 2 (area 1, the largest) and legs 2^-16 x 2^-16 (area 2^-33)
    s = 2.0 ** -16
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 2, 0], [4, 0, 0], [4 + s, 0, 0], [4, s, 0]], np.float32)
    t = np.array([[3, 4, 5], [0, 1, 2]], np.int32)
    area = sr.areas(v, t)
    assert area[1] == 1.0 and area[0] == 2.0 ** -33
    assert list(sr.table(v, t)) == [0, 2 ** 31]
    assert (sr.sample(v, t, 10000, 0)[3] == 1).all()
    # weights stay below 2^32 whatever the scale
    for scale in (1e-30, 1.0, 1e30):
        w = sr.weights(np.array([0.999999, 0.5, 1e-3]) * scale)
        assert w.max() < 2 ** 32 and w.max() >= 2 ** 31
