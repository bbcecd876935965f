"""Ray casting on constructed scenes (tests/raycast_ref.py), exactly.

The rule, on every ray and with no share left out: t_hit is bit-identical to the float32 brute-force
restatement of the kernel's own primitive test; primitive_ids names a triangle of the minimal-t set
and geometry_ids the geometry it belongs to; primitive_uvs is bit-identical to the restatement's for
that triangle; a miss is inf / INVALID_ID.  The restatement has no tree, so this isolates the build, the
box test, the pruning and the traversal stack from the primitive test's own rounding.  On the exact
scenes (dyadic coordinates, directions of 0 and powers of two) the float64 oracle must agree bit for
bit too.  tests/test_raycast_ref.py holds the restatement to the oracle without a device.

Against the kernel before the box test chose its planes by the direction's sign, before the pruning got
the box test's slack and before the stack was sized to the admitted depth, 15 of these 30 failed on an
MI355X, with the counts a float32 CPU emulation of that traversal gives as well:
- a zero direction component with the origin on a box bound (0 * inf = NaN culled the box; misses
  returned for hits): axis_parallel 2160 of 2352 rays, bounds 25 of 81, ties 16 of 72, three_geometries
  179 of 1875, all_centroids_identical 52 / 102 / 130 of 3267 for n = 2 / 3 / >= 255 (and the last check
  of the out-of-range test, which casts the ties scene);
- pruning without the box test's slack: generic 12 of 9132 rays, 1 ulp farther than brute force;
- the 64-entry stack: ladder 8 of 143 rays, a farther triangle's depth returned without any error.
"""
import numpy as np
import pytest

import oracle
import raycast_ref as rr

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _scene(scene):
    from mqr.raycasting import RaycastingScene
    s = RaycastingScene()
    for g, (v, t) in enumerate(scene.geoms):
        assert s.add_triangles(v, t) == g
    return s


def _same_bits(got, want, what):
    bad = np.flatnonzero(_bits(got) != _bits(want))
    assert bad.size == 0, (f"{what}: {bad.size} of {got.size} differ; first at {bad[:8]}: "
                           f"got {np.asarray(got).ravel()[bad[:8]]}, want {np.asarray(want).ravel()[bad[:8]]}")


def _check(scene, out, ref=None):
    """The comparison rule of the module docstring on one cast's outputs."""
    from mqr.raycasting import INVALID_ID
    P, gid, pid = scene.soup()
    if ref is None:
        ref = rr.brute_force(P, scene.rays)
    t = out["t_hit"].numpy().reshape(-1)
    g = out["geometry_ids"].numpy().reshape(-1)
    p = out["primitive_ids"].numpy().reshape(-1)
    uv = out["primitive_uvs"].numpy().reshape(-1, 2)
    print(f"{scene.name}: {len(t)} rays, {int(np.isfinite(ref.t).sum())} hits, "
          f"{int((_bits(t) != _bits(ref.t)).sum())} t differ")
    _same_bits(t, ref.t, f"{scene.name} t_hit vs float32 brute force")
    if scene.all_hit:
        assert np.isfinite(t).all()
    miss = np.isinf(ref.t)
    assert np.all(g[miss] == INVALID_ID) and np.all(p[miss] == INVALID_ID)
    hit = np.flatnonzero(~miss)
    nt = np.array([len(tt) for _, tt in scene.geoms])
    assert np.all(g[hit] < len(nt))
    assert np.all(p[hit] < nt[g[hit]])
    base = np.concatenate([[0], np.cumsum(nt)])[:-1]
    tri = base[g[hit]] + p[hit]
    assert np.array_equal(gid[tri], g[hit]) and np.array_equal(pid[tri], p[hit])
    at = ref.lookup(hit, tri)
    assert np.all(at >= 0), f"{scene.name}: {(at < 0).sum()} reported primitives are not in the minimal-t set"
    _same_bits(uv[hit, 0], ref.u[at], f"{scene.name} u")
    _same_bits(uv[hit, 1], ref.v[at], f"{scene.name} v")
    if scene.exact:
        V, T = scene.merged()
        ot, _ = oracle.raycast(V, T, scene.rays)
        _same_bits(t, ot, f"{scene.name} t_hit vs the float64 oracle")
    return ref


@pytest.mark.parametrize("build", [rr.cube_inside, rr.axis_parallel, rr.grid_box_oblique,
                                   rr.bounds_and_degenerate_relations, rr.ties, rr.three_geometries],
                         ids=lambda f: f.__name__)
def test_exact_scene(build):
    scene = build()
    _check(scene, _scene(scene).cast_rays(scene.rays))


def test_degenerate_triangles_are_never_hit_and_change_nothing():
    scene, plain = rr.cube_with_degenerates(), rr.cube_inside()
    out = _scene(scene).cast_rays(scene.rays)
    _check(scene, out)
    assert np.array_equal(scene.rays, plain.rays)
    want = _scene(plain).cast_rays(plain.rays)
    _same_bits(out["t_hit"].numpy(), want["t_hit"].numpy(), "t_hit with and without the degenerate triangles")
    back = scene.extra["cube_prim"][out["primitive_ids"].numpy()]
    assert np.all(back >= 0)
    # the same triangle wherever the other scene's answer is not a tie-break between equal hits
    ref = rr.brute_force(plain.soup()[0], plain.rays)
    single = np.bincount(ref.ray, minlength=len(ref.t)) == 1
    assert single.any() and np.array_equal(back[single], want["primitive_ids"].numpy()[single])


@pytest.mark.parametrize("n", rr.SAME_CENTROID_N)
def test_all_centroids_identical(n):
    scene = rr.same_centroid(n)
    _check(scene, _scene(scene).cast_rays(scene.rays))


def test_far_outlier_collapses_morton_cells():
    scene = rr.grid_box_oblique(outlier=True)
    _check(scene, _scene(scene).cast_rays(scene.rays))


@pytest.mark.parametrize("index", [10, -1, np.iinfo(np.int32).max])
def test_triangle_index_out_of_range_raises(index):
    from mqr.raycasting import RaycastingScene
    good = rr.ties()
    v, t = good.geoms[0]
    assert len(v) == 10   # 10 is the first index past the vertex array
    bad_t = t.copy()
    bad_t[3, 1] = index
    s = RaycastingScene()
    s.add_triangles(v, bad_t)
    for _ in range(2):   # the scene object stays usable: it reports the same error again
        with pytest.raises(RuntimeError, match="out of range"):
            s.cast_rays(good.rays)
        with pytest.raises(RuntimeError, match="out of range"):
            s.cast_pinhole(np.eye(3), np.eye(4), 4, 4)
        assert s.triangle_count() == len(t)
    _check(good, _scene(good).cast_rays(good.rays))   # and so does the library


@pytest.fixture(scope="module")
def generic():
    scene = rr.generic()
    return scene, rr.brute_force(scene.soup()[0], scene.rays)


def test_generic_scene_equals_float32_brute_force(generic):
    scene, ref = generic
    _check(scene, _scene(scene).cast_rays(scene.rays), ref)


def test_ladder_deep_tree():
    """A tree with 66 nested nodes whose children are both internal, every box entered at t = 0: the
    result equals brute force on every ray, or the build refuses the tree.  A silently wrong depth is
    the failure."""
    scene = rr.ladder()
    s = _scene(scene)
    try:
        out = s.cast_rays(scene.rays)
    except RuntimeError as e:
        assert "deeper" in str(e)
        return
    ref = _check(scene, out)
    assert np.array_equal(out["primitive_ids"].numpy(), np.arange(len(scene.rays)))
    assert np.array_equal(ref.tri, np.arange(len(scene.rays)))


def _cameras(nf):
    Ks, Ts = [], []
    for f in range(nf):
        # skew, and K[2, 2] != 1: the general inverse
        K = np.array([[9.0 + f, 0.375, 5.25 - f], [0.0, 8.5, 4.75 + 0.5 * f], [0.0, 0.0, 1.25]])
        a, b = 0.3 + 0.2 * f, -0.2 + 0.15 * f
        Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
        Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
        T = np.eye(4)
        T[:3, :3] = Rx @ Ry
        T[:3, 3] = [0.1 - 0.2 * f, -0.3, 5.0 + 0.25 * f]
        Ks.append(K)
        Ts.append(T)
    return np.array(Ks), np.array(Ts)


@pytest.mark.parametrize("nf", [1, 3])
@pytest.mark.parametrize("W,H", [(1, 1), (7, 9), (8, 8), (9, 8), (13, 11)])
def test_pinhole_equals_rays(generic, W, H, nf):
    """cast_pinhole == create_rays_pinhole + cast_rays, bit for bit, on image sizes around the 8 x 8 wave
    tile, with a K that takes the general-inverse branch; both equal brute force on those rays."""
    from mqr.raycasting import RaycastingScene
    scene, _ = generic
    s = _scene(scene)
    K, T = _cameras(nf)
    assert K[0, 0, 1] != 0 and K[0, 2, 2] != 1
    fused = s.cast_pinhole(K, T, W, H, full=True)
    rays = np.stack([RaycastingScene.create_rays_pinhole(K[f], T[f], W, H).numpy() for f in range(nf)])
    assert rays.shape == (nf, H, W, 6) and fused["t_hit"].numpy().shape == (nf, H, W)
    split = s.cast_rays(rays)
    for k in ("t_hit", "primitive_uvs", "primitive_normals"):
        _same_bits(fused[k].numpy(), split[k].numpy(), f"{k}, fused vs explicit rays")
    for k in ("geometry_ids", "primitive_ids"):
        assert np.array_equal(fused[k].numpy(), split[k].numpy())
    cams = rr.Scene("pinhole", scene.geoms, rays.reshape(-1, 6), exact=False)
    _check(cams, fused)
    if nf == 1:   # a single camera is passed unstacked as well
        one = s.cast_pinhole(K[0], T[0], W, H, full=True)
        assert one["t_hit"].numpy().shape == (H, W)
        _same_bits(one["t_hit"].numpy(), fused["t_hit"].numpy(), "single camera vs a stack of one")
    if (W, H) == (13, 11):
        assert np.isfinite(fused["t_hit"].numpy()).any() and np.isinf(fused["t_hit"].numpy()).any()


def test_t_hit_does_not_depend_on_the_optional_outputs(generic):
    """The ids, uvs and normals are optional outputs (four optional pieces of the casts' staging block when
    the results go to the host): t_hit is the same bits with and without them, for both casts, with the
    results left in HBM (the Python layer) and staged to host arrays (the C entry points)."""
    from mqr import _lib
    from mqr._lib import MQR_HOST, call, ptr
    from mqr.raycasting import RaycastingScene
    scene, _ = generic
    s = _scene(scene)
    W, H, nf = 7, 9, 3
    K, T = _cameras(nf)
    full = s.cast_pinhole(K, T, W, H, full=True)["t_hit"].numpy()
    assert np.isfinite(full).any()
    _same_bits(s.cast_pinhole(K, T, W, H, full=False)["t_hit"].numpy(), full, "cast_pinhole, full=False vs True")
    rays = np.stack([RaycastingScene.create_rays_pinhole(K[f], T[f], W, H).numpy() for f in range(nf)])
    _same_bits(s.cast_rays(rays, full=True)["t_hit"].numpy(), full, "cast_rays, full=True vs the pinhole cast")
    _same_bits(s.cast_rays(rays, full=False)["t_hit"].numpy(), full, "cast_rays, full=False vs True")
    # host outputs: t_hit alone, then with every optional output
    n = nf * H * W
    r = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
    Kc, Tc = np.ascontiguousarray(K, np.float64), np.ascontiguousarray(T, np.float64)
    for with_optional in (False, True):
        opt = [np.empty(n, np.uint32), np.empty(n, np.uint32), np.empty((n, 2), np.float32),
               np.empty((n, 3), np.float32)] if with_optional else [None] * 4
        po = [None if a is None else ptr(a) for a in opt]
        t = np.empty(n, np.float32)
        call("mqr_scene_cast_pinhole", s._h, ptr(Kc, _lib._f64p), ptr(Tc, _lib._f64p), nf, H, W, ptr(t), *po, MQR_HOST)
        _same_bits(t.reshape(nf, H, W), full, f"cast_pinhole to the host, optional outputs {with_optional}")
        t = np.empty(n, np.float32)
        call("mqr_scene_cast_rays", s._h, ptr(r), n, MQR_HOST, ptr(t), *po, MQR_HOST)
        _same_bits(t.reshape(nf, H, W), full, f"cast_rays to the host, optional outputs {with_optional}")
