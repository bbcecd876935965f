"""The float32 restatement of the ray caster's primitive test (tests/raycast_ref.py) against the
float64 oracle, and the shape of the constructed scenes.  No GPU: tests/test_gpu_raycast_cases.py casts
the same scenes on the device against the restatement.

On the exact scenes float32 and float64 arithmetic are both exact, so the restatement and the oracle
must agree bit for bit: any difference is a mistake in the restatement."""
import numpy as np
import pytest

import oracle
import raycast_ref as rr


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("scene", rr.exact_scenes(), ids=lambda s: s.name)
def test_restatement_equals_oracle_on_exact_scenes(scene):
    assert scene.exact
    P, _, _ = scene.soup()
    ref = rr.brute_force(P, scene.rays)
    V, T = scene.merged()
    assert np.array_equal(V[T], P)
    t, prim = oracle.raycast(V, T, scene.rays)
    assert np.array_equal(_bits(t), _bits(ref.t))
    assert np.array_equal(prim, ref.first())   # the oracle keeps the first triangle of a tie
    assert np.all(np.isinf(ref.t) | ((ref.t > 0) & np.isfinite(ref.t)))
    if scene.all_hit:
        assert np.all(np.isfinite(ref.t))


def test_exact_scenes_cover_what_they_claim():
    by = {s.name: s for s in rr.exact_scenes()}
    refs = {k: rr.brute_force(s.soup()[0], s.rays) for k, s in by.items() if not k.startswith("same_centroid")}
    # the cube from inside: ties of two (edges, the face diagonal) and of three and more (vertices)
    ref = refs["cube_inside"]
    sizes = np.bincount(ref.ray, minlength=len(ref.t))
    assert sizes.min() >= 1 and {1, 2}.issubset(set(sizes)) and sizes.max() >= 3
    # axis-parallel rays: both signs of zero, origins in the plane of a face, and every ray hits
    s = by["axis_parallel"]
    d = s.rays[:, 3:]
    assert np.all((d == 0).sum(axis=1) == 2) and np.signbit(d[d == 0]).any() and not np.signbit(d[d == 0]).all()
    assert np.isfinite(refs["axis_parallel"].t).all()
    # hits on every bound of the triangle, hits behind a t = 0 triangle, and misses
    ref, s = refs["bounds"], by["bounds"]
    on_a = ref.tri == 0
    assert (ref.u[on_a] == 0).any() and (ref.v[on_a] == 0).any() and (ref.u[on_a] + ref.v[on_a] == 1).any()
    start_on_a = (s.rays[:, 2] == 1) & np.all(s.rays[:, 3:] == [0, 0, 1], axis=1)
    assert start_on_a.sum() == 3 and np.all(ref.t[start_on_a] == 1) and np.all(ref.first()[start_on_a] == 1)
    zero_d = np.all(s.rays[:, 3:] == 0, axis=1)
    assert zero_d.sum() == 3 and np.isinf(ref.t[zero_d]).all() and np.isinf(ref.t).sum() > 12
    # ties: sets of five (the coincident and duplicated triangles) and of two (the shared edge)
    sizes = np.bincount(refs["ties"].ray, minlength=len(refs["ties"].t))
    assert {0, 1, 2, 5}.issubset(set(sizes))
    # degenerate triangles are never hit and change nothing
    ref, s = refs["cube_degenerates"], by["cube_degenerates"]
    assert np.all(s.extra["cube_prim"][ref.tri] >= 0)
    assert np.array_equal(_bits(ref.t), _bits(refs["cube_inside"].t))
    # the outlier collapses every other centroid into one Morton cell
    keys = rr.morton_keys(by["grid_box_outlier"].soup()[0])
    assert len(np.unique(keys)) == 2 and (keys == keys.min()).sum() == len(keys) - 1
    # all three geometries' hits occur; the middle geometry has no triangle
    s = by["three_geometries"]
    _, gid, _ = s.soup()
    assert len(s.geoms[1][1]) == 0 and set(gid[refs["three_geometries"].tri]) == {0, 2}


@pytest.mark.parametrize("n", rr.SAME_CENTROID_N)
def test_same_centroid_scenes_have_one_morton_key(n):
    s = rr.same_centroid(n)
    P, _, _ = s.soup()
    assert len(P) == n
    assert np.all(rr.morton_keys(P) == 0)
    ref = rr.brute_force(P, s.rays)
    assert np.isfinite(ref.t).any() and (n > 3 or np.isinf(ref.t).any())


def test_ladder_tree_is_deeper_than_the_traversal_stack_was():
    """k_morton's keys of the ladder are 2^0 .. 2^62 (two each), 0 (sixteen) and 2^63 - 1, the Karras tree
    over them has a chain of more than 64 nodes whose children are both internal, every box contains
    every ray's origin, and every triangle is the unique nearest hit of its own ray."""
    s = rr.ladder()
    P, _, _ = s.soup()
    n = len(P)
    assert n == 143
    keys = rr.morton_keys(P)
    want = sorted([0] * 16 + [1 << b for b in range(63)] * 2 + [(1 << 63) - 1])
    assert sorted(int(k) for k in keys) == want
    order = np.argsort(keys, kind="stable")
    deepest, need = rr.tree_depths(rr.karras_tree(keys[order]))
    assert need > 64 and deepest > 64, (deepest, need)
    assert deepest < 96
    lo, hi = P.min(axis=1), P.max(axis=1)
    for r in s.rays:
        assert np.all(lo < r[:3]) and np.all(r[:3] < hi)
    ref = rr.brute_force(P, s.rays)
    assert np.array_equal(np.bincount(ref.ray, minlength=n), np.ones(n, np.int64))
    assert np.array_equal(ref.tri, np.arange(n))
    # ... by a margin far above float32 rounding of t (a few units at these magnitudes)
    t_all, _, _ = rr._tri_test(P, s.rays[:, :3], s.rays[:, 3:])
    second = np.sort(t_all, axis=1)[:, 1]
    assert np.all(second - ref.t > 16.0), float((second - ref.t).min())


def test_generic_scene_shape():
    s = rr.generic()
    P, gid, _ = s.soup()
    assert len(P) == 1012 and (gid == 1).sum() == 512 and not s.exact
    assert len(s.rays) == 7 * 1012 + 2048
    ref = rr.brute_force(P, s.rays)
    hit = np.isfinite(ref.t)
    assert 0.5 < hit.mean() < 1.0
    assert np.all(hit[6 * 1012:7 * 1012])   # a ray aimed at a centroid hits that triangle or one before it


def test_pinhole_rays_general_intrinsics():
    """create_rays_pinhole with skew and K[2, 2] != 1 (the adjugate inverse the device path uses too):
    the directions are R^T K^-1 (x + 0.5, y + 0.5, 1) to float32 rounding."""
    from mqr.raycasting import RaycastingScene
    K = np.array([[9.0, 0.375, 5.25], [0.0, 8.5, 4.75], [0.0, 0.0, 1.25]])
    a = 0.3
    T = np.eye(4)
    T[:3, :3] = [[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]]
    T[:3, 3] = [0.1, -0.3, 5.0]
    rays = RaycastingScene.create_rays_pinhole(K, T, 13, 11).numpy()
    assert rays.shape == (11, 13, 6) and rays.dtype == np.float32
    x, y = np.meshgrid(np.arange(13) + 0.5, np.arange(11) + 0.5)
    want = np.stack([x, y, np.ones_like(x)], axis=-1) @ (T[:3, :3].T @ np.linalg.inv(K)).T
    assert np.abs(rays[..., 3:] - want).max() < 1e-6 * np.abs(want).max()
    assert np.abs(rays[..., :3] - (-T[:3, :3].T @ T[:3, 3])).max() < 1e-6
