"""The numpy reference of the colour-map optimisation rules (tests/colormap_ref.py) on known
answers, and the conditions that make exact and tight comparisons with the kernels meaningful on the
inputs tests/test_gpu_colormap.py uses: the pair counts cover every reduction path, every stability
margin is far above float64 rounding, and the summation-order sensitivity of the poses is far below the
movement the GPU test checks.  CPU only."""
import numpy as np
import pytest

import colormap_ref as cr

ITERS = 30  # the most iterations any GPU test runs on these inputs


def _plane_scene(images_fn, n=3, H=48, W=64, z=1.5, f=60.0, stride=2):
    """n keyframes in front of the wall Z = z, translated along x; vertices on the wall."""
    K = np.array([[f, 0, (W - 1) / 2.0], [0, f, (H - 1) / 2.0], [0, 0, 1.0]])
    T = np.stack([np.eye(4) for _ in range(n)])
    T[:, 0, 3] = -0.05 * (np.arange(n) - (n - 1) / 2.0)  # world -> camera: the camera sits at +0.05 (c - 1)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    images = []
    for c in range(n):
        X = np.stack([(x - K[0, 2]) / f * z - T[c, 0, 3], (y - K[1, 2]) / f * z, np.full_like(x, z)], -1)
        g = np.clip(np.round(images_fn(X) * 255.0), 0, 255).astype(np.uint8)
        images.append(np.repeat(g[..., None], 3, -1))
    t_hit = np.full((n, H, W), z, np.float32)
    V = np.stack([((x - K[0, 2]) / f * z)[::stride, ::stride].ravel() + 0.003,
                  ((y - K[1, 2]) / f * z)[::stride, ::stride].ravel() + 0.002,
                  np.full(x[::stride, ::stride].size, z)], 1).astype(np.float32)
    return V, np.stack(images), t_hit, np.repeat(K[None], n, 0), T


def test_constant_image_keeps_poses():
    V, images, t_hit, K, T = _plane_scene(lambda X: np.full(X.shape[:2], 0.5))
    ref = cr.Reference(V, images, t_hit, K, T)
    assert (ref.pairs_per_keyframe > 100).all()
    JTJ, JTr, r2, cnt = ref.systems()
    assert (cnt > 100).all() and np.all(JTJ == 0.0) and np.all(JTr == 0.0) and np.all(r2 == 0.0)
    res, _, _, moved, _ = ref.optimize(2)
    assert not moved.any() and np.array_equal(ref.E, T) and np.all(res == 0.0)


def test_linear_ramp_gradient_and_jacobian():
    """A ramp of `slope` grey per pixel along x: the unnormalised Sobel of §2.4 ({-1, 0, 1} x {1, 2, 1},
    taps summing to 8 per unit slope) gives dx = 8 slope in the interior and dy = 0 -- 'dIdx = slope' in
    Sobel units, the scale run_rigid_optimizer's Jacobian uses -- and J of one vertex is the hand-computed
    vector."""
    H, W, f, z = 48, 64, 60.0, 1.5
    K = np.array([[f, 0, (W - 1) / 2.0], [0, f, (H - 1) / 2.0], [0, 0, 1.0]])
    ramp = np.tile((20 + 3 * np.arange(W)).astype(np.uint8), (H, 1))  # slope 3 / 255 per pixel
    images = np.repeat(ramp[None, :, :, None], 3, -1)
    gray, dx, dy = cr.utility_images(images)
    slope = 3.0 / 255.0
    assert np.abs(dx[0, 2:-2, 2:-2] - 8 * slope).max() < 1e-6
    assert np.abs(dy[0, 2:-2, 2:-2]).max() < 1e-6
    assert np.abs(gray[0, 2:-2, 2:-2] - ramp[2:-2, 2:-2] / 255.0).max() < 1e-6
    V = np.array([[0.21, -0.13, z]], np.float32)
    T = np.eye(4)[None].copy()
    T[0, :3, 3] = (0.01, 0.02, 0.03)
    ref = cr.Reference(V, images, np.full((1, H, W), z + 0.03, np.float32), K[None], T)
    assert list(ref.pairs_per_keyframe) == [1]
    t = ref.terms(0)
    assert t.shape == (1, 29) and t[0, 0] == 1.0
    gx, gy, gz = (float(V[0, a]) + T[0, a, 3] for a in range(3))
    v0 = 8 * slope * f / gz
    v2 = -(v0 * gx) / gz
    J = np.array([gy * v2, gz * v0 - gx * v2, -gy * v0, v0, 0.0, v2])
    want = np.array([J[a] * J[b] for a in range(6) for b in range(a, 6)])
    assert np.allclose(t[0, 8:], want, rtol=1e-5, atol=1e-9), (t[0, 8:], want)
    # the residual against the nearest-pixel proxy of the same image: bilinear - nearest of a ramp
    u = f * gx / gz + K[0, 2]
    assert abs(np.sqrt(t[0, 1]) - abs(u - np.floor(u + 0.5)) * slope) < 1e-6


def test_true_poses_residual_does_not_grow():
    """Texture-consistent images at the true poses: iterating leaves the residual where it is or lower."""
    tex = lambda X: 0.5 + 0.25 * np.sin(9.0 * X[..., 0] + 0.3) + 0.2 * np.sin(7.0 * X[..., 1] + 1.0)  # noqa: E731
    V, images, t_hit, K, T = _plane_scene(tex)
    ref = cr.Reference(V, images, t_hit, K, T)
    res, cnt, _, moved, _ = ref.optimize(10)
    assert moved.all() and (cnt > 300).all()
    assert res[-1] <= res[0], res
    assert res.max() <= res[0], res


def test_masks_match_the_oracle():
    import oracle
    d = cr.gpu_test_inputs()["odd"]
    m = cr.boundary_masks(d["t_hit"], 3.0, 0.1, 3)
    for c in (0, 4):
        dep, om = oracle.depth_boundary_mask(d["t_hit"][c], 3.0, 0.1, 3)
        assert np.array_equal(m[c], om) and np.array_equal(cr.truncated_depth(d["t_hit"][c], 3.0), dep)


@pytest.mark.parametrize("name", ["even", "odd"])
def test_gpu_inputs_cover_the_reduction_paths(name):
    d = cr.gpu_test_inputs()[name]
    assert d["images"].shape[:3] == ((6, 96, 128) if name == "even" else (6, 97, 131))
    assert 2000 < len(d["V"]) < 8000 and len(d["V"]) % 256 != 0
    pairs = cr.reference_run(name, ITERS)["init"]["pairs"]
    assert pairs[5] == 0, "the keyframe looking away"
    assert 1 <= pairs[4] <= 63, "a single partial wave"
    assert any(p > 256 and p % 256 for p in pairs), "a partial last chunk"
    assert pairs.max() > 1024, "several chunks"


@pytest.mark.parametrize("name", ["even", "odd"])
def test_stability_margins(name):
    run = cr.reference_run(name, ITERS)
    init = run["init"]
    for k, v in list(init["margins"].items()) + list(init["system_margins"].items()):
        assert v >= 1e-7, (k, v)
    for it, m in enumerate(run["margins"]):
        for k, v in m.items():
            assert v >= 1e-7, (it, k, v)


def test_order_sensitivity():
    """s: the largest pose difference after 5 iterations between list-order and reversed-order sums; m: the
    smallest movement of a keyframe that moved.  Measured 1.7e-14 / 4.8e-14 and 1.7e-4 / 2.0e-4 (even /
    odd); recorded as S_ORDER and M_MOVE."""
    s, m = 0.0, np.inf
    for name in ("even", "odd"):
        a, b = cr.reference_run(name, 5), cr.reference_run(name, 5, "reversed")
        assert np.array_equal(a["counts"], b["counts"])
        s = max(s, float(np.abs(a["ref"].E - b["ref"].E).max()))
        m = min(m, float(a["movement"][a["moved"]].min()))
        kept = ~a["moved"].any(0)
        assert list(kept) == [False] * 5 + [True]
        assert np.array_equal(a["ref"].E[kept], a["ref"].E0[kept])
    print(f"order sensitivity s = {s:.3e}, smallest movement m = {m:.3e}")
    assert s <= cr.S_ORDER, s
    assert m >= cr.M_MOVE, m
    assert 1000 * s <= 1e-3 * m
    assert 1000 * cr.S_ORDER <= 1e-3 * cr.M_MOVE


@pytest.mark.parametrize("name", ["even", "odd"])
def test_reference_converges(name):
    d = cr.gpu_test_inputs()[name]
    run = cr.reference_run(name, ITERS)
    ref = run["ref"]
    e0, e1 = cr.pose_error(ref, d["T_pert"], d["T_true"]), cr.pose_error(ref, ref.E, d["T_true"])
    print(f"{name}: residual {run['residuals'][0]:.5f} -> {run['residuals'][-1]:.5f}, pose error {e0:.3f} -> {e1:.3f} px")
    assert cr.converged(ref, d["T_pert"], ref.E, d["T_true"], run["residuals"])
    assert e1 < 0.7 * e0
