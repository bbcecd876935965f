"""Known answers for the numpy restatement of the coloured volume's rule (tests/colorvolume_ref.py, DESIGN.md
§2.11), on the CPU: what the GPU tests (tests/test_gpu_color_volume.py) compare the kernels with."""
import numpy as np
import pytest

import colorvolume_ref as cr
import oracle
import volumecast_ref as vr

VS, R = 0.05, 8
K = np.array([[40.0, 0, 16.0], [0, 40.0, 12.0], [0, 0, 1.0]])
T = np.eye(4)
H, W = 24, 32
KEY = np.array([[0, 0, 2]], np.int32)  # z in [0.8, 1.2): in front of the camera at the origin


def _flat(depth):
    return np.full((H, W), depth, np.float32)


def _img(rgb, h=H, w=W):
    return np.broadcast_to(np.asarray(rgb, np.uint8), (h, w, 3)).copy()


def test_constant_small_integer_colours_give_their_exact_mean():
    v = cr.ColorVolume(VS, R)
    cols = [(3, 40, 200), (5, 42, 100), (10, 38, 0), (6, 40, 100)]
    for c in cols:
        ok, colored = v.integrate_frame(KEY, _flat(1.0), K, T, 1.0, 3.0, 8.0, _img(c), K)
    seen = ok.reshape(-1)
    assert seen.any() and np.array_equal(ok, colored)
    k = len(cols)
    assert (v.weight[0][seen] == k).all()
    # sums of k small integers and their running means are exact in float32 only when every partial mean is:
    # the partial means here are 3, 4, 6, 6 / 40, 41, 40, 40 / 200, 150, 100, 100
    want = np.array([6, 40, 100], np.float32)
    assert np.array_equal(v.color[0][seen], np.broadcast_to(want, (int(seen.sum()), 3)))
    assert not v.color[0][~seen].any() and not v.weight[0][~seen].any()


def test_voxel_outside_the_colour_image_keeps_its_colour_and_gains_weight():
    v = cr.ColorVolume(VS, R)
    v.integrate_frame(KEY, _flat(1.0), K, T, 1.0, 3.0, 8.0, _img((10, 20, 30)), K)
    before = v.color.copy()
    # a colour camera whose image lies wholly to the right of every projection: u_c < 0 for all voxels
    Kc = K.copy()
    Kc[0, 2] = -1000.0
    ok, colored = v.integrate_frame(KEY, _flat(1.0), K, T, 1.0, 3.0, 8.0, _img((200, 200, 200)), Kc)
    assert ok.any() and not colored.any()
    assert np.array_equal(v.color, before)
    assert (v.weight[0][ok[0]] == 2).all()
    # half in: the block projects to u_c in [10, 27.5] with cx = 10, a 16-pixel-wide colour image covers u_c <= 15
    Kc[0, 2] = 10.0
    ok, colored = v.integrate_frame(KEY, _flat(1.0), K, T, 1.0, 3.0, 8.0, _img((0, 0, 0), H, 16), Kc)
    assert colored.any() and (ok & ~colored).any()
    assert np.array_equal(v.color[0][(ok & ~colored)[0]], before[0][(ok & ~colored)[0]])
    assert (v.weight[0][ok[0]] == 3).all()


def test_rejected_frame_changes_nothing():
    v = cr.ColorVolume(VS, R)
    v.integrate_frame(KEY, _flat(1.0), K, T, 1.0, 3.0, 8.0, _img((10, 20, 30)), K)
    state = (v.tsdf.copy(), v.weight.copy(), v.color.copy())
    for depth in (0.0, 5.0, 0.2):  # invalid, past depth_max, and far in front of every voxel (sdf < -trunc)
        ok, colored = v.integrate_frame(KEY, _flat(depth), K, T, 1.0, 3.0, 8.0, _img((250, 250, 250)), K)
        assert not ok.any() and not colored.any()
    for a, b in zip(state, (v.tsdf, v.weight, v.color)):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("Rb,scale", [(8, 1.0), (16, 1000.0)])
def test_tsdf_and_weight_equal_the_cpu_oracle_bit_for_bit(Rb, scale):
    from mqr import synthetic
    seq = synthetic.make_sequence("sphere", n=4, height=48, width=64, f=52.5, noise=True, seed=3)
    Kd, Tw = seq["K"].astype(np.float64), seq["T_wc"].astype(np.float64)
    depth = (seq["depth"] * np.float32(scale)).astype(np.float32)
    ref = oracle.OracleVBG(0.02, Rb, 256)
    v = cr.ColorVolume(0.02, Rb)
    for i in range(4):
        keys = ref.integrate_frame(depth[i], Kd[i], Tw[i], scale, 3.0, 4.0)
        v.integrate_frame(keys, depth[i], Kd[i], Tw[i], scale, 3.0, 4.0)
    ok_, ot, ow = cr.canon(*ref.export())
    k, t, w, _ = cr.canon(*v.export())
    assert len(k) > 8 and np.array_equal(k, ok_)
    assert np.array_equal(w, ow) and (w > 0).any()
    assert np.array_equal(t.view(np.uint32), ot.view(np.uint32))


def test_ray_cast_colour_of_a_uniform_volume_is_that_colour():
    import volumecast_cases as vc
    case = vc.random_case(8, 108, 2, 24, 32)
    vol = vr.Volume(case["keys"], case["tsdf"], case["weight"], case["voxel_size"], case["R"])
    out = vr.ray_cast(vol, None, case["K"], case["T"], case["H"], case["W"], **case["kw"])
    assert out["hit"].any() and not out["hit"].all()
    uniform = np.broadcast_to(np.array([51.0, 102.0, 255.0], np.float32), (len(case["keys"]), 8 ** 3, 3))
    col = cr.cast_color(vol, uniform, out["vertex"], out["hit"])
    assert not col[~out["hit"]].any()
    # S > 0 wherever a hit has a corner with weight > 0; there (sum r c / sum r) / 255 is c / 255 up to the
    # rounding of the 8-term sums (c is constant, so the quotient is c (1 + O(8 eps)))
    lit = col.any(axis=-1)
    # (a quarter of the 27 blocks is absent and a crossing is interpolated from the last observed sample, so
    # some hit vertices lie in absent blocks: S = 0 there)
    assert lit.sum() > 0.5 * out["hit"].sum()
    want = np.array([51.0, 102.0, 255.0]) / 255.0
    assert np.abs(col[lit] - want).max() <= 16 * np.finfo(np.float32).eps
    # with no colour anywhere, or no volume, everything is 0
    assert not cr.cast_color(vol, np.zeros_like(uniform), out["vertex"], out["hit"]).any()


def test_edge_colours_interpolate_with_the_vertex_ratio():
    keys = np.array([[0, 0, 0], [1, 0, 0]], np.int32)
    t = np.full((2, 8, 8, 8), 0.5, np.float32)
    t[1] = -0.25  # a sign change on the block seam x = 7 -> 8 only
    w = np.full_like(t, 5.0)
    c = np.zeros((2, 8, 8, 8, 3), np.float32)
    c[0] = (30.0, 60.0, 90.0)
    c[1] = (60.0, 0.0, 255.0)
    m, dup, seam = cr.edge_colors(keys, t, w, c, VS, 8, 3.0)
    assert dup == 0 and len(m) == 64 and seam == set(m)
    ratio = np.float32(0.5) / np.float32(0.75)
    pos = np.array([np.float32(VS) * (np.float32(7) + ratio), np.float32(VS) * np.float32(2),
                    np.float32(VS) * np.float32(3)], np.float32)
    want = ((np.float32(1) - ratio) * c[0, 0, 0, 0] + ratio * c[1, 0, 0, 0]) / np.float32(255)
    assert np.array_equal(m[cr.pos_key(pos)], want)
    # an end under the threshold takes the edge out
    w[1, 3, 2, 0] = 1.0
    m2, _, _ = cr.edge_colors(keys, t, w, c, VS, 8, 3.0)
    assert len(m2) == 63 and cr.pos_key(pos) not in m2
