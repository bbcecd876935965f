"""The coloured VoxelBlockGrid on the GPU against its numpy restatement
(tests/colorvolume_ref.py): the colour integrate pass, the coloured extractions, the ray-cast colour map, the
contents round trip, the refusals and the fuse_color_volume pipeline piece.  Nothing here has a tolerance: the
rule has a fixed float32 operation order, and the (tsdf, weight) of a coloured volume are those of a colourless
one fed the same depth, bit for bit."""
import ctypes

import numpy as np
import pytest

import colorvolume_ref as cr
import oracle
import volumecast_cases as vc
import volumecast_ref as vr

pytestmark = pytest.mark.gpu

VS, DMAX, TM = 0.02, 3.0, 4.0
H, W = 48, 64
NAMES = ("tsdf", "weight", "color")
N_FRAMES = 130  # past kMaxBatch = 127: a batch seam


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _colour_cameras(seq, Hc, Wc, zoom=1.8):
    """(images (n,Hc,Wc,3) uint8, K_color (n,3,3)): render_color at the depth poses with a longer lens, so part
    of the depth frustum -- the sphere's top and bottom -- falls outside the colour image."""
    from mqr import synthetic
    n = len(seq["K"])
    f = float(seq["K"][0][0, 0]) * Wc / W * zoom
    Kc = np.array([[f, 0, (Wc - 1) / 2.0], [0, f, (Hc - 1) / 2.0], [0, 0, 1.0]])
    imgs = np.stack([synthetic.render_color("sphere", Kc, seq["T_cw"][i][:3, :3].astype(np.float64),
                                            seq["T_cw"][i][:3, 3].astype(np.float64), Hc, Wc) for i in range(n)])
    return imgs, np.broadcast_to(Kc, (n, 3, 3)).copy()


@pytest.fixture(scope="module")
def data():
    """The sphere ring: 130 noisy 64 x 48 depth frames, colour frames at 80 x 60 and 40 x 30, and the blocks each
    frame touches (the CPU oracle's touch) for 2 cm voxels at R = 8 and 16.  Read-only."""
    from mqr import _lib, synthetic
    _lib.load()
    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible")
    seq = synthetic.make_sequence("sphere", n=N_FRAMES, height=H, width=W, f=52.5, noise=True, seed=21)
    d = dict(depth=np.ascontiguousarray(seq["depth"], np.float32), K=seq["K"].astype(np.float64),
             T=seq["T_wc"].astype(np.float64))
    d["big"], d["Kbig"] = _colour_cameras(seq, 60, 80)
    d["small"], d["Ksmall"] = _colour_cameras(seq, 30, 40)
    assert d["big"].any(axis=-1).mean() > 0.2 and d["small"].any(axis=-1).mean() > 0.2
    d["touched"] = {}
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d


def _ref_integrate(data, ref, depth, K, T, imgs=None, Kc=None, scale=1.0, ids=None):
    """The restatement over the frames, each with the blocks it touches (the CPU oracle's touch; cached under
    the frames' ids when they are the fixture's unmodified frames)."""
    touched = []
    for j in range(len(depth)):
        key = None if ids is None else (ref.R, int(ids[j]))
        if key is None or key not in data["touched"]:
            t = oracle.touch(depth[j], K[j], T[j], VS, ref.R, scale, DMAX, TM)
            if key is None:
                touched.append(t)
                continue
            data["touched"][key] = t
        touched.append(data["touched"][key])
    ref.integrate(touched, depth, K, T, scale, DMAX, TM, imgs, Kc)


def _grid(R, color=True, block_count=256):
    from mqr.vbg import VoxelBlockGrid
    return VoxelBlockGrid(attr_names=NAMES if color else NAMES[:2], voxel_size=VS, block_resolution=R,
                          block_count=block_count, device="HIP:0")


def _check(vbg, ref, plain=None):
    """Colours bit-equal to the restatement; tsdf and weight bit-equal to the colourless grid `plain` (and to the
    restatement, which the CPU tests pin on the oracle)."""
    gk, gt, gw, gc = cr.canon(*vbg.export())
    rk, rt, rw, rc = cr.canon(*ref.export())
    assert np.array_equal(gk, rk), "block sets differ"
    if plain is not None:
        pk, pt, pw = cr.canon(*plain.export())
        assert np.array_equal(gk, pk)
        assert np.array_equal(_bits(gt), _bits(pt)) and np.array_equal(_bits(gw), _bits(pw)), \
            "a coloured volume's tsdf / weight differ from a colourless volume's"
    seen = gw > 0
    assert np.array_equal(gw, rw) and np.array_equal(_bits(gt)[seen], _bits(rt)[seen])
    same = _bits(gc) == _bits(rc)
    assert same.all(), f"{int((~same).sum())} of {same.size} colour values differ"
    assert (gc > 0).any() and (gc[seen] == 0).all(axis=-1).any(), "expected coloured and uncoloured seen voxels"
    return gc


def _run(data, R, frames, size="big", calls=None, block_count=256, scale=1.0, width=None, frame_ok=None):
    """integrate_frames(colors=) over `frames` (split into `calls`), on a coloured and a colourless grid, and the
    restatement over the same frames."""
    frames = np.asarray(frames)
    depth = data["depth"][frames]
    modified = scale != 1.0 or width is not None
    if scale != 1.0:
        depth = depth * np.float32(scale)
    if width is not None:  # (an odd height with it: an odd pixel count, which the 8-byte window reads cannot take)
        depth = np.ascontiguousarray(depth[:, :H - 1, :width])
    K, T = data["K"][frames], data["T"][frames]
    imgs, Kc = data[size][frames], data["K" + size][frames]
    vbg, plain, ref = _grid(R, True, block_count), _grid(R, False, block_count), cr.ColorVolume(VS, R)
    kw = dict(depth_scale=scale, depth_max=DMAX, trunc_voxel_multiplier=TM)
    for sl in (calls or [slice(None)]):
        ok = None if frame_ok is None else np.asarray(frame_ok, np.uint8)[sl]
        vbg.integrate_frames(depth[sl], K[sl], T[sl], frame_ok=ok, colors=imgs[sl], color_intrinsics=Kc[sl], **kw)
        plain.integrate_frames(depth[sl], K[sl], T[sl], frame_ok=ok, **kw)
        idx = np.arange(len(frames))[sl]
        if ok is not None:
            idx = idx[ok.astype(bool)]
        _ref_integrate(data, ref, depth[idx], K[idx], T[idx], imgs[idx], Kc[idx], scale,
                       None if modified else frames[idx])
    return vbg, plain, ref


# ------------------------------------------------------------------------------------------ 1. integrate
@pytest.mark.parametrize("R,size", [(8, "small"), (16, "big")])
def test_three_frames_one_call(data, R, size):
    vbg, plain, ref = _run(data, R, [0, 40, 85], size)
    assert vbg.has_color and not plain.has_color
    _check(vbg, ref, plain)


@pytest.mark.parametrize("R", [8, 16])
def test_second_call_onto_existing_blocks(data, R):
    vbg, plain, ref = _run(data, R, [0, 3, 6, 3, 0, 9], "big", calls=[slice(0, 3), slice(3, 6)])
    _check(vbg, ref, plain)


def test_batch_seam_130_frames(data):
    vbg, plain, ref = _run(data, 8, np.arange(N_FRAMES), "small")
    _check(vbg, ref, plain)
    assert vbg.export()[2].max() > 10


def test_depth_scale_1000_takes_the_exact_kernel(data):
    from mqr import _lib
    vbg, plain, ref = _run(data, 16, [0, 1, 2, 60], "small", scale=1000.0)
    var = ctypes.c_int(-1)
    _lib.call("mqr_vbg_last_kernel", vbg.handle, ctypes.byref(var))
    assert var.value == 2
    _check(vbg, ref, plain)


def test_odd_frame_width_takes_the_dword_gathers(data):
    from mqr import _lib
    vbg, plain, ref = _run(data, 16, [0, 1, 2, 60], "big", width=63)
    var = ctypes.c_int(-1)
    _lib.call("mqr_vbg_last_kernel", vbg.handle, ctypes.byref(var))
    assert var.value == 4
    _check(vbg, ref, plain)


def test_frame_ok_skips_a_frame(data):
    vbg, plain, ref = _run(data, 8, [0, 1, 2, 3], "big", frame_ok=[1, 0, 1, 1])
    _check(vbg, ref, plain)
    assert vbg.export()[2].max() == 3


def test_pool_growth_keeps_colours(data):
    vbg, plain, ref = _run(data, 8, [0, 20, 40, 60, 80, 100], "small", calls=[slice(0, 2), slice(2, 6)],
                           block_count=4)
    assert vbg.capacity() > 16 and vbg.size() > 16  # grew several times
    _check(vbg, ref, plain)


def _reset_case(data, R, device_frames):
    """Bright frames, reset, then other frames: voxels of re-used blocks the second round never updates must
    be 0, not stale."""
    from mqr._lib import DeviceBuffer
    first, second = np.array([0, 1, 2, 3]), np.array([65, 66])
    bright = np.full_like(data["big"][first], 255)
    vbg, ref = _grid(R), cr.ColorVolume(VS, R)
    kw = dict(depth_scale=1.0, depth_max=DMAX, trunc_voxel_multiplier=TM)
    keep = []

    def feed(frames, imgs):
        d, c = data["depth"][frames], imgs
        if device_frames:  # no synchronise anywhere: the calls return with their integrates queued
            keep.extend([DeviceBuffer.from_array(d), DeviceBuffer.from_array(c)])
            d, c = (keep[-2], len(frames), H, W), (keep[-1], len(frames)) + c.shape[1:3]
        vbg.integrate_frames(d, data["K"][frames], data["T"][frames], colors=c,
                             color_intrinsics=data["Kbig"][frames], **kw)

    feed(first, bright)
    vbg.reset()
    feed(second, data["big"][second])
    _ref_integrate(data, ref, data["depth"][second], data["K"][second], data["T"][second], data["big"][second],
                   data["Kbig"][second], ids=second)
    gc = _check(vbg, ref)
    gw = cr.canon(*vbg.export())[2]
    assert not gc[gw == 0].any(), "stale colours in never-updated voxels"
    return vbg


@pytest.mark.parametrize("R", [8, 16])
def test_reset_leaves_no_stale_colours(data, R):
    _reset_case(data, R, device_frames=False)


def test_reset_behind_queued_device_integrates(data):
    vbg = _reset_case(data, 16, device_frames=True)
    n = ctypes.c_int64(-1)
    from mqr import _lib
    _lib.call("mqr_vbg_flips", vbg.handle, ctypes.byref(n))
    assert n.value == 0  # a coloured volume declines the set swap: the reset queued behind the integrate


def test_empty_second_frame_raises_and_keeps_frame_0(data):
    frames = np.array([0, 1, 2])
    depth = data["depth"][frames].copy()
    depth[1] = 0
    kw = dict(depth_scale=1.0, depth_max=DMAX, trunc_voxel_multiplier=TM)
    vbg, plain, ref = _grid(8), _grid(8, False), cr.ColorVolume(VS, 8)
    with pytest.raises(RuntimeError, match="No block is touched"):
        plain.integrate_frames(depth, data["K"][frames], data["T"][frames], **kw)
    with pytest.raises(RuntimeError, match="No block is touched"):
        vbg.integrate_frames(depth, data["K"][frames], data["T"][frames], colors=data["small"][frames],
                             color_intrinsics=data["Ksmall"][frames], **kw)
    _ref_integrate(data, ref, depth[:1], data["K"][:1], data["T"][:1], data["small"][:1], data["Ksmall"][:1], ids=[0])
    _check(vbg, ref, plain)
    # and again with a volume that has integrated before (the first batch of the call is then speculative)
    vbg.reset()
    ref2 = cr.ColorVolume(VS, 8)
    with pytest.raises(RuntimeError, match="No block is touched"):
        vbg.integrate_frames(depth, data["K"][frames], data["T"][frames], colors=data["small"][frames],
                             color_intrinsics=data["Ksmall"][frames], **kw)
    _ref_integrate(data, ref2, depth[:1], data["K"][:1], data["T"][:1], data["small"][:1], data["Ksmall"][:1],
                   ids=[0])
    _check(vbg, ref2)


def test_colour_frames_written_late_on_a_side_stream(data):
    """The colour stack is a torch tensor a side stream is still filling when integrate_frames is called inside
    ``torch.cuda.stream(s)``: no synchronise, the library orders itself behind the stream."""
    import torch
    frames = np.array([0, 50, 100])
    imgs = np.ascontiguousarray(data["big"][frames])
    s = torch.cuda.Stream()
    pinned = torch.from_numpy(imgs.copy()).pin_memory()
    dev = torch.zeros(imgs.shape, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    vbg, ref = _grid(16), cr.ColorVolume(VS, 16)
    with torch.cuda.stream(s):
        torch.cuda._sleep(50_000_000)  # ~tens of ms: the copy lands well after the call below is made
        dev.copy_(pinned, non_blocking=True)
        vbg.integrate_frames(data["depth"][frames], data["K"][frames], data["T"][frames], colors=dev,
                             color_intrinsics=data["Kbig"][frames], depth_scale=1.0, depth_max=DMAX,
                             trunc_voxel_multiplier=TM)
    dev.record_stream(s)
    _ref_integrate(data, ref, data["depth"][frames], data["K"][frames], data["T"][frames], imgs, data["Kbig"][frames],
                   ids=frames)
    _check(vbg, ref)


def test_depth_only_calls_leave_colours_alone_and_new_blocks_black(data):
    vbg, ref = _grid(8), cr.ColorVolume(VS, 8)
    kw = dict(depth_scale=1.0, depth_max=DMAX, trunc_voxel_multiplier=TM)
    a, b = np.array([0, 1]), np.array([64, 65])
    vbg.integrate_frames(data["depth"][a], data["K"][a], data["T"][a], colors=data["small"][a],
                         color_intrinsics=data["Ksmall"][a], **kw)
    vbg.integrate_frames(data["depth"][b], data["K"][b], data["T"][b], **kw)  # the far side: new blocks
    _ref_integrate(data, ref, data["depth"][a], data["K"][a], data["T"][a], data["small"][a], data["Ksmall"][a], ids=a)
    n_before = len(ref.index)
    _ref_integrate(data, ref, data["depth"][b], data["K"][b], data["T"][b], ids=b)
    assert len(ref.index) > n_before
    _check(vbg, ref)


def test_only_uint8_colour_and_only_coloured_volumes(data):
    from mqr.vbg import VoxelBlockGrid
    f = np.array([0])
    kw = dict(depth_scale=1.0, depth_max=DMAX, trunc_voxel_multiplier=TM)
    vbg = _grid(8)
    for bad in (data["small"][f].astype(np.float32), data["small"][f].astype(np.uint16)):
        with pytest.raises(ValueError):
            vbg.integrate_frames(data["depth"][f], data["K"][f], data["T"][f], colors=bad,
                                 color_intrinsics=data["Ksmall"][f], **kw)
    with pytest.raises(ValueError):  # sizes must match when the depth intrinsics are used
        vbg.integrate_frames(data["depth"][f], data["K"][f], data["T"][f], colors=data["small"][f], **kw)
    with pytest.raises(ValueError):
        _grid(8, False).integrate_frames(data["depth"][f], data["K"][f], data["T"][f], colors=data["small"][f],
                                         color_intrinsics=data["Ksmall"][f], **kw)
    assert vbg.size() == 0
    for names, ch, dt in ((("tsdf", "weight", "colour"), None, None), (NAMES, ((1), (1), (1)), None),
                          (NAMES, None, (np.float32, np.float32, np.uint8)), (("tsdf", "color"), None, None)):
        with pytest.raises(NotImplementedError):
            VoxelBlockGrid(attr_names=names, attr_channels=ch, attr_dtypes=dt, voxel_size=VS, block_resolution=8,
                           block_count=4, device="HIP:0")
    ok = VoxelBlockGrid(attr_names=NAMES, attr_dtypes=(np.float32,) * 3, attr_channels=((1), (1), (3)), voxel_size=VS,
                        block_resolution=8, block_count=4, device="HIP:0")
    assert ok.has_color


def test_per_frame_colour_overload_equals_the_batched_call(data):
    frames = [0, 1, 2]
    a, b = _grid(8), _grid(8)
    for i in frames:
        keys = a.compute_unique_block_coordinates(data["depth"][i], data["K"][i], data["T"][i], 1.0, DMAX, TM)
        a.integrate(keys, data["depth"][i], data["small"][i], data["K"][i], data["Ksmall"][i], data["T"][i], 1.0,
                    DMAX, TM)
    b.integrate_frames(data["depth"][frames], data["K"][frames], data["T"][frames], colors=data["small"][frames],
                       color_intrinsics=data["Ksmall"][frames], depth_scale=1.0, depth_max=DMAX,
                       trunc_voxel_multiplier=TM)
    for x, y in zip(cr.canon(*a.export()), cr.canon(*b.export())):
        assert np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x,
                              y.view(np.uint32) if y.dtype == np.float32 else y)
    with pytest.raises(ValueError):
        a.integrate(keys, data["depth"][0], data["small"][0].astype(np.float32), data["K"][0], data["Ksmall"][0],
                    data["T"][0], 1.0, DMAX, TM)


# ------------------------------------------------------------------------------------------ 2. extraction
@pytest.fixture(scope="module")
def fused(data):
    """R -> (coloured grid of 8 ring frames, its exported contents)."""
    out = {}
    frames = np.arange(0, N_FRAMES, 16)[:8]
    for R, size in ((8, "small"), (16, "big")):
        vbg = _grid(R)
        vbg.integrate_frames(data["depth"][frames], data["K"][frames], data["T"][frames], colors=data[size][frames],
                             color_intrinsics=data["K" + size][frames], depth_scale=1.0, depth_max=DMAX,
                             trunc_voxel_multiplier=TM)
        out[R] = (vbg, vbg.export())
    return out


@pytest.mark.parametrize("R", [8, 16])
@pytest.mark.parametrize("mesh", [True, False])
def test_extracted_colours_match_the_edge_map(fused, R, mesh):
    vbg, (keys, tsdf, weight, color) = fused[R]
    thr = 1.5
    edge, dup, seam = cr.edge_colors(keys, tsdf, weight, color, VS, R, thr)  # (asserts no tsdf is exactly 0)
    assert dup == 0
    g = vbg.extract_triangle_mesh(weight_threshold=thr) if mesh else vbg.extract_point_cloud(weight_threshold=thr)
    pos = g.vertices if mesh else g.points
    col = g.vertex_colors if mesh else g.colors
    assert (g.vertex["colors"] if mesh else g.point["colors"]).is_cuda
    assert col is not None and col.shape == pos.shape and col.dtype == np.float32 and len(pos) > 500
    unmatched, differ, on_seam = 0, 0, 0
    for p, c in zip(pos, col):
        k = cr.pos_key(p)
        want = edge.get(k)
        if want is None:
            unmatched += 1
            continue
        differ += not np.array_equal(_bits(c), _bits(want))
        on_seam += k in seam
    assert unmatched == 0, f"{unmatched} of {len(pos)} vertices are on no edge of the restatement"
    assert differ == 0, f"{differ} of {len(pos)} colours differ"
    assert on_seam > 0
    # (1 - ratio) c_o + ratio c_e with both colours at 255 is 255 up to four roundings (1 - ratio, the two
    # products, the sum), and the division adds one: at most 1 + 5 * 2^-24, asserted as 1 + 8 * 2^-24
    assert (col > 0).any() and col.max() <= 1.0 + 8 * 2.0 ** -24


def test_colourless_geometry_reports_no_colours(data):
    vbg = _grid(8, False)
    f = np.arange(0, N_FRAMES, 16)[:8]
    vbg.integrate_frames(data["depth"][f], data["K"][f], data["T"][f], depth_scale=1.0, depth_max=DMAX,
                         trunc_voxel_multiplier=TM)
    mesh, pcd = vbg.extract_triangle_mesh(weight_threshold=1.5), vbg.extract_point_cloud(weight_threshold=1.5)
    assert len(mesh.vertices) > 100 and not mesh.has_vertex_colors() and mesh.vertex_colors is None
    assert len(pcd.points) > 100 and not pcd.has_colors() and pcd.colors is None


# ------------------------------------------------------------------------------------------ 3. ray cast
def _cast_case(case, seed):
    from mqr.vbg import VoxelBlockGrid
    rng = np.random.default_rng(seed)
    R, n = case["R"], len(case["keys"])
    color = rng.integers(0, 256, (n, R, R, R, 3)).astype(np.float32) + rng.random((n, R, R, R, 3)).astype(np.float32)
    color = np.minimum(color, np.float32(255))
    vbg = VoxelBlockGrid(attr_names=NAMES, voxel_size=case["voxel_size"], block_resolution=R,
                         block_count=max(n, 1), device="HIP:0")
    vbg.import_blocks(case["keys"], case["tsdf"], case["weight"], color=color)
    return vbg, color


@pytest.mark.parametrize("R,hw,refine,drop_corner", [(8, (48, 64), True, False), (16, (49, 65), False, False),
                                                     (8, (49, 65), True, True)])
def test_ray_cast_colour_bit_for_bit(R, hw, refine, drop_corner):
    case = vc.random_case(R, 100 + R, 2, hw[0], hw[1], refine=refine)
    if drop_corner:  # a block next to observed surface goes: S covers fewer than 8 corners around some hits
        surface = [i for i in range(len(case["keys"])) if (case["tsdf"][i] > 0).any() and (case["tsdf"][i] < 0).any()]
        keep = np.ones(len(case["keys"]), bool)
        keep[surface[len(surface) // 2]] = False
        case = dict(case, keys=case["keys"][keep], tsdf=case["tsdf"][keep], weight=case["weight"][keep])
    vbg, color = _cast_case(case, 7 + R)
    vol = vr.Volume(case["keys"], case["tsdf"], case["weight"], case["voxel_size"], R)
    want = vr.ray_cast(vol, None, case["K"], case["T"], case["H"], case["W"], **case["kw"])
    want_col = cr.cast_color(vol, color, want["vertex"], want["hit"])
    out = vbg.ray_cast_frames(case["K"], case["T"], case["W"], case["H"], render_attributes=("vertex", "color"),
                              **case["kw"])
    assert out["color"].is_cuda and out["color"].shape == (2, hw[0], hw[1], 3)
    got_v, got = out["vertex"].numpy(), out["color"].numpy()
    assert np.array_equal(_bits(got_v), _bits(want["vertex"]))
    same = _bits(got) == _bits(want_col)
    assert same.all(), f"{int((~same).sum())} of {same.size} colour values differ"
    hit = want["hit"]
    assert 0.05 < hit.mean() < 0.9 and not got[~hit].any() and (got[hit] > 0).any()
    # (sum r c / sum r) / 255 with c <= 255: the two 8-term sums, their products, the quotient and the division
    # each round once, under 20 roundings of 2^-24 in all -- asserted as 1 + 32 * 2^-24
    assert got.max() <= 1.0 + 32 * 2.0 ** -24
    if drop_corner:  # some hit has a corner in an absent block and still a colour
        g = [np.floor(want["vertex"][..., a] / np.float32(case["voxel_size"])).astype(np.int64) for a in range(3)]
        absent = np.zeros(hit.shape, bool)
        for k in range(8):
            b = [(g[a] + ((k >> a) & 1)) // R for a in range(3)]
            absent |= vol.lookup(*b) < 0
        assert (absent & hit & got.any(axis=-1)).any()
    # "color" alone, and through Open3D's single-frame signature
    alone = vbg.ray_cast(None, case["K"][0], case["T"][0], case["W"], case["H"], ("color",), **{
        k: case["kw"][k] for k in ("depth_scale", "depth_min", "depth_max", "weight_threshold",
                                   "trunc_voxel_multiplier")})
    assert list(alone) == ["color"] and alone["color"].shape == (hw[0], hw[1], 3)
    if not refine:
        assert np.array_equal(_bits(alone["color"].numpy()), _bits(want_col[0]))


def test_ray_cast_colour_needs_a_coloured_volume():
    from mqr import _lib
    from mqr.vbg import VoxelBlockGrid
    case = vc.random_case(8, 108, 1, 5, 7)
    vbg = VoxelBlockGrid(voxel_size=case["voxel_size"], block_resolution=8, block_count=32, device="HIP:0")
    vbg.import_blocks(case["keys"], case["tsdf"], case["weight"])
    with pytest.raises(ValueError):
        vbg.ray_cast_frames(case["K"], case["T"], 7, 5, render_attributes=("depth", "color"))
    buf = _lib.DeviceBuffer(4 * 5 * 7 * 3)
    K, T = np.ascontiguousarray(case["K"], np.float64), np.ascontiguousarray(case["T"], np.float64)
    rc = _lib._lib.mqr_vbg_ray_cast_color(vbg.handle, None, 0, _lib.MQR_HOST, _lib.ptr(K, _lib._f64p),
                                          _lib.ptr(T, _lib._f64p), 1, 5, 7, 1.0, 0.1, 3.0, 3.0, 8.0, 8, 0.0, 0, None,
                                          None, None, buf.ptr, _lib.MQR_DEVICE)
    assert rc == 2 and b"no colour" in _lib._lib.mqr_last_error()


# ------------------------------------------------------------------------------------------ 4. contents, refusals
def test_save_load_round_trip(fused, tmp_path, data):
    from mqr.vbg import VoxelBlockGrid
    vbg, (keys, tsdf, weight, color) = fused[8]
    path = str(tmp_path / "coloured.npz")
    vbg.save(path)
    with np.load(path) as z:
        assert sorted(z.files) == ["block_resolution", "color", "key", "tsdf", "voxel_size", "weight"]
        assert z["color"].shape == (len(keys), 8, 8, 8, 3) and z["color"].dtype == np.float32
    back = VoxelBlockGrid.load(path, device="HIP:0")
    assert back.has_color
    for x, y in zip(cr.canon(*back.export()), cr.canon(keys, tsdf, weight, color)):
        assert np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x,
                              y.view(np.uint32) if y.dtype == np.float32 else y)
    # a colourless file has no colour key and loads as a colourless volume; importing without colours leaves 0
    plain = _grid(8, False)
    plain.import_blocks(keys, tsdf, weight)
    p2 = str(tmp_path / "plain.npz")
    plain.save(p2)
    with np.load(p2) as z:
        assert sorted(z.files) == ["block_resolution", "key", "tsdf", "voxel_size", "weight"]
    assert not VoxelBlockGrid.load(p2, device="HIP:0").has_color
    dark = _grid(8)
    dark.import_blocks(keys, tsdf, weight)
    assert not dark.export()[3].any()


def test_merge_pack_and_owned_extraction_refuse_a_coloured_volume(fused):
    from mqr import _lib
    vbg = fused[8][0]
    L = _lib._lib
    n = vbg.size()
    keys = _lib.DeviceBuffer.from_array(np.ascontiguousarray(fused[8][1][0], np.int32))
    packed = _lib.DeviceBuffer(n * 512 * 2 * 4)
    assert L.mqr_vbg_pack_weighted(vbg.handle, keys.ptr, n, packed.ptr) == 2
    assert b"coloured" in L.mqr_last_error()
    assert L.mqr_vbg_unpack_weighted(vbg.handle, keys.ptr, n, packed.ptr) == 2
    g = ctypes.c_void_p()
    assert L.mqr_extract_mesh_owned(vbg.handle, 1.5, n, ctypes.byref(g)) == 2 and not g.value
    assert b"coloured" in L.mqr_last_error()
    other = _grid(8)
    locals_ = (ctypes.c_void_p * 1)(vbg.handle)
    outs = (ctypes.c_void_p * 1)(other.handle)
    owned = ctypes.c_int64()
    assert L.mqr_merge_local(locals_, 1, 0, 0, outs, ctypes.byref(owned)) == 2
    assert b"coloured" in L.mqr_last_error()
    assert vbg.size() == n  # nothing was touched
    h = ctypes.c_void_p()
    assert L.mqr_vbg_create_color(ctypes.c_float(VS), 12, 8, 0, ctypes.byref(h)) == 2 and not h.value


# ------------------------------------------------------------------------------------------ 5. the pipeline piece
def test_fuse_color_volume_from_geometry_equals_rendering_first(data):
    from mqr.color_volume import fuse_color_volume
    f = np.arange(0, N_FRAMES, 16)[:8]
    geo = _grid(8, False)
    geo.integrate_frames(data["depth"][f], data["K"][f], data["T"][f], depth_scale=1.0, depth_max=DMAX,
                         trunc_voxel_multiplier=TM)
    views = np.array([0, 16, 32, 48, 64])
    K, T, imgs = data["Kbig"][views], data["T"][views], data["big"][views]
    kw = dict(voxel_size=VS, block_resolution=8, block_count=64, depth_max=DMAX, trunc_voxel_multiplier=TM,
              device="HIP:0", weight_threshold=1.5)
    a = fuse_color_volume(imgs, K, T, geometry=geo, batch=2, **kw)
    depth = geo.ray_cast_frames(K, T, 80, 60, render_attributes=("depth",), depth_scale=1.0, depth_min=0.1,
                                depth_max=DMAX, weight_threshold=1.5, trunc_voxel_multiplier=TM)["depth"].numpy()
    assert (depth > 0).mean() > 0.1
    b = fuse_color_volume(imgs, K, T, depths=depth, batch=3, **kw)
    assert a.has_color and a.size() > 8
    for x, y in zip(cr.canon(*a.export()), cr.canon(*b.export())):
        assert np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x,
                              y.view(np.uint32) if y.dtype == np.float32 else y)
    assert (a.export()[3] > 0).any()
    mesh = a.extract_triangle_mesh(weight_threshold=1.5)
    assert mesh.has_vertex_colors() and len(mesh.vertices) > 100
