"""VoxelBlockGrid.ray_cast on the GPU (csrc/volumecast.hip) against its numpy restatement
(tests/volumecast_ref.py, float32: the rule has a fixed operation order, so there is no tolerance), its
ordering behind queued integrates, its argument checks, and the colour-aligned-depth stage built on it.
Volumes are built with import_blocks from tests/volumecast_cases.py."""
import ctypes
import functools

import numpy as np
import pytest

import volumecast_cases as vc
import volumecast_ref as vr

pytestmark = pytest.mark.gpu

ATTRS = ("depth", "vertex", "normal")


def _vbg(case):
    from mqr.vbg import VoxelBlockGrid
    vbg = VoxelBlockGrid(voxel_size=case["voxel_size"], block_resolution=case["R"],
                         block_count=max(len(case["keys"]), 1), device="HIP:0")
    if len(case["keys"]):
        vbg.import_blocks(case["keys"], case["tsdf"], case["weight"])
    return vbg


def _gpu(vbg, case, block_coords=None, attrs=ATTRS, frames=slice(None), **kw):
    out = vbg.ray_cast_frames(case["K"][frames], case["T"][frames], case["W"], case["H"], render_attributes=attrs,
                              block_coords=block_coords, **{**case["kw"], **kw})
    return {k: v.numpy() for k, v in out.items()}


def _ref(case, block_coords=None, **kw):
    vol = vr.Volume(case["keys"], case["tsdf"], case["weight"], case["voxel_size"], case["R"])
    return vr.ray_cast(vol, block_coords, case["K"], case["T"], case["H"], case["W"], **{**case["kw"], **kw})


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _assert_same(got, want, what=""):
    for k in ATTRS:
        if k in got:
            same = _bits(got[k]) == _bits(want[k])
            assert same.all(), f"{what} {k}: {int((~same).sum())} of {same.size} values differ"


# ------------------------------------------------------------------------------------------ 1. bit for bit
@pytest.mark.parametrize("name", ["low_weight_crossing", "absent_block_gap", "seam_surface", "plane", "empty",
                                  "step_cap"])
@pytest.mark.parametrize("refine", [False, True])
def test_known_answer_volumes_bit_for_bit(name, refine):
    case = getattr(vc, name)()
    want = _ref(case, refine=refine)
    got = _gpu(_vbg(case), case, refine=refine)
    _assert_same(got, want, name)
    if name in ("empty", "step_cap"):
        assert not got["depth"].any() and not got["vertex"].any() and not got["normal"].any()
    else:
        assert (got["depth"] > 0).all()


def test_clipped_behind_and_negative_keys_bit_for_bit():
    for case in (vc.plane(depth_max=0.9), vc.plane(depth_min=1.1), vc.plane(extra_keys=[(0, 0, -2), (0, 0, -1)]),
                 vc.plane(shift=(-3, -2, -5))):
        _assert_same(_gpu(_vbg(case), case, refine=True), _ref(case, refine=True))


# R, (H, W), range_map_down_factor, pixel_offset, refine, block_coords subset, frames: every value of each
# (tile, wave and coarse-cell edges: 1 x 1, 7 x 5, 64 x 48, 65 x 49) in a covering selection, not the product
RANDOM = [
    (8, (1, 1), 8, 0.0, False, False, 1),
    (8, (5, 7), 1, 0.5, True, True, 2),
    (8, (48, 64), 8, 0.0, True, False, 3),
    (8, (49, 65), 16, 0.0, False, True, 1),
    (16, (49, 65), 16, 0.5, True, False, 2),
    (16, (48, 64), 1, 0.5, False, True, 1),
    (16, (5, 7), 8, 0.0, True, False, 3),
    (16, (1, 1), 16, 0.5, True, True, 2),
]


@pytest.mark.parametrize("R,hw,df,off,refine,subset,n", RANDOM)
def test_random_volume_bit_for_bit(R, hw, df, off, refine, subset, n):
    """A seeded 3 x 3 x 3-block volume with holes, weights 3..6 with 3 % at 0..3 (threshold 3) and +-0 / denormal
    tsdf."""
    case = vc.random_case(R, 100 + R, n, hw[0], hw[1], range_map_down_factor=df, pixel_offset=off, refine=refine)
    coords = None
    if subset:  # every other block, an absent one and one outside the key range
        coords = np.concatenate([case["keys"][::2], [[9, 9, 9], [1 << 22, 0, 0]]]).astype(np.int32)
    want = _ref(case, coords)
    got = _gpu(_vbg(case), case, coords)
    _assert_same(got, want, f"R={R} {hw} df={df}")
    if hw[0] >= 48:  # the views see surface and background, refined crossings and whole normal stencils
        assert 0.05 < want["hit"].mean() < 0.9 and (got["normal"] != 0).any()
        assert want["refined"].any() == bool(refine)


def test_open3d_signature_and_attributes():
    case = vc.random_case(8, 108, 1, 48, 64)
    vbg = _vbg(case)
    kw = {k: case["kw"][k] for k in ("depth_scale", "depth_min", "depth_max", "weight_threshold",
                                     "trunc_voxel_multiplier")}
    out = vbg.ray_cast(None, case["K"][0], case["T"][0], 64, 48, ("depth", "normal"), **kw)
    assert sorted(out) == ["depth", "normal"]
    assert out["depth"].shape == (48, 64, 1) and out["normal"].shape == (48, 64, 3) and out["depth"].is_cuda
    want = _ref(case)
    assert np.array_equal(_bits(out["depth"].numpy()[..., 0]), _bits(want["depth"][0]))
    assert np.array_equal(_bits(out["normal"].numpy()), _bits(want["normal"][0]))
    scaled = vbg.ray_cast(None, case["K"][0], case["T"][0], 64, 48, **dict(kw, depth_scale=1000.0))
    assert list(scaled) == ["depth"]
    assert np.array_equal(scaled["depth"].numpy()[..., 0], want["depth"][0] * np.float32(1000.0))
    for bad in (("color",), ("depth", "colour"), ()):
        with pytest.raises(ValueError):
            vbg.ray_cast(None, case["K"][0], case["T"][0], 64, 48, bad)


# ------------------------------------------------------------------------------------------ 2. batch, residency
def _raw_cast(vbg, case, out_loc, frames=slice(None), flags=1):
    """mqr_vbg_ray_cast through the C ABI: host outputs (MQR_HOST) or device buffers copied back."""
    from mqr import _lib
    K = np.ascontiguousarray(case["K"][frames], np.float64)
    T = np.ascontiguousarray(case["T"][frames], np.float64)
    n, H, W = len(K), case["H"], case["W"]
    kw = case["kw"]
    shapes = {"depth": (n, H, W), "vertex": (n, H, W, 3), "normal": (n, H, W, 3)}
    if out_loc == _lib.MQR_HOST:
        host = {k: np.full(s, -7.0, np.float32) for k, s in shapes.items()}
        ptrs = [_lib.ptr(host[k]) for k in ATTRS]
    else:
        bufs = {k: _lib.DeviceBuffer(4 * int(np.prod(s))) for k, s in shapes.items()}
        ptrs = [bufs[k].ptr for k in ATTRS]
    _lib.call("mqr_vbg_ray_cast", vbg.handle, None, 0, _lib.MQR_HOST, _lib.ptr(K, _lib._f64p),
              _lib.ptr(T, _lib._f64p), n, H, W, kw["depth_scale"], kw["depth_min"], kw["depth_max"],
              kw["weight_threshold"], kw["trunc_voxel_multiplier"], 8, 0.5, flags, *ptrs, out_loc)
    if out_loc == _lib.MQR_HOST:
        return host
    return {k: bufs[k].to_array(shapes[k], np.float32) for k in ATTRS}


def test_batch_equals_single_equals_repeat_and_residency():
    from mqr import _lib
    case = vc.random_case(16, 116, 3, 49, 65)
    vbg = _vbg(case)
    dev = _raw_cast(vbg, case, _lib.MQR_DEVICE)
    host = _raw_cast(vbg, case, _lib.MQR_HOST)
    again = _raw_cast(vbg, case, _lib.MQR_DEVICE)
    for k in ATTRS:
        assert host[k].tobytes() == dev[k].tobytes() == again[k].tobytes(), k
        for f in range(3):
            one = _raw_cast(vbg, case, _lib.MQR_HOST if f % 2 else _lib.MQR_DEVICE, frames=slice(f, f + 1))
            assert one[k][0].tobytes() == dev[k][f].tobytes(), (k, f)
    assert (dev["depth"] > 0).any()
    r, m = vbg.ray_cast_last_ms()
    assert r > 0 and m > 0


# ------------------------------------------------------------------------------------------ 3. pending integrate
class _Dev:
    def __init__(self, t):
        self.ptr = ctypes.c_void_p(t.data_ptr())


def test_ray_cast_orders_itself_behind_queued_integrates():
    """integrate_frames on device frames returns with its last integrate queued; a ray cast issued at once must
    render the finished volume -- the same bytes as a cast after mqr_device_synchronize.  The same after a
    reset behind that unfinished integrate (the volume's second table / pool set) and a new integrate."""
    import torch
    from mqr import _lib, synthetic
    from mqr.vbg import VoxelBlockGrid
    kw = dict(depth_scale=1.0, depth_max=4.0, trunc_voxel_multiplier=10.0)
    ckw = dict(depth_scale=1.0, depth_max=4.0, trunc_voxel_multiplier=10.0, weight_threshold=2.0, refine=True,
               render_attributes=ATTRS)
    seqs = [synthetic.make_sequence("room", n=n, height=240, width=320, f=262.5, noise=True, seed=s)
            for n, s in ((127, 41), (48, 42))]
    vbg = VoxelBlockGrid(voxel_size=0.01, block_resolution=16, block_count=256, device="cuda:0")
    results = []
    for seq in seqs:
        depth = torch.from_numpy(np.ascontiguousarray(seq["depth"], np.float32)).cuda()
        K, T = seq["K"].astype(np.float64), seq["T_wc"].astype(np.float64)
        torch.cuda.synchronize()
        B, H, W = depth.shape
        vbg.reset()  # (the second time: behind the first sequence's cast, nothing in flight)
        if results:  # an integrate in flight at the reset: the sets swap
            vbg.integrate_frames((_Dev(depth), B, H, W), K, T, **kw)
            vbg.reset()
        vbg.integrate_frames((_Dev(depth), B, H, W), K, T, **kw)
        first = {k: v.numpy() for k, v in vbg.ray_cast_frames(K[:2], T[:2], W // 2, H // 2, **ckw).items()}
        _lib.call("mqr_device_synchronize", 0)
        settled = {k: v.numpy() for k, v in vbg.ray_cast_frames(K[:2], T[:2], W // 2, H // 2, **ckw).items()}
        for k in ATTRS:
            assert first[k].tobytes() == settled[k].tobytes(), k
        assert (settled["depth"] > 0).mean() > 0.5
        results.append(settled["depth"])
    assert not np.array_equal(results[0], results[1])


# ------------------------------------------------------------------------------------------ 4. the mesh path
@functools.lru_cache(None)
def _sphere_vbg():
    _, keys, tsdf, weight = vc.sphere_volume()
    return _vbg(dict(keys=keys, tsdf=tsdf, weight=weight, voxel_size=vc.SPHERE["voxel_size"], R=vc.SPHERE["R"]))


SPHERE_CAST = dict(depth_max=vc.SPHERE["depth_max"], weight_threshold=vc.SPHERE["weight_threshold"],
                   trunc_voxel_multiplier=vc.SPHERE["trunc"])


def _both_casts(ds):
    """(volume cast, mesh cast, K, T, mesh) of the sphere volume through raycast_in_color_view on one dataset."""
    from mqr.o3d_utils import compute_o3d_intrinsic_matrices
    from mqr.raycasting import RaycastingScene, raycast_in_color_view
    vbg = _sphere_vbg()
    vol = np.stack(list(raycast_in_color_view(vbg, ds, **SPHERE_CAST)))
    mesh = vbg.extract_triangle_mesh(weight_threshold=vc.SPHERE["weight_threshold"])
    scene = RaycastingScene(device="HIP:0")
    scene.add_triangles(mesh)
    msh = np.stack(list(raycast_in_color_view(scene, ds)))
    with pytest.raises(TypeError):  # the thresholds are the volume cast's: the mesh path takes none
        next(raycast_in_color_view(scene, ds, **SPHERE_CAST))
    K = compute_o3d_intrinsic_matrices(ds).astype(np.float32).astype(np.float64)
    T = ds.transforms.extrinsics_wc.astype(np.float32).astype(np.float64)
    # the restatement agrees with the kernel bit for bit on this volume too
    _, keys, tsdf, weight = vc.sphere_volume()
    H, W = vol.shape[1:]
    want = vr.ray_cast(vr.Volume(keys, tsdf, weight, vc.SPHERE["voxel_size"], vc.SPHERE["R"]), None, K, T, H, W,
                       depth_scale=1.0, depth_min=0.1, pixel_offset=0.5, refine=True, **SPHERE_CAST)
    assert np.array_equal(_bits(np.where(np.isfinite(vol), vol, 0)), _bits(want["depth"]))
    return vol, msh, K, T, mesh


def test_volume_cast_against_the_mesh_cast():
    """The oracle's sphere volume through raycast_in_color_view, once as the volume and once as the mesh
    extracted from it (weight threshold 1.5 both), on one dataset that contains the silhouette
    (volumecast_cases.SILHOUETTE_VIEW: two 224 x 24 strips at the capture's focal length, both limbs and the
    background in view).  Left out: the pixels within one pixel of either path's silhouette, 4.2 % (asserted
    < 5 %; tests/test_volumecast_ref.py checks the same with the restatement: 4.17 %).  Outside that band both hit
    or both miss (asserted: no pixel hit by one path only).  On the rest |volume - mesh| <= the CPU sphere test's
    bound on the volume cast (2 x 0.05168 = 0.10336 m) + the mesh's own error against the analytic sphere (brute
    force of tests/raycast_ref.py over the extracted mesh: 0.0381 m on the restatement's side) = 0.1415 m;
    measured difference 0.1323 m there."""
    vol, msh, K, T, mesh = _both_casts(vc.sphere_color_dataset(**vc.SILHOUETTE_VIEW))
    assert vol.shape == msh.shape == (2, 24, 224) and vol.dtype == np.float32
    assert np.isfinite(vol).any() and not np.isfinite(vol).all()
    share, one_only, diff, mesh_err = vc.compare_with_mesh_cast(vol, msh, K, T, mesh.vertices, mesh.triangles)
    print(f"band share {share:.4f}, one path only {one_only}, |volume - mesh| {diff:.5f}, mesh error {mesh_err:.5f}, "
          f"bound {vc.SPHERE_BOUND + mesh_err:.5f}")
    assert share < vc.BAND_SHARE_MAX
    assert one_only == 0
    assert diff <= vc.SPHERE_BOUND + mesh_err


def test_volume_cast_against_the_mesh_cast_inside_the_silhouette():
    """The same on two 64 x 48 long-lens views (f = 240) whose every ray passes the sphere's centre within half its
    radius, the region the CPU sphere test's bound covers: both hit everywhere, nothing is left out, and
    |volume - mesh| (measured 0.0489 m) <= 0.10336 + the mesh's own error there (0.0204 m)."""
    vol, msh, K, T, mesh = _both_casts(vc.sphere_color_dataset(n=2))
    assert np.isfinite(vol).all() and np.isfinite(msh).all()
    share, one_only, diff, mesh_err = vc.compare_with_mesh_cast(vol, msh, K, T, mesh.vertices, mesh.triangles)
    print(f"|volume - mesh| {diff:.5f}, mesh error {mesh_err:.5f}, bound {vc.SPHERE_BOUND + mesh_err:.5f}")
    assert share == 0 and one_only == 0 and diff <= vc.SPHERE_BOUND + mesh_err


# ------------------------------------------------------------------------------------------ 5. argument errors
def test_argument_errors_then_a_valid_call():
    from mqr import _lib
    case = vc.plane()
    vbg = _vbg(case)
    K, T = case["K"], case["T"]
    good = dict(n=1, H=5, W=7, dmin=0.1, dmax=3.0, df=8, K=K, T=T, outs=(True, True, True))

    def call(**over):
        a = {**good, **over}
        Kc, Tc = np.ascontiguousarray(a["K"], np.float64), np.ascontiguousarray(a["T"], np.float64)
        bufs = [np.zeros((5, 7, 3), np.float32) for _ in range(3)]
        ptrs = [_lib.ptr(b) if w else None for b, w in zip(bufs, a["outs"])]
        return _lib._lib.mqr_vbg_ray_cast(vbg.handle, None, 0, _lib.MQR_HOST, _lib.ptr(Kc, _lib._f64p),
                                          _lib.ptr(Tc, _lib._f64p), a["n"], a["H"], a["W"], 1.0, a["dmin"], a["dmax"],
                                          3.0, 8.0, a["df"], 0.0, 0, *ptrs, _lib.MQR_HOST), bufs

    def broken(M, i, j, v):
        M = np.array(M, np.float64)
        M[0, i, j] = v
        return M

    bad = [dict(n=0), dict(n=-1), dict(H=0), dict(W=0), dict(H=-3), dict(df=0), dict(df=-8), dict(dmin=-0.5),
           dict(dmax=0.1), dict(dmax=0.05), dict(K=broken(K, 0, 2, np.nan)), dict(K=broken(K, 1, 1, np.inf)),
           dict(T=broken(T, 1, 3, np.nan)), dict(T=broken(T, 0, 0, -np.inf)), dict(K=broken(K, 0, 0, 0.0)),
           dict(K=broken(K, 1, 1, 0.0)), dict(outs=(False, False, False))]
    _lib.load()
    for over in bad:
        rc, bufs = call(**over)
        assert rc != 0, over
        assert _lib._lib.mqr_last_error().decode().startswith("ray_cast:"), over
        assert not any(b.any() for b in bufs), over  # nothing was launched
        rc, bufs = call()
        assert rc == 0 and (bufs[0].reshape(-1)[:35] > 0).all(), over
    for outs in ((True, False, False), (False, True, False), (False, False, True)):
        assert call(outs=outs)[0] == 0


# ------------------------------------------------------------------------------------------ 6. end to end
def test_render_color_aligned_depth_end_to_end(tmp_path):
    """A capture directory holding the two sides' colour datasets: render_color_aligned_depth writes one file per
    side and timestamp; each loads back equal to raycast_in_color_view's map for that frame, with inf where
    nothing is hit (the right side's wide views see past the sphere)."""
    from mqr.dataio import DataIO
    from mqr.models import Side
    from mqr.raycasting import raycast_in_color_view, render_color_aligned_depth
    vbg = _sphere_vbg()
    io = DataIO(tmp_path)
    sets = {Side.LEFT: vc.sphere_color_dataset(n=3, side_value="left"),
            Side.RIGHT: vc.sphere_color_dataset(n=2, H=24, W=32, f=30.0, side_value="right")}
    for side, ds in sets.items():
        path = io.color.image_path_config.get_color_dataset_path(side=side)
        path.parent.mkdir(parents=True, exist_ok=True)
        ds.save(path)
    n = render_color_aligned_depth(vbg, io, batch=2, **SPHERE_CAST)
    assert n == 5
    saw_inf = False
    for side, ds in sets.items():
        d = io.rgbd.rgbd_path_config.get_color_aligned_depth_dir(side)
        assert sorted(p.name for p in d.glob("*.npy")) == sorted(f"{int(t)}.npy" for t in ds.timestamps)
        for t, want in zip(ds.timestamps, raycast_in_color_view(vbg, ds, **SPHERE_CAST)):
            got = io.rgbd.load_color_aligned_depth(side, int(t))
            assert got.dtype == np.float32 and got.shape == want.shape and got.tobytes() == want.tobytes()
            assert not (got == 0).any() and np.isfinite(got).any()
            saw_inf |= bool(np.isinf(got).any())
    assert saw_inf
