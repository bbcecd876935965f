"""The numpy restatement of the volume ray cast (tests/volumecast_ref.py) checked on its own:
an affine field whose refined depth is analytic, the oracle's sphere against the analytic sphere, hand-built
known answers, and the colour-aligned-depth I/O and frame selection around it.  No GPU.
"""
import os

import numpy as np
import pytest

import volumecast_cases as vc
import volumecast_ref as vr


def _cast(case, ft=np.float32, block_keys=None, **kw):
    vol = vr.Volume(case["keys"], case["tsdf"], case["weight"], case["voxel_size"], case["R"])
    return vr.ray_cast(vol, block_keys, case["K"], case["T"], case["H"], case["W"], ft=ft, **{**case["kw"], **kw})


# ---------------------------------------------------------------------------------------------- 1. affine field
AFFINE_F32_VS_F64 = 2.57e-7  # measured: largest |float32 - float64| refined depth over both image sizes


@pytest.mark.parametrize("H,W", [(12, 16), (13, 17)])
def test_affine_field_refined_depth_is_analytic(H, W):
    """tsdf = n . p + e on a 2 x 2 x 2-block volume: the trilinear samples reproduce an affine field, so where
    the crossing is refined the depth is the ray-plane depth t = -(n . o + e) / (n . d).  Measured here: the
    float64 restatement is within 7e-16 of it; the float32 one differs from the float64 one by at most 2.57e-7
    (16 x 12: 2.35e-7, 17 x 13: 2.57e-7).  Tolerance 4 x 2.57e-7 for both.  Between 34 % and 46 % of each view's
    pixels are refined (76-78 % hit; near the volume's faces a sample lacks a corner and the nearest-voxel
    crossing is kept), asserted as > 30 %.  The third camera sits inside the volume on the negative side:
    all misses."""
    case = vc.affine(H, W)
    o32, o64 = _cast(case, refine=True), _cast(case, np.float64, refine=True)
    n, e = vc.AFFINE_PLANE
    tol = 4 * AFFINE_F32_VS_F64
    yy, xx = np.mgrid[0:H, 0:W]
    for f in range(2):
        K, T = case["K"][f], case["T"][f]
        Rm = T[:3, :3]
        o = -Rm.T @ T[:3, 3]
        d = np.stack([(xx - K[0, 2]) / K[0, 0], (yy - K[1, 2]) / K[1, 1], np.ones((H, W))], -1) @ Rm
        t = -(n @ o + e) / (d @ n)
        m = o64["refined"][f]
        assert np.array_equal(m, o32["refined"][f]) and m.mean() > 0.3
        print(f"{W}x{H} view {f}: refined {m.mean():.3f}, |f64 - analytic| {np.abs(o64['depth'][f] - t)[m].max():.3g}, "
              f"|f32 - f64| {np.abs(o32['depth'][f] - o64['depth'][f])[m].max():.3g}")
        assert np.abs(o64["depth"][f] - t)[m].max() <= tol
        assert np.abs(o32["depth"][f].astype(np.float64) - t)[m].max() <= tol
        # the vertex is the point at that depth along the ray
        p = o + t[..., None] * d
        assert np.abs(o64["vertex"][f] - p)[m].max() <= tol
    for o_ in (o32, o64):
        assert not o_["hit"][2].any() and not o_["depth"][2].any() and not o_["normal"][2].any()


# ---------------------------------------------------------------------------------------------- 2. sphere
def test_sphere_depth():
    """The oracle's sphere volume (8 noise-free 64 x 48 frames, 2 cm voxels, truncation 4 voxels) rendered from
    its first four cameras by the float64 restatement, against the analytic sphere, over the rays that pass the
    centre within half the radius (well inside the silhouette: 992 pixels, all of them hit).  Measured maximum
    |depth - analytic|: 0.05168 m with refine off and on (the worst pixel keeps its nearest-voxel crossing: a
    trilinear sample there lacks a corner observed twice); median 0.0110 m off, 0.0068 m on.  Asserted: the
    maximum within 2 x 0.05168 for both, and refine not worse than off in maximum and median."""
    seq, keys, tsdf, weight = vc.sphere_volume()
    vol = vr.Volume(keys, tsdf, weight, vc.SPHERE["voxel_size"], vc.SPHERE["R"])
    K, T = seq["K"][:4].astype(np.float64), seq["T_wc"][:4].astype(np.float64)
    stats = {}
    for refine in (False, True):
        o = vr.ray_cast(vol, None, K, T, 48, 64, depth_scale=1.0, depth_min=0.1, depth_max=vc.SPHERE["depth_max"],
                        weight_threshold=vc.SPHERE["weight_threshold"], trunc_voxel_multiplier=vc.SPHERE["trunc"],
                        refine=refine, ft=np.float64)
        err = []
        for f in range(4):
            ana, b = vc.sphere_analytic(K[f], T[f], 48, 64)
            inside = b < 0.25
            assert o["hit"][f][inside].all()
            err.append(np.abs(o["depth"][f] - ana)[inside])
        err = np.concatenate(err)
        stats[refine] = (err.max(), np.median(err))
        print(f"refine {refine}: {len(err)} pixels, max {err.max():.5f}, median {np.median(err):.5f}")
        assert err.max() <= vc.SPHERE_BOUND
    assert stats[True][0] <= stats[False][0] and stats[True][1] <= stats[False][1]


def test_sphere_silhouette_against_the_mesh_cast():
    """The GPU comparison of the volume cast with the mesh cast (tests/test_gpu_volume_cast.py), checked here
    with the restatement (float32, pixel centres, refine) against the brute-force cast of the oracle's mesh, both
    at weight threshold 1.5, on the views of volumecast_cases.SILHOUETTE_VIEW (two 224 x 24 strips at the
    capture's focal length: both limbs of the sphere and the background are in view).  Measured: 4.17 % of the
    pixels lie within one pixel of either silhouette (asserted < 5 %); outside that band no pixel is hit by one
    path only (asserted: none); over the rest |volume - mesh| is at most 0.1323 m, against the bound of the
    sphere test above (2 x 0.05168 = 0.10336 m) plus the mesh's own error against the analytic sphere there
    (0.0381 m) = 0.1415 m.  At a longer focal length the rule does not hold one pixel off the silhouette: the
    march reads the voxel at floor(p / voxel), which widens the volume's silhouette by up to a voxel (192 x 48
    at f = 240, where a voxel is 3 pixels: 69 of 17 545 pixels outside the band are hit by one path only)."""
    import oracle
    import raycast_ref as rr
    from mqr.o3d_utils import compute_o3d_intrinsic_matrices
    from mqr.raycasting import RaycastingScene
    seq, keys, tsdf, weight = vc.sphere_volume()
    ds = vc.sphere_color_dataset(**vc.SILHOUETTE_VIEW)
    K = compute_o3d_intrinsic_matrices(ds).astype(np.float32).astype(np.float64)
    T = ds.transforms.extrinsics_wc.astype(np.float32).astype(np.float64)
    H, W = vc.SILHOUETTE_VIEW["H"], vc.SILHOUETTE_VIEW["W"]
    o = vr.ray_cast(vr.Volume(keys, tsdf, weight, vc.SPHERE["voxel_size"], vc.SPHERE["R"]), None, K, T, H, W,
                    depth_scale=1.0, depth_min=0.1, depth_max=vc.SPHERE["depth_max"], pixel_offset=0.5, refine=True,
                    weight_threshold=vc.SPHERE["weight_threshold"], trunc_voxel_multiplier=vc.SPHERE["trunc"])
    vol = np.where(o["hit"], o["depth"], np.inf).astype(np.float32)
    ref = oracle.OracleVBG(vc.SPHERE["voxel_size"], vc.SPHERE["R"], 512)
    for i in range(8):
        ref.integrate_frame(seq["depth"][i], seq["K"][i].astype(np.float64), seq["T_wc"][i].astype(np.float64), 1.0,
                            vc.SPHERE["depth_max"], vc.SPHERE["trunc"])
    verts, _, tris = ref.extract_mesh(vc.SPHERE["weight_threshold"])
    P = verts[tris]
    msh = np.stack([rr.brute_force(P, RaycastingScene.create_rays_pinhole(K[f], T[f], W, H).numpy()).t.reshape(H, W)
                    for f in range(len(K))])
    assert np.isfinite(vol).any() and not np.isfinite(vol).all()  # surface and background
    share, one_only, diff, mesh_err = vc.compare_with_mesh_cast(vol, msh, K, T, verts, tris)
    print(f"band share {share:.4f}, one path only {one_only}, |volume - mesh| {diff:.4f}, mesh error {mesh_err:.4f}")
    assert share < vc.BAND_SHARE_MAX
    assert one_only == 0
    assert diff <= vc.SPHERE_BOUND + mesh_err


# ---------------------------------------------------------------------------------------------- 3. known answers
def test_low_weight_crossing_is_skipped():
    """The crossing at 0.9 m is under the weight threshold: no hit there; the valid crossing at 1.7 m is found
    (within the nearest-voxel lookup's one voxel without refine, on it with refine)."""
    case = vc.low_weight_crossing()
    o = _cast(case)
    assert o["hit"].all() and (o["depth"] >= 1.7 - 1e-6).all() and (o["depth"] <= 1.7 + vc.VOXEL + 1e-6).all()
    r = _cast(case, refine=True)
    assert r["refined"].all() and np.abs(r["depth"] - 1.7).max() < 1e-6
    # with every weight valid the first crossing is the hit
    first = _cast(dict(case, weight=np.full_like(case["weight"], 5.0)))
    assert first["hit"].all() and (first["depth"] < 1.0).all()


def test_absent_blocks_are_skipped_by_a_block():
    """Blocks z = 2, 3 are absent: from the free space of block 1 the ray advances a block (0.4 m) per step
    across them and finds the surface at 1.8 m in block 4 -- in 5 steps, not the 20-odd of voxel steps."""
    o = _cast(vc.absent_block_gap())
    assert o["hit"].all() and (o["steps"] == 5).all()
    assert (o["depth"] >= 1.8 - 1e-6).all() and (o["depth"] <= 1.8 + vc.VOXEL + 1e-6).all()


def test_surface_on_a_seam_with_the_neighbour_absent():
    """tsdf = 0 on the last lattice layer of block z = 2, block z = 3 absent: the hit is found, the trilinear
    samples lack their far corners, so refine keeps the nearest-voxel crossing and the normal is zero."""
    case = vc.seam_surface()
    o, r = _cast(case), _cast(case, refine=True)
    assert o["hit"].all() and not r["refined"].any()
    assert np.array_equal(o["depth"], r["depth"]) and (o["depth"] >= 1.15 - 1e-6).all() and (o["depth"] < 1.2).all()
    assert not r["normal"].any()


def test_depth_range_clips_the_surface_away():
    assert _cast(vc.plane())["hit"].all()
    for kw in (dict(depth_max=0.9), dict(depth_min=1.1)):
        o = _cast(vc.plane(**kw))
        assert not o["hit"].any() and not o["depth"].any() and not o["vertex"].any()


def test_block_behind_the_camera_changes_nothing():
    a = _cast(vc.plane())
    b = _cast(vc.plane(extra_keys=[(0, 0, -2), (0, 0, -1)]))  # wholly behind; touching the camera plane
    assert a["hit"].all() and np.isinf(a["range_min"]).sum() == np.isinf(b["range_min"]).sum()
    for k in ("depth", "vertex", "normal"):
        assert np.array_equal(a[k], b[k])
    p = vc.plane()
    o = _cast(dict(p, keys=np.array([[0, 0, -2]], np.int32), tsdf=p["tsdf"][:1], weight=p["weight"][:1]))
    assert not o["hit"].any() and np.isinf(o["range_min"]).all()


def test_negative_block_keys():
    a = _cast(vc.plane(), refine=True)
    shifted = vc.plane(shift=(-3, -2, -5))
    assert shifted["keys"].max() < 0
    b = _cast(shifted, refine=True)
    assert a["hit"].all() and b["hit"].all()
    for o in (a, b):  # the plane 1 m ahead, within the nearest-voxel lookup's one voxel
        assert (o["depth"] >= 1.0 - 1e-5).all() and (o["depth"] <= 1.0 + vc.VOXEL + 1e-5).all()
        assert np.allclose(o["normal"][..., 2], -1.0, atol=1e-4)  # the gradient points at the camera
        assert np.abs(o["normal"][..., :2]).max() < 1e-4


def test_empty_volume_and_empty_block_list():
    o = _cast(vc.empty())
    assert not o["hit"].any() and not o["depth"].any() and np.isinf(o["range_min"]).all()
    o = _cast(vc.plane(), block_keys=np.zeros((0, 3), np.int32))
    assert not o["hit"].any()
    o = _cast(vc.plane(), block_keys=np.array([[7, 7, 7], [1 << 22, 0, 0]]))  # absent, out of the key range
    assert not o["hit"].any()


def test_step_cap_ends_the_march():
    o = _cast(vc.step_cap())
    assert not o["hit"].any() and (o["steps"] == vr.MAX_STEPS).all()
    assert (o["range_max"] > 0.01 * (vr.MAX_STEPS + 8)).all()  # the ray was still inside its range


# ---------------------------------------------------------------------------------------------- 4. I/O and selection
def test_rgbd_data_io_round_trip_and_paths(tmp_path):
    from mqr.dataio import DataIO, RGBDDataIO, RGBDPaths
    from mqr.models import Side
    io = DataIO(tmp_path)
    assert isinstance(io.rgbd, RGBDDataIO) and isinstance(io.rgbd.rgbd_path_config, RGBDPaths)
    # the reference's names (config/project_path_config.py COLOR_ALIGNED_DEPTH_DIR_MAP, "<timestamp>.npy")
    names = {Side.LEFT: "left_color_aligned_depth", Side.RIGHT: "right_color_aligned_depth"}
    d = np.arange(12, dtype=np.float32).reshape(3, 4)
    d[1, 2] = np.inf
    for side in Side:
        p = io.rgbd.rgbd_path_config.get_color_aligned_depth_path(side=side, timestamp=1234)
        assert p == io.project_dir / names[side] / "1234.npy"
        with pytest.raises(FileNotFoundError):
            io.rgbd.load_color_aligned_depth(side=side, timestamp=1234)
        io.rgbd.save_color_aligned_depth(depth_map=d, side=side, timestamp=1234)
        back = io.rgbd.load_color_aligned_depth(side=side, timestamp=1234)
        assert back.dtype == np.float32 and np.array_equal(back, d) and os.path.exists(p)


class _Recorder:
    """Stands in for the scene: raycast_in_color_view is replaced by a generator that records its datasets."""


def _dataset(ts):
    from mqr.models import CameraDataset, CoordinateSystem, Transforms
    n = len(ts)
    q = np.tile(np.array([0.0, 0.0, 0.0, 1.0]), (n, 1))
    return CameraDataset(directory_relative_path="left_camera", image_file_names=np.array([f"{t}.png" for t in ts]),
                         timestamps=np.asarray(ts), fx=np.full(n, 10.0), fy=np.full(n, 10.0), cx=np.full(n, 2.0),
                         cy=np.full(n, 1.5), transforms=Transforms(CoordinateSystem.OPEN3D, np.zeros((n, 3)), q),
                         widths=np.full(n, 4), heights=np.full(n, 3))


@pytest.mark.parametrize("optimized,only", [(False, False), (False, True), (True, False), (True, True)])
def test_render_color_aligned_depth_frame_selection(tmp_path, monkeypatch, optimized, only):
    from mqr import raycasting
    from mqr.dataio import DataIO
    from mqr.models import Side
    full = {Side.LEFT: _dataset([10, 20, 30, 40]), Side.RIGHT: _dataset([11, 21, 31])}
    opt = {Side.LEFT: _dataset([20, 40]), Side.RIGHT: _dataset([31])}
    io = DataIO(tmp_path)
    monkeypatch.setattr(io.color, "load_color_dataset", lambda side, use_cache=True: full[side])
    calls = []

    def fake_cast(scene, dataset, batch=16, **kw):
        calls.append([int(t) for t in dataset.timestamps])
        for t in dataset.timestamps:
            yield np.full((3, 4), float(t), np.float32)

    monkeypatch.setattr(raycasting, "raycast_in_color_view", fake_cast)
    n = raycasting.render_color_aligned_depth(_Recorder(), io, opt if optimized else None, only)
    if optimized:
        want = ([] if only else [[10, 30]]) + [[20, 40]] + ([] if only else [[11, 21]]) + [[31]]
        written = {Side.LEFT: [20, 40] if only else [10, 20, 30, 40], Side.RIGHT: [31] if only else [11, 21, 31]}
    else:
        want = [] if only else [[10, 20, 30, 40], [11, 21, 31]]
        written = {Side.LEFT: [] if only else [10, 20, 30, 40], Side.RIGHT: [] if only else [11, 21, 31]}
    assert calls == want and n == sum(len(v) for v in written.values())
    for side, ts in written.items():
        d = io.rgbd.rgbd_path_config.get_color_aligned_depth_dir(side)
        assert sorted(p.name for p in d.glob("*.npy")) == sorted(f"{t}.npy" for t in ts)
        for t in ts:
            assert (io.rgbd.load_color_aligned_depth(side, t) == float(t)).all()
