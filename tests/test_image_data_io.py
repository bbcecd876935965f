"""The colour side of mqr.dataio / mqr.models on the CPU against the reference's recorded results
(tests/golden/colorframes_golden.npz): PoseInterpolator, load_camera_characteristics, build_color_dataset,
Transforms.apply_local_transform; timestamps and path handling; load_rgb / load_rgb_batch from PNG;
convert_yuv_directory's counts, summary lines and clean-up on a temporary project (host path)."""
import json
import os

import numpy as np
import pytest

import colorframes_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "colorframes_golden.npz")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture()
def project(golden, tmp_path):
    """The synthetic project the golden records were made on: poses, the left camera's characteristics and
    empty PNG files."""
    (tmp_path / "hmd_poses.csv").write_text(str(golden["pose_csv"]))
    (tmp_path / "left_camera_characteristics.json").write_text(str(golden["cam_json"]))
    (tmp_path / "left_camera_rgb").mkdir()
    for name in golden["ds_png_names"]:
        (tmp_path / "left_camera_rgb" / str(name)).write_bytes(b"")
    return tmp_path


def test_pose_interpolation_matches_the_reference(golden, project):
    from mqr.dataio import PoseInterpolator
    interp = PoseInterpolator(project / "hmd_poses.csv")
    found = golden["pose_found"]
    assert found.any() and not found.all()
    for ts, ok, pos, rot in zip(golden["pose_times"], found, golden["pose_pos"], golden["pose_rot"]):
        got = interp.interpolate_pose(int(ts))
        assert (got is not None) == bool(ok), ts
        if ok:
            assert np.array_equal(got[0], pos) and np.array_equal(got[1], rot), ts
    assert len(interp.hmd_pose_df) == 8  # the three bad lines are gone
    assert list(interp.hmd_pose_df["unix_time"]) == sorted(interp.hmd_pose_df["unix_time"])


def test_camera_characteristics_match_the_reference(golden, project, capsys):
    from mqr.dataio import ImageDataIO
    from mqr.models import Side
    io = ImageDataIO(project)
    for side in Side:
        c = io.load_camera_characteristics(side)
        got = np.array([c.width, c.height, c.fx, c.fy, c.cx, c.cy], np.float64)
        assert np.array_equal(got, golden[f"cam_{side.value}_values"])
        assert np.array_equal(np.asarray(c.transl, np.float64), golden[f"cam_{side.value}_transl"])
        assert np.array_equal(np.asarray(c.rot_quat, np.float64), golden[f"cam_{side.value}_rot"])
    assert "Using LEFT camera characteristics" in capsys.readouterr().out  # the right side fell back
    assert golden["cam_left_transl"][2] == -json.loads(str(golden["cam_json"]))["pose"]["translation"][2]
    os.remove(project / "left_camera_characteristics.json")
    with pytest.raises(FileNotFoundError):
        io.load_camera_characteristics(Side.RIGHT)


def test_build_color_dataset_matches_the_reference(golden, project):
    from mqr.dataio import DataIO
    from mqr.models import CameraDataset, Side
    io = DataIO(project)
    ds = io.color.build_color_dataset(Side.LEFT)
    want = {k[3:]: golden[k] for k in golden if k.startswith("ds_") and k != "ds_png_names"}
    got = ds.to_dict()
    assert set(got) == set(want) and len(ds) == 4
    for k, v in want.items():
        g = np.asarray(got[k])
        assert g.dtype == v.dtype and np.array_equal(g, v), k
    assert got["fx"].dtype == np.int64  # the reference's np.full_like of the timestamps truncates the intrinsics
    # load_color_dataset caches it, and reads the cache back
    again = io.color.load_color_dataset(Side.LEFT, use_cache=True)
    assert io.color.paths.get_color_dataset_path(Side.LEFT).exists()
    cached = io.color.load_color_dataset(Side.LEFT, use_cache=True)
    for k, v in want.items():
        assert np.array_equal(np.asarray(again.to_dict()[k]), v) and np.array_equal(np.asarray(cached.to_dict()[k]), v)
    assert io.color.load_optimized_color_dataset(Side.LEFT) is None
    io.color.save_optimized_color_dataset(ds[:2], Side.LEFT)
    assert isinstance(io.color.load_optimized_color_dataset(Side.LEFT), CameraDataset)
    assert len(io.color.load_optimized_color_dataset(Side.LEFT)) == 2
    with pytest.raises(Exception, match="No valid timestamps"):
        io.color.build_color_dataset(Side.RIGHT)
    # the documented difference: without PNGs the raw frames are listed
    for p in (project / "left_camera_rgb").iterdir():
        p.unlink()
    (project / "left_camera_raw").mkdir()
    stems = [n[:-4] for n in want["image_file_names"]]
    for s in stems:
        (project / "left_camera_raw" / f"{s}.yuv").write_bytes(b"")
    raw_ds = io.color.build_color_dataset(Side.LEFT)
    assert list(raw_ds.image_file_names) == [f"{s}.yuv" for s in stems]
    assert raw_ds.directory_relative_path == "left_camera_raw"
    assert np.array_equal(raw_ds.timestamps, want["timestamps"])
    assert np.array_equal(raw_ds.transforms.positions, want["positions"])


def test_apply_local_transform_matches_the_reference(golden):
    from mqr.models import CoordinateSystem, Transforms
    tr = Transforms(CoordinateSystem.UNITY, golden["local_positions"], golden["local_rotations"])
    out = tr.apply_local_transform(local_position=golden["local_lp"], local_rotation=golden["local_lr"])
    assert out.coordinate_system == CoordinateSystem.UNITY
    assert np.array_equal(out.positions, golden["local_out_positions"])
    assert np.array_equal(out.rotations, golden["local_out_rotations"])


def test_timestamps_and_format_info(tmp_path, capsys):
    from mqr.dataio import ColorPaths, ImageDataIO
    from mqr.models import Side
    io = ImageDataIO(ColorPaths(tmp_path))
    raw = tmp_path / "right_camera_raw"
    raw.mkdir()
    for name in ("30.yuv", "._10.yuv", "__20.yuv", "x7.yuv", "_.yuv", "40.txt"):
        (raw / name).write_bytes(b"\x01\x02")
    assert io.get_yuv_timestamps(Side.RIGHT) == [10, 30, 20]  # sorted by file name, as the reference lists them
    assert io.get_yuv_timestamps(Side.LEFT) == [] and io.get_rgb_timestamps(Side.RIGHT) == []
    out = capsys.readouterr().out
    assert "Skipping non-timestamped YUV file: x7.yuv" in out and "_.yuv" in out
    assert np.array_equal(io.load_yuv(Side.RIGHT, 30), [1, 2])
    (tmp_path / "right_camera_image_format.json").write_text(json.dumps({
        "width": 8, "height": 4, "format": "YUV_420_888",
        "planes": [{"bufferSize": 56, "rowStride": 16, "pixelStride": 1}, {"bufferSize": 23, "rowStride": 16, "pixelStride": 2},
                   {"bufferSize": 23, "rowStride": 16, "pixelStride": 2}],
        "baseTime": {"baseMonoTimeNs": 5, "baseUnixTimeMs": 7}}))
    f = io.load_image_format_info(Side.RIGHT)
    assert (f.width, f.height, f.format, len(f.planes)) == (8, 4, "YUV_420_888", 3)
    assert (f.planes[1].buffer_size, f.planes[1].row_stride, f.planes[1].pixel_stride) == (23, 16, 2)
    assert (f.base_time.mono_time_ns, f.base_time.unix_time_ns) == (5, 7)
    with pytest.raises(FileNotFoundError):
        io.load_hmd_poses()


def _write_project(tmp_path, side, frames, row_pad=4):
    """Raw NV12 frames of one side with their format JSON -> (planes, {timestamp: file bytes})."""
    H, W = next(iter(frames.values())).shape[:2]
    d = tmp_path / f"{side.value}_camera_raw"
    d.mkdir(exist_ok=True)
    files = {}
    for ts, rgb in frames.items():
        planes, buf = ref.to_yuv_file(rgb, row_pad)
        buf.tofile(d / f"{ts}.yuv")
        files[ts] = buf
    (tmp_path / f"{side.value}_camera_image_format.json").write_text(json.dumps({
        "width": W, "height": H, "format": "YUV_420_888",
        "planes": [{"bufferSize": b, "rowStride": r, "pixelStride": p} for b, r, p in planes],
        "baseTime": {"baseMonoTimeNs": 0, "baseUnixTimeMs": 0}}))
    return planes, files


def test_load_rgb_from_png_and_from_raw(tmp_path):
    pytest.importorskip("PIL")
    from mqr.dataio import ImageDataIO
    from mqr.models import Side
    rng = np.random.default_rng(4)
    io = ImageDataIO(tmp_path)
    a, b = (rng.integers(0, 256, (6, 10, 3), dtype=np.uint8) for _ in range(2))
    io.save_rgb(a, Side.LEFT, 100)
    io.save_bgr(b[..., ::-1], Side.LEFT, 200)
    assert io.get_rgb_timestamps(Side.LEFT) == [100, 200]
    assert np.array_equal(io.load_rgb(Side.LEFT, 100), a) and np.array_equal(io.load_rgb(Side.LEFT, 200), b)
    batch = io.load_rgb_batch(Side.LEFT, [200, 100, 200])  # PNGs only: no device is touched
    assert batch.shape == (3, 6, 10, 3) and np.array_equal(batch[0], b) and np.array_equal(batch[1], a)
    with pytest.raises(FileNotFoundError):
        io.load_rgb(Side.LEFT, 300)
    with pytest.raises(FileNotFoundError):
        io.load_rgb_batch(Side.LEFT, [100, 300])
    # no PNG, but the raw frame: load_rgb converts it on the host
    planes, files = _write_project(tmp_path, Side.LEFT, {300: a})
    assert np.array_equal(io.load_rgb(Side.LEFT, 300), ref.decode(files[300], 10, 6, planes))


def test_convert_yuv_directory_counts_and_cleanup(tmp_path, capsys):
    pytest.importorskip("PIL")
    from mqr import colorframes as cf
    from mqr.dataio import ImageDataIO
    from mqr.models import Side, Yuv2RgbConfig
    rng = np.random.default_rng(8)
    H, W = 12, 20
    busy = lambda: rng.integers(10, 246, (H, W, 3), dtype=np.uint8)  # noqa: E731
    left = {1000: busy(), 1033: np.full((H, W, 3), 90, np.uint8), 1066: busy(), 1099: busy()}
    left[1099][..., 2] = 2  # blue underexposed
    planes, files = _write_project(tmp_path, Side.LEFT, left)
    _write_project(tmp_path, Side.RIGHT, {2000: busy(), 2033: busy()})
    (tmp_path / "right_camera_raw" / "2066.yuv").write_bytes(b"\x00" * 40)  # too short: an exception
    cfg = Yuv2RgbConfig(blur_filter=True, blur_threshold=50.0, exposure_filter=True, exposure_threshold_low=0.02,
                        exposure_threshold_high=0.02)
    io = ImageDataIO(tmp_path)
    out = cf.convert_yuv_directory(io, cfg, device=None, batch=3)
    text = capsys.readouterr().out
    assert list(out) == [Side.LEFT, Side.RIGHT]
    kept, images = out[Side.LEFT]
    assert kept == [1000, 1066] and images.shape == (2, H, W, 3)
    assert np.array_equal(images[1], ref.decode(files[1066], W, H, planes))
    assert out[Side.RIGHT][0] == [2000, 2033]
    # the reference's summary lines
    assert f"[Info] 2 images written to {io.paths.get_rgb_dir(Side.LEFT)}" in text
    assert "[Info] 2 images were excluded by filtering." in text
    assert f"[Info] Cleaned up raw YUV directory after conversion: {io.paths.get_yuv_dir(Side.LEFT)}" in text
    assert "[Error] 1 files failed due to exceptions." in text
    assert f"[Warning] Keeping raw YUV directory for debugging: {io.paths.get_yuv_dir(Side.RIGHT)}" in text
    assert "Failed in Side.RIGHT/2066" in text
    # a side without exceptions loses its raw directory, the other keeps it
    assert not io.paths.get_yuv_dir(Side.LEFT).exists() and io.paths.get_yuv_dir(Side.RIGHT).exists()
    assert io.get_rgb_timestamps(Side.LEFT) == [1000, 1066] and io.get_rgb_timestamps(Side.RIGHT) == [2000, 2033]
    assert np.array_equal(io.load_rgb(Side.LEFT, 1000), images[0])
    # no filters, no PNGs, nothing removed
    _write_project(tmp_path, Side.LEFT, left)
    off = Yuv2RgbConfig(False, 50.0, False, 0.02, 0.02)
    out = cf.convert_yuv_directory(io, off, write_png=False, remove_yuv=False, device=None, return_images=False,
                                   sides=[Side.LEFT])
    assert out == {Side.LEFT: ([1000, 1033, 1066, 1099], None)}
    assert io.paths.get_yuv_dir(Side.LEFT).exists() and io.get_rgb_timestamps(Side.LEFT) == [1000, 1066]
