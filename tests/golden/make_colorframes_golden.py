"""Golden colour-frame and colour-dataset records from the reference's own functions.  Tests never run this.

Run where the reference checkout is available:
    python tests/golden/make_colorframes_golden.py <the reference's scripts directory>
It imports the reference's utils/image_utils.py, dataio/image_data_io.py, dataio/helpers/pose_interpolator.py
and models/transforms.py (read-only) with ``cv2`` and ``open3d`` stubbed, calls them on the small inputs built
below and stores inputs and results in tests/golden/colorframes_golden.npz.  Nothing from the reference is
copied.  No result here passes through OpenCV: ``cv2.calcHist`` is replaced by an exact ``np.bincount`` of
channel 0 as a float32 column (what calcHist returns, unambiguously), and the conversions that need
``cv2.cvtColor`` are not recorded.

Records (the keys of the npz):
  i420_<case>_{raw,planes,size,out}, i420_<case>_order        convert_yuv420_888_to_i420 per layout:
      planar      8x4, row strides 16 / 8 / 12 with padding, pixel strides 1 (V rows at planes[2].row_stride)
      nv12short   8x4, row strides 16, Android's short planes: 16*3+8, 16*1+7, 16*1+7 bytes, chroma stride 2
      nv21        the same bytes read as "NV21"
      chroma4     chroma pixel stride 4 (the reference still steps by 2)
      ystride2    Y pixel stride 2
      wide        36x6 NV12, row strides 40 (a second group of four pixels and a width that is 0 mod 4)
  i420_errors, i420_error_raised    nv12short one byte short of the U plane's last row; a 7x4 frame through
                                    convert_yuv420_888_to_bgr (its reshape)
  exposure_images, exposure_args, exposure_verdicts           is_over_or_under_exposed
  pose_csv, pose_times, pose_found, pose_pos, pose_rot        PoseInterpolator.interpolate_pose
  cam_json, cam_<side>_{values,transl,rot}                    load_camera_characteristics (right falls back)
  ds_png_names, ds_<field>                                    build_color_dataset on empty PNG files
  local_{positions,rotations,lp,lr,out_positions,out_rotations}   Transforms.apply_local_transform
"""
import json
import os
import sys
import tempfile
import types
from pathlib import Path
from unittest import mock

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def import_reference(ref_scripts):
    cv2 = types.ModuleType("cv2")

    def calc_hist(images, channels, mask, hist_size, ranges):
        a = np.asarray(images[0])
        ch = a[..., channels[0]] if a.ndim == 3 else a
        return np.bincount(ch.ravel(), minlength=hist_size[0]).astype(np.float32).reshape(-1, 1)

    cv2.calcHist = calc_hist
    sys.modules["cv2"] = cv2
    sys.modules["open3d"] = mock.MagicMock()
    sys.path.insert(0, ref_scripts)
    from config.project_path_config import ImagePathConfig
    from dataio.helpers.pose_interpolator import PoseInterpolator
    from dataio.image_data_io import ImageDataIO
    from models.image_format_info import BaseTime, ImageFormatInfo, ImagePlaneInfo
    from models.side import Side
    from models.transforms import CoordinateSystem, Transforms
    from utils import image_utils
    return types.SimpleNamespace(**locals())


def layouts():
    """name -> (width, height, [(buffer_size, row_stride, pixel_stride)] * 3, uv_order, file bytes)"""
    short = [(16 * 3 + 8, 16, 1), (16 + 7, 16, 2), (16 + 7, 16, 2)]
    return {
        "planar": (8, 4, [(64, 16, 1), (16, 8, 1), (24, 12, 1)], "NV12", 64 + 16 + 24),
        "nv12short": (8, 4, short, "NV12", 56 + 23 + 23),
        "nv21": (8, 4, short, "NV21", 56 + 23 + 23),
        "chroma4": (8, 4, [(64, 16, 1), (32, 16, 4), (32, 16, 4)], "NV12", 64 + 32 + 32),
        "ystride2": (8, 4, [(64, 16, 2), (16 + 7, 16, 2), (16 + 7, 16, 2)], "NV12", 64 + 23 + 23),
        "wide": (36, 6, [(40 * 5 + 36, 40, 1), (40 * 2 + 35, 40, 2), (40 * 2 + 35, 40, 2)], "NV12", 236 + 115 + 115),
    }


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref = import_reference(sys.argv[1])
    rng = np.random.default_rng(20)
    out = {}

    def fmt(w, h, planes):
        return ref.ImageFormatInfo(width=w, height=h, format="YUV_420_888",
                                   planes=[ref.ImagePlaneInfo(*p) for p in planes], base_time=ref.BaseTime(0, 0))

    # ---- I420 bytes
    cases = layouts()
    for name, (w, h, planes, order, n) in cases.items():
        raw = rng.integers(0, 256, n, dtype=np.uint8)
        out[f"i420_{name}_raw"] = raw
        out[f"i420_{name}_planes"] = np.array(planes, np.int64)
        out[f"i420_{name}_size"] = np.array([w, h], np.int64)
        out[f"i420_{name}_order"] = np.array(order)
        out[f"i420_{name}_out"] = ref.image_utils.convert_yuv420_888_to_i420(raw, fmt(w, h, planes), order)
    out["i420_cases"] = np.array(list(cases))
    w, h, planes, order, n = cases["nv12short"]
    raised = []
    for label, call in (
            ("nv12short_one_byte_short", lambda: ref.image_utils.convert_yuv420_888_to_i420(
                out["i420_nv12short_raw"][:56 + 16 + 7], fmt(w, h, planes), order)),
            ("odd_width_bgr", lambda: ref.image_utils.convert_yuv420_888_to_bgr(
                rng.integers(0, 256, 56 + 23 + 23, dtype=np.uint8), fmt(7, 4, planes)))):
        try:
            call()
            raised.append("none")
        except Exception as e:  # the class name is the record
            raised.append(type(e).__name__)
        print(label, raised[-1])
    out["i420_errors"] = np.array(["nv12short_one_byte_short", "odd_width_bgr"])
    out["i420_error_raised"] = np.array(raised)

    # ---- exposure verdicts: 25x40 = 1000 pixels, so 20 pixels are the 0.02 share exactly
    def image(n_dark, n_not_bright, channels):
        """n_dark pixels <= 5 (spread over 0..5), n_not_bright pixels <= 250 in all, the rest 251..255"""
        v = np.concatenate([np.arange(n_dark) % 6, 6 + np.arange(n_not_bright - n_dark) % 245,
                            251 + np.arange(1000 - n_not_bright) % 5]).astype(np.uint8)
        v = rng.permutation(v).reshape(25, 40)
        if channels == 1:
            return np.repeat(v[..., None], 3, axis=2), True
        return np.stack([v, rng.integers(0, 256, v.shape, dtype=np.uint8),
                         rng.integers(0, 256, v.shape, dtype=np.uint8)], axis=2), False

    images, args, verdicts = [], [], []
    for n_dark, n_nb, low, high, ch in [(19, 500, 0.02, 0.02, 3), (20, 500, 0.02, 0.02, 3), (21, 500, 0.02, 0.02, 3),
                                        (0, 19, 0.02, 0.02, 3), (0, 20, 0.02, 0.02, 3), (0, 21, 0.02, 0.02, 3),
                                        (50, 500, 0.05, 0.02, 1), (51, 500, 0.05, 0.02, 1), (10, 100, 0.02, 0.1, 1),
                                        (10, 99, 0.02, 0.1, 1), (0, 1000, 0.02, 0.02, 3), (1000, 1000, 0.02, 0.02, 3)]:
        img, grey = image(n_dark, n_nb, ch)
        verdict = ref.image_utils.is_over_or_under_exposed(img[..., 0] if grey else img, low_thresh=low, high_thresh=high)
        images.append(img)
        args.append([low, high, float(grey)])
        verdicts.append(bool(verdict))
    out["exposure_images"] = np.stack(images)
    out["exposure_args"] = np.array(args, np.float64)  # low, high, 1 = given as a single-channel image
    out["exposure_verdicts"] = np.array(verdicts)
    print("exposure", verdicts)

    # ---- poses and datasets on a synthetic project
    t0 = 1700000000000
    quats = rng.normal(size=(8, 4))
    quats /= np.linalg.norm(quats, axis=1, keepdims=True)
    pos = rng.normal(size=(8, 3))
    times = [t0, t0 + 20000, t0 + 40000, t0 + 40000, t0 + 55000, t0 + 120000, t0 + 10000, t0 + 200000]
    lines = ["unix_time,ovr_timestamp,pos_x,pos_y,pos_z,rot_x,rot_y,rot_z,rot_w"]
    for i, t in enumerate(times):  # (row 6 is out of time order: the reference sorts)
        lines.append(",".join([str(t), repr(0.5 * i)] + [repr(float(x)) for x in pos[i]] + [repr(float(x)) for x in quats[i]]))
    lines.insert(3, "1700000000500,1.0,2.0,3.0")  # short line: NaN fields, dropped
    lines.insert(5, "1700000000600,1.0,0,0,0,0,0,0,1,99,98")  # too many fields: skipped
    lines.insert(7, "1700000000700,0.1,,0.0,0.0,0.0,0.0,0.0,1.0")  # a gap: dropped
    csv = "\n".join(lines) + "\n"
    queries = [t0 + 5000, t0, t0 + 200000, t0 - 10000, t0 - 30000, t0 - 30001, t0 + 230000, t0 + 230001, t0 + 40000,
               t0 + 47000, t0 + 85000, t0 + 86000, t0 + 160000, t0 + 15000, 1700000000600]
    cam = {"sensor": {"activeArraySize": {"left": 0, "top": 0, "right": 1280, "bottom": 960}},
           "intrinsics": {"fx": 867.25, "fy": 866.75, "cx": 641.5, "cy": 478.25},
           "pose": {"translation": [0.031, -0.018, 0.062], "rotation": [0.1, -0.2, 0.05, 0.97]}}
    q = np.array(cam["pose"]["rotation"])
    cam["pose"]["rotation"] = [float(x) for x in q / np.linalg.norm(q)]
    png_names = [f"{t0 + 5000}.png", f"{t0 + 47000}.png", f"._{t0 + 15000}.png", f"_{t0 + 86000}.png", "notes.png",
                 f"{t0 + 160000}.png", f"{t0 + 230001}.png", f"{t0 + 200000}.png"]
    with tempfile.TemporaryDirectory() as tmp:
        project = Path(tmp).resolve()
        (project / "hmd_poses.csv").write_text(csv)
        (project / "left_camera_characteristics.json").write_text(json.dumps(cam))
        (project / "left_camera_rgb").mkdir()
        for n in png_names:
            (project / "left_camera_rgb" / n).write_bytes(b"")
        interp = ref.PoseInterpolator(project / "hmd_poses.csv")
        found, ppos, prot = [], [], []
        for ts in queries:
            r = interp.interpolate_pose(ts)
            found.append(r is not None)
            ppos.append(np.zeros(3) if r is None else np.asarray(r[0], np.float64))
            prot.append(np.zeros(4) if r is None else np.asarray(r[1], np.float64))
        io = ref.ImageDataIO(ref.ImagePathConfig(project))
        for side in (ref.Side.LEFT, ref.Side.RIGHT):
            c = io.load_camera_characteristics(side)
            out[f"cam_{side.value}_values"] = np.array([c.width, c.height, c.fx, c.fy, c.cx, c.cy], np.float64)
            out[f"cam_{side.value}_transl"] = np.asarray(c.transl, np.float64)
            out[f"cam_{side.value}_rot"] = np.asarray(c.rot_quat, np.float64)
        ds = io.build_color_dataset(ref.Side.LEFT)
        for k, v in ds.to_dict().items():
            out[f"ds_{k}"] = np.asarray(v)
        print("dataset", ds.image_file_names, ds.fx.dtype, ds.fx)
    out["pose_csv"] = np.array(csv)
    out["pose_times"] = np.array(queries, np.int64)
    out["pose_found"] = np.array(found)
    out["pose_pos"] = np.stack(ppos)
    out["pose_rot"] = np.stack(prot)
    out["cam_json"] = np.array(json.dumps(cam))
    out["ds_png_names"] = np.array(png_names)
    print("poses found", found)

    # ---- Transforms.apply_local_transform
    tr = ref.Transforms(coordinate_system=ref.CoordinateSystem.UNITY, positions=pos, rotations=quats)
    lp, lr = rng.normal(size=3), rng.normal(size=4)
    lr /= np.linalg.norm(lr)
    moved = tr.apply_local_transform(local_position=lp, local_rotation=lr)
    out.update(local_positions=pos, local_rotations=quats, local_lp=lp, local_lr=lr,
               local_out_positions=np.asarray(moved.positions), local_out_rotations=np.asarray(moved.rotations))

    path = os.path.join(HERE, "colorframes_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
