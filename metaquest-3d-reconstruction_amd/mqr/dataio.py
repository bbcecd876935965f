"""Capture-directory access (Quest layout): the depth side for the fusion path, and the colour side
(ColorPaths, ImageDataIO, PoseInterpolator below; raw camera frames are decoded by mqr.colorframes).

Mirror of the reference's ``DepthDataIO`` (scripts/dataio/depth_data_io.py:14-261) and of the
path layout in ``config/project_path_config.py:39-61, 148-196``:

    <project>/left_depth/<timestamp>.raw          float32 little-endian NDC depth buffer (H*W)
    <project>/left_depth_descriptors.csv          one row per frame (timestamp, size, near/far,
                                                  FOV tangents, UNITY pose)
    <project>/left_depth_confidence/<ts>.npz      {confidence_map f64, valid_count i32}
    <project>/dataset/left_depth_dataset.npz      DepthDataset cache

Same skip rules as the reference: missing file or invalid buffer (all 0, all 1, any NaN, any
negative) -> ``None`` and the frame is dropped.
"""
from __future__ import annotations

from pathlib import Path
from typing import Optional

import numpy as np

from .depth_utils import compute_depth_camera_params, convert_depth_to_linear
from .models import ConfidenceMap, CoordinateSystem, DepthDataset, Side, Transforms

DESCRIPTOR_COLUMNS = [
    "timestamp_ms", "width", "height", "near_z", "far_z",
    "fov_left_angle_tangent", "fov_right_angle_tangent", "fov_top_angle_tangent", "fov_down_angle_tangent",
    "create_pose_location_x", "create_pose_location_y", "create_pose_location_z",
    "create_pose_rotation_x", "create_pose_rotation_y", "create_pose_rotation_z", "create_pose_rotation_w",
]


class DepthPaths:
    def __init__(self, project_dir: Path):
        self.project_dir = Path(project_dir).resolve()

    def depth_dir(self, side: Side) -> Path:
        return self.project_dir / f"{side.value}_depth"

    def depth_map_path(self, side: Side, timestamp: int) -> Path:
        return self.depth_dir(side) / f"{int(timestamp)}.raw"

    def descriptor_path(self, side: Side) -> Path:
        return self.project_dir / f"{side.value}_depth_descriptors.csv"

    def confidence_dir(self, side: Side) -> Path:
        return self.project_dir / f"{side.value}_depth_confidence"

    def confidence_path(self, side: Side, timestamp: int) -> Path:
        return self.confidence_dir(side) / f"{int(timestamp)}.npz"

    def dataset_path(self, side: Side) -> Path:
        return self.project_dir / "dataset" / f"{side.value}_depth_dataset.npz"


class DepthDataIO:
    def __init__(self, project_dir: Path):
        self.paths = DepthPaths(project_dir)
        self.depth_datasets: dict = {}

    # -- descriptors / datasets --------------------------------------------------------
    def load_depth_descriptors(self, side: Side):
        import pandas as pd
        return pd.read_csv(self.paths.descriptor_path(side))

    def build_depth_dataset(self, side: Side) -> DepthDataset:
        df = self.load_depth_descriptors(side)
        cols = {c: [] for c in ("ts", "fx", "fy", "cx", "cy", "pos", "rot", "w", "h", "n", "f", "names")}
        for _, row in df.iterrows():
            ts, w, h = int(row["timestamp_ms"]), int(row["width"]), int(row["height"])
            near, far = float(row["near_z"]), float(row["far_z"])
            fx, fy, cx, cy = compute_depth_camera_params(
                float(row["fov_left_angle_tangent"]), float(row["fov_right_angle_tangent"]),
                float(row["fov_top_angle_tangent"]), float(row["fov_down_angle_tangent"]), w, h)
            if self.load_depth_map(side, ts, w, h, near, far) is None:
                continue
            cols["names"].append(f"{ts}.raw")
            cols["ts"].append(ts)
            cols["fx"].append(fx)
            cols["fy"].append(fy)
            cols["cx"].append(cx)
            cols["cy"].append(cy)
            cols["pos"].append(np.array([row["create_pose_location_x"], row["create_pose_location_y"],
                                         row["create_pose_location_z"]]))
            cols["rot"].append(np.array([row["create_pose_rotation_x"], row["create_pose_rotation_y"],
                                         row["create_pose_rotation_z"], row["create_pose_rotation_w"]]))
            cols["w"].append(w)
            cols["h"].append(h)
            cols["n"].append(near)
            cols["f"].append(far)
        rel = str(self.paths.depth_dir(side).relative_to(self.paths.project_dir))
        return DepthDataset(
            directory_relative_path=rel, image_file_names=np.array(cols["names"]), timestamps=np.array(cols["ts"]),
            fx=np.array(cols["fx"]), fy=np.array(cols["fy"]), cx=np.array(cols["cx"]), cy=np.array(cols["cy"]),
            transforms=Transforms(CoordinateSystem.UNITY, np.array(cols["pos"]), np.array(cols["rot"])),
            widths=np.array(cols["w"]), heights=np.array(cols["h"]), nears=np.array(cols["n"]),
            fars=np.array(cols["f"]))

    def load_depth_dataset(self, side: Side, use_cache: bool = True) -> DepthDataset:
        if side in self.depth_datasets:
            return self.depth_datasets[side]
        path = self.paths.dataset_path(side)
        if use_cache and path.exists():
            ds = DepthDataset.load(path)
        else:
            ds = self.build_depth_dataset(side)
            ds.save(path)
        self.depth_datasets[side] = ds
        return ds

    # -- depth maps -----------------------------------------------------------------------
    @staticmethod
    def is_depth_map_valid(depth_map: np.ndarray) -> bool:
        ok = (depth_map != 0).any() and (depth_map != 1).any()
        ok = ok and not np.isnan(depth_map).any()
        ok = ok and (depth_map >= 0).all()
        return bool(ok)

    def load_raw_depth(self, side: Side, timestamp: int, width: int, height: int) -> Optional[np.ndarray]:
        path = self.paths.depth_map_path(side, timestamp)
        if not path.exists():
            return None
        return np.fromfile(path, dtype="<f4").reshape((int(height), int(width)))

    def load_depth_map(self, side: Side, timestamp: int, width: int, height: int, near: float,
                       far: float) -> Optional[np.ndarray]:
        raw = self.load_raw_depth(side, timestamp, width, height)
        if raw is None or not self.is_depth_map_valid(raw):
            return None
        return convert_depth_to_linear(raw, near, far)

    def load_depth_map_by_index(self, side: Side, dataset: DepthDataset, index: int) -> Optional[np.ndarray]:
        if index < 0 or index >= len(dataset.timestamps):
            return None
        return self.load_depth_map(side, dataset.timestamps[index], dataset.widths[index], dataset.heights[index],
                                   dataset.nears[index], dataset.fars[index])

    # -- confidence maps --------------------------------------------------------------------
    def exists_depth_confidence_map_dir(self, side: Side) -> bool:
        return self.paths.confidence_dir(side).exists()

    def load_confidence_map(self, side: Side, timestamp: int) -> Optional[ConfidenceMap]:
        path = self.paths.confidence_path(side, timestamp)
        if not path.exists():
            return None
        try:
            data = np.load(path)
            return ConfidenceMap(confidence_map=data["confidence_map"], valid_count=data["valid_count"])
        except Exception as e:  # the reference logs and returns None (depth_data_io.py:100-103)
            print(f"[Error] Failed to load confidence map for {side.name} at timestamp {timestamp}: {e}")
            return None

    def save_confidence_map(self, side: Side, timestamp: int, confidence_map: ConfidenceMap) -> None:
        path = self.paths.confidence_path(side, timestamp)
        path.parent.mkdir(parents=True, exist_ok=True)
        np.savez(path, confidence_map=confidence_map.confidence_map, valid_count=confidence_map.valid_count)


# ======================================================================================= colour side
class ColorPaths:
    """The camera paths of the reference's ImagePathConfig (config/project_path_config.py:6-36, 84-127),
    under its method names:

        <project>/left_camera_raw/<timestamp>.yuv        raw YUV_420_888 frame
        <project>/left_camera_rgb/<timestamp>.png        converted frame
        <project>/left_camera_image_format.json          width, height, planes, base time
        <project>/left_camera_characteristics.json       intrinsics and the camera's pose on the headset
        <project>/hmd_poses.csv                          headset poses
        <project>/dataset/left_camera_dataset[_optimized].npz
    """

    def __init__(self, project_dir: Path):
        self.project_dir = Path(project_dir).resolve()

    def get_yuv_dir(self, side: Side) -> Path:
        return self.project_dir / f"{side.value}_camera_raw"

    def get_yuv_image_paths(self, side: Side) -> list:
        return sorted(self.get_yuv_dir(side).glob("*.yuv"))

    def get_rgb_dir(self, side: Side) -> Path:
        return self.project_dir / f"{side.value}_camera_rgb"

    def get_rgb_file_path(self, side: Side, timestamp: int) -> Path:
        return self.get_rgb_dir(side) / f"{timestamp}.png"

    def get_rgb_image_paths(self, side: Side) -> list:
        return sorted(self.get_rgb_dir(side).glob("*.png"))

    def get_camera_characteristic_json_path(self, side: Side) -> Path:
        return self.project_dir / f"{side.value}_camera_characteristics.json"

    def get_camera_format_format_json_path(self, side: Side) -> Path:
        return self.project_dir / f"{side.value}_camera_image_format.json"

    def get_hmd_pose_csv_path(self) -> Path:
        return self.project_dir / "hmd_poses.csv"

    def get_color_dataset_path(self, side: Side) -> Path:
        return self.project_dir / "dataset" / f"{side.value}_camera_dataset.npz"

    def get_optimized_color_dataset_path(self, side: Side) -> Path:
        return self.project_dir / "dataset" / f"{side.value}_camera_dataset_optimized.npz"

    def get_relative_path(self, path: Path) -> Path:
        return path.relative_to(self.project_dir)


class PoseInterpolator:
    """Headset pose at a camera timestamp (dataio/helpers/pose_interpolator.py): the nearest pose rows
    before and after it within 30 ms, linearly / spherically interpolated; one of them alone when the
    other is missing; None when neither is there.  The same pandas calls as the reference, so bad CSV
    lines, rows with gaps and duplicate times are treated alike."""

    def __init__(self, pose_csv_path: Path):
        self.pose_csv_path = pose_csv_path
        self._df = None

    @property
    def hmd_pose_df(self):
        if self._df is None:
            import pandas as pd
            df = pd.read_csv(self.pose_csv_path, on_bad_lines="skip").dropna()
            self._df = df.sort_values("unix_time").reset_index(drop=True)
        return self._df

    def find_nearest_frames(self, timestamp: int, window_ms: int = 30):
        window = window_ms * 1000
        df = self.hmd_pose_df
        before = df[df["unix_time"] <= timestamp]
        after = df[df["unix_time"] >= timestamp]
        prev = before.iloc[-1] if not before.empty and abs(timestamp - before.iloc[-1]["unix_time"]) <= window else None
        nxt = after.iloc[0] if not after.empty and abs(after.iloc[0]["unix_time"] - timestamp) <= window else None
        return prev, nxt

    def interpolate_pose(self, timestamp: int):
        from scipy.spatial.transform import Rotation, Slerp
        prev, nxt = self.find_nearest_frames(timestamp)
        if prev is None and nxt is None:
            return None

        def pos(r):
            return np.array([r["pos_x"], r["pos_y"], r["pos_z"]])

        def rot(r):
            return np.array([r["rot_x"], r["rot_y"], r["rot_z"], r["rot_w"]])

        if prev is None:
            return pos(nxt), rot(nxt)
        if nxt is None:
            return pos(prev), rot(prev)
        t0, t1 = prev["unix_time"], nxt["unix_time"]
        alpha = (timestamp - t0) / (t1 - t0) if t1 != t0 else 0.0
        rots = Rotation.from_quat([list(rot(prev)), list(rot(nxt))])
        return (1 - alpha) * pos(prev) + alpha * pos(nxt), Slerp([0, 1], rots)(alpha).as_quat()


class ImageDataIO:
    """The reference's ImageDataIO (scripts/dataio/image_data_io.py) without OpenCV: PNGs go through Pillow
    (mqr.colorframes.read_png / write_png), raw frames through mqr.colorframes.  `project_dir`: the capture
    directory, or a path object with ColorPaths' methods (the reference's ImagePathConfig)."""

    def __init__(self, project_dir):
        self.image_path_config = project_dir if hasattr(project_dir, "get_yuv_dir") else ColorPaths(project_dir)
        self.paths = self.image_path_config
        self._format_info: dict = {}

    # -- timestamps ------------------------------------------------------------------------
    def _parse_timestamp_stem(self, stem: str, filename: str, prefix: str) -> Optional[int]:
        if stem.startswith("._"):  # macOS resource-fork sidecar
            stem = stem[2:]
        elif stem.startswith("_"):
            stem = stem.lstrip("_")
        if stem == "" or not stem.isdigit():
            print(f"[Warning] Skipping non-timestamped {prefix} file: {filename}")
            return None
        return int(stem)

    def _timestamps(self, paths, prefix: str) -> list:
        out = []
        for p in paths:
            ts = self._parse_timestamp_stem(p.stem, p.name, prefix=prefix)
            if ts is not None:
                out.append(ts)
        return out

    def get_yuv_timestamps(self, side: Side) -> list:
        return self._timestamps(self.image_path_config.get_yuv_image_paths(side=side), "YUV")

    def get_rgb_timestamps(self, side: Side) -> list:
        return self._timestamps(self.image_path_config.get_rgb_image_paths(side=side), "RGB")

    # -- frames ----------------------------------------------------------------------------
    def _yuv_path(self, side: Side, timestamp: int) -> Path:
        return self.image_path_config.get_yuv_dir(side=side) / f"{timestamp}.yuv"

    def load_yuv(self, side: Side, timestamp: int) -> np.ndarray:
        return np.fromfile(self._yuv_path(side, timestamp), dtype=np.uint8)

    def _cached_format_info(self, side: Side):
        if side not in self._format_info:
            self._format_info[side] = self.load_image_format_info(side)
        return self._format_info[side]

    def load_rgb(self, side: Side, timestamp: int) -> np.ndarray:
        """(H,W,3) uint8 RGB: the PNG, or -- where there is none and the raw frame is there -- the raw
        frame converted on the host."""
        from . import colorframes
        path = self.image_path_config.get_rgb_file_path(side=side, timestamp=timestamp)
        if not path.exists() and self._yuv_path(side, timestamp).exists():
            bgr = colorframes.convert_yuv420_888_to_bgr(self.load_yuv(side, timestamp), self._cached_format_info(side))
            return np.ascontiguousarray(bgr[..., ::-1])
        return colorframes.read_png(path)

    def load_rgb_batch(self, side: Side, timestamps, device=None) -> np.ndarray:
        """(N,H,W,3) uint8 RGB frames of `timestamps`, in order: PNGs where they exist, the others decoded
        from their raw frames in one batch on `device` (default 0).  FileNotFoundError for a timestamp
        with neither; ValueError when the frames differ in size."""
        from . import colorframes
        from ._io import io_pool
        timestamps = [int(t) for t in timestamps]
        cfg = self.image_path_config
        raw_idx = [i for i, ts in enumerate(timestamps)
                   if not cfg.get_rgb_file_path(side=side, timestamp=ts).exists()]
        for i in raw_idx:
            if not self._yuv_path(side, timestamps[i]).exists():
                raise FileNotFoundError(f"Image file not found or cannot be read: "
                                        f"{cfg.get_rgb_file_path(side=side, timestamp=timestamps[i])}")
        frames: list = [None] * len(timestamps)
        raw_set = set(raw_idx)
        png_idx = [i for i in range(len(timestamps)) if i not in raw_set]
        for i, im in zip(png_idx, io_pool().map(lambda i: colorframes.read_png(
                cfg.get_rgb_file_path(side=side, timestamp=timestamps[i])), png_idx)):
            frames[i] = im
        if raw_idx:
            raws = list(io_pool().map(lambda i: self.load_yuv(side, timestamps[i]), raw_idx))
            rgb = colorframes.decode_color_frames(raws, self._cached_format_info(side), order="rgb",
                                                  device=0 if device is None else int(device))
            for k, i in enumerate(raw_idx):
                frames[i] = rgb[k]
        if len({f.shape for f in frames}) > 1:
            raise ValueError(f"colour frames of differing sizes: {sorted({f.shape[:2] for f in frames})}")
        if not frames:
            return np.zeros((0, 0, 0, 3), np.uint8)
        return np.stack(frames)

    def save_rgb(self, rgb: np.ndarray, side: Side, timestamp: int):
        from . import colorframes
        path = self.image_path_config.get_rgb_file_path(side=side, timestamp=timestamp)
        path.parent.mkdir(parents=True, exist_ok=True)
        colorframes.write_png(path, rgb)

    def save_bgr(self, bgr: np.ndarray, side: Side, timestamp: int):
        self.save_rgb(rgb=np.asarray(bgr)[..., ::-1], side=side, timestamp=timestamp)

    # -- records ---------------------------------------------------------------------------
    def load_image_format_info(self, side: Side):
        import json
        from .models import BaseTime, ImageFormatInfo, ImagePlaneInfo
        with open(self.image_path_config.get_camera_format_format_json_path(side)) as f:
            d = json.load(f)
        planes = [ImagePlaneInfo(buffer_size=p["bufferSize"], row_stride=p["rowStride"], pixel_stride=p["pixelStride"])
                  for p in d["planes"]]
        base = d["baseTime"]
        # (the reference stores baseUnixTimeMs in the field it calls unix_time_ns)
        return ImageFormatInfo(width=d["width"], height=d["height"], format=d["format"], planes=planes,
                               base_time=BaseTime(mono_time_ns=base["baseMonoTimeNs"],
                                                  unix_time_ns=base["baseUnixTimeMs"]))

    def load_camera_characteristics(self, side: Side):
        import json
        from scipy.spatial.transform import Rotation
        from .models import CameraCharacteristics
        cfg = self.image_path_config
        path = cfg.get_camera_characteristic_json_path(side)
        if not path.exists():  # reuse the other side's rather than fail
            other = Side.LEFT if side == Side.RIGHT else Side.RIGHT
            fallback = cfg.get_camera_characteristic_json_path(other)
            if not fallback.exists():
                raise FileNotFoundError(f"Camera characteristics JSON not found for {side.name} at {path} "
                                        f"and fallback {fallback} is also missing.")
            print(f"[Warning] Camera characteristics for {side.name} not found at {path}. "
                  f"Using {other.name} camera characteristics from {fallback} as a fallback.")
            path = fallback
        with open(path, "r", encoding="utf-8") as f:
            c = json.load(f)
        size = c["sensor"]["activeArraySize"]
        k = c["intrinsics"]
        transl = c["pose"]["translation"]
        transl[2] *= -1
        if len(transl) < 3:
            transl = np.array((0, 0, 0))
        q = c["pose"]["rotation"]
        if len(q) >= 4:
            rot = Rotation.from_quat((-q[0], -q[1], q[2], q[3])).inv()
            rot *= Rotation.from_euler("x", np.pi)  # Android camera pose -> headset world convention
            q = rot.as_quat()
        else:
            q = np.array((0, 0, 0, 1))
        return CameraCharacteristics(width=size["right"] - size["left"], height=size["bottom"] - size["top"],
                                     fx=k["fx"], fy=k["fy"], cx=k["cx"], cy=k["cy"], transl=transl, rot_quat=q)

    def load_hmd_poses(self):
        import pandas as pd
        path = self.image_path_config.get_hmd_pose_csv_path()
        if not path.exists():
            raise FileNotFoundError(f"HMD poses CSV file not found at {path}")
        return pd.read_csv(path)

    # -- datasets --------------------------------------------------------------------------
    def load_color_dataset(self, side: Side, use_cache: bool = True):
        from .models import CameraDataset
        path = self.image_path_config.get_color_dataset_path(side=side)
        if use_cache and path.exists():
            print(f"[Info] Loading cached color dataset for {side.name} from {path} ...")
            try:
                return CameraDataset.load(path)
            except Exception as e:
                print(f"[Error] Color dataset cache is corrupted or invalid. Rebuilding cache from the original source\n{e}")
        else:
            print(f"[Info] Color dataset not found for {side.name}. Rebuilding cache from the original source...")
        ds = self.build_color_dataset(side=side)
        ds.save(path)
        return ds

    def load_optimized_color_dataset(self, side: Side):
        from .models import CameraDataset
        path = self.image_path_config.get_optimized_color_dataset_path(side=side)
        if path.exists():
            try:
                return CameraDataset.load(path)
            except Exception:
                print("[Error] Optimized color dataset cache is corrupted or invalid.")
        return None

    def save_optimized_color_dataset(self, dataset, side: Side):
        path = self.image_path_config.get_optimized_color_dataset_path(side=side)
        path.parent.mkdir(parents=True, exist_ok=True)
        dataset.save(path)

    def build_color_dataset(self, side: Side):
        """image_data_io.py:228-297.  One difference, for the PNG-free path: when the RGB directory holds
        no PNG, the frames listed are the raw ``.yuv`` ones (directory and file names then name those)."""
        from .models import CameraDataset
        cfg = self.image_path_config
        interpolator = PoseInterpolator(pose_csv_path=cfg.get_hmd_pose_csv_path())
        cam = self.load_camera_characteristics(side=side)
        paths, prefix, directory = cfg.get_rgb_image_paths(side=side), "RGB", cfg.get_rgb_dir(side=side)
        if not paths:
            paths, prefix, directory = cfg.get_yuv_image_paths(side=side), "YUV", cfg.get_yuv_dir(side=side)
        names, timestamps, positions, rotations = [], [], [], []
        for path in paths:
            ts = self._parse_timestamp_stem(path.stem, path.name, prefix=prefix)
            if ts is None:
                continue
            pose = interpolator.interpolate_pose(ts)
            if pose is None:
                print(f"[Warning] No pose found for timestamp {ts}. Skipping this image.")
                continue
            names.append(path.name)
            timestamps.append(ts)
            positions.append(pose[0])
            rotations.append(pose[1])
        if len(timestamps) == 0:
            raise Exception("[Error] No valid timestamps found. Unable to build color dataset for side: {}.".format(
                side.name))
        hmd = Transforms(coordinate_system=CoordinateSystem.UNITY, positions=np.array(positions),
                         rotations=np.array(rotations))
        camera = hmd.apply_local_transform(local_position=cam.transl, local_rotation=cam.rot_quat)
        # (np.full_like of the integer timestamps, as the reference: the intrinsics are truncated to integers)
        return CameraDataset(
            directory_relative_path=str(cfg.get_relative_path(directory)), image_file_names=np.array(names),
            timestamps=np.array(timestamps), fx=np.full_like(timestamps, cam.fx), fy=np.full_like(timestamps, cam.fy),
            cx=np.full_like(timestamps, cam.cx), cy=np.full_like(timestamps, cam.cy), transforms=camera,
            widths=np.full_like(timestamps, cam.width), heights=np.full_like(timestamps, cam.height))


# ======================================================================================= reconstruction side
class ReconstructionPaths:
    """The result paths of the reference's ReconstructionPathConfig (config/project_path_config.py:229-247),
    under its method names:

        <project>/reconstruction/colorless_vbg.npz          the fused volume
        <project>/reconstruction/colorless.ply              its point cloud
        <project>/reconstruction/colorless_mesh_raw.ply     the extracted mesh
        <project>/reconstruction/colorless_mesh_clean.ply   ... after the component filter
        <project>/reconstruction/color_mesh.ply             the coloured mesh
        <project>/reconstruction/color.ply                  the coloured point cloud sampled from it
    """

    def __init__(self, project_dir: Path):
        self.project_dir = Path(project_dir).resolve()

    def _result(self, name: str) -> Path:
        return self.project_dir / "reconstruction" / name

    def get_colorless_vbg_path(self) -> Path:
        return self._result("colorless_vbg.npz")

    def get_colorless_pcd_path(self) -> Path:
        return self._result("colorless.ply")

    def get_colorless_mesh_raw_path(self) -> Path:
        return self._result("colorless_mesh_raw.ply")

    def get_colorless_mesh_clean_path(self) -> Path:
        return self._result("colorless_mesh_clean.ply")

    def get_colored_mesh_path(self) -> Path:
        return self._result("color_mesh.ply")

    def get_colored_pcd_path(self) -> Path:
        return self._result("color.ply")

    def get_relative_path(self, path: Path) -> Path:
        return path.relative_to(self.project_dir)


class ReconstructionDataIO:
    """The result writers of the reference's ReconstructionDataIO (scripts/dataio/reconstruction_data_io.py:
    42-145) without Open3D: PLY files go through mqr.geometry's host writers (binary, Open3D's legacy layout;
    colours as ``uchar red / green / blue`` when the geometry has them), the volume through
    ``VoxelBlockGrid.save`` / ``load``.  `project_dir`: the capture directory, or a path object with
    ReconstructionPaths' methods (the reference's ReconstructionPathConfig).  The ``_legacy`` writers take
    what ``to_legacy()`` returns -- with or without Open3D installed -- or the tensor geometry itself; a
    geometry held in HBM is copied to the host once, by the write."""

    def __init__(self, project_dir):
        self.reconstruction_path_config = (project_dir if hasattr(project_dir, "get_colored_pcd_path")
                                           else ReconstructionPaths(project_dir))
        self.paths = self.reconstruction_path_config

    @staticmethod
    def _ready(path: Path) -> str:
        path.parent.mkdir(parents=True, exist_ok=True)
        return str(path)

    # -- the volume ------------------------------------------------------------------------
    def load_colorless_vbg(self, device=None):
        from .vbg import VoxelBlockGrid
        path = self.paths.get_colorless_vbg_path()
        if not path.exists():
            return None
        return VoxelBlockGrid.load(str(path), device=device)

    def save_colorless_vbg(self, vbg):
        vbg.save(self._ready(self.paths.get_colorless_vbg_path()))

    # -- colourless geometry ---------------------------------------------------------------
    def save_colorless_pcd_legacy(self, pcd):
        from .geometry import write_point_cloud
        write_point_cloud(self._ready(self.paths.get_colorless_pcd_path()), pcd, write_ascii=False, compressed=True)

    def save_colorless_mesh_raw_legacy(self, mesh):
        from .geometry import write_triangle_mesh
        write_triangle_mesh(self._ready(self.paths.get_colorless_mesh_raw_path()), mesh)

    def save_colorless_mesh_clean_legacy(self, mesh):
        from .geometry import write_triangle_mesh
        write_triangle_mesh(self._ready(self.paths.get_colorless_mesh_clean_path()), mesh)

    # -- coloured geometry -----------------------------------------------------------------
    def load_colored_mesh(self):
        from .geometry import read_triangle_mesh
        path = self.paths.get_colored_mesh_path()
        return read_triangle_mesh(str(path)) if path.exists() else None

    def save_colored_mesh_legacy(self, mesh):
        from .geometry import write_triangle_mesh
        write_triangle_mesh(self._ready(self.paths.get_colored_mesh_path()), mesh)

    def save_colored_mesh(self, mesh):
        self.save_colored_mesh_legacy(mesh)

    def load_colored_pcd(self, device=None, print_progress: bool = True):
        from .geometry import read_point_cloud
        path = self.paths.get_colored_pcd_path()
        if not path.exists():
            return None
        pcd = read_point_cloud(str(path))
        return pcd if device is None else pcd.to(device)

    def save_colored_pcd_legacy(self, pcd):
        from .geometry import write_point_cloud
        write_point_cloud(self._ready(self.paths.get_colored_pcd_path()), pcd, write_ascii=False, compressed=True)

    def save_colored_pcd(self, pcd):
        self.save_colored_pcd_legacy(pcd)


class RGBDPaths:
    """Colour-aligned depth maps (config/project_path_config.py RGBDPathConfig):
    ``<project>/<side>_color_aligned_depth/<timestamp>.npy``."""

    COLOR_ALIGNED_DEPTH_DIR_MAP = {Side.LEFT: "left_color_aligned_depth", Side.RIGHT: "right_color_aligned_depth"}

    def __init__(self, project_dir: Path):
        self.project_dir = Path(project_dir)

    def get_color_aligned_depth_filename(self, timestamp: int) -> str:
        return f"{timestamp}.npy"

    def get_color_aligned_depth_dir(self, side: Side) -> Path:
        return self.project_dir / self.COLOR_ALIGNED_DEPTH_DIR_MAP[side]

    def get_color_aligned_depth_path(self, side: Side, timestamp: int) -> Path:
        return self.get_color_aligned_depth_dir(side) / self.get_color_aligned_depth_filename(timestamp)


class RGBDDataIO:
    """The reference's ``RGBDDataIO`` (scripts/dataio/rgbd_data_io.py): one ``np.save`` file per colour frame."""

    def __init__(self, image_data_io, depth_data_io, rgbd_path_config: RGBDPaths):
        self.image_data_io = image_data_io
        self.depth_data_io = depth_data_io
        self.rgbd_path_config = rgbd_path_config

    def load_color_aligned_depth(self, side: Side, timestamp: int) -> np.ndarray:
        path = self.rgbd_path_config.get_color_aligned_depth_path(side=side, timestamp=timestamp)
        if not path.exists():
            raise FileNotFoundError(f"Color-aligned depth file not found: {path}")
        return np.load(path)

    def save_color_aligned_depth(self, depth_map: np.ndarray, side: Side, timestamp: int):
        path = self.rgbd_path_config.get_color_aligned_depth_path(side=side, timestamp=timestamp)
        path.parent.mkdir(parents=True, exist_ok=True)
        np.save(path, depth_map)


class DataIO:
    """A capture directory: ``.depth`` (DepthDataIO), ``.color`` (ImageDataIO), ``.rgbd`` (RGBDDataIO, the
    colour-aligned depth maps) and ``.reconstruction`` (ReconstructionDataIO, the results)."""

    def __init__(self, project_dir: Path):
        self.project_dir = Path(project_dir).resolve()
        self.depth = DepthDataIO(self.project_dir)
        self.color = ImageDataIO(self.project_dir)
        self.rgbd = RGBDDataIO(self.color, self.depth, RGBDPaths(self.project_dir))
        self.reconstruction = ReconstructionDataIO(self.project_dir)
