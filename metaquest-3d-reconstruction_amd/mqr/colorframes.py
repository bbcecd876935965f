"""Colour-frame ingestion: Quest camera frames (``<side>_camera_raw/<ts>.yuv``, Android YUV_420_888) to
RGB on the GPU, with the reference's frame filters -- the colour twin of ``mqr.ingest``.  Mirrors

    convert_yuv420_888_to_i420 / _to_bgr, is_blur_image, is_over_or_under_exposed   scripts/utils/image_utils.py
    process_file, FilterFn, convert_yuv_directory            scripts/processing/yuv_conversion/convert_yuv_dir.py

``decode_color_frames`` decodes a batch on the device (libmqr_hip.so: colorframes.hip) into the
``(N,H,W,3)`` uint8 layout ``mqr.color`` reads, optionally with two exact per-frame statistics: the
256-bin histogram of the blue channel (the exposure verdict -- the reference's FilterFn hands the BGR image
to a function that reads channel 0) and the integer sums of the grey image's 3x3 Laplacian and of its
square (the blur score).  ``device=None`` selects the vectorised host path instead, which is also what
``convert_yuv420_888_to_i420`` / ``_to_bgr`` are.

The reference unpacks a frame in three branches; ``resolve_layout`` turns them into one byte-addressing
record, quirks included (U starts at ``planes[0].buffer_size`` whatever the Y rows cover; with a chroma
pixel stride other than 1, U and V are both read from the U plane's rows at an element step of 2 whatever
the pixel stride says, V one byte after U, swapped for "NV21").

Parity UNPINNED against OpenCV: the I420 -> BGR conversion, BGR -> grey and the ksize-1 Laplacian restate
OpenCV 4.x as recalled (``cv2`` was not available); the constants live in csrc/color_convert.hpp alone and
reach the host path through ``mqr_color_constants``.

Two known departures from the reference: a frame file so short that a row has exactly ONE of its bytes is
an error here (numpy broadcasts that byte over the reference's row), and the blur score is the exactly
rounded variance where the reference's ``ndarray.var()`` carries a few ulp of float64 rounding.
"""
from __future__ import annotations

import ctypes
import shutil
import traceback
from dataclasses import dataclass, fields
from typing import Optional

import numpy as np

from . import _lib
from ._lib import MQR_DEVICE, MQR_HOST, call, ptr
from .models import Side


# ------------------------------------------------------------------------------------------- layout
@dataclass(frozen=True)
class YuvLayout:
    """Byte (row, col) of a plane sits at base + row * row_stride + col * step of its frame; every such
    byte lies below valid_bytes (mqr_yuv_layout, include/mqr.h)."""
    y_base: int
    y_row_stride: int
    y_pixel_stride: int
    u_base: int
    u_row_stride: int
    u_step: int
    v_base: int
    v_row_stride: int
    v_step: int
    valid_bytes: int


class _CLayout(ctypes.Structure):
    _fields_ = [(f.name, ctypes.c_int64) for f in fields(YuvLayout)]


def _layout(format_info, uv_order: str, n_bytes: int) -> YuvLayout:
    """The reference's unpacking (image_utils.py:19-57) as a layout; ValueError where its numpy row
    assignment raises: a plane row it reads is not wholly inside the n_bytes of the file."""
    planes = format_info.planes
    if len(planes) != 3:
        raise ValueError("Expected 3 planes for YUV420_888 format")
    W, H, n = int(format_info.width), int(format_info.height), int(n_bytes)
    cw, ch = W // 2, H // 2
    u_off = int(planes[0].buffer_size)
    ps_uv, rs_uv = int(planes[1].pixel_stride), int(planes[1].row_stride)
    if ps_uv == 1:
        v_off = u_off + int(planes[1].buffer_size)
        u = (u_off, rs_uv, 1)
        v = (v_off, int(planes[2].row_stride), 1)
    else:  # both from the U plane's rows, element step 2 whatever ps_uv is; a row slice holds cw * ps_uv bytes
        if 2 * (cw - 1) + 1 >= cw * ps_uv and cw > 0:
            raise ValueError(f"chroma pixel stride {ps_uv} leaves no interleaved (U,V) pairs to read")
        first, second = (u_off, rs_uv, 2), (u_off + 1, rs_uv, 2)
        u, v = (second, first) if uv_order == "NV21" else (first, second)
    lay = YuvLayout(0, int(planes[0].row_stride), int(planes[0].pixel_stride), *u, *v, n)
    for name, base, rs, step, rows, cols in (("Y", lay.y_base, lay.y_row_stride, lay.y_pixel_stride, H, W),
                                             ("U", lay.u_base, lay.u_row_stride, lay.u_step, ch, cw),
                                             ("V", lay.v_base, lay.v_row_stride, lay.v_step, ch, cw)):
        if rows <= 0 or cols <= 0:
            continue
        if base < 0 or rs < 0 or step <= 0:
            raise ValueError(f"{name} plane: base {base}, row stride {rs}, step {step} cannot be unpacked")
        last = base + (rows - 1) * rs + (cols - 1) * step
        if last >= n:
            raise ValueError(f"{name} plane needs byte {last} of a frame of {n} bytes "
                             f"(could not broadcast a short row into shape ({cols},))")
    return lay


def resolve_layout(format_info, uv_order: str = "NV12", n_bytes: Optional[int] = None) -> YuvLayout:
    """The kernel's plane layout for frames of `n_bytes` bytes (default: the three buffer sizes together).
    ValueError for anything the reference's conversion raises on: not three planes, an odd width or
    height (its reshape), a file too short for a row it reads."""
    if len(format_info.planes) != 3:
        raise ValueError("Expected 3 planes for YUV420_888 format")
    W, H = int(format_info.width), int(format_info.height)
    if W <= 0 or H <= 0 or W % 2 or H % 2:
        raise ValueError(f"cannot reshape an I420 buffer of a {W}x{H} frame: width and height must be even")
    if n_bytes is None:
        n_bytes = sum(int(p.buffer_size) for p in format_info.planes)
    return _layout(format_info, uv_order, n_bytes)


def _bytes(raw_data) -> np.ndarray:
    a = np.frombuffer(raw_data, dtype=np.uint8) if not isinstance(raw_data, np.ndarray) else raw_data
    if a.dtype != np.uint8:
        a = np.frombuffer(np.ascontiguousarray(a), dtype=np.uint8)
    return np.ascontiguousarray(a).reshape(-1)


def _plane(buf: np.ndarray, base: int, rs: int, step: int, rows: int, cols: int) -> np.ndarray:
    """(rows, cols) strided view of a validated plane."""
    if rows <= 0 or cols <= 0:
        return np.empty((max(rows, 0), max(cols, 0)), np.uint8)
    return np.lib.stride_tricks.as_strided(buf[base:], shape=(rows, cols), strides=(rs, step), writeable=False)


def _planes(buf, lay: YuvLayout, W: int, H: int):
    return (_plane(buf, lay.y_base, lay.y_row_stride, lay.y_pixel_stride, H, W),
            _plane(buf, lay.u_base, lay.u_row_stride, lay.u_step, H // 2, W // 2),
            _plane(buf, lay.v_base, lay.v_row_stride, lay.v_step, H // 2, W // 2))


def convert_yuv420_888_to_i420(raw_data, format_info, uv_order="NV12") -> np.ndarray:
    """The frame's Y, U and V planes packed one after another (image_utils.py:19-57), without the row loop."""
    buf = _bytes(raw_data)
    y, u, v = _planes(buf, _layout(format_info, uv_order, buf.size), int(format_info.width), int(format_info.height))
    return np.concatenate([y.ravel(), u.ravel(), v.ravel()])


# ------------------------------------------------------------------------------------------- arithmetic
_CONSTANTS = None


def color_constants() -> dict:
    """The integer constants of the colour arithmetic, from the library (csrc/color_convert.hpp)."""
    global _CONSTANTS
    if _CONSTANTS is None:
        out = np.zeros(10, np.int32)
        call("mqr_color_constants", ptr(out, _lib._i32p), 10)
        names = ("CY", "CUB", "CUG", "CVG", "CVR", "SHIFT", "GREY_B", "GREY_G", "GREY_R", "GREY_SHIFT")
        _CONSTANTS = {k: int(x) for k, x in zip(names, out)}
    return _CONSTANTS


def _yuv_to_image(y, u, v, order: str) -> np.ndarray:
    """(..., H, W) Y and (..., H/2, W/2) U, V uint8 -> (..., H, W, 3) uint8 in `order`."""
    c = color_constants()
    rnd, sh = 1 << (c["SHIFT"] - 1), c["SHIFT"]
    yy = np.maximum(y.astype(np.int32) - 16, 0) * c["CY"]
    uu, vv = u.astype(np.int32) - 128, v.astype(np.int32) - 128

    def up(t):  # one chroma term per 2x2 block
        return np.repeat(np.repeat(t, 2, axis=-2), 2, axis=-1)

    r = np.clip((yy + up(rnd + c["CVR"] * vv)) >> sh, 0, 255)
    g = np.clip((yy + up(rnd + c["CVG"] * vv + c["CUG"] * uu)) >> sh, 0, 255)
    b = np.clip((yy + up(rnd + c["CUB"] * uu)) >> sh, 0, 255)
    return np.stack((b, g, r) if order == "bgr" else (r, g, b), axis=-1).astype(np.uint8)


def convert_yuv420_888_to_bgr(raw_data, format_info, uv_order="NV12") -> np.ndarray:
    """(H,W,3) uint8 BGR image of one frame (image_utils.py:60-71), on the host."""
    buf = _bytes(raw_data)
    lay = resolve_layout(format_info, uv_order, buf.size)
    return _yuv_to_image(*_planes(buf, lay, int(format_info.width), int(format_info.height)), "bgr")


def _order(order: str) -> str:
    o = str(order).lower()
    if o not in ("rgb", "bgr"):
        raise ValueError(f"order must be 'rgb' or 'bgr', got {order!r}")
    return o


def frame_statistics(images: np.ndarray, order: str = "bgr"):
    """Host computation of the device's statistics for (N,H,W,3) or (H,W,3) uint8 images in `order`:
    (hist (N,256) uint32 of the blue channel, sums (N,2) int64 = sum and sum of squares of the grey
    image's ksize-1 Laplacian, border reflect-101)."""
    c = color_constants()
    im = np.asarray(images, dtype=np.uint8)
    im = im[None] if im.ndim == 3 else im
    bi, ri = (0, 2) if _order(order) == "bgr" else (2, 0)
    hist = np.stack([np.bincount(f[..., bi].ravel(), minlength=256) for f in im]).astype(np.uint32)
    x = im.astype(np.int64)
    grey = (c["GREY_B"] * x[..., bi] + c["GREY_G"] * x[..., 1] + c["GREY_R"] * x[..., ri]
            + (1 << (c["GREY_SHIFT"] - 1))) >> c["GREY_SHIFT"]
    p = np.pad(grey, ((0, 0), (1, 1), (1, 1)), mode="reflect")
    lap = p[:, :-2, 1:-1] + p[:, 2:, 1:-1] + p[:, 1:-1, :-2] + p[:, 1:-1, 2:] - 4 * grey
    sums = np.stack([lap.sum(axis=(1, 2)), (lap * lap).sum(axis=(1, 2))], axis=1).astype(np.int64)
    return hist, sums


# ------------------------------------------------------------------------------------------- device decode
def _pack_frames(raw):
    """-> (argument, location, N, n_bytes, frame stride, keep-alive)."""
    from .ingest import ctypes_ptr
    if isinstance(raw, tuple):
        p, N, n_bytes = raw
        return ctypes_ptr(p), MQR_DEVICE, int(N), int(n_bytes), int(n_bytes), raw
    if isinstance(raw, np.ndarray) and raw.ndim == 2:
        a = np.ascontiguousarray(raw, dtype=np.uint8)
        return ptr(a), MQR_HOST, a.shape[0], a.shape[1], a.shape[1], a
    frames = [_bytes(r) for r in raw]
    sizes = {f.size for f in frames}
    if len(sizes) > 1:
        raise ValueError(f"frames of one batch must have one size, got {sorted(sizes)}")
    n_bytes = sizes.pop() if sizes else 0
    stride = (n_bytes + 3) & ~3  # frame bases 4-byte aligned: the kernel's wide loads apply
    a = np.zeros((len(frames), stride), np.uint8)
    for i, f in enumerate(frames):
        a[i, :n_bytes] = f
    return ptr(a), MQR_HOST, len(frames), n_bytes, stride, a


def decode_color_frames(raw, format_info, uv_order="NV12", order="rgb", stats=False, device=0, out_ptr=None):
    """Decode N equally laid-out raw frames.  raw: a list of byte arrays, an (N, n_bytes) uint8 array
    (frames packed back to back, whatever their size) or (device_ptr, N, n_bytes) for frames in HBM.

    Returns the (N,H,W,3) uint8 images in `order` ("rgb" / "bgr") as a host array, or None when `out_ptr`
    (a device pointer with room for N*H*W*3 bytes) received them; with `stats`, (images, hist, sums):
    hist (N,256) uint32 of the blue channel, sums (N,2) int64 (see frame_statistics).  device=None: the
    host path (no GPU touched; raw and the result on the host)."""
    order = _order(order)
    W, H = int(format_info.width), int(format_info.height)
    if device is None:
        if isinstance(raw, tuple) or out_ptr is not None:
            raise ValueError("device=None (the host path) takes and returns host arrays")
        frames = [_bytes(r) for r in raw]
        lays = [resolve_layout(format_info, uv_order, f.size) for f in frames]
        img = np.empty((len(frames), H, W, 3), np.uint8)
        for i, (f, lay) in enumerate(zip(frames, lays)):
            img[i] = _yuv_to_image(*_planes(f, lay, W, H), order)
        return (img, *frame_statistics(img, order)) if stats else img
    arg, loc, N, n_bytes, stride, keep = _pack_frames(raw)
    if N == 0:
        empty = np.zeros((0, H, W, 3), np.uint8) if out_ptr is None else None
        return (empty, np.zeros((0, 256), np.uint32), np.zeros((0, 2), np.int64)) if stats else empty
    lay = resolve_layout(format_info, uv_order, n_bytes)
    c_lay = _CLayout(*(getattr(lay, f.name) for f in fields(YuvLayout)))
    out = None
    if out_ptr is None:
        out = np.empty((N, H, W, 3), np.uint8)
        out_arg, out_loc = ptr(out), MQR_HOST
    else:
        from .ingest import ctypes_ptr
        out_arg, out_loc = ctypes_ptr(out_ptr), MQR_DEVICE
    hist = np.zeros((N, 256), np.uint32) if stats else None
    sums = np.zeros((N, 2), np.int64) if stats else None
    call("mqr_decode_color_frames", int(device), arg, loc, N, stride, W, H, ctypes.c_void_p(ctypes.addressof(c_lay)),
         int(order == "bgr"), out_arg, out_loc, None if hist is None else ptr(hist), None if sums is None else ptr(sums))
    del keep
    return (out, hist, sums) if stats else out


# ------------------------------------------------------------------------------------------- frame filters
def blur_score(sums, n_pixels: int) -> float:
    """Population variance of the Laplacian from its exact sums (sum x, sum x^2) over n_pixels values:
    (n * sum x^2 - (sum x)^2) / n^2 in Python integers, then one true division -- the correctly rounded
    float64 of the exact rational."""
    s1, s2, n = int(sums[0]), int(sums[1]), int(n_pixels)
    if n <= 0:
        raise ValueError("blur_score needs at least one pixel")
    return (n * s2 - s1 * s1) / (n * n)


def is_blur_image(img_bgr, blur_threshold=50.0, sums=None) -> bool:
    """image_utils.py:86-90.  `sums`: the frame's Laplacian sums from the device, with img_bgr then only
    needed for its shape (or an (H, W) pair)."""
    if sums is None:
        sums = frame_statistics(img_bgr, "bgr")[1][0]
    shape = img_bgr.shape if hasattr(img_bgr, "shape") else tuple(img_bgr)
    return bool(blur_score(sums, int(shape[0]) * int(shape[1])) < blur_threshold)


def is_over_or_under_exposed(img, low_thresh=0.02, high_thresh=0.02, hist=None) -> bool:
    """image_utils.py:78-83: the verdict on channel 0 of whatever image it is given (the reference's
    FilterFn gives the BGR image: blue), with its float32 ``hist / hist.sum()`` and ``np.cumsum``.
    `hist`: that channel's 256 integer counts from the device; img is then not read (may be None)."""
    if hist is None:
        a = np.asarray(img, dtype=np.uint8)
        hist = np.bincount((a[..., 0] if a.ndim == 3 else a).ravel(), minlength=256)
    h = np.asarray(hist).astype(np.float32).ravel()  # cv2.calcHist returns float32 counts
    h = h / h.sum()
    cum = np.cumsum(h)
    return bool(cum[5] > low_thresh or cum[250] < high_thresh)


class FilterFn:
    """convert_yuv_dir.py:40-54: True keeps the frame.  hist / sums: the device's statistics of the frame."""

    def __init__(self, config):
        self.config = config

    def __call__(self, bgr_img, hist=None, sums=None) -> bool:
        if self.config.blur_filter and is_blur_image(bgr_img, blur_threshold=self.config.blur_threshold, sums=sums):
            return False
        if self.config.exposure_filter and is_over_or_under_exposed(
                bgr_img, low_thresh=self.config.exposure_threshold_low,
                high_thresh=self.config.exposure_threshold_high, hist=hist):
            return False
        return True


# ------------------------------------------------------------------------------------------- PNG
def _pillow():
    try:
        from PIL import Image
    except ImportError as e:
        raise ImportError("reading and writing PNG colour frames needs Pillow (PIL), which is not installed; "
                          "the raw-frame path (decode_color_frames, load_rgb_batch on .yuv files) works without it"
                          ) from e
    return Image


def write_png(path, rgb: np.ndarray) -> None:
    _pillow().fromarray(np.ascontiguousarray(rgb, dtype=np.uint8), "RGB").save(str(path), format="PNG",
                                                                               compress_level=3)


def read_png(path) -> np.ndarray:
    """(H,W,3) uint8 RGB."""
    Image = _pillow()
    try:
        with Image.open(str(path)) as im:
            return np.asarray(im.convert("RGB"), dtype=np.uint8)
    except (FileNotFoundError, OSError) as e:
        raise FileNotFoundError(f"Image file not found or cannot be read: {path}") from e


# ------------------------------------------------------------------------------------------- directory
def convert_yuv_directory(image_io, config, write_png=True, remove_yuv=True, device=0, batch=32,
                          return_images=True, sides=None):
    """convert_yuv_dir.py:57-105 without the per-frame host work: for each side the raw frames are read on
    mqr._io.io_pool, decoded `batch` at a time on `device` (None: the host path) together with the
    statistics the enabled filters need, filtered, and (write_png) written as PNG through
    image_io.save_rgb.  Prints the reference's summary lines; removes a side's raw directory only when
    remove_yuv and the side finished without exceptions.

    Returns {side: (kept timestamps, (K,H,W,3) uint8 RGB images of the kept frames, or None unless
    return_images)}, so a caller can go on without the PNGs."""
    from ._io import io_pool
    keep_fn = FilterFn(config)
    want_stats = bool(config.blur_filter or config.exposure_filter)
    result = {}
    for side in (Side if sides is None else sides):
        cfg = image_io.image_path_config
        timestamps = image_io.get_yuv_timestamps(side)
        processed = excluded = failed = 0
        kept_ts, kept_img = [], []

        def fail(ts, text):
            nonlocal failed
            failed += 1
            print(f"[Exception] Worker failed: Failed in {side}/{ts}:\n{text}")

        def load(ts):
            try:
                return image_io.load_yuv(side=side, timestamp=ts), None
            except Exception:
                return None, traceback.format_exc()

        fmt, fmt_error = None, None
        if timestamps:
            try:
                fmt = image_io.load_image_format_info(side=side)
            except Exception:
                fmt_error = traceback.format_exc()
        by_size = {}  # frame size -> [(timestamp, bytes)], in timestamp order
        for ts, (raw, err) in zip(timestamps, io_pool().map(load, timestamps)):
            if err is None and fmt_error is not None:
                err = fmt_error
            if err is None:
                try:
                    resolve_layout(fmt, "NV12", raw.size)
                except Exception:
                    err = traceback.format_exc()
            if err is not None:
                fail(ts, err)
            else:
                by_size.setdefault(raw.size, []).append((ts, raw))
        decoded = {}  # timestamp -> (rgb image, keep)
        for group in by_size.values():
            for s in range(0, len(group), max(1, int(batch))):
                part = group[s:s + max(1, int(batch))]
                try:
                    got = decode_color_frames([r for _, r in part], fmt, order="rgb", stats=want_stats, device=device)
                    imgs, hist, sums = got if want_stats else (got, None, None)
                except Exception:
                    text = traceback.format_exc()
                    for ts, _ in part:
                        fail(ts, text)
                    continue
                for i, (ts, _) in enumerate(part):
                    keep = keep_fn(imgs[i].shape, hist[i], sums[i]) if want_stats else True
                    decoded[ts] = (imgs[i], keep)
        for ts in timestamps:
            if ts not in decoded:
                continue
            img, keep = decoded.pop(ts)
            if not keep:
                excluded += 1
                continue
            try:
                if write_png:
                    image_io.save_rgb(rgb=img, side=side, timestamp=ts)
            except Exception:
                fail(ts, traceback.format_exc())
                continue
            processed += 1
            kept_ts.append(ts)
            if return_images:
                kept_img.append(img)

        print(f"[Info] {processed} images written to {cfg.get_rgb_dir(side)}")
        if excluded > 0:
            print(f"[Info] {excluded} images were excluded by filtering.")
        if failed > 0:
            print(f"[Error] {failed} files failed due to exceptions.")
        yuv_dir = cfg.get_yuv_dir(side=side)
        if remove_yuv and failed == 0 and yuv_dir.exists():
            try:
                shutil.rmtree(yuv_dir)
                print(f"[Info] Cleaned up raw YUV directory after conversion: {yuv_dir}")
            except Exception as e:
                print(f"[Warning] Failed to remove raw YUV directory {yuv_dir}: {e}")
        elif failed > 0:
            print(f"[Warning] Keeping raw YUV directory for debugging: {yuv_dir}")
        images = None
        if return_images:
            images = np.stack(kept_img) if kept_img else np.zeros((0, 0, 0, 3), np.uint8)
        result[side] = (kept_ts, images)
    return result
