"""The colour-frame decode on the GPU, timed.

A batch of `--frames` (64) raw camera frames of 1280x960 in an NV12 layout with padded row strides (1344
bytes per row) and Android's short chroma planes, random bytes.  (The reference records no frame size: it is
read per capture from <side>_camera_image_format.json, so 1280x960 is this probe's choice, the active array of
the golden camera record, and not a figure of the reference's.)  After `--warmup` untimed rounds, `--repeats`
rounds time:

  decode alone / decode with statistics, frames and images in HBM: the kernels' device time from hip events
      around them on the library's stream (mqr_color_frames_last_ms), and the whole call under the host clock;
  the same two calls with frames and images on the host: the difference to the device time is the staging
      (upload of the frames, download of the images, through the library's copy helpers);
  the host path (mqr.colorframes.decode_color_frames(device=None)) on `--host-frames` frames, for context.

Algorithmic bytes: decode 1.5 W H read + 3 W H written per frame; the statistics pass reads the 3 W H image
again (its halo re-reads, 18 x 66 positions per 16 x 64 tile, are not counted) and writes 1040 bytes per frame.
GB/s = those bytes over the device time, and as a fraction of the MI355X's 8 TB/s HBM peak.  No figure here
is a pass criterion.  Writes profiles/color_frames.json and prints it.

    python tools/color_frames_probe.py [--repeats 20] [--warmup 3] [--frames 64]
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "metaquest-3d-reconstruction_amd"))

import numpy as np  # noqa: E402

HBM_PEAK_GBS = 8000.0


def spread(ms):
    ms = sorted(ms)
    return {"median": ms[len(ms) // 2], "min": ms[0], "max": ms[-1], "repeats": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=960)
    ap.add_argument("--row-stride", type=int, default=1344)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-frames", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "color_frames.json"))
    a = ap.parse_args()
    if a.repeats < 20:
        raise SystemExit("color_frames_probe: at least 20 repetitions")

    from mqr import _lib
    from mqr import colorframes as cf
    from mqr.models import BaseTime, ImageFormatInfo, ImagePlaneInfo
    if _lib.device_count() < 1:
        raise SystemExit("color_frames_probe: no GPU (nothing is written)")
    N, W, H, rs = a.frames, a.width, a.height, a.row_stride
    ysz, csz = rs * (H - 1) + W, rs * (H // 2 - 1) + W - 1
    fmt = ImageFormatInfo(W, H, "YUV_420_888", [ImagePlaneInfo(ysz, rs, 1), ImagePlaneInfo(csz, rs, 2),
                                                ImagePlaneInfo(csz, rs, 2)], BaseTime(0, 0))
    n_bytes = ysz + 2 * csz
    stride = (n_bytes + 3) & ~3
    raw = np.random.default_rng(0).integers(0, 256, (N, stride), dtype=np.uint8)
    frames = [r[:n_bytes] for r in raw]
    src = _lib.DeviceBuffer.from_array(raw)
    dst = _lib.DeviceBuffer(N * H * W * 3)

    def device_ms():
        d, s = ctypes.c_float(), ctypes.c_float()
        _lib.call("mqr_color_frames_last_ms", 0, ctypes.byref(d), ctypes.byref(s))
        return d.value, s.value

    def run(stats, on_device):
        host, dec, st = [], [], []
        for r in range(a.warmup + a.repeats):
            t0 = time.perf_counter()
            if on_device:
                cf.decode_color_frames((src.ptr, N, stride), fmt, stats=stats, out_ptr=dst)
            else:
                cf.decode_color_frames(raw, fmt, stats=stats)
            t = (time.perf_counter() - t0) * 1e3
            if r >= a.warmup:
                d, s = device_ms()
                host.append(t)
                dec.append(d)
                st.append(s)
        return spread(host), spread(dec), spread(st)

    px = W * H
    decode_bytes = 1.5 * px + 3 * px
    stats_bytes = 3 * px + 256 * 4 + 16
    out = {"frames": N, "width": W, "height": H, "row_stride": rs, "frame_bytes": n_bytes, "frame_stride": stride,
           "layout": "NV12, padded rows, short chroma planes; frame bases 4-byte aligned (the wide path)",
           "frame_size_note": "the reference records no frame size; it reads it per capture from the format JSON",
           "what": "device ms: hip events around the kernels on the library's stream; call ms: host clock around "
                   "decode_color_frames (every call drains its stream before returning)",
           "hbm_peak_gbs": HBM_PEAK_GBS,
           "algorithmic_bytes_per_frame": {"decode": decode_bytes, "statistics": stats_bytes}}
    for label, stats in (("decode", False), ("decode_with_statistics", True)):
        call_dev, dec, st = run(stats, True)
        call_host, _, _ = run(stats, False)
        dev_total = dec["median"] + st["median"]
        rec = {"device_ms": {"decode_kernel": dec, "statistics_pass": st},
               "device_ms_per_frame": dev_total / N,
               "call_ms_frames_in_hbm": call_dev, "call_ms_per_frame_in_hbm": call_dev["median"] / N,
               "call_ms_frames_on_host": call_host, "call_ms_per_frame_on_host": call_host["median"] / N,
               "host_staging_ms": call_host["median"] - call_dev["median"],
               "host_staging_ms_per_frame": (call_host["median"] - call_dev["median"]) / N}
        gbs = N * decode_bytes / (dec["median"] * 1e-3) / 1e9
        rec["decode_gbs"] = gbs
        rec["decode_fraction_of_hbm_peak"] = gbs / HBM_PEAK_GBS
        if stats:
            sg = N * stats_bytes / (st["median"] * 1e-3) / 1e9
            rec["statistics_gbs"] = sg
            rec["statistics_fraction_of_hbm_peak"] = sg / HBM_PEAK_GBS
        out[label] = rec
        print(f"color_frames_probe: {label} timed", file=sys.stderr, flush=True)

    # unaligned packed frames (stride = n_bytes + 1): the byte path, for the price of the general case
    odd = np.ascontiguousarray(np.random.default_rng(1).integers(0, 256, (N, n_bytes + 1 + n_bytes % 2), dtype=np.uint8))
    osrc = _lib.DeviceBuffer.from_array(odd)
    dec = []
    for r in range(a.warmup + a.repeats):
        cf.decode_color_frames((osrc.ptr, N, odd.shape[1]), fmt, out_ptr=dst)
        if r >= a.warmup:
            dec.append(device_ms()[0])
    out["decode_unaligned_frames"] = {"frame_stride": int(odd.shape[1]), "decode_kernel_ms": spread(dec),
                                      "device_ms_per_frame": spread(dec)["median"] / N}

    # the host path, for context
    hn = max(1, min(a.host_frames, N))
    t = []
    for r in range(1 + 3):
        t0 = time.perf_counter()
        cf.decode_color_frames(frames[:hn], fmt, stats=True, device=None)
        if r >= 1:
            t.append((time.perf_counter() - t0) * 1e3 / hn)
    out["host_path_ms_per_frame_with_statistics"] = spread(t)
    t = []
    for r in range(1 + 3):
        t0 = time.perf_counter()
        cf.decode_color_frames(frames[:hn], fmt, device=None)
        if r >= 1:
            t.append((time.perf_counter() - t0) * 1e3 / hn)
    out["host_path_ms_per_frame"] = spread(t)

    # the device result is the host path's
    got = cf.decode_color_frames(frames[:hn], fmt, stats=True)
    want = cf.decode_color_frames(frames[:hn], fmt, stats=True, device=None)
    out["device_equals_host_path"] = bool(all(np.array_equal(x, y) for x, y in zip(got, want)))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
