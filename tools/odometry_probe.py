"""The odometry information batch of one synthetic 100-frame VGA fragment, timed on the GPU.

The pair list is the reference's upper bound for a fragment (make_fragments.py:106-240 with fragment size
100 and odometry_loop_interval 10): 99 odometry pairs (i, i + 1) and all 45 pairs of the 10 key frames,
144 in all, at the capture's true relative poses.  The frames are decoded once and left in HBM; each
timed call is one mqr.odometry.odometry_information_pairs on them (pair upload, ONE launch of the pair
kernel, the per-pair finalize, the 6x6 results back) and ends behind a device synchronise, so the time
is a whole call's, not the kernel's alone.  Three warm-up calls, then `--repeats` timed ones.

Bytes under the stated count: every pair reads its source frame once (4 B per pixel, a coalesced
stream) and at most one 4-byte target depth per source pixel (the gather); slabs and results are
small beside that.  The fraction of HBM peak is those bytes over the median call time over 8000 GB/s;
most of a fragment's frames are re-read from cache by later pairs, so it is a rate of algorithmic
bytes, not of HBM traffic.  Writes profiles/odometry_pairs.json and prints it.

    python tools/odometry_probe.py [--frames 100] [--interval 10] [--repeats 200]
"""
import argparse
import itertools
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "metaquest-3d-reconstruction_amd"))

import numpy as np  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--interval", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "odometry_pairs.json"))
    a = ap.parse_args()

    from mqr import _lib, synthetic
    from mqr.odometry import odometry_information_pairs
    if _lib.device_count() < 1:
        raise SystemExit("odometry_probe: no GPU (there is no CPU fallback; nothing is written)")
    H, W = 480, 640
    seq = synthetic.make_sequence_fast("room", poses=synthetic.room_loop_poses(5 * a.frames)[:a.frames], height=H,
                                       width=W, device="cuda:0")
    depth = seq["depth_t"].cpu().numpy()
    N = depth.shape[0]
    keys = list(range(0, N, a.interval))
    pairs = [(i, i + 1) for i in range(N - 1)] + list(itertools.combinations(keys, 2))
    src = np.array([p[0] for p in pairs], np.int32)
    tgt = np.array([p[1] for p in pairs], np.int32)
    Twc, Tcw = seq["T_wc"].astype(np.float64), seq["T_cw"].astype(np.float64)
    T = np.stack([Twc[b] @ Tcw[i] for i, b in pairs])
    K = seq["K"][0].astype(np.float64)
    buf = _lib.DeviceBuffer.from_array(depth)
    frames = (buf, N, H, W)

    def call():
        t0 = time.perf_counter()
        info, counts = odometry_information_pairs(frames, K, src, tgt, T, 0.07, 1.0, 3.0)
        return time.perf_counter() - t0, info, counts
    for _ in range(3):
        _, info0, counts0 = call()
    times = []
    identical = True
    for _ in range(a.repeats):
        dt, info, counts = call()
        identical = identical and np.array_equal(info, info0) and np.array_equal(counts, counts0)
        times.append(dt * 1e3)
    buf.free()
    times.sort()
    med = times[len(times) // 2]
    nbytes = len(pairs) * H * W * 4 * 2
    out = {
        "capture": {"scene": "room", "frames": N, "height": H, "width": W, "key_frame_interval": a.interval},
        "pairs": {"total": len(pairs), "odometry": N - 1, "key_frame": len(pairs) - (N - 1)},
        "accepted_pixels": {"min": int(counts0.min()), "median": int(np.median(counts0)), "max": int(counts0.max())},
        "ms_per_call": {"median": med, "min": times[0], "max": times[-1], "repeats": a.repeats, "warmup": 3,
                        "what": "host clock around one odometry_information_pairs call on device frames: pair upload, "
                                "one pair-kernel launch, finalize, results to the host, synchronise"},
        "bytes": {"total": nbytes,
                  "count": "per pair: the source frame once (4 B per pixel) + at most one 4-byte gathered target "
                           "depth per source pixel"},
        "algorithmic_gb_per_s": nbytes / (med * 1e-3) / 1e9,
        "fraction_of_hbm_peak": nbytes / (med * 1e-3) / 1e9 / HBM_PEAK_GBS,
        "hbm_peak_gb_per_s": HBM_PEAK_GBS,
        "repeat_bit_identical": bool(identical),
    }
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
