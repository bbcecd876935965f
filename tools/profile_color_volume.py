"""What the coloured volume costs, on C2's frames: 500 VGA depth frames of the room walk at
5 mm voxels, with a 1280 x 960 colour stack of the same poses in HBM.  A coloured and a colourless
VoxelBlockGrid take the same depth frames alternately in one process, one untimed round first; medians over
`--repeats` rounds are recorded:

  integrate.pass_ms              events on the caller stream around ``integrate_frames`` (device frames: the call
                                 makes that stream wait for its last integrate), coloured and colourless
  integrate.integrate_kernels_ms the library's own events around each batch's integrate launches (mqr_vbg_stats);
                                 the colour pass runs inside them, so coloured - colourless is the colour kernel
  integrate.color_kernel_bytes   the stated byte count: per (block, frame) pair R^3 x (4 B depth + 3 B colour
                                 pixel), per block and batch R^3 x (8 B (tsdf, weight) read + 12 B colours read
                                 + 12 B colours written) -- every voxel counted as accepted and coloured
  extraction                     extract_triangle_mesh / extract_point_cloud at 3.0, host clock (the calls drain
                                 their stream), with and without colours
  ray_cast                       one batch of 1280 x 960 views, the march's device time per frame
                                 (mqr_vbg_ray_cast_last_ms) with ("depth",) and with ("depth", "color")

`--bench-this` / `--bench-parent` name files holding bench.py's JSON result line of this commit and of its
parent on the same box; both are copied into the record with their ms_per_step ratio.  No figure here is a
pass / fail condition.  Writes profiles/color_volume.json and prints it.

    python tools/profile_color_volume.py [--frames 500] [--repeats 5]
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

H, W, HC, WC = 480, 640, 960, 1280
KW = dict(depth_scale=1.0, depth_max=4.0, trunc_voxel_multiplier=10.0)


def median(x):
    return float(np.median(x))


def last_json_line(path):
    with open(path) as f:
        lines = [ln for ln in f.read().splitlines() if ln.strip().startswith("{")]
    return json.loads(lines[-1])


class _Ptr:
    def __init__(self, t):
        self.keep = t
        self.ptr = ctypes.c_void_p(t.data_ptr())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=500)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--views", type=int, default=16)
    ap.add_argument("--bench-this", default=None)
    ap.add_argument("--bench-parent", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "color_volume.json"))
    a = ap.parse_args()

    import torch
    from mqr import _lib, synthetic
    from mqr.vbg import VoxelBlockGrid
    if _lib.device_count() < 1:
        raise SystemExit("profile_color_volume: no GPU (there is no CPU fallback; nothing is written)")
    poses = synthetic.room_loop_poses(a.frames)
    seq = synthetic.make_sequence_fast("room", poses=poses, height=H, width=W, seed=0, device="cuda:0")
    depth = seq["depth_t"].contiguous()
    B = depth.shape[0]
    K, T = seq["K"].astype(np.float64), seq["T_wc"].astype(np.float64)
    Kc1 = K[0].copy()
    Kc1[:2] *= WC / W  # the same field of view at twice the size
    Kc1[0, 2], Kc1[1, 2] = K[0][0, 2] * WC / W + 0.5, K[0][1, 2] * HC / H + 0.5
    color = torch.empty((B, HC, WC, 3), dtype=torch.uint8, device="cuda:0")
    for i in range(0, B, 50):  # (the float64 renderer's temporaries: 50 frames at a time)
        color[i:i + 50] = synthetic.render_color_torch("room", Kc1, poses[i:i + 50], HC, WC, device="cuda:0")
    Kc = np.tile(Kc1, (B, 1, 1))
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    print(f"profile_color_volume: {B} depth frames {W}x{H}, colour stack {WC}x{HC} "
          f"({color.numel() / 2**30:.2f} GiB) in HBM", file=sys.stderr, flush=True)

    grids = {"colored": VoxelBlockGrid(attr_names=("tsdf", "weight", "color"), voxel_size=0.005, block_resolution=16,
                                       block_count=40000, device=0),
             "colorless": VoxelBlockGrid(voxel_size=0.005, block_resolution=16, block_count=40000, device=0)}
    for g in grids.values():
        g.profile(True)
    dptr, cptr = _Ptr(depth), _Ptr(color)
    rec = {k: {"pass": [], "kernels": []} for k in grids}
    stats = {}
    for rep in range(1 + a.repeats):
        for name, g in grids.items():
            g.reset()
            _lib.call("mqr_device_synchronize", 0)
            g.stats(reset=True)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            if name == "colored":
                g.integrate_frames((dptr, B, H, W), K, T, colors=(cptr, B, HC, WC), color_intrinsics=Kc, **KW)
            else:
                g.integrate_frames((dptr, B, H, W), K, T, **KW)
            e1.record()
            torch.cuda.synchronize()
            s = g.stats(reset=True)
            if rep:
                rec[name]["pass"].append(e0.elapsed_time(e1))
                rec[name]["kernels"].append(s["integrate_ms"])
            stats[name] = s
    out = {"arguments": {k: v for k, v in vars(a).items() if k not in ("out", "bench_this", "bench_parent")},
           "what": "C2's frames with a 1280x960 colour stack in HBM; events, one untimed round, medians over "
                   "`repeats` rounds alternating the coloured and the colourless volume in one process",
           "capture": {"scene": "room", "frames": int(B), "depth": [W, H], "color": [WC, HC], "voxel_size": 0.005,
                       "blocks": grids["colored"].size()}}
    pc, pp = median(rec["colored"]["pass"]), median(rec["colorless"]["pass"])
    kc, kp = median(rec["colored"]["kernels"]), median(rec["colorless"]["kernels"])
    s = stats["colored"]
    R3 = 16 ** 3
    nbytes = int(s["frame_blocks"]) * R3 * 7 + int(s["union_blocks"]) * R3 * 32
    out["integrate"] = {
        "pass_ms": {"colored": pc, "colorless": pp, "colored_over_colorless": pc / pp},
        "integrate_kernels_ms": {"colored": kc, "colorless": kp},
        "color_kernel_ms": kc - kp, "color_kernel_share_of_colored_pass": (kc - kp) / pc,
        "block_frame_pairs": int(s["frame_blocks"]), "block_batches": int(s["union_blocks"]),
        "color_kernel_bytes": nbytes, "color_kernel_bytes_per_s": nbytes / ((kc - kp) * 1e-3) if kc > kp else None,
        "samples": rec}
    print("profile_color_volume: integrate measured", file=sys.stderr, flush=True)

    def save():
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)

    save()
    ex = {}
    for what in ("extract_triangle_mesh", "extract_point_cloud"):
        ex[what] = {}
        for name, g in grids.items():
            t = []
            n = 0
            for rep in range(1 + a.repeats):
                t0 = time.perf_counter()
                geom = getattr(g, what)(weight_threshold=3.0)
                dt = 1e3 * (time.perf_counter() - t0)
                n = int(geom.vertex.positions.shape[0] if what.endswith("mesh") else geom.point.positions.shape[0])
                del geom
                if rep:
                    t.append(dt)
            ex[what][name] = {"ms": median(t), "vertices": n}
        ex[what]["colored_over_colorless"] = ex[what]["colored"]["ms"] / ex[what]["colorless"]["ms"]
    out["extraction"] = ex
    save()

    pick = np.linspace(0, B - 1, a.views).round().astype(int)
    g = grids["colored"]
    rc = {}
    cast_kw = dict(depth_scale=1.0, depth_max=4.0, weight_threshold=3.0, trunc_voxel_multiplier=10.0)
    for label, attrs in (("depth", ("depth",)), ("depth_color", ("depth", "color"))):
        m = []
        for rep in range(1 + a.repeats):
            g.ray_cast_frames(Kc[pick], T[pick], WC, HC, render_attributes=attrs, **cast_kw)
            if rep:
                m.append(g.ray_cast_last_ms()[1] / a.views)
        rc[label] = {"march_ms_per_frame": median(m)}
    rc["color_over_depth"] = rc["depth_color"]["march_ms_per_frame"] / rc["depth"]["march_ms_per_frame"]
    out["ray_cast"] = {"size": [WC, HC], "views": int(a.views), **rc}

    if a.bench_this and a.bench_parent:
        this, parent = last_json_line(a.bench_this), last_json_line(a.bench_parent)
        out["bench"] = {"this_commit": this, "parent_commit": parent,
                        "ms_per_step_ratio": this["ms_per_step"] / parent["ms_per_step"]}
    save()
    print(json.dumps({k: v for k, v in out.items() if k != "bench"}, indent=1))


if __name__ == "__main__":
    main()
