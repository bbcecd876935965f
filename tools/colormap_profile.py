"""The rigid colour-map optimisation of C5, timed on the GPU.

C5's capture (bench.py's c5_leg: a LEFT + RIGHT walk through the 8 x 8 x 3 m hall, 3 mm voxels) is fused
and its mesh extracted; every (frames / keyframes)-th frame is a 640 x 480 colour keyframe with ray-cast
colour-aligned depth, its pose moved by a seeded few millimetres / milliradians.  The mesh, the depth
and the images stay in HBM.  One timed run is mqr.color.ColorMapOptimizer.optimize(iters) from those
poses: the device time between two events on the optimiser's stream around the loop's launches (three
per iteration, no host read in between), and the host clock around the whole call (which adds the
per-iteration records' and the poses' way back).  `--warmup` untimed runs, then `--repeats` timed ones,
each from the same start; median and spread are recorded.

Bytes under the stated count, per visibility pair and iteration: the pair's vertex index (4) and position
(12), its proxy intensity (8) and four 16-byte taps of the interleaved (gray, dx, dy) image (64) in the
systems kernel, plus index (4), one 16-byte nearest tap and the position's share in the proxy kernel.
The gather rate is the taps' bytes (64 per pair) over the device time per iteration -- a rate of
algorithmic bytes, not of HBM traffic.  Writes profiles/colormap_optimize.json and prints it.

    python tools/colormap_profile.py [--frames-per-side 2000] [--keyframes 100] [--iters 100] [--repeats 5]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "metaquest-3d-reconstruction_amd"))

import numpy as np  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec


def small_motion(rng, scale):
    w, t = rng.uniform(-scale, scale, 3), rng.uniform(-scale, scale, 3)
    th = np.linalg.norm(w)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    D = np.eye(4)
    D[:3, :3] = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
    D[:3, 3] = t
    return D


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames-per-side", type=int, default=2000)
    ap.add_argument("--keyframes", type=int, default=100)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--voxel", type=float, default=0.003)
    ap.add_argument("--perturb", type=float, default=0.003)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "colormap_optimize.json"))
    a = ap.parse_args()

    from mqr import _lib, synthetic
    from mqr.color import ColorMapOptimizer, RigidOptimizerOption, colormap_build_tag
    from mqr.raycasting import RaycastingScene
    from mqr.vbg import VoxelBlockGrid
    if _lib.device_count() < 1:
        raise SystemExit("colormap_profile: no GPU (there is no CPU fallback; nothing is written)")
    import ctypes
    H, W = 480, 640
    left = synthetic.hall_loop_poses(a.frames_per_side)
    poses = left + [(R_, t_ + R_[:, 0] * 0.064) for R_, t_ in left]
    seq = synthetic.make_sequence_fast("hall", poses=poses, height=H, width=W, seed=5, device="cuda:0")
    depth = seq["depth_t"].contiguous()
    B = depth.shape[0]
    K, T = seq["K"].astype(np.float64), seq["T_wc"].astype(np.float64)

    class _P:
        ptr = ctypes.c_void_p(depth.data_ptr())

    vbg = VoxelBlockGrid(voxel_size=a.voxel, block_resolution=16, block_count=16384, device=0)
    vbg.integrate_frames((_P, B, H, W), K, T, depth_scale=1.0, depth_max=4.0, trunc_voxel_multiplier=10.0)
    mesh = vbg.extract_triangle_mesh(weight_threshold=1.5)
    nv, nt = len(mesh.vertex.positions), len(mesh.triangle.indices)
    key = [int(i) for i in np.linspace(0, B, a.keyframes, endpoint=False)]
    imgs = synthetic.render_color_torch("hall", K[0], [poses[i] for i in key], H, W, device="cuda:0").cpu().numpy()
    del depth, seq
    import torch
    torch.cuda.empty_cache()
    scene = RaycastingScene(device=0)
    scene.add_triangles(mesh)
    Kk, Tk = np.ascontiguousarray(K[key]), np.ascontiguousarray(T[key])
    t_hit = scene.cast_pinhole(Kk, Tk, W, H)["t_hit"]
    rng = np.random.default_rng(7)
    T0 = np.stack([small_motion(rng, a.perturb) @ t for t in Tk])

    t0 = time.perf_counter()
    opt = ColorMapOptimizer(mesh.vertex.positions, imgs, t_hit, Kk, T0, RigidOptimizerOption())
    create_s = time.perf_counter() - t0
    pairs = opt.pairs_per_keyframe
    dev_ms, host_ms, res0, cnt0, poses0 = [], [], None, None, None
    identical = True
    for r in range(a.warmup + a.repeats):
        opt.poses = T0
        t0 = time.perf_counter()
        res, cnt = opt.optimize(a.iters)
        dt = (time.perf_counter() - t0) * 1e3
        if res0 is None:
            res0, cnt0, poses0 = res, cnt, opt.poses
        identical = identical and np.array_equal(res, res0) and np.array_equal(cnt, cnt0) and np.array_equal(opt.poses, poses0)
        if r >= a.warmup:
            host_ms.append(dt)
            dev_ms.append(opt.last_optimize_ms)
    t0 = time.perf_counter()
    opt.colors()
    colors_s = time.perf_counter() - t0
    opt.close()
    dev_ms.sort()
    host_ms.sort()
    med = dev_ms[len(dev_ms) // 2]
    per_iter = med / a.iters
    terms = float(np.mean(cnt0))
    P = int(pairs.sum())
    out = {
        "source_tag": colormap_build_tag(),
        "capture": {"scene": "hall", "frames": B, "height": H, "width": W, "voxel_size": a.voxel,
                    "keyframes": len(key), "perturbation": a.perturb},
        "mesh": {"vertices": nv, "triangles": nt},
        "visibility_pairs": {"total": P, "per_keyframe_min": int(pairs.min()), "per_keyframe_median": int(np.median(pairs)),
                             "per_keyframe_max": int(pairs.max()), "chunks_of_256": int(((pairs + 255) // 256).sum())},
        "iterations": a.iters,
        "terms_per_iteration": terms,
        "residual": {"first": float(res0[0]), "last": float(res0[-1])},
        "device_ms_per_run": {"median": med, "min": dev_ms[0], "max": dev_ms[-1], "repeats": a.repeats, "warmup": a.warmup,
                              "what": "events on the optimiser's stream around the loop's launches of one optimize(iters)"},
        "host_ms_per_run": {"median": host_ms[len(host_ms) // 2], "min": host_ms[0], "max": host_ms[-1],
                            "what": "host clock around the same call (adds the records' and poses' copies and the final synchronise)"},
        "ms_per_iteration": per_iter,
        "pairs_per_iteration": P,
        "gather": {"bytes_per_pair": 64, "gb_per_s": 64.0 * P / (per_iter * 1e-3) / 1e9,
                   "count": "four 16-byte (gray, dx, dy, pad) taps per visibility pair in the systems kernel"},
        "algorithmic_bytes_per_pair": {"systems": 4 + 12 + 8 + 64, "proxy": 4 + 16},
        "algorithmic_gb_per_s": (88.0 + 20.0) * P / (per_iter * 1e-3) / 1e9,
        "fraction_of_hbm_peak": (88.0 + 20.0) * P / (per_iter * 1e-3) / 1e9 / HBM_PEAK_GBS,
        "hbm_peak_gb_per_s": HBM_PEAK_GBS,
        "launches_per_iteration": 3,
        "create_s": create_s,
        "colors_s": colors_s,
        "repeat_bit_identical": bool(identical),
    }
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
