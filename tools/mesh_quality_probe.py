"""The mesh quality metrics on the GPU, timed against the mesh filter on the same mesh.

C5's capture (bench.py's c5_leg, as tools/colormap_profile.py builds it: a LEFT + RIGHT walk through the
8 x 8 x 3 m hall, 3 mm voxels) is fused, its mesh extracted and filtered; the filtered mesh stays in HBM.
After `--warmup` untimed rounds, `--repeats` rounds alternate mqr.evaluation.compute_raw_metrics and
mqr.meshfilter.filter_mesh_components on that mesh, each under the host clock around the call (both
drain their stream before they return).  The filter is the yardstick: it does the same edge sort plus
its compaction passes and a host round trip.  The same is recorded for the mesh of C2's capture
(bench.py's headline: 500 frames of the room walk, 5 mm voxels).

Algorithmic bytes, computed here: 12 nv (1 + has_color) + 12 nt read once, plus the edge sort's payload
of 3 nt * 12 B (u64 key + int32 slot) read and written per radix pass, ceil((32 + bits(nv)) / 8) passes of
8 bits.  Their rate over the measured time is a rate of algorithmic bytes, not of HBM traffic (the corner
sort, the normals and the two passes over run heads are not in the count).  Writes
profiles/mesh_quality.json and prints it.

    python tools/mesh_quality_probe.py [--frames-per-side 2000] [--repeats 20] [--warmup 2]
"""
import argparse
import contextlib
import ctypes
import io
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "metaquest-3d-reconstruction_amd"))

import numpy as np  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec


def spread(ms):
    ms = sorted(ms)
    return {"median": ms[len(ms) // 2], "min": ms[0], "max": ms[-1], "repeats": len(ms)}


def fuse(scene, poses, seed, voxel, block_count, weight_threshold):
    from mqr import synthetic
    from mqr.vbg import VoxelBlockGrid
    H, W = 480, 640
    seq = synthetic.make_sequence_fast(scene, poses=poses, height=H, width=W, seed=seed, device="cuda:0")
    depth = seq["depth_t"].contiguous()
    B = depth.shape[0]
    K, T = seq["K"].astype(np.float64), seq["T_wc"].astype(np.float64)

    class _P:
        ptr = ctypes.c_void_p(depth.data_ptr())

    vbg = VoxelBlockGrid(voxel_size=voxel, block_resolution=16, block_count=block_count, device=0)
    vbg.integrate_frames((_P, B, H, W), K, T, depth_scale=1.0, depth_max=4.0, trunc_voxel_multiplier=10.0)
    mesh = vbg.extract_triangle_mesh(weight_threshold=weight_threshold)
    print(f"mesh_quality_probe: {scene}: {B} frames fused, mesh extracted", file=sys.stderr, flush=True)
    del depth, seq, vbg
    import torch
    torch.cuda.empty_cache()
    return mesh, B


def measure(mesh, repeats, warmup):
    from mqr.evaluation import compute_raw_metrics
    from mqr.meshfilter import filter_mesh_components
    sink = io.StringIO()
    with contextlib.redirect_stdout(sink):
        mesh = filter_mesh_components(mesh)  # the pipeline's order: extract, filter, then score
    nv, nt = len(mesh.vertex.positions), len(mesh.triangle.indices)
    has_color = mesh.vertex.get("colors") is not None
    q_ms, f_ms, first, identical = [], [], None, True
    for r in range(warmup + repeats):
        t0 = time.perf_counter()
        m = compute_raw_metrics(mesh)
        t1 = time.perf_counter()
        with contextlib.redirect_stdout(sink):
            out = filter_mesh_components(mesh)
        t2 = time.perf_counter()
        del out
        first = first or m
        identical = identical and m == first
        if r >= warmup:
            q_ms.append((t1 - t0) * 1e3)
            f_ms.append((t2 - t1) * 1e3)
    print(f"mesh_quality_probe: {nt} triangles timed", file=sys.stderr, flush=True)
    passes = -(-(32 + int(nv).bit_length()) // 8)
    read = 12 * nv * (1 + int(has_color)) + 12 * nt
    sort = 2 * 3 * nt * 12 * passes
    q = spread(q_ms)
    gbs = (read + sort) / (q["median"] * 1e-3) / 1e9
    from dataclasses import asdict
    return {
        "vertices": nv, "triangles": nt, "has_color": has_color,
        "quality_ms": q, "filter_ms": spread(f_ms), "quality_over_filter": q["median"] / spread(f_ms)["median"],
        "what": "host clock around each call, alternating in one run; both calls drain their stream before returning",
        "algorithmic_bytes": {"mesh_read": read, "sort_payload_per_pass": 3 * nt * 12, "radix_passes": passes,
                              "sort_read_plus_write": sort, "total": read + sort},
        "algorithmic_gb_per_s": gbs, "fraction_of_hbm_peak": gbs / HBM_PEAK_GBS,
        "ns_per_triangle": q["median"] * 1e6 / nt,
        "repeat_bit_identical": bool(identical),
        "metrics": {k: v for k, v in asdict(first).items() if k not in ("name", "path")},
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames-per-side", type=int, default=2000)
    ap.add_argument("--c2-frames", type=int, default=500)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_quality.json"))
    a = ap.parse_args()
    if a.repeats < 20:
        raise SystemExit("mesh_quality_probe: at least 20 repetitions")

    from mqr import _lib, synthetic
    if _lib.device_count() < 1:
        raise SystemExit("mesh_quality_probe: no GPU (there is no CPU fallback; nothing is written)")
    out = {"hbm_peak_gb_per_s": HBM_PEAK_GBS}
    left = synthetic.hall_loop_poses(a.frames_per_side)
    poses = left + [(R_, t_ + R_[:, 0] * 0.064) for R_, t_ in left]
    mesh, B = fuse("hall", poses, 5, 0.003, 16384, 1.5)
    out["c5"] = {"capture": {"scene": "hall", "frames": B, "voxel_size": 0.003}, **measure(mesh, a.repeats, a.warmup)}
    del mesh
    mesh, B = fuse("room", synthetic.room_loop_poses(a.c2_frames), 0, 0.005, 40000, 3.0)
    out["c2"] = {"capture": {"scene": "room", "frames": B, "voxel_size": 0.005}, **measure(mesh, a.repeats, a.warmup)}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
