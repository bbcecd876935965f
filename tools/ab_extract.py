#!/usr/bin/env python3
"""Timing probe of extract_triangle_mesh on the bench volume (C2, one process).

python tools/ab_extract.py --reps 15 [--block-resolution 12]
Prints one JSON line: the median (and every) wall ms of mqr_extract_mesh (device-resident, the
bench's extract_ms), the counts and an order-independent hash of the mesh.  --block-resolution
other than 8 / 16 times the generic byte-tile path.  To compare two builds of the library, run it in
alternating processes with MQR_HIP_LIB naming each (as tools/raycast_workload.py) and compare the
medians and the hashes.

What was compared this way and decided, the verdicts beside the code in extract.hip and in DESIGN
§4.2: the per-cube triangle counts from the count pass, the LDS row maps of the emission pass and the
scan's totals written straight into pinned host memory (round 5,
profiles/r05_ab_extract_direct_totals.json) all won and are the code.  Round 4 also measured, and
removed: an emission over a compacted list of the blocks with output, the block's tsdf staged in LDS
for the interior vertex taps, XCD bands of the pool (profiles/r04_ab_extract.json), the count pass
emitting the vertices (0.264 vs 0.237 ms) and a vertex and a triangle workgroup per block (0.187 vs
0.179 ms); round 3 measured a merged vertex / triangle item loop and 512-thread emission blocks: no
change (profiles/r03_ab_integrate_windows.json).
"""
import argparse
import ctypes
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "metaquest-3d-reconstruction_amd"))
sys.path.insert(0, ROOT)


def mesh_digest(p, n, t):
    """sha1 of the mesh as a set: the vertex records (position, normal) and the triangles' corner
    positions, each sorted by bit pattern.  The pool's block order, and with it the order of the
    output, differs from process to process; the set does not."""
    import numpy as np
    h = hashlib.sha1()
    for rows in (np.hstack([p, n]), p[t].reshape(len(t), 9)):
        u = np.ascontiguousarray(rows).view(np.uint32)
        h.update(u[np.lexsort(u.T[::-1])].tobytes())
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--threshold", type=float, default=1.5)
    ap.add_argument("--block-resolution", type=int, default=16)
    a = ap.parse_args()
    import numpy as np
    import torch
    from bench import _DevPtr
    from mqr import _lib, synthetic
    from mqr.vbg import VoxelBlockGrid
    seq = synthetic.make_sequence_fast("room", poses=synthetic.room_loop_poses(500), device="cuda:0")
    d = seq["depth_t"].contiguous()
    B, H, W = d.shape
    R = a.block_resolution
    # the same voxels at any R: the block capacity scales with the inverse block volume
    vbg = VoxelBlockGrid(voxel_size=0.005, block_resolution=R, block_count=int(40000 * max(1.0, (16 / R) ** 3)),
                         device=0)
    vbg.integrate_frames((_DevPtr(d.data_ptr()), B, H, W), seq["K"].astype(np.float64),
                         seq["T_wc"].astype(np.float64), depth_scale=1.0, depth_max=4.0, trunc_voxel_multiplier=10.0)
    torch.cuda.synchronize()
    times = []
    for r in range(a.reps + 1):  # the first extraction (no capacity hint yet) is not timed
        g = ctypes.c_void_p()
        t0 = time.perf_counter()
        _lib.call("mqr_extract_mesh", vbg.handle, float(a.threshold), ctypes.byref(g))
        dt = (time.perf_counter() - t0) * 1e3
        if r > 0:
            times.append(dt)
        if r == a.reps:
            nv, nt = ctypes.c_int64(), ctypes.c_int64()
            _lib.call("mqr_geom_counts", g, ctypes.byref(nv), ctypes.byref(nt))
            p = np.empty((nv.value, 3), np.float32)
            n = np.empty((nv.value, 3), np.float32)
            t = np.empty((nt.value, 3), np.int32)
            _lib.call("mqr_geom_copy", g, p.ctypes.data_as(ctypes.c_void_p), n.ctypes.data_as(ctypes.c_void_p),
                      t.ctypes.data_as(ctypes.c_void_p), 0)
        _lib.call("mqr_geom_free", g)
    print(json.dumps({"lib": _lib.LIB_PATH, "block_resolution": R, "ms": float(np.median(times)),
                      "ms_all": [round(x, 4) for x in times], "vertices": int(len(p)), "triangles": int(len(t)),
                      "sha1": mesh_digest(p, n, t), "blocks": vbg.size(), "threshold": a.threshold}))


if __name__ == "__main__":
    main()
