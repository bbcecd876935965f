"""Colour-aligned depth from the TSDF volume itself (csrc/volumecast.hip, VoxelBlockGrid.ray_cast_frames) beside
the mesh path it can stand in for (extract at 1.5, filter components, BVH build, cast_pinhole), on C2's volume
(500 frames of the room walk, 5 mm voxels) and, with --c5, on C5's (a LEFT + RIGHT walk through the hall, 3 mm
voxels).  The captures are tools/mesh_quality_probe.py's.  Per volume and per view size (1280 x 960, 640 x 480),
`--views` colour views spread over the walk, cast 16 at a time as raycast_in_color_view does, at the pixel
centres, metric depth:

  volume.range_ms / march_ms   device time per frame of the two kernels (events on the volume's stream,
                               mqr_vbg_ray_cast_last_ms), with and without refine;
  volume.wall_ms_per_frame     the host clock around the same calls (results left in HBM);
  mesh.setup_ms                extract, filter and BVH build once each (host clock; each call drains its stream);
  mesh.cast_ms_per_frame       cast_pinhole alone; mesh.total_ms_per_frame adds the setup spread over the views.

The two paths alternate in one process, `--repeats` times after one untimed round; medians are recorded.
`difference` compares the two depth maps over the first `--diff-views` views: over pixels both hit, the median,
p99 and max of |volume - mesh|; the pixels only one of them hit (a mesh hit beyond the volume cast's depth_max
counts as a miss); with and without refine.  The volume path skips
the component filter, so fragments the filter removes stay visible to it.  No figure here is a pass / fail
condition.  Writes profiles/volume_cast.json and prints it.

    python tools/volume_cast_probe.py [--c5] [--views 100] [--repeats 5]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

BATCH = 16
SIZES = ((1280, 960, 1050.0), (640, 480, 525.0))


def median(x):
    return float(np.median(x))


def fuse(scene, poses, seed, voxel, block_count):
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
    from mqr import _lib
    _lib.call("mqr_device_synchronize", 0)
    del depth
    import torch
    torch.cuda.empty_cache()
    print(f"volume_cast_probe: {scene}: {B} frames fused, {vbg.size()} blocks", file=sys.stderr, flush=True)
    return vbg, B, T


def measure(vbg, T_all, a, label):
    from mqr import _lib
    from mqr.meshfilter import filter_mesh_components
    from mqr.raycasting import RaycastingScene
    pick = np.linspace(0, len(T_all) - 1, a.views).round().astype(int)
    T = np.ascontiguousarray(T_all[pick], np.float64)
    cast_kw = dict(depth_scale=1.0, depth_max=4.0, weight_threshold=3.0, trunc_voxel_multiplier=10.0, pixel_offset=0.5)
    sync = lambda: _lib.call("mqr_device_synchronize", 0)  # noqa: E731

    def mesh_setup():
        t = [time.perf_counter()]
        mesh = vbg.extract_triangle_mesh(weight_threshold=1.5)
        t.append(time.perf_counter())
        with contextlib.redirect_stdout(io.StringIO()):
            mesh = filter_mesh_components(mesh)
        t.append(time.perf_counter())
        scene = RaycastingScene(device=0)
        scene.add_triangles(mesh)
        _lib.call("mqr_scene_build", scene._h)
        sync()
        t.append(time.perf_counter())
        return scene, mesh, [1e3 * (y - x) for x, y in zip(t, t[1:])]

    out = {"blocks": vbg.size(), "views": int(a.views), "batch": BATCH, "repeats": a.repeats, "sizes": {}}
    for W, H, f in SIZES:
        K = np.tile(np.array([[f, 0, W / 2.0], [0, f, H / 2.0], [0, 0, 1.0]]), (a.views, 1, 1))
        rec = {"volume": {}, "mesh": {}}
        vol = {r: {"range": [], "march": [], "wall": []} for r in (False, True)}
        setup, cast = [], []
        triangles = 0
        for rep in range(1 + a.repeats):
            for refine in (False, True):
                rng_ms = mar_ms = 0.0
                t0 = time.perf_counter()
                for i in range(0, a.views, BATCH):
                    vbg.ray_cast_frames(K[i:i + BATCH], T[i:i + BATCH], W, H, refine=refine, **cast_kw)
                    r, m = vbg.ray_cast_last_ms()
                    rng_ms += r
                    mar_ms += m
                wall = 1e3 * (time.perf_counter() - t0)
                if rep:
                    vol[refine]["range"].append(rng_ms / a.views)
                    vol[refine]["march"].append(mar_ms / a.views)
                    vol[refine]["wall"].append(wall / a.views)
            scene, mesh, st = mesh_setup()
            triangles = len(mesh.triangle.indices)
            t0 = time.perf_counter()
            for i in range(0, a.views, BATCH):
                scene.cast_pinhole(K[i:i + BATCH], T[i:i + BATCH], W, H)
            sync()
            c = 1e3 * (time.perf_counter() - t0)
            if rep:
                setup.append(st)
                cast.append(c / a.views)
            del scene, mesh
        for refine in (False, True):
            rec["volume"]["refine" if refine else "plain"] = {
                "range_ms_per_frame": median(vol[refine]["range"]), "march_ms_per_frame": median(vol[refine]["march"]),
                "wall_ms_per_frame": median(vol[refine]["wall"])}
        setup = np.array(setup)
        rec["mesh"] = {"triangles_after_filter": int(triangles),
                       "setup_ms": {"extract": median(setup[:, 0]), "filter": median(setup[:, 1]),
                                    "bvh_build": median(setup[:, 2])},
                       "cast_ms_per_frame": median(cast),
                       "total_ms_per_frame": median(cast) + float(np.median(setup.sum(axis=1))) / a.views}
        # ---- how the two depth maps differ
        scene, mesh, _ = mesh_setup()
        n = min(a.diff_views, a.views)
        t_hit = scene.cast_pinhole(K[:n], T[:n], W, H)["t_hit"].numpy()
        hm = t_hit < cast_kw["depth_max"]  # (the volume cast stops at depth_max: farther mesh hits count as misses)
        rec["difference"] = {"views": int(n), "pixels": int(hm.size)}
        for refine in (False, True):
            d = vbg.ray_cast_frames(K[:n], T[:n], W, H, refine=refine, **cast_kw)["depth"].numpy()
            hv = d > 0
            both = hv & hm
            e = np.abs(d[both] - t_hit[both])
            rec["difference"]["refine" if refine else "plain"] = {
                "both_hit": int(both.sum()), "volume_only": int((hv & ~hm).sum()), "mesh_only": int((hm & ~hv).sum()),
                "median_abs_m": float(np.median(e)), "p99_abs_m": float(np.percentile(e, 99)), "max_abs_m": float(e.max())}
            del d
        del scene, mesh, t_hit
        out["sizes"][f"{W}x{H}"] = rec
        print(f"volume_cast_probe: {label}: {W} x {H} measured", file=sys.stderr, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--c5", action="store_true", help="also measure C5's volume (minutes of fusing)")
    ap.add_argument("--frames-per-side", type=int, default=2000)
    ap.add_argument("--c2-frames", type=int, default=500)
    ap.add_argument("--views", type=int, default=100)
    ap.add_argument("--diff-views", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "volume_cast.json"))
    a = ap.parse_args()

    from mqr import _lib, synthetic
    if _lib.device_count() < 1:
        raise SystemExit("volume_cast_probe: no GPU (there is no CPU fallback; nothing is written)")
    out = {"arguments": {k: v for k, v in vars(a).items() if k != "out"},
           "what": "HIP events on the volume's stream (range_ms, march_ms) and the host clock (wall, mesh path); "
                   "medians over `repeats` alternating rounds after one untimed round"}

    def save():
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)

    vbg, B, T = fuse("room", synthetic.room_loop_poses(a.c2_frames), 0, 0.005, 40000)
    out["c2"] = {"capture": {"scene": "room", "frames": B, "voxel_size": 0.005}, **measure(vbg, T, a, "c2")}
    del vbg
    save()
    if a.c5:
        left = synthetic.hall_loop_poses(a.frames_per_side)
        poses = left + [(R_, t_ + R_[:, 0] * 0.064) for R_, t_ in left]
        vbg, B, T = fuse("hall", poses, 5, 0.003, 16384)
        out["c5"] = {"capture": {"scene": "hall", "frames": B, "voxel_size": 0.003}, **measure(vbg, T, a, "c5")}
        del vbg
        save()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
