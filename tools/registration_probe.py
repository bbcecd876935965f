"""Pose-graph edges of a synthetic room capture's fragments, timed three ways:

  (a) batched   mqr.fragments.build_pose_graph_for_scene: three batched calls on one CloudSet
  (b) single    the same pairs one at a time through the single-pair functions (compute_pcd_pair_edge)
  (c) cpu       the CPU restatement of the same rules (tests/registration_ref.py), one process

The fragments come from integrate_fragment_point_clouds with the clouds left in HBM; (a) and (b) read
them in place, (c) gets host copies (not timed).  Each timed call ends in the host reading its
results, i.e. behind a device synchronise.  (a) and (b) are warmed once, then run alternately
`--repeats` times; (c) runs once.  Writes profiles/registration_pairs.json and prints it.

    python tools/registration_probe.py [--frames 500] [--fragment 100] [--repeats 5] [--skip-cpu]
"""
import argparse
import contextlib
import io as _io
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "metaquest-3d-reconstruction_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=500)
    ap.add_argument("--fragment", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--skip-cpu", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "registration_pairs.json"))
    a = ap.parse_args()

    import registration_ref as ref
    from mqr import synthetic
    from mqr.dataio import DepthDataIO
    from mqr.fragments import (FragmentPoseRefinementConfig, build_pose_graph_for_scene, fragment_datasets,
                               integrate_fragment_point_clouds)
    from mqr.models import CoordinateSystem, Side
    from mqr.registration import CloudSet

    seq = synthetic.make_sequence_fast("room", poses=synthetic.room_loop_poses(a.frames), device="cuda:0")
    cap = {"raw": seq["raw_t"].cpu().numpy(), "unity": seq["unity"], "tangents": seq["tangents"], "near": seq["near"],
           "far": seq["far"], "width": seq["width"], "height": seq["height"]}
    tmp = tempfile.mkdtemp()
    try:
        synthetic.write_capture(tmp, cap)
        dio = DepthDataIO(tmp)
        ds = dio.load_depth_dataset(Side.LEFT)
        ds.transforms = ds.transforms.convert_coordinate_system(target_coordinate_system=CoordinateSystem.OPEN3D,
                                                                is_camera=True)
        frags = fragment_datasets(ds, a.fragment)
        cfg = FragmentPoseRefinementConfig(device="CUDA:0", use_confidence_filtered_depth=False, voxel_size=0.01,
                                           block_count=50_000, depth_max=4.0, trunc_voxel_multiplier=8.0)
        res = integrate_fragment_point_clouds(dio, {Side.LEFT: frags}, cfg, keep_on_device=True)
    finally:
        shutil.rmtree(tmp)
    clouds = {Side.LEFT: [r[1] for r in res if r is not None]}
    n_clouds = len(clouds[Side.LEFT])

    def run(batched, stats=None):
        with contextlib.redirect_stdout(_io.StringIO()):
            t0 = time.perf_counter()
            g, _ = build_pose_graph_for_scene(clouds, cfg, batched=batched, stats=stats)
            return (time.perf_counter() - t0) * 1e3, g

    stats = {}
    _, ga = run(True, stats)   # warm-up of every shape both paths use
    _, gb = run(False)
    same = len(ga.edges) == len(gb.edges) and all(
        x.transformation.tobytes() == y.transformation.tobytes() and x.information.tobytes() == y.information.tobytes()
        for x, y in zip(ga.edges, gb.edges))
    ta, tb = [], []
    for _ in range(a.repeats):
        ta.append(run(True)[0])
        tb.append(run(False)[0])

    cs = CloudSet(clouds[Side.LEFT])
    levels = {"full": cs.counts}
    for v in cfg.icp_voxel_sizes:
        levels[f"voxel_{v}"] = [len(cs.voxel_down_sample(i, v)) for i in range(n_clouds)]
    levels[f"every_{int(cfg.pre_filter_every_k_points)}"] = [-(-c // int(cfg.pre_filter_every_k_points))
                                                              for c in cs.counts]
    cs.close()

    out = {"capture": {"scene": "room", "frames": a.frames, "fragment_size": a.fragment, "fragments": n_clouds,
                       "voxel_size": cfg.voxel_size},
           "pairs": stats.get("pairs"), "icp_pairs": stats.get("icp_pairs"), "edges": len(ga.edges),
           "points_per_level": levels, "repeats": a.repeats,
           "batched_ms": sorted(round(x, 3) for x in ta), "single_ms": sorted(round(x, 3) for x in tb),
           "batched_ms_median": round(float(np.median(ta)), 3), "single_ms_median": round(float(np.median(tb)), 3),
           "batched_equals_single_bitwise": bool(same)}
    if not a.skip_cpu:
        host = {Side.LEFT: [c.points for c in clouds[Side.LEFT]]}
        t0 = time.perf_counter()
        edges, why = ref.pose_graph(host, cfg)
        out["cpu_reference_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        out["cpu_decisions"] = why
        out["cpu_edges"] = len(edges)
        if len(edges) == len(ga.edges):
            out["max_abs_T_diff_vs_cpu"] = max((float(np.abs(e.transformation - x["transformation"]).max())
                                                for e, x in zip(ga.edges, edges)), default=0.0)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
