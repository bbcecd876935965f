"""Surface sampling on the GPU (csrc/meshsample.hip), timed on C2's mesh and, with --c5, on C5's.

The captures are tools/mesh_quality_probe.py's (C2: 500 frames of the room walk, 5 mm voxels; C5: a LEFT +
RIGHT walk through the hall, 3 mm voxels): fused, extracted and filtered, the mesh left in HBM with random
per-vertex colours beside it.  n = 2 * vertices (the reference's points_per_vertex_ratio of 2.0).  After
`--warmup` untimed calls, `--repeats` calls of mqr_mesh_sample_points time, inputs and outputs in HBM, the
outputs allocated once:

  call_ms    events on the call's stream (the caller's) around everything the call enqueues (the input checks and the
             host's read of their flags included);
  table_ms   the selection table alone: areas, weights, scan, coarse table;
  sample_ms  the sample kernel alone: the default two-level search (coarse table, then one 256-entry segment)
             and, alternating with it call by call, the one-level search over the whole table
             (mqr_mesh_sample_set_flat_search); the outputs of the two are compared;
  host_clock_ms  the host clock around the same calls (each drains its stream before returning).

`python_call_ms` is TriangleMesh.sample_points_uniformly as a caller uses it (colours attached as a host
tensor, as optimize_color_pose leaves them: their upload and the output allocations are inside).  The baseline
is the only way the parent commit samples a mesh: compare_mesh_to_ground_truth.mesh_to_point_cloud(mesh, n) on
the host (numpy, float64 cumsum; positions only, no normals or colours), host clock, `--host-repeats` calls.
`ply_write_ms_once` is the host writer's time for the coloured cloud.  Writes profiles/mesh_sample.json and
prints it.

    python tools/mesh_sample_probe.py [--c5] [--repeats 20] [--warmup 3]
"""
import argparse
import contextlib
import ctypes
import io
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "metaquest-3d-reconstruction_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402


def spread(ms):
    ms = sorted(ms)
    return {"median": ms[len(ms) // 2], "min": ms[0], "max": ms[-1], "repeats": len(ms)}


def measure(mesh, a, label):
    from mqr import _lib
    from mqr import compare_mesh_to_ground_truth as cm
    from mqr.geometry import Tensor, device_mesh, mesh_fields, write_point_cloud
    d = device_mesh(mesh_fields(mesh), normals=True)
    assert d is not None and d.normals is not None, "the probe times a mesh held in HBM"
    nv, nt, n = d.nv, d.nt, 2 * d.nv
    col = np.random.default_rng(0).random((nv, 3)).astype(np.float32)
    cbuf = _lib.DeviceBuffer.from_array(col)
    outs = [_lib.DeviceBuffer(12 * n) for _ in range(3)]
    vp = ctypes.c_void_p

    def call():
        _lib.call("mqr_mesh_sample_points", d.device, vp(d.positions), nv, vp(d.normals), cbuf.ptr, vp(d.triangles), nt,
                  _lib.MQR_DEVICE, n, 0, 0, outs[0].ptr, outs[1].ptr, outs[2].ptr, None, _lib.MQR_DEVICE)

    def last_ms():
        ms = [ctypes.c_float() for _ in range(3)]
        _lib.call("mqr_mesh_sample_last_ms", d.device, *[ctypes.byref(x) for x in ms])
        return [x.value for x in ms]

    rec = {"two_level": {"call": [], "table": [], "sample": [], "host": []},
           "one_level": {"call": [], "table": [], "sample": [], "host": []}}
    pos = {}
    for r in range(a.warmup + a.repeats):
        for flat, key in ((0, "two_level"), (1, "one_level")):  # alternating, in one run
            _lib.call("mqr_mesh_sample_set_flat_search", flat)
            t0 = time.perf_counter()
            call()
            host = (time.perf_counter() - t0) * 1e3
            if r >= a.warmup:
                c, t, s = last_ms()
                for k, x in zip(("call", "table", "sample", "host"), (c, t, s, host)):
                    rec[key][k].append(x)
            if r == 0:
                pos[key] = outs[0].to_array((n, 3), np.float32)
    _lib.call("mqr_mesh_sample_set_flat_search", 0)
    print(f"mesh_sample_probe: {label}: device calls timed", file=sys.stderr, flush=True)
    out = {"vertices": nv, "triangles": nt, "n": n, "ratio": 2.0, "warmup": a.warmup,
           "fields": "positions, normals, colours; inputs and outputs in HBM",
           "call_ms": spread(rec["two_level"]["call"]), "table_ms": spread(rec["two_level"]["table"]),
           "sample_ms": spread(rec["two_level"]["sample"]), "host_clock_ms": spread(rec["two_level"]["host"]),
           "one_level_search": {"call_ms": spread(rec["one_level"]["call"]),
                                "sample_ms": spread(rec["one_level"]["sample"]),
                                "outputs_equal_two_level": bool(np.array_equal(pos["two_level"].view(np.uint32),
                                                                               pos["one_level"].view(np.uint32)))},
           "table_bytes": 8 * nt, "coarse_table_bytes": 8 * ((nt + 255) // 256)}
    out["samples_per_s"] = n / (out["call_ms"]["median"] * 1e-3)
    del pos

    # ---- the Python entry as a caller uses it
    mesh.vertex["colors"] = Tensor(col)
    py, pc = [], None
    for r in range(a.warmup + a.repeats):
        pc = None  # the previous cloud's buffers go back before the next call allocates
        t0 = time.perf_counter()
        pc = mesh.sample_points_uniformly(n)
        if r >= a.warmup:
            py.append((time.perf_counter() - t0) * 1e3)
    out["python_call_ms"] = spread(py)
    with tempfile.TemporaryDirectory() as tmp:
        t0 = time.perf_counter()
        write_point_cloud(os.path.join(tmp, "color.ply"), pc)
        out["ply_write_ms_once"] = (time.perf_counter() - t0) * 1e3
        out["ply_bytes"] = os.path.getsize(os.path.join(tmp, "color.ply"))
    del pc
    del mesh.vertex["colors"]
    print(f"mesh_sample_probe: {label}: python entry and writer timed", file=sys.stderr, flush=True)

    # ---- the baseline: the parent commit's only sampler, on the host
    m = cm._Mesh(mesh)
    m.vertices  # the mesh's one copy to the host is not part of the baseline
    base = []
    for r in range(1 + a.host_repeats):
        t0 = time.perf_counter()
        p = cm.mesh_to_point_cloud(m, n)
        if r >= 1:
            base.append((time.perf_counter() - t0) * 1e3)
    assert p.shape == (n, 3)
    out["host_baseline_ms"] = {**spread(base), "warmup": 1,
                               "what": "compare_mesh_to_ground_truth.mesh_to_point_cloud(mesh, n): numpy on the "
                                       "host, positions only, the mesh already on the host"}
    out["host_baseline_over_device_call"] = out["host_baseline_ms"]["median"] / out["call_ms"]["median"]
    out["host_baseline_over_python_call"] = out["host_baseline_ms"]["median"] / out["python_call_ms"]["median"]
    for b in outs + [cbuf]:
        b.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--c5", action="store_true", help="also time C5's mesh (minutes of fusing)")
    ap.add_argument("--frames-per-side", type=int, default=2000)
    ap.add_argument("--c2-frames", type=int, default=500)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_sample.json"))
    a = ap.parse_args()
    if a.repeats < 20:
        raise SystemExit("mesh_sample_probe: at least 20 repetitions")

    from mqr import _lib, synthetic
    if _lib.device_count() < 1:
        raise SystemExit("mesh_sample_probe: no GPU (there is no CPU fallback; nothing is written)")
    from mesh_quality_probe import fuse
    from mqr.meshfilter import filter_mesh_components

    def filtered(mesh):
        with contextlib.redirect_stdout(io.StringIO()):
            return filter_mesh_components(mesh)

    out = {"what": "HIP events on the call's stream (call, table, sample) and the host clock around calls that "
                   "drain their stream before returning; median, min, max over `repeats`"}
    if os.path.exists(a.out):  # a run without --c5 keeps an earlier record's C5 block, marked as older
        with open(a.out) as f:
            old = json.load(f).get("c5")
        if old is not None and not a.c5:
            old["kept_from_an_earlier_record"] = True
            out["c5"] = old
    mesh, B = fuse("room", synthetic.room_loop_poses(a.c2_frames), 0, 0.005, 40000, 3.0)
    out["c2"] = {"capture": {"scene": "room", "frames": B, "voxel_size": 0.005}, **measure(filtered(mesh), a, "c2")}
    del mesh
    if a.c5:
        left = synthetic.hall_loop_poses(a.frames_per_side)
        poses = left + [(R_, t_ + R_[:, 0] * 0.064) for R_, t_ in left]
        mesh, B = fuse("hall", poses, 5, 0.003, 16384, 1.5)
        out["c5"] = {"capture": {"scene": "hall", "frames": B, "voxel_size": 0.003}, **measure(filtered(mesh), a, "c5")}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
