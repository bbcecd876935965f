"""Mesh simplification on the GPU (csrc/meshsimplify.hip, mqr.downsample_mesh), timed on C2's mesh and, with
--c5, on C5's.

The captures are tools/mesh_quality_probe.py's (C2: 500 frames of the room walk, 5 mm voxels; C5: a LEFT +
RIGHT walk through the hall, 3 mm voxels): fused, extracted and filtered, the mesh left in HBM with random
per-vertex colours beside it in HBM.  Per mesh and per target (50 %, 10 %, 1 % of the vertices, the fit rule):

  downsample_wall_ms  the host clock around downsample_mesh(mesh, percent) as a caller uses it (the search's
                      count calls, the clustering call and the result's allocation inside), after one untimed
                      call, `--wall-repeats` calls;
  count_calls         the mqr_mesh_cluster_count calls of one downsample_mesh, and the size and count chosen;
  simplify_ms         device time of one mqr_mesh_simplify_clustering at the chosen size (events on the call's
                      stream, mqr_mesh_simplify_last_ms: whole call, the part up to the output vertices, the
                      triangles), after `--warmup` untimed calls, `--repeats` calls;
  count_ms            device time of one mqr_mesh_cluster_count at the chosen size, the same way;
  stats               the call's stats[8];
  algorithmic_bytes   the bytes the call's passes move when each array is read and written once per pass (the
                      vertex and triangle sorts as hipcub runs them: 8 bits per pass, keys and values read and
                      written in each, a histogram read of the keys first), and the fraction of the HBM peak
                      (8 TB/s) that simplify_ms makes of them.

`host_numpy_ms_once` is the wall time of tests/simplify_ref.py's simplify (the numpy restatement of the rule) on
the same mesh on the host at the 10 % size, once: the host figure the device call replaces.  No time here is a
pass / fail condition.  Writes profiles/mesh_simplify.json and prints it.

    python tools/mesh_simplify_probe.py [--c5] [--repeats 20] [--warmup 3]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

HBM_PEAK = 8.0e12
PERCENTS = (50, 10, 1)


def spread(ms):
    ms = sorted(ms)
    return {"median": ms[len(ms) // 2], "min": ms[0], "max": ms[-1], "repeats": len(ms)}


def algorithmic_bytes(st, normals, colors):
    """Bytes of one call, every array read and written once per pass (see the module docstring)."""
    nv, C, nt, kept = st[0], st[1], st[2], st[5]
    fields = 1 + int(normals) + int(colors)
    vbits = 3 * max(1, int(st[7] - 1).bit_length())            # an upper bound: the widest axis' bits, three times
    vpass = -(-vbits // 8)
    bc = max(1, int(C - 1).bit_length())
    tpass = -(-(3 * bc) // 8) if C < (1 << 21) else -(-bc // 8) + -(-(32 + bc) // 8)
    b = 12 * nv * 2 + 12 * nt                                  # finite check, bounds, index check
    b += 12 * nv + 12 * nv                                     # keys + iota: read positions, write (8 + 4)
    b += 8 * nv + vpass * 2 * 12 * nv                          # vertex sort: histogram, then passes of (8 + 4) in and out
    b += 12 * nv + 8 * nv + 2 * 8 * nv + 8 * nv + 4 * C        # heads (+ flags), two scans, segment starts
    b += 4 * nv + 12 * nv * fields + 4 * nv + 12 * C * fields  # cells: indices, gathers, map, outputs
    b += 12 * nt + 12 * nt + 12 * nt                           # triples: corners, map gathers, key + iota
    b += 8 * nt + tpass * 2 * 12 * nt                          # triangle sort
    b += 12 * nt + 4 * nt + 8 * nt + 12 * nt + 12 * kept       # keep, scan, compaction
    return int(b), {"vertex_sort_passes": vpass, "triangle_sort_passes": tpass}


def measure(mesh, a, label):
    from mqr import _lib
    from mqr.downsample_mesh import downsample_mesh, fit_voxel_size, reference_voxel_size, target_vertex_count
    from mqr.geometry import DeviceArray, ResidentMesh, Tensor, device_mesh, mesh_fields
    import simplify_ref as sr
    d = device_mesh(mesh_fields(mesh), normals=True)
    assert d is not None and d.normals is not None, "the probe times a mesh held in HBM"
    nv, nt = d.nv, d.nt
    col = np.random.default_rng(0).random((nv, 3)).astype(np.float32)
    cbuf = _lib.DeviceBuffer.from_array(col, d.device)
    mesh.vertex["colors"] = Tensor(DeviceArray(cbuf, cbuf.ptr.value, col.shape, col.dtype, d.device))
    vp = ctypes.c_void_p

    def last_ms():
        ms = [ctypes.c_float() for _ in range(3)]
        _lib.call("mqr_mesh_simplify_last_ms", d.device, *[ctypes.byref(x) for x in ms])
        return [x.value for x in ms]

    out = {"vertices": nv, "triangles": nt, "fields": "positions, normals, colours; inputs and the result in HBM",
           "warmup": a.warmup, "targets": {}}
    size10 = None
    for pct in PERCENTS:
        target = target_vertex_count(nv, pct)
        rec = {"target": target}
        wall, res = [], None
        for k in range(1 + a.wall_repeats):
            res = None  # the previous result's block goes back before the next call allocates
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(io.StringIO()):
                res = downsample_mesh(mesh, pct)
            if k >= 1:
                wall.append((time.perf_counter() - t0) * 1e3)
        rec["downsample_wall_ms"] = {**spread(wall), "warmup": 1}
        rec["vertices_reached"] = len(res.vertex.positions)
        rec["triangles_reached"] = len(res.triangle.indices)
        del res
        # the search downsample_mesh ran, once more through its public pieces: its calls, the size it chose
        r = ResidentMesh(mesh)
        lo, hi = r.bounds()
        v_ref = reference_voxel_size(float(np.linalg.norm(hi - lo)), target)
        size, count, seen = fit_voxel_size(r.cluster_count, v_ref, target)
        assert count == rec["vertices_reached"], (count, rec["vertices_reached"])
        rec["count_calls"] = len(seen)
        rec["voxel_size"] = size
        rec["reference_voxel_size"] = v_ref
        rec["vertices_at_reference_voxel_size"] = seen[0][1]
        if pct == 10:
            size10 = size
        sim, cnt, stats = {"call": [], "vertex": [], "triangle": []}, [], None
        for k in range(a.warmup + a.repeats):
            g, st = vp(), np.zeros(8, np.int64)
            _lib.call("mqr_mesh_simplify_clustering", d.device, vp(d.positions), nv, vp(d.normals), cbuf.ptr,
                      vp(d.triangles), nt, _lib.MQR_DEVICE, size, ctypes.byref(g), _lib.ptr(st, _lib._i64p))
            ms = last_ms()
            _lib.call("mqr_geom_free", g)
            if k >= a.warmup:
                for key, x in zip(("call", "vertex", "triangle"), ms):
                    sim[key].append(x)
            stats = [int(x) for x in st]
        for k in range(a.warmup + a.repeats):
            r.cluster_count(size)
            if k >= a.warmup:
                cnt.append(last_ms()[0])
        r.free()
        rec["simplify_ms"] = {k: spread(x) for k, x in sim.items()}
        rec["count_ms"] = spread(cnt)
        rec["stats"] = stats
        b, passes = algorithmic_bytes(stats, True, True)
        rec["algorithmic_bytes"] = b
        rec.update(passes)
        rec["fraction_of_hbm_peak"] = b / (rec["simplify_ms"]["call"]["median"] * 1e-3) / HBM_PEAK
        out["targets"][str(pct)] = rec
        print(f"mesh_simplify_probe: {label}: {pct} % timed", file=sys.stderr, flush=True)
    # ---- the host figure: the numpy restatement on the same mesh, once
    host = mesh.cpu()
    v, t, n = host.vertices, host.triangles, host.vertex_normals
    print(f"mesh_simplify_probe: {label}: numpy restatement running", file=sys.stderr, flush=True)
    t0 = time.perf_counter()
    want = sr.simplify(v, t, size10, n, col)
    out["host_numpy_ms_once"] = (time.perf_counter() - t0) * 1e3
    out["host_numpy_what"] = "tests/simplify_ref.py simplify() at the 10 % size, the mesh already on the host"
    out["host_numpy_stats_equal_device"] = [int(x) for x in want[4]] == out["targets"]["10"]["stats"]
    out["host_numpy_over_device_call"] = (out["host_numpy_ms_once"]
                                          / out["targets"]["10"]["simplify_ms"]["call"]["median"])
    del mesh.vertex["colors"]
    cbuf.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--c5", action="store_true", help="also time C5's mesh (minutes of fusing)")
    ap.add_argument("--frames-per-side", type=int, default=2000)
    ap.add_argument("--c2-frames", type=int, default=500)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--wall-repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_simplify.json"))
    a = ap.parse_args()
    if a.repeats < 20:
        raise SystemExit("mesh_simplify_probe: at least 20 repetitions")

    from mqr import _lib, synthetic
    if _lib.device_count() < 1:
        raise SystemExit("mesh_simplify_probe: no GPU (there is no CPU fallback; nothing is written)")
    from mesh_quality_probe import fuse
    from mqr.meshfilter import filter_mesh_components

    def filtered(mesh):
        with contextlib.redirect_stdout(io.StringIO()):
            return filter_mesh_components(mesh)

    out = {"what": "HIP events on the call's stream (simplify_ms, count_ms) and the host clock (downsample_wall_ms, "
                   "host_numpy_ms_once); median, min, max over `repeats`"}
    if os.path.exists(a.out):  # a run without --c5 keeps an earlier record's C5 block, marked as older
        with open(a.out) as f:
            old = json.load(f).get("c5")
        if old is not None and not a.c5:
            old["kept_from_an_earlier_record"] = True
            out["c5"] = old

    def save():
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)

    mesh, B = fuse("room", synthetic.room_loop_poses(a.c2_frames), 0, 0.005, 40000, 3.0)
    out["c2"] = {"capture": {"scene": "room", "frames": B, "voxel_size": 0.005}, **measure(filtered(mesh), a, "c2")}
    del mesh
    save()
    if a.c5:
        left = synthetic.hall_loop_poses(a.frames_per_side)
        poses = left + [(R_, t_ + R_[:, 0] * 0.064) for R_, t_ in left]
        mesh, B = fuse("hall", poses, 5, 0.003, 16384, 1.5)
        out["c5"] = {"capture": {"scene": "hall", "frames": B, "voxel_size": 0.003}, **measure(filtered(mesh), a, "c5")}
        save()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
