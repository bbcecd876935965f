"""Grow-only device scratch (GrowBuf, csrc/devmem.hip) regrown and then reused while it still holds the
larger call's contents.  Per module, through the Python wrappers: a small call, a call large enough that
every buffer of the module regrows (more than 1.5x the small call's bytes, the largest growth factor any
module uses), and the small call again.  The third result is bit-identical to the first, and the large one
is checked the way the module's own test checks it.

The buffers of odometry, decoding, the packed counts and the mesh filter live for the life of the process,
so whether a call regrows them depends on what ran before it.  The three calls of every module therefore run
in one fresh process (this file run as a script), which the tests start once; they check what it saved."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---------------------------------------------------------------- odometry information pairs
# device buffers of mqr_odometry_information_pairs (1.5x growth, 4096-byte floor): frames, pair records
# (104 B each), slabs (22 doubles per pair and 1024-pixel tile), outputs (36 doubles + one int64 per pair)
#   small  2 frames of 8 x 8, 1 pair:     frames 512 B, pairs 104 B, slabs 176 B, outputs 296 B -> all at the floor
#   large  4 frames of 64 x 96, 16 pairs: frames 98 304 B, slabs 22 * 8 * 16 * 6 = 16 896 B, outputs 4 736 B
#          (frames and slabs regrow past 1.5x the floor, the outputs regrow; the 1 664 B of pair records still
#          fit the floor allocation)
def _odometry_inputs():
    import odometry_ref as ref
    from mqr import synthetic
    seq = synthetic.make_sequence("room", n=4, height=64, width=96, f=84.0, noise=True, seed=7,
                                  poses=synthetic.room_loop_poses(96)[:4])
    depth = np.ascontiguousarray(seq["depth"], np.float32)
    Twc, Tcw = seq["T_wc"].astype(np.float64), seq["T_cw"].astype(np.float64)
    pairs = [(a, b) for a in range(4) for b in range(4) if a != b] + [(0, 1), (1, 2), (2, 3), (3, 0)]
    src = np.array([a for a, _ in pairs], np.int32)
    tgt = np.array([b for _, b in pairs], np.int32)
    T = np.stack([ref.perturbed(Twc[b] @ Tcw[a], 200 + i) for i, (a, b) in enumerate(pairs)])
    K = seq["K"][0].astype(np.float64)
    # the central 8 x 8 pixels of frame 0, twice (a few millimetres apart, T_small): the principal point moves
    small = np.ascontiguousarray(depth[[0, 0], 28:36, 44:52])
    K_small = K.copy()
    K_small[0, 2] -= 44.0
    K_small[1, 2] -= 28.0
    return dict(depth=depth, small=small, K=K, K_small=K_small, src=src, tgt=tgt, T=T,
                T_small=ref.perturbed(np.eye(4), 300))


def _run_odometry():
    import odometry_ref as ref
    from mqr.odometry import odometry_information_pairs
    d = _odometry_inputs()
    out = {}
    for tag in ("first", "large", "third"):
        if tag == "large":
            r = odometry_information_pairs(d["depth"], d["K"], d["src"], d["tgt"], d["T"], ref.DIST_THRESHOLD, 1.0,
                                           ref.DEPTH_MAX)
        else:
            r = odometry_information_pairs(d["small"], d["K_small"], [0], [1], d["T_small"], ref.DIST_THRESHOLD, 1.0,
                                           ref.DEPTH_MAX)
        out[tag + ".info"], out[tag + ".counts"] = r
    return out


def test_odometry_information_pairs(runs):
    import odometry_ref as ref
    d = _odometry_inputs()
    assert d["depth"].shape == (4, 64, 96) and len(d["src"]) == 16 and d["small"].shape == (2, 8, 8)
    for k in ("info", "counts"):
        assert _bits_equal(runs[f"odometry.third.{k}"], runs[f"odometry.first.{k}"]), k
    info, counts = runs["odometry.large.info"], runs["odometry.large.counts"]
    rinfo, rcounts, m = ref.information_pairs(d["depth"], d["K"], d["src"], d["tgt"], d["T"], ref.DIST_THRESHOLD, 1.0,
                                              ref.DEPTH_MAX)
    print("margins", m, "counts", counts.tolist())
    assert m["round"] >= 1e-7 and m["dist"] >= 1e-7  # no decision within rounding: equal counts are meaningful
    assert np.array_equal(counts, rcounts) and counts.min() > 0
    for p in range(len(info)):  # as tests/test_gpu_odometry.py: float64 sums taken in a different order
        err = np.abs(info[p] - rinfo[p]).max() / np.abs(rinfo[p]).max()
        assert err <= 1e-9, (p, err)
        assert np.array_equal(info[p], info[p].T)
    _, scounts, sm = ref.information_pairs(d["small"], d["K_small"], [0], [1], d["T_small"][None],
                                           ref.DIST_THRESHOLD, 1.0, ref.DEPTH_MAX)
    assert sm["round"] >= 1e-7 and sm["dist"] >= 1e-7 and scounts[0] > 0
    assert np.array_equal(runs["odometry.first.counts"], scounts)


# ---------------------------------------------------------------- registration information pairs
# scratch of one cloud set (1.5x growth, 4096-byte floor): pair descriptors (48 B each), pair state (176 B),
# slabs (22 doubles per pair and 256-point block of its source), information (288 B per pair)
#   small  1 pair:    48 B, 176 B, 22 * 8 * 3 = 528 B, 288 B -> all at the floor
#   large  140 pairs: 6 720 B, 24 640 B, 22 * 8 * 504 = 88 704 B, 40 320 B -> each more than 1.5x the floor (6 144 B)
REG_SIZES = [600, 1000, 777, 1500, 64]
REG_RADIUS = 0.1


def _registration_inputs():
    import registration_ref as ref
    clouds = [ref.apply(ref.motion(0.4 * i, -0.3 * i, 0.5 * i, (0.004 * i, -0.003 * i, 0.002 * i)),
                        ref.surface(n + 3, 10 + i)[:n]) for i, n in enumerate(REG_SIZES)]
    pairs = [(a, b) for a in range(5) for b in range(5) if a != b]
    src = np.array([a for a, _ in pairs] * 7, np.int32)
    tgt = np.array([b for _, b in pairs] * 7, np.int32)
    return clouds, src, tgt


def _run_registration():
    from mqr.registration import CloudSet
    clouds, src, tgt = _registration_inputs()
    cs = CloudSet(clouds)
    out = {}
    for tag in ("first", "large", "third"):
        s, t = (src, tgt) if tag == "large" else ([0], [1])
        out[tag + ".info"] = cs.information_pairs(s, t, REG_RADIUS, np.eye(4))
    cs.close()
    return out


def test_registration_information_pairs(runs):
    import registration_ref as ref
    clouds, src, tgt = _registration_inputs()
    assert [len(c) for c in clouds] == REG_SIZES and len(src) == 140
    assert _bits_equal(runs["registration.third.info"], runs["registration.first.info"])
    got = runs["registration.large.info"]
    m = ref.Margins()
    for i in range(20):  # as tests/test_gpu_registration.py: equal inlier counts, sums within 1e-9
        exp = ref.information(clouds[src[i]], clouds[tgt[i]], REG_RADIUS, np.eye(4), m)
        assert got[i][3, 3] == exp[3, 3] == got[i][4, 4] == got[i][5, 5] and exp[3, 3] > 0, i
        assert np.array_equal(got[i], got[i].T)
        rel = float(np.abs(got[i] - exp).max() / np.abs(exp).max())
        assert rel <= 1e-9, (i, rel)
    print("tie margin", m.tie, "radius margin", m.radius)
    assert m.tie > 1e-9 and m.radius > 1e-9
    for i in range(20, 140):  # the repeats of a pair within the batch
        assert np.array_equal(got[i], got[i % 20]), i
    assert np.array_equal(runs["registration.first.info"][0], got[0])


# ---------------------------------------------------------------- depth decode
# device buffers of the decode context (exact growth): scratch = staged raw + staged output, and the
# per-frame parameter / flag arrays (for at least 256 frames)
#   small  2 frames of 24 x 32:   scratch 2 * 6 144 = 12 288 B, frame arrays for 256 frames
#   large  390 frames of 24 x 32: scratch 2 * 1 198 080 = 2 396 160 B, frame arrays for 390 frames (1.52x)
def _decode_inputs(golden_dir):
    g = np.load(os.path.join(golden_dir, "decode_golden.npz"))
    return g["raw"], g["params"][0], g["linear64"][0], g["valid"]


def _run_decode():
    from mqr.ingest import decode_depth_frames
    raw, (near, far), _, _ = _decode_inputs(os.path.join(ROOT, "tests", "golden"))
    big = np.ascontiguousarray(np.tile(raw, (65, 1, 1)))
    out = {}
    for tag in ("first", "large", "third"):
        r = big if tag == "large" else raw[:2]
        out[tag + ".depth"], out[tag + ".ok"] = decode_depth_frames(r, [np.float64(near)] * len(r),
                                                                    [np.float64(far)] * len(r))
    return out


def test_depth_decode(runs, golden_dir):
    raw, _, linear, valid = _decode_inputs(golden_dir)
    assert raw.shape == (6, 24, 32)
    for k in ("depth", "ok"):
        assert _bits_equal(runs[f"decode.third.{k}"], runs[f"decode.first.{k}"]), k
    assert runs["decode.large.depth"].shape == (390, 24, 32)
    # the reference's own decode (tests/golden/decode_golden.npz), bit for bit
    assert np.array_equal(runs["decode.large.ok"], np.tile(valid, 65))
    assert np.array_equal(runs["decode.large.depth"].view(np.uint32), np.tile(linear, (65, 1, 1)).view(np.uint32))
    assert np.array_equal(runs["decode.first.depth"].view(np.uint32), linear[:2].view(np.uint32))


# ---------------------------------------------------------------- packed confidence counts
# device buffers of mqr_confidence_counts (exact growth): the maps (8 + 4 B per pixel) and the pairs (2 B)
#   small  1 reference frame of 30 x 40:  maps 9 728 + 4 800 = 14 528 B, pairs 2 400 B
#   large  7 reference frames of 30 x 40: maps 67 328 + 33 600 = 100 928 B, pairs 16 800 B (7x)
CONF_RANGE = 2


def _counts_inputs():
    from mqr import synthetic
    return synthetic.make_sequence("room", n=7, height=30, width=40, f=33.0, noise=True, seed=6)


def _run_counts():
    import ctypes
    from mqr import _lib
    seq = _counts_inputs()
    B, H, W = seq["depth"].shape
    depth = np.ascontiguousarray(seq["depth"], np.float32)
    Tcw = np.ascontiguousarray(seq["T_cw"].astype(np.float32).reshape(B, 16))
    Tci = np.ascontiguousarray(np.linalg.inv(seq["T_cw"]).astype(np.float32).reshape(B, 16))
    K32 = np.ascontiguousarray(seq["K"], np.float32)
    out = {}
    for tag in ("first", "large", "third"):
        a, b = (0, B) if tag == "large" else (3, 4)
        counts = np.full((b - a, H, W), 0xFFFF, np.uint16)
        packed = ctypes.c_int(-1)
        _lib.call("mqr_confidence_counts", 0, _lib.ptr(depth), _lib.MQR_HOST, B, H, W, _lib.ptr(K32, _lib._f32p),
                  _lib.ptr(Tcw, _lib._f32p), _lib.ptr(Tci, _lib._f32p), None, a, b, CONF_RANGE, 3.0, 0.05,
                  _lib.ptr(counts), ctypes.byref(packed))
        assert packed.value == 1
        out[tag + ".counts"] = counts
    return out


def test_packed_confidence_counts(runs):
    import oracle
    seq = _counts_inputs()
    assert seq["depth"].shape == (7, 30, 40)
    assert _bits_equal(runs["counts.third.counts"], runs["counts.first.counts"])
    counts = runs["counts.large.counts"]
    valid, cons = (counts & 0xFF).astype(np.int32), (counts >> 8).astype(np.int32)
    assert (cons <= valid).all() and 0 < valid.max() <= 2 * CONF_RANGE
    Tinv = np.linalg.inv(seq["T_cw"])
    for i in range(7):  # as tests/test_gpu_stream_order.py: the pairs expand to the oracle's maps exactly
        oc, ov = oracle.confidence(seq["depth"], seq["K"], seq["T_cw"], Tinv, i, CONF_RANGE, 3.0, 0.05)
        with np.errstate(divide="ignore", invalid="ignore"):
            c = np.true_divide(cons[i], valid[i])
        c[valid[i] == 0] = 0.0
        assert np.array_equal(valid[i], ov) and np.array_equal(c.view(np.uint64), oc.view(np.uint64)), i
    assert np.array_equal(runs["counts.first.counts"][0], counts[3])


# ---------------------------------------------------------------- mesh-filter components
# device buffers: the arena, 128 B per triangle + 96 B per vertex + 32 MiB (exact growth), and the result's
# block from the device-block cache (whole MiB)
#   small  the 12-vertex, 8-triangle known-answer mesh, no normals: arena 33 556 608 B, result block 1 MiB
#   large  a 240 x 240 grid (57 600 + 27 vertices, 114 242 + 24 triangles) with normals:
#          arena 33 554 432 + 20 158 240 = 53 712 672 B (1.6x), result block 3 MiB
MF_MIN_SMALL, MF_MIN_LARGE = 2, 50


def _meshfilter_inputs():
    G = 240
    ii, jj = np.meshgrid(np.arange(G), np.arange(G), indexing="ij")
    sheet = np.stack([ii * 0.01, jj * 0.01, 0.002 * np.sin(ii * 0.3) * np.cos(jj * 0.2)], -1).reshape(-1, 3)

    def grid_triangles(g, base):
        a = (np.arange(g - 1)[:, None] * g + np.arange(g - 1)[None, :]).ravel() + base
        return np.concatenate([np.stack([a, a + g, a + 1], 1), np.stack([a + 1, a + g, a + g + 1], 1)])

    # three floating 3 x 3 patches (8 triangles each) above the sheet: components the filter removes
    patches, tris = [], [grid_triangles(G, 0)]
    for k in range(3):
        pi, pj = np.meshgrid(np.arange(3), np.arange(3), indexing="ij")
        patches.append(np.stack([0.3 * k + pi * 0.01, 0.5 + pj * 0.01, np.full(pi.shape, 0.2)], -1).reshape(-1, 3))
        tris.append(grid_triangles(3, G * G + 9 * k))
    V = np.ascontiguousarray(np.concatenate([sheet] + patches), np.float32)
    T = np.ascontiguousarray(np.concatenate(tris), np.int32)
    N = np.random.default_rng(2).standard_normal(V.shape).astype(np.float32)
    return V, N, T


def _run_meshfilter():
    from mqr.meshfilter import filter_mesh_components_gpu
    from test_oracle_meshfilter import T as T_KAT, V as V_KAT
    V, N, T = _meshfilter_inputs()
    out = {}
    for tag in ("first", "large", "third"):
        if tag == "large":
            v, n, t, st = filter_mesh_components_gpu(V, N, T, MF_MIN_LARGE)
            out[tag + ".n"] = n
        else:
            v, _, t, st = filter_mesh_components_gpu(V_KAT, None, T_KAT, MF_MIN_SMALL)
        out[tag + ".v"], out[tag + ".t"] = v, t
        out[tag + ".stats"] = np.array([st[k] for k in sorted(st)], np.int64)
        out["stats_keys"] = np.array(sorted(st))
    return out


def test_mesh_filter_components(runs):
    import meshfilter_ref as mf
    from test_oracle_meshfilter import T as T_KAT, V as V_KAT
    V, N, T = _meshfilter_inputs()
    assert len(V) == 57627 and len(T) == 114266
    for k in ("v", "t", "stats"):
        assert _bits_equal(runs[f"meshfilter.third.{k}"], runs[f"meshfilter.first.{k}"]), k
    # as tests/test_gpu_meshfilter.py: the CPU restatement's arrays and statistics, bit for bit
    for tag, ref in (("large", mf.filter_mesh_components(V, N, T, MF_MIN_LARGE)),
                     ("first", mf.filter_mesh_components(V_KAT, None, T_KAT, MF_MIN_SMALL))):
        rv, rn, rt, rst = ref
        assert np.array_equal(runs[f"meshfilter.{tag}.t"], rt)
        assert np.array_equal(runs[f"meshfilter.{tag}.v"].view(np.uint32), rv.view(np.uint32))
        if rn is not None:
            assert np.array_equal(runs[f"meshfilter.{tag}.n"].view(np.uint32), rn.view(np.uint32))
        st = dict(zip(runs["meshfilter.stats_keys"].tolist(), runs[f"meshfilter.{tag}.stats"].tolist()))
        for k, val in rst.items():
            assert st[k] == val, (tag, k, st[k], val)
        if tag == "large":
            assert rst["clusters"] == 4 and rst["kept_clusters"] == 1 and len(rt) == 114242


# ---------------------------------------------------------------- mesh extraction
# the volume's extraction scratch (1.25x growth): ~9.1 KB per block at R = 16 (neighbour table, counts and
# offsets, row records, bit planes).  One volume: filled with one view's blocks, emptied and filled from all
# six frames (more than 1.5x the blocks, asserted), emptied and filled with the one view's blocks again.
# A block's place in the pool decides where its output goes, and integration hands places out with atomics;
# the one-view fill therefore imports the blocks one by one in key order, which fixes the places.
EX = dict(vs=0.02, R=16, dmax=3.0, tm=4.0, thr=1.5)


def _extract_inputs():
    from mqr import synthetic
    return synthetic.make_sequence("sphere", n=6, height=120, width=160, f=131.25, noise=True, seed=1)


def _run_extract():
    from gpu_helpers import canon_blocks
    from mqr.vbg import VoxelBlockGrid
    seq = _extract_inputs()
    args = dict(depth_scale=1.0, depth_max=EX["dmax"], trunc_voxel_multiplier=EX["tm"])
    one = VoxelBlockGrid(voxel_size=EX["vs"], block_resolution=EX["R"], block_count=64)
    # three frames' blocks stand in for "small": one frame alone leaves no cube with every corner seen twice
    one.integrate_frames(seq["depth"][:1].repeat(3, 0), seq["K"][:1].repeat(3, 0), seq["T_wc"][:1].repeat(3, 0), **args)
    keys, tsdf, weight = canon_blocks(*one.export())
    vbg = VoxelBlockGrid(voxel_size=EX["vs"], block_resolution=EX["R"], block_count=64)
    out = {"small_blocks": np.int64(len(keys))}
    for tag in ("first", "large", "third"):
        if tag == "large":
            vbg.integrate_frames(seq["depth"], seq["K"], seq["T_wc"], **args)
            out["large_blocks"] = np.int64(vbg.size())
        else:
            for i in range(len(keys)):
                vbg.import_blocks(keys[i:i + 1], tsdf[i:i + 1], weight[i:i + 1])
        mesh = vbg.extract_triangle_mesh(weight_threshold=EX["thr"])
        out[tag + ".v"], out[tag + ".n"], out[tag + ".t"] = mesh.vertices, mesh.vertex_normals, mesh.triangles
        vbg.reset()
    return out


def test_mesh_extraction(runs):
    import oracle
    from gpu_helpers import compare_meshes, compare_points_normals
    seq = _extract_inputs()
    print("blocks", runs["extract.small_blocks"], runs["extract.large_blocks"])
    assert runs["extract.large_blocks"] > 1.5 * runs["extract.small_blocks"] > 0
    for k in ("v", "n", "t"):
        assert _bits_equal(runs[f"extract.third.{k}"], runs[f"extract.first.{k}"]), k
    K, T = seq["K"].astype(np.float64), seq["T_wc"].astype(np.float64)
    for tag, frames in (("large", range(6)), ("first", (0, 0, 0))):  # as tests/test_gpu_tsdf.py
        ref = oracle.OracleVBG(EX["vs"], EX["R"], 64)
        for i in frames:
            ref.integrate_frame(seq["depth"][i], K[i], T[i], 1.0, EX["dmax"], EX["tm"])
        ov, on, ot = ref.extract_mesh(EX["thr"])
        assert len(ot) > 100, tag
        compare_meshes(runs[f"extract.{tag}.v"], runs[f"extract.{tag}.t"], ov, ot, pos_tol=0.0)
        compare_points_normals(runs[f"extract.{tag}.v"], runs[f"extract.{tag}.n"], ov, on, 1e-6)


# ---------------------------------------------------------------- the fresh process
RUNNERS = dict(odometry=_run_odometry, registration=_run_registration, decode=_run_decode, counts=_run_counts,
               meshfilter=_run_meshfilter, extract=_run_extract)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """{module.call.array: value} of the three calls of every module, made by one fresh process."""
    out = str(tmp_path_factory.mktemp("scratch_reuse") / "runs.npz")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), out], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    with np.load(out) as z:
        return {k: z[k] for k in z.files}


if __name__ == "__main__":
    for path in (os.path.join(ROOT, "metaquest-3d-reconstruction_amd"), os.path.join(ROOT, "oracle"), ROOT):
        sys.path.insert(0, path)
    results = {}
    for name, fn in RUNNERS.items():
        for key, value in fn().items():
            results[f"{name}.{key}"] = np.asarray(value)
    np.savez(sys.argv[1], **results)
