"""numpy float64 restatement of the odometry information rules (DESIGN "odometry information rules").
Test infrastructure: the product never imports this.  Vectorised over whole images, so it shares
nothing with the kernel's tiles or its reduction order.

Besides the matrix it reports two margins over all tested pixels: the smallest distance of a projected
u or v from a rounding boundary (k + 0.5), and the smallest |r^2 - thr^2| / thr^2.  An exact comparison
of counts with another float64 implementation is meaningful only while both are far above float64
rounding (tests/test_odometry_ref.py asserts >= 1e-7 on the inputs the GPU tests use).
"""
import numpy as np


def _valid(d, depth_max):
    with np.errstate(invalid="ignore"):
        return (d > 0.0) & (d <= depth_max) & np.isfinite(d)


def _round_half_away(x):
    return np.sign(x) * np.floor(np.abs(x) + 0.5)


def information(src_depth, tgt_depth, K, T, dist_threshold, depth_scale=1.0, depth_max=3.0):
    """-> (info (6, 6) float64, count int, margins dict(round=..., dist=...)); a margin is inf when no
    pixel reached its test."""
    src = np.asarray(src_depth, np.float32).astype(np.float64) / depth_scale
    tgt = np.asarray(tgt_depth, np.float32).astype(np.float64) / depth_scale
    H, W = src.shape
    K = np.asarray(K, np.float64)
    T = np.asarray(T, np.float64)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    margins = {"round": np.inf, "dist": np.inf}
    m = _valid(src, depth_max)
    d = src[m]
    s = np.stack([d * ((xx[m] - cx) / fx), d * ((yy[m] - cy) / fy), d], 1)
    q = s @ T[:3, :3].T + T[:3, 3]
    q = q[q[:, 2] > 0.0]
    with np.errstate(all="ignore"):
        u = fx * q[:, 0] / q[:, 2] + cx
        v = fy * q[:, 1] / q[:, 2] + cy
    for w in (u, v):
        f = w[np.isfinite(w)]
        if len(f):
            margins["round"] = min(margins["round"], float(np.abs(np.abs(f - np.floor(f)) - 0.5).min()))
    ur, vr = _round_half_away(u), _round_half_away(v)
    with np.errstate(invalid="ignore"):
        inb = (ur >= 0) & (ur < W) & (vr >= 0) & (vr < H)
    q, ur, vr = q[inb], ur[inb], vr[inb]
    dt = tgt[vr.astype(np.int64), ur.astype(np.int64)]
    ok = _valid(dt, depth_max)
    q, ur, vr, dt = q[ok], ur[ok], vr[ok], dt[ok]
    g = np.stack([dt * ((ur - cx) / fx), dt * ((vr - cy) / fy), dt], 1)
    r2 = ((g - q) ** 2).sum(1)
    thr2 = dist_threshold * dist_threshold
    if len(r2) and thr2 > 0:
        margins["dist"] = float((np.abs(r2 - thr2) / thr2).min())
    g = g[r2 <= thr2]
    n = len(g)
    J = np.zeros((n, 3, 6))
    J[:, 0, 1], J[:, 0, 2], J[:, 0, 3] = g[:, 2], -g[:, 1], 1.0
    J[:, 1, 0], J[:, 1, 2], J[:, 1, 4] = -g[:, 2], g[:, 0], 1.0
    J[:, 2, 0], J[:, 2, 1], J[:, 2, 5] = g[:, 1], -g[:, 0], 1.0
    info = np.einsum("nki,nkj->ij", J, J)
    return info, n, margins


def information_pairs(depths, K, src, tgt, T, dist_threshold, depth_scale=1.0, depth_max=3.0):
    """The batched form: (info (P, 6, 6), counts (P,), the smallest margins over the batch)."""
    T = np.asarray(T, np.float64)
    if T.ndim == 2:
        T = np.broadcast_to(T, (len(src), 4, 4))
    infos, counts, mr, md = [], [], np.inf, np.inf
    for p, (a, b) in enumerate(zip(src, tgt)):
        i, n, m = information(depths[a], depths[b], K, T[p], dist_threshold, depth_scale, depth_max)
        infos.append(i)
        counts.append(n)
        mr, md = min(mr, m["round"]), min(md, m["dist"])
    return (np.stack(infos) if infos else np.zeros((0, 6, 6))), np.array(counts, np.int64), {"round": mr, "dist": md}


def perturbed(T, seed, trans=0.003, rot=0.002):
    """T moved by a few millimetres / milliradians (a seeded small rigid motion applied on the left)."""
    rng = np.random.default_rng(seed)
    w = rng.uniform(-rot, rot, 3)
    t = rng.uniform(-trans, trans, 3)
    th = np.linalg.norm(w)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
    D = np.eye(4)
    D[:3, :3], D[:3, 3] = R, t
    return D @ np.asarray(T, np.float64)


def gpu_test_inputs():
    """The inputs of tests/test_gpu_odometry.py, built once on the CPU: two room sequences (60 x 80, and
    one rendered larger and cropped to 61 x 83), the 7 odometry + 3 skip pairs, and their true and
    perturbed relative poses.  K of the cropped sequence is the uncropped one (a crop at the origin)."""
    from mqr import synthetic
    out = {}
    for name, (h, w, ch, cw, seed) in {"even": (60, 80, 60, 80, 5), "odd": (64, 88, 61, 83, 6)}.items():
        # the first 8 poses of a 96-pose loop: neighbours a few degrees and centimetres apart
        seq = synthetic.make_sequence("room", n=8, height=h, width=w, f=70.0, noise=True, seed=seed,
                                      poses=synthetic.room_loop_poses(96)[:8])
        depth = np.ascontiguousarray(seq["depth"][:, :ch, :cw])
        src = np.array(list(range(7)) + [0, 2, 4], np.int32)
        tgt = np.array(list(range(1, 8)) + [2, 5, 7], np.int32)
        Twc, Tcw = seq["T_wc"].astype(np.float64), seq["T_cw"].astype(np.float64)
        T_true = np.stack([Twc[b] @ Tcw[a] for a, b in zip(src, tgt)])
        T_pert = np.stack([perturbed(T, 100 + i) for i, T in enumerate(T_true)])
        out[name] = dict(depth=depth, K=seq["K"][0].astype(np.float64), src=src, tgt=tgt, T_true=T_true, T_pert=T_pert)
    return out


def degenerate_cases(d):
    """(frames, src, tgt, T) of the degenerate pairs, from one entry of gpu_test_inputs()."""
    base = d["depth"]
    N, H, W = base.shape
    frames = np.concatenate([base[:2], np.zeros((4, H, W), np.float32)])
    frames[2] = 0.0                                  # 2: all-zero frame
    frames[3] = base[1]
    frames[3, :, W // 2:] = 0.0                      # 3: frame 1 with a zeroed half
    frames[4] = base[0] + 3.5                        # 4: every depth above depth_max
    frames[5] = base[0]
    frames[5, ::3, ::5] = np.nan                     # 5: NaN depths sprinkled in
    frames[5, 1, 1] = np.inf
    T01 = d["T_true"][0]
    behind = T01.copy()
    behind[2, 3] -= 20.0                             # every point behind the target camera
    aside = T01.copy()
    aside[0, 3] += 500.0                             # every point projects out of bounds
    cases = [(2, 1, T01), (0, 2, T01), (0, 3, T01), (0, 1, behind), (0, 1, aside), (4, 1, T01), (0, 4, T01),
             (5, 1, T01), (0, 5, np.eye(4)), (0, 0, np.eye(4)), (1, 1, T01), (0, 1, T01)]
    src = np.array([c[0] for c in cases], np.int32)
    tgt = np.array([c[1] for c in cases], np.int32)
    return frames, src, tgt, np.stack([c[2] for c in cases])


DIST_THRESHOLD = 0.07
DEPTH_MAX = 3.0
