"""numpy float64 restatement of the colour-map optimisation rules.
Test infrastructure: the product never imports this.  Vectorised over whole visibility lists, so it
shares nothing with the kernel's chunks or its reduction order (sums are sequential in list order, or
in reversed order for the order-sensitivity measurement).

Besides the results it reports stability margins over every projection it evaluates: the smallest
distance of u / v from a margin (or validity) bound, from a round() flip (k + 0.5), from an (int) step
(an integer), and the smallest | |d - depth| - threshold | of the visibility test.  An exact comparison
of counts with another implementation is meaningful only while these are far above float64 rounding
(tests/test_colormap_ref.py asserts >= 1e-7 on the inputs the GPU tests use).
"""
import numpy as np

# Open3D RigidOptimizerOption defaults, RGBDImage depth_trunc
OPT = dict(max_depth=2.5, vis_thr=0.03, margin=10, disc_thr=0.1, half=3, depth_trunc=3.0)

# Measured by tests/test_colormap_ref.py::test_order_sensitivity on gpu_test_inputs() (5 iterations from
# the perturbed poses): S_ORDER = the largest element-wise pose difference between summing each keyframe's
# terms in list order and in reversed order, M_MOVE = the smallest per-keyframe pose movement (largest
# element-wise |delta E| of one iteration) among keyframes that moved.  Measured s = 1.7e-14 / 4.8e-14 and
# m = 1.7e-4 / 2.0e-4 on the even / odd set; the constants are the bounds the test holds them to (s from
# above, m from below).  The GPU tolerance is 1000 S_ORDER.
S_ORDER = 2.0e-13
M_MOVE = 1.0e-4


# ------------------------------------------------------------------ images
def _filter3(img, taps, axis):
    """Clamped 3-tap filter: a float32 image of float64 sums of float32 products."""
    img = np.asarray(img, np.float32)
    n = img.shape[axis]
    idx = np.arange(n)
    s = np.zeros(img.shape, np.float64)
    for k in range(3):
        src = np.take(img, np.clip(idx + k - 1, 0, n - 1), axis=axis)
        s = s + (src * np.float32(taps[k])).astype(np.float64)
    return s.astype(np.float32)


def utility_images(rgb):
    """(gray, dx, dy) float32 (N, H, W) of RGB uint8 (N, H, W, 3)."""
    c = np.asarray(rgb, np.uint8).astype(np.float32)
    g0 = (np.float32(0.2990) * c[..., 0] + np.float32(0.5870) * c[..., 1] + np.float32(0.1140) * c[..., 2]) / np.float32(255.0)
    gray = _filter3(_filter3(g0, (0.25, 0.5, 0.25), 2), (0.25, 0.5, 0.25), 1)
    dx = _filter3(_filter3(gray, (-1, 0, 1), 2), (1, 2, 1), 1)
    dy = _filter3(_filter3(gray, (1, 2, 1), 2), (-1, 0, 1), 1)
    return gray, dx, dy


def truncated_depth(t_hit, depth_trunc):
    t = np.asarray(t_hit, np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(t >= np.float32(depth_trunc), np.float32(0), t).astype(np.float32)


def boundary_masks(t_hit, depth_trunc, disc_thr, half):
    """uint8 (N, H, W): 255 within `half` pixels of a depth discontinuity."""
    d = truncated_depth(t_hit, depth_trunc)
    dx = _filter3(_filter3(d, (-1, 0, 1), 2), (1, 2, 1), 1).astype(np.float64)
    dy = _filter3(_filter3(d, (1, 2, 1), 2), (-1, 0, 1), 1).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        m0 = np.sqrt(dx * dx + dy * dy) > disc_thr
    N, H, W = m0.shape
    pad = np.zeros((N, H + 2 * half, W + 2 * half), bool)
    pad[:, half:half + H, half:half + W] = m0
    out = np.zeros_like(m0)
    for a in range(2 * half + 1):
        for b in range(2 * half + 1):
            out |= pad[:, a:a + H, b:b + W]
    return np.where(out, 255, 0).astype(np.uint8)


# ------------------------------------------------------------------ projections
def _round_half_away(x):
    x = np.asarray(x, np.float64)
    return np.sign(x) * np.floor(np.abs(x) + 0.5)


def _camera(E, V):
    X, Y, Z = (V[:, a].astype(np.float64) for a in range(3))
    g = [E[r, 0] * X + E[r, 1] * Y + E[r, 2] * Z + E[r, 3] for r in range(3)]
    return g[0], g[1], g[2]


def _project(E, K, V):
    gx, gy, gz = _camera(E, V)
    with np.errstate(all="ignore"):
        u = (gx * K[0, 0]) / gz + K[0, 2]
        v = (gy * K[1, 1]) / gz + K[1, 2]
    return gx, gy, gz, u, v


def _f32_threshold(b):
    """The float64 value at which float32(x) >= b starts to hold for a float32-representable b > 0: half a
    float32 step below b (round to nearest)."""
    b32 = np.asarray(b, np.float32)
    below = np.nextafter(b32, np.float32(-np.inf)).astype(np.float64)
    return (b32.astype(np.float64) + below) / 2.0


class Margins:
    """The smallest stability margins seen so far (inf: the test was never reached)."""

    def __init__(self):
        self.bound = self.round = self.int = self.vis = np.inf

    def _min(self, name, a):
        a = np.asarray(a, np.float64)
        a = a[np.isfinite(a)]
        if a.size:
            setattr(self, name, min(getattr(self, name), float(np.abs(a).min())))

    def bounds(self, u, v, H, W, margin, validity=False, f32=False):
        """u, v float64.  f32: the test runs on float32(u): it flips where u crosses _f32_threshold(bound)."""
        t = _f32_threshold if f32 else (lambda b: np.float64(b))
        for w, n in ((u, W), (v, H)):
            self._min("bound", w - t(margin))
            self._min("bound", w - t(n - margin))
            if validity:
                self._min("bound", w)
                self._min("bound", w - (n - 1))

    def rounds(self, u, v):
        """u, v float64 whose float32 value is rounded half away from zero: roundf(float32(u)) flips where
        |u| crosses _f32_threshold(k + 0.5)."""
        for w in (u, v):
            w = np.abs(np.asarray(w, np.float64))
            w = w[np.isfinite(w) & (w < 1e6)]
            self._min("round", w - _f32_threshold(np.floor(w) + 0.5))

    def ints(self, u, v):
        for w in (u, v):
            w = np.asarray(w, np.float64)
            self._min("int", w - np.round(w))

    def as_dict(self):
        return dict(bound=self.bound, round=self.round, int=self.int, vis=self.vis)

    def smallest(self):
        return min(self.as_dict().values())


def _in_margin(u, v, H, W, margin):
    with np.errstate(invalid="ignore"):
        return (u >= margin) & (u < W - margin) & (v >= margin) & (v < H - margin)


def _float_uv(E, K, V):
    """float32 (u, v, d) and the float64 (u, v) they were rounded from."""
    _, _, gz, u, v = _project(E, K, V)
    with np.errstate(all="ignore"):
        return u.astype(np.float32), v.astype(np.float32), gz.astype(np.float32), u, v


def _nearest(u, v, H, W):
    """(ok, ui, vi) of float32 u, v: the rounded pixel where it lies inside the image."""
    ru, rv = _round_half_away(u), _round_half_away(v)
    with np.errstate(invalid="ignore"):
        ok = (ru >= 0) & (ru < W) & (rv >= 0) & (rv < H)
    ui = np.where(ok, ru, 0).astype(np.int64)
    vi = np.where(ok, rv, 0).astype(np.int64)
    return ok, ui, vi


class Reference:
    """State of the optimiser: utility images, masks, visibility lists (at the initial poses), poses."""

    def __init__(self, V, images, t_hit, K, T_wc, opt=None):
        o = dict(OPT)
        o.update(opt or {})
        self.o = o
        self.V = np.ascontiguousarray(V, np.float32).reshape(-1, 3)
        self.images = np.ascontiguousarray(images, np.uint8)
        self.N, self.H, self.W = self.images.shape[:3]
        self.K = np.asarray(K, np.float64).reshape(self.N, 3, 3)
        self.E = np.asarray(T_wc, np.float64).reshape(self.N, 4, 4).copy()
        self.E0 = self.E.copy()
        self.gray, self.dx, self.dy = utility_images(self.images) if self.N else (np.zeros((0, self.H, self.W), np.float32),) * 3
        self.depth = truncated_depth(np.asarray(t_hit, np.float32).reshape(self.N, self.H, self.W), o["depth_trunc"])
        self.mask = boundary_masks(np.asarray(t_hit, np.float32).reshape(self.N, self.H, self.W), o["depth_trunc"],
                                   o["disc_thr"], o["half"])
        self.margins = Margins()  # of the visibility pass
        self.lists = [self._visible(c) for c in range(self.N)]  # image -> vertex, ascending
        self.proxy = self.compute_proxy(self.margins)

    def _visible(self, c):
        H, W, o = self.H, self.W, self.o
        u, v, d, u64, v64 = _float_uv(self.E[c], self.K[c], self.V)
        ok, ui, vi = _nearest(u, v, H, W)
        with np.errstate(invalid="ignore"):
            ok &= d >= 0
        self.margins.rounds(u64[ok], v64[ok])
        ds = self.depth[c][vi, ui]
        with np.errstate(invalid="ignore"):
            ok &= ~(ds > o["max_depth"])
            ok &= self.mask[c][vi, ui] != 255
            diff = np.abs(d - ds).astype(np.float32).astype(np.float64)  # float difference, compared in float64
            self.margins._min("vis", (diff - o["vis_thr"])[ok])
            ok &= diff < o["vis_thr"]
        return np.nonzero(ok)[0]

    @property
    def pairs_per_keyframe(self):
        return np.array([len(l) for l in self.lists], np.int64)

    def compute_proxy(self, mg=None):
        nv = len(self.V)
        s, n = np.zeros(nv), np.zeros(nv, np.int64)
        for c in range(self.N):  # keyframe order
            ids = self.lists[c]
            u, v, _, u64, v64 = _float_uv(self.E[c], self.K[c], self.V[ids])
            ok, ui, vi = _nearest(u, v, self.H, self.W)
            ok &= _in_margin(u, v, self.H, self.W, self.o["margin"])
            if mg is not None:
                mg.bounds(u64, v64, self.H, self.W, self.o["margin"], f32=True)
                mg.rounds(u64, v64)
            s[ids[ok]] = s[ids[ok]] + self.gray[c][vi[ok], ui[ok]].astype(np.float64)
            n[ids[ok]] += 1
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(n > 0, s / np.maximum(n, 1), 0.0)

    def terms(self, c, mg=None):
        """(n, 29) float64 terms of keyframe c in list order (skipped terms are absent)."""
        H, W, m = self.H, self.W, self.o["margin"]
        ids = self.lists[c]
        K = self.K[c]
        gx, gy, gz, u, v = _project(self.E[c], K, self.V[ids])
        if mg is not None:
            mg.bounds(u, v, H, W, m, validity=True)
            mg.ints(u, v)
        with np.errstate(invalid="ignore"):
            ok = _in_margin(u, v, H, W, m) & (u >= 0) & (u <= W - 1) & (v >= 0) & (v <= H - 1)
        gx, gy, gz, u, v, ids = gx[ok], gy[ok], gz[ok], u[ok], v[ok], ids[ok]
        ui = np.clip(u.astype(np.int64), 0, W - 2)
        vi = np.clip(v.astype(np.int64), 0, H - 2)
        pu, pv = u - ui, v - vi

        def lerp(img):
            a00, a01 = img[vi, ui].astype(np.float64), img[vi + 1, ui].astype(np.float64)
            a10, a11 = img[vi, ui + 1].astype(np.float64), img[vi + 1, ui + 1].astype(np.float64)
            return (a00 * (1.0 - pv) + a01 * pv) * (1.0 - pu) + (a10 * (1.0 - pv) + a11 * pv) * pu

        gray, dIdx, dIdy = lerp(self.gray[c]), lerp(self.dx[c]), lerp(self.dy[c])
        invz = 1.0 / gz
        v0, v1 = dIdx * K[0, 0] * invz, dIdy * K[1, 1] * invz
        v2 = -(v0 * gx + v1 * gy) * invz
        J = [-gz * v1 + gy * v2, gz * v0 - gx * v2, -gy * v0 + gx * v1, v0, v1, v2]
        r = gray - self.proxy[ids]
        cols = [np.ones_like(r), r * r] + [J[a] * r for a in range(6)]
        cols += [J[a] * J[b] for a in range(6) for b in range(a, 6)]
        return np.stack(cols, 1) if len(r) else np.zeros((0, 29))

    def system(self, c, order="forward", mg=None):
        """(JTJ (6,6), JTr (6,), r2, count) of keyframe c; sums sequential in list (or reversed) order."""
        t = self.terms(c, mg)
        if order == "reversed":
            t = t[::-1]
        S = np.cumsum(t, axis=0)[-1] if len(t) else np.zeros(29)
        JTJ = np.zeros((6, 6))
        k = 8
        for a in range(6):
            for b in range(a, 6):
                JTJ[a, b] = JTJ[b, a] = S[k]
                k += 1
        return JTJ, S[2:8].copy(), float(S[1]), int(S[0])

    def systems(self, order="forward", mg=None):
        out = [self.system(c, order, mg) for c in range(self.N)]
        return (np.stack([o[0] for o in out]) if out else np.zeros((0, 6, 6)),
                np.stack([o[1] for o in out]) if out else np.zeros((0, 6)),
                np.array([o[2] for o in out]), np.array([o[3] for o in out], np.int64))

    def iterate(self, order="forward"):
        """One iteration -> (residual, count, margins dict, moved (N,) bool, movement (N,))."""
        mg = Margins()
        JTJ, JTr, r2, cnt = self.systems(order, mg)
        moved = np.zeros(self.N, bool)
        move = np.zeros(self.N)
        for c in range(self.N):
            if cnt[c] < 6:
                continue
            x = ldlt_solve(JTJ[c], -JTr[c])
            if x is None:
                continue
            new = apply_delta(x, self.E[c])
            move[c] = np.abs(new - self.E[c]).max()
            moved[c] = True
            self.E[c] = new
        self.proxy = self.compute_proxy(mg)
        residual = 0.0
        for c in range(self.N):
            residual += r2[c]
        return residual, int(cnt.sum()), mg.as_dict(), moved, move

    def optimize(self, n, order="forward"):
        """n iterations -> (residuals (n,), counts (n,), margins per iteration, moved (n, N), movement (n, N))."""
        out = [self.iterate(order) for _ in range(n)]
        return (np.array([o[0] for o in out]), np.array([o[1] for o in out], np.int64), [o[2] for o in out],
                np.array([o[3] for o in out]).reshape(n, self.N), np.array([o[4] for o in out]).reshape(n, self.N))

    def mean_colors(self):
        """(float64 mean colours (V, 3), counts (V,) int32) over the visibility pairs at the current poses
        (no fill of the unsampled vertices)."""
        nv = len(self.V)
        s, n = np.zeros((nv, 3)), np.zeros(nv, np.int32)
        for c in range(self.N):
            ids = self.lists[c]
            u, v, _, _, _ = _float_uv(self.E[c], self.K[c], self.V[ids])
            ok, ui, vi = _nearest(u, v, self.H, self.W)
            ok &= _in_margin(u, v, self.H, self.W, self.o["margin"])
            px = self.images[c][vi[ok], ui[ok]].astype(np.float32) / np.float32(255.0)
            s[ids[ok]] = s[ids[ok]] + px.astype(np.float64)
            n[ids[ok]] += 1
        return np.where(n[:, None] > 0, s / np.maximum(n, 1)[:, None], 0.0), n


def ldlt_solve(A, b):
    """x of A x = b by LDL^T, or None when a pivot is non-positive or non-finite or x is non-finite."""
    L, D = np.zeros((6, 6)), np.zeros(6)
    ok = True
    with np.errstate(all="ignore"):
        for j in range(6):
            d = A[j, j]
            for k in range(j):
                d -= L[j, k] * L[j, k] * D[k]
            D[j] = d
            if not (d > 0.0 and np.isfinite(d)):
                ok = False
            for i in range(j + 1, 6):
                s = A[i, j]
                for k in range(j):
                    s -= L[i, k] * L[j, k] * D[k]
                L[i, j] = s / d
        if not ok:
            return None
        x = np.zeros(6)
        for i in range(6):
            s = b[i]
            for k in range(i):
                s -= L[i, k] * x[k]
            x[i] = s
        x = x / D
        for i in range(5, -1, -1):
            s = x[i]
            for k in range(i + 1, 6):
                s -= L[k, i] * x[k]
            x[i] = s
    return x if np.isfinite(x).all() else None


def delta_rotation(x):
    """Rz(x2) Ry(x1) Rx(x0)."""
    sa, ca, sb, cb, sg, cg = np.sin(x[0]), np.cos(x[0]), np.sin(x[1]), np.cos(x[1]), np.sin(x[2]), np.cos(x[2])
    return np.array([[cg * cb, cg * sb * sa - sg * ca, cg * sb * ca + sg * sa],
                     [sg * cb, sg * sb * sa + cg * ca, sg * sb * ca - cg * sa],
                     [-sb, cb * sa, cb * ca]])


def apply_delta(x, E):
    R = delta_rotation(x)
    out = E.copy()
    for r in range(3):
        for k in range(4):
            s = (R[r, 0] * E[0, k] + R[r, 1] * E[1, k]) + R[r, 2] * E[2, k]
            if k == 3:
                s += x[3 + r]
            out[r, k] = s
    return out


def pose_error(ref, E, E_true):
    """Mean over the keyframes that have visibility pairs of the mean distance, in pixels, between the
    projections of the keyframe's visible vertices under E[c] and under E_true[c]: the pose error as the
    images see it.  (Element-wise matrix differences do not rank poses the way the optimiser does: a
    rotation and a translation error that cancel in the image are invisible to it.)"""
    out = []
    for c in range(ref.N):
        ids = ref.lists[c]
        if len(ids) == 0:
            continue
        _, _, _, u, v = _project(np.asarray(E)[c], ref.K[c], ref.V[ids])
        _, _, _, ut, vt = _project(np.asarray(E_true)[c], ref.K[c], ref.V[ids])
        out.append(np.hypot(u - ut, v - vt).mean())
    return float(np.mean(out)) if out else 0.0


def converged(ref0, T_start, T_end, T_true, residuals):
    """The convergence condition (shared with the GPU test): the residual of the last iteration is
    strictly below the first's, and the mean pose error against the true poses is lower than at the start."""
    return bool(residuals[-1] < residuals[0]) and pose_error(ref0, T_end, T_true) < pose_error(ref0, T_start, T_true)


def perturbed_set(T_true, seed, trans=0.004, rot=0.004):
    """The keyframe poses moved by one seeded small rigid motion (a few millimetres / milliradians,
    applied on the left) with alternating sign.  The optimiser pulls every pose towards the consensus
    of the keyframes that see the same vertices, not towards the truth; perturbations that cancel
    between neighbours put that consensus at the truth, so a working optimiser must lower the pose
    error.  (Independent perturbations leave their mean as a bias the images cannot see.)"""
    rng = np.random.default_rng(seed)
    x = np.concatenate([rng.uniform(-rot, rot, 3), rng.uniform(-trans, trans, 3)])
    return np.stack([apply_delta(x if i % 2 == 0 else -x, np.asarray(T, np.float64)) for i, T in enumerate(T_true)])


# ------------------------------------------------------------------ inputs of the GPU tests
F = 100.0
PATCH = (40, 64, 50, 76)  # rows y0:y1, columns x0:x1 where the patch keyframe's ray cast hits

_inputs = None


def gpu_test_inputs():
    """The inputs of tests/test_gpu_colormap.py, built once on the CPU from mqr.synthetic: per set 6
    keyframes of the room (96 x 128, and one rendered at 100 x 136 and cropped to 97 x 131; K is the
    uncropped one, a crop at the origin), their colour images and noise-free depth as t_hit, vertices =
    the back-projected depth pixels (stride 3) of three frames between the keyframes, the true poses and
    seeded perturbed ones.  Keyframes 0-3 look across the room (hundreds to thousands of pairs), 4 has
    ray-cast hits only in a small patch (1..63 pairs), 5 looks the other way (0 pairs)."""
    global _inputs
    if _inputs is not None:
        return _inputs
    from mqr import synthetic
    P = synthetic.room_loop_poses(192)
    flip = np.diag([-1.0, 1.0, -1.0])
    key = [P[0], P[2], P[4], P[6], P[8], (P[2][0] @ flip, P[2][1])]
    src = [P[1], P[3], P[5]]
    out = {}
    for name, (h, w, ch, cw, seed) in {"even": (96, 128, 96, 128, 11), "odd": (100, 136, 97, 131, 12)}.items():
        K = np.array([[F, 0, (w - 1) / 2.0], [0, F, (h - 1) / 2.0], [0, 0, 1.0]])
        sc = synthetic.SCENES["room"]
        images = np.stack([synthetic.render_color("room", K, R, t, h, w)[:ch, :cw] for R, t in key])
        t_hit = np.stack([synthetic.render_depth(sc, K, R, t, h, w)[:ch, :cw] for R, t in key])
        y0, y1, x0, x1 = PATCH
        patch = np.full_like(t_hit[4], np.inf)
        patch[y0:y1, x0:x1] = t_hit[4][y0:y1, x0:x1]
        t_hit[4] = patch
        verts = []
        for R, t in src:
            z = synthetic.render_depth(sc, K, R, t, h, w).astype(np.float64)[:ch:3, :cw:3]
            v, u = np.mgrid[0:ch:3, 0:cw:3]
            dc = np.stack([(u - K[0, 2]) / F, (v - K[1, 2]) / F, np.ones_like(z)], -1)
            pw = (dc * z[..., None]) @ np.asarray(R).T + np.asarray(t)
            verts.append(pw[z > 0])
        V = np.concatenate(verts).astype(np.float32)
        T_true = np.zeros((len(key), 4, 4))
        for i, (R, t) in enumerate(key):  # world -> camera of a camera -> world rotation R and eye t
            T_true[i, :3, :3] = np.asarray(R).T
            T_true[i, :3, 3] = -np.asarray(R).T @ np.asarray(t)
            T_true[i, 3, 3] = 1.0
        T_pert = perturbed_set(T_true, seed)
        out[name] = dict(V=np.ascontiguousarray(V), images=np.ascontiguousarray(images),
                         t_hit=np.ascontiguousarray(t_hit), K=np.repeat(K[None], len(key), 0), T_true=T_true,
                         T_pert=T_pert)
    _inputs = out
    return out


_runs = {}


def reference_run(name, n, order="forward"):
    """The reference optimisation of gpu_test_inputs()[name] from the perturbed poses, n iterations,
    computed once per process and shared (callers must not modify it):
    dict(ref=the Reference after the run, residuals, counts, margins, moved, movement, init=the systems,
    proxies, pair counts and visibility margins before the first iteration)."""
    key = (name, n, order)
    if key not in _runs:
        d = gpu_test_inputs()[name]
        ref = Reference(d["V"], d["images"], d["t_hit"], d["K"], d["T_pert"])
        mg = Margins()
        init = dict(systems=ref.systems(mg=mg), proxy=ref.proxy.copy(), pairs=ref.pairs_per_keyframe,
                    margins=dict(ref.margins.as_dict()), system_margins=mg.as_dict())
        res, cnt, margins, moved, move = ref.optimize(n, order)
        _runs[key] = dict(ref=ref, residuals=res, counts=cnt, margins=margins, moved=moved, movement=move, init=init)
    return _runs[key]
