"""numpy restatement of the volume ray-cast rule (csrc/volumecast.hip), vectorised over
pixels with masks.  Test infrastructure: the product never imports this.

``ft`` is the numpy float type every operation of the rule runs in: ``np.float32`` repeats the kernels'
operations in their order and is the bit-for-bit pin; ``np.float64`` (parameters not rounded to float32
either) is the accuracy yardstick.  The volume is given as exported arrays: keys (N, 3) int32, tsdf and
weight (N, R, R, R) float32 indexed [z][y][x].
"""
import numpy as np

K_BIAS = 1 << 20
MAX_STEPS = 2048  # csrc/volumecast.hip kMaxSteps


class Volume:
    def __init__(self, keys, tsdf, weight, voxel_size, R):
        self.keys = np.asarray(keys, np.int64).reshape(-1, 3)
        self.R = int(R)
        n = len(self.keys)
        self.tsdf = np.asarray(tsdf, np.float32).reshape(n, self.R ** 3)
        self.weight = np.asarray(weight, np.float32).reshape(n, self.R ** 3)
        self.voxel_size = voxel_size
        packed = self._pack(self.keys[:, 0], self.keys[:, 1], self.keys[:, 2])
        self._order = np.argsort(packed, kind="stable")
        self._sorted = packed[self._order]

    @staticmethod
    def _pack(x, y, z):
        return ((x + K_BIAS) << 42) | ((y + K_BIAS) << 21) | (z + K_BIAS)

    def lookup(self, x, y, z):
        """Buffer index of each block (x, y, z) (int64 arrays), -1 where absent or out of the key range."""
        x, y, z = (np.asarray(a, np.int64) for a in (x, y, z))
        ok = np.ones(x.shape, bool)
        for a in (x, y, z):
            ok &= (a >= -K_BIAS) & (a < K_BIAS)
        out = np.full(x.shape, -1, np.int64)
        if len(self._sorted) == 0 or not ok.any():
            return out
        p = self._pack(np.where(ok, x, 0), np.where(ok, y, 0), np.where(ok, z, 0))
        i = np.minimum(np.searchsorted(self._sorted, p), len(self._sorted) - 1)
        found = ok & (self._sorted[i] == p)
        out[found] = self._order[i[found]]
        return out

    def voxel(self, buf, lx, ly, lz):
        """(tsdf, weight) float32 of voxel (lx, ly, lz) of buffer buf (0 where buf < 0)."""
        idx = (lz * self.R + ly) * self.R + lx
        b = np.where(buf >= 0, buf, 0)
        i = np.where(buf >= 0, idx, 0)
        if len(self.keys) == 0:
            z = np.zeros(np.shape(buf), np.float32)
            return z, z.copy()
        return self.tsdf[b, i], self.weight[b, i]


def _par(x, ft):
    """A float parameter as the C ABI passes it (float32), in the working type."""
    return ft(x) if ft is np.float64 else ft(np.float32(x))


def frame_params(K, T, ft):
    """make_frame_params (csrc/vbg.hip): float32 K and extrinsic, float32 of the float64 rigid inverse."""
    K = np.asarray(K, np.float64).reshape(3, 3)
    T = np.asarray(T, np.float64).reshape(4, 4)
    fx, fy, cx, cy = (ft(K[0, 0]), ft(K[1, 1]), ft(K[0, 2]) + ft(0), ft(K[1, 2]) + ft(0))  # (-0 -> +0)
    ext = T[:3, :].astype(ft)
    P = np.zeros((3, 4))
    P[:, :3] = T[:3, :3].T
    for i in range(3):
        P[i, 3] = -((P[i, 0] * T[0, 3] + P[i, 1] * T[1, 3]) + P[i, 2] * T[2, 3])
    return dict(fx=fx, fy=fy, cx=cx, cy=cy, ext=ext, pose=P.astype(ft))


def range_map(vol, block_keys, fps, H, W, df, dmin, dmax, ft):
    """(rmin, rmax) (n, Hc, Wc) and the whole-map ranges (gmin, gmax) (n,) of k_cast_range."""
    n = len(fps)
    Hc, Wc = -(-H // df), -(-W // df)
    rmin = np.full((n, Hc, Wc), np.inf, ft)
    rmax = np.zeros((n, Hc, Wc), ft)
    gmin = np.full(n, np.inf, ft)
    gmax = np.zeros(n, ft)
    if block_keys is None:
        keys = vol.keys
    else:
        keys = np.asarray(block_keys, np.int64).reshape(-1, 3)
        keys = keys[vol.lookup(keys[:, 0], keys[:, 1], keys[:, 2]) >= 0]
    if len(keys) == 0 or len(vol.keys) == 0:
        return rmin, rmax, gmin, gmax
    voxel = _par(vol.voxel_size, ft)
    c = np.arange(8)
    corner = np.stack([c & 1, (c >> 1) & 1, c >> 2], axis=1)  # (8, 3)
    ws = ((keys[:, None, :] + corner[None]) * vol.R).astype(ft) * voxel  # (B, 8, 3)
    xs, ys, zs = ws[..., 0], ws[..., 1], ws[..., 2]
    inf = ft(np.inf)
    with np.errstate(all="ignore"):
        for f, fp in enumerate(fps):
            e = fp["ext"]
            xc = xs * e[0, 0] + ys * e[0, 1] + zs * e[0, 2] + e[0, 3]
            yc = xs * e[1, 0] + ys * e[1, 1] + zs * e[1, 2] + e[1, 3]
            zc = xs * e[2, 0] + ys * e[2, 1] + zs * e[2, 2] + e[2, 3]
            front = zc > 0
            behind = 8 - front.sum(axis=1)
            pu = fp["fx"] * xc / zc + fp["cx"]
            pv = fp["fy"] * yc / zc + fp["cy"]
            zlo = np.fmin(np.fmin.reduce(zc, axis=1), inf)
            zhi = np.fmax(np.fmax.reduce(zc, axis=1), -inf)
            zlo = np.fmin(np.fmax(zlo, dmin), dmax)
            zhi = np.fmin(np.fmax(zhi, dmin), dmax)
            zlo = np.where(behind > 0, dmin, zlo)
            live = (behind < 8) & (zlo < zhi)
            for b in np.nonzero(live)[0]:
                if behind[b]:
                    gmin[f] = min(gmin[f], zlo[b])
                    gmax[f] = max(gmax[f], zhi[b])
                    continue
                ulo = np.fmin(np.fmin.reduce(pu[b]), inf)
                uhi = np.fmax(np.fmax.reduce(pu[b]), -inf)
                vlo = np.fmin(np.fmin.reduce(pv[b]), inf)
                vhi = np.fmax(np.fmax.reduce(pv[b]), -inf)
                x0 = np.fmax(np.floor(ulo) - ft(1), ft(0))
                x1 = np.fmin(np.floor(uhi) + ft(1), ft(W - 1))
                y0 = np.fmax(np.floor(vlo) - ft(1), ft(0))
                y1 = np.fmin(np.floor(vhi) + ft(1), ft(H - 1))
                if not (x0 <= x1 and y0 <= y1):
                    continue
                cx0, cx1, cy0, cy1 = int(x0) // df, int(x1) // df, int(y0) // df, int(y1) // df
                rmin[f, cy0:cy1 + 1, cx0:cx1 + 1] = np.minimum(rmin[f, cy0:cy1 + 1, cx0:cx1 + 1], zlo[b])
                rmax[f, cy0:cy1 + 1, cx0:cx1 + 1] = np.maximum(rmax[f, cy0:cy1 + 1, cx0:cx1 + 1], zhi[b])
    return rmin, rmax, gmin, gmax


def trilinear(vol, px, py, pz, wthr, ft):
    """(value, usable) of the trilinear tsdf at the world points: 8 lattice corners in order dx + 2 dy + 4 dz."""
    voxel = _par(vol.voxel_size, ft)
    R = vol.R
    one = ft(1)
    g = [px / voxel, py / voxel, pz / voxel]
    g0 = [np.floor(a) for a in g]
    ok = np.ones(px.shape, bool)
    for a in g0:
        ok &= np.abs(a) < ft(2.0 ** 24)  # (a NaN fails)
    fr = [a - b for a, b in zip(g, g0)]
    i0 = [np.where(ok, a, 0).astype(np.int64) for a in g0]
    total = np.zeros(px.shape, ft)
    for k in range(8):
        d = (k & 1, (k >> 1) & 1, k >> 2)
        X = [i0[a] + d[a] for a in range(3)]
        B = [x // R for x in X]
        L = [x - b * R for x, b in zip(X, B)]
        buf = vol.lookup(*B)
        buf = np.where(ok, buf, -1)
        t, w = vol.voxel(buf, *L)
        ok = ok & (buf >= 0) & (w.astype(ft) >= wthr)
        wx, wy, wz = (fr[a] if d[a] else one - fr[a] for a in range(3))
        total = total + ((wx * wy) * wz) * t.astype(ft)
    return total, ok


def ray_cast(vol, block_keys, K, T, H, W, depth_scale=1000.0, depth_min=0.1, depth_max=3.0, weight_threshold=3.0,
             trunc_voxel_multiplier=8.0, range_map_down_factor=8, pixel_offset=0.0, refine=False, ft=np.float32,
             max_steps=MAX_STEPS):
    """The rule for n frames (K (n,3,3), T (n,4,4) world -> camera).  Returns a dict: depth (n,H,W), vertex and
    normal (n,H,W,3), range_min / range_max (n,Hc,Wc) with the whole-map ranges folded in, and for the tests
    hit, refined (the crossing was recomputed from the trilinear samples) and steps (march steps taken)."""
    K = np.asarray(K, np.float64).reshape(-1, 3, 3)
    T = np.asarray(T, np.float64).reshape(-1, 4, 4)
    n = len(K)
    df = int(range_map_down_factor)
    fps = [frame_params(K[f], T[f], ft) for f in range(n)]
    voxel = _par(vol.voxel_size, ft)
    R = vol.R
    bs = voxel * ft(R)
    dmin, dmax, wthr, off, dscale = (_par(a, ft) for a in (depth_min, depth_max, weight_threshold, pixel_offset,
                                                           depth_scale))
    trunc = voxel * _par(trunc_voxel_multiplier, ft)
    rmin, rmax, gmin, gmax = range_map(vol, block_keys, fps, H, W, df, dmin, dmax, ft)
    rmin = np.fmin(rmin, gmin[:, None, None])
    rmax = np.fmax(rmax, gmax[:, None, None])
    out = dict(depth=np.zeros((n, H, W), ft), vertex=np.zeros((n, H, W, 3), ft), normal=np.zeros((n, H, W, 3), ft),
               range_min=rmin, range_max=rmax, hit=np.zeros((n, H, W), bool), refined=np.zeros((n, H, W), bool),
               steps=np.zeros((n, H, W), np.int64))
    lim = ft(K_BIAS)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    yy, xx = yy.reshape(-1), xx.reshape(-1)
    with np.errstate(all="ignore"):
        for f, fp in enumerate(fps):
            P = fp["pose"]
            xc = ((xx.astype(ft) + off) - fp["cx"]) / fp["fx"]
            yc = ((yy.astype(ft) + off) - fp["cy"]) / fp["fy"]
            o = [P[0, 3], P[1, 3], P[2, 3]]
            d = [(xc * P[a, 0] + yc * P[a, 1] + P[a, 2] + P[a, 3]) - o[a] for a in range(3)]
            zmin = rmin[f][yy // df, xx // df]
            zmax = rmax[f][yy // df, xx // df]
            N = H * W
            t = zmin.copy()
            t_prev = zmin.copy()
            tp = np.full(N, -1, ft)
            ts_ = np.full(N, 1, ft)
            p = [np.zeros(N, ft) for _ in range(3)]
            hit = np.zeros(N, bool)
            steps = np.zeros(N, np.int64)
            active = zmin < zmax
            for _ in range(max_steps):
                idx = np.nonzero(active)[0]
                if len(idx) == 0:
                    break
                steps[idx] += 1
                ta = t[idx]
                pa = [o[a] + ta * d[a][idx] for a in range(3)]
                for a in range(3):
                    p[a][idx] = pa[a]
                bf = [np.floor(q / bs) for q in pa]
                inr = np.ones(len(idx), bool)
                for q in bf:
                    inr &= (q >= -lim) & (q < lim)
                bi = [np.where(inr, q, 0).astype(np.int64) for q in bf]
                buf = np.where(inr, vol.lookup(*bi), -1)
                absent = buf < 0
                rm1 = ft(R - 1)
                vi = [np.where(absent, 0, np.fmin(np.fmax(np.floor((pa[a] - bf[a] * bs) / voxel), ft(0)), rm1))
                      .astype(np.int64) for a in range(3)]
                tv, wv = vol.voxel(buf, *vi)
                tv, wv = tv.astype(ft), wv.astype(ft)
                cur = np.where(absent, ts_[idx], tv)
                h = ~absent & (tp[idx] > 0) & (wv >= wthr) & (cur <= 0)
                ts_[idx] = cur
                hit[idx[h]] = True
                go = ~h
                gi = idx[go]
                tp[gi] = cur[go]
                ab = absent[go]
                t_prev[gi] = np.where(ab, t_prev[gi], ta[go])
                t[gi] = np.where(ab, ta[go] + bs, ta[go] + np.fmax(cur[go] * trunc, voxel))
                active[idx[h]] = False
                active[gi] = t[gi] < zmax[gi]
            tstar = np.zeros(N, ft)
            hi = np.nonzero(hit)[0]
            refined = np.zeros(N, bool)
            if len(hi):
                th, tph, a0, b0 = t[hi], t_prev[hi], tp[hi], ts_[hi]
                tsr = (th * a0 - tph * b0) / (a0 - b0)
                if refine:
                    a, oka = trilinear(vol, *[o[k] + tph * d[k][hi] for k in range(3)], wthr, ft)
                    b, okb = trilinear(vol, *[p[k][hi] for k in range(3)], wthr, ft)
                    use = oka & okb & (a > 0) & (b <= 0)
                    tsr = np.where(use, (th * a - tph * b) / (a - b), tsr)
                    refined[hi] = use
                tstar[hi] = tsr
                hp = [o[k] + tsr * d[k][hi] for k in range(3)]
                s, ok = [], np.ones(len(hi), bool)
                for k in range(6):
                    e = -voxel if k & 1 else voxel
                    q = [hp[a] + e if a == k >> 1 else hp[a] for a in range(3)]
                    val, u = trilinear(vol, *q, wthr, ft)
                    s.append(val)
                    ok &= u
                nx, ny, nz = s[0] - s[1], s[2] - s[3], s[4] - s[5]
                norm = (np.sqrt(nx * nx + ny * ny + nz * nz).astype(np.float64) + 1e-5).astype(ft)
                nrm = np.stack([np.where(ok, c / norm, ft(0)) for c in (nx, ny, nz)], axis=1)
                out["depth"][f].reshape(-1)[hi] = tsr * dscale
                out["vertex"][f].reshape(-1, 3)[hi] = np.stack(hp, axis=1)
                out["normal"][f].reshape(-1, 3)[hi] = nrm
            out["hit"][f] = hit.reshape(H, W)
            out["refined"][f] = refined.reshape(H, W)
            out["steps"][f] = steps.reshape(H, W)
    return out
