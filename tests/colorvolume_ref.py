"""numpy float32 restatement of the coloured volume's rule (csrc/vbg_kernels.hpp
k_integrate_color, csrc/extract.hip mc_edge_color, csrc/volumecast.hip trilinear_color).  Test infrastructure:
the product never imports this.

Every operation runs in float32 in the kernels' order (they are built without contraction), so the pins are
bit for bit.  Blocks are held as tsdf / weight (N, R^3) and color (N, R^3, 3), voxels [z][y][x].
"""
import numpy as np

import volumecast_ref as vr

F = np.float32


class ColorVolume:
    """Integrate over a block list with masks, in frame order: ``integrate(touched, ...)`` takes the block keys
    each frame touched (the touch's output: the frames of a block's mask are the frames that list it)."""

    def __init__(self, voxel_size, R):
        self.voxel_size = F(voxel_size)
        self.R = int(R)
        self.index = {}
        self.tsdf = np.zeros((0, self.R ** 3), F)
        self.weight = np.zeros((0, self.R ** 3), F)
        self.color = np.zeros((0, self.R ** 3, 3), F)

    def reset(self):
        self.__init__(self.voxel_size, self.R)

    def keys(self):
        return np.array(list(self.index), np.int32).reshape(-1, 3)

    def _buffers(self, keys):
        """Buffer indices of the keys, allocating (tsdf, weight, colour all 0) the ones not yet held."""
        new = [tuple(int(v) for v in k) for k in keys if tuple(int(v) for v in k) not in self.index]
        for k in new:
            self.index[k] = len(self.index)
        if new:
            n, R3 = len(new), self.R ** 3
            self.tsdf = np.concatenate([self.tsdf, np.zeros((n, R3), F)])
            self.weight = np.concatenate([self.weight, np.zeros((n, R3), F)])
            self.color = np.concatenate([self.color, np.zeros((n, R3, 3), F)])
        return np.array([self.index[tuple(int(v) for v in k)] for k in keys], np.int64)

    def integrate_frame(self, keys, depth, K, T, depth_scale, depth_max, trunc_mult, color=None, K_color=None):
        """One frame over the blocks `keys` (n, 3): the depth test and (tsdf, weight) update of k_integrate
        (SURVEY A.3), and, with `color` (Hc, Wc, 3) uint8 and its intrinsic, the colour update of §2.11.
        Returns the per-voxel (accepted, coloured) masks (n, R^3) for the tests."""
        keys = np.asarray(keys, np.int64).reshape(-1, 3)
        buf = self._buffers(keys)
        R, vs = self.R, self.voxel_size
        depth = np.asarray(depth, F)
        H, W = depth.shape
        fp = vr.frame_params(K, T, F)
        e = fp["ext"]
        a = np.arange(R)
        Z, Y, X = (g.reshape(-1) for g in np.meshgrid(a, a, a, indexing="ij"))
        xs = (keys[:, 0, None] * R + X[None]).astype(F) * vs
        ys = (keys[:, 1, None] * R + Y[None]).astype(F) * vs
        zs = (keys[:, 2, None] * R + Z[None]).astype(F) * vs
        sdf_trunc = vs * F(trunc_mult)
        depth_scale, depth_max = F(depth_scale), F(depth_max)
        with np.errstate(all="ignore"):
            xc = ((xs * e[0, 0] + ys * e[0, 1]) + zs * e[0, 2]) + e[0, 3]
            yc = ((xs * e[1, 0] + ys * e[1, 1]) + zs * e[1, 2]) + e[1, 3]
            zc = ((xs * e[2, 0] + ys * e[2, 1]) + zs * e[2, 2]) + e[2, 3]
            inv_z = F(1) / zc
            u = fp["fx"] * xc * inv_z + fp["cx"]
            v = fp["fy"] * yc * inv_z + fp["cy"]
            inside = (v >= 0) & (u >= 0) & (v <= F(H - 1)) & (u <= F(W - 1))
            ui = np.where(inside, u, 0).astype(np.int64)
            vi = np.where(inside, v, 0).astype(np.int64)
            d = depth[vi, ui] / depth_scale
            sdf = d - zc
            ok = inside & ~((d <= 0) | (d > depth_max) | (zc <= 0) | (sdf < -sdf_trunc))
            sdf = np.where(sdf < sdf_trunc, sdf, sdf_trunc) / sdf_trunc
            wgt = self.weight[buf]
            inv_wsum = F(1) / (wgt + F(1))
            self.tsdf[buf] = np.where(ok, (wgt * self.tsdf[buf] + sdf) * inv_wsum, self.tsdf[buf])
            self.weight[buf] = np.where(ok, wgt + F(1), wgt)
            colored = np.zeros_like(ok)
            if color is not None:
                color = np.asarray(color)
                assert color.dtype == np.uint8 and color.ndim == 3 and color.shape[2] == 3
                Hc, Wc = color.shape[:2]
                Kc = np.asarray(K_color, np.float64).reshape(3, 3)
                fxc, fyc, cxc, cyc = F(Kc[0, 0]), F(Kc[1, 1]), F(Kc[0, 2]), F(Kc[1, 2])
                uc = fxc * xc * inv_z + cxc
                vc = fyc * yc * inv_z + cyc
                colored = ok & (vc >= 0) & (uc >= 0) & (vc <= F(Hc - 1)) & (uc <= F(Wc - 1))
                uci = np.where(colored, uc, 0).astype(np.int64)
                vci = np.where(colored, vc, 0).astype(np.int64)
                px = color[vci, uci].astype(F)  # (n, R^3, 3)
                c = self.color[buf]
                self.color[buf] = np.where(colored[..., None], (wgt[..., None] * c + px) * inv_wsum[..., None], c)
        return ok, colored

    def integrate(self, touched, depths, Kd, T, depth_scale, depth_max, trunc_mult, colors=None, Kc=None):
        """Frames in order; touched[f] = the block keys frame f touched."""
        for f in range(len(depths)):
            self.integrate_frame(touched[f], depths[f], Kd[f], T[f], depth_scale, depth_max, trunc_mult,
                                 None if colors is None else colors[f], None if colors is None else Kc[f])

    def export(self):
        R = self.R
        n = len(self.index)
        return (self.keys(), self.tsdf.reshape(n, R, R, R), self.weight.reshape(n, R, R, R),
                self.color.reshape(n, R, R, R, 3))


def canon(keys, *arrays):
    """Blocks sorted by key (x, then y, then z): (keys, arrays...) in one order for comparisons."""
    keys = np.asarray(keys).reshape(-1, 3)
    o = np.lexsort(keys.T[::-1])
    return (keys[o], *[np.asarray(a)[o] for a in arrays])


def pos_key(pos):
    """A position's three float32 bit patterns as one bytes key."""
    return np.ascontiguousarray(pos, F).tobytes()


def edge_colors(keys, tsdf, weight, color, voxel_size, R, thr):
    """{position bits: colour} over every +x / +y / +z edge o -> e with a sign change (tsdf_o * tsdf_e < 0) and
    both ends present with weight >= thr: the vertex sits at voxel_size * (X_o + ratio e_axis) and takes
    ((1 - ratio) c_o + ratio c_e) / 255, ratio = (0 - tsdf_o) / (tsdf_e - tsdf_o).  Also returns the number of
    edges whose position was already in the map (0 when positions identify edges, which needs tsdf != 0) and the
    set of keys of the edges that cross a block seam (origin voxel on the block's last layer along the edge)."""
    keys = np.asarray(keys, np.int64).reshape(-1, 3)
    n = len(keys)
    vs = F(voxel_size)
    vol = vr.Volume(keys, tsdf, weight, voxel_size, R)
    t = np.asarray(tsdf, F).reshape(n, R, R, R)
    w = np.asarray(weight, F).reshape(n, R, R, R)
    c = np.asarray(color, F).reshape(n, R, R, R, 3)
    assert not (t[w >= thr] == 0).any(), "a tsdf of exactly 0: positions would not identify edges"
    gx, gy, gz = (g.reshape(n, R, R, R) for g in _lattice(keys, R))
    out, dup, seam = {}, 0, set()
    local = np.broadcast_to(np.arange(R), (n, R, R, R))
    for axis in range(3):
        d = [int(axis == 0), int(axis == 1), int(axis == 2)]
        nb = vol.lookup(keys[:, 0] + d[0], keys[:, 1] + d[1], keys[:, 2] + d[2])
        have = nb >= 0
        nbi = np.where(have, nb, 0)
        ax = 3 - axis  # array axis of the lattice axis ([n][z][y][x])
        first = [slice(None)] * 4
        first[ax] = slice(0, 1)
        rest = [slice(None)] * 4
        rest[ax] = slice(1, None)

        def shifted(a, fill):
            edge = np.where(have.reshape((n,) + (1,) * (a.ndim - 1)), a[nbi][tuple(first)], fill)
            return np.concatenate([a[tuple(rest)], edge], axis=ax)

        te, we, ce = shifted(t, F(0)), shifted(w, F(-1)), shifted(c, F(0))
        with np.errstate(all="ignore"):
            m = (w >= thr) & (we >= thr) & (t * te < 0)
            ratio = (F(0) - t[m]) / (te[m] - t[m])
            g = [gx[m], gy[m], gz[m]]
            pos = np.stack([vs * (g[a].astype(F) + (ratio if a == axis else F(0))) for a in range(3)], axis=1)
            col = ((F(1) - ratio)[:, None] * c[m] + ratio[:, None] * ce[m]) / F(255)
            last = np.moveaxis(local, 3, ax)[m] == R - 1  # the origin's local coordinate along the edge
        for p, q, s in zip(pos, col, last):
            k = p.tobytes()
            dup += k in out
            out[k] = q
            if s:
                seam.add(k)
    return out, dup, seam


def _lattice(keys, R):
    a = np.arange(R)
    Z, Y, X = np.meshgrid(a, a, a, indexing="ij")
    return (keys[:, 0, None, None, None] * R + X[None], keys[:, 1, None, None, None] * R + Y[None],
            keys[:, 2, None, None, None] * R + Z[None])


def cast_color(vol, color, vertex, hit):
    """The ray-cast colour at the hit vertices (§2.11): the 8 lattice corners of volumecast_ref.trilinear, its
    fractions, corner order and seam handling; a corner counts when it exists and has w > 0, with
    r = (wx wy) wz; the result is (sum r c / sum r) / 255, 0 when sum r is not > 0 and on a miss.
    vol: volumecast_ref.Volume; color (N, R^3, 3); vertex (..., 3) float32; hit (...) bool."""
    R = vol.R
    voxel = F(vol.voxel_size)
    color = np.asarray(color, F).reshape(len(vol.keys), R ** 3, 3)
    shape = np.shape(hit)
    p = np.asarray(vertex, F).reshape(-1, 3)
    hit = np.asarray(hit, bool).reshape(-1)
    one = F(1)
    with np.errstate(all="ignore"):
        g = [p[:, a] / voxel for a in range(3)]
        g0 = [np.floor(a) for a in g]
        ok = hit.copy()
        for a in g0:
            ok &= np.abs(a) < F(2.0 ** 24)
        fr = [a - b for a, b in zip(g, g0)]
        i0 = [np.where(ok, a, 0).astype(np.int64) for a in g0]
        S = np.zeros(len(p), F)
        acc = np.zeros((len(p), 3), F)
        for k in range(8):
            d = (k & 1, (k >> 1) & 1, k >> 2)
            X = [i0[a] + d[a] for a in range(3)]
            B = [x // R for x in X]
            L = [x - b * R for x, b in zip(X, B)]
            buf = np.where(ok, vol.lookup(*B), -1)
            _, w = vol.voxel(buf, *L)
            use = (buf >= 0) & (w > 0)
            wx, wy, wz = (fr[a] if d[a] else one - fr[a] for a in range(3))
            r = (wx * wy) * wz
            idx = (L[2] * R + L[1]) * R + L[0]
            cc = color[np.where(use, buf, 0), np.where(use, idx, 0)] if len(vol.keys) else np.zeros((len(p), 3), F)
            S = np.where(use, S + r, S)
            acc = np.where(use[:, None], acc + r[:, None] * cc, acc)
        out = np.where((S > 0)[:, None], (acc / S[:, None]) / F(255), F(0)).astype(F)
    return out.reshape(shape + (3,))
