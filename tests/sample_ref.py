"""Numpy restatement of the surface-sampling rule of csrc/meshsample.hip, operation for
operation, so that the kernel and this file agree bit for bit.  Test infrastructure: the product never
imports this.

Every floating-point step is float64 on the float32 inputs; numpy rounds each product and sum on its own
(no contraction), float64 sqrt and division are correctly rounded.  The selection is integer arithmetic.
"""
import numpy as np

GOLDEN = 0x9E3779B97F4A7C15
_M1 = np.uint64(0xBF58476D1CE4E5B9)
_M2 = np.uint64(0x94D049BB133111EB)
_LO32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def splitmix64(seed: int, k):
    """Output number ``k`` (1-based, array or int) of SplitMix64 seeded with ``seed``, as uint64."""
    k = np.asarray(k, np.uint64)
    with np.errstate(over="ignore"):
        z = np.uint64(int(seed) & (2 ** 64 - 1)) + k * np.uint64(GOLDEN)
        z = (z ^ (z >> np.uint64(30))) * _M1
        z = (z ^ (z >> np.uint64(27))) * _M2
        return z ^ (z >> np.uint64(31))


def mulhi64(a, b):
    """The high 64 bits of the 128-bit product of uint64 arrays, by 32-bit halves."""
    a, b = np.asarray(a, np.uint64), np.asarray(b, np.uint64)
    a0, a1, b0, b1 = a & _LO32, a >> _S32, b & _LO32, b >> _S32
    with np.errstate(over="ignore"):  # no partial sum below overflows: each is < 2^64 by construction
        p00, p01, p10, p11 = a0 * b0, a0 * b1, a1 * b0, a1 * b1
        mid = (p00 >> _S32) + (p01 & _LO32) + (p10 & _LO32)  # < 3 * 2^32
        return p11 + (p01 >> _S32) + (p10 >> _S32) + (mid >> _S32)


def cross(vertices, triangles):
    """(b - a) x (c - a) per triangle in float64, each product rounded on its own: (nt, 3)."""
    v = np.asarray(vertices, np.float32).astype(np.float64)
    t = np.asarray(triangles).reshape(-1, 3)
    a, b, c = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    u, w = b - a, c - a
    x = u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1]
    y = u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2]
    z = u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]
    return np.stack([x, y, z], 1)


def norm3(n):
    return np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])


def areas(vertices, triangles):
    return 0.5 * norm3(cross(vertices, triangles))


def weights(area):
    """Integer weights floor(area 2^(32 - e)), the largest area being m 2^e with m in [0.5, 1): uint64 < 2^32."""
    area = np.asarray(area, np.float64)
    _, e = np.frexp(area.max())
    return np.floor(np.ldexp(area, 32 - int(e))).astype(np.uint64)


def table(vertices, triangles):
    """The inclusive uint64 prefix sum of the weights."""
    return np.cumsum(weights(areas(vertices, triangles)), dtype=np.uint64)


def choose(cum, n, seed, first=0):
    """Triangle index of samples ``first .. first + n - 1`` and their two point words (r1, r2)."""
    i = np.arange(first, first + n, dtype=np.uint64)
    with np.errstate(over="ignore"):
        c0 = np.uint64(3) * i + np.uint64(1)
        r0, r1, r2 = splitmix64(seed, c0), splitmix64(seed, c0 + np.uint64(1)), splitmix64(seed, c0 + np.uint64(2))
    total = cum[-1]
    if total == 0:
        raise ValueError("every triangle is degenerate")
    target = mulhi64(r0, np.full(n, total, np.uint64))
    return np.searchsorted(cum, target, side="right").astype(np.int64), r1, r2


def barycentric(r1, r2):
    u1 = (r1 >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    u2 = (r2 >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    s = np.sqrt(u1)
    return 1.0 - s, s * (1.0 - u2), s * u2


def _blend(field, t, k, wa, wb, wc):
    f = np.asarray(field, np.float32).astype(np.float64)
    a, b, c = f[t[k, 0]], f[t[k, 1]], f[t[k, 2]]
    return ((wa[:, None] * a + wb[:, None] * b) + wc[:, None] * c).astype(np.float32)


def sample(vertices, triangles, n, seed=0, normals=None, colors=None, use_triangle_normal=False):
    """-> (positions (n, 3) float32, normals or None, colors or None, triangle index (n,) int32)."""
    t = np.asarray(triangles).reshape(-1, 3)
    if len(t) == 0:
        raise ValueError("the mesh has no triangles")
    k, r1, r2 = choose(table(vertices, t), int(n), seed)
    wa, wb, wc = barycentric(r1, r2)
    pos = _blend(vertices, t, k, wa, wb, wc)
    nrm = None
    if use_triangle_normal:
        c = cross(vertices, t)[k]
        with np.errstate(invalid="ignore", divide="ignore"):
            nrm = (c / norm3(c)[:, None]).astype(np.float32)
    elif normals is not None:
        nrm = _blend(normals, t, k, wa, wb, wc)
    col = None if colors is None else _blend(colors, t, k, wa, wb, wc)
    return pos, nrm, col, k.astype(np.int32)
