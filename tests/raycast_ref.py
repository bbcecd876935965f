"""Float32 restatement of the ray caster's primitive test, and the constructed scenes that pin it.
Test infrastructure (numpy only): the product never imports this.

``brute_force`` runs Moeller-Trumbore over every triangle in float32, operation by operation as
csrc/raycast.hip's k_leaves and tri_test do it: e1 / e2 as float32 differences, the same left-to-right
sums, inv = 1 / det, inclusive u / v bounds, 0 < t < inf, NaN falling through the comparisons the way it
does on the device.  It has no tree: whatever the kernel's build, box test, pruning and stack do, the
kernel must return this minimum.  Per ray it gives the minimal t, the set of triangles attaining it and
(u, v) for each member of that set.

``morton_keys`` and ``karras_tree`` restate k_morton's quantisation and k_radix_tree's split rule, so
that a scene's tree shape (the ladder's depth) can be checked without a device.

The scene builders return ``Scene`` objects.  In an *exact* scene every coordinate is a small dyadic
number and every direction component is 0 or a power of two, so that 1 / d, det and all products are
exact in float32 and float64 alike: there the float64 oracle must agree bit for bit as well.
"""
from dataclasses import dataclass, field

import numpy as np

F = np.float32


@dataclass
class Scene:
    name: str
    geoms: list            # [(vertices (nv, 3) float32, triangles (nt, 3) int32)], in add_triangles order
    rays: np.ndarray       # (R, 6) float32
    exact: bool = True     # float32 and float64 arithmetic both exact: the oracle must agree bit for bit
    all_hit: bool = False  # a closed surface cast from inside: every t must be finite
    extra: dict = field(default_factory=dict)

    def soup(self):
        """(corners (N, 3, 3) float32, geometry id (N,), primitive id (N,)) over all geometries."""
        P, G, I = [], [], []
        for g, (v, t) in enumerate(self.geoms):
            if len(t):
                P.append(v[t])
                G.append(np.full(len(t), g, np.int64))
                I.append(np.arange(len(t), dtype=np.int64))
        return np.concatenate(P).astype(F), np.concatenate(G), np.concatenate(I)

    def merged(self):
        """One (vertices, triangles) pair for oracle.raycast: triangle order = soup order."""
        V, T, base = [], [], 0
        for v, t in self.geoms:
            V.append(v)
            T.append(t + base)
            base += len(v)
        return np.concatenate(V).astype(F), np.concatenate(T).astype(np.int32)


# ---------------------------------------------------------------------------------- brute force
@dataclass
class Ref:
    t: np.ndarray      # (R,) float32, inf on a miss
    ray: np.ndarray    # members of the minimal-t sets, flattened and sorted by (ray, tri): ray index,
    tri: np.ndarray    # soup triangle index,
    u: np.ndarray      # and that triangle's (u, v) for the ray
    v: np.ndarray
    ntri: int

    def first(self):
        """Smallest soup index of each ray's minimal set, -1 on a miss (the oracle's primitive)."""
        out = np.full(len(self.t), -1, np.int64)
        r, at = np.unique(self.ray, return_index=True)   # members are sorted by (ray, tri)
        out[r] = self.tri[at]
        return out

    def lookup(self, ray, tri):
        """Position of (ray, tri) among the members, -1 where tri is not in ray's minimal set."""
        key = self.ray * self.ntri + self.tri
        q = np.asarray(ray, np.int64) * self.ntri + np.asarray(tri, np.int64)
        pos = np.searchsorted(key, q)
        pos = np.minimum(pos, max(len(key) - 1, 0))
        ok = (key[pos] == q) if len(key) else np.zeros(len(q), bool)
        return np.where(ok, pos, -1)


def _tri_test(P, o, d):
    """tri_test for rays (r, 3) x triangles (n, 3, 3) -> t (inf where it returns early), u, v; float32."""
    a = P[None, :, 0, :]
    e1 = (P[:, 1, :] - P[:, 0, :])[None]          # k_leaves: float32 differences
    e2 = (P[:, 2, :] - P[:, 0, :])[None]
    dx, dy, dz = d[:, None, 0], d[:, None, 1], d[:, None, 2]
    px = dy * e2[..., 2] - dz * e2[..., 1]
    py = dz * e2[..., 0] - dx * e2[..., 2]
    pz = dx * e2[..., 1] - dy * e2[..., 0]
    det = (e1[..., 0] * px + e1[..., 1] * py) + e1[..., 2] * pz
    inv = F(1.0) / det
    tx, ty, tz = o[:, None, 0] - a[..., 0], o[:, None, 1] - a[..., 1], o[:, None, 2] - a[..., 2]
    u = ((tx * px + ty * py) + tz * pz) * inv
    qx = ty * e1[..., 2] - tz * e1[..., 1]
    qy = tz * e1[..., 0] - tx * e1[..., 2]
    qz = tx * e1[..., 1] - ty * e1[..., 0]
    v = ((dx * qx + dy * qy) + dz * qz) * inv
    t = ((e2[..., 0] * qx + e2[..., 1] * qy) + e2[..., 2] * qz) * inv
    # the early returns, with NaN failing every comparison as it does on the device
    out = (det == 0) | (u < 0) | (u > 1) | (v < 0) | (u + v > 1)
    ok = ~out & (t > 0) & (t < np.inf)
    return np.where(ok, t, F(np.inf)), u, v


def brute_force(P, rays, chunk=256):
    P = np.ascontiguousarray(P, F)
    rays = np.ascontiguousarray(rays, F).reshape(-1, 6)
    R, n = len(rays), len(P)
    tmin = np.empty(R, F)
    mr, mt, mu, mv = [], [], [], []
    with np.errstate(all="ignore"):
        for s in range(0, R, chunk):
            t, u, v = _tri_test(P, rays[s:s + chunk, :3], rays[s:s + chunk, 3:])
            assert t.dtype == F and u.dtype == F and v.dtype == F
            m = t.min(axis=1)
            tmin[s:s + chunk] = m
            r, k = np.nonzero((t == m[:, None]) & np.isfinite(t))
            mr.append(r + s)
            mt.append(k)
            mu.append(u[r, k])
            mv.append(v[r, k])
    return Ref(tmin, np.concatenate(mr).astype(np.int64), np.concatenate(mt).astype(np.int64),
               np.concatenate(mu), np.concatenate(mv), n)


# ---------------------------------------------------------------------------------- tree shape
def _spread21(x):
    v = np.uint64(x) & np.uint64(0x1fffff)
    for s, m in ((32, 0x1f00000000ffff), (16, 0x1f0000ff0000ff), (8, 0x100f00f00f00f00f),
                 (4, 0x10c30c30c30c30c3), (2, 0x1249249249249249)):
        v = (v | (v << np.uint64(s))) & np.uint64(m)
    return v


def morton_keys(P):
    """k_gather_tris' centroid bounds and k_morton's keys of soup triangles P (N, 3, 3), in float32."""
    P = np.ascontiguousarray(P, F)
    third = F(1.0) / F(3.0)
    c = ((P[:, 0, :] + P[:, 1, :]) + P[:, 2, :]) * third
    lo, hi = c.min(axis=0), c.max(axis=0)
    ext = hi - lo
    with np.errstate(all="ignore"):
        s = np.where(ext > 0, (c - lo) / ext, F(0))
    s = np.minimum(np.maximum(s, F(0)), F(1)).astype(F)
    q = np.minimum(s * F(2097152.0), F(2097151.0)).astype(np.uint32)
    return np.array([int(_spread21(a)) << 2 | int(_spread21(b)) << 1 | int(_spread21(z)) for a, b, z in q],
                    dtype=np.uint64)


def karras_tree(keys):
    """k_radix_tree on sorted keys -> child (n - 1, 2): >= 0 internal node, < 0 leaf ~index."""
    k = [int(x) for x in keys]
    n = len(k)
    assert all(k[i] <= k[i + 1] for i in range(n - 1))

    def delta(i, j):
        if j < 0 or j >= n:
            return -1
        if k[i] == k[j]:
            return 64 + (64 - (i ^ j).bit_length())
        return 64 - (k[i] ^ k[j]).bit_length()

    child = np.zeros((n - 1, 2), np.int64)
    for i in range(n - 1):
        d = 1 if delta(i, i + 1) - delta(i, i - 1) >= 0 else -1
        dmin = delta(i, i - d)
        lmax = 2
        while delta(i, i + lmax * d) > dmin:
            lmax <<= 1
        l, t = 0, lmax >> 1
        while t >= 1:
            if delta(i, i + (l + t) * d) > dmin:
                l += t
            t >>= 1
        j = i + l * d
        dnode = delta(i, j)
        s, t = 0, (l + 1) >> 1
        while True:
            if delta(i, i + (s + t) * d) > dnode:
                s += t
            if t == 1:
                break
            t = (t + 1) >> 1
        gamma = i + s * d + min(d, 0)
        lo_, hi_ = min(i, j), max(i, j)
        child[i, 0] = ~gamma if lo_ == gamma else gamma
        child[i, 1] = ~(gamma + 1) if hi_ == gamma + 1 else gamma + 1
    return child


def tree_depths(child):
    """(deepest internal node's depth (root 0), most stack entries a traversal can need): one entry is
    pushed at every node whose children are both internal, so the need is the largest count of such
    nodes on a root path."""
    deepest = need = 0
    todo = [(0, 0, 0)]
    while todo:
        node, depth, pushed = todo.pop()
        deepest = max(deepest, depth)
        c0, c1 = child[node]
        if c0 >= 0 and c1 >= 0:
            pushed += 1
        need = max(need, pushed)
        for c in (c0, c1):
            if c >= 0:
                todo.append((int(c), depth + 1, pushed))
    return deepest, need


# ---------------------------------------------------------------------------------- scene builders
def _rays(o, d):
    o, d = np.broadcast_arrays(np.asarray(o, F), np.asarray(d, F))
    return np.concatenate([o, d], axis=-1).reshape(-1, 6).astype(F)


def _pow2_or_zero(x):
    m, _ = np.frexp(np.abs(x))
    return np.all((x == 0) | (m == 0.5), axis=-1)


_CUBE_V = np.array([[x, y, z] for z in (0, 1) for y in (0, 1) for x in (0, 1)], F)
_CUBE_T = np.array([[0, 1, 3], [0, 3, 2], [4, 7, 5], [4, 6, 7],     # z = 0, z = 1
                    [0, 5, 1], [0, 4, 5], [2, 3, 7], [2, 7, 6],     # y = 0, y = 1
                    [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]], np.int32)  # x = 0, x = 1


def _cube_rays():
    pts = [np.array(p) / 2.0 for p in np.ndindex(3, 3, 3) if p != (1, 1, 1)]  # face centres, edge midpoints, vertices
    for f in range(3):                                                        # both diagonals of every face
        for side in (0.0, 1.0):
            for a in (0.25, 0.75):
                for b in (0.25, 0.75):
                    p = np.empty(3)
                    p[f], p[(f + 1) % 3], p[(f + 2) % 3] = side, a, b
                    pts.append(p)
    signs = np.array([p for p in np.ndindex(3, 3, 3) if p != (1, 1, 1)], np.float64) - 1.0
    rays = []
    for o in ([0.5, 0.5, 0.5], [0.25, 0.5, 0.75], [0.75, 0.75, 0.75], [0.125, 0.375, 0.625], [0.5, 0.25, 0.5]):
        o = np.array(o)
        d = np.array(pts) - o
        d = d[_pow2_or_zero(d) & np.any(d != 0, axis=1)]   # aimed rays whose components are 0 or +-2^k
        rays.append(_rays(o, d))
        for scale in ([1, 1, 1], [0.5, 2, 1], [4, 0.25, 0.5]):
            rays.append(_rays(o, signs * np.array(scale)))
    return np.concatenate(rays)


def cube_inside():
    """The unit cube (12 triangles) cast from inside: through every face centre, shared edge midpoint and
    vertex and along the face diagonals, from the centre and from off-centre dyadic origins."""
    return Scene("cube_inside", [(_CUBE_V.copy(), _CUBE_T.copy())], _cube_rays(), all_hit=True)


def _grid_box(n=4):
    """The closed box [0, n]^3, every face n x n unit squares of two triangles: 12 n^2 triangles whose
    leaf and internal-node boxes have their bounds on the integer grid."""
    tris = []
    for f in range(3):
        a, b = (f + 1) % 3, (f + 2) % 3
        for side in (0, n):
            for i in range(n):
                for j in range(n):
                    q = np.zeros((4, 3))
                    q[:, f] = side
                    q[:, a] = [i, i + 1, i + 1, i]
                    q[:, b] = [j, j, j + 1, j + 1]
                    tris += [q[[0, 1, 2]], q[[0, 2, 3]]]
    P = np.array(tris, F)
    return P.reshape(-1, 3), np.arange(3 * len(P), dtype=np.int32).reshape(-1, 3)


def axis_parallel():
    """Axis-parallel rays inside the grid box, with +0 and -0 in the zero components.  The two fixed
    origin coordinates take the values 0 and 4 (in the plane of a box face: bounds of leaves, of internal
    nodes and of the root), 1, 2 and 3 (on grid lines: leaf and internal-node bounds) and 0.5 and 3.5
    (strictly inside), for each axis, each direction and each side."""
    V, T = _grid_box(4)
    vals = [0.0, 0.5, 1.0, 2.0, 3.0, 3.5, 4.0]
    rays = []
    for f in range(3):
        a, b = (f + 1) % 3, (f + 2) % 3
        for step in (1.0, -1.0, 0.5, -2.0):
            for za in (0.0, -0.0):
                for zb in (0.0, -0.0):
                    for p in vals:
                        for q in vals:
                            o, d = np.empty(3), np.empty(3)
                            o[f], o[a], o[b] = 1.5, p, q
                            d[f], d[a], d[b] = step, za, zb
                            rays.append(np.concatenate([o, d]))
    return Scene("axis_parallel", [(V, T)], np.array(rays, F), all_hit=True)


def grid_box_oblique(outlier=False):
    """The grid box cast from an inside origin along every direction of {+-0.5, +-1, +-2}^3 (no zero
    component).  With ``outlier`` one far triangle (~1.3e30) stretches the centroid bounds so that every
    other triangle falls into one Morton cell."""
    V, T = _grid_box(4)
    geoms = [(V, T)]
    if outlier:
        A, h = 2.0 ** 100, 2.0 ** 90
        geoms.append((np.array([[A, A, A], [A + h, A, A], [A, A + h, A]], F), np.array([[0, 1, 2]], np.int32)))
    c = [-2.0, -1.0, -0.5, 0.5, 1.0, 2.0]
    d = np.array([[x, y, z] for x in c for y in c for z in c])
    rays = np.concatenate([_rays([1.5, 2.5, 0.5], d), _rays([2.0, 2.0, 2.0], d), _rays([0.25, 3.75, 1.0], d)])
    return Scene("grid_box_outlier" if outlier else "grid_box_oblique", geoms, rays, all_hit=True)


def bounds_and_degenerate_relations():
    """Hits exactly at u = 0, v = 0, u + v = 1 and at the vertices of a triangle, and just outside them; the
    origin on a triangle (t = 0: skipped, the next one behind is hit); coplanar rays, rays pointing away
    and the zero direction (misses)."""
    V = np.array([[0, 0, 1], [1, 0, 1], [0, 1, 1],            # A, in z = 1
                  [-1, -1, 2], [3, -1, 2], [-1, 3, 2]], F)    # B, in z = 2, behind all of A
    T = np.array([[0, 1, 2], [3, 4, 5]], np.int32)
    e = 2.0 ** -20
    xy = [(0, 0.5), (0.5, 0), (0.5, 0.5), (0, 0), (1, 0), (0, 1), (0.25, 0.25),         # on A's bounds / inside
          (-e, 0.5), (0.5, -e), (0.5 + e, 0.5), (-e, -e), (1 + e, 0), (0, 1 + e),        # just outside A
          (-1, -1), (3, -1), (-1, 3), (1, 1), (1, -1), (-1, 1), (3, 3), (-1 - e, 0)]     # B's bounds
    rays = [_rays([[x, y, 0] for x, y in xy], [0, 0, 1]),
            _rays([[x, y, 0] for x, y in xy], [0, -0.0, 2]),
            _rays([[x, y, 4] for x, y in xy], [-0.0, 0, -0.5]),
            _rays([[0.25, 0.25, 1], [0, 0.5, 1], [0, 0, 1]], [0, 0, 1]),     # origin on A: B behind is hit
            _rays([[0.25, 0.25, 1], [0.5, 0.5, 1]], [0, 0, -1]),             # origin on A, nothing behind
            _rays([[0.25, 0.25, 2]], [[0, 0, 1], [0, 0, -1]]),               # origin on B
            _rays([[-2, 0.25, 1], [-2, 0.25, 2], [0.25, -2, 1]], [[1, 0, 0], [1, 0, 0], [0, 1, 0]]),  # coplanar
            _rays([[-2, 0, 1], [0, 0, 1]], [[1, 0, 0], [1, 1, 0]]),          # coplanar, along A's edges
            _rays([[0.25, 0.25, 0]], [[0, 0, -1], [1, 0, -1], [0, -2, -0.5]]),   # pointing away
            _rays([[0.25, 0.25, 0], [0.25, 0.25, 1], [0, 0, 0]], [[0, 0, 0], [-0.0, 0, -0.0], [0, 0, 0]])]
    return Scene("bounds", [(V, T)], np.concatenate(rays))


def ties():
    """Equal-t ties: two coincident triangles of opposite winding, duplicated triangles, and two
    triangles sharing the hit edge (and the hit vertex)."""
    V = np.array([[0, 0, 1], [2, 0, 1], [0, 2, 1],                       # coincident / duplicated
                  [4, 0, 1], [6, 0, 1], [6, 2, 1], [4, 2, 1],            # a square, split along 4-6
                  [0, 0, 1], [2, 0, 1], [0, 2, 1]], F)                   # the same corners as other vertices
    T = np.array([[0, 1, 2], [0, 2, 1], [0, 1, 2], [7, 8, 9], [1, 2, 0],
                  [3, 4, 5], [3, 5, 6]], np.int32)
    xy = [(0.5, 0.5), (0.25, 1), (1, 1), (0, 0), (2, 0), (0, 1), (1, 0), (1.5, 0.25),
          (5, 1), (4.5, 0.5), (5.5, 1.5), (4, 0), (6, 2), (5, 0.5), (4.5, 1.5), (3, 1), (6, 0), (4, 2)]
    rays = [_rays([[x, y, 0] for x, y in xy], [0, 0, 1]),
            _rays([[x, y, 3] for x, y in xy], [0, 0, -2]),
            _rays([[x - 1, y + 0.5, 0] for x, y in xy], [1, -0.5, 1]),
            _rays([[x + 0.5, y + 2, -1] for x, y in xy], [-0.25, -1, 1])]
    return Scene("ties", [(V, T)], np.concatenate(rays))


def cube_with_degenerates():
    """cube_inside with repeated-index and zero-area triangles mixed in (they are never hit and must not
    change any other ray); extra['cube_prim'] maps this scene's primitives to cube_inside's (-1: degenerate)."""
    V = np.concatenate([_CUBE_V, np.array([[0.5, 0.5, 0.5], [0.25, 0.25, 0.25], [0.75, 0.75, 0.75],
                                           [0, 0.5, 0], [0, 1, 0]], F)])
    deg = [[0, 0, 7], [5, 5, 5], [9, 8, 10], [0, 11, 12], [3, 7, 3], [8, 8, 8], [9, 10, 8]]
    T, back = [], []
    for i, t in enumerate(_CUBE_T):
        if i % 2 == 0:
            T.append(deg[i // 2])
            back.append(-1)
        T.append(list(t))
        back.append(i)
    T.append(deg[6])
    back.append(-1)
    return Scene("cube_degenerates", [(V, np.array(T, np.int32))], _cube_rays(), all_hit=True,
                 extra={"cube_prim": np.array(back)})


def same_centroid(n):
    """n coplanar right triangles (z = 1) of different sizes, positions and windings whose vertex sums
    are all exactly (4, 4, 3): every centroid is the same float32 value, the centroid extent is zero and
    every Morton key is 0, so the tree is split by index alone.  n = 1 is the kernel's tree-less path."""
    # corner x0 and leg a with 3 x0 + a = 4 and |a| a power of two (so det is one too)
    legs = [(a, (4.0 - a) / 3.0) for a in (1.0, 4.0, 16.0, 0.25, -2.0, -8.0, -0.5, -32.0)]
    fam = []
    for w in (0, 1):
        for ax, x0 in legs:
            for ay, y0 in legs:
                p = [[x0, y0, 1], [x0 + ax, y0, 1], [x0, y0 + ay, 1]]
                fam.append(p if w == 0 else [p[0], p[2], p[1]])
    fam = np.array(fam, F)
    order = np.random.default_rng(n).permutation(len(fam))
    P = fam[order[np.arange(n) % len(fam)]]
    assert np.all(P.sum(axis=1) == np.array([4, 4, 3], F))
    g = np.arange(-8.0, 12.25, 0.625)
    xy = np.array([[x, y] for x in g for y in g])
    o = np.concatenate([xy, np.zeros((len(xy), 1))], axis=1)
    rays = np.concatenate([_rays(o, [0, 0, 1]), _rays(o + [0.5, 0.25, 0], [-0.5, -0.25, 1]),
                           _rays(o + [0, 0, 3], [0, -0.0, -2])])
    return Scene(f"same_centroid_{n}", [(P.reshape(-1, 3), np.arange(3 * n, dtype=np.int32).reshape(-1, 3))], rays)


def three_geometries():
    """Three geometries, the middle one empty (vertices but no triangles)."""
    g0 = (np.array([[0, 0, 1], [2, 0, 1], [2, 2, 1], [0, 2, 1]], F), np.array([[0, 1, 2], [0, 2, 3]], np.int32))
    g1 = (np.array([[0, 0, 0.5], [1, 0, 0.5], [0, 1, 0.5]], F), np.zeros((0, 3), np.int32))
    g2 = (np.array([[1, 1, 2], [5, 1, 2], [5, 5, 2], [1, 5, 2], [1, 1, 0.5], [1.5, 1, 0.5], [1, 1.5, 0.5]], F),
          np.array([[0, 1, 2], [0, 2, 3], [4, 5, 6]], np.int32))
    g = np.arange(-0.5, 5.75, 0.25)
    o = np.array([[x, y, 0] for x in g for y in g])
    rays = np.concatenate([_rays(o, [0, 0, 1]), _rays(o + [0, 0, 4], [0, 0, -1]), _rays(o, [0.25, 0.5, 1])])
    return Scene("three_geometries", [g0, g1, g2], rays)


def _octahedron(levels):
    v = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    t = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    v = [np.array(p, np.float64) for p in v]
    for _ in range(levels):
        mid, nt = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[k] = len(v) - 1
            return mid[k]
        for a, b, c in t:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nt += [(a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca)]
        t = nt
    return np.array(v), np.array(t, np.int32)


def generic():
    """Inexact arithmetic: a seeded soup of 500 random triangles and a closed, subdivided octahedron of 512
    (shared vertices).  From a fixed origin, rays aimed at every triangle's vertices, edge midpoints and
    centroid (d = float32(target - origin)), and 2048 seeded random rays."""
    rng = np.random.default_rng(20250)
    c = rng.uniform(-3, 3, (500, 1, 3))
    soup = (c + rng.normal(0, 1, (500, 3, 3)) * rng.uniform(0.05, 0.8, (500, 1, 1))).astype(F)
    ov, ot = _octahedron(3)
    ov = (ov * 1.25 + [0.3, -0.2, 0.4]).astype(F)
    geoms = [(soup.reshape(-1, 3), np.arange(1500, dtype=np.int32).reshape(-1, 3)), (ov, ot)]
    P = np.concatenate([soup, ov[ot]]).astype(np.float64)
    origin = np.array([0.4, -5.5, 0.9], F)
    targets = np.concatenate([P[:, 0], P[:, 1], P[:, 2], (P[:, 0] + P[:, 1]) / 2, (P[:, 1] + P[:, 2]) / 2,
                              (P[:, 2] + P[:, 0]) / 2, P.mean(axis=1)]).astype(F)
    aimed = _rays(origin, targets - origin)
    ro = rng.uniform(-4, 4, (2048, 3))
    rd = rng.normal(0, 1, (2048, 3))
    return Scene("generic", geoms, np.concatenate([aimed, _rays(ro, rd)]), exact=False)


def ladder():
    """A tree deeper than 64 levels.  Centroids at 2^i on one axis each (i = 0..20 on x, y and z) between a
    low corner (0, 0, 0) and a high corner (E, E, E), E = 2^21: with the centroid extent E the Morton
    cells are the integers, so these triangles have the keys 2^0 .. 2^62 and the tree peels one key off
    per level.  Two triangles at each of them, sixteen at the low corner, one at the high corner: every
    node down the chain has two internal children.

    All coordinates are integers below 2^24 whose sums are exact, so every centroid is exact in float32.
    Every triangle contains the disc of radius R = 0.875 E about its centroid, which contains the rays, and
    its box contains the rays' common origin height: every box is entered at t = 0.  Each triangle lies in a
    tangent plane of the paraboloid z = B + A |xy - X0|^2 (to integer rounding), the tangent point chosen
    on the circle of those whose plane passes through the triangle's centroid; a ray cast down at the
    tangent point meets that plane above all the others.  One ray per triangle."""
    E = 2.0 ** 21
    cents = []
    for i in range(21):
        for axis in range(3):
            c = np.zeros(3)
            c[axis] = 2.0 ** i
            cents += [c, c]
    cents += [np.zeros(3)] * 16 + [np.full(3, E)]
    cents = np.array(cents)
    n = len(cents)
    X0, B, A, R, z0 = np.array([E / 2, E / 2]), 1.25 * E, 2.0 ** -18, 0.875 * E, 1.5 * E
    # tan(phi), the tangent point's angle off the centroid's direction, from equally spaced candidates in
    # [-1, 1]: the triangles nearest X0 (the steepest planes) choose first and get the smallest |tan|
    m = cents[:, :2] - X0
    near = np.argsort(np.linalg.norm(m, axis=1), kind="stable")
    tans = np.linspace(-1.0, 1.0, 4 * n)
    tans = list(tans[np.argsort(np.abs(tans), kind="stable")])

    def tangent_point(i, tan):
        mh = m[i] / np.linalg.norm(m[i])
        phi = np.arctan(tan)
        e = np.array([mh[0] * np.cos(phi) - mh[1] * np.sin(phi), mh[0] * np.sin(phi) + mh[1] * np.cos(phi)])
        me = m[i] @ e
        return (me - np.sqrt(me * me + (B - cents[i, 2]) / A)) * e   # |p|^2 - 2 p.m = (B - c.z) / A, p = s e

    # the first free tan whose tangent point keeps 2600 units from those placed: planes whose tangent
    # points are d apart differ by A d^2 (26 units) at them
    pts = np.full((n, 2), np.inf)
    for i in near:
        for k, tan in enumerate(tans):
            p = tangent_point(i, tan)
            if np.min(np.linalg.norm(pts - p, axis=1)) >= 2600.0:
                pts[i] = p
                del tans[k]
                break
    assert np.isfinite(pts).all()
    P = np.empty((n, 3, 3))
    rays = np.empty((n, 6))
    for i in range(n):
        p = pts[i]
        G = 2 * A * p                                          # the plane's gradient
        gh = G / np.linalg.norm(G)
        o0 = np.rint(2 * R * gh)                               # one vertex up the gradient: a high box top
        o1 = np.rint(2 * R * np.array([-0.5 * gh[0] - np.sqrt(0.75) * gh[1], np.sqrt(0.75) * gh[0] - 0.5 * gh[1]]))
        o2 = -(o0 + o1)
        zo = [np.rint(G @ o0), np.rint(G @ o1)]
        zo.append(-(zo[0] + zo[1]))
        for k, (o, z) in enumerate(zip((o0, o1, o2), zo)):
            P[i, k, :2] = cents[i, :2] + o
            P[i, k, 2] = cents[i, 2] + z
        rays[i] = [X0[0] + p[0], X0[1] + p[1], z0, 0, 0, -1]
    assert np.abs(P).max() < 2 ** 24 and np.array_equal(P, P.astype(F).astype(np.float64))
    return Scene("ladder", [(P.reshape(-1, 3).astype(F), np.arange(3 * n, dtype=np.int32).reshape(-1, 3))],
                 rays.astype(F), exact=False, all_hit=True)


def exact_scenes():
    return [cube_inside(), axis_parallel(), grid_box_oblique(), grid_box_oblique(outlier=True),
            bounds_and_degenerate_relations(), ties(), cube_with_degenerates(), three_geometries()] + \
           [same_centroid(n) for n in SAME_CENTROID_N]


SAME_CENTROID_N = (1, 2, 3, 255, 256, 257, 1025)
