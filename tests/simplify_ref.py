"""The vertex-clustering rule of DESIGN §2.9 in plain numpy: the yardstick of tests/test_simplify_ref.py and
tests/test_gpu_mesh_simplify.py.  Written from the rule's text, not from csrc/meshsimplify.hip.

Vertices are float32; all arithmetic is float64 on the widened values.
  grid       origin = (double)min_bound - voxel_size * 0.5, cell(i) = floor(((double)p_i - origin) / voxel_size);
  vertices   output vertex j is the j-th distinct cell in order of first appearance over i = 0 .. nv - 1;
  position   the members' values summed in ascending input index (from +0), divided by (double)count, rounded
             to float32; normals and colours the same way;
  triangles  (a, b, c) = map[corners]; dropped when two are equal; rotated so the smallest index comes first;
             dropped when the same rotated triple occurred at a lower input index; survivors keep input order.
Errors: ValueError for a voxel size that is not finite and positive, no vertices, a non-finite coordinate or an
index outside [0, nv); GridTooFine for 2^21 or more cells along an axis.

Also the scalar rules of the reference's downsample_mesh (scripts/downsample_fbx_mesh.py:143-150, 232-238) and
the voxel-size search of mqr/downsample_mesh.py's docstring, over this file's own count function."""
import math

import numpy as np

AXIS_CELLS = 1 << 21


class GridTooFine(RuntimeError):
    pass


def cells(v, voxel_size):
    """Integer cell coordinates (nv, 3) int64 and the cell count along each axis."""
    voxel_size = float(voxel_size)
    if not math.isfinite(voxel_size) or voxel_size <= 0.0:
        raise ValueError("voxel_size must be finite and > 0")
    v = np.asarray(v, np.float32).reshape(-1, 3)
    if len(v) == 0:
        raise ValueError("no vertices")
    if not np.isfinite(v).all():
        raise ValueError("a vertex coordinate is not finite")
    p = v.astype(np.float64)
    origin = p.min(0) - voxel_size * 0.5
    with np.errstate(over="ignore"):
        q = np.floor((p - origin) / voxel_size)
    axis = q.max(0) + 1.0
    if (axis >= AXIS_CELLS).any():
        raise GridTooFine("the grid is too fine")
    return q.astype(np.int64), axis.astype(np.int64)


def first_appearance(c):
    """map (nv,) and the number of distinct rows of c, numbered in order of first appearance."""
    key = (c[:, 0] << 42) | (c[:, 1] << 21) | c[:, 2]
    _, first, inv = np.unique(key, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")          # sorted-unique position -> rank by first appearance
    rank = np.empty(len(first), np.int64)
    rank[order] = np.arange(len(first))
    return rank[inv.reshape(-1)], len(first)


def cluster_count(v, voxel_size):
    return first_appearance(cells(v, voxel_size)[0])[1]


def ordered_means(values, mp, n_out):
    """Per output vertex: the members' rows summed in ascending input index in float64, from +0, divided by the
    count, rounded to float32.  Cells are walked member rank by member rank (each step adds one member to every
    cell that still has one), which is the sequential sum of each cell; a few very large cells finish through
    np.cumsum, which is sequential too."""
    x = np.asarray(values, np.float32).reshape(-1, 3).astype(np.float64)
    order = np.argsort(mp, kind="stable")             # members of a cell, ascending input index
    count = np.bincount(mp, minlength=n_out)
    start = np.concatenate([[0], np.cumsum(count)[:-1]])
    by_pop = np.argsort(-count, kind="stable")         # cells, largest first: the active ones are a prefix
    pops = count[by_pop]
    acc = np.zeros((n_out, 3), np.float64)
    r = 0
    while True:
        active = int(np.searchsorted(-pops, -r, side="left"))   # cells with more than r members
        if active == 0:
            break
        if active <= 16:
            for j in by_pop[:active]:
                rest = x[order[start[j] + r:start[j] + count[j]]]
                acc[j] = np.cumsum(np.concatenate([acc[j][None], rest]), axis=0)[-1]
            break
        cj = by_pop[:active]
        acc[cj] = acc[cj] + x[order[start[cj] + r]]
        r += 1
    return (acc / count[:, None].astype(np.float64)).astype(np.float32)


def rotate_smallest_first(t):
    k = np.argmin(t, axis=1)  # three distinct entries where it matters: the smallest is unique
    i = np.arange(len(t))
    return np.stack([t[i, k], t[i, (k + 1) % 3], t[i, (k + 2) % 3]], 1)


def simplify(v, t, voxel_size, normals=None, colors=None):
    """-> (positions, normals or None, colors or None, triangles int32, stats int64[8])."""
    v = np.asarray(v, np.float32).reshape(-1, 3)
    t = np.zeros((0, 3), np.int64) if t is None else np.asarray(t).reshape(-1, 3).astype(np.int64)
    c, axis = cells(v, voxel_size)
    if len(t) and (t.min() < 0 or t.max() >= len(v)):
        raise ValueError("a triangle index is outside [0, nv)")
    mp, n_out = first_appearance(c)
    pos = ordered_means(v, mp, n_out)
    nrm = None if normals is None else ordered_means(normals, mp, n_out)
    col = None if colors is None else ordered_means(colors, mp, n_out)
    m = mp[t]
    collapsed = (m[:, 0] == m[:, 1]) | (m[:, 1] == m[:, 2]) | (m[:, 0] == m[:, 2])
    live = np.flatnonzero(~collapsed)
    rot = rotate_smallest_first(m[live]) if len(live) else np.zeros((0, 3), np.int64)
    if len(rot):
        if n_out <= 1 << 21:   # three indices in one integer: the same distinct triples, found faster
            _, first = np.unique((rot[:, 0] << 42) | (rot[:, 1] << 21) | rot[:, 2], return_index=True)
        else:
            _, first = np.unique(rot, axis=0, return_index=True)
        keep = np.sort(first)                                  # the lowest input index of each triple
    else:
        keep = np.zeros(0, np.int64)
    tri = rot[keep].astype(np.int32)
    stats = np.array([len(v), n_out, len(t), int(collapsed.sum()), len(live) - len(keep), len(keep),
                      int(np.bincount(mp).max()), int(axis.max())], np.int64)
    return pos, nrm, col, tri, stats


# ---- the scalar rules of downsample_mesh and the voxel-size search ------------------------------------------
def target_count(n, percent):
    if percent <= 0 or percent > 100:
        raise ValueError("Target vertex percentage must be between 0 and 100")
    return max(4, int(n * (percent / 100.0)))


def diagonal(v):
    p = np.asarray(v, np.float32).reshape(-1, 3).astype(np.float64)
    return float(np.linalg.norm(p.max(0) - p.min(0)))


def v_ref(diag, target):
    return diag / (target ** (1 / 3)) * 1.2


def fit(count, vref, target):
    """(size, count, evaluations) of the search: double from v_ref while the count is above the target, halve
    below it while the count is under the target and the grid is not too fine, 16 geometric bisection steps
    (a grid that is too fine counts as "above the target" and is not an evaluation), then the evaluated size
    with the smallest |C - target|, the larger size on a tie."""
    seen = []

    def C(x):
        n = count(x)
        seen.append((x, n))
        return n

    hi = vref
    k = 0
    while C(hi) > target and k < 32:
        hi *= 2.0
        k += 1
    lo = hi / 2.0
    k = 0
    while k < 32:
        try:
            if not C(lo) < target:
                break
        except GridTooFine:
            break
        lo /= 2.0
        k += 1
    for _ in range(16):
        mid = math.sqrt(lo * hi)
        try:
            above = C(mid) > target
        except GridTooFine:
            above = True
        lo, hi = (mid, hi) if above else (lo, mid)
    best = None
    for x, n in seen:
        d = abs(n - target)
        if best is None or d < best[0] or (d == best[0] and x > best[1]):
            best = (d, x, n)
    return best[1], best[2], seen


def downsample(v, t, percent, rule="fit", normals=None, colors=None):
    """The triangle-mesh branch of downsample_mesh: (voxel size, simplify(...) result); None when the target is
    not below the vertex count."""
    v = np.asarray(v, np.float32).reshape(-1, 3)
    target = target_count(len(v), percent)
    if target >= len(v):
        return None
    d = diagonal(v)
    if d <= 0:
        raise ValueError("Mesh bounding box has zero size, cannot downsample")
    size = v_ref(d, target)
    if rule == "fit":
        size = fit(lambda x: cluster_count(v, x), size, target)[0]
    return size, simplify(v, t, size, normals, colors)
