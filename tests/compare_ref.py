"""Numpy restatement of the ground-truth comparison report: test infrastructure only, never
imported by the product.  Everything is float64 on float32 inputs and brute force.

Tolerances, derived (u = 2^-53, the unit round-off of float64):

* Counts (samples within a threshold, overlap, holes, points), bounds, and what follows from them by the same
  IEEE operations on both sides (extent ratios, centre offsets, precision, recall, F-score) are exact: 0.
* A distance is sqrt((dx dx + dy dy) + dz dz): five roundings after exact differences of float32 values, at
  most 4 u relative.  Two implementations that follow the rule agree bit for bit; against an implementation
  that rounds differently (an FMA in a BLAS dot product) a distance statistic that picks one value (min, max,
  median, Hausdorff) gets relative 2^-51.
* Both sides add the same correctly rounded terms (the distance rule above, the same cross products): only
  the order of the n - 1 additions and the closing operations (a division, a halving, an abs) differ.  A sum
  of n terms in a fixed order is within (n - 1) u of the exact sum, relative to the sum of the terms'
  magnitudes; a mean or a sum (Chamfer, area, volume) is held to relative (n + 4) 2^-53 of that scale, which
  for sums with cancellation (the signed volume) is not the result.  (Two orders could differ by twice
  (n - 1) u if every rounding of one erred up and of the other down; the bound does not allow for that.)
* std = sqrt(S / n), S = sum (x - mean)^2.  With every deviation off by d <= 2 e max|x| (e the mean's
  relative tolerance), |dS| <= 2 sqrt(n S) d + (n + 4) 2^-53 S, so |d std| <= d + (n + 4) 2^-53 std: the mean's
  relative tolerance on the scale 3 max|x|.
* IoU = o / u with o <= u: |d IoU| <= (|do| + |du|) / u <= 3 (tol(vs) + tol(vg)) / u.
* After an alignment the samples are rounded to float32 before the search: each coordinate moves by at most
  2^-24 max|coordinate|, a point by sqrt(3) times that, and the distance to a set is 1-Lipschitz in the query
  and in the set, so every distance statistic gets the absolute sqrt(3) 2^-24 max|coordinate| on top (std:
  twice, one for the value and one for the mean).
"""
import numpy as np

U = 2.0 ** -53
EXACT = ("precision", "recall", "f_score", "num_scan_points", "num_gt_points", "num_holes_scan", "num_holes_gt",
         "bounding_box_ratio", "center_offset")
PICKED = ("hausdorff_distance", "median_point_to_surface", "max_point_to_surface", "threshold")
SUMMED = ("chamfer_distance", "mean_point_to_surface", "std_point_to_surface", "surface_area_scan",
          "surface_area_gt", "volume_scan", "volume_gt", "volume_overlap")
FIELDS = ("chamfer_distance", "hausdorff_distance", "mean_point_to_surface", "median_point_to_surface",
          "std_point_to_surface", "max_point_to_surface", "precision", "recall", "f_score", "volume_scan",
          "volume_gt", "volume_overlap", "volume_iou", "bounding_box_ratio", "center_offset", "num_scan_points",
          "num_gt_points", "surface_area_scan", "surface_area_gt", "num_holes_scan", "num_holes_gt")
OVERLAP_SAMPLES, OVERLAP_THRESHOLD = 10000, 0.01


def tolerance(field, n, scale):
    """Absolute tolerance of ``field`` reduced over ``n`` terms of magnitude ``scale`` (module docstring)."""
    if field in EXACT:
        return 0.0
    if field in PICKED:
        return 2.0 ** -51 * scale
    if field in SUMMED:
        return (n + 4) * U * scale
    raise KeyError(field)


def lipschitz(max_coordinate):
    return np.sqrt(3.0) * 2.0 ** -24 * max_coordinate


# ---------------------------------------------------------------------------- primitives
def nearest(queries, targets, chunk=256):
    """(dist, idx) of the nearest target of every query: d2 = (dx dx + dy dy) + dz dz in float64, the lowest
    index among equal d2, dist = sqrt(d2)."""
    q, t = np.asarray(queries, np.float32).astype(np.float64), np.asarray(targets, np.float32).astype(np.float64)
    dist, idx = np.empty(len(q)), np.empty(len(q), np.int32)
    for s in range(0, len(q), chunk):
        d = q[s:s + chunk, None, :] - t[None, :, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        j = d2.argmin(1)  # the first minimum: the lowest index
        idx[s:s + chunk] = j
        dist[s:s + chunk] = np.sqrt(d2[np.arange(len(j)), j])
    return dist, idx


def distance_stats(x, threshold):
    x = np.asarray(x, np.float64)
    return dict(mean=float(np.mean(x)), std=float(np.std(x)), min=float(np.min(x)), max=float(np.max(x)),
                median=float(np.median(x)), count_below=int(np.sum(x < threshold)), count=len(x))


def _corners(v, t):
    v = np.asarray(v, np.float32).astype(np.float64)
    return v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]


def surface_area(v, t):
    """(area, scale): sum of 0.5 |(p1 - p0) x (p2 - p0)|; the scale bounds the terms' magnitudes."""
    if len(t) == 0:
        return 0.0, 0.0
    a, b, c = _corners(v, t)
    area = 0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1)
    scale = 0.5 * np.linalg.norm(b - a, axis=1) * np.linalg.norm(c - a, axis=1)
    return float(area.sum()), float(scale.sum())


def edge_runs(t):
    """slot -> (min, max) key for every edge slot 3 t + e, and the multiplicity of each key."""
    t = np.asarray(t).reshape(-1, 3)
    a = t.reshape(-1)
    b = t[:, [1, 2, 0]].reshape(-1)
    keys = list(zip(np.minimum(a, b).tolist(), np.maximum(a, b).tolist()))
    mult = {}
    for k in keys:
        mult[k] = mult.get(k, 0) + 1
    return keys, mult, (a < b)


def closed_oriented(t):
    """Every edge run has length exactly 2 and its two triangles traverse it in opposite directions."""
    keys, mult, asc = edge_runs(t)
    if len(keys) == 0 or any(m != 2 for m in mult.values()):
        return False
    seen = {}
    for k, up in zip(keys, asc.tolist()):
        if k in seen and seen[k] == up:
            return False
        seen[k] = up
    return True


def volume(v, t):
    """(volume, scale): |sum p0 . (p1 x p2) / 6| for a closed oriented mesh, else 0."""
    if len(t) == 0:
        return 0.0, 0.0
    a, b, c = _corners(v, t)
    terms = np.einsum("ij,ij->i", a, np.cross(b, c)) / 6.0
    scale = float((np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1) * np.linalg.norm(c, axis=1)).sum() / 6.0)
    return (abs(float(terms.sum())) if closed_oriented(t) else 0.0), scale


def boundary_edges(t):
    """The edges on exactly one triangle as (min, max), ascending by slot."""
    keys, mult, _ = edge_runs(t)
    return np.array([k for k in keys if mult[k] == 1], np.int32).reshape(-1, 2)


def hole_perimeters(boundary, v):
    """The boundary walk: vertices in order of first appearance each start a walk along their first neighbour
    with an unvisited edge; every step takes the first unvisited neighbour; a walk that is back at its start
    after more than two edges is a hole."""
    v = np.asarray(v, np.float64)
    nbrs, order = {}, []
    for a, b in np.asarray(boundary).reshape(-1, 2).tolist():
        for x in (a, b):
            if x not in nbrs:
                nbrs[x] = []
                order.append(x)
        nbrs[a].append(b)
        nbrs[b].append(a)
    done = set()

    def free(x):
        for w in nbrs[x]:
            if (min(x, w), max(x, w)) not in done:
                return w
        return None

    out, n_edges = [], len(np.asarray(boundary).reshape(-1, 2))
    for start in order:
        w = free(start)
        if w is None:
            continue
        path, x, steps = [start], start, 0
        while w is not None and (min(x, w), max(x, w)) not in done:
            done.add((min(x, w), max(x, w)))
            steps += 1
            x = w
            path.append(x)
            if x == start and steps > 2:
                out.append(sum(float(np.linalg.norm(v[path[i]] - v[path[i + 1]])) for i in range(len(path) - 1)))
                break
            w = free(x)
            if steps > n_edges:
                break
    return out


def count_holes(v, t, ratio=0.01):
    """(holes at or above the bar, all perimeters, the bar)."""
    if len(t) == 0:
        return 0, [], 0.0
    v32 = np.asarray(v, np.float32).astype(np.float64)
    bar = float(np.linalg.norm(v32.max(0) - v32.min(0)) * ratio)
    per = hole_perimeters(boundary_edges(t), v32)
    return sum(1 for p in per if p >= bar), per, bar


def sample(v, t, num_points, seed):
    """The sampling rule (mqr.compare_mesh_to_ground_truth's docstring), restated."""
    v = np.asarray(v, np.float32)
    t = np.asarray(t).reshape(-1, 3)
    if num_points is None:
        return v.copy()
    if len(t) == 0:
        if len(v) <= num_points:
            return v.copy()
        return v[np.random.default_rng(seed).choice(len(v), size=num_points, replace=False)]
    a, b, c = _corners(v, t)
    cum = np.cumsum(0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1))
    rng = np.random.default_rng(seed)
    k = np.minimum(np.searchsorted(cum, rng.random(num_points) * cum[-1], side="right"), len(t) - 1)
    s = np.sqrt(rng.random(num_points))[:, None]
    r2 = rng.random(num_points)[:, None]
    return ((1.0 - s) * a[k] + (s * (1.0 - r2)) * b[k] + (s * r2) * c[k]).astype(np.float32)


# ---------------------------------------------------------------------------- the report
def report(scan_v, scan_t, gt_v, gt_t, threshold=None, num_sample_points=50000, align_method="none",
           scale_normalize=False, seed=0, round_aligned=True, icp=None, icp_tol=0.0):
    """(metrics dict with FIELDS and ``threshold``, absolute tolerances per field).  ``round_aligned=False``
    keeps the moved samples in float64, as the reference does.  ``align_method="icp"`` takes the ICP step from
    the caller: ``icp(source float32, target float32) -> 4x4`` on the centred samples, its entries trusted to
    ``icp_tol`` (a point then moves by at most sqrt(3) icp_tol (|x| + |y| + |z| + 1), added to the slack)."""
    scan_v, gt_v = np.asarray(scan_v, np.float32), np.asarray(gt_v, np.float32)
    scan_t, gt_t = np.asarray(scan_t).reshape(-1, 3), np.asarray(gt_t).reshape(-1, 3)
    sp = sample(scan_v, scan_t, num_sample_points, seed).astype(np.float64)
    gp = sample(gt_v, gt_t, num_sample_points, seed + 1).astype(np.float64)
    moved = scale_normalize or align_method != "none"
    if scale_normalize:
        lo, hi = sp.min(0), sp.max(0)
        cur, tgt = np.linalg.norm(hi - lo), float(np.linalg.norm(gp.max(0) - gp.min(0)))
        if cur != 0:
            c = (lo + hi) * 0.5
            sp = (sp - c) * float(tgt / cur) + c
    icp_slack = 0.0
    if align_method in ("center", "icp"):
        sp = sp + (gp.mean(0) - sp.mean(0))
        if align_method == "icp":
            T = np.asarray(icp(sp.astype(np.float32), gp.astype(np.float32)), np.float64)
            icp_slack = np.sqrt(3.0) * icp_tol * (np.abs(sp).sum(1).max() + 1.0)
            sp = sp @ T[:3, :3].T + T[:3, 3]
    elif align_method != "none":
        raise ValueError(f"unknown alignment {align_method!r}")
    if moved and round_aligned:
        sp = sp.astype(np.float32).astype(np.float64)
    slack = lipschitz(max(np.abs(sp).max(), np.abs(gp).max())) + icp_slack if moved else 0.0

    g64 = gt_v.astype(np.float64)
    s64 = scan_v.astype(np.float64)
    g_ext, s_ext = g64.max(0) - g64.min(0), s64.max(0) - s64.min(0)
    thr = float(np.linalg.norm(g_ext) * 0.01) if threshold is None else float(threshold)
    if thr == 0.0:
        raise ValueError("zero-extent ground truth")

    s2g, g2s, p2s = nearest(sp, gp)[0], nearest(gp, sp)[0], nearest(sp, gt_v)[0]
    a, b, c = distance_stats(s2g, thr), distance_stats(g2s, thr), distance_stats(p2s, thr)
    precision, recall = a["count_below"] / len(sp), b["count_below"] / len(gp)
    f = float(2 * (precision * recall) / (precision + recall)) if precision + recall > 0 else 0.0

    so = sample(scan_v, scan_t, OVERLAP_SAMPLES, seed + 2)
    go = sample(gt_v, gt_t, OVERLAP_SAMPLES, seed + 3)
    od = nearest(so, go)[0]
    ratio = int(np.sum(od < OVERLAP_THRESHOLD)) / len(so)
    vs, vs_scale = volume(scan_v, scan_t)
    vg, vg_scale = volume(gt_v, gt_t)
    vo = vs * ratio
    union = vs + vg - vo
    sa, sa_scale = surface_area(scan_v, scan_t)
    ga, ga_scale = surface_area(gt_v, gt_t)

    m = dict(
        chamfer_distance=a["mean"] + b["mean"], hausdorff_distance=max(a["max"], b["max"]),
        mean_point_to_surface=c["mean"], median_point_to_surface=c["median"], std_point_to_surface=c["std"],
        max_point_to_surface=c["max"], precision=precision, recall=recall, f_score=f, volume_scan=vs, volume_gt=vg,
        volume_overlap=vo, volume_iou=vo / union if union > 0 else 0.0,
        bounding_box_ratio=tuple(float(s_ext[k] / g_ext[k]) if g_ext[k] > 0 else 0.0 for k in range(3)),
        center_offset=tuple(float(x) for x in ((s64.min(0) + s64.max(0)) * 0.5 - (g64.min(0) + g64.max(0)) * 0.5)),
        num_scan_points=len(sp), num_gt_points=len(gp), surface_area_scan=sa, surface_area_gt=ga,
        num_holes_scan=count_holes(scan_v, scan_t)[0], num_holes_gt=count_holes(gt_v, gt_t)[0], threshold=thr)

    n = max(len(sp), len(gp))
    tol = {k: 0.0 for k in EXACT}
    tol["threshold"] = tolerance("threshold", 1, thr)
    tol["chamfer_distance"] = tolerance("chamfer_distance", n, m["chamfer_distance"]) + 2 * slack
    tol["hausdorff_distance"] = tolerance("hausdorff_distance", 1, m["hausdorff_distance"]) + slack
    tol["mean_point_to_surface"] = tolerance("mean_point_to_surface", len(sp), c["mean"]) + slack
    tol["median_point_to_surface"] = tolerance("median_point_to_surface", 1, c["median"]) + slack
    tol["max_point_to_surface"] = tolerance("max_point_to_surface", 1, c["max"]) + slack
    tol["std_point_to_surface"] = tolerance("std_point_to_surface", len(sp), 3 * c["max"]) + 2 * slack
    tol["surface_area_scan"] = tolerance("surface_area_scan", len(scan_t), sa_scale)
    tol["surface_area_gt"] = tolerance("surface_area_gt", len(gt_t), ga_scale)
    tol["volume_scan"] = tolerance("volume_scan", len(scan_t), vs_scale)
    tol["volume_gt"] = tolerance("volume_gt", len(gt_t), vg_scale)
    tol["volume_overlap"] = tolerance("volume_overlap", len(scan_t), vs_scale)
    tol["volume_iou"] = 3 * (tol["volume_scan"] + tol["volume_gt"]) / union + 2.0 ** -51 if union > 0 else 0.0
    return m, tol


def compare(got, want, tol, label=""):
    """Assert every FIELDS entry (and the threshold) of ``got`` within ``tol`` of ``want``; prints each figure."""
    bad = []
    for k in FIELDS + ("threshold",):
        g, w = np.atleast_1d(np.asarray(got[k], np.float64)), np.atleast_1d(np.asarray(want[k], np.float64))
        err = float(np.abs(g - w).max())
        print(f"{label} {k}: got {got[k]!r} want {want[k]!r} |diff| {err:.3e} tol {tol[k]:.3e}")
        if not err <= tol[k]:
            bad.append((k, got[k], want[k], err, tol[k]))
    assert not bad, f"{label}: {bad}"


# ---------------------------------------------------------------------------- meshes the tests share
def octahedron(levels=3):
    """Octahedron subdivided ``levels`` times on the unit sphere: closed, consistently oriented."""
    v = [np.array(p, float) for p in [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]]
    t = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    for _ in range(levels):
        mid, t2 = {}, []

        def midpoint(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[k] = len(v) - 1
            return mid[k]

        for a, b, c in t:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            t2 += [(a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca)]
        t = t2
    return np.array(v).astype(np.float32), np.array(t, np.int32)


def grid(n, seed, noise=0.02, span=1.8, z=0.6):
    """Open n x n vertex grid over [-span / 2, span / 2]^2 at height z, noisy, two triangles per cell."""
    rng = np.random.default_rng(seed)
    x = np.linspace(-span / 2, span / 2, n)
    xs, ys = np.meshgrid(x, x, indexing="ij")
    v = np.stack([xs.reshape(-1), ys.reshape(-1), np.full(n * n, z)], 1) + noise * rng.standard_normal((n * n, 3))
    i = (np.arange(n - 1)[:, None] * n + np.arange(n - 1)[None, :]).reshape(-1)
    t = np.concatenate([np.stack([i, i + n, i + 1], 1), np.stack([i + 1, i + n, i + n + 1], 1)])
    return v.astype(np.float32), t.astype(np.int32)


def drop_cells(t, n, cells):
    """The grid's triangles without both triangles of the (row, column) cells."""
    nc = (n - 1) * (n - 1)
    keep = np.ones(len(t), bool)
    for r, c in cells:
        keep[r * (n - 1) + c] = keep[nc + r * (n - 1) + c] = False
    return t[keep]


def pinhole(v, t, tri, eps=1e-3):
    """Replace triangle ``tri`` by a ring of six triangles around a similar triangle eps times its size, left open."""
    A, B, C = (int(x) for x in t[tri])
    v64 = v.astype(np.float64)
    g = (v64[A] + v64[B] + v64[C]) / 3.0
    n = len(v)
    inner = np.stack([g + eps * (v64[k] - g) for k in (A, B, C)]).astype(np.float32)
    a, b, c = n, n + 1, n + 2
    ring = np.array([(A, B, b), (A, b, a), (B, C, c), (B, c, b), (C, A, a), (C, a, c)], np.int32)
    return np.concatenate([v, inner]), np.concatenate([np.delete(t, tri, 0), ring])


def strip(nt, seed=0):
    """nt triangles on a zig-zag of nt + 2 noisy vertices, consistently wound."""
    rng = np.random.default_rng(seed)
    k = np.arange(nt + 2)
    v = np.stack([0.5 * k, (k % 2).astype(float), np.zeros(nt + 2)], 1)
    v = (v + 0.1 * rng.standard_normal(v.shape)).astype(np.float32)
    i = np.arange(nt)
    t = np.where((i % 2 == 0)[:, None], np.stack([i, i + 1, i + 2], 1), np.stack([i + 1, i, i + 2], 1)).astype(np.int32)
    return v, t
