"""CPU restatement of the registration rules (DESIGN "registration rules"; ISSUE sections 1 and 4) in
float64 with numpy and scipy's cKDTree: test infrastructure only, never imported by the product.

Besides its results every correspondence pass reports two margins, over the source points that have
a correspondence or miss one:
  tie     the smallest gap between a source point's nearest and second-nearest target distance
  radius  the smallest |d - radius| of a nearest distance
While both stay far above float64 rounding, the set of correspondences does not depend on how the
distance is rounded, and an exact comparison of inlier counts with the device is meaningful.
"""
import itertools

import numpy as np
from scipy.spatial import cKDTree


# ---------------------------------------------------------------- inputs
def surface(n, seed, noise=0.0):
    """Three bumpy walls of a 2 m room corner, n/3 uniform samples each, shifted by -1 m per axis."""
    rng = np.random.default_rng(seed)
    m = n // 3
    walls = []
    for k in range(3):
        u = rng.uniform(0.0, 2.0, m)
        v = rng.uniform(0.0, 2.0, m)
        w = 0.05 * np.sin(5 * u) * np.cos(4 * v) + 0.03 * np.sin(11 * u + 1.3 * v)
        walls.append(np.stack([(u, v, w), (u, w, v), (w, u, v)][k], 1))
    p = np.concatenate(walls) - 1.0
    if noise:
        p = p + rng.normal(0.0, noise, p.shape)
    return np.ascontiguousarray(p, np.float32)


def motion(rx_deg, ry_deg, rz_deg, t):
    a, b, c = np.deg2rad([rx_deg, ry_deg, rz_deg])
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    Rz = np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
    T = np.eye(4)
    T[:3, :3] = Rz @ Ry @ Rx
    T[:3, 3] = t
    return T


def apply(T, p):
    """float32 cloud moved by T (computed in float64, rounded once)."""
    return np.ascontiguousarray(p.astype(np.float64) @ T[:3, :3].T + T[:3, 3], np.float32)


TRUE_MOTION = motion(2.0, -1.5, 2.5, (0.03, -0.02, 0.025))


def icp_pair():
    """The 6000-point pair of the ICP tests: (source, target, true source-to-target motion)."""
    src = surface(6000, 1)
    tgt = apply(TRUE_MOTION, surface(6000, 2, noise=0.002))
    return src, tgt, TRUE_MOTION


# ---------------------------------------------------------------- rules
def voxel_down(points, v):
    """key = floor(p / v) in float64; members summed in ascending original index in float64, divided
    by the count, rounded to float32; rows in ascending (kx, ky, kz)."""
    p = np.asarray(points, np.float32)
    if not v > 0:
        return p
    key = np.floor(p.astype(np.float64) / float(v)).astype(np.int64)
    uniq, inv = np.unique(key, axis=0, return_inverse=True)  # lexicographic: kx, then ky, then kz
    inv = inv.reshape(-1)
    cnt = np.bincount(inv, minlength=len(uniq)).astype(np.float64)
    # np.bincount adds its weights one by one in index order: the fixed summation order of the rule
    out = np.stack([np.bincount(inv, weights=p[:, a].astype(np.float64), minlength=len(uniq)) / cnt
                    for a in range(3)], 1)
    return np.ascontiguousarray(out, np.float32)


class Margins:
    def __init__(self):
        self.tie = np.inf
        self.radius = np.inf

    def update(self, d1, d2, radius):
        near = d1 <= radius
        if near.any():
            self.tie = min(self.tie, float((d2[near] - d1[near]).min()))
        if len(d1):
            self.radius = min(self.radius, float(np.abs(d1 - radius).min()))


def correspondences(src, tree, tgt64, T, radius, margins=None):
    """(q, t, d) of the source points that have a target within the radius under T."""
    q = src.astype(np.float64) @ T[:3, :3].T + T[:3, 3]
    k = 2 if len(tgt64) > 1 else 1
    d, j = tree.query(q, k=k)
    if k == 1:
        d, j = d[:, None], j[:, None]
        d = np.concatenate([d, np.full_like(d, np.inf)], 1)
    if margins is not None:
        margins.update(d[:, 0], d[:, 1], radius)
    ok = d[:, 0] <= radius
    return q[ok], tgt64[j[ok, 0]], d[ok, 0]


def _stats(n_src, d):
    n = len(d)
    return n / n_src, (float(np.sqrt(np.sum(d * d) / n)) if n else 0.0)


def evaluate(source, target, radius, T=None, every_k=1, margins=None):
    T = np.eye(4) if T is None else np.asarray(T, np.float64)
    s, t = (source[::every_k], target[::every_k]) if every_k > 1 else (source, target)
    t64 = t.astype(np.float64)
    q, tt, d = correspondences(s, cKDTree(t64), t64, T, radius, margins)
    fit, rmse = _stats(len(s), d)
    return dict(fitness=fit, inlier_rmse=rmse, count=len(d))


def kabsch(q, t, perm=None):
    if perm is not None:
        q, t = q[perm], t[perm]
    mq, mt = q.sum(0) / len(q), t.sum(0) / len(t)
    H = (q - mq).T @ (t - mt)
    U, _, Vt = np.linalg.svd(H)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T))])
    R = Vt.T @ D @ U.T
    dT = np.eye(4)
    dT[:3, :3] = R
    dT[:3, 3] = mt - R @ mq
    return dT


def icp(source, target, voxel_sizes, max_dists, max_iters, rel_fitness, rel_rmse, T_init=None, permute_seed=None):
    """Multi-scale point-to-point ICP by the rules of DESIGN.  Returns a dict: transformation,
    fitness, inlier_rmse, num_iterations (per level), counts (inliers of every pass, per level),
    margins."""
    T = np.eye(4) if T_init is None else np.array(T_init, np.float64)
    rng = np.random.default_rng(permute_seed) if permute_seed is not None else None
    margins = Margins()
    iters, counts = [], []
    fit = rmse = 0.0
    for l, v in enumerate(voxel_sizes):
        s, t = voxel_down(source, v), voxel_down(target, v)
        t64 = t.astype(np.float64)
        tree = cKDTree(t64)
        prev_fit = prev_rmse = 0.0
        n_it, cl = 0, []
        for _ in range(int(max_iters[l])):
            q, tt, d = correspondences(s, tree, t64, T, max_dists[l], margins)
            fit, rmse = _stats(len(s), d)
            n_it += 1
            cl.append(len(d))
            if len(d) < 3:
                break
            T = kabsch(q, tt, rng.permutation(len(q)) if rng is not None else None) @ T
            if abs(prev_fit - fit) < rel_fitness[l] and abs(prev_rmse - rmse) < rel_rmse[l]:
                break
            prev_fit, prev_rmse = fit, rmse
        iters.append(n_it)
        counts.append(cl)
    return dict(transformation=T, fitness=fit, inlier_rmse=rmse, num_iterations=iters, counts=counts,
                margins=margins)


def information(source, target, radius, T, margins=None):
    t64 = target.astype(np.float64)
    _, t, _ = correspondences(source, cKDTree(t64), t64, np.asarray(T, np.float64), radius, margins)
    x, y, z = t[:, 0], t[:, 1], t[:, 2]
    o, l = np.zeros_like(x), np.ones_like(x)
    G = np.stack([np.stack([o, z, -y, l, o, o], 1), np.stack([-z, o, x, o, l, o], 1),
                  np.stack([y, -x, o, o, o, l], 1)], 1)  # (n, 3, 6)
    return np.einsum("nia,nib->ab", G, G)


# ---------------------------------------------------------------- pose graph
def pair_edge(clouds, source_node, target_node, config, uncertain, margins=None):
    """refine_fragment_poses.py:122-193 on host clouds.  Returns (edge dict | None, why): why is
    'pre_filter', 'not_converged' or 'kept'."""
    s, t = clouds[source_node], clouds[target_node]
    if config.use_pre_filtering and uncertain:
        r = evaluate(s, t, config.pre_filter_max_corr_dist, np.eye(4), int(config.pre_filter_every_k_points), margins)
        if r["fitness"] < config.pre_filter_fitness_threshold or \
                r["inlier_rmse"] > config.pre_filter_inlier_rmse_threshold:
            return None, "pre_filter"
    r = icp(s, t, config.icp_voxel_sizes, config.max_corr_dists, config.max_iterations, config.relative_fitnesses,
            config.relative_rmses)
    if margins is not None:
        margins.tie = min(margins.tie, r["margins"].tie)
        margins.radius = min(margins.radius, r["margins"].radius)
    converged = r["fitness"] >= config.icp_fitness_threshold or r["inlier_rmse"] <= config.icp_inlier_rmse_threshold
    if uncertain and not converged:
        return None, "not_converged"
    info = information(s, t, config.max_corr_dists[-1], r["transformation"], margins)
    return dict(source_node_id=source_node, target_node_id=target_node, transformation=r["transformation"],
                information=info, uncertain=uncertain, confidence=1.0, num_iterations=r["num_iterations"]), "kept"


def pair_list(counts_by_side):
    """(source node, target node, uncertain) in the reference's order: odometry, then combinations."""
    pairs, base = [], 0
    for c in counts_by_side:
        pairs += [(base + i, base + i + 1, False) for i in range(c - 1)]
        base += c
    pairs += [(a, b, True) for a, b in itertools.combinations(range(base), 2)]
    return pairs


def pose_graph(clouds_by_side, config, margins=None):
    """refine_fragment_poses.py:196-271.  clouds_by_side: {side: [cloud, ...]}.  Returns (edges,
    decisions): decisions[i] is 'kept' / 'pre_filter' / 'not_converged' for pair i."""
    clouds = [c for cs in clouds_by_side.values() for c in cs]
    edges, why = [], []
    for a, b, unc in pair_list([len(cs) for cs in clouds_by_side.values()]):
        e, w = pair_edge(clouds, a, b, config, unc, margins)
        why.append(w)
        if e is not None:
            edges.append(e)
    return edges, why
