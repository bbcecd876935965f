"""Vectorised numpy restatement of the reference's raw mesh quality metrics
(scripts/evaluation/evaluate_fbx_quality.py, compute_raw_metrics_for_mesh; rules in DESIGN §2.5).

``raw_metrics(vertices, triangles, colors=None)`` returns ``(metrics, scales)``: the reference's fields
(without name / path) and, for the tolerances, the largest ``|element|`` of the population behind each
mean / std field.  All arithmetic is float64; a sum of squares is ``(x^2 + y^2) + z^2``.  Also the mesh
builders the GPU tests share.
"""
import numpy as np

FLOAT_FIELDS = ("mean_aspect_ratio", "mean_skewness", "boundary_edge_ratio", "normal_deviation_avg_deg",
                "dihedral_min_deg", "dihedral_max_deg", "dihedral_penalty", "surface_roughness",
                "vertex_density_stddev", "uncolored_vertex_ratio", "color_gradient_stddev")
INT_FIELDS = ("degenerate_triangles", "non_manifold_edges", "component_count", "total_edges", "num_vertices",
              "num_triangles")
BOOL_FIELDS = ("is_single_component", "has_color", "is_manifold", "is_watertight")
FIELDS = ("mean_aspect_ratio", "mean_skewness", "degenerate_triangles", "non_manifold_edges", "boundary_edge_ratio",
          "component_count", "total_edges", "normal_deviation_avg_deg", "dihedral_min_deg", "dihedral_max_deg",
          "dihedral_penalty", "surface_roughness", "is_single_component", "vertex_density_stddev", "has_color",
          "uncolored_vertex_ratio", "color_gradient_stddev", "is_manifold", "is_watertight", "num_vertices",
          "num_triangles")
# fields that pass through an acos: the extra angle slack of the tolerance model (degrees)
ANGLE_FIELDS = ("normal_deviation_avg_deg", "dihedral_min_deg", "dihedral_max_deg", "dihedral_penalty",
                "surface_roughness")
ANGLE_SLACK_DEG = 1e-5
REL = 1e-11


def tolerance(field, scales):
    """|difference| allowed for a float field: 1e-11 of its population's largest element (reordered float64
    sums of <= 1e4 terms: n * 2^-53 ~ 1e-12, x10), plus 1e-5 degrees for fields behind an acos (an argument k
    ulp off moves acos by at most sqrt(2 k 2^-52) rad = 8.5e-7 deg * sqrt(k); 1e-5 covers k ~ 100), and
    1e-5 / 60 for the mean skewness (an angle divided by 60 degrees).  boundary_edge_ratio is exact."""
    tol = REL * scales.get(field, 0.0)
    if field in ANGLE_FIELDS:
        tol += ANGLE_SLACK_DEG
    if field == "mean_skewness":
        tol += ANGLE_SLACK_DEG / 60.0
    return tol


def _norm(a):
    return np.sqrt((a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1]) + a[..., 2] * a[..., 2])


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _unit(a):
    """a / |a|, a zero vector stays zero (Eigen's normalize())."""
    z = (a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1]) + a[..., 2] * a[..., 2]
    out = a.copy()
    nz = z > 0
    out[nz] = a[nz] / np.sqrt(z[nz])[:, None]
    return out


def _angle(a, b):
    an = a / (_norm(a) + 1e-12)[:, None]
    bn = b / (_norm(b) + 1e-12)[:, None]
    return np.arccos(np.clip(_dot(an, bn), -1.0, 1.0))


def triangle_normals(v, t):
    return _cross(v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]])


def vertex_normals(v, t):
    """Sum of the unnormalised triangle normals per vertex, added in ascending triangle index, corners
    0, 1, 2 within a triangle (np.add.at is sequential in index order), then normalised."""
    tn = triangle_normals(v, t)
    vn = np.zeros_like(v)
    np.add.at(vn, t.reshape(-1), np.repeat(tn, 3, axis=0))
    return _unit(vn)


def _components(nv, u, w):
    parent = np.arange(nv)

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b in zip(u.tolist(), w.tolist()):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    return int(sum(1 for i in range(nv) if parent[i] == i))


def raw_metrics(vertices, triangles, colors=None):
    v = np.asarray(vertices, np.float64)
    t = np.asarray(triangles, np.int64)
    nv, nt = len(v), len(t)
    if nv == 0 or nt == 0:
        raise ValueError("mesh has no geometry")
    m, scales = {}, {}
    # ---- shape
    p0, p1, p2 = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    tn = _cross(p1 - p0, p2 - p0)
    rep = (t[:, 0] == t[:, 1]) | (t[:, 1] == t[:, 2]) | (t[:, 2] == t[:, 0])
    ok = ~(rep | (0.5 * _norm(tn) < 1e-10))
    q0, q1, q2 = p0[ok], p1[ok], p2[ok]
    m["degenerate_triangles"] = int(nt - ok.sum())
    if ok.any():
        e = np.stack([_norm(q1 - q0), _norm(q2 - q1), _norm(q0 - q2)], 1)
        ar = e.max(1) / np.maximum(e.min(1), 1e-12)
        ang = np.stack([_angle(q1 - q0, q2 - q0), _angle(q2 - q1, q0 - q1), _angle(q0 - q2, q1 - q2)], 1)
        th = np.radians(60.0)
        sk = np.clip(np.maximum((th - ang.min(1)) / th, (ang.max(1) - th) / th), 0.0, 1.0)
        m["mean_aspect_ratio"], m["mean_skewness"] = float(np.mean(ar)), float(np.mean(sk))
        scales["mean_aspect_ratio"], scales["mean_skewness"] = float(ar.max()), float(sk.max())
    else:
        m["mean_aspect_ratio"], m["mean_skewness"] = 1.0, 0.0
    # ---- topology: entries (i0,i1), (i1,i2), (i2,i0) of every triangle, u == v dropped
    a = t.reshape(-1)
    b = t[:, [1, 2, 0]].reshape(-1)
    face = np.repeat(np.arange(nt), 3)
    keep = a != b
    lo, hi, face = np.minimum(a, b)[keep], np.maximum(a, b)[keep], face[keep]
    key = lo * (nv + 1) + hi
    order = np.argsort(key, kind="stable")
    key, face = key[order], face[order]
    uk, start, mult = np.unique(key, return_index=True, return_counts=True)
    eu, ev = uk // (nv + 1), uk % (nv + 1)
    total = len(uk)
    boundary = int((mult == 1).sum())
    m["total_edges"] = total
    m["non_manifold_edges"] = int((mult > 2).sum())
    m["boundary_edge_ratio"] = float(boundary / total) if total else 0.0
    m["component_count"] = _components(nv, eu, ev)
    m["is_manifold"] = m["non_manifold_edges"] == 0
    m["is_watertight"] = bool(m["is_manifold"] and boundary == 0 and m["component_count"] == 1)
    m["is_single_component"] = m["component_count"] == 1
    # ---- smoothness
    vn = vertex_normals(v, t)
    tnn = _unit(tn)
    if total:
        n1, n2 = vn[eu], vn[ev]
        dev = np.degrees(np.arccos(np.clip(_dot(n1, n2) / ((_norm(n1) + 1e-12) * (_norm(n2) + 1e-12)), -1.0, 1.0)))
        m["normal_deviation_avg_deg"] = float(np.mean(dev))
        scales["normal_deviation_avg_deg"] = float(dev.max())
    else:
        m["normal_deviation_avg_deg"] = 0.0
    two = mult == 2
    if two.any():
        f0, f1 = face[start[two]], face[start[two] + 1]
        dih = np.degrees(_angle(tnn[f0], tnn[f1]))
        m["dihedral_min_deg"], m["dihedral_max_deg"] = float(dih.min()), float(dih.max())
        m["dihedral_penalty"] = max(0.0, 30.0 - m["dihedral_min_deg"]) + max(0.0, m["dihedral_max_deg"] - 170.0)
        m["surface_roughness"] = float(np.std(dih))
        scales["surface_roughness"] = float(dih.max())
    else:
        m["dihedral_min_deg"], m["dihedral_max_deg"] = 180.0, 0.0
        m["dihedral_penalty"], m["surface_roughness"] = 0.0, 0.0
    # ---- completeness
    mn = v.min(0)
    ext = v.max(0) - mn
    ext[ext == 0.0] = 1e-6
    vox = ext / 10
    vol = (vox[0] * vox[1]) * vox[2]
    if vol <= 0.0:
        vol = 1.0
    idx = np.clip(np.floor((v - mn) / vox).astype(int), 0, 9)
    counts = np.bincount(idx[:, 0] * 100 + idx[:, 1] * 10 + idx[:, 2], minlength=1000)
    dens = counts[counts > 0].astype(float) / vol
    m["vertex_density_stddev"] = float(np.std(dens))
    scales["vertex_density_stddev"] = float(dens.max())
    # ---- colour
    m["has_color"] = colors is not None
    if colors is None:
        m["uncolored_vertex_ratio"], m["color_gradient_stddev"] = 1.0, 0.0
    else:
        c = np.asarray(colors, np.float64)
        m["uncolored_vertex_ratio"] = 0.0
        if total:
            g = _norm(c[eu] - c[ev])
            m["color_gradient_stddev"] = float(np.std(g))
            scales["color_gradient_stddev"] = float(g.max())
        else:
            m["color_gradient_stddev"] = 0.0
    m["num_vertices"], m["num_triangles"] = nv, nt
    return m, scales


# ---------------------------------------------------------------------- meshes the tests share
def grid_mesh(n, m, rng=None, noise=0.0, step=(1.0, 1.0), z=0.0):
    """(n x m) vertex grid, two triangles per cell; float32 coordinates."""
    ys, xs = np.meshgrid(np.arange(m, dtype=np.float32) * np.float32(step[1]),
                         np.arange(n, dtype=np.float32) * np.float32(step[0]))
    v = np.stack([xs.reshape(-1), ys.reshape(-1), np.full(n * m, z, np.float32)], 1).astype(np.float32)
    if rng is not None:
        v = (v + (noise * rng.standard_normal(v.shape)).astype(np.float32)).astype(np.float32)
    i = (np.arange(n - 1)[:, None] * m + np.arange(m - 1)[None, :]).reshape(-1)
    t = np.concatenate([np.stack([i, i + m, i + 1], 1), np.stack([i + 1, i + m, i + m + 1], 1)]).astype(np.int32)
    return v, t


def strip_mesh(nt, seed=0):
    """nt triangles on a zig-zag of nt + 2 noisy vertices, with colours."""
    rng = np.random.default_rng(seed)
    k = np.arange(nt + 2)
    v = np.stack([0.5 * k, (k % 2).astype(float), np.zeros(nt + 2)], 1)
    v = (v + 0.1 * rng.standard_normal(v.shape)).astype(np.float32)
    i = np.arange(nt)
    t = np.where((i % 2 == 0)[:, None], np.stack([i, i + 1, i + 2], 1), np.stack([i + 1, i, i + 2], 1)).astype(np.int32)
    c = rng.random((nt + 2, 3)).astype(np.float32)
    return v, t, c
