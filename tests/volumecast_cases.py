"""Hand-built volumes and cameras for the volume ray-cast tests (tests/test_volumecast_ref.py on the CPU,
tests/test_gpu_volume_cast.py on the GPU).  Test infrastructure: the product never imports this.

A case is a dict: keys (N,3) int32, tsdf / weight (N,R,R,R) float32 [z][y][x], voxel_size, R, K (n,3,3),
T (n,4,4) world -> camera, H, W and kw (the cast's keyword arguments).  Lattice point X sits at X * voxel_size
(SURVEY A.1), so a field given on integer lattice coordinates is exact in float32.
"""
import numpy as np

VOXEL = 0.05  # R = 8: 0.4 m blocks
KW = dict(depth_scale=1.0, depth_min=0.1, depth_max=3.0, weight_threshold=3.0, trunc_voxel_multiplier=8.0)


def lattice(keys, R):
    """Integer lattice coordinates (X, Y, Z), each (N,R,R,R) indexed [z][y][x], of the blocks' voxels."""
    keys = np.asarray(keys, np.int64).reshape(-1, 3)
    a = np.arange(R)
    Z, Y, X = np.meshgrid(a, a, a, indexing="ij")
    return (keys[:, 0, None, None, None] * R + X[None], keys[:, 1, None, None, None] * R + Y[None],
            keys[:, 2, None, None, None] * R + Z[None])


def camera(eye, f, H, W, forward=(0.0, 0.0, 1.0), up=(0.0, -1.0, 0.0), centre=None):
    """(K, T_wc) of a pinhole camera at `eye` looking along `forward` (Open3D convention: x right, y down);
    principal point `centre` (cx, cy), by default the middle of the image."""
    fw = np.asarray(forward, np.float64)
    fw = fw / np.linalg.norm(fw)
    r = np.cross(fw, np.asarray(up, np.float64))
    r /= np.linalg.norm(r)
    d = np.cross(fw, r)
    Rcw = np.stack([r, d, fw], axis=1)  # camera -> world
    T = np.eye(4)
    T[:3, :3] = Rcw.T
    T[:3, 3] = -Rcw.T @ np.asarray(eye, np.float64)
    cx, cy = (W / 2.0, H / 2.0) if centre is None else centre
    K = np.array([[f, 0.0, cx], [0.0, f, cy], [0.0, 0.0, 1.0]])
    return K, T


def _case(keys, tsdf, weight, cams, H, W, R=8, voxel=VOXEL, **kw):
    keys = np.asarray(keys, np.int32).reshape(-1, 3)
    return dict(keys=keys, tsdf=np.ascontiguousarray(tsdf, np.float32), weight=np.ascontiguousarray(weight, np.float32),
                voxel_size=voxel, R=R, K=np.stack([c[0] for c in cams]), T=np.stack([c[1] for c in cams]), H=H, W=W,
                kw={**KW, **kw})


def _column(zs, x=0, y=0):
    return [(x, y, z) for z in zs]


def low_weight_crossing(H=5, W=7):
    """A first crossing at Z = 18 (0.9 m) whose voxels (Z 16..21) are under the weight threshold, negative
    values behind it up to Z = 21, then free space again and a valid crossing at Z = 34 (1.7 m)."""
    keys = _column(range(1, 5))
    _, _, Z = lattice(keys, 8)
    tsdf = np.clip(np.where(Z < 22, (18 - Z) * 0.125, (34 - Z) * 0.125), -1, 1)
    weight = np.where((Z >= 16) & (Z < 22), 1.0, 5.0)
    return _case(keys, tsdf, weight, [camera((0.2, 0.2, 0.0), 40.0, H, W)], H, W)


def absent_block_gap(H=5, W=7):
    """Observed free space in block z = 1, nothing in blocks z = 2, 3, the surface at Z = 36 (1.8 m) in block 4."""
    keys = _column((1, 4))
    _, _, Z = lattice(keys, 8)
    tsdf = np.clip((36 - Z) * 0.125, -1, 1)
    return _case(keys, tsdf, np.full(tsdf.shape, 5.0), [camera((0.2, 0.2, 0.0), 40.0, H, W)], H, W)


def seam_surface(H=5, W=7):
    """tsdf = 0 exactly on the last lattice layer (Z = 23, 1.15 m) of block z = 2; block z = 3 is absent."""
    keys = _column((1, 2))
    _, _, Z = lattice(keys, 8)
    tsdf = np.clip((23 - Z) * 0.125, -1, 1)
    return _case(keys, tsdf, np.full(tsdf.shape, 5.0), [camera((0.2, 0.2, 0.0), 40.0, H, W)], H, W)


def plane(H=5, W=7, extra_keys=(), shift=(0, 0, 0), **kw):
    """A plane at Z = 20 (1.0 m in front of the camera) in blocks z = 1, 2, optionally with more blocks
    (all free space) and the whole scene shifted by `shift` blocks."""
    keys = np.asarray(_column((1, 2)) + list(extra_keys), np.int64).reshape(-1, 3)
    _, _, Z = lattice(keys, 8)
    tsdf = np.clip((20 - Z) * 0.125, -1, 1)
    s = np.asarray(shift, np.int64)
    eye = np.array([0.2, 0.2, 0.0]) + s * 8 * VOXEL
    return _case(keys + s, tsdf, np.full(tsdf.shape, 5.0), [camera(eye, 40.0, H, W)], H, W, **kw)


def empty(H=5, W=7):
    z = np.zeros((0, 8, 8, 8), np.float32)
    return _case(np.zeros((0, 3), np.int32), z, z, [camera((0.2, 0.2, 0.0), 40.0, H, W)], H, W)


def step_cap(n_blocks=270):
    """All-positive tsdf (0.01, so every step is one voxel) in a 21.6 m row of blocks, 1 cm voxels, one ray down
    the row's axis: it is still inside the row when it has taken the march's step cap (2048 steps = 20.48 m)."""
    keys = _column(range(1, 1 + n_blocks))
    tsdf = np.full((n_blocks, 8, 8, 8), 0.01, np.float32)
    return _case(keys, tsdf, np.full(tsdf.shape, 5.0), [camera((0.04, 0.04, 0.0), 40.0, 1, 1, centre=(0.0, 0.0))], 1, 1, voxel=0.01,
                 depth_max=30.0)


def affine(H, W):
    """2 x 2 x 2 blocks, R = 8, 1/16 m voxels: tsdf = 0.5 + 0.125 x + 0.0625 y - z (metres; exact in float32 on
    the lattice), weights 5.  Three cameras: head-on, oblique, and inside the volume on the negative side."""
    voxel = 0.0625
    keys = [(x, y, z) for z in range(2) for y in range(2) for x in range(2)]
    X, Y, Z = lattice(keys, 8)
    tsdf = 0.5 + 0.125 * (X * voxel) + 0.0625 * (Y * voxel) - Z * voxel
    assert np.abs(tsdf).max() < 1
    cams = [camera((0.5, 0.5, -1.0), 1.25 * W, H, W),
            camera((0.9, 0.2, -0.9), 1.25 * W, H, W, forward=(-0.25, 0.2, 1.0)),
            camera((0.5, 0.5, 0.8), 1.25 * W, H, W)]
    return _case(keys, tsdf, np.full(tsdf.shape, 5.0), cams, H, W, voxel=voxel)


AFFINE_PLANE = (np.array([0.125, 0.0625, -1.0]), 0.5)  # tsdf = n . p + e


def random_volume(R, seed, voxel=None):
    """3 x 3 x 3 blocks around a negative-key corner with holes, weights around the threshold, and tsdf (a
    noisy ball) with +-0 and denormals."""
    rng = np.random.default_rng(seed)
    voxel = voxel or 0.4 / R
    base = np.array([-2, -1, 1])
    keys = np.array([(x, y, z) for z in range(3) for y in range(3) for x in range(3)]) + base
    keys = keys[rng.random(len(keys)) > 0.25]
    X, Y, Z = lattice(keys, R)
    c = (base + 1.5) * R
    r = np.sqrt((X - c[0]) ** 2 + (Y - c[1]) ** 2 + (Z - c[2]) ** 2)
    tsdf = np.clip((r - 0.9 * R) / (0.4 * R), -1, 1) + 0.05 * rng.standard_normal(r.shape)  # a noisy ball
    tsdf = np.clip(tsdf, -1, 1).astype(np.float32)
    pick = rng.random(tsdf.shape)
    tsdf[pick < 0.01] = 0.0
    tsdf[(pick >= 0.01) & (pick < 0.02)] = -0.0
    tsdf[(pick >= 0.02) & (pick < 0.025)] = 1e-42
    tsdf[(pick >= 0.025) & (pick < 0.03)] = -1e-42
    # mostly observed (3..6, the threshold 3 included), 3 % around or under it (0..3)
    weight = np.where(rng.random(tsdf.shape) < 0.03, rng.integers(0, 4, tsdf.shape),
                      rng.integers(3, 7, tsdf.shape)).astype(np.float32)
    centre = c * voxel
    return keys, tsdf, weight, voxel, centre


def random_cameras(centre, n, H, W, seed):
    rng = np.random.default_rng(seed)
    cams = []
    for _ in range(n):
        d = rng.standard_normal(3)
        d /= np.linalg.norm(d)
        eye = centre - 1.3 * d
        cams.append(camera(eye, 0.9 * W, H, W, forward=d + 0.1 * rng.standard_normal(3),
                           up=(0.1, -1.0, 0.2)))
    return cams


def random_case(R, seed, n, H, W, **kw):
    keys, tsdf, weight, voxel, centre = random_volume(R, seed)
    return _case(keys, tsdf, weight, random_cameras(centre, n, H, W, seed + 1), H, W, R=R, voxel=voxel, **kw)


# ---- the oracle sphere (tests/test_oracle_tsdf.py's geometry): 8 noise-free 64 x 48 frames, 2 cm voxels
SPHERE = dict(voxel_size=0.02, R=8, depth_max=3.0, trunc=4.0, weight_threshold=1.5)
# Largest |depth - analytic| of the float64 restatement over rays passing the sphere's centre within half its
# radius, measured by tests/test_volumecast_ref.py::test_sphere_depth (refine off and on: 0.05168 both; the
# median falls from 0.0110 to 0.0068 with refine).  Asserted there with a 2x margin; the GPU comparison with
# the mesh path builds on the same bound.
SPHERE_MEASURED_MAX = 0.05168
SPHERE_BOUND = 2 * SPHERE_MEASURED_MAX

_sphere = None


def sphere_volume():
    """(seq, keys, tsdf, weight) of the sphere integrated by the CPU oracle; computed once, read-only."""
    global _sphere
    if _sphere is None:
        import oracle
        from mqr import synthetic
        seq = synthetic.make_sequence("sphere", n=8, height=48, width=64, f=52.5, noise=False, seed=0)
        v = oracle.OracleVBG(SPHERE["voxel_size"], SPHERE["R"], 512)
        for i in range(8):
            v.integrate_frame(seq["depth"][i], seq["K"][i].astype(np.float64), seq["T_wc"][i].astype(np.float64), 1.0,
                              SPHERE["depth_max"], SPHERE["trunc"])
        keys, tsdf, weight = v.export()
        for a in (keys, tsdf, weight):
            a.setflags(write=False)
        _sphere = (seq, keys, tsdf, weight)
    return _sphere


def sphere_analytic(K, T, H, W, offset=0.0):
    """(analytic z-depth of the r = 0.5 m sphere (0 = miss), distance at which each ray passes the centre)
    for the rays through pixel (x + offset, y + offset)."""
    from mqr import synthetic
    Rm, t = T[:3, :3], T[:3, 3]
    eye = -Rm.T @ t
    Kc = np.array(K, np.float64)
    Kc[0, 2] -= offset
    Kc[1, 2] -= offset
    depth = synthetic.render_depth(synthetic.SCENES["sphere"], Kc, Rm.T, eye, H, W).astype(np.float64)
    yy, xx = np.mgrid[0:H, 0:W]
    dc = np.stack([(xx - Kc[0, 2]) / Kc[0, 0], (yy - Kc[1, 2]) / Kc[1, 1], np.ones((H, W))], -1) @ Rm
    dn = dc / np.linalg.norm(dc, axis=-1, keepdims=True)
    return depth, np.linalg.norm(np.cross(np.broadcast_to(eye, dn.shape), dn), axis=-1)


def sphere_color_dataset(n=2, H=48, W=64, f=240.0, side_value="left"):
    """A colour CameraDataset on the sphere capture's first n ring poses: long-lens views framed inside the
    sphere's well-observed front (every ray passes the centre within half the radius)."""
    from mqr.models import CameraDataset, CoordinateSystem, Transforms
    seq = sphere_volume()[0]
    o3d = seq["unity"].convert_coordinate_system(CoordinateSystem.OPEN3D, is_camera=True)
    ts = 1000 + 33 * np.arange(n)
    return CameraDataset(
        directory_relative_path=f"{side_value}_camera", image_file_names=np.array([f"{t}.png" for t in ts]),
        timestamps=ts, fx=np.full(n, f), fy=np.full(n, f), cx=np.full(n, W / 2.0), cy=np.full(n, H / 2.0),
        transforms=Transforms(CoordinateSystem.OPEN3D, o3d.positions[:n].copy(), o3d.rotations[:n].copy()),
        widths=np.full(n, W), heights=np.full(n, H))


# Views that contain the silhouette, for the comparison of the volume cast with the mesh cast: the capture's own
# focal length (one 2 cm voxel is 0.7 pixel at the sphere's distance, so the floor lookup's wider silhouette
# stays inside a one-pixel band), a 224 x 24 strip around the ring's horizon (the limbs are in view, the
# sphere's caps, which the ring sees only at grazing angles and which are holes in both paths, are not).
SILHOUETTE_VIEW = dict(n=2, H=24, W=224, f=52.5)
BAND_SHARE_MAX = 0.05


def silhouette_band(hit):
    """Pixels within one pixel (3 x 3 neighbourhood) of a hit / miss boundary of the (n, H, W) mask."""
    hit = np.asarray(hit, bool)
    p = np.pad(hit, ((0, 0), (1, 1), (1, 1)), mode="edge")
    H, W = hit.shape[1:]
    near_hit = np.zeros_like(hit)
    near_miss = np.zeros_like(hit)
    for dy in range(3):
        for dx in range(3):
            w = p[:, dy:dy + H, dx:dx + W]
            near_hit |= w
            near_miss |= ~w
    return near_hit & near_miss


def compare_with_mesh_cast(vol, msh, K, T, mesh_vertices, mesh_triangles):
    """The issue's comparison of two (n, H, W) depth maps with inf on a miss (volume cast, mesh cast): returns
    (share of pixels within one pixel of either silhouette, pixels outside that band that only one path hits,
    max |volume - mesh| over the rest, the mesh's own error there: brute force of tests/raycast_ref.py over the
    triangles against the analytic sphere)."""
    import raycast_ref as rr
    from mqr.raycasting import RaycastingScene
    hv, hm = np.isfinite(vol), np.isfinite(msh)
    band = silhouette_band(hv) | silhouette_band(hm)
    keep = ~band
    one_only = int(((hv != hm) & keep).sum())
    both = keep & hv & hm
    diff = float(np.abs(vol[both] - msh[both]).max())
    P = np.asarray(mesh_vertices, np.float32)[np.asarray(mesh_triangles)]
    n, H, W = vol.shape
    mesh_err = 0.0
    for f in range(n):
        rays = RaycastingScene.create_rays_pinhole(K[f], T[f], W, H).numpy()[both[f]]
        ana = sphere_analytic(K[f], T[f], H, W, offset=0.5)[0][both[f]]
        bf = rr.brute_force(P, rays).t
        assert (ana > 0).all()
        mesh_err = max(mesh_err, float(np.abs(bf - ana).max()))
    return float(band.mean()), one_only, diff, mesh_err
