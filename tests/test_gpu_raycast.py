"""Ray casting (row f1: RaycastingScene for colour-aligned depth) vs the brute-force float64
oracle (oracle/mqr_oracle.c orc_raycast).  Parity against Embree itself is unpinned (Open3D is
not installed here); the bar: hit/miss agreement >= 99.9 % of rays, |dt| <= 1e-5 * t on common
hits, the fused pinhole path bit-identical to create_rays_pinhole + cast_rays.  The exact cases (edges,
vertices, axis-parallel rays, ties, duplicate Morton keys, deep trees) are in test_gpu_raycast_cases.py."""
import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def room_mesh():
    from mqr import synthetic
    from mqr.vbg import VoxelBlockGrid
    seq = synthetic.make_sequence("room", n=16, height=120, width=160, f=131.25, noise=True, seed=41)
    v = VoxelBlockGrid(voxel_size=0.02, block_resolution=8, block_count=512)
    v.integrate_frames(seq["depth"], seq["K"], seq["T_wc"], depth_scale=1.0, depth_max=4.0,
                       trunc_voxel_multiplier=6.0)
    m = v.extract_triangle_mesh(weight_threshold=1.5)
    return m.vertices.astype(np.float32), m.triangles.astype(np.int32), seq


def _cams(seq, idx):
    return seq["K"][idx].astype(np.float64), seq["T_wc"][idx].astype(np.float64)


def test_unit_square_known_answer():
    from mqr.raycasting import INVALID_ID, RaycastingScene
    V = np.array([[-1, -1, 2], [1, -1, 2], [1, 1, 2], [-1, 1, 2]], np.float32)
    T = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    s = RaycastingScene()
    assert s.add_triangles(V, T) == 0
    K = np.array([[100.0, 0, 49.5], [0, 100.0, 49.5], [0, 0, 1]])
    out = s.cast_pinhole(K, np.eye(4), 100, 100, full=True)
    t = out["t_hit"].numpy()
    assert np.all(t[:, :] == 2.0) or np.all(np.abs(t - 2.0) < 1e-6)
    n = out["primitive_normals"].numpy()
    assert np.allclose(np.abs(n[..., 2]), 1.0)
    # a ray pointing away misses
    r = np.array([[0, 0, 0, 0, 0, -1], [0, 0, 0, 0.1, 0.1, 1]], np.float32)
    o = s.cast_rays(r)
    assert np.isinf(o["t_hit"].numpy()[0]) and o["geometry_ids"].numpy()[0] == INVALID_ID
    assert o["t_hit"].numpy()[1] == np.float32(2.0) and o["primitive_ids"].numpy()[1] in (0, 1)


def test_pinhole_matches_oracle(room_mesh):
    from mqr.raycasting import RaycastingScene
    V, T, seq = room_mesh
    assert T.shape[0] > 5000
    s = RaycastingScene(device=0)
    s.add_triangles(V, T)
    K, Tw = _cams(seq, [1, 7])
    got = s.cast_pinhole(K, Tw, 80, 60)["t_hit"].numpy()
    for f in range(2):
        Kf = K[f].copy()
        Kf[:2] *= 0.5  # the cast above is at half resolution: scale the intrinsics the same way
        got_f = s.cast_pinhole(Kf, Tw[f], 80, 60)["t_hit"].numpy()
        rays = RaycastingScene.create_rays_pinhole(Kf, Tw[f], 80, 60).numpy()
        ref, _ = oracle.raycast(V, T, rays)
        hit_g, hit_r = np.isfinite(got_f), np.isfinite(ref)
        assert (hit_g == hit_r).mean() >= 0.999
        both = hit_g & hit_r
        assert both.sum() > 0.5 * got_f.size
        assert np.all(np.abs(got_f[both] - ref[both]) <= 1e-5 * ref[both] + 1e-6)
        # fused path == explicit rays, bit for bit
        assert np.array_equal(got_f, s.cast_rays(rays, full=False)["t_hit"].numpy())
    assert got.shape == (2, 60, 80)


def test_geometry_ids_and_primitives(room_mesh):
    from mqr.raycasting import RaycastingScene
    V, T, seq = room_mesh
    half = T.shape[0] // 2
    one, two = RaycastingScene(), RaycastingScene()
    one.add_triangles(V, T)
    assert two.add_triangles(V, T[:half]) == 0 and two.add_triangles(V, T[half:]) == 1
    assert two.triangle_count() == T.shape[0]
    K, Tw = _cams(seq, [3])
    a = one.cast_pinhole(K[0], Tw[0], 160, 120, full=True)
    b = two.cast_pinhole(K[0], Tw[0], 160, 120, full=True)
    assert np.array_equal(a["t_hit"].numpy(), b["t_hit"].numpy())
    hit = np.isfinite(a["t_hit"].numpy())
    g, p = b["geometry_ids"].numpy()[hit], b["primitive_ids"].numpy()[hit]
    glob = np.where(g == 0, p, p + half)
    pa = a["primitive_ids"].numpy()[hit]
    assert (glob == pa).mean() > 0.999
    # the hit lies on the reported triangle: barycentric reconstruction == ray point
    uv = a["primitive_uvs"].numpy()[hit]
    tri = V[T[pa]]
    pt = tri[:, 0] + uv[:, :1] * (tri[:, 1] - tri[:, 0]) + uv[:, 1:] * (tri[:, 2] - tri[:, 0])
    rays = RaycastingScene.create_rays_pinhole(K[0], Tw[0], 160, 120).numpy()[hit]
    ray_pt = rays[:, :3] + a["t_hit"].numpy()[hit][:, None] * rays[:, 3:]
    assert np.abs(pt - ray_pt).max() < 1e-4


def test_empty_scene_raises():
    from mqr.raycasting import RaycastingScene
    s = RaycastingScene()
    with pytest.raises(RuntimeError):
        s.cast_rays(np.zeros((1, 6), np.float32))


def test_raycast_in_color_view_matches_per_frame(room_mesh):
    from mqr.raycasting import RaycastingScene, raycast_in_color_view

    class DS:  # the attributes raycast_in_color_view reads from a CameraDataset
        def __init__(self, seq, n):
            self.widths = np.full(n, 160)
            self.heights = np.full(n, 120)
            self._K = seq["K"][:n]
            self.transforms = type("T", (), {"extrinsics_wc": seq["T_wc"][:n]})()

        def __len__(self):
            return len(self.widths)

        def get_intrinsic_matrices(self):
            k = self._K.copy()
            k[:, 0, 2] = self.widths - k[:, 0, 2]   # undone by compute_o3d_intrinsic_matrices
            return k

    V, T, seq = room_mesh
    s = RaycastingScene()
    s.add_triangles(V, T)
    ds = DS(seq, 5)
    maps = list(raycast_in_color_view(s, ds, batch=2))
    assert len(maps) == 5
    for i, m in enumerate(maps):
        ref = s.cast_pinhole(seq["K"][i].astype(np.float64), seq["T_wc"][i].astype(np.float64), 160, 120)
        assert np.array_equal(m, ref["t_hit"].numpy())
