"""Row f1 / C5: per-vertex colour projection vs the CPU oracle, on a mesh extracted from a fused
room capture, with the colour-aligned depth ray-cast from that mesh as the reference does
(raycast_in_color_view):

* mqr_color_vertices (visibility + average) vs oracle.color_vertices;
* mqr_color_map (run_rigid_optimizer's complete colouring with the poses as given: RGBD depth
  truncation, depth-discontinuity masks, float64 means, 3-NN fill of unseen vertices) vs
  oracle.color_map -- with keyframes that see only part of the room, so masks and the fill act.

Both restate Open3D's colour-map code as recalled (parity unpinned against Open3D itself, which is
not installed).  Bit-identical colours and counts; colours close to the analytic texture the
frames were rendered with wherever a keyframe sees the vertex."""
import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scene():
    from mqr import _lib, synthetic
    from mqr.vbg import VoxelBlockGrid
    _lib.load()
    seq = synthetic.make_sequence("room", n=24, height=240, width=320, f=262.5, noise=True, seed=4)
    vbg = VoxelBlockGrid(voxel_size=0.01, block_resolution=16, block_count=512)
    vbg.integrate_frames(seq["depth"], seq["K"], seq["T_wc"], depth_scale=1.0, depth_max=4.0,
                         trunc_voxel_multiplier=10.0)
    mesh = vbg.extract_triangle_mesh(weight_threshold=1.5)
    poses = synthetic.room_loop_poses(24)
    key = list(range(0, 24, 3))  # keyframes
    K = seq["K"][key].astype(np.float64)
    T = seq["T_wc"][key].astype(np.float64)
    Ko = K[0].copy()
    imgs = np.stack([synthetic.render_color("room", Ko, poses[i][0], poses[i][1], 240, 320) for i in key])
    return mesh, imgs, K, T


@pytest.fixture(scope="module")
def partial_view(scene):
    """3 of the 8 keyframes, which see only part of the room, and their colour-aligned depth cast from the mesh."""
    from mqr.raycasting import RaycastingScene
    mesh, imgs, K, T = scene
    sel = [0, 3, 6]
    imgs, K, T = imgs[sel], K[sel], T[sel]
    rs = RaycastingScene()
    rs.add_triangles(mesh.vertices, mesh.triangles)
    t_hit = rs.cast_pinhole(K, T, 320, 240)["t_hit"].numpy()
    return mesh, imgs, K, T, t_hit


def test_color_matches_oracle(scene):
    from mqr.color import MARGIN, MAX_DEPTH, VISIBILITY_THRESHOLD, project_vertex_colors
    from mqr.raycasting import RaycastingScene
    from mqr import synthetic
    mesh, imgs, K, T = scene
    gc, gn = project_vertex_colors(mesh, imgs, K, T, complete=False)
    rs = RaycastingScene()
    rs.add_triangles(mesh.vertices, mesh.triangles)
    depth = rs.cast_pinhole(K, T, 320, 240)["t_hit"].numpy()
    oc, on = oracle.color_vertices(mesh.vertices, imgs, depth, K, T, MAX_DEPTH, VISIBILITY_THRESHOLD, MARGIN)
    assert np.array_equal(gn, on)
    assert np.array_equal(gc, oc)
    seen = gn > 0
    assert seen.mean() > 0.3
    err = np.abs(gc[seen] - synthetic.texture(mesh.vertices[seen])).mean()
    assert err < 0.05, err


def test_color_thresholds_and_empty(scene):
    from mqr.color import color_vertices
    mesh, imgs, K, T = scene
    N, H, W = imgs.shape[:3]
    far = np.full((N, H, W), 10.0, np.float32)  # every depth beyond max_depth: nothing visible
    c, n = color_vertices(mesh.vertices[:1000], imgs, far, K, T)
    assert (n == 0).all() and (c == 0).all()
    c, n = color_vertices(np.zeros((0, 3), np.float32), imgs, far, K, T)
    assert c.shape == (0, 3)


def test_color_map_masks_and_fill_match_oracle(partial_view):
    """The complete colouring with 3 of the 8 keyframes: the depth-boundary masks drop samples at
    silhouettes (counts below the unmasked average's), and the vertices no keyframe samples take
    the mean of their 3 nearest sampled vertices -- all bit-identical to the oracle."""
    from mqr.color import color_map, color_vertices
    from mqr import synthetic
    mesh, imgs, K, T, t_hit = partial_view
    gc, gn = color_map(mesh.vertices, imgs, t_hit, K, T)
    oc, on = oracle.color_map(mesh.vertices, imgs, t_hit, K, T)
    assert np.array_equal(gn, on)
    assert np.array_equal(gc, oc)
    _, n_plain = color_vertices(mesh.vertices, imgs, t_hit, K, T)
    assert (gn <= n_plain).all() and (gn < n_plain).sum() > 100, "masks drop silhouette samples"
    unseen = gn == 0
    assert 0.2 < unseen.mean() < 0.95
    assert (np.abs(gc[unseen]).sum(1) > 0).mean() > 0.99, "unseen vertices are filled from their neighbours"
    seen = ~unseen
    assert np.abs(gc[seen] - synthetic.texture(mesh.vertices[seen])).mean() < 0.05


@pytest.mark.parametrize("knn", [1, 2, 8])
def test_color_map_fill_matches_oracle_for_other_knn(partial_view, knn):
    """The same partial view filled from 1, 2 and 8 neighbours: one search kernel serves every knn, and the
    oracle check above exercises it at knn = 3 only.  Counts and colours bit-identical to the oracle."""
    from mqr.color import color_map
    mesh, imgs, K, T, t_hit = partial_view
    gc, gn = color_map(mesh.vertices, imgs, t_hit, K, T, knn=knn)
    oc, on = oracle.color_map(mesh.vertices, imgs, t_hit, K, T, knn=knn)
    assert np.array_equal(gn, on)
    assert np.array_equal(gc, oc)
    unseen = gn == 0
    assert 0.2 < unseen.mean() < 0.95
    assert (np.abs(gc[unseen]).sum(1) > 0).mean() > 0.99, "unseen vertices are filled from their neighbours"
