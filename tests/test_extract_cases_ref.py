"""What the constructed extraction volumes (tests/extract_cases.py) cover, and the oracle's known
answers on them.  No GPU: tests/test_gpu_extract_cases.py extracts the same volumes (the same
constants) on the device against the oracle."""
import numpy as np
import pytest

import extract_cases as ec
import oracle


def _oracle_vbg(keys, tsdf, weight, R):
    ref = oracle.OracleVBG(ec.VOXEL_SIZE, R, len(keys) + 16)
    ref.import_blocks(keys, tsdf, weight)
    return ref


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("R", sorted(ec.DENSE))
def test_dense_volumes_cover_every_case_in_every_seam_class(R):
    """All 256 cube cases occur among the valid cubes of each of the 8 seam classes (cube inside the
    block; crossing +x, +y, +z; the three block edges; the 8-block corner), at both thresholds the
    device test uses (all weights are 3.0)."""
    hist = np.zeros((8, 256), np.int64)
    for G, seed in ec.DENSE[R]:
        vol = ec.dense_signs(R, G, seed)
        assert np.abs(vol.keys).max() <= 64 and vol.keys.min() < 0 < vol.keys.max()
        assert len(vol.keys) == G ** 3 and len(np.unique(vol.keys, axis=0)) == G ** 3
        mag = np.abs(vol.tsdf)
        assert 0.05 <= mag.min() and mag.max() <= 1.0
        for thr in (ec.THRESHOLD, 0.0):
            assert ec.weight_ok(vol, thr).all()
        hist += ec.case_histogram(vol.sign, ec.weight_ok(vol), R)
    assert (hist > 0).sum(axis=1).tolist() == [256] * 8
    # the corner class is the enumerated one: one cube per inner block corner
    assert hist[7].sum() == sum((G - 1) ** 3 for G, _ in ec.DENSE[R])


def test_case_coverage_counts_a_known_grid():
    """One negative voxel in a 2-block cube of R = 2: the eight cubes around it are the eight
    single-corner cases, each in the seam class of its origin."""
    sign = np.zeros((4, 4, 4), bool)
    sign[2, 2, 2] = True
    ok = np.ones((4, 4, 4), bool)
    hist = ec.case_histogram(sign, ok, 2)
    assert hist[:, 0].sum() == 27 - 8 and hist.sum() == 27
    for k, (dx, dy, dz) in enumerate(ec.mc_tables.VTX_SHIFTS):
        cls = dx | dy << 1 | dz << 2   # origin 2 - d: at R-1 = 1 iff d == 1
        assert hist[cls, 1 << k] == 1
    ok[0, 0, 0] = False
    assert ec.case_histogram(sign, ok, 2).sum() == 26
    assert ec.case_coverage(sign, ok, 2).tolist() == [2, 2, 2, 2, 2, 2, 2, 1]  # class 7 is the one cube at (1, 1, 1)


@pytest.mark.parametrize("R", sorted(ec.MIXED))
def test_mixed_volumes_have_complete_and_incomplete_blocks(R):
    G, seed, drop = ec.MIXED[R]
    vol = ec.dense_signs(R, G, seed, weights="mixed", drop=drop)
    complete = ec.complete_blocks(vol.present)
    assert complete.sum() >= 8 and (vol.present & ~complete).sum() >= 8
    assert ec.isolated_blocks(vol.present).sum() >= 1
    assert len(vol.keys) == vol.present.sum() < G ** 3
    low = (vol.weight <= ec.THRESHOLD).mean()
    assert 0.08 <= low <= 0.12
    assert set(np.unique(vol.weight).tolist()) == set(ec.MIXED_WEIGHTS)
    dead = vol.weight == 0
    assert np.abs(vol.tsdf[dead]).max() > 40 and np.abs(vol.tsdf[~dead]).max() <= 1.0
    # cubes at the threshold itself are not valid: coverage is counted with weight > thr
    ok = ec.weight_ok(vol)
    assert not ok[vol.wgrid == ec.THRESHOLD].any()
    assert (ec.case_coverage(vol.sign, ok, R)[:7] > 128).all()


def test_sparse_sheet_has_output_on_both_sides_of_the_scan_tile():
    R, n, seed = ec.SPARSE
    keys, tsdf, weight, has_output = ec.sparse_many(R, n, seed)
    assert n > ec.SCAN_TILE and len(keys) == n == len(np.unique(keys, axis=0))
    assert has_output[:ec.SCAN_TILE].any() and has_output[ec.SCAN_TILE:].any()
    assert not has_output[ec.SCAN_TILE - 1] or not has_output[ec.SCAN_TILE]  # an empty block next to the carry
    ref = _oracle_vbg(keys, tsdf, weight, R)
    pos, _, tri = ref.extract_mesh(ec.THRESHOLD)
    # the owning block of every vertex (ratios lie in [0.047, 0.953]: no vertex sits on a voxel)
    vox = np.floor(pos.astype(np.float64) / ec.VOXEL_SIZE + 0.01).astype(np.int64)
    blk = vox // R
    index = {tuple(k): i for i, k in enumerate(keys.tolist())}
    owner = np.array([index[tuple(b)] for b in np.unique(blk, axis=0).tolist()])
    assert (owner < ec.SCAN_TILE).any() and (owner >= ec.SCAN_TILE).any()
    assert set(np.nonzero(has_output)[0].tolist()) <= set(owner.tolist())
    assert len(owner) < n // 2 and len(tri) > 0


@pytest.mark.parametrize("R", sorted(ec.SPHERES))
def test_oracle_sphere_is_a_closed_surface(R):
    """Watertight, Euler characteristic 2, vertices on the sphere, normals radial."""
    G = ec.SPHERES[R]
    radius = ec.SPHERE_RADIUS * R
    vol = ec.sphere(R, G, radius)
    assert vol.keys.min() == -(G // 2) and vol.keys.max() == G // 2 - 1
    hist = ec.case_histogram(vol.sign, ec.weight_ok(vol), R)
    assert (hist[:, 1:255].sum(axis=1) > 0).all()  # the surface crosses faces, edges and corners of blocks
    pos, nrm, tri = _oracle_vbg(*vol[:3], R).extract_mesh(ec.THRESHOLD)
    watertight, euler = ec.mesh_topology(len(pos), tri)
    assert watertight and euler == 2
    assert len(np.unique(tri)) == len(pos)
    # linear interpolation of a distance field of curvature 1 / r is off by about h^2 / (8 r) = 0.011
    # voxel at r = 11.3 (less at R = 12): 0.05 voxel leaves room, one voxel would hide a wrong tap
    err, dot = ec.sphere_errors(pos, nrm, radius)
    assert err < 0.05 and dot > 0.99, (err, dot)


def test_oracle_scaled_volume_keeps_the_mesh_and_loses_the_points():
    """tsdf * 2^-100: ratios are quotients, so positions and triangles do not move; every product
    tsdf_i * tsdf_o underflows to -0, which is not < 0, so no point is extracted."""
    R = 8
    G, seed = ec.SCALED[R]
    vol = ec.dense_signs(R, G, seed)
    small = ec.scaled(vol, -100)
    assert np.array_equal(small.tsdf < 0, vol.tsdf < 0) and (small.tsdf != 0).all()
    a = _oracle_vbg(*vol[:3], R)
    b = _oracle_vbg(*small[:3], R)
    pa, _, ta = a.extract_mesh(ec.THRESHOLD)
    pb, _, tb = b.extract_mesh(ec.THRESHOLD)
    assert len(ta) > 10000
    assert np.array_equal(_bits(pa), _bits(pb)) and np.array_equal(ta, tb)
    assert len(a.extract_points(ec.THRESHOLD)[0]) == len(pa)
    assert len(b.extract_points(ec.THRESHOLD)[0]) == 0
    # denormal tsdf: still a mesh of the same connectivity
    tiny = ec.scaled(vol, -130)
    assert ((np.abs(tiny.tsdf) < np.finfo(np.float32).tiny) & (tiny.tsdf != 0)).all()
    pc, _, tc = _oracle_vbg(*tiny[:3], R).extract_mesh(ec.THRESHOLD)
    assert np.array_equal(tc, ta) and np.isfinite(pc).all()


def test_oracle_signed_zeros_are_not_negative():
    R = 8
    G, seed = ec.ZEROS[R]
    vol = ec.dense_signs(R, G, seed, zeros=0.03)
    z = vol.tsdf == 0
    neg0 = z & np.signbit(vol.tsdf)
    assert 0.02 < neg0.mean() < 0.04 and 0.02 < (z & ~neg0).mean() < 0.04
    assert not (vol.tsdf[z] < 0).any()
    ref = _oracle_vbg(*vol[:3], R)
    pos, nrm, tri = ref.extract_mesh(ec.THRESHOLD)
    # the triangle count is the table's for the case of every valid cube, zeros counted as positive
    assert len(tri) == ec.triangles_per_block(vol, vol.keys).sum()
    assert np.isfinite(pos).all() and np.isfinite(nrm).all()
    # a zero gives ratio 0 on the voxel's own edges and ratio 1 on the three edges that end at it: up to
    # six vertices sit on the voxel together
    _, cnt = np.unique(_bits(pos), axis=0, return_counts=True)
    assert (cnt > 1).any() and cnt.max() <= 6
    # points need tsdf_i * tsdf_o < 0, which no zero satisfies; the mesh needs only a sign change
    pts, _ = ref.extract_points(ec.THRESHOLD)
    assert 0 < len(pts) < len(pos)


@pytest.mark.parametrize("R", sorted(ec.DENSE))
def test_oracle_triangle_count_is_the_tables(R):
    """The numpy cube classification (used for the owned-extraction prefix) agrees with the oracle:
    triangles = sum of TRI_COUNT[case] over the valid cubes."""
    for vol in (ec.dense_signs(R, 3, 11), ec.dense_signs(R, 4, 11, weights="mixed", drop=0.25)):
        _, _, tri = _oracle_vbg(*vol[:3], R).extract_mesh(ec.THRESHOLD)
        assert len(tri) == ec.triangles_per_block(vol, vol.keys).sum() > 0
