"""Surface extraction (extract.hip) on volumes whose contents were chosen, against the CPU oracle.

The volumes come from tests/extract_cases.py; what they cover (all 256 cube cases in all 8 seam
classes, complete and incomplete 27-neighbourhoods, weights at the threshold, garbage under weight 0,
signed zeros, underflowing and denormal products, NaN, more blocks than one scan tile) is asserted
without a GPU in tests/test_extract_cases_ref.py from the same constants.

Every comparison is exact and ordered: the device's arrays against the oracle's, element for element,
floats by their bit patterns.  The oracle is given the blocks in the device's buffer order, so equal
arrays also pin the output order the header of extract.hip documents ((block, voxel, edge) for
vertices and points, (block, cube, triangle) for triangles), which mesh_passes and the owned
extraction's triangle prefix rely on.
"""
import ctypes

import numpy as np
import pytest

import extract_cases as ec
import oracle

pytestmark = pytest.mark.gpu

THR = ec.THRESHOLD


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_bits(what, got, want):
    """Exact, ordered equality of two float32 (or int32) arrays by bit pattern."""
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    g, w = (_bits(got), _bits(want)) if got.dtype == np.float32 else (got, want)
    if not np.array_equal(g, w):
        bad = np.nonzero((g != w).reshape(len(g), -1).any(axis=1))[0]
        i = int(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {len(g)} rows differ, first at {i}: {got[i]} != {want[i]}")


def _pair(keys, tsdf, weight, R):
    """The volume on the device and, with the blocks in the device's buffer order, in the oracle."""
    from mqr.vbg import VoxelBlockGrid
    vbg = VoxelBlockGrid(voxel_size=ec.VOXEL_SIZE, block_resolution=R, block_count=len(keys) + 16, device=0)
    vbg.import_blocks(keys, tsdf, weight)
    dk, dt, dw = vbg.export()
    # the import stored what it was given (signed zeros, denormals and NaN included)
    od, oi = np.lexsort(dk.T[::-1]), np.lexsort(keys.T[::-1])
    assert np.array_equal(dk[od], keys[oi])
    assert np.array_equal(_bits(dt)[od], _bits(tsdf)[oi]) and np.array_equal(_bits(dw)[od], _bits(weight)[oi])
    ref = oracle.OracleVBG(ec.VOXEL_SIZE, R, len(keys) + 16)
    ref.import_blocks(dk, dt, dw)
    return vbg, ref, dk


def _check_mesh(vbg, ref, thr=THR):
    m = vbg.extract_triangle_mesh(weight_threshold=thr)
    ov, on, ot = ref.extract_mesh(thr)
    gv, gn, gt = m.vertices, m.vertex_normals, m.triangles
    _same_bits("triangles", gt, ot)
    _same_bits("vertex positions", gv, ov)
    _same_bits("vertex normals", gn, on)
    return gv, gn, gt


def _check_points(vbg, ref, thr=THR):
    pc = vbg.extract_point_cloud(weight_threshold=thr)
    op, on = ref.extract_points(thr)
    gp, gn = pc.points, pc.normals
    _same_bits("point positions", gp, op)
    _same_bits("point normals", gn, on)
    return gp, gn


@pytest.mark.parametrize("R", [8, 16, 12, 4])
def test_all_cases_all_seams(R):
    """Dense all-valid volumes that hold every cube case in every seam class: the triangle table, its
    packed form, the per-cube counts and the cube index, inside blocks and across faces, edges and
    corners of blocks.  At R = 16 a block has ~6000 vertices (above kRowMap: the binary row search).
    The second threshold's extraction runs with the first one's counts as speculative capacities."""
    for G, seed in ec.DENSE[R]:
        vol = ec.dense_signs(R, G, seed)
        vbg, ref, _ = _pair(*vol[:3], R)
        gv, _, gt = _check_mesh(vbg, ref, THR)
        assert len(gt) == ec.triangles_per_block(vol, vol.keys).sum() > 1000
        _check_mesh(vbg, ref, 0.0)
        gp, _ = _check_points(vbg, ref, THR)
        assert len(gp) == len(gv)  # no zeros, all valid: every crossing edge is a vertex and a point


@pytest.mark.parametrize("R", [8, 16, 12])
def test_mixed_weights_absent_blocks_and_garbage(R):
    """Weights around the threshold (1.5 itself is not valid), a quarter of the blocks of two slabs
    removed, one block without any neighbour, arbitrary tsdf under weight 0: cube validity across absent
    neighbours, and the normal components carried from the voxel's previous edge where a side's block
    is absent -- next to blocks whose 26 neighbours all exist (the 13-tap path)."""
    G, seed, drop = ec.MIXED[R]
    vol = ec.dense_signs(R, G, seed, weights="mixed", drop=drop)
    vbg, ref, _ = _pair(*vol[:3], R)
    _, _, gt = _check_mesh(vbg, ref)
    assert len(gt) == ec.triangles_per_block(vol, vol.keys).sum() > 1000
    gp, _ = _check_points(vbg, ref)
    assert len(gp) > 1000
    _check_mesh(vbg, ref, 0.0)  # now only weight 0 is invalid: 1.0 and 1.5 count


@pytest.mark.parametrize("R", [8, 12])
def test_signed_zeros(R):
    """+0.0 and -0.0 are not negative: ratio-0 and ratio-1 vertices, some coincident, and fewer points
    than vertices (0 * x < 0 is false)."""
    G, seed = ec.ZEROS[R]
    vol = ec.dense_signs(R, G, seed, zeros=0.03)
    vbg, ref, _ = _pair(*vol[:3], R)
    gv, _, _ = _check_mesh(vbg, ref)
    gp, _ = _check_points(vbg, ref)
    assert 0 < len(gp) < len(gv)
    assert len(np.unique(_bits(gv), axis=0)) < len(gv)


@pytest.mark.parametrize("R", [8, 16, 12])
def test_underflowing_and_denormal_products(R):
    """tsdf * 2^-100: the mesh is the unscaled volume's (positions and triangles; ratios are quotients)
    and no product tsdf_i * tsdf_o is below zero (each underflows to -0), so there is no point.
    tsdf * 2^-130: denormal operands in the ratio's division and in the product test."""
    G, seed = ec.SCALED[R]
    vol = ec.dense_signs(R, G, seed)
    vbg, ref, _ = _pair(*vol[:3], R)
    gv, _, gt = _check_mesh(vbg, ref)
    assert len(_check_points(vbg, ref)[0]) == len(gv)
    small = ec.scaled(vol, -100)
    vbg, ref, _ = _pair(*small[:3], R)
    sv, _, st = _check_mesh(vbg, ref)
    _same_bits("scaled volume's positions", sv, gv)
    _same_bits("scaled volume's triangles", st, gt)
    assert len(vbg.extract_point_cloud(weight_threshold=THR).points) == 0
    assert len(ref.extract_points(THR)[0]) == 0
    tiny = ec.scaled(vol, -130)
    vbg, ref, _ = _pair(*tiny[:3], R)
    _, _, tt = _check_mesh(vbg, ref)
    _same_bits("denormal volume's triangles", tt, gt)
    _check_points(vbg, ref)


@pytest.mark.parametrize("R", [8, 12])
def test_nan_is_neither_negative_nor_positive(R):
    """2 % NaN tsdf on valid voxels: counts and triangle indices equal the oracle's; positions and
    normals are NaN where the oracle's are and bit-equal elsewhere (payloads are not compared)."""
    G, seed = ec.NANS[R]
    vol = ec.dense_signs(R, G, seed, nans=0.02)
    assert 0.01 < np.isnan(vol.tsdf).mean() < 0.03
    vbg, ref, _ = _pair(*vol[:3], R)
    m = vbg.extract_triangle_mesh(weight_threshold=THR)
    pc = vbg.extract_point_cloud(weight_threshold=THR)
    ov, on, ot = ref.extract_mesh(THR)
    op, opn = ref.extract_points(THR)
    _same_bits("triangles", m.triangles, ot)
    assert np.isnan(ov).any() and np.isnan(on).any()
    for what, got, want in (("vertex positions", m.vertices, ov), ("vertex normals", m.vertex_normals, on),
                            ("point positions", pc.points, op), ("point normals", pc.normals, opn)):
        assert got.shape == want.shape, (what, got.shape, want.shape)
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan), what
        assert np.array_equal(_bits(got)[~nan], _bits(want)[~nan]), what
    assert not np.isnan(op).any() and len(op) > 0  # a NaN product is not < 0: no point lies on a NaN edge


def test_more_blocks_than_one_scan_tile():
    """8492 blocks, two thirds of them without output: the count scan's tile loop and carry, the
    emission's early returns and its LDS row map (few outputs per block).  The second extraction of each
    kind emits into capacities guessed from the first."""
    R, n, seed = ec.SPARSE
    keys, tsdf, weight, has_output = ec.sparse_many(R, n, seed)
    vbg, ref, dk = _pair(keys, tsdf, weight, R)
    flag = dict(zip(map(tuple, keys.tolist()), has_output.tolist()))
    out_dev = np.array([flag[tuple(k)] for k in dk.tolist()])
    assert out_dev[:ec.SCAN_TILE].any() and out_dev[ec.SCAN_TILE:].any()
    for _ in range(2):
        _, _, gt = _check_mesh(vbg, ref)
        gp, _ = _check_points(vbg, ref)
    assert len(gt) > 0 and len(gp) > 0


def _extract_owned_raw(vbg, n_owned, thr=THR):
    """mqr_extract_mesh_owned's arrays as they are (mqr.distributed.extract_mesh_owned re-indexes)."""
    from mqr import _lib
    g = ctypes.c_void_p()
    _lib.call("mqr_extract_mesh_owned", vbg.handle, float(thr), int(n_owned), ctypes.byref(g))
    try:
        nv, nt = ctypes.c_int64(), ctypes.c_int64()
        _lib.call("mqr_geom_counts", g, ctypes.byref(nv), ctypes.byref(nt))
        pos = np.empty((nv.value, 3), np.float32)
        nrm = np.empty((nv.value, 3), np.float32)
        tri = np.empty((nt.value, 3), np.int32)
        _lib.call("mqr_geom_copy", g, _lib.ptr(pos), _lib.ptr(nrm), _lib.ptr(tri) if nt.value else None,
                  _lib.MQR_HOST)
    finally:
        _lib._lib.mqr_geom_free(g)
    return pos, nrm, tri


def test_owned_extraction_is_a_triangle_prefix():
    """Owned-block extraction on a dense volume: all the vertices, and the triangles of the cubes whose
    origin lies in the first n_owned blocks -- the first T(n_owned) rows of the full mesh's, T from the
    numpy cube classification and the table's per-case counts."""
    R, G, seed = ec.OWNED
    vol = ec.dense_signs(R, G, seed)
    vbg, ref, dk = _pair(*vol[:3], R)
    fv, fn, ft = _check_mesh(vbg, ref)
    per_block = ec.triangles_per_block(vol, dk)
    size = vbg.size()
    assert size == G ** 3 and per_block.sum() == len(ft)
    for n_owned in (0, 1, size // 2, size):
        pos, nrm, tri = _extract_owned_raw(vbg, n_owned)
        T = int(per_block[:n_owned].sum())
        assert (T == 0) == (n_owned == 0) and (T == len(ft)) == (n_owned == size)
        _same_bits(f"vertex positions (n_owned={n_owned})", pos, fv)
        _same_bits(f"vertex normals (n_owned={n_owned})", nrm, fn)
        _same_bits(f"triangles (n_owned={n_owned})", tri, ft[:T])


@pytest.mark.parametrize("R", sorted(ec.SPHERES))
def test_sphere(R):
    """An analytic sphere through block faces, edges and corners: the oracle's mesh, and on the device's
    own arrays a closed surface (every directed edge once, its reverse once; V - E + F = 2) on the
    sphere with radial normals -- a check of the indices that does not go through the oracle."""
    G = ec.SPHERES[R]
    radius = ec.SPHERE_RADIUS * R
    vol = ec.sphere(R, G, radius)
    vbg, ref, _ = _pair(*vol[:3], R)
    gv, gn, gt = _check_mesh(vbg, ref)
    _check_points(vbg, ref)
    watertight, euler = ec.mesh_topology(len(gv), gt)
    assert watertight and euler == 2
    assert len(np.unique(gt)) == len(gv)
    # linear interpolation of a distance field of curvature 1 / r is off by about h^2 / (8 r) = 0.011
    # voxel at r = 11.3 (less at R = 12): 0.05 voxel leaves room, one voxel would hide a wrong tap
    err, dot = ec.sphere_errors(gv, gn, radius)
    assert err < 0.05 and dot > 0.99, (err, dot)


@pytest.mark.parametrize("kind", ["mesh", "points"])
def test_block_resolution_one_is_refused(kind):
    """At R = 1 the extraction tile [-1, R + 1] would reach two blocks away: both entry points refuse
    the volume, naming its resolution, before anything is launched."""
    from mqr import _lib
    from mqr.vbg import VoxelBlockGrid
    vbg = VoxelBlockGrid(voxel_size=ec.VOXEL_SIZE, block_resolution=1, block_count=16, device=0)
    with pytest.raises(_lib.MqrError, match=r"block_resolution >= 2, got 1"):
        if kind == "mesh":
            vbg.extract_triangle_mesh(weight_threshold=THR)
        else:
            vbg.extract_point_cloud(weight_threshold=THR)
