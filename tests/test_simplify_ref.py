"""Hand-built cases for tests/simplify_ref.py, the numpy restatement of the vertex-clustering rule,
and the parts of mqr.downsample_mesh that need no GPU: its scalar rules, its voxel-size search and the command
line.  The expected values of the scalar rules are worked out by hand from the text of the reference's
``scripts/downsample_fbx_mesh.py`` (lines 143-150 and 232-238); the reference function itself cannot run here
(it needs Open3D and Aspose.3D, and neither is installed).  The same cases run on the device in
tests/test_gpu_mesh_simplify.py."""
import numpy as np
import pytest

import simplify_ref as sr


def f32(x):
    return np.array(x, np.float32).reshape(-1, 3)


# ---- hand-built meshes (shared with the GPU file) -------------------------------------------------------------
def cube_case():
    """The eight corners of a unit cube, twelve triangles, in one cell of size 4."""
    v = f32([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)])
    t = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6],
                  [0, 6, 4], [1, 5, 7], [1, 7, 3]], np.int32)
    return v, t, 4.0


def isolated_case():
    """Every vertex in a cell of its own (spacing 1, cells of 0.25); triangles start at any corner."""
    v = f32([[3, 0, 0], [0, 0, 0], [1, 0, 0], [0, 2, 0], [0, 0, 5], [2, 2, 2]])
    t = np.array([[0, 1, 2], [2, 1, 3], [5, 4, 3], [4, 3, 0], [3, 5, 1]], np.int32)
    return v, t, 0.25


def boundary_case():
    """Powers of two with voxel_size 0.25 and min bound 0: origin = -0.125, so x lies in cell
    floor((x + 0.125) / 0.25), every step exact.  0.125 is exactly on the face between cells 0 and 1."""
    xs = [0.0, -0.0, 0.125, 0.0625, 0.25, 0.375, 0.5, 1.0, 2.0, 0.124999994]
    v = f32([[x, 0.0, 0.0] for x in xs])
    want_cell = [0, 0, 1, 0, 1, 2, 2, 4, 8, 0]
    return v, 0.25, want_cell


def negative_case():
    """Negative coordinates and -0.0, min bound -2: origin = -2.125."""
    xs = [-2.0, -1.875, -1.0, -0.0, 0.0, -0.125, 0.5]
    v = f32([[x, x, x] for x in xs])
    want_x = [0, 1, 4, 8, 8, 8, 10]  # floor((x + 2.125) / 0.25)
    return v, 0.25, want_x


def triangle_case():
    """Nine isolated vertices plus a twin of vertex 0 (same cell): collapsed, duplicate, rotated duplicate and
    opposite-orientation triangles."""
    v = f32([[i, 0, 0] for i in range(9)] + [[0.01, 0, 0]])
    t = np.array([
        [4, 5, 6],   # 0 kept, stored as (4, 5, 6)
        [0, 9, 3],   # 1 collapsed: vertices 0 and 9 share a cell
        [1, 2, 3],   # 2 kept
        [1, 2, 3],   # 3 duplicate, same rotation
        [5, 6, 4],   # 4 duplicate of 0 given as (b, c, a)
        [3, 2, 1],   # 5 opposite orientation of 2: another triple, kept as (1, 3, 2)
        [6, 4, 5],   # 6 duplicate of 0 given as (c, a, b)
        [9, 1, 2],   # 7 kept: (0, 1, 2) through the twin
        [0, 1, 2],   # 8 duplicate of 7
        [7, 7, 8],   # 9 collapsed in the input already
        [2, 1, 3],   # 10 the orientation of 5 from another corner: duplicate of 5
    ], np.int32)
    want = np.array([[4, 5, 6], [1, 2, 3], [1, 3, 2], [0, 1, 2]], np.int32)
    return v, t, 0.25, want


# ---- the rule ------------------------------------------------------------------------------------------------
def test_cube_in_one_cell_has_the_exact_mean():
    v, t, vs = cube_case()
    pos, nrm, col, tri, st = sr.simplify(v, t, vs, normals=v * 2, colors=v * 0.25)
    assert np.array_equal(pos, f32([0.5, 0.5, 0.5])) and np.array_equal(nrm, f32([1, 1, 1]))
    assert np.array_equal(col, f32([0.125, 0.125, 0.125]))
    assert tri.shape == (0, 3) and tri.dtype == np.int32
    assert st.tolist() == [8, 1, 12, 12, 0, 0, 8, 1]
    assert sr.cluster_count(v, vs) == 1


def test_isolated_vertices_come_back_with_rotated_triangles():
    v, t, vs = isolated_case()
    pos, _, _, tri, st = sr.simplify(v, t, vs)
    assert np.array_equal(pos.view(np.uint32), v.view(np.uint32))
    assert tri.tolist() == [[0, 1, 2], [1, 3, 2], [3, 5, 4], [0, 4, 3], [1, 3, 5]]
    # the widest axis is z, 0 .. 5: floor((5 + 0.125) / 0.25) = 20, so 21 cells (x has 13, y has 9)
    assert st.tolist() == [6, 6, 5, 0, 0, 5, 1, 21]


def test_isolated_axis_cells_is_the_widest_axis():
    v, t, vs = isolated_case()
    assert sr.cells(v, vs)[1].tolist() == [13, 9, 21]


def test_boundary_exact_coordinates():
    v, vs, want = boundary_case()
    c, axis = sr.cells(v, vs)
    assert c[:, 0].tolist() == want and (c[:, 1:] == 0).all()
    assert axis.tolist() == [9, 1, 1]
    pos, _, _, _, st = sr.simplify(v, None, vs)
    # first appearance: cells 0, 1, 2, 4, 8; cell 0 holds 0.0, -0.0, 0.0625 and the float32 below 0.125
    assert st[1] == 5 and st[6] == 4
    want0 = np.float32((((0.0 + -0.0) + 0.0625) + float(np.float32(0.124999994))) / 4.0)
    assert pos[0, 0] == want0 and pos[1, 0] == np.float32((0.125 + 0.25) / 2.0)
    assert pos[2, 0] == np.float32((0.375 + 0.5) / 2.0) and pos[3, 0] == 1.0 and pos[4, 0] == 2.0


def test_negative_coordinates_and_minus_zero():
    v, vs, want = negative_case()
    c, _ = sr.cells(v, vs)
    assert c[:, 0].tolist() == want and c[:, 1].tolist() == want
    pos, _, _, _, st = sr.simplify(v, None, vs)
    assert st[1] == 5
    # -0.0, 0.0 and -0.125 share a cell: the mean of the x column is (-0.0 + 0.0 - 0.125) / 3
    assert pos[3, 0] == np.float32(-0.125 / 3.0) and pos[0, 0] == -2.0
    # a cell whose only member is -0.0 sums from +0: the mean is +0.0
    one = sr.simplify(f32([[-0.0, -0.0, -0.0], [1, 1, 1]]), None, 0.25)[0]
    assert not np.signbit(one[0]).any()


def test_triangle_rules():
    v, t, vs, want = triangle_case()
    pos, _, _, tri, st = sr.simplify(v, t, vs)
    assert tri.tolist() == want.tolist()
    assert st.tolist() == [10, 9, 11, 2, 5, 4, 2, 33]
    assert pos[0, 0] == np.float32((0.0 + float(np.float32(0.01))) / 2.0)


def test_no_triangles():
    v, _, vs = isolated_case()
    pos, nrm, col, tri, st = sr.simplify(v, None, vs, colors=v)
    assert tri.shape == (0, 3) and nrm is None and np.array_equal(col, v) and st[2] == st[5] == 0


def test_first_appearance_orders():
    # cells visited in the order 2, 0, 2, 1, 0: output vertices are cells 2, 0, 1
    v = f32([[2, 0, 0], [0, 0, 0], [2.1, 0, 0], [1, 0, 0], [0.1, 0, 0]])
    t = np.array([[3, 0, 1], [4, 3, 2], [1, 3, 0]], np.int32)
    pos, _, _, tri, st = sr.simplify(v, t, 1.0)
    # origin -0.5: cells floor(x + 0.5) = 2, 0, 2, 1, 0
    assert pos[:, 0].tolist() == [np.float32((2.0 + float(np.float32(2.1))) / 2), np.float32(0.1) / 2, 1.0]
    # triangles map to (2, 0, 1), (1, 2, 0), (1, 2, 0): one triple (0, 1, 2), kept at its first index
    assert tri.tolist() == [[0, 1, 2]] and st[4] == 2


def test_errors():
    v, t, vs = isolated_case()
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            sr.simplify(v, t, bad)
    with pytest.raises(ValueError):
        sr.simplify(v[:0], None, vs)
    nan = v.copy()
    nan[2, 1] = np.nan
    with pytest.raises(ValueError):
        sr.simplify(nan, t, vs)
    for idx in (len(v), -1):
        bt = t.copy()
        bt[1, 2] = idx
        with pytest.raises(ValueError):
            sr.simplify(v, bt, vs)
    with pytest.raises(sr.GridTooFine):
        sr.simplify(f32([[0, 0, 0], [1, 0, 0]]), None, 1e-7)
    # 2^21 - 1 cells pass, 2^21 do not: x = 2^21 - 2 lies in cell floor(2^21 - 2 + 0.5) = 2^21 - 2
    assert sr.cells(f32([[0, 0, 0], [2 ** 21 - 2, 0, 0]]), 1.0)[1][0] == 2 ** 21 - 1
    with pytest.raises(sr.GridTooFine):
        sr.cells(f32([[0, 0, 0], [2 ** 21 - 1, 0, 0]]), 1.0)


def test_ordered_sum_is_sequential():
    """Values whose float64 sum depends on the order: 1, then 2^53 ones-in-the-last-place apart."""
    vals = f32([[2.0 ** 60, 1.0, -2.0 ** 60]] * 1)
    x = np.concatenate([f32([[2.0 ** 60, 0, 0]]), f32([[1.0, 0, 0]] * 40), f32([[-2.0 ** 60, 0, 0]])])
    got = sr.ordered_means(x, np.zeros(len(x), np.int64), 1)
    acc = 0.0
    for a in x[:, 0].astype(np.float64):
        acc += a
    assert got[0, 0] == np.float32(acc / len(x)) and vals.shape == (1, 3)
    # two cells interleaved, more than 16 cells in all, so the rank-by-rank path runs too
    rng = np.random.default_rng(0)
    y = (rng.standard_normal((500, 3)) * 1e6).astype(np.float32)
    mp = rng.integers(0, 40, 500)
    mp[:40] = np.arange(40)
    got = sr.ordered_means(y, mp, 40)
    for j in (0, 7, 39):
        acc = np.zeros(3)
        for row in y[mp == j].astype(np.float64):
            acc = acc + row
        assert np.array_equal(got[j], (acc / (mp == j).sum()).astype(np.float32))


# ---- downsample_mesh: scalar rules -------------------------------------------------------------------------
def test_scalar_rules_by_hand():
    from mqr.downsample_mesh import reference_voxel_size, target_vertex_count
    # int(1000 * (10 / 100.0)) = 100; 33.3 / 100.0 is 0.33299999999999996 in float64 and 1000 times that is
    # 332.99999999999994, which int() truncates to 332 (the reference's expression, evaluated as it stands);
    # the floor of 4 vertices
    for n, pct, want in ((1000, 10, 100), (1000, 33.3, 332), (7, 50, 4), (3, 100, 4), (20580000, 1, 205800),
                         (1000, 0.05, 4), (1000, 25, 250), (1000, 100, 1000)):
        assert target_vertex_count(n, pct) == want == sr.target_count(n, pct)
    for bad in (0, -5, 100.0001, 250):
        with pytest.raises(ValueError, match="between 0 and 100"):
            target_vertex_count(1000, bad)
        with pytest.raises(ValueError):
            sr.target_count(1000, bad)
    # diagonal of a 3 x 4 x 12 box is 13; target 1000 -> 13 / 10 * 1.2 up to the cube root's rounding
    want = 13.0 / (1000 ** (1 / 3)) * 1.2
    assert reference_voxel_size(13.0, 1000) == want == sr.v_ref(13.0, 1000) and abs(want - 1.56) < 1e-12
    assert sr.diagonal(f32([[0, 0, 0], [3, 4, 12], [1, 1, 1]])) == 13.0


def test_early_return_is_the_same_object_and_value_errors():
    from mqr.downsample_mesh import downsample_mesh
    from mqr.geometry import TriangleMesh
    v, t, _ = cube_case()
    mesh = TriangleMesh(v, np.zeros_like(v), t)
    assert downsample_mesh(mesh, 100) is mesh       # target 8 >= 8
    small = TriangleMesh(v[:4], np.zeros_like(v[:4]), t[:1])
    assert downsample_mesh(small, 1) is small       # target max(4, 0) = 4 >= 4
    pair = (v, t)
    assert downsample_mesh(pair, 100) is pair       # any mesh holder comes back as it is


def test_percent_and_rule_errors_need_no_gpu():
    from mqr.downsample_mesh import downsample_mesh
    from mqr.geometry import TriangleMesh
    v, t, _ = cube_case()
    mesh = TriangleMesh(v, np.zeros_like(v), t)
    for bad in (0, -1, 100.5):
        with pytest.raises(ValueError, match="between 0 and 100"):
            downsample_mesh(mesh, bad)
    with pytest.raises(ValueError, match="voxel_size_rule"):
        downsample_mesh(mesh, 50, voxel_size_rule="quadric")
    flat = TriangleMesh(np.ones((40, 3), np.float32), np.zeros((40, 3), np.float32), np.array([[0, 1, 2]], np.int32))
    with pytest.raises(ValueError, match="zero size"):
        downsample_mesh(flat, 50)                    # host bounds: the diagonal is 0 before anything is uploaded
    bad_v = np.ones((40, 3), np.float32)
    bad_v[3, 1] = np.inf
    with pytest.raises(ValueError, match="not finite"):
        downsample_mesh(TriangleMesh(bad_v, np.zeros_like(bad_v), np.array([[0, 1, 2]], np.int32)), 50)
    with pytest.raises(NotImplementedError):
        mesh.simplify_vertex_clustering(0.5, contraction="Quadric")
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="voxel_size"):
            mesh.simplify_vertex_clustering(bad)


# ---- the voxel-size search -----------------------------------------------------------------------------------
def surface(n, seed):
    """n points on a wavy sheet: the occupied cells grow like 1 / v^2, not 1 / v^3."""
    rng = np.random.default_rng(seed)
    xy = rng.random((n, 2))
    return np.column_stack([xy, 0.1 * np.sin(6 * xy[:, 0]) * np.cos(5 * xy[:, 1])]).astype(np.float32)


@pytest.mark.parametrize("n,pct", [(4000, 50), (4000, 10), (4000, 1), (300, 25), (5, 90)])
def test_fit_is_never_worse_than_v_ref(n, pct):
    from mqr.downsample_mesh import fit_voxel_size
    from mqr.geometry import GridTooFine
    v = surface(n, n + pct)
    target = sr.target_count(n, pct)
    vref = sr.v_ref(sr.diagonal(v), target)
    size, count, seen = sr.fit(lambda x: sr.cluster_count(v, x), vref, target)
    assert seen[0][0] == vref and (size, count) in seen and count == sr.cluster_count(v, size)
    assert abs(count - target) <= abs(seen[0][1] - target)
    assert all(abs(count - target) <= abs(c - target) for _, c in seen)
    assert all(x <= size for x, c in seen if abs(c - target) == abs(count - target))

    def count_fn(x):  # the product's search over the same count function gives the same answer
        try:
            return sr.cluster_count(v, x)
        except sr.GridTooFine as e:
            raise GridTooFine(str(e)) from e
    got = fit_voxel_size(count_fn, vref, target)
    assert got[0] == size and got[1] == count and got[2] == seen


def test_fit_stops_at_the_grid_limit():
    """Two points: the count never reaches a target of 4, so the halving runs into the 2^21 limit and stops."""
    v = f32([[0, 0, 0], [1, 1, 1]])
    size, count, seen = sr.fit(lambda x: sr.cluster_count(v, x), 1.0, 4)
    assert count == 2 and all(c <= 2 for _, c in seen)
    assert size == max(x for x, c in seen if c == 2)


# ---- the command line ---------------------------------------------------------------------------------------
def test_cli_round_trip(tmp_path, capsys):
    """--vertex-percent 100 returns the input mesh, so the round trip needs no GPU: what is written is what was
    read (positions, normals, colours through uint8, triangles).  Exit codes as the reference script's."""
    from mqr.downsample_mesh import main
    from mqr.geometry import Tensor, TriangleMesh, read_triangle_mesh, write_triangle_mesh
    v, t, _ = cube_case()
    mesh = TriangleMesh(v, v * 0.5, t)
    mesh.vertex["colors"] = Tensor((np.arange(24).reshape(8, 3) * 10 / 255.0).astype(np.float32))
    src, dst = tmp_path / "in.ply", tmp_path / "sub" / "out.ply"
    write_triangle_mesh(str(src), mesh)
    assert main([str(src), str(dst), "--vertex-percent", "100"]) == 0
    out = read_triangle_mesh(str(dst))
    assert np.array_equal(out.vertices, v) and np.array_equal(out.triangles, t)
    assert np.array_equal(out.vertex_normals, v * 0.5) and np.array_equal(out.vertex_colors, mesh.vertex_colors)
    assert "returning original mesh" in capsys.readouterr().out
    assert main([str(src), str(dst), "--vertex-percent", "0"]) == 1
    assert main([str(tmp_path / "missing.ply"), str(dst)]) == 1
    err = capsys.readouterr().err
    assert "between 0 and 100" in err and "not found" in err
    with pytest.raises(SystemExit):
        main([str(src), str(dst), "--voxel-size-rule", "quadric"])
