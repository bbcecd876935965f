"""Colours through the host PLY writers and readers (mqr.geometry), ``PointCloud`` colours, and the result
paths of ``mqr.dataio.ReconstructionDataIO`` (reference ``reconstruction_data_io.py:57-145``).  No GPU."""
import struct

import numpy as np
import pytest

from mqr import geometry
from mqr.dataio import DataIO, ReconstructionDataIO

# colour values whose bytes pin floor(clamp(c, 0, 1) * 255 + 0.5): the ends, a tie, outside the range, and
# 126.5 / 255.  The expected bytes are literals worked out by hand: as float32, 126.5 / 255 is
# 0.4960784316062927, a little above the tie (times 255: 126.50000006), so it rounds up to 127.
EDGE = np.array([0.0, 1.0, 0.5, -0.1, 1.2, 126.5 / 255.0], np.float64)
EDGE_BYTES = [0, 255, 128, 0, 255, 127]


def expected_bytes(c):
    c = np.asarray(c, np.float64)
    return np.floor(np.clip(c, 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8)


def header_of(path):
    data = open(path, "rb").read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    return data[:end].decode().splitlines(), data[end:]


def colours(n, seed=0):
    c = np.random.default_rng(seed).random((n, 3)).astype(np.float32)
    c.reshape(-1)[:len(EDGE)] = EDGE.astype(np.float32)
    return c


def small_mesh(colors=True):
    rng = np.random.default_rng(3)
    v = rng.normal(size=(9, 3)).astype(np.float32)
    nrm = rng.normal(size=(9, 3)).astype(np.float32)
    t = np.array([[0, 1, 2], [2, 3, 4], [4, 5, 6], [6, 7, 8]], np.int32)
    m = geometry.TriangleMesh(v, nrm, t)
    if colors:
        m.vertex["colors"] = geometry.Tensor(colours(9))
    return m


def test_color_to_uint8_edge_values():
    assert list(geometry.color_to_uint8(EDGE.astype(np.float32))) == EDGE_BYTES
    # the float32 just below that one is under the tie (times 255: 126.4999925) and rounds down
    below = np.nextafter(np.float32(126.5 / 255.0), np.float32(0))
    assert geometry.color_to_uint8(below) == 126
    # float64 colours that give x.5 exactly round up: floor(x.5 + 0.5)
    halves = np.array([126.5, 0.5, 254.5]) / 255.0
    assert list(halves * 255.0) == [126.5, 0.5, 254.5]
    assert list(geometry.color_to_uint8(halves)) == [127, 1, 255]
    assert geometry.color_to_uint8(np.float64(0.5)) == 128  # floor(127.5 + 0.5)


def test_coloured_mesh_round_trip(tmp_path):
    m = small_mesh()
    p = tmp_path / "color_mesh.ply"
    assert geometry.write_triangle_mesh(str(p), m)
    header, body = header_of(p)
    assert header == ["ply", "format binary_little_endian 1.0", "comment Created by Open3D", "element vertex 9",
                      "property double x", "property double y", "property double z",
                      "property double nx", "property double ny", "property double nz",
                      "property uchar red", "property uchar green", "property uchar blue",
                      "element face 4", "property list uchar uint vertex_indices", "end_header"]
    assert len(body) == 9 * (6 * 8 + 3) + 4 * 13
    want = expected_bytes(m.vertex_colors)
    assert list(want.reshape(-1)[:6]) == EDGE_BYTES
    rec = np.frombuffer(body, np.dtype([("d", "<f8", (6,)), ("c", "u1", (3,))]), 9)
    assert np.array_equal(rec["c"], want)
    assert np.array_equal(rec["d"][:, :3], m.vertices.astype(np.float64))
    back = geometry.read_triangle_mesh(str(p))
    assert np.array_equal(back.vertices, m.vertices) and np.array_equal(back.vertex_normals, m.vertex_normals)
    assert np.array_equal(back.triangles, m.triangles)
    assert back.has_vertex_colors() and back.vertex_colors.dtype == np.float32
    assert np.array_equal(back.vertex_colors, (want.astype(np.float64) / 255.0).astype(np.float32))
    # write_vertex_colors=False leaves them out; TriangleMesh.write_ply carries them
    q = tmp_path / "plain.ply"
    geometry.write_triangle_mesh(str(q), m, write_vertex_colors=False)
    assert not any("red" in ln for ln in header_of(q)[0])
    assert not geometry.read_triangle_mesh(str(q)).has_vertex_colors()
    m.write_ply(str(q))
    assert q.read_bytes() == p.read_bytes()
    assert np.array_equal(m.cpu().vertex_colors, m.vertex_colors)


def test_coloured_cloud_round_trip(tmp_path):
    rng = np.random.default_rng(4)
    pts, nrm, col = (rng.normal(size=(11, 3)).astype(np.float32), rng.normal(size=(11, 3)).astype(np.float32),
                     colours(11, 1))
    pc = geometry.PointCloud(pts, nrm, colors=col)
    assert pc.has_colors() and np.array_equal(pc.colors, col) and np.array_equal(pc.point.colors.numpy(), col)
    p = tmp_path / "color.ply"
    assert geometry.write_point_cloud(str(p), pc, write_ascii=False, compressed=True)
    header, body = header_of(p)
    assert header == ["ply", "format binary_little_endian 1.0", "comment Created by Open3D", "element vertex 11",
                      "property double x", "property double y", "property double z",
                      "property double nx", "property double ny", "property double nz",
                      "property uchar red", "property uchar green", "property uchar blue", "end_header"]
    assert len(body) == 11 * 51
    want = expected_bytes(col)
    back = geometry.read_point_cloud(str(p))
    assert np.array_equal(back.points, pts) and np.array_equal(back.normals, nrm)
    assert back.colors.dtype == np.float32
    assert np.array_equal(back.colors, (want.astype(np.float64) / 255.0).astype(np.float32))
    assert list(np.round(back.colors.reshape(-1)[:6] * 255).astype(int)) == EDGE_BYTES
    # cpu(), write_ply() and to_legacy() (without Open3D: the cloud itself) carry the colours
    q = tmp_path / "again.ply"
    pc.cpu().write_ply(str(q))
    assert q.read_bytes() == p.read_bytes()
    assert np.array_equal(pc.uniform_down_sample(3).colors, col[::3])
    legacy = pc.to_legacy()
    assert np.array_equal(np.asarray(legacy.colors, np.float32), col)


def documented_bytes(verts, normals, tris):
    """The colourless layout, built from its description: header lines, then per vertex six little-endian
    doubles, then per face a count byte 3 and three little-endian uint32."""
    lines = ["ply", "format binary_little_endian 1.0", "comment Created by Open3D", f"element vertex {len(verts)}",
             "property double x", "property double y", "property double z",
             "property double nx", "property double ny", "property double nz"]
    if tris is not None:
        lines += [f"element face {len(tris)}", "property list uchar uint vertex_indices"]
    out = ("\n".join(lines + ["end_header"]) + "\n").encode()
    for p, n in zip(verts, normals):
        out += struct.pack("<6d", *[float(x) for x in p], *[float(x) for x in n])
    for t in ([] if tris is None else tris):
        out += struct.pack("<B3I", 3, *[int(x) for x in t])
    return out


def test_files_without_colours_are_unchanged(tmp_path):
    m = small_mesh(colors=False)
    p = tmp_path / "mesh.ply"
    geometry.write_triangle_mesh(str(p), m)
    assert p.read_bytes() == documented_bytes(m.vertices, m.vertex_normals, m.triangles)
    m.write_ply(str(p))
    assert p.read_bytes() == documented_bytes(m.vertices, m.vertex_normals, m.triangles)
    pc = geometry.PointCloud(m.vertices, m.vertex_normals)
    geometry.write_point_cloud(str(p), pc)
    assert p.read_bytes() == documented_bytes(m.vertices, m.vertex_normals, None)
    pc.write_ply(str(p))
    assert p.read_bytes() == documented_bytes(m.vertices, m.vertex_normals, None)
    back = geometry.read_point_cloud(str(p))
    assert back.colors is None and not back.has_colors() and np.array_equal(back.points, m.vertices)


def test_point_cloud_without_colours_behaves_as_before():
    rng = np.random.default_rng(6)
    pts, nrm = rng.normal(size=(7, 3)).astype(np.float32), rng.normal(size=(7, 3)).astype(np.float32)
    pc = geometry.PointCloud(pts, nrm, "HIP:0")  # device stays the third positional argument
    assert pc.device == "HIP:0" and sorted(pc.point) == ["normals", "positions"]
    assert pc.colors is None and not pc.has_colors()
    with pytest.raises(AttributeError):
        pc.point.colors
    c = pc.cpu()
    assert c.device == "CPU:0" and sorted(c.point) == ["normals", "positions"] and np.array_equal(c.points, pts)
    d = pc.uniform_down_sample(2)
    assert sorted(d.point) == ["normals", "positions"] and np.array_equal(d.normals, nrm[::2])
    assert geometry.mesh_fields(small_mesh(colors=False)).colors is None


def test_reconstruction_data_io_writes_the_reference_paths(tmp_path):
    io = DataIO(tmp_path).reconstruction
    assert isinstance(io, ReconstructionDataIO)
    m, plain = small_mesh(), small_mesh(colors=False)
    pc = geometry.PointCloud(m.vertices, m.vertex_normals, colors=m.vertex_colors)

    class Volume:  # the volume's own writer is the GPU suite's; here only the path
        def save(self, file_name):
            np.savez(file_name, voxel_size=np.float32(0.01))

    io.save_colorless_pcd_legacy(geometry.PointCloud(plain.vertices, plain.vertex_normals).to_legacy())
    io.save_colorless_mesh_raw_legacy(plain.to_legacy())
    io.save_colorless_mesh_clean_legacy(plain.to_legacy())
    io.save_colored_mesh_legacy(m.to_legacy())
    io.save_colored_pcd_legacy(pc.to_legacy())
    io.save_colorless_vbg(Volume())
    rec = tmp_path / "reconstruction"
    names = ["colorless.ply", "colorless_mesh_raw.ply", "colorless_mesh_clean.ply", "color_mesh.ply", "color.ply",
             "colorless_vbg.npz"]
    assert sorted(f.name for f in rec.iterdir()) == sorted(names)
    assert not geometry.read_triangle_mesh(str(rec / "colorless_mesh_raw.ply")).has_vertex_colors()
    assert (rec / "colorless_mesh_raw.ply").read_bytes() == (rec / "colorless_mesh_clean.ply").read_bytes()
    assert geometry.read_point_cloud(str(rec / "colorless.ply")).colors is None
    mesh_back, pcd_back = io.load_colored_mesh(), io.load_colored_pcd()
    want = (expected_bytes(m.vertex_colors).astype(np.float64) / 255.0).astype(np.float32)
    assert np.array_equal(mesh_back.vertex_colors, want) and np.array_equal(pcd_back.colors, want)
    assert np.array_equal(pcd_back.points, m.vertices)
    # the tensor-geometry writers go to the same files; a path object may stand in for the directory
    before = (rec / "color_mesh.ply").read_bytes(), (rec / "color.ply").read_bytes()
    io2 = ReconstructionDataIO(io.paths)
    io2.save_colored_mesh(m)
    io2.save_colored_pcd(pc)
    assert ((rec / "color_mesh.ply").read_bytes(), (rec / "color.ply").read_bytes()) == before
    assert ReconstructionDataIO(tmp_path / "none").load_colored_pcd() is None
    assert ReconstructionDataIO(tmp_path / "none").load_colorless_vbg() is None
