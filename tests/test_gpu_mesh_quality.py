"""Mesh quality metrics on the device (csrc/meshquality.hip through mqr.evaluation.compute_raw_metrics)
against the reference's own outputs (golden) and the numpy restatement (quality_ref).  Integer and boolean
fields are exact; float fields use quality_ref.tolerance (derived there)."""
from dataclasses import asdict

import numpy as np
import pytest

import quality_ref as qr
from test_quality_ref import CASES, compare, golden, golden_mesh, golden_raw  # noqa: F401  (golden: fixture)

pytestmark = pytest.mark.gpu


def metrics(mesh):
    from mqr.evaluation import compute_raw_metrics
    d = asdict(compute_raw_metrics(mesh, name="m"))
    return {f: d[f] for f in qr.FIELDS}


@pytest.mark.parametrize("case", CASES)
def test_golden_cases(golden, case):
    v, t, c = golden_mesh(golden, case)
    _, scales = qr.raw_metrics(v, t, c)
    got = metrics((v, t) if c is None else (v, t, c))
    compare(got, golden_raw(golden, case), scales, case)


@pytest.mark.parametrize("nt", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_strips_at_wave_workgroup_and_slab_edges(nt):
    v, t, c = qr.strip_mesh(nt, seed=nt)
    want, scales = qr.raw_metrics(v, t, c)
    compare(metrics((v, t, c)), want, scales, f"strip{nt}")
    want, scales = qr.raw_metrics(v, t, None)
    compare(metrics((v, t)), want, scales, f"strip{nt} no colour")


def test_repeated_call_is_bit_identical(golden):
    v, t, c = golden_mesh(golden, "big")
    a, b = metrics((v, t, c)), metrics((v, t, c))
    assert a == b


def test_float64_input_is_rounded_to_float32(golden):
    v, t, c = golden_mesh(golden, "mixed")
    v64 = v.astype(np.float64) * (1.0 + 2.0 ** -40)  # not float32-representable; rounds back to v
    assert (v64.astype(np.float32) == v).all() and (v64 != v).any()
    assert metrics((v64, t.astype(np.int64), c.astype(np.float64))) == metrics((v, t, c))


@pytest.fixture(scope="module")
def room():
    """The 16-frame 160x120 room of tests/test_gpu_meshfilter.py, extracted and left in HBM."""
    from mqr import synthetic
    from mqr.vbg import VoxelBlockGrid
    seq = synthetic.make_sequence("room", n=16, height=120, width=160, f=131.25, noise=True, seed=43)
    vol = VoxelBlockGrid(voxel_size=0.02, block_resolution=8, block_count=512)
    vol.integrate_frames(seq["depth"], seq["K"], seq["T_wc"], depth_scale=1.0, depth_max=4.0,
                         trunc_voxel_multiplier=6.0)
    return vol.extract_triangle_mesh(weight_threshold=1.0)


def test_device_resident_mesh_equals_its_host_copy(room):
    from mqr.geometry import device_ptr
    assert device_ptr(room.vertex.positions) is not None  # evaluated in place
    on_device = metrics(room)
    host = room.cpu()
    assert device_ptr(host.vertex.positions) is None
    assert on_device == metrics(host)
    assert on_device["num_triangles"] == host.triangles.shape[0] > 1000 and not on_device["has_color"]


def test_triangle_order_does_not_matter(room):
    host = room.cpu()
    v, t = host.vertices, host.triangles
    _, scales = qr.raw_metrics(v, t, None)
    a = metrics((v, t))
    b = metrics((v, t[np.random.default_rng(3).permutation(len(t))]))
    compare(b, a, scales, "permuted")


def test_index_range_is_rejected_on_host_arrays(golden):
    from mqr.evaluation import compute_raw_metrics
    v, t, _ = golden_mesh(golden, "closed")
    bad = t.copy()
    bad[100, 1] = len(v)
    with pytest.raises(ValueError):  # numpy rejects it before any launch
        compute_raw_metrics((v, bad))
    assert metrics((v, t))["is_watertight"]  # and the library is fine afterwards


def test_ply_file_with_colours(golden, tmp_path):
    from mqr.evaluation import compute_raw_metrics_for_mesh
    v, t, c = golden_mesh(golden, "mixed")
    c8 = np.round(c * 255).astype(np.uint8)
    rec = np.empty(len(v), dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"),
                                  ("blue", "u1")])
    rec["x"], rec["y"], rec["z"] = v.T
    rec["red"], rec["green"], rec["blue"] = c8.T
    faces = np.empty(len(t), dtype=[("c", "u1"), ("i", "<u4", (3,))])
    faces["c"], faces["i"] = 3, t
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {len(v)}", "property float x",
              "property float y", "property float z", "property uchar red", "property uchar green",
              "property uchar blue", f"element face {len(t)}", "property list uchar uint vertex_indices", "end_header"]
    path = tmp_path / "mixed.ply"
    path.write_bytes(("\n".join(header) + "\n").encode() + rec.tobytes() + faces.tobytes())
    got = compute_raw_metrics_for_mesh(path, "mixed")
    c32 = (c8.astype(np.float64) / 255.0).astype(np.float32)
    want, scales = qr.raw_metrics(v, t, c32)
    assert got.name == "mixed" and got.path == path
    compare(got, want, scales, "ply")


def test_device_resident_nan_ends_as_an_error(golden):
    """A mesh already in HBM cannot be checked with numpy: the vertex pass raises the flag and the call fails
    before any kernel gathers (NaN coordinates are read, never used as addresses)."""
    from mqr import _lib
    from mqr.evaluation import compute_raw_metrics
    from mqr.geometry import DeviceArray, Tensor, TriangleMesh
    v, t, _ = golden_mesh(golden, "flat")
    bad = v.copy()
    bad[40, 2] = np.nan
    bv, bt = _lib.DeviceBuffer.from_array(bad), _lib.DeviceBuffer.from_array(t)
    mesh = TriangleMesh(Tensor(DeviceArray(bv, bv.ptr.value, bad.shape, np.float32, 0)), np.zeros_like(bad),
                        Tensor(DeviceArray(bt, bt.ptr.value, t.shape, np.int32, 0)), device="HIP:0")
    with pytest.raises(_lib.MqrError, match="not finite"):
        compute_raw_metrics(mesh)
    good = _lib.DeviceBuffer.from_array(v)
    mesh = TriangleMesh(Tensor(DeviceArray(good, good.ptr.value, v.shape, np.float32, 0)), np.zeros_like(v),
                        Tensor(DeviceArray(bt, bt.ptr.value, t.shape, np.int32, 0)), device="HIP:0")
    assert asdict(compute_raw_metrics(mesh))["total_edges"] == 208
