"""mqr.geometry's mesh unpacking (mesh_fields, device_mesh, host_rows): which inputs each consumer reads in
place in HBM and which it sends down its host path.  The DeviceArrays carry made-up pointers that nothing
dereferences, and the library is never loaded.  The expected values are each consumer's rules as
device_mesh's docstring states them."""
import numpy as np
import pytest

from mqr.geometry import (DeviceArray, DeviceMesh, Tensor, TriangleMesh, device_mesh, host_rows, mesh_fields)

PV, PT, PN, PC = 0x1000, 0x2000, 0x3000, 0x4000
NV, NT = 5, 7


def dev(ptr, shape, dtype=np.float32, device=0):
    return Tensor(DeviceArray(None, ptr, shape, dtype, device))


def mesh(v=None, t=None, n=None, c=None, device="HIP:0"):
    """A tensor mesh in HBM on device 0 unless a field says otherwise."""
    m = TriangleMesh(dev(PV, (NV, 3)) if v is None else v, dev(PN, (NV, 3)) if n is None else n,
                     dev(PT, (NT, 3), np.int32) if t is None else t, device=device)
    if c is not None:
        m.vertex["colors"] = c
    return m


# the three consumers, as their modules call the helper
def filter_view(m):
    from mqr.vbg import parse_device
    f = mesh_fields(m)
    return device_mesh(f, parse_device(f.device), normals=True)


def quality_view(m):
    return device_mesh(mesh_fields(m), colors=True, strict=True)


def raycast_view(m, triangles=None, scene_device=0):
    return device_mesh(mesh_fields(m, triangles), scene_device)


def view(normals=None, colors=None, device=0, nv=NV, nt=NT):
    return DeviceMesh(device, PV, nv, PT, nt, normals, colors)


def test_resident_tensor_mesh():
    m = mesh(c=dev(PC, (NV, 3)))
    assert filter_view(m) == view(normals=PN)
    assert quality_view(m) == view(colors=PC)
    assert raycast_view(m) == view()
    assert quality_view(mesh()) == view()  # no colours: still in place


@pytest.mark.parametrize("field", ["v", "t"])
def test_wrong_dtype(field):
    m = mesh(v=dev(PV, (NV, 3), np.float64)) if field == "v" else mesh(t=dev(PT, (NT, 3), np.int64))
    assert filter_view(m) is None and quality_view(m) is None and raycast_view(m) is None


def test_wrong_device():
    m = mesh(v=dev(PV, (NV, 3), device=1), t=dev(PT, (NT, 3), np.int32, device=1), device="HIP:0")
    assert filter_view(m) is None      # not on parse_device(mesh.device)
    assert quality_view(m) is None     # mesh.device disagrees with the tensors
    assert raycast_view(m) is None     # not on the scene's device
    assert raycast_view(m, scene_device=1) == view(device=1)


@pytest.mark.parametrize("field", ["v", "t"])
def test_trailing_dimension_other_than_3(field):
    m = mesh(v=dev(PV, (NV, 4))) if field == "v" else mesh(t=dev(PT, (NT, 4), np.int32))
    assert filter_view(m) is None and quality_view(m) is None and raycast_view(m) is None


def test_positions_on_the_device_and_indices_on_the_host():
    m = mesh(t=Tensor(np.zeros((NT, 3), np.int32)))
    assert filter_view(m) is None and quality_view(m) is None and raycast_view(m) is None
    m = mesh(t=dev(PT, (NT, 3), np.int32, device=1))  # ... or on another device
    assert filter_view(m) is None and quality_view(m) is None and raycast_view(m) is None


@pytest.mark.parametrize("n", [dev(PN, (NV + 1, 3)), dev(PN, (NV, 3), np.float64), dev(PN, (NV, 3), device=1),
                               Tensor(np.zeros((NV, 3), np.float32))])
def test_unfit_normals_are_left_out_by_the_filter(n):
    assert filter_view(mesh(n=n)) == view(normals=None)
    assert quality_view(mesh(n=n)) == view() and raycast_view(mesh(n=n)) == view()  # they never ask for normals


@pytest.mark.parametrize("c", [Tensor(np.zeros((NV, 3), np.float32)), dev(PC, (NV, 3), device=1),
                               dev(PC, (NV, 3), np.float64), dev(PC, (NV, 4)), dev(PC, (0, 3)),
                               Tensor(np.zeros((0, 3), np.float32))])
def test_unfit_colours_send_the_whole_mesh_to_the_quality_host_path(c):
    """Colours on the host, elsewhere, not float32, wrong-shaped or empty (the host path then counts an
    empty array as no colours)."""
    m = mesh(c=c)
    assert quality_view(m) is None
    assert filter_view(m) == view(normals=PN) and raycast_view(m) == view()  # the others do not read colours


def test_mesh_device_that_disagrees():
    m = mesh(device="HIP:1")  # the tensors are on device 0
    assert quality_view(m) is None
    assert filter_view(m) is None
    assert raycast_view(m) == view()                       # the scene's device decides, not mesh.device
    assert quality_view(mesh(device=None)) == view()       # no mesh.device: the positions' device
    m1 = mesh(v=dev(PV, (NV, 3), device=1), t=dev(PT, (NT, 3), np.int32, device=1), device="HIP:1")
    assert quality_view(m1) == view(device=1) and filter_view(m1) == view(device=1)


class Legacy:
    """A legacy mesh whose attributes (unusually) hold device Tensors: it still never takes the device path."""

    def __init__(self, colors=True):
        self.vertices, self.triangles = dev(PV, (NV, 3)), dev(PT, (NT, 3), np.int32)
        self.vertex_normals, self.vertex_colors = dev(PN, (NV, 3)), dev(PC, (NV, 3))
        self._colors = colors

    def has_vertex_colors(self):
        return self._colors


def test_legacy_mesh():
    m = Legacy()
    f = mesh_fields(m)
    assert (f.positions, f.triangles, f.normals, f.colors) == (m.vertices, m.triangles, m.vertex_normals,
                                                               m.vertex_colors)
    assert f.kind == "legacy" and f.device is None
    assert filter_view(m) is None and quality_view(m) is None and raycast_view(m) is None
    assert mesh_fields(Legacy(colors=False)).colors is None  # has_vertex_colors() is honoured


def test_tuple():
    v, t, c = dev(PV, (NV, 3)), dev(PT, (NT, 3), np.int32), dev(PC, (NV, 3))
    f = mesh_fields((v, t, c))
    assert (f.positions, f.triangles, f.normals, f.colors, f.kind) == (v, t, None, c, "tuple")
    assert mesh_fields([v, t]).colors is None
    assert quality_view((v, t, c)) is None and quality_view((v, t)) is None  # tuples never take the device path
    for bad in ((v,), (v, t, c, c)):
        with pytest.raises(ValueError, match="expected"):
            mesh_fields(bad)


def test_loose_tensors_of_shape_h_w_3():
    v, t = dev(PV, (4, 6, 3)), dev(PT, (2, 5, 3), np.int32)
    assert raycast_view(v, t) == view(nv=24, nt=10)  # counts: the product of the leading dimensions
    assert raycast_view(v, t, scene_device=1) is None
    assert raycast_view(np.zeros((NV, 3), np.float32), np.zeros((NT, 3), np.int32)) is None
    assert raycast_view([[0.0, 0.0, 0.0]] * 3, [[0, 1, 2]]) is None  # plain lists: the host path


def test_empty_device_mesh_is_a_view_with_zero_counts():
    """The consumers decide: the filter returns its input, the quality pass raises ValueError."""
    m = mesh(v=dev(0, (0, 3)), t=dev(0, (0, 3), np.int32), n=dev(0, (0, 3)))
    assert filter_view(m) == DeviceMesh(0, 0, 0, 0, 0, 0, None)
    assert quality_view(m) == DeviceMesh(0, 0, 0, 0, 0, None, None)


def test_host_rows():
    a = host_rows(np.arange(12, dtype=np.float64).reshape(2, 2, 3)[:, ::-1], np.float32)
    assert a.dtype == np.float32 and a.shape == (4, 3) and a.flags.c_contiguous
    assert np.array_equal(a[0], [3, 4, 5])
    t = host_rows(Tensor(np.arange(6, dtype=np.int64).reshape(2, 3)), np.int32)
    assert t.dtype == np.int32 and t.shape == (2, 3)
    assert host_rows([[0, 1, 2]], np.int32).shape == (1, 3)
