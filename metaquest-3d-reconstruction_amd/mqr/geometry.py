"""Result containers returned by the fusion path (duck-type what the reference's callers use).

The reference consumes Open3D tensor geometry:
  * ``vbg.extract_point_cloud().to_legacy()`` (reconstruct_scene.py:90) and
    ``pcd.point.positions.shape[0]`` (refine_fragment_poses.py:39-42);
  * ``mesh.to_legacy()``, ``mesh.cpu()``, ``mesh.device``, ``mesh.to(device)``
    (reconstruct_scene.py:105-122, 186-198; o3d_utils.py:258, 304-307).
These classes expose the same attribute paths over numpy arrays; ``to_legacy()`` returns a real
Open3D legacy object when ``open3d`` is importable and otherwise returns ``self`` (which offers
``points`` / ``vertices`` / ``triangles`` / ``*_normals`` arrays and a binary PLY writer).

Results of the device path (extraction, mesh filtering, ray casts) stay in HBM, as Open3D's tensor
geometry on a CUDA device does: their Tensors hold a device array and copy it to the host once, on
the first host access (``.numpy()``, indexing, ``.cpu()``, ``to_legacy()``, pickling).  Consumers of
this package (``RaycastingScene.add_triangles``, ``filter_mesh_components``, ``color_map``) take the
device arrays in place, so extract -> filter -> cast -> colour moves no mesh over PCIe.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional

import numpy as np


class DeviceArray:
    """A C-order array in HBM: device pointer, shape, numpy dtype, device index, and the object that owns
    the memory (kept alive with the array)."""

    def __init__(self, owner, ptr: int, shape, dtype, device_id: int):
        self.owner = owner
        self.ptr = int(ptr or 0)
        self.shape = tuple(int(x) for x in shape)
        self.dtype = np.dtype(dtype)
        self.device_id = int(device_id)

    @property
    def nbytes(self) -> int:
        return int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize

    def host(self) -> np.ndarray:
        from . import _lib
        out = np.empty(self.shape, self.dtype)
        if out.nbytes:
            _lib.call("mqr_memcpy", ctypes.c_void_p(out.ctypes.data), _lib.MQR_HOST, ctypes.c_void_p(self.ptr),
                      _lib.MQR_DEVICE, out.nbytes, self.device_id)
        return out


class Tensor:
    """Minimal tensor facade (``.numpy()``, ``.shape``, ``.dtype``, indexing) over a host array or a
    DeviceArray (copied to the host once, on first host access)."""

    def __init__(self, array):
        if isinstance(array, DeviceArray):
            self._a, self._d = None, array
        else:
            self._a, self._d = np.asarray(array), None

    def numpy(self) -> np.ndarray:
        if self._a is None:
            self._a = self._d.host()
        return self._a

    def device_array(self):
        """The DeviceArray behind this tensor, or None for a host tensor."""
        return self._d

    @property
    def is_cuda(self) -> bool:
        return self._d is not None

    @property
    def shape(self):
        return self._d.shape if self._a is None else self._a.shape

    @property
    def dtype(self):
        return self._d.dtype if self._a is None else self._a.dtype

    def __len__(self):
        return self.shape[0]

    def __getitem__(self, i):
        return self.numpy()[i]

    def __array__(self, dtype=None, copy=None):
        a = self.numpy()
        return a if dtype is None else a.astype(dtype)

    def cpu(self):
        return self if self._d is None else Tensor(self.numpy())

    def __getstate__(self):  # across processes: host arrays only
        return {"_a": self.numpy(), "_d": None}

    def __repr__(self):
        where = "HBM" if self._d is not None else "host"
        return f"mqr.Tensor(shape={self.shape}, dtype={self.dtype}, {where})"


class DeviceGeom:
    """Owner of one mqr_geom result (extraction / mesh filter): its arrays stay in HBM until the last
    Tensor over them is gone.  ``tensors()`` -> (positions, normals, triangles) Tensors over them."""

    def __init__(self, handle, device_id: int):
        from . import _lib
        self._h = handle
        self.device_id = int(device_id)
        nv, nt = ctypes.c_int64(), ctypes.c_int64()
        _lib.call("mqr_geom_counts", handle, ctypes.byref(nv), ctypes.byref(nt))
        self.nv, self.nt = int(nv.value), int(nt.value)
        p, n, t = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        _lib.call("mqr_geom_device_ptrs", handle, ctypes.byref(p), ctypes.byref(n), ctypes.byref(t))
        self._ptrs = (p.value or 0, n.value or 0, t.value or 0)

    def tensors(self):
        p, n, t = self._ptrs
        return (Tensor(DeviceArray(self, p, (self.nv, 3), np.float32, self.device_id)),
                Tensor(DeviceArray(self, n, (self.nv, 3), np.float32, self.device_id)),
                Tensor(DeviceArray(self, t, (self.nt, 3), np.int32, self.device_id)))

    def __del__(self):
        try:
            from . import _lib
            if self._h is not None and self._h.value and _lib._lib is not None:
                _lib._lib.mqr_geom_free(self._h)
            self._h = None
        except Exception:
            pass


def device_ptr(x, device_id=None):
    """(pointer, device index) of a tensor / array held in HBM (a device-backed Tensor or DeviceArray),
    else None; with device_id given, None unless it lives on that device."""
    d = x.device_array() if isinstance(x, Tensor) else x if isinstance(x, DeviceArray) else None
    if d is None or (device_id is not None and d.device_id != int(device_id)):
        return None
    return d.ptr, d.device_id


class MeshFields(NamedTuple):
    """A mesh's raw fields as its holder keeps them (Tensors, arrays or lists; None for what is absent)."""
    positions: object
    triangles: object
    normals: object
    colors: object
    kind: str      # "tensor", "legacy", "tuple" or "loose"
    device: object  # the mesh object's ``device`` attribute, if it has one


def mesh_fields(mesh, triangles=None) -> MeshFields:
    """Unpack a tensor mesh (``.vertex`` / ``.triangle``), a legacy mesh (``.vertices`` / ``.triangles`` /
    ``.vertex_normals`` / ``.vertex_colors``, no colours when ``has_vertex_colors()`` says so), a
    ``(vertices, triangles[, colors])`` tuple, or a loose ``vertices, triangles`` pair."""
    if triangles is not None:
        return MeshFields(mesh, triangles, None, None, "loose", None)
    if isinstance(mesh, (tuple, list)):
        if len(mesh) not in (2, 3):
            raise ValueError("expected (vertices, triangles[, colors])")
        return MeshFields(mesh[0], mesh[1], None, mesh[2] if len(mesh) == 3 else None, "tuple", None)
    dev = getattr(mesh, "device", None)
    if hasattr(mesh, "vertex") and hasattr(mesh, "triangle"):
        vx = mesh.vertex
        return MeshFields(vx.positions, mesh.triangle.indices, getattr(vx, "normals", None),
                          getattr(vx, "colors", None), "tensor", dev)
    c = getattr(mesh, "vertex_colors", None)
    if hasattr(mesh, "has_vertex_colors") and not mesh.has_vertex_colors():
        c = None
    return MeshFields(mesh.vertices, mesh.triangles, getattr(mesh, "vertex_normals", None), c, "legacy", dev)


class DeviceMesh(NamedTuple):
    """Device pointers and counts of a mesh held in HBM; normals / colors are None unless requested and fit."""
    device: int
    positions: int
    nv: int
    triangles: int
    nt: int
    normals: Optional[int]
    colors: Optional[int]


def device_mesh(f: MeshFields, device_id=None, normals=False, colors=False, strict=False) -> Optional[DeviceMesh]:
    """The mesh in place, when positions (float32, trailing dimension 3) and triangles (int32, trailing
    dimension 3) are both in HBM on one device; None sends the caller down its host path.

    Only tensor meshes and loose pairs qualify: a legacy mesh or a tuple never takes the device path.  The
    counts are the products of the leading dimensions, so loose ``(H, W, 3)`` Tensors are accepted.  With
    ``device_id`` both arrays must live on that device.  Without it the device is the positions' own, and a
    ``mesh.device`` that names another device gives None.  A requested optional field is returned when it is
    on that device, float32 and shaped like the positions; one that is absent or unfit has the pointer None,
    and with ``strict`` one that is present but unfit gives None for the whole mesh.  The consumers' rules:

    * filter_mesh_components: ``device_id`` is ``parse_device(mesh.device)``.  Unfit normals are left out:
      the filter runs without them and the result's normals are zeros.  (On its host path, normals whose row
      count differs from the positions' are dropped.)  Zero triangles returns the input object with the
      reference's warning, on either path.
    * compute_raw_metrics: no ``device_id``, colours ``strict``: unfit colours send the whole mesh down the
      host path, where an empty colour array counts as no colours and every array is validated with numpy.
      A device mesh with ``nv == 0`` or ``nt == 0`` raises ValueError.
    * RaycastingScene.add_triangles and the colour stages: ``device_id`` is the scene's device; positions and
      triangles only.
    """
    if f.kind not in ("tensor", "loose"):
        return None
    v, t = f.positions, f.triangles
    pv = device_ptr(v, device_id)
    pt = None if pv is None else device_ptr(t, pv[1])
    if pt is None or v.dtype != np.float32 or t.dtype != np.int32 or v.shape[-1:] != (3,) or t.shape[-1:] != (3,):
        return None
    dev = pv[1]
    if device_id is None and f.device is not None:
        from .vbg import parse_device
        if parse_device(f.device) != dev:
            return None

    def fit(x, wanted):
        ok = wanted and x is not None and x.dtype == np.float32 and tuple(x.shape) == tuple(v.shape)
        p = device_ptr(x, dev) if ok else None
        return None if p is None else p[0]

    pn, pc = fit(f.normals, normals), fit(f.colors, colors)
    unfit = (normals and f.normals is not None and pn is None) or (colors and f.colors is not None and pc is None)
    if strict and unfit:
        return None
    return DeviceMesh(dev, pv[0], int(np.prod(v.shape[:-1])), pt[0], int(np.prod(t.shape[:-1])), pn, pc)


def host_array(x) -> np.ndarray:
    return x.numpy() if hasattr(x, "numpy") else np.asarray(x)


def host_rows(x, dtype) -> np.ndarray:
    """The one host conversion of a mesh field: contiguous, ``dtype`` (float32 / int32), shape (-1, 3)."""
    return np.ascontiguousarray(host_array(x), dtype=dtype).reshape(-1, 3)


def _tensor(x):
    return x if isinstance(x, Tensor) else Tensor(x)


class Image:
    """Depth image wrapper (stands in for o3d.t.geometry.Image over a float32 H x W array)."""

    def __init__(self, tensor=None, device=None):
        a = tensor.numpy() if hasattr(tensor, "numpy") else np.asarray(tensor)
        self._a = np.ascontiguousarray(a, dtype=np.float32)
        if self._a.ndim == 3 and self._a.shape[2] == 1:
            self._a = self._a[:, :, 0]
        self.device = device

    def as_tensor(self):
        return Tensor(self._a)

    def numpy(self):
        return self._a

    @property
    def rows(self):
        return self._a.shape[0]

    @property
    def columns(self):
        return self._a.shape[1]


class _AttrMap(dict):
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError as e:
            raise AttributeError(k) from e


def _try_open3d():
    try:
        import open3d  # noqa: F401
        return open3d
    except Exception:
        return None


def _write_ply(path, verts, normals=None, tris=None):
    """Binary little-endian PLY in the layout Open3D's legacy writers use (``write_point_cloud`` /
    ``write_triangle_mesh`` with ``write_ascii=False``, reference ``reconstruction_data_io.py:57-94``;
    upstream FilePLY.cpp as recalled -- VERIFY): a ``comment Created by Open3D`` line, vertex
    coordinates and normals as ``double`` (the legacy geometry holds float64), faces as a ``uchar``
    count followed by ``uint`` indices.  The float32 device values widen to float64 exactly."""
    verts = np.asarray(verts, np.float64).reshape(-1, 3)
    n = len(verts)
    props = ["property double x", "property double y", "property double z"]
    cols = [verts]
    if normals is not None and len(normals) == n:
        props += ["property double nx", "property double ny", "property double nz"]
        cols.append(np.asarray(normals, np.float64).reshape(-1, 3))
    header = ["ply", "format binary_little_endian 1.0", "comment Created by Open3D", f"element vertex {n}"] + props
    if tris is not None:
        header += [f"element face {len(tris)}", "property list uchar uint vertex_indices"]
    header.append("end_header")
    with open(path, "wb") as f:
        f.write(("\n".join(header) + "\n").encode())
        f.write(np.ascontiguousarray(np.concatenate(cols, axis=1), dtype="<f8").tobytes())
        if tris is not None:
            t = np.asarray(tris).reshape(-1, 3)
            if len(t) and (t.min() < 0 or t.max() >= max(n, 1)):
                raise ValueError("triangle index out of range")
            rec = np.empty(len(t), dtype=[("c", "u1"), ("i", "<u4", (3,))])
            rec["c"] = 3
            rec["i"] = t.astype(np.uint32)
            f.write(rec.tobytes())


def read_ply(path):
    """Minimal reader for binary little-endian PLY files with vertex (float / double properties)
    and optional face (list uchar int / uint) elements: returns (properties dict, faces or None)."""
    sizes = {"char": "i1", "uchar": "u1", "short": "<i2", "ushort": "<u2", "int": "<i4", "uint": "<u4",
             "float": "<f4", "double": "<f8", "int8": "i1", "uint8": "u1", "int32": "<i4", "uint32": "<u4",
             "float32": "<f4", "float64": "<f8"}
    with open(path, "rb") as f:
        data = f.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode().splitlines()
    if lines[0] != "ply" or lines[1] != "format binary_little_endian 1.0":
        raise ValueError("not a binary little-endian PLY")
    elems = []
    for ln in lines[2:]:
        tok = ln.split()
        if tok[0] == "element":
            elems.append((tok[1], int(tok[2]), []))
        elif tok[0] == "property":
            elems[-1][2].append(tok[1:])
    off = end
    props, faces = {}, None
    for name, count, plist in elems:
        if name == "vertex":
            dt = np.dtype([(p[1], sizes[p[0]]) for p in plist])
            arr = np.frombuffer(data, dt, count, off)
            off += dt.itemsize * count
            props = {k: arr[k] for k in dt.names}
        elif name == "face":
            (_, cnt_t, idx_t, _), = plist
            dt = np.dtype([("c", sizes[cnt_t]), ("i", sizes[idx_t], (3,))])
            arr = np.frombuffer(data, dt, count, off)
            if count and (arr["c"] != 3).any():
                raise ValueError("non-triangle face")
            off += dt.itemsize * count
            faces = arr["i"].astype(np.int64)
    return props, faces


class PointCloud:
    def __init__(self, positions, normals, device=None):
        self.point = _AttrMap(positions=_tensor(positions), normals=_tensor(normals))
        self.device = device

    @classmethod
    def from_device(cls, geom: DeviceGeom, device=None):
        p, n, _ = geom.tensors()
        return cls(p, n, device=device)

    @property
    def points(self):
        return self.point.positions.numpy()

    @property
    def normals(self):
        return self.point.normals.numpy()

    def cpu(self):
        return PointCloud(self.point.positions.cpu(), self.point.normals.cpu(), device="CPU:0")

    def to(self, device):
        self.device = device
        return self

    def to_legacy(self):
        o3d = _try_open3d()
        if o3d is None:
            return self
        pcd = o3d.geometry.PointCloud()
        pcd.points = o3d.utility.Vector3dVector(self.points.astype(np.float64))
        pcd.normals = o3d.utility.Vector3dVector(self.normals.astype(np.float64))
        return pcd

    def write_ply(self, path):
        _write_ply(path, self.points, self.normals)

    def uniform_down_sample(self, every_k_points: int):
        """Points 0, k, 2k, ... (``o3d.t.geometry.PointCloud.uniform_down_sample``) as a host cloud."""
        k = int(every_k_points)
        if k < 1:
            raise ValueError("every_k_points must be >= 1")
        return PointCloud(self.points[::k].copy(), self.normals[::k].copy(), device=self.device)

    def voxel_down_sample(self, voxel_size: float):
        """Mean position per occupied voxel, in ascending voxel order, computed on the GPU
        (mqr.registration.CloudSet; a cloud held in HBM is read in place).  Positions only: the
        registration path reads nothing else, so the result's normals are zero."""
        from .registration import CloudSet
        d = device_ptr(self.point.positions)
        cs = CloudSet([self], d[1] if d else 0)
        try:
            p = cs.voxel_down_sample(0, voxel_size)
        finally:
            cs.close()
        return PointCloud(p, np.zeros_like(p), device=self.device)


class TriangleMesh:
    def __init__(self, vertices, normals, triangles, device=None):
        self.vertex = _AttrMap(positions=_tensor(vertices), normals=_tensor(normals))
        self.triangle = _AttrMap(indices=_tensor(triangles))
        self.device = device

    @classmethod
    def from_device(cls, geom: DeviceGeom, device=None):
        return cls(*geom.tensors(), device=device)

    @property
    def vertices(self):
        return self.vertex.positions.numpy()

    @property
    def vertex_normals(self):
        return self.vertex.normals.numpy()

    @property
    def triangles(self):
        return self.triangle.indices.numpy()

    def cpu(self):
        return TriangleMesh(self.vertex.positions.cpu(), self.vertex.normals.cpu(), self.triangle.indices.cpu(),
                            device="CPU:0")

    def to(self, device):
        self.device = device
        return self

    def to_legacy(self):
        o3d = _try_open3d()
        if o3d is None:
            return self
        m = o3d.geometry.TriangleMesh()
        m.vertices = o3d.utility.Vector3dVector(self.vertices.astype(np.float64))
        m.vertex_normals = o3d.utility.Vector3dVector(self.vertex_normals.astype(np.float64))
        m.triangles = o3d.utility.Vector3iVector(self.triangles.astype(np.int32))
        return m

    def write_ply(self, path):
        _write_ply(path, self.vertices, self.vertex_normals, self.triangles)


# ---- o3d.io mirror for the reference's writers (reconstruction_data_io.py:57-94) -------------------
def write_point_cloud(filename, pointcloud, write_ascii=False, compressed=False, print_progress=False):
    """``o3d.io.write_point_cloud`` for ``.ply`` (binary; ``compressed`` has no effect on PLY in
    Open3D either).  Returns True like Open3D."""
    if write_ascii:
        raise NotImplementedError("ASCII PLY is not written by the reference pipeline")
    if not str(filename).lower().endswith(".ply"):
        raise ValueError("only .ply is supported")
    _write_ply(filename, pointcloud.points, pointcloud.normals)
    return True


def write_triangle_mesh(filename, mesh, write_ascii=False, compressed=False, write_vertex_normals=True,
                        write_vertex_colors=True, write_triangle_uvs=True, print_progress=False):
    """``o3d.io.write_triangle_mesh`` for ``.ply`` meshes without colours (the colorless raw and
    clean meshes, ``reconstruction_data_io.py:68-78``).  Returns True like Open3D."""
    if write_ascii:
        raise NotImplementedError("ASCII PLY is not written by the reference pipeline")
    if not str(filename).lower().endswith(".ply"):
        raise ValueError("only .ply is supported")
    normals = mesh.vertex_normals if write_vertex_normals else None
    _write_ply(filename, mesh.vertices, normals, mesh.triangles)
    return True


def read_triangle_mesh(filename):
    """Read a PLY mesh written by ``write_triangle_mesh`` (or any binary PLY with x/y/z[, nx/ny/nz]
    and triangle faces) back as a :class:`TriangleMesh` (float32 positions, int32 triangles)."""
    props, faces = read_ply(filename)
    v = np.stack([props["x"], props["y"], props["z"]], 1).astype(np.float32)
    nrm = (np.stack([props["nx"], props["ny"], props["nz"]], 1).astype(np.float32) if "nx" in props
           else np.zeros_like(v))
    tris = (faces if faces is not None else np.zeros((0, 3))).astype(np.int32)
    return TriangleMesh(v, nrm, tris)
