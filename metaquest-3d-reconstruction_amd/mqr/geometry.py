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

    def colors(self):
        """The result's vertex colours as a Tensor over HBM, or None (made by the extraction of a coloured volume
        and by the simplification of a coloured mesh)."""
        from . import _lib
        c = ctypes.c_void_p()
        _lib.call("mqr_geom_device_colors", self._h, ctypes.byref(c))
        if not c.value:
            return None
        return Tensor(DeviceArray(self, c.value, (self.nv, 3), np.float32, self.device_id))

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


class GridTooFine(RuntimeError):
    """A clustering grid of 2^21 or more cells along an axis."""


class ResidentMesh:
    """A mesh's arrays as device pointers for the clustering entries (csrc/meshsimplify.hip): in place when the
    mesh is held in HBM (``device_mesh``), else validated on the host and uploaded once, before the first call
    that needs the device, to ``parse_device(mesh.device)``.  ``in_place`` tells which; ``free()`` releases what
    was uploaded."""

    def __init__(self, mesh):
        from .vbg import parse_device
        f = mesh_fields(mesh)
        d = device_mesh(f, normals=True, colors=True)
        self._held, self._pending, self._host_v = [], [], None
        self.positions = self.triangles = self.normals = self.colors = None
        self.in_place = d is not None
        try:
            if d is not None:
                self.device, self.nv, self.nt = d.device, d.nv, d.nt
                self.positions, self.triangles = d.positions, d.triangles
                self.normals = d.normals if d.normals is not None or f.normals is None else self._rows("normals", f.normals)
                self.colors = d.colors if d.colors is not None or f.colors is None else self._rows("colors", f.colors)
            else:
                self.device = parse_device(f.device)
                v = host_rows(f.positions, np.float32)
                t = np.asarray(host_array(f.triangles)).reshape(-1, 3)
                self.nv, self.nt = len(v), len(t)
                if not np.isfinite(v).all():
                    raise ValueError("a vertex coordinate is not finite")
                if len(t) and (t.min() < 0 or t.max() >= len(v)):
                    raise ValueError(f"a triangle index is outside [0, {len(v)})")
                self._host_v = v
                self._later("positions", v)
                self._later("triangles", np.ascontiguousarray(t, dtype=np.int32))
                if f.normals is not None:
                    self.normals = self._rows("normals", f.normals)
                if f.colors is not None:
                    self.colors = self._rows("colors", f.colors)
        except Exception:
            self.free()
            raise

    def _later(self, attr, a):
        if len(a):
            self._pending.append((attr, a))

    def _rows(self, name, x):
        rows = host_rows(x, np.float32)
        if rows.shape != (self.nv, 3):
            raise ValueError(f"vertex {name} must be {(self.nv, 3)}, got {rows.shape}")
        self._later(name, rows)
        return None

    def _upload(self):
        from . import _lib
        while self._pending:
            attr, a = self._pending.pop(0)
            self._held.append(_lib.DeviceBuffer.from_array(a, self.device))
            setattr(self, attr, self._held[-1].ptr.value)

    def free(self):
        for b in self._held:
            b.free()
        self._held, self._pending = [], []

    def bounds(self):
        """(min, max) of the coordinates, float64: numpy on a host mesh, mqr_vertex_bounds in HBM (a -0 reads +0)."""
        from . import _lib
        if self._host_v is not None:
            return self._host_v.min(0).astype(np.float64) + 0.0, self._host_v.max(0).astype(np.float64) + 0.0
        lo, hi = np.empty(3, np.float64), np.empty(3, np.float64)
        _clustering_call("mqr_vertex_bounds", self.device, ctypes.c_void_p(self.positions), self.nv, _lib.MQR_DEVICE,
                         _lib.ptr(lo, _lib._f64p), _lib.ptr(hi, _lib._f64p))
        return lo, hi

    def cluster_count(self, voxel_size: float) -> int:
        """The vertex count ``simplify`` would give at ``voxel_size`` (mqr_mesh_cluster_count)."""
        from . import _lib
        self._upload()
        n = ctypes.c_int64()
        _clustering_call("mqr_mesh_cluster_count", self.device, ctypes.c_void_p(self.positions), self.nv,
                         _lib.MQR_DEVICE, float(voxel_size), ctypes.byref(n))
        return int(n.value)

    def simplify(self, voxel_size: float):
        """mqr_mesh_simplify_clustering -> (DeviceGeom, stats[8])."""
        from . import _lib
        self._upload()
        vp = ctypes.c_void_p
        g, stats = vp(), np.zeros(8, np.int64)
        _clustering_call("mqr_mesh_simplify_clustering", self.device, vp(self.positions), self.nv, vp(self.normals),
                         vp(self.colors), vp(self.triangles), self.nt, _lib.MQR_DEVICE, float(voxel_size),
                         ctypes.byref(g), _lib.ptr(stats, _lib._i64p))
        return DeviceGeom(g, self.device), stats


def _clustering_call(name, *args):
    """The library's input errors as the Python mirror reports them: ValueError for bad values, GridTooFine
    (a RuntimeError) for a grid past the limit; anything else stays an MqrError."""
    from . import _lib
    try:
        return _lib.call(name, *args)
    except _lib.MqrError as e:
        msg = str(e)
        if "too fine" in msg:
            raise GridTooFine(msg) from e
        if any(k in msg for k in ("not finite", "outside [0", "voxel_size must", "no vertices")):
            raise ValueError(msg) from e
        raise


def _contraction_is_average(contraction) -> bool:
    """None and anything named Average (a string or an enum member such as Open3D's
    SimplificationContraction.Average) select the one contraction there is; Quadric is NotImplementedError."""
    if contraction is None:
        return True
    name = str(getattr(contraction, "name", contraction)).rsplit(".", 1)[-1].lower()
    if name == "average":
        return True
    if name == "quadric":
        raise NotImplementedError("simplify_vertex_clustering: only the Average contraction is implemented "
                                  "(Quadric is out of scope, DESIGN §7)")
    raise ValueError(f"simplify_vertex_clustering: unknown contraction {contraction!r}")


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


def color_to_uint8(colors) -> np.ndarray:
    """Open3D's ColorToUint8 as recalled (VERIFY): ``floor(clamp(c, 0, 1) * 255 + 0.5)`` as uint8, in float64."""
    c = np.clip(np.asarray(colors, np.float64), 0.0, 1.0)
    return np.floor(c * 255.0 + 0.5).astype(np.uint8)


def _write_ply(path, verts, normals=None, tris=None, colors=None):
    """Binary little-endian PLY in the layout Open3D's legacy writers use (``write_point_cloud`` /
    ``write_triangle_mesh`` with ``write_ascii=False``, reference ``reconstruction_data_io.py:57-145``;
    upstream FilePLY.cpp as recalled -- VERIFY): a ``comment Created by Open3D`` line, vertex
    coordinates and normals as ``double`` (the legacy geometry holds float64), then -- for geometry with
    colours -- ``uchar red / green / blue`` (``color_to_uint8``), faces as a ``uchar`` count followed by
    ``uint`` indices.  The float32 device values widen to float64 exactly.  Without colours the file is
    byte for byte what it was before colours were supported."""
    verts = np.asarray(verts, np.float64).reshape(-1, 3)
    n = len(verts)
    props = ["property double x", "property double y", "property double z"]
    cols = [verts]
    if normals is not None and len(normals) == n:
        props += ["property double nx", "property double ny", "property double nz"]
        cols.append(np.asarray(normals, np.float64).reshape(-1, 3))
    rgb = None
    if colors is not None and len(colors) == n:
        props += ["property uchar red", "property uchar green", "property uchar blue"]
        rgb = color_to_uint8(colors).reshape(-1, 3)
    header = ["ply", "format binary_little_endian 1.0", "comment Created by Open3D", f"element vertex {n}"] + props
    if tris is not None:
        header += [f"element face {len(tris)}", "property list uchar uint vertex_indices"]
    header.append("end_header")
    with open(path, "wb") as f:
        f.write(("\n".join(header) + "\n").encode())
        body = np.ascontiguousarray(np.concatenate(cols, axis=1), dtype="<f8")
        if rgb is None:
            f.write(body.tobytes())
        else:
            rec = np.empty(n, dtype=[("d", "<f8", (body.shape[1],)), ("c", "u1", (3,))])
            rec["d"] = body
            rec["c"] = rgb
            f.write(rec.tobytes())
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
    def __init__(self, positions, normals, device=None, colors=None):
        self.point = _AttrMap(positions=_tensor(positions), normals=_tensor(normals))
        if colors is not None:
            self.point["colors"] = _tensor(colors)
        self.device = device

    @classmethod
    def from_device(cls, geom: DeviceGeom, device=None):
        p, n, _ = geom.tensors()
        return cls(p, n, device=device, colors=geom.colors())

    @property
    def points(self):
        return self.point.positions.numpy()

    @property
    def normals(self):
        return self.point.normals.numpy()

    @property
    def colors(self):
        """The per-point colours (float32 in [0, 1]) as a host array, or None for a cloud without colours."""
        c = self.point.get("colors")
        return None if c is None else c.numpy()

    def has_colors(self) -> bool:
        return self.point.get("colors") is not None

    def cpu(self):
        c = self.point.get("colors")
        return PointCloud(self.point.positions.cpu(), self.point.normals.cpu(), device="CPU:0",
                          colors=None if c is None else c.cpu())

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
        if self.has_colors():
            pcd.colors = o3d.utility.Vector3dVector(self.colors.astype(np.float64))
        return pcd

    def write_ply(self, path):
        _write_ply(path, self.points, self.normals, colors=self.colors)

    def uniform_down_sample(self, every_k_points: int):
        """Points 0, k, 2k, ... (``o3d.t.geometry.PointCloud.uniform_down_sample``) as a host cloud."""
        k = int(every_k_points)
        if k < 1:
            raise ValueError("every_k_points must be >= 1")
        c = self.colors
        return PointCloud(self.points[::k].copy(), self.normals[::k].copy(), device=self.device,
                          colors=None if c is None else c[::k].copy())

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
        mesh = cls(*geom.tensors(), device=device)
        c = geom.colors()
        if c is not None:
            mesh.vertex["colors"] = c
        return mesh

    @property
    def vertices(self):
        return self.vertex.positions.numpy()

    @property
    def vertex_normals(self):
        return self.vertex.normals.numpy()

    @property
    def triangles(self):
        return self.triangle.indices.numpy()

    @property
    def vertex_colors(self):
        """The per-vertex colours (``vertex["colors"]``, float32 in [0, 1]) as a host array, or None."""
        c = self.vertex.get("colors")
        return None if c is None else _tensor(c).numpy()

    def has_vertex_colors(self) -> bool:
        return self.vertex.get("colors") is not None

    def cpu(self):
        mesh = TriangleMesh(self.vertex.positions.cpu(), self.vertex.normals.cpu(), self.triangle.indices.cpu(),
                            device="CPU:0")
        if self.has_vertex_colors():
            mesh.vertex["colors"] = _tensor(self.vertex["colors"]).cpu()
        return mesh

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
        if self.has_vertex_colors():
            m.vertex_colors = o3d.utility.Vector3dVector(self.vertex_colors.astype(np.float64))
        return m

    def write_ply(self, path):
        _write_ply(path, self.vertices, self.vertex_normals, self.triangles, colors=self.vertex_colors)

    def sample_points_uniformly(self, number_of_points: int, use_triangle_normal: bool = False, seed: int = 0):
        """``number_of_points`` area-weighted samples of the surface as a :class:`PointCloud` (Open3D's
        ``sample_points_uniformly``; reference ``reconstruct_scene.py:151-171``), drawn on the GPU
        (csrc/meshsample.hip).  A mesh held in HBM is read in place and the cloud stays on its device; a host
        mesh is sampled on ``parse_device(self.device)`` and the cloud comes back to the host.  The cloud
        carries ``point.colors`` when the mesh has ``vertex["colors"]``; normals are the vertex normals under
        the point's barycentric weights (not renormalised), or the triangle's unit normal with
        ``use_triangle_normal``.

        The rule is this package's own (Open3D's ``std::mt19937`` stream is not matched): sample
        ``i`` depends on the mesh, ``seed`` and ``i`` alone, so calls with another ``number_of_points`` share
        their first samples, and host and device meshes give identical bits.  ``RuntimeError`` for
        ``number_of_points <= 0`` or a mesh without triangles (as Open3D), and for a mesh whose every triangle
        is degenerate; ``ValueError`` for a non-finite coordinate, a triangle index out of range, or normals /
        colours that are not shaped like the positions (checked on the host before anything is launched)."""
        from . import _lib
        from .vbg import parse_device
        n = int(number_of_points)
        if n <= 0:
            raise RuntimeError("[sample_points_uniformly] number_of_points <= 0")
        f = mesh_fields(self)
        if int(np.prod(f.triangles.shape[:-1])) == 0 or int(np.prod(f.positions.shape[:-1])) == 0:
            raise RuntimeError("[sample_points_uniformly] input mesh has no triangles")
        seed = int(seed) & (2 ** 64 - 1)
        d = device_mesh(f, normals=True, colors=True)
        held = []  # device buffers of fields uploaded for this call

        def upload(name, x, dev, nv):
            # a field that is not usable in place (a host tensor, another dtype or device): the kernel gathers
            # nv rows from it and the C ABI takes no length, so its shape is checked here, before any launch
            rows = host_rows(x, np.float32)
            if rows.shape != (nv, 3):
                raise ValueError(f"vertex {name} must be {(nv, 3)}, got {rows.shape}")
            held.append(_lib.DeviceBuffer.from_array(rows, dev))
            return held[-1].ptr.value

        try:
            if d is not None:
                dev, nv, nt, loc = d.device, d.nv, d.nt, _lib.MQR_DEVICE
                pv, pt = d.positions, d.triangles
                pn = (None if use_triangle_normal else d.normals if d.normals is not None
                      else upload("normals", f.normals, dev, nv))
                pc = (None if f.colors is None else d.colors if d.colors is not None
                      else upload("colors", f.colors, dev, nv))
            else:
                dev, loc = parse_device(self.device), _lib.MQR_HOST
                v, t = host_rows(f.positions, np.float32), np.asarray(host_array(f.triangles)).reshape(-1, 3)
                if not np.isfinite(v).all():
                    raise ValueError("a vertex coordinate is not finite")
                if t.min() < 0 or t.max() >= len(v):
                    raise ValueError(f"a triangle index is outside [0, {len(v)})")
                t = np.ascontiguousarray(t, dtype=np.int32)
                hn = None if use_triangle_normal else host_rows(f.normals, np.float32)
                hc = None if f.colors is None else host_rows(f.colors, np.float32)
                for name, x in (("normals", hn), ("colors", hc)):
                    if x is not None and x.shape != v.shape:
                        raise ValueError(f"vertex {name} must be {v.shape}, got {x.shape}")
                nv, nt = len(v), len(t)
                pv, pt = v.ctypes.data, t.ctypes.data
                pn, pc = (None if x is None else x.ctypes.data for x in (hn, hc))
            if d is not None:
                outs = [_lib.DeviceBuffer(12 * n, dev) for _ in range(3 if pc is not None else 2)]
                optr = [b.ptr.value for b in outs]
                wrap = [Tensor(DeviceArray(b, b.ptr.value, (n, 3), np.float32, dev)) for b in outs]
            else:
                outs = [np.empty((n, 3), np.float32) for _ in range(3 if pc is not None else 2)]
                optr = [a.ctypes.data for a in outs]
                wrap = outs
            vp = ctypes.c_void_p
            try:
                _lib.call("mqr_mesh_sample_points", int(dev), vp(pv), nv, vp(pn), vp(pc), vp(pt), nt, loc, n, seed,
                          1 if use_triangle_normal else 0, vp(optr[0]), vp(optr[1]),
                          vp(optr[2]) if pc is not None else None, None, loc)
            except _lib.MqrError as e:
                if "not finite" in str(e) or "outside [0" in str(e):
                    raise ValueError(str(e)) from e
                raise
        finally:
            for b in held:
                b.free()
        return PointCloud(wrap[0], wrap[1], device=self.device, colors=wrap[2] if pc is not None else None)

    def simplify_vertex_clustering(self, voxel_size: float, contraction=None):
        """Open3D's ``simplify_vertex_clustering(voxel_size, SimplificationContraction.Average)`` (reference
        ``scripts/downsample_fbx_mesh.py:244-270``) on the GPU (csrc/meshsimplify.hip): one output vertex per
        occupied cell of a grid of ``voxel_size`` -- the mean of the cell's vertices, normals and
        ``vertex["colors"]`` -- and the triangles that keep three distinct corners, once each.  The rule is
        DESIGN §2.9, restated from Open3D as recalled (unpinned); output vertices and triangles are in order of
        first appearance where Open3D follows its hash containers.  A mesh held in HBM is read in place and the
        result stays on its device; a host mesh runs on ``parse_device(self.device)`` and comes back as host
        arrays; both give identical bits.  Only the Average contraction exists (``contraction`` None or Average;
        Quadric raises NotImplementedError).  ``ValueError`` for a non-finite coordinate, a triangle index out of
        range, normals or colours not shaped like the positions, or a ``voxel_size`` that is not finite and
        positive; ``RuntimeError`` (``GridTooFine``) for a grid of 2^21 or more cells along an axis."""
        return simplify_vertex_clustering(self, voxel_size, contraction)


def simplify_vertex_clustering(mesh, voxel_size: float, contraction=None):
    """:meth:`TriangleMesh.simplify_vertex_clustering` for anything ``mesh_fields`` unpacks (a tensor or legacy
    mesh, a ``(vertices, triangles[, colors])`` tuple); the result is a :class:`TriangleMesh`."""
    _contraction_is_average(contraction)
    voxel_size = float(voxel_size)
    if not np.isfinite(voxel_size) or voxel_size <= 0.0:
        raise ValueError(f"voxel_size must be finite and > 0, got {voxel_size}")
    r = ResidentMesh(mesh)
    try:
        if r.nv == 0:
            raise ValueError("[simplify_vertex_clustering] the mesh has no vertices")
        return _simplified_mesh(r, voxel_size, mesh_fields(mesh).device)[0]
    finally:
        r.free()


def _simplified_mesh(r: ResidentMesh, voxel_size: float, device):
    """(TriangleMesh, stats) of one clustering call on a resident mesh: in HBM when the input was, else host arrays."""
    geom, stats = r.simplify(voxel_size)
    p, n, t = geom.tensors()
    c = geom.colors()
    if not r.in_place:
        p, n, t = Tensor(p.numpy()), Tensor(n.numpy()), Tensor(t.numpy())
        c = None if c is None else Tensor(c.numpy())
    mesh = TriangleMesh(p, n, t, device=device)
    if c is not None:
        mesh.vertex["colors"] = c
    return mesh, stats


# ---- o3d.io mirror for the reference's writers (reconstruction_data_io.py:57-145) ------------------
def _colors_of(obj, attr):
    """The colour array of a legacy-style geometry (``.colors`` / ``.vertex_colors``), or None when it has
    none (``has_colors()`` / ``has_vertex_colors()`` honoured where the object has them; an empty array is none)."""
    has = getattr(obj, "has_" + attr, None)
    if callable(has) and not has():
        return None
    c = getattr(obj, attr, None)
    if c is None:
        return None
    c = np.asarray(c)
    return c if c.size else None


def write_point_cloud(filename, pointcloud, write_ascii=False, compressed=False, print_progress=False):
    """``o3d.io.write_point_cloud`` for ``.ply`` (binary; ``compressed`` has no effect on PLY in
    Open3D either); a cloud with colours gets ``uchar red / green / blue``.  Returns True like Open3D."""
    if write_ascii:
        raise NotImplementedError("ASCII PLY is not written by the reference pipeline")
    if not str(filename).lower().endswith(".ply"):
        raise ValueError("only .ply is supported")
    _write_ply(filename, pointcloud.points, pointcloud.normals, colors=_colors_of(pointcloud, "colors"))
    return True


def write_triangle_mesh(filename, mesh, write_ascii=False, compressed=False, write_vertex_normals=True,
                        write_vertex_colors=True, write_triangle_uvs=True, print_progress=False):
    """``o3d.io.write_triangle_mesh`` for ``.ply`` meshes (the colorless raw and clean meshes and the
    coloured mesh, ``reconstruction_data_io.py:68-101``): vertex colours are written when the mesh has them
    and ``write_vertex_colors`` is set.  Returns True like Open3D."""
    if write_ascii:
        raise NotImplementedError("ASCII PLY is not written by the reference pipeline")
    if not str(filename).lower().endswith(".ply"):
        raise ValueError("only .ply is supported")
    normals = mesh.vertex_normals if write_vertex_normals else None
    colors = _colors_of(mesh, "vertex_colors") if write_vertex_colors else None
    _write_ply(filename, mesh.vertices, normals, mesh.triangles, colors=colors)
    return True


def _ply_vertex_fields(props):
    v = np.stack([props["x"], props["y"], props["z"]], 1).astype(np.float32)
    nrm = (np.stack([props["nx"], props["ny"], props["nz"]], 1).astype(np.float32) if "nx" in props
           else np.zeros_like(v))
    col = None
    if all(k in props for k in ("red", "green", "blue")):
        col = (np.stack([props["red"], props["green"], props["blue"]], 1).astype(np.float64) / 255.0).astype(np.float32)
    return v, nrm, col


def read_triangle_mesh(filename):
    """Read a PLY mesh written by ``write_triangle_mesh`` (or any binary PLY with x/y/z[, nx/ny/nz][, red/green/
    blue] and triangle faces) back as a :class:`TriangleMesh` (float32 positions, int32 triangles; colours
    ``uchar / 255`` as float32 in ``vertex["colors"]`` when the file has them)."""
    props, faces = read_ply(filename)
    v, nrm, col = _ply_vertex_fields(props)
    tris = (faces if faces is not None else np.zeros((0, 3))).astype(np.int32)
    mesh = TriangleMesh(v, nrm, tris)
    if col is not None:
        mesh.vertex["colors"] = Tensor(col)
    return mesh


def read_point_cloud(filename):
    """Read a PLY point cloud written by ``write_point_cloud`` back as a :class:`PointCloud` (float32
    positions and normals -- zeros when the file has none -- and colours ``uchar / 255`` as float32 when the
    file has them)."""
    props, _ = read_ply(filename)
    v, nrm, col = _ply_vertex_fields(props)
    return PointCloud(v, nrm, colors=col)
