"""filter_mesh_components on the GPU.

Same signature, messages and result as the reference's
``processing/reconstruction/utils/o3d_utils.py:241-321``: drop edge-connected triangle clusters
smaller than ``min_triangle_count`` (keep the largest if none qualifies), then the Open3D legacy
clean-up sequence (unreferenced vertices, degenerate / duplicated triangles, duplicated vertices,
non-manifold edges).  All of it runs in libmqr_hip.so (csrc/meshfilter.hip); non-manifold edges
are visited in ascending vertex-pair order where Open3D uses its hash-map order.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from ._lib import MQR_HOST, call, ptr
from .geometry import DeviceGeom, Tensor, TriangleMesh, device_mesh, host_rows, mesh_fields


STAT_KEYS = ("input_triangles", "clusters", "kept_clusters", "small_cluster_triangles", "largest_cluster",
             "non_manifold_removed", "triangles", "vertices")


def filter_mesh_components_gpu(vertices, normals, triangles, min_triangle_count: int = 2000, device: int = 0):
    """Arrays in, (vertices, normals, triangles, stats dict) out."""
    v, t = host_rows(vertices, np.float32), host_rows(triangles, np.int32)
    n = None if normals is None else host_rows(normals, np.float32)
    g = ctypes.c_void_p()
    stats = np.zeros(8, np.int64)
    call("mqr_mesh_filter_components", int(device), ptr(v), None if n is None else ptr(n), v.shape[0], ptr(t),
         t.shape[0], MQR_HOST, int(min_triangle_count), ctypes.byref(g), ptr(stats, _lib._i64p))
    try:
        nv, nt = ctypes.c_int64(), ctypes.c_int64()
        call("mqr_geom_counts", g, ctypes.byref(nv), ctypes.byref(nt))
        pos = np.empty((nv.value, 3), np.float32)
        nrm = np.empty((nv.value, 3), np.float32)
        tri = np.empty((nt.value, 3), np.int32)
        call("mqr_geom_copy", g, ptr(pos), ptr(nrm), ptr(tri) if nt.value else None, MQR_HOST)
    finally:
        call("mqr_geom_free", g)
    return pos, (nrm if n is not None else None), tri, dict(zip(STAT_KEYS, (int(x) for x in stats)))


def _filter_device(d, min_triangle_count):
    """The tensor mesh in HBM (``d``: its DeviceMesh), filtered without a host round trip; the result stays in HBM."""
    g = ctypes.c_void_p()
    stats = np.zeros(8, np.int64)
    call("mqr_mesh_filter_components", d.device, ctypes.c_void_p(d.positions),
         None if d.normals is None else ctypes.c_void_p(d.normals), d.nv, ctypes.c_void_p(d.triangles), d.nt,
         _lib.MQR_DEVICE, int(min_triangle_count), ctypes.byref(g), ptr(stats, _lib._i64p))
    geom = DeviceGeom(g, d.device)
    p, n, t = geom.tensors()
    if d.normals is None:
        n = Tensor(np.zeros((geom.nv, 3), np.float32))
    return p, n, t, dict(zip(STAT_KEYS, (int(x) for x in stats)))


def filter_mesh_components(mesh, min_triangle_count: int = 2000):
    """Drop-in for the reference's filter_mesh_components (o3d_utils.py:241-321).  A mesh in HBM (this
    package's extraction) is filtered there and the result stays there, as the reference's tensor mesh
    does on its CUDA device.  Which meshes take the device path: geometry.device_mesh."""
    from .vbg import parse_device
    f = mesh_fields(mesh)
    dev_id = parse_device(f.device)
    d = device_mesh(f, dev_id, normals=True)
    if d is None:
        v, t = host_rows(f.positions, np.float32), host_rows(f.triangles, np.int32)
    if (t.shape[0] if d is None else d.nt) == 0:
        print("[Warning] Mesh filtering: Input mesh has no triangles, returning as-is")
        return mesh
    if d is not None:
        pos, nrm, tri, st = _filter_device(d, min_triangle_count)
    else:
        n = None if f.normals is None else host_rows(f.normals, np.float32)
        if n is not None and n.shape[0] != v.shape[0]:
            n = None
        pos, nrm, tri, st = filter_mesh_components_gpu(v, n, t, min_triangle_count, dev_id)
        if nrm is None:
            nrm = np.zeros_like(pos)
    return _report_filter(TriangleMesh(pos, nrm, tri, device=f.device), st, min_triangle_count)


def _report_filter(out, st, min_triangle_count):
    """The reference's messages (o3d_utils.py:288-319) from the filter's statistics."""
    kept, comps = st["kept_clusters"], st["clusters"]
    if st["largest_cluster"] < min_triangle_count:  # no cluster qualified: the largest was kept
        print(f"[Warning] Mesh filtering: No components have >= {min_triangle_count} triangles. "
              f"Largest component has {st['largest_cluster']} triangles.")
        print("[Warning] Mesh filtering: Returning largest component only.")
    removed = comps - kept
    if removed > 0:
        print(f"[Info] Mesh filtering: Found {comps} connected component(s)")
        print(f"[Info] Mesh filtering: Removed {removed} small component(s) with < {min_triangle_count} triangles")
        print(f"[Info] Mesh filtering: Removed {st['small_cluster_triangles']} triangles from small components")
        print(f"[Info] Mesh filtering: Kept {kept} component(s) with >= {min_triangle_count} triangles")
        print(f"[Info] Mesh filtering: Final mesh has {st['triangles']} triangles (was {st['input_triangles']})")
    else:
        print(f"[Info] Mesh filtering: All {comps} component(s) have >= {min_triangle_count} triangles, "
              f"no filtering needed")
    return out
