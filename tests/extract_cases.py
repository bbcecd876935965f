"""Hand-built volumes for the surface-extraction tests, and what they cover.  Plain numpy: no GPU,
no oracle.  tests/test_extract_cases_ref.py asserts the coverage these volumes promise and
tests/test_gpu_extract_cases.py extracts them on the device against the oracle; both take their
(R, G, seed) tuples from the constants below, so the asserted coverage is the tested coverage.

Layout.  A volume is ``Volume(keys, tsdf, weight, ...)``: the first three fields are what
``import_blocks`` takes (keys (n,3) int32 = block (x, y, z); tsdf / weight (n,R,R,R) float32 indexed
[block, z, y, x]).  The remaining fields are the global grids ([z, y, x] over the G^3 block cube,
G*R voxels a side) the coverage counters read: ``sign`` (tsdf < 0), ``wgrid`` (the weights) and
``present`` (per block [bz, by, bx]: the block is in the volume), and the block-grid ``origin``.

Cube corner k sits at mc_tables.VTX_SHIFTS[k] from the cube's origin voxel and sets bit k of the case
when its tsdf is negative (include/mqr_mc_tables.h).
"""
from __future__ import annotations

import os
import sys
from typing import NamedTuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import mc_tables  # noqa: E402

ORIGIN = (-3, -2, -4)   # block-grid origin of the dense volumes: small keys, negatives included
VOXEL_SIZE = 0.01
THRESHOLD = 1.5         # the weights of mode (b) are drawn around it; 1.5 itself is not valid
MIXED_WEIGHTS = (3.0, 2.0, 1.5, 1.0, 0.0)
MIXED_PROBS = (0.55, 0.35, 0.04, 0.03, 0.03)   # 10 % of the voxels at or below the threshold
SCAN_TILE = 8192        # kScanTile of k_scan_counts (extract.hip): 1024 threads x 8 counts

# The all-valid volumes of the "all cases, all seams" test, per block resolution: (G, seed) each.
# Their union covers all 256 cube cases in each of the 8 seam classes (asserted on the CPU).
DENSE = {
    8: ((8, 1),),
    16: ((8, 1),),
    12: ((8, 1),),
    4: ((8, 1), (8, 2)),
}
# Mode (b): mixed weights, dropped blocks, garbage under weight 0.  (R -> (G, seed, drop share))
MIXED = {8: (6, 3, 0.25), 16: (6, 3, 0.25), 12: (6, 3, 0.25)}
ZEROS = {8: (4, 5), 12: (4, 5)}       # (G, seed): 3 % +0.0 and 3 % -0.0
NANS = {8: (4, 6), 12: (4, 6)}        # (G, seed): 2 % NaN
SCALED = {8: (4, 7), 16: (3, 7), 12: (3, 7)}   # (G, seed) of the 2^-100 / 2^-130 volumes
SPARSE = (8, SCAN_TILE + 300, 8)      # (R, blocks, seed)
OWNED = (8, 4, 9)                     # (R, G, seed)
SPHERES = {8: 4, 12: 4}               # R -> G; radius = SPHERE_RADIUS * R voxels
SPHERE_RADIUS = 1.4125                # x R: 11.3 voxels at R = 8, through the block corners (+-R, +-R, 0)


class Volume(NamedTuple):
    keys: np.ndarray
    tsdf: np.ndarray
    weight: np.ndarray
    sign: np.ndarray
    wgrid: np.ndarray
    present: np.ndarray
    origin: tuple
    R: int


def _to_blocks(grid, R, G):
    """[z, y, x] global grid -> (G^3, R, R, R) blocks in (bz, by, bx) order."""
    return np.ascontiguousarray(grid.reshape(G, R, G, R, G, R).transpose(0, 2, 4, 1, 3, 5)).reshape(G ** 3, R, R, R)


def _pack(tsdf_grid, wgrid, present, origin, R, G, rng):
    """Blocks of the present part of the grid, in a seeded random order (the order is the
    importer's business; a sorted one would hide a dependence on it)."""
    bz, by, bx = np.nonzero(present)
    keys = np.stack([bx + origin[0], by + origin[1], bz + origin[2]], axis=1).astype(np.int32)
    sel = (bz * G + by) * G + bx
    order = rng.permutation(len(sel))
    tsdf = _to_blocks(tsdf_grid, R, G)[sel][order]
    weight = _to_blocks(wgrid, R, G)[sel][order]
    assert np.abs(keys).max() <= 64
    return keys[order], tsdf.astype(np.float32), weight.astype(np.float32)


def dense_signs(R, G, seed, weights="valid", drop=0.0, zeros=0.0, nans=0.0, origin=ORIGIN):
    """G^3 blocks of independent random signs, magnitudes uniform in [0.05, 1].  The cube at every
    8-block corner (origin voxel R-1 on all three axes within its block) then gets its eight corner
    signs overwritten so that these cubes enumerate the cases 0, 1, 2, ... (mod 256): there is one
    such cube per block corner, (G-1)^3 in all, R voxels apart, so random signs cannot cover them.

    weights: "valid" = all 3.0; "mixed" = MIXED_WEIGHTS with MIXED_PROBS, a weight-0 voxel carrying
    an arbitrary tsdf in [-50, 50] (normals read it whatever its weight), and a share ``drop`` of the
    blocks of the last two x-slabs removed, with the cube's far corner block left without any
    neighbour.  zeros / nans: that share of the voxels set to +0.0 and as many to -0.0 / to NaN."""
    rng = np.random.default_rng(seed)
    N = R * G
    mag = rng.uniform(0.05, 1.0, (N, N, N)).astype(np.float32)
    neg = rng.random((N, N, N)) < 0.5
    wgrid = np.full((N, N, N), 3.0, np.float32)
    present = np.ones((G, G, G), bool)
    if weights == "mixed":
        wgrid = rng.choice(np.array(MIXED_WEIGHTS, np.float32), size=(N, N, N), p=MIXED_PROBS)
        garbage = rng.uniform(-50.0, 50.0, (N, N, N)).astype(np.float32)
        dead = wgrid == 0
        mag[dead] = np.abs(garbage[dead])
        neg[dead] = garbage[dead] < 0
        present[:, :, G - 2:] &= rng.random((G, G, 2)) >= drop
        present[G - 2:, G - 2:, G - 2:] = False
        present[G - 1, G - 1, G - 1] = True
    else:
        assert weights == "valid" and drop == 0.0
    n = 0
    for bz in range(G - 1):
        for by in range(G - 1):
            for bx in range(G - 1):
                x, y, z = bx * R + R - 1, by * R + R - 1, bz * R + R - 1
                for k, (dx, dy, dz) in enumerate(mc_tables.VTX_SHIFTS):
                    neg[z + dz, y + dy, x + dx] = (n >> k) & 1
                n = (n + 1) % 256
    tsdf = np.where(neg, -mag, mag).astype(np.float32)
    if zeros:
        u = rng.random((N, N, N))
        tsdf[u < zeros] = 0.0
        tsdf[(u >= zeros) & (u < 2 * zeros)] = -0.0
    if nans:
        tsdf[rng.random((N, N, N)) < nans] = np.nan
    keys, bt, bw = _pack(tsdf, wgrid, present, origin, R, G, rng)
    return Volume(keys, bt, bw, tsdf < 0, wgrid, present, tuple(origin), R)


def sphere(R, G, radius, centre=(0.3, -0.2, 0.1), scale=0.125):
    """An analytic sphere: tsdf = scale * (|p - centre| - radius) at the voxel positions p (in
    voxels) of a G^3 block cube centred on the origin (keys -G/2 .. G/2-1), all weights 3.0.  With
    radius ~ sqrt(2) R the surface crosses block faces, edges and the corners (+-R, +-R, 0)."""
    N = R * G
    o = -(G // 2)
    c = np.arange(N, dtype=np.float64) + o * R
    z, y, x = np.meshgrid(c, c, c, indexing="ij")
    d = np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2)
    tsdf = (scale * (d - radius)).astype(np.float32)
    wgrid = np.full((N, N, N), 3.0, np.float32)
    present = np.ones((G, G, G), bool)
    keys, bt, bw = _pack(tsdf, wgrid, present, (o, o, o), R, G, np.random.default_rng(0))
    return Volume(keys, bt, bw, tsdf < 0, wgrid, present, (o, o, o), R)


def sparse_many(R, n_blocks, seed, width=96, origin=(-40, -50, 3)):
    """A one-block-thick sheet of n_blocks blocks (more than one tile of the count scan), all
    weights 3.0, in row-major order of the sheet (not shuffled: ``has_output`` is in that order).
    Every third block holds three negative voxels, two of them off the block's faces (their
    vertices belong to the block itself), one anywhere (its cubes may cross a seam); every other
    block is uniformly positive, so most blocks have no output at all.
    Returns (keys, tsdf, weight, has_output)."""
    rng = np.random.default_rng(seed)
    i = np.arange(n_blocks)
    keys = np.stack([i % width + origin[0], i // width + origin[1], np.full(n_blocks, origin[2])], 1).astype(np.int32)
    assert np.abs(keys).max() <= 64
    tsdf = rng.uniform(0.05, 1.0, (n_blocks, R, R, R)).astype(np.float32)
    weight = np.full((n_blocks, R, R, R), 3.0, np.float32)
    has_output = i % 3 == 0
    for b in np.nonzero(has_output)[0]:
        inner = rng.integers(1, R - 1, (2, 3))
        anyw = rng.integers(0, R, (1, 3))
        for z, y, x in np.concatenate([inner, anyw]):
            tsdf[b, z, y, x] = -abs(tsdf[b, z, y, x])
    return keys, tsdf, weight, has_output


def scaled(vol, exponent):
    """The volume with every tsdf multiplied by 2^exponent (exact in float32 down to the denormals,
    where it rounds)."""
    return vol._replace(tsdf=np.ldexp(vol.tsdf, exponent).astype(np.float32))


# ---- coverage counters ---------------------------------------------------------------------------

def weight_ok(vol, thr=THRESHOLD):
    """[z, y, x]: the voxel's block is present and its weight is above the threshold."""
    R = vol.R
    p = np.repeat(np.repeat(np.repeat(vol.present, R, 0), R, 1), R, 2)
    return p & (vol.wgrid > thr)


def cube_cases(sign, ok):
    """Per cube origin voxel [z, y, x]: (case index, valid).  A cube is valid iff its eight corners
    are all ok; cubes reaching past the grid are not."""
    N = sign.shape[0]
    case = np.zeros((N, N, N), np.int32)
    valid = np.ones((N, N, N), bool)
    valid[-1, :, :] = valid[:, -1, :] = valid[:, :, -1] = False
    for k, (dx, dy, dz) in enumerate(mc_tables.VTX_SHIFTS):
        case[:N - dz, :N - dy, :N - dx] |= sign[dz:, dy:, dx:].astype(np.int32) << k
        valid[:N - dz, :N - dy, :N - dx] &= ok[dz:, dy:, dx:]
    return case, valid


def seam_class(N, R):
    """[z, y, x] -> 0..7: bit 0 / 1 / 2 set iff the cube origin is at R-1 on x / y / z, i.e. the
    cube reaches into the +x / +y / +z neighbour block."""
    s = (np.arange(N) % R == R - 1).astype(np.int32)
    return s[None, None, :] | (s[None, :, None] << 1) | (s[:, None, None] << 2)


def case_histogram(sign, ok, R):
    """(8, 256) counts of valid cubes per seam class and case."""
    case, valid = cube_cases(sign, ok)
    cls = seam_class(sign.shape[0], R)
    return np.bincount((cls[valid] * 256 + case[valid]).ravel(), minlength=8 * 256).reshape(8, 256)


def case_coverage(sign, ok, R):
    """Per seam class, how many of the 256 cases occur among the valid cubes."""
    return (case_histogram(sign, ok, R) > 0).sum(axis=1)


def complete_blocks(present):
    """[bz, by, bx]: the block is present and so are all 26 of its neighbours."""
    G = present.shape[0]
    p = np.zeros((G + 2,) * 3, bool)
    p[1:-1, 1:-1, 1:-1] = present
    out = present.copy()
    for dz in range(3):
        for dy in range(3):
            for dx in range(3):
                out &= p[dz:dz + G, dy:dy + G, dx:dx + G]
    return out


def isolated_blocks(present):
    """[bz, by, bx]: the block is present and none of its 26 neighbours is."""
    G = present.shape[0]
    p = np.zeros((G + 2,) * 3, np.int32)
    p[1:-1, 1:-1, 1:-1] = present
    cnt = sum(p[dz:dz + G, dy:dy + G, dx:dx + G] for dz in range(3) for dy in range(3) for dx in range(3))
    return present & (cnt == 1)


def triangles_per_block(vol, keys, thr=THRESHOLD):
    """Triangles of the valid cubes whose origin lies in each block of ``keys`` (n,3), in that order:
    the sum of mc_tables.TRI_COUNT[case] over the block's cubes."""
    R = vol.R
    G = vol.present.shape[0]
    case, valid = cube_cases(vol.sign, weight_ok(vol, thr))
    per_cube = np.where(valid, np.asarray(mc_tables.TRI_COUNT, np.int64)[case], 0)
    per_block = per_cube.reshape(G, R, G, R, G, R).sum(axis=(1, 3, 5))   # [bz, by, bx]
    k = np.asarray(keys, np.int64) - np.asarray(vol.origin, np.int64)
    return per_block[k[:, 2], k[:, 1], k[:, 0]]


# ---- mesh properties (sphere known answers; run on the oracle's and on the device's arrays) ---------

def mesh_topology(n_vertices, tri):
    """(watertight, V - E + F): watertight = every directed edge occurs once and so does its reverse."""
    tri = np.asarray(tri, np.int64)
    a = np.concatenate([tri[:, 0], tri[:, 1], tri[:, 2]])
    b = np.concatenate([tri[:, 1], tri[:, 2], tri[:, 0]])
    fwd = a * n_vertices + b
    rev = b * n_vertices + a
    ufwd, cnt = np.unique(fwd, return_counts=True)
    watertight = bool((cnt == 1).all() and np.array_equal(ufwd, np.unique(rev)))
    edges = len(np.unique(np.minimum(a, b) * n_vertices + np.maximum(a, b)))
    used = len(np.unique(tri))
    return watertight, used - edges + len(tri)


def sphere_errors(pos, nrm, radius, centre=(0.3, -0.2, 0.1), voxel_size=VOXEL_SIZE):
    """(max | |p - c| - radius | in voxels, min normal . radial) over the vertices."""
    p = np.asarray(pos, np.float64) / voxel_size - np.asarray(centre)
    d = np.linalg.norm(p, axis=1)
    return float(np.abs(d - radius).max()), float(((np.asarray(nrm, np.float64) * p).sum(1) / d).min())

