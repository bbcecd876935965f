"""Plain numpy restatement of the colour-frame decode, written independently of the product's host path
(mqr/colorframes.py): index arithmetic instead of strided views, floor division instead of shifts, its own
copy of the constants.  Test infrastructure: the product never imports this.

The three arithmetic pieces restate OpenCV 4.x as recalled (parity UNPINNED against OpenCV):

  I420 -> BGR   y = max(0, Y-16) * 1220542, u = U-128, v = V-128, rnd = 2^19
                r = sat8((y + 1673527 v + rnd) // 2^20)
                g = sat8((y - 852492 v - 409993 u + rnd) // 2^20)
                b = sat8((y + 2116026 u + rnd) // 2^20)          one (U,V) per 2x2 block
  BGR -> grey   (3735 B + 19235 G + 9798 R + 2^14) // 2^15
  Laplacian     [[0,1,0],[1,-4,1],[0,1,0]], border reflect-101

Hand-computed known answers (Y, U, V) -> (R, G, B), asserted by tests/test_colorframes_ref.py:
  (0, 128, 128)   -> (0, 0, 0)         y clamps at 16: max(0, -16) = 0, every channel 2^19 // 2^20 = 0
  (16, 128, 128)  -> (0, 0, 0)
  (17, 128, 128)  -> (1, 1, 1)         (1220542 + 524288) // 1048576 = 1
  (235, 128, 128) -> (255, 255, 255)   (219 * 1220542 + 524288) // 2^20 = 267822986 // 2^20 = 255, no clamp yet
  (255, 128, 128) -> (255, 255, 255)   292233826 // 2^20 = 278, clamped
  (0, 0, 0)       -> (0, 154, 0)       r: (-214211456 + 524288) // 2^20 = -204 -> 0; b: -270327040 // 2^20 < 0 -> 0
                                       g: (109118976 + 52479104 + 524288) // 2^20 = 162122368 // 2^20 = 154
  (255, 255, 255) -> (255, 125, 255)   g: (291709538 - 108266484 - 52069111 + 524288) // 2^20 = 131898231 // 2^20 = 125
  (0, 255, 255)   -> (203, 0, 255)     g: (-108266484 - 52069111 + 524288) < 0 -> 0; r, b: see KNOWN
  (255, 0, 0)     -> (74, 255, 20)     g: (291709538 + 161598080 + 524288) // 2^20 = 432 -> 255; r, b: see KNOWN
"""
import numpy as np

CY, CUB, CUG, CVG, CVR = 1220542, 2116026, -409993, -852492, 1673527
ONE = 1 << 20

# (Y, U, V) -> (R, G, B)
KNOWN = {
    (0, 128, 128): (0, 0, 0),
    (16, 128, 128): (0, 0, 0),
    (17, 128, 128): (1, 1, 1),
    (235, 128, 128): (255, 255, 255),
    (255, 128, 128): (255, 255, 255),
    (0, 0, 0): (0, 154, 0),
    (255, 255, 255): (255, 125, 255),
    # r: (1673527 * 127 + 524288) // 2^20 = 213062217 // 2^20 = 203; b: (2116026 * 127 + 524288) // 2^20 = 256
    (0, 255, 255): (203, 0, 255),
    # r: (291709538 - 214211456 + 524288) // 2^20 = 78022370 // 2^20 = 74; b: (291709538 - 270851328 + 524288) // 2^20 = 20
    (255, 0, 0): (74, 255, 20),
}


def layout_of(width, height, planes, uv_order="NV12"):
    """The reference's three unpacking branches (scripts/utils/image_utils.py:19-57) as byte addresses:
    {plane: (base, row stride, step, rows, cols)}.  planes: [(buffer_size, row_stride, pixel_stride)] * 3."""
    (ysz, yrs, yps), (usz, urs, ups), (_, vrs, _) = planes
    cw, ch = width // 2, height // 2
    if ups == 1:
        u, v = (ysz, urs, 1), (ysz + usz, vrs, 1)
    elif uv_order == "NV21":
        u, v = (ysz + 1, urs, 2), (ysz, urs, 2)
    else:
        u, v = (ysz, urs, 2), (ysz + 1, urs, 2)
    return {"y": (0, yrs, yps, height, width), "u": u + (ch, cw), "v": v + (ch, cw)}


def unpack(raw, layout):
    """-> Y (H,W), U, V (H/2,W/2) uint8 by explicit index arithmetic."""
    raw = np.asarray(raw, np.uint8).reshape(-1)
    out = []
    for name in ("y", "u", "v"):
        base, rs, step, rows, cols = layout[name]
        idx = base + rs * np.arange(rows)[:, None] + step * np.arange(cols)[None, :]
        out.append(raw[idx])
    return out


def yuv_to_rgb(Y, U, V):
    """(H,W) Y and (H/2,W/2) U, V -> (H,W,3) uint8 RGB."""
    y = np.maximum(Y.astype(np.int64) - 16, 0) * CY
    u = np.kron(U.astype(np.int64) - 128, np.ones((2, 2), np.int64))
    v = np.kron(V.astype(np.int64) - 128, np.ones((2, 2), np.int64))
    half = ONE // 2
    r = (y + CVR * v + half) // ONE
    g = (y + CVG * v + CUG * u + half) // ONE
    b = (y + CUB * u + half) // ONE
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


def decode(raw, width, height, planes, uv_order="NV12", order="rgb"):
    rgb = yuv_to_rgb(*unpack(raw, layout_of(width, height, planes, uv_order)))
    return rgb[..., ::-1].copy() if order == "bgr" else rgb


def grey_of(rgb):
    x = rgb.astype(np.int64)
    return (3735 * x[..., 2] + 19235 * x[..., 1] + 9798 * x[..., 0] + (1 << 14)) // (1 << 15)


def laplacian(grey):
    """ksize-1 Laplacian of an (H,W) integer image, border reflect-101 (row -1 is row 1, row H is row H-2)."""
    H, W = grey.shape
    ys = np.concatenate([[1], np.arange(H), [H - 2]])
    xs = np.concatenate([[1], np.arange(W), [W - 2]])
    p = grey.astype(np.int64)[ys][:, xs]
    return p[:-2, 1:-1] + p[2:, 1:-1] + p[1:-1, :-2] + p[1:-1, 2:] - 4 * p[1:-1, 1:-1]


def statistics(rgb):
    """-> (256-bin histogram of blue, uint32; [sum, sum of squares] of the Laplacian, int64) of one RGB image."""
    lap = laplacian(grey_of(rgb))
    return (np.bincount(rgb[..., 2].ravel(), minlength=256).astype(np.uint32),
            np.array([lap.sum(), (lap * lap).sum()], np.int64))


def to_yuv_file(rgb, row_pad=0):
    """An NV12 frame file (Android's short chroma planes) whose decode resembles `rgb`: (planes, bytes).
    A plain BT.601 forward transform -- only used to make test frames, never compared against."""
    H, W = rgb.shape[:2]
    x = rgb.astype(np.float64)
    y = 16 + (65.481 * x[..., 0] + 128.553 * x[..., 1] + 24.966 * x[..., 2]) / 255
    u = 128 + (-37.797 * x[..., 0] - 74.203 * x[..., 1] + 112.0 * x[..., 2]) / 255
    v = 128 + (112.0 * x[..., 0] - 93.786 * x[..., 1] - 18.214 * x[..., 2]) / 255

    def pool(c):
        return c.reshape(H // 2, 2, W // 2, 2).mean(axis=(1, 3))

    rs = W + row_pad
    ysz, csz = rs * (H - 1) + W, rs * (H // 2 - 1) + W - 1
    buf = np.zeros(ysz + 2 * csz, np.uint8)
    q = lambda c: np.clip(np.rint(c), 0, 255).astype(np.uint8)  # noqa: E731
    for r in range(H):
        buf[r * rs:r * rs + W] = q(y[r])
    uu, vv = q(pool(u)), q(pool(v))
    for r in range(H // 2):
        row = np.stack([uu[r], vv[r]], axis=1).ravel()
        n = min(W, len(buf) - (ysz + r * rs))
        buf[ysz + r * rs:ysz + r * rs + n] = row[:n]
    return [(ysz, rs, 1), (csz, rs, 2), (csz, rs, 2)], buf
