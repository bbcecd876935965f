"""The colour-frame decode on the GPU (csrc/colorframes.hip, mqr.colorframes.decode_color_frames) against the
numpy restatement (tests/colorframes_ref.py): exact equality of every image byte, histogram bin and Laplacian
sum, over the reference's recorded layouts, unaligned packed batches, widths that are no multiple of the
vector width, more than one workgroup, every (U,V) pair with both clamps, single-bin histogram contention, the
extreme Laplacian, host / HBM input and output, both channel orders and null statistics pointers; then the
device-resident images through ColorMapOptimizer and optimize_color_pose through load_rgb_batch."""
import ctypes
import json
import os

import numpy as np
import pytest

import colorframes_ref as ref

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "colorframes_golden.npz")


@pytest.fixture(scope="module")
def golden():
    from mqr import _lib
    _lib.load()
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def fmt(width, height, planes):
    from mqr.models import BaseTime, ImageFormatInfo, ImagePlaneInfo
    return ImageFormatInfo(width=int(width), height=int(height), format="YUV_420_888",
                           planes=[ImagePlaneInfo(*(int(x) for x in p)) for p in planes], base_time=BaseTime(0, 0))


def nv12(W, H, pad, rng=None, extra=0):
    """An NV12 frame with padded rows and Android's short chroma planes: (planes, random bytes)."""
    rs = W + pad
    ysz, csz = rs * (H - 1) + W, rs * (H // 2 - 1) + W - 1
    planes = [(ysz, rs, 1), (csz, rs, 2), (csz, rs, 2)]
    n = ysz + 2 * csz + extra
    return planes, (np.zeros(n, np.uint8) if rng is None else rng.integers(0, 256, n, dtype=np.uint8))


def expect(raws, W, H, planes, uv_order="NV12"):
    rgb = np.stack([ref.decode(r, W, H, planes, uv_order) for r in raws])
    stats = [ref.statistics(im) for im in rgb]
    return rgb, np.stack([s[0] for s in stats]), np.stack([s[1] for s in stats])


def check(raw, W, H, planes, uv_order="NV12", **kw):
    from mqr import colorframes as cf
    frames = raw if isinstance(raw, list) else list(raw)
    rgb, hist, sums = expect(frames, W, H, planes, uv_order)
    got, gh, gs = cf.decode_color_frames(raw, fmt(W, H, planes), uv_order, stats=True, **kw)
    assert got.dtype == np.uint8 and got.shape == rgb.shape and np.array_equal(got, rgb)
    assert gh.dtype == np.uint32 and np.array_equal(gh, hist)
    assert gs.dtype == np.int64 and np.array_equal(gs, sums)
    assert np.array_equal(cf.decode_color_frames(raw, fmt(W, H, planes), uv_order, **kw), rgb)  # statistics pointers null
    return got


def test_every_recorded_layout(golden):
    for name in golden["i420_cases"]:
        raw = golden[f"i420_{name}_raw"]
        w, h = (int(x) for x in golden[f"i420_{name}_size"])
        planes = [tuple(int(x) for x in p) for p in golden[f"i420_{name}_planes"]]
        order = str(golden[f"i420_{name}_order"])
        check([raw], w, h, planes, order)  # one frame, 4-byte aligned base
        check(np.stack([raw, raw[::-1], raw]), w, h, planes, order)  # packed back to back


def test_packed_frames_of_odd_size():
    rng = np.random.default_rng(11)
    for W, H, pad in ((8, 4, 8), (36, 6, 4)):
        planes, _ = nv12(W, H, pad)
        n = nv12(W, H, pad, extra=1)[1].size
        n += (n + 1) % 2  # odd: the bases of frames 1 and 2 are at 1 and 2 mod 4 (or 3 and 2)
        assert n % 2 == 1
        raw = rng.integers(0, 256, (3, n), dtype=np.uint8)
        check(raw, W, H, planes)
        check(list(raw), W, H, planes)  # the same frames repacked at an aligned stride: the wide path


# (1090 x 272: 18 x 17 = 306 statistics tiles, more than the workgroups one frame gets: they stride)
@pytest.mark.parametrize("W,H,pad", [(70, 6, 2), (70, 6, 3), (130, 34, 6), (130, 34, 0), (132, 34, 4), (2, 2, 0),
                                     (1090, 272, 2)])
def test_widths_and_workgroups(W, H, pad):
    rng = np.random.default_rng(W * H + pad)
    planes, _ = nv12(W, H, pad)
    raw = rng.integers(0, 256, (2, nv12(W, H, pad)[1].size), dtype=np.uint8)
    check(raw, W, H, planes)
    check(list(raw), W, H, planes, "NV21")


def test_planar_and_strided_planes():
    rng = np.random.default_rng(3)
    W, H = 132, 10
    # planar, 4-byte aligned rows (wide Y, byte chroma); planar with odd strides; Y pixel stride 2; chroma stride 4
    for planes in ([(144 * H, 144, 1), (72 * H // 2, 72, 1), (80 * H // 2, 80, 1)],
                   [(133 * H, 133, 1), (67 * H // 2, 67, 1), (69 * H // 2, 69, 1)],
                   [(270 * H, 270, 2), (136 * H // 2, 136, 2), (136 * H // 2, 136, 2)],
                   [(136 * H, 136, 1), (264 * H // 2, 264, 4), (264 * H // 2, 264, 4)]):
        raw = rng.integers(0, 256, (2, sum(p[0] for p in planes)), dtype=np.uint8)
        check(raw, W, H, planes)


def test_every_chroma_pair_and_both_clamps():
    """512x512: block (i, j) carries (U, V) = (i, j); its four Y values step through the three sets."""
    from mqr import colorframes as cf
    W = H = 512
    planes, _ = nv12(W, H, 0)
    frames = []
    for ys in ((0, 15, 16, 17), (127, 128, 129, 200), (234, 235, 236, 255)):
        _, buf = nv12(W, H, 0)
        y = np.zeros((H, W), np.uint8)
        y[0::2, 0::2], y[0::2, 1::2], y[1::2, 0::2], y[1::2, 1::2] = ys
        buf[:W * H] = y.ravel()
        uv = np.zeros((H // 2, W), np.uint8)
        uv[:, 0::2] = np.arange(256)[:, None]
        uv[:, 1::2] = np.arange(256)[None, :]
        buf[W * H:W * H + uv.size] = uv.ravel()
        frames.append(buf)
    rgb, hist, sums = expect(frames, W, H, planes)
    for c in range(3):  # both clamps are hit on every channel
        assert rgb[..., c].min() == 0 and rgb[..., c].max() == 255
    pairs = set()
    for f in frames:
        y, u, v = ref.unpack(f, ref.layout_of(W, H, planes))
        pairs |= set(zip(u.ravel().tolist(), v.ravel().tolist()))
    assert len(pairs) == 65536
    got, gh, gs = cf.decode_color_frames(frames, fmt(W, H, planes), stats=True)
    assert np.array_equal(got, rgb) and np.array_equal(gh, hist) and np.array_equal(gs, sums)
    bgr = cf.decode_color_frames(frames, fmt(W, H, planes), order="bgr")
    assert np.array_equal(bgr, rgb[..., ::-1])


def test_constant_frame_and_checkerboard():
    from mqr import colorframes as cf
    W, H = 130, 34
    planes, const = nv12(W, H, 6)
    const[:] = 128  # grey 130: one histogram bin takes every pixel, the Laplacian is zero
    _, board = nv12(W, H, 6)
    board[:] = 128
    rs = planes[0][1]
    yy = (np.indices((H, rs)).sum(0) % 2 * 255).astype(np.uint8)
    board[:planes[0][0]] = yy.ravel()[:planes[0][0]]
    got, hist, sums = cf.decode_color_frames([const, board], fmt(W, H, planes), stats=True)
    rgb, rh, rsums = expect([const, board], W, H, planes)
    assert np.array_equal(got, rgb) and np.array_equal(hist, rh) and np.array_equal(sums, rsums)
    assert hist[0].max() == W * H and (hist[0] > 0).sum() == 1 and tuple(sums[0]) == (0, 0)
    assert hist[1][0] == hist[1][255] == W * H // 2
    assert tuple(sums[1]) == (0, W * H * 1020 * 1020)  # every pixel at the extreme +-1020
    assert cf.blur_score(sums[1], W * H) == 1020.0 ** 2 and cf.blur_score(sums[0], W * H) == 0.0


def test_device_input_output_and_orders():
    from mqr import colorframes as cf
    from mqr._lib import DeviceBuffer
    rng = np.random.default_rng(17)
    W, H = 68, 10
    planes, _ = nv12(W, H, 4)
    for extra in (0, 1):  # an aligned and an unaligned frame stride
        raw = rng.integers(0, 256, (3, nv12(W, H, 4, extra=extra)[1].size), dtype=np.uint8)
        rgb, hist, sums = expect(list(raw), W, H, planes)
        src = DeviceBuffer.from_array(raw)
        dst = DeviceBuffer(rgb.nbytes)
        for order, want in (("rgb", rgb), ("bgr", rgb[..., ::-1])):
            out = cf.decode_color_frames((src.ptr, 3, raw.shape[1]), fmt(W, H, planes), order=order, stats=True)
            assert np.array_equal(out[0], want) and np.array_equal(out[1], hist) and np.array_equal(out[2], sums)
            none, gh, gs = cf.decode_color_frames(raw, fmt(W, H, planes), order=order, stats=True, out_ptr=dst)
            assert none is None and np.array_equal(dst.to_array(rgb.shape, np.uint8), want)
            assert np.array_equal(gh, hist) and np.array_equal(gs, sums)  # blue is blue in either order
            assert cf.decode_color_frames((src, 3, raw.shape[1]), fmt(W, H, planes), order=order, out_ptr=dst.ptr) is None
            assert np.array_equal(dst.to_array(rgb.shape, np.uint8), want)
        src.free()
        dst.free()
    assert cf.decode_color_frames([], fmt(W, H, planes)).shape == (0, H, W, 3)


def test_each_statistic_alone_and_host_side_checks():
    """The C entry point with one statistics pointer null at a time, and its bounds check, which runs on
    the host before anything is launched."""
    from mqr import _lib
    from mqr import colorframes as cf
    rng = np.random.default_rng(23)
    W, H = 36, 6
    planes, _ = nv12(W, H, 4)
    raw = rng.integers(0, 256, (2, nv12(W, H, 4)[1].size), dtype=np.uint8)
    rgb, hist, sums = expect(list(raw), W, H, planes)
    lay = cf.resolve_layout(fmt(W, H, planes), "NV12", raw.shape[1])

    def call(layout, gh, gs, n_frames=2, w=W, h=H):
        c = cf._CLayout(*(getattr(layout, f) for f, _ in cf._CLayout._fields_))
        out = np.zeros((n_frames, h, w, 3), np.uint8)
        _lib.call("mqr_decode_color_frames", 0, _lib.ptr(raw), _lib.MQR_HOST, n_frames, raw.shape[1], w, h,
                  ctypes.c_void_p(ctypes.addressof(c)), 0, _lib.ptr(out), _lib.MQR_HOST,
                  None if gh is None else _lib.ptr(gh), None if gs is None else _lib.ptr(gs))
        return out

    gh, gs = np.zeros((2, 256), np.uint32), np.zeros((2, 2), np.int64)
    assert np.array_equal(call(lay, gh, None), rgb) and np.array_equal(gh, hist)
    assert np.array_equal(call(lay, None, gs), rgb) and np.array_equal(gs, sums)
    import dataclasses
    for bad in (dataclasses.replace(lay, valid_bytes=lay.v_base + 2 * lay.v_row_stride + 2 * (W // 2 - 1)),  # one short
                dataclasses.replace(lay, y_row_stride=lay.y_row_stride + 100), dataclasses.replace(lay, u_base=-1),
                dataclasses.replace(lay, u_step=40), dataclasses.replace(lay, valid_bytes=raw.shape[1] + 1)):
        with pytest.raises(_lib.MqrError):
            call(bad, None, None)
    with pytest.raises(_lib.MqrError):
        call(lay, None, None, w=W + 1)
    with pytest.raises(ValueError):
        cf.decode_color_frames(raw[:, :lay.v_base + 2 * lay.v_row_stride + W - 2], fmt(W, H, planes))  # the last V is missing


# ---------------------------------------------------------------- device-resident images downstream
def test_colormap_optimizer_takes_device_images():
    from mqr._lib import DeviceBuffer
    from mqr.color import ColorMapOptimizer, RigidOptimizerOption, color_map
    from mqr.geometry import DeviceArray, Tensor
    rng = np.random.default_rng(31)
    W, H, N = 16, 12, 2
    gx, gy = np.meshgrid(np.linspace(-0.5, 0.5, 24), np.linspace(-0.4, 0.4, 20))
    V = np.stack([gx.ravel(), gy.ravel(), np.ones(gx.size)], axis=1).astype(np.float32)  # a plane 1 m ahead
    K = np.tile(np.array([[12.0, 0, 7.5], [0, 12.0, 5.5], [0, 0, 1]]), (N, 1, 1))
    T = np.tile(np.eye(4), (N, 1, 1))
    T[1, 0, 3] = 0.02
    t_hit = np.ones((N, H, W), np.float32)
    images = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    option = RigidOptimizerOption(maximum_iteration=2, image_boundary_margin=1)
    buf = DeviceBuffer.from_array(images)
    dev = Tensor(DeviceArray(buf, buf.ptr.value, images.shape, np.uint8, 0))
    tb = DeviceBuffer.from_array(t_hit)
    dev_t = Tensor(DeviceArray(tb, tb.ptr.value, t_hit.shape, np.float32, 0))
    results = []
    for im, th in ((images, t_hit), (dev, t_hit), (dev, dev_t), (images, dev_t)):
        with ColorMapOptimizer(V, im, th, K, T, option) as o:
            pairs = o.pairs_per_keyframe
            res, _ = o.optimize(2)
            colors, counts = o.colors()
            results.append((pairs, res, colors, counts, o.poses))
    assert results[0][0].min() > 20 and (results[0][3] > 0).sum() > 20 and results[0][2].std() > 0.05
    for other in results[1:]:
        for a, b in zip(results[0], other):
            assert np.array_equal(a, b)
    host = color_map(V, images, t_hit, K, T, margin=1)
    for im, th in ((dev, t_hit), (dev, dev_t)):
        got = color_map(V, im, th, K, T, margin=1)
        assert np.array_equal(got[0], host[0]) and np.array_equal(got[1], host[1])
    with pytest.raises(ValueError):
        ColorMapOptimizer(V, Tensor(DeviceArray(buf, buf.ptr.value, (N, H, W * 3), np.uint8, 0)), t_hit, K, T)


class _Config:
    weight_threshold = 1.5
    estimated_vertex_number = -1
    min_triangle_count = 200
    device = "HIP:0"
    use_dataset_cache = False
    interval = 2
    max_iteration = 2


class _LoadRgbOnly:
    """What optimize_color_pose had before load_rgb_batch: a colour IO with load_color_dataset and load_rgb."""

    def __init__(self, io):
        self._io = io

    def load_color_dataset(self, side, use_cache):
        return self._io.load_color_dataset(side=side, use_cache=use_cache)

    def load_rgb(self, side, timestamp):
        return self._io.load_rgb(side=side, timestamp=timestamp)


class _Holder:
    def __init__(self, color):
        self.color = color


def test_optimize_color_pose_through_load_rgb_batch(tmp_path):
    """Raw frames only, no PNGs: load_rgb_batch decodes each side's keyframes on the device, load_rgb one
    at a time on the host; the coloured mesh and the poses are the same."""
    from mqr import synthetic
    from mqr.color_map_optimization import optimize_color_pose
    from mqr.dataio import ImageDataIO
    from mqr.models import CameraDataset, Side
    from mqr.vbg import VoxelBlockGrid
    H, W, n = 128, 160, 8
    poses = synthetic.room_loop_poses(96)[:n]
    datasets, seqs = {}, {}
    for side, off in ((Side.LEFT, None), (Side.RIGHT, 0.06)):
        seq = synthetic.make_sequence("room", n=n, height=H, width=W, f=110.0, noise=False, poses=poses, side_offset=off)
        K = seq["K"].astype(np.float64)
        ts = 1000 + 33 * np.arange(n)
        shifted = poses if off is None else [(R, t + R[:, 0] * off) for R, t in poses]
        d = tmp_path / f"{side.value}_camera_raw"
        d.mkdir()
        for i, (R, t) in enumerate(shifted):
            planes, buf = ref.to_yuv_file(synthetic.render_color("room", K[i], R, t, H, W), row_pad=8)
            buf.tofile(d / f"{ts[i]}.yuv")
        (tmp_path / f"{side.value}_camera_image_format.json").write_text(json.dumps({
            "width": W, "height": H, "format": "YUV_420_888",
            "planes": [{"bufferSize": b, "rowStride": r, "pixelStride": p} for b, r, p in planes],
            "baseTime": {"baseMonoTimeNs": 0, "baseUnixTimeMs": 0}}))
        datasets[side] = CameraDataset(
            directory_relative_path=f"{side.value}_camera_raw", image_file_names=np.array([f"{t}.yuv" for t in ts]),
            timestamps=ts, fx=K[:, 0, 0].copy(), fy=K[:, 1, 1].copy(), cx=W - K[:, 0, 2], cy=K[:, 1, 2].copy(),
            transforms=seq["unity"], widths=np.full(n, W), heights=np.full(n, H))
        seqs[side] = seq

    class IO(ImageDataIO):
        batches = 0

        def load_color_dataset(self, side, use_cache=True):
            return datasets[side]

        def load_rgb_batch(self, side, timestamps, device=None):
            IO.batches += 1
            return super().load_rgb_batch(side, timestamps, device=device)

    io = IO(tmp_path)
    left = io.load_rgb_batch(Side.LEFT, datasets[Side.LEFT].timestamps[:3])
    assert left.shape == (3, H, W, 3) and left.std() > 10
    for i in range(3):  # device decode == host decode, frame by frame
        assert np.array_equal(left[i], io.load_rgb(Side.LEFT, int(datasets[Side.LEFT].timestamps[i])))
    IO.batches = 0
    seq = seqs[Side.LEFT]
    vbg = VoxelBlockGrid(voxel_size=0.02, block_resolution=16, block_count=64)
    vbg.integrate_frames(seq["depth"], seq["K"], seq["T_wc"], depth_scale=1.0, depth_max=4.0, trunc_voxel_multiplier=6.0)
    mesh_a, out_a = optimize_color_pose(vbg, _Holder(io), _Config)
    assert IO.batches == 2  # once per side
    mesh_b, out_b = optimize_color_pose(vbg, _Holder(_LoadRgbOnly(io)), _Config)
    assert IO.batches == 2
    ca, cb = mesh_a.vertex.colors.numpy(), mesh_b.vertex.colors.numpy()
    assert len(ca) > 1000 and ca.std() > 0.05 and np.array_equal(ca, cb)
    assert np.array_equal(mesh_a.vertices, mesh_b.vertices)
    for side in (Side.LEFT, Side.RIGHT):
        assert len(out_a[side]) == n // 2
        assert np.array_equal(out_a[side].transforms.positions, out_b[side].transforms.positions)
        assert np.array_equal(out_a[side].transforms.rotations, out_b[side].transforms.rotations)
