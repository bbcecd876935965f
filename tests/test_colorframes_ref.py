"""mqr.colorframes on the CPU: the host path and resolve_layout against the reference's recorded I420 bytes
and errors (tests/golden/colorframes_golden.npz), the restatement (tests/colorframes_ref.py) against its
hand-computed answers, the host path against the restatement, the exposure verdicts against the reference's,
and blur_score against the exact rational and against np.var of the restated Laplacian."""
import os
from fractions import Fraction
from types import SimpleNamespace

import numpy as np
import pytest

import colorframes_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "colorframes_golden.npz")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def fmt(width, height, planes):
    from mqr.models import BaseTime, ImageFormatInfo, ImagePlaneInfo
    return ImageFormatInfo(width=int(width), height=int(height), format="YUV_420_888",
                           planes=[ImagePlaneInfo(*(int(x) for x in p)) for p in planes], base_time=BaseTime(0, 0))


def case(golden, name):
    w, h = golden[f"i420_{name}_size"]
    return (golden[f"i420_{name}_raw"], int(w), int(h), [tuple(int(x) for x in p) for p in golden[f"i420_{name}_planes"]],
            str(golden[f"i420_{name}_order"]))


def test_known_answers_of_the_restatement():
    for (Y, U, V), want in ref.KNOWN.items():
        got = ref.yuv_to_rgb(np.full((2, 2), Y, np.uint8), np.full((1, 1), U, np.uint8), np.full((1, 1), V, np.uint8))
        assert [tuple(p) for p in got.reshape(-1, 3)] == [want] * 4, (Y, U, V)
    assert ref.grey_of(np.array([[[255, 255, 255]]], np.uint8))[0, 0] == 255
    assert ref.grey_of(np.array([[[255, 0, 0]]], np.uint8))[0, 0] == (9798 * 255 + 16384) >> 15 == 76
    board = (np.indices((6, 8)).sum(0) % 2 * 255).astype(np.int64)
    lap = ref.laplacian(board)
    assert np.array_equal(lap, np.where(board == 0, 1020, -1020))  # reflect-101 keeps the parity at the border
    ramp = np.arange(5)[None, :] * np.ones((4, 1), np.int64)
    assert np.array_equal(ref.laplacian(ramp), np.array([[2, 0, 0, 0, -2]] * 4))


def test_constants_have_one_home():
    from mqr import colorframes as cf
    c = cf.color_constants()
    assert (c["CY"], c["CUB"], c["CUG"], c["CVG"], c["CVR"], c["SHIFT"]) == (ref.CY, ref.CUB, ref.CUG, ref.CVG, ref.CVR, 20)
    assert (c["GREY_B"], c["GREY_G"], c["GREY_R"], c["GREY_SHIFT"]) == (3735, 19235, 9798, 15)


def test_i420_matches_the_reference(golden):
    from mqr import colorframes as cf
    assert len(golden["i420_cases"]) == 6
    for name in golden["i420_cases"]:
        raw, w, h, planes, order = case(golden, name)
        got = cf.convert_yuv420_888_to_i420(raw, fmt(w, h, planes), order)
        assert got.dtype == np.uint8 and np.array_equal(got, golden[f"i420_{name}_out"]), name
        # bytes objects too, as np.frombuffer takes them
        assert np.array_equal(cf.convert_yuv420_888_to_i420(raw.tobytes(), fmt(w, h, planes), order), got)
        # the restatement's unpacking agrees
        y, u, v = ref.unpack(raw, ref.layout_of(w, h, planes, order))
        assert np.array_equal(np.concatenate([y.ravel(), u.ravel(), v.ravel()]), got), name


def test_layout_quirks(golden):
    from mqr import colorframes as cf
    raw, w, h, planes, _ = case(golden, "nv12short")
    lay = cf.resolve_layout(fmt(w, h, planes), "NV12", len(raw))
    assert (lay.y_base, lay.y_row_stride, lay.y_pixel_stride) == (0, 16, 1)
    assert (lay.u_base, lay.u_row_stride, lay.u_step) == (56, 16, 2) and (lay.v_base, lay.v_step) == (57, 2)
    assert lay.valid_bytes == 102 == cf.resolve_layout(fmt(w, h, planes)).valid_bytes
    swapped = cf.resolve_layout(fmt(w, h, planes), "NV21", len(raw))
    assert (swapped.u_base, swapped.v_base) == (57, 56)
    _, w, h, planes, _ = case(golden, "chroma4")  # the step stays 2 whatever the pixel stride says
    lay = cf.resolve_layout(fmt(w, h, planes), "NV12", 128)
    assert (lay.u_base, lay.u_step, lay.v_base, lay.v_step) == (64, 2, 65, 2)
    _, w, h, planes, _ = case(golden, "planar")  # V after the U buffer, at its own row stride; the order is ignored
    for order in ("NV12", "NV21"):
        lay = cf.resolve_layout(fmt(w, h, planes), order, 104)
        assert (lay.u_base, lay.u_row_stride, lay.u_step, lay.v_base, lay.v_row_stride, lay.v_step) == (64, 8, 1, 80, 12, 1)
    _, w, h, planes, _ = case(golden, "ystride2")
    assert cf.resolve_layout(fmt(w, h, planes), "NV12", 110).y_pixel_stride == 2


def test_errors_follow_the_reference(golden):
    from mqr import colorframes as cf
    assert list(golden["i420_errors"]) == ["nv12short_one_byte_short", "odd_width_bgr"]
    assert list(golden["i420_error_raised"]) == ["ValueError", "ValueError"]
    raw, w, h, planes, order = case(golden, "nv12short")
    f = fmt(w, h, planes)
    cf.convert_yuv420_888_to_i420(raw[:56 + 16 + 8], f, order)  # the last byte any row needs is there
    for call in (cf.convert_yuv420_888_to_i420, cf.convert_yuv420_888_to_bgr):
        with pytest.raises(ValueError):
            call(raw[:56 + 16 + 7], f, order)
    with pytest.raises(ValueError):
        cf.resolve_layout(f, order, 56 + 16 + 7)
    with pytest.raises(ValueError):
        cf.decode_color_frames([raw[:56 + 16 + 7]], f, device=None)
    with pytest.raises(ValueError):  # Y rows short
        cf.convert_yuv420_888_to_i420(raw[:55], f, order)
    for ww, hh in ((7, 4), (8, 3)):
        with pytest.raises(ValueError):
            cf.convert_yuv420_888_to_bgr(raw, fmt(ww, hh, planes))
        with pytest.raises(ValueError):
            cf.resolve_layout(fmt(ww, hh, planes), "NV12", len(raw))
    for n in (2, 4):
        with pytest.raises(ValueError, match="Expected 3 planes"):
            cf.convert_yuv420_888_to_i420(raw, fmt(w, h, (planes * 2)[:n]))
        with pytest.raises(ValueError, match="Expected 3 planes"):
            cf.resolve_layout(fmt(w, h, (planes * 2)[:n]))
    with pytest.raises(ValueError):  # a chroma pixel stride of 0 leaves the reference an empty row slice
        cf.convert_yuv420_888_to_i420(raw, fmt(w, h, [planes[0], (23, 16, 0), planes[2]]))


def test_host_path_matches_the_restatement(golden):
    from mqr import colorframes as cf
    for name in golden["i420_cases"]:
        raw, w, h, planes, order = case(golden, name)
        want = ref.decode(raw, w, h, planes, order, "bgr")
        got = cf.convert_yuv420_888_to_bgr(raw, fmt(w, h, planes), order)
        assert got.shape == (h, w, 3) and got.dtype == np.uint8 and np.array_equal(got, want), name
        rgb, hist, sums = cf.decode_color_frames([raw, raw], fmt(w, h, planes), order, order="rgb", stats=True, device=None)
        assert rgb.shape == (2, h, w, 3) and np.array_equal(rgb[1], want[..., ::-1])
        rh, rs = ref.statistics(rgb[0])
        assert hist.dtype == np.uint32 and sums.dtype == np.int64
        assert np.array_equal(hist, [rh, rh]) and np.array_equal(sums, [rs, rs]), name
    # both clamps on every channel: every (Y, U, V) corner and the known answers
    Y = np.array([[0, 15, 16, 17], [234, 235, 236, 255]], np.uint8)
    for U in (0, 1, 127, 128, 129, 254, 255):
        for V in (0, 1, 127, 128, 129, 254, 255):
            raw = np.concatenate([Y.ravel(), [U, V, U, V]]).astype(np.uint8)
            planes = [(8, 4, 1), (3, 4, 2), (3, 4, 2)]
            got = cf.convert_yuv420_888_to_bgr(raw, fmt(4, 2, planes))
            assert np.array_equal(got, ref.decode(raw, 4, 2, planes, order="bgr")), (U, V)
    for (y, u, v), want in ref.KNOWN.items():
        raw = np.array([y, y, y, y, u, v], np.uint8)
        got = cf.convert_yuv420_888_to_bgr(raw, fmt(2, 2, [(4, 2, 1), (1, 2, 2), (1, 2, 2)]))
        assert [tuple(p) for p in got.reshape(-1, 3)] == [want[::-1]] * 4


def test_exposure_verdicts_match_the_reference(golden):
    from mqr import colorframes as cf
    assert len(golden["exposure_verdicts"]) == 12 and golden["exposure_verdicts"].any() and not golden["exposure_verdicts"].all()
    for img, (low, high, grey), want in zip(golden["exposure_images"], golden["exposure_args"], golden["exposure_verdicts"]):
        given = img[..., 0] if grey else img
        assert cf.is_over_or_under_exposed(given, low_thresh=low, high_thresh=high) == bool(want)
        # from the integer histogram, as the device hands it over (blue = channel 0 of the BGR image)
        hist = cf.frame_statistics(img, "bgr")[0][0]
        assert hist.sum() == img.shape[0] * img.shape[1]
        assert cf.is_over_or_under_exposed(None, low_thresh=low, high_thresh=high, hist=hist) == bool(want)
        assert np.array_equal(cf.frame_statistics(img[..., ::-1], "rgb")[0][0], hist)


def test_blur_score_is_the_rounded_exact_variance():
    from mqr import colorframes as cf
    rng = np.random.default_rng(5)
    for shape, scale in (((6, 8), 256), ((34, 130), 256), ((34, 130), 8), ((240, 320), 256)):
        rgb = rng.integers(0, scale, shape + (3,), dtype=np.uint8)
        lap = ref.laplacian(ref.grey_of(rgb))
        n = lap.size
        s1, s2 = int(lap.sum()), int((lap * lap).sum())
        hist, sums = cf.frame_statistics(rgb, "rgb")
        assert (int(sums[0, 0]), int(sums[0, 1])) == (s1, s2)
        score = cf.blur_score(sums[0], n)
        exact = Fraction(n * s2 - s1 * s1, n * n)
        assert isinstance(score, float) and score == exact.numerator / exact.denominator
        assert abs(Fraction(score) - exact) <= Fraction(np.spacing(score)) / 2  # correctly rounded
        # np.var: two passes in float64 with pairwise sums, no cancellation -- a few dozen ulp at these sizes
        assert abs(score - np.var(lap.astype(np.float64))) <= 1e-12 * score
        assert cf.is_blur_image(rgb[..., ::-1], blur_threshold=score) is False
        assert cf.is_blur_image(rgb[..., ::-1], blur_threshold=np.nextafter(score, np.inf)) is True
        assert cf.is_blur_image(shape, blur_threshold=np.nextafter(score, np.inf), sums=sums[0]) is True
    # sums that would cancel in floating point: a large mean, a tiny variance
    n = 1 << 20
    s1 = 1000 * n + 1
    s2 = 1000 * 1000 * n + 2000 + 1
    assert cf.blur_score((s1, s2), n) == (n - 1) / (n * n)
    assert cf.blur_score((0, 0), 4) == 0.0
    with pytest.raises(ValueError):
        cf.blur_score((0, 0), 0)


def test_filter_fn():
    from mqr import colorframes as cf
    from mqr.models import Yuv2RgbConfig
    rng = np.random.default_rng(9)
    sharp = rng.integers(10, 246, (24, 32, 3), dtype=np.uint8)  # nothing near either end
    flat = np.full((24, 32, 3), 128, np.uint8)
    dark = sharp.copy()
    dark[..., 0] = rng.integers(0, 6, (24, 32))  # blue underexposed, the other channels busy
    cfg = Yuv2RgbConfig.parse({"blur_filter": True, "blur_threshold": 50.0, "exposure_filter": True,
                               "exposure_threshold_low": 0.02, "exposure_threshold_high": 0.02, "ignored": 1})
    keep = cf.FilterFn(cfg)
    assert keep(sharp) is True and keep(flat) is False and keep(dark) is False
    assert cf.FilterFn(SimpleNamespace(blur_filter=False, exposure_filter=False))(flat) is True
    only_blur = SimpleNamespace(blur_filter=True, blur_threshold=50.0, exposure_filter=False)
    assert cf.FilterFn(only_blur)(dark) is True
    # the verdict is on channel 0 of the BGR image: the same pixels with the dark channel last pass
    assert keep(np.ascontiguousarray(dark[..., ::-1])) is True
    for img in (sharp, flat, dark):
        hist, sums = cf.frame_statistics(img, "bgr")
        assert keep(img.shape, hist[0], sums[0]) == keep(img)


def test_png_round_trip(tmp_path):
    pytest.importorskip("PIL")
    from mqr import colorframes as cf
    rgb = np.random.default_rng(2).integers(0, 256, (12, 18, 3), dtype=np.uint8)
    cf.write_png(tmp_path / "a.png", rgb)
    assert np.array_equal(cf.read_png(tmp_path / "a.png"), rgb)
    with pytest.raises(FileNotFoundError):
        cf.read_png(tmp_path / "missing.png")
