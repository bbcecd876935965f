"""Batched odometry information matrices (csrc/odometry.hip, mqr.odometry) against the numpy restatement
of their rules (tests/odometry_ref.py): equal counts (the inputs' rounding and distance margins are
asserted on the CPU, tests/test_odometry_ref.py) and matrices within the tolerance of float64 sums
taken in a different order; bit-identical repeats, batches and single pairs; degenerate pairs; bad
arguments."""
import numpy as np
import pytest

import odometry_ref as ref

pytestmark = pytest.mark.gpu

THR, DMAX = ref.DIST_THRESHOLD, ref.DEPTH_MAX


@pytest.fixture(scope="module")
def inputs():
    from mqr import _lib
    _lib.load()
    d = ref.gpu_test_inputs()
    for v in d.values():
        v["depth"].setflags(write=False)
    return d


@pytest.fixture(scope="module")
def reference(inputs):
    """(info, counts) of the numpy restatement per (sequence, pose set), computed once."""
    out = {}
    for name, d in inputs.items():
        for which in ("T_true", "T_pert"):
            out[name, which] = ref.information_pairs(d["depth"], d["K"], d["src"], d["tgt"], d[which], THR, 1.0, DMAX)[:2]
    return out


def _check(info, counts, rinfo, rcounts):
    assert np.array_equal(counts, rcounts), (counts.tolist(), rcounts.tolist())
    for p in range(len(info)):
        scale = np.abs(rinfo[p]).max()
        err = np.abs(info[p] - rinfo[p]).max() / scale if scale > 0 else np.abs(info[p]).max()
        assert err <= 1e-9, (p, err)
        assert np.array_equal(info[p], info[p].T)
        assert info[p][3, 3] == info[p][4, 4] == info[p][5, 5] == counts[p]


@pytest.mark.parametrize("name", ["even", "odd"])
@pytest.mark.parametrize("which", ["T_true", "T_pert"])
def test_matches_the_reference(inputs, reference, name, which):
    from mqr.odometry import odometry_information_pairs
    d = inputs[name]
    info, counts = odometry_information_pairs(d["depth"], d["K"], d["src"], d["tgt"], d[which], THR, 1.0, DMAX)
    assert info.shape == (10, 6, 6) and counts.dtype == np.int64
    _check(info, counts, *reference[name, which])


@pytest.mark.parametrize("name", ["even", "odd"])
def test_batch_single_pair_and_repeat_are_bit_identical(inputs, name):
    from mqr._lib import DeviceBuffer
    from mqr.geometry import DeviceArray, Tensor
    from mqr.odometry import odometry_information_pairs
    d = inputs[name]
    args = (d["K"], d["src"], d["tgt"], d["T_pert"], THR, 1.0, DMAX)
    info, counts = odometry_information_pairs(d["depth"], *args)
    info2, counts2 = odometry_information_pairs(d["depth"], *args)
    assert np.array_equal(info, info2) and np.array_equal(counts, counts2)
    for p in range(10):  # P = 1: each pair alone
        i1, c1 = odometry_information_pairs(d["depth"], d["K"], d["src"][p:p + 1], d["tgt"][p:p + 1],
                                            d["T_pert"][p], THR, 1.0, DMAX)
        assert np.array_equal(i1[0], info[p]) and c1[0] == counts[p]
    # the same frames resident in HBM: as (buffer, N, H, W) and as a device-backed Tensor
    buf = DeviceBuffer.from_array(d["depth"])
    try:
        N, H, W = d["depth"].shape
        i3, c3 = odometry_information_pairs((buf, N, H, W), *args)
        assert np.array_equal(i3, info) and np.array_equal(c3, counts)
        t = Tensor(DeviceArray(buf, buf.ptr.value, (N, H, W), np.float32, 0))
        i4, c4 = odometry_information_pairs(t, *args)
        assert np.array_equal(i4, info) and np.array_equal(c4, counts)
        i5, _ = odometry_information_pairs(t, d["K"], [3], [4], d["T_pert"][3], THR, 1.0, DMAX)
        assert np.array_equal(i5[0], info[3])
    finally:
        buf.free()


def test_degenerate_pairs_give_clean_results(inputs):
    from mqr.odometry import odometry_information_pairs
    d = inputs["odd"]
    base = d["depth"]
    frames, src, tgt, T = ref.degenerate_cases(d)
    info, counts = odometry_information_pairs(frames, d["K"], src, tgt, T, THR, 1.0, DMAX)
    rinfo, rcounts, m = ref.information_pairs(frames, d["K"], src, tgt, T, THR, 1.0, DMAX)
    assert m["round"] >= 1e-7 and m["dist"] >= 1e-7
    assert np.isfinite(info).all()
    _check(info, counts, rinfo, rcounts)
    zero = [0, 1, 3, 4, 5, 6]
    assert not counts[zero].any() and not info[zero].any()
    assert 0 < counts[2] < counts[11] and counts[10] > 0 and 0 < counts[7] and 0 < counts[8]
    assert counts[9] == int(((base[0] > 0) & (base[0] <= DMAX)).sum())  # src == tgt at the identity


def test_bad_arguments(inputs):
    from mqr._lib import MqrError
    from mqr.odometry import odometry_information_pairs
    d = inputs["even"]
    info, counts = odometry_information_pairs(d["depth"], d["K"], [], [], np.zeros((0, 4, 4)), THR)
    assert info.shape == (0, 6, 6) and counts.shape == (0,)
    for src, tgt in (([8], [0]), ([0], [-1])):
        with pytest.raises(MqrError, match="out of range"):
            odometry_information_pairs(d["depth"], d["K"], src, tgt, np.eye(4), THR)
    T = np.eye(4)
    T[1, 3] = np.nan
    with pytest.raises(MqrError, match="non-finite"):
        odometry_information_pairs(d["depth"], d["K"], [0], [1], T, THR)
    K = d["K"].copy()
    K[0, 0] = np.inf
    with pytest.raises(MqrError, match="non-finite"):
        odometry_information_pairs(d["depth"], K, [0], [1], np.eye(4), THR)


def test_n_pairs_zero_touches_nothing_through_the_c_abi():
    from mqr import _lib
    # null buffers and a zero shape: a call that touched anything would fail
    _lib.call("mqr_odometry_information_pairs", 0, None, _lib.MQR_HOST, 0, 0, 0, None, 0, None, None, None, 0.07, 1.0,
              3.0, None, None)


def test_single_pair_form_equals_the_batched_entry(inputs):
    from mqr.geometry import Image
    from mqr.odometry import compute_odometry_information_matrix, odometry_information_pairs
    d = inputs["odd"]
    info, _ = odometry_information_pairs(d["depth"], d["K"], d["src"], d["tgt"], d["T_pert"], THR, 1.0, DMAX)
    for p in (0, 8):
        a, b = d["src"][p], d["tgt"][p]
        one = compute_odometry_information_matrix(Image(d["depth"][a]), Image(d["depth"][b]), d["K"], d["T_pert"][p],
                                                  dist_threshold=THR, depth_scale=1.0, depth_max=DMAX)
        assert one.shape == (6, 6) and one.dtype == np.float64
        assert np.array_equal(one, info[p])
    arr = compute_odometry_information_matrix(d["depth"][0], d["depth"][1], d["K"], d["T_pert"][0], THR, 1.0, DMAX)
    assert np.array_equal(arr, info[0])
