"""The numpy restatement of the odometry information rules (tests/odometry_ref.py) on its own: the
margins that make exact count comparisons meaningful on the GPU tests' inputs, and the rules' direct
consequences."""
import numpy as np
import pytest

import odometry_ref as ref


@pytest.fixture(scope="module")
def inputs():
    return ref.gpu_test_inputs()


@pytest.mark.parametrize("name", ["even", "odd"])
@pytest.mark.parametrize("which", ["T_true", "T_pert"])
def test_margins_of_the_gpu_inputs(inputs, name, which):
    d = inputs[name]
    info, counts, m = ref.information_pairs(d["depth"], d["K"], d["src"], d["tgt"], d[which], ref.DIST_THRESHOLD,
                                            1.0, ref.DEPTH_MAX)
    print(name, which, "counts", counts.tolist(), "margins", m)
    assert m["round"] >= 1e-7 and m["dist"] >= 1e-7
    # the pairs overlap: every one accepts a substantial part of the image
    assert (counts > 0.2 * d["depth"].shape[1] * d["depth"].shape[2]).all()


def test_margins_of_the_degenerate_cases(inputs):
    frames, src, tgt, T = ref.degenerate_cases(inputs["odd"])
    info, counts, m = ref.information_pairs(frames, inputs["odd"]["K"], src, tgt, T, ref.DIST_THRESHOLD, 1.0,
                                            ref.DEPTH_MAX)
    print("degenerate counts", counts.tolist(), "margins", m)
    assert m["round"] >= 1e-7 and m["dist"] >= 1e-7
    assert not counts[[0, 1, 3, 4, 5, 6]].any() and 0 < counts[2] < counts[11] and counts[10] > 0


def test_shapes_of_the_gpu_inputs(inputs):
    assert inputs["even"]["depth"].shape == (8, 60, 80)
    assert inputs["odd"]["depth"].shape == (8, 61, 83)
    assert (61 * 83) % 64 != 0 and (61 * 83) % 1024 != 0
    assert len(inputs["even"]["src"]) == 10


def test_identity_self_pair_counts_the_valid_pixels(inputs):
    d = inputs["odd"]["depth"][3]
    info, n, _ = ref.information(d, d, inputs["odd"]["K"], np.eye(4), ref.DIST_THRESHOLD, 1.0, ref.DEPTH_MAX)
    assert n == int(((d > 0) & (d <= ref.DEPTH_MAX)).sum()) and n > 1000
    assert np.array_equal(info, info.T)
    assert info[3, 3] == info[4, 4] == info[5, 5] == n


def test_symmetry_and_count_on_a_moved_pair(inputs):
    d = inputs["even"]
    info, n, _ = ref.information(d["depth"][0], d["depth"][2], d["K"], d["T_pert"][7], ref.DIST_THRESHOLD, 1.0,
                                 ref.DEPTH_MAX)
    assert np.array_equal(info, info.T)
    assert info[3, 3] == info[5, 5] == n
    assert np.all(np.linalg.eigvalsh(info) > 0)


def test_hand_computed_2x2():
    K = np.eye(3)
    src = np.array([[1.0, 2.0], [0.0, 1.0]], np.float32)  # pixel (x=0, y=1) invalid
    # g = (0, 0, 1), (2, 0, 2), (1, 1, 1)
    want = np.array([[7, -1, -5, 0, -4, 1],
                     [-1, 11, -1, 4, 0, -3],
                     [-5, -1, 6, -1, 3, 0],
                     [0, 4, -1, 3, 0, 0],
                     [-4, 0, 3, 0, 3, 0],
                     [1, -3, 0, 0, 0, 3]], np.float64)
    info, n, _ = ref.information(src, src, K, np.eye(4), 0.07)
    assert n == 3 and np.array_equal(info, want)
    # the target 0.5 m off at (1, 1): that pixel is rejected by the distance test
    tgt = src.copy()
    tgt[1, 1] = 1.5
    info2, n2, m = ref.information(src, tgt, K, np.eye(4), 0.07)
    g3 = np.array([[0, 1, -1, 1, 0, 0], [-1, 0, 1, 0, 1, 0], [1, -1, 0, 0, 0, 1]], np.float64)
    assert n2 == 2 and np.array_equal(info2, want - g3.T @ g3)
    # depths above depth_max, NaN and a point behind the camera count for nothing
    bad = np.array([[np.nan, 5.0], [0.0, -1.0]], np.float32)
    info3, n3, _ = ref.information(bad, src, K, np.eye(4), 0.07)
    assert n3 == 0 and not info3.any()
    back = np.eye(4)
    back[2, 3] = -10.0
    assert ref.information(src, src, K, back, 0.07)[1] == 0
