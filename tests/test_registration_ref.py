"""The CPU restatement of the registration rules (tests/registration_ref.py) is a usable yardstick:
it recovers a known motion, its result does not depend on summation order, and on the test pair no
correspondence decision sits within float64 rounding of a tie or of the radius -- the condition that
makes an exact comparison with the device (tests/test_gpu_registration.py) meaningful.  Plus the
declarations the feature adds to the C header and the fragment configuration.  No GPU needed."""
import dataclasses
import os
import re

import numpy as np
import pytest

import registration_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LEVELS = dict(voxel_sizes=[0.05, 0.025, 0.0125], max_dists=[0.1, 0.05, 0.025], max_iters=[50, 31, 14],
              rel_fitness=[1e-6] * 3, rel_rmse=[1e-6] * 3)


@pytest.fixture(scope="module")
def icp_result():
    src, tgt, T_true = ref.icp_pair()
    return ref.icp(src, tgt, **LEVELS), T_true, src, tgt


def test_reference_icp_recovers_the_motion(icp_result):
    r, T_true, _, _ = icp_result
    err = float(np.abs(r["transformation"] - T_true).max())
    print("max |T - T_true| =", err, "iterations", r["num_iterations"], "fitness", r["fitness"])
    assert err < 5e-3
    assert r["fitness"] > 0.5 and 0 < r["inlier_rmse"] < 0.025


def test_reference_icp_does_not_depend_on_summation_order(icp_result):
    r, _, src, tgt = icp_result
    p = ref.icp(src, tgt, permute_seed=7, **LEVELS)
    diff = float(np.abs(p["transformation"] - r["transformation"]).max())
    print("max |T_permuted - T| =", diff)
    assert p["counts"] == r["counts"] and p["num_iterations"] == r["num_iterations"]
    assert diff < 1e-12


def test_reference_margins_allow_an_exact_comparison(icp_result):
    r, _, src, tgt = icp_result
    m = r["margins"]
    # the other passes the GPU tests compare: evaluate at identity / the true motion, full and every 30th
    # point, and the information matrix at the ICP result
    for T in (np.eye(4), ref.TRUE_MOTION):
        for k in (1, 30):
            ref.evaluate(src, tgt, 0.1, T, k, m)
    ref.information(src, tgt, 0.025, r["transformation"], m)
    print("tie margin", m.tie, "radius margin", m.radius)
    assert m.tie > 1e-9 and m.radius > 1e-9


def test_voxel_down_rule_on_a_hand_case():
    p = np.array([[0.01, 0.01, 0.01], [-0.01, 0.01, 0.01], [0.04, 0.03, 0.02], [0.05, 0.0, 0.0],
                  [-0.05, 0.0, 0.0], [-0.050001, 0.0, 0.0]], np.float32)
    out = ref.voxel_down(p, 0.05)
    # float32(0.05) lies just above 0.05 and float32(-0.05) just below -0.05, so their keys are 1 and -2:
    # (-2,0,0) [rows 4, 5], (-1,0,0) [row 1], (0,0,0) [rows 0, 2], (1,0,0) [row 3]
    assert out.shape == (4, 3) and out.dtype == np.float32
    exp = np.array([(p[4].astype(np.float64) + p[5]) / 2, p[1].astype(np.float64),
                    (p[0].astype(np.float64) + p[2]) / 2, p[3].astype(np.float64)]).astype(np.float32)
    assert np.array_equal(out, exp)


def test_header_declares_the_registration_calls():
    src = open(os.path.join(ROOT, "include", "mqr.h")).read()
    names = set(re.findall(r"^\s*int\s+(mqr_\w+)\s*\(", src, flags=re.M))
    for must in ("mqr_cloudset_create", "mqr_cloudset_destroy", "mqr_cloudset_voxel_down", "mqr_evaluate_pairs",
                 "mqr_icp_pairs", "mqr_information_pairs"):
        assert must in names, must
    from mqr import _lib
    for must in ("mqr_cloudset_create", "mqr_cloudset_voxel_down", "mqr_evaluate_pairs", "mqr_icp_pairs",
                 "mqr_information_pairs"):
        assert must in _lib.SIGNATURES and must in _lib.ORDERED, must


def test_fragment_config_has_the_reference_registration_fields():
    from mqr.fragments import FragmentPoseRefinementConfig
    from mqr.registration import ICPConvergenceCriteria
    c = FragmentPoseRefinementConfig()
    expect = dict(use_pre_filtering=True, pre_filter_every_k_points=30, pre_filter_max_corr_dist=0.1,
                  pre_filter_inlier_rmse_threshold=0.05, pre_filter_fitness_threshold=0.2,
                  icp_voxel_sizes=[0.05, 0.025, 0.0125], max_corr_dists=[0.1, 0.05, 0.025],
                  max_iterations=[50, 31, 14], relative_fitnesses=[1e-6] * 3, relative_rmses=[1e-6] * 3,
                  icp_fitness_threshold=0.2, icp_inlier_rmse_threshold=0.05, dist_threshold=0.07,
                  edge_prune_threshold=0.25)
    for k, v in expect.items():
        assert getattr(c, k) == v, k
    # appended after the existing fields: positional construction of the old fields still works
    names = [f.name for f in dataclasses.fields(c)]
    assert names[:10] == ["device", "use_confidence_filtered_depth", "confidence_threshold", "valid_count_threshold",
                          "voxel_size", "block_resolution", "block_count", "depth_max", "trunc_voxel_multiplier",
                          "use_multi_threading"]
    assert names[10:] == list(expect)
    crit = c.icp_criteria_list
    assert crit == [ICPConvergenceCriteria(1e-6, 1e-6, 50), ICPConvergenceCriteria(1e-6, 1e-6, 31),
                    ICPConvergenceCriteria(1e-6, 1e-6, 14)]


def test_pair_order_matches_the_reference():
    from mqr.fragments import pose_graph_pairs
    assert pose_graph_pairs([2, 2]) == ref.pair_list([2, 2]) == [
        (0, 1, False), (2, 3, False), (0, 1, True), (0, 2, True), (0, 3, True), (1, 2, True), (1, 3, True),
        (2, 3, True)]
