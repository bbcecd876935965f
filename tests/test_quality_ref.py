"""Mesh quality on the CPU: the numpy restatement against the reference's own outputs (golden), the host
side of mqr.evaluation (scores, CSV, input checks).  The golden values come from running the reference's
compute_raw_metrics_for_mesh / compute_quality_scores (tests/golden/make_quality_golden.py)."""
import csv
import os

import numpy as np
import pytest

import quality_ref as qr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "quality_golden.npz")
CASES = ("mixed", "closed", "flat", "alldegenerate", "big")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        g = {k: z[k] for k in z.files}
    for a in g.values():
        a.setflags(write=False)
    assert tuple(g["fields"]) == qr.FIELDS and tuple(g["cases"]) == CASES
    return g


def golden_mesh(g, case):
    return g[case + "_vertices"], g[case + "_triangles"], g.get(case + "_colors")


def golden_raw(g, case):
    return dict(zip(qr.FIELDS, g[case + "_raw"]))


def compare(got, want, scales, label=""):
    """Every field: integers and booleans exact, floats within quality_ref.tolerance."""
    for f in qr.FIELDS:
        a, b = got[f] if isinstance(got, dict) else getattr(got, f), want[f]
        if f in qr.FLOAT_FIELDS and f != "boundary_edge_ratio":
            tol = qr.tolerance(f, scales)
            print(f"{label} {f}: got {float(a)!r} want {float(b)!r} |d| {abs(float(a) - float(b)):.3e} tol {tol:.3e}")
            assert abs(float(a) - float(b)) <= tol, (label, f, a, b, tol)
        else:
            assert float(a) == float(b), (label, f, a, b)


def raw_from_golden(g, case):
    from mqr.evaluation import RawMeshMetrics
    r = golden_raw(g, case)
    kw = {f: (int(r[f]) if f in qr.INT_FIELDS else bool(r[f]) if f in qr.BOOL_FIELDS else float(r[f]))
          for f in qr.FIELDS}
    return RawMeshMetrics(name=case, path=None, **kw)


@pytest.mark.parametrize("case", CASES)
def test_restatement_matches_the_reference(golden, case):
    v, t, c = golden_mesh(golden, case)
    got, scales = qr.raw_metrics(v, t, c)
    compare(got, golden_raw(golden, case), scales, case)


def test_golden_pins_every_branch(golden):
    mixed, closed = golden_raw(golden, "mixed"), golden_raw(golden, "closed")
    flat, alld = golden_raw(golden, "flat"), golden_raw(golden, "alldegenerate")
    assert mixed["degenerate_triangles"] == 3 and mixed["non_manifold_edges"] >= 1 and mixed["component_count"] == 4
    assert mixed["has_color"] and not mixed["is_manifold"]
    assert closed["is_watertight"] and closed["boundary_edge_ratio"] == 0.0 and not closed["has_color"]
    assert closed["uncolored_vertex_ratio"] == 1.0 and closed["color_gradient_stddev"] == 0.0
    assert flat["dihedral_min_deg"] == flat["dihedral_max_deg"] and 1.1e-4 < flat["dihedral_min_deg"] < 1.2e-4
    assert (alld["mean_aspect_ratio"], alld["mean_skewness"], alld["dihedral_min_deg"], alld["dihedral_max_deg"]) == \
        (1.0, 0.0, 180.0, 0.0)
    assert alld["degenerate_triangles"] == 3 and alld["non_manifold_edges"] == 1
    assert golden_raw(golden, "big")["num_triangles"] == 4418


def test_scores_match_the_reference(golden):
    from mqr.evaluation import compute_quality_scores
    scores = compute_quality_scores([raw_from_golden(golden, c) for c in CASES])
    assert [s.name for s in scores] == list(CASES)
    for s, want in zip(scores, golden["scores"]):
        for f, w in zip(golden["score_fields"], want):
            assert abs(getattr(s, str(f)) - w) <= 1e-12, (s.name, f, getattr(s, str(f)), w)


def test_scores_empty_and_constant_batches(golden):
    from mqr.evaluation import compute_quality_scores, min_max_normalize
    assert compute_quality_scores([]) == []
    assert min_max_normalize(np.zeros(0)).shape == (0,)
    m = raw_from_golden(golden, "mixed")
    scores = compute_quality_scores([m, m])
    for s in scores:  # every normalised term is 0.5
        assert s.S_shape == 0.5 and abs(s.S_topology - 0.5) <= 1e-15 and abs(s.S_smooth - 0.5) <= 1e-15
        assert s.S_color == 0.5 and s.Q_norm == 0.5
        assert abs(s.S_complete - (0.5 * (1.0 - m.boundary_edge_ratio) + 0.2 * 0.5)) <= 1e-15
    single = compute_quality_scores([raw_from_golden(golden, "closed")])[0]
    assert single.S_bonuses == 1.0 and single.S_color == 0.5 and single.Q_norm == 0.5


def test_host_arrays_are_checked_before_any_library_call(golden, monkeypatch):
    from mqr import _lib, evaluation

    def no_call(*a, **k):
        raise AssertionError("the library was called")

    monkeypatch.setattr(evaluation, "call", no_call)
    monkeypatch.setattr(_lib, "load", no_call)
    v, t, _ = golden_mesh(golden, "flat")
    with pytest.raises(ValueError):
        evaluation.compute_raw_metrics((np.zeros((0, 3), np.float32), t))
    with pytest.raises(ValueError):
        evaluation.compute_raw_metrics((v, np.zeros((0, 3), np.int32)))
    bad = v.copy()
    bad[7, 1] = np.nan
    with pytest.raises(ValueError):
        evaluation.compute_raw_metrics((bad, t))
    for idx in (len(v), -1):
        tb = t.copy()
        tb[3, 2] = idx
        with pytest.raises(ValueError):
            evaluation.compute_raw_metrics((v, tb))
    with pytest.raises(ValueError):
        evaluation.compute_raw_metrics((v, t, np.zeros((3, 3), np.float32)))


def test_dataclasses_mirror_the_reference_order():
    from dataclasses import fields

    from mqr.evaluation import QualityScores, RawMeshMetrics
    assert tuple(f.name for f in fields(RawMeshMetrics)) == ("name", "path") + qr.FIELDS
    assert tuple(f.name for f in fields(QualityScores)) == (
        "name", "path", "S_shape", "S_topology", "S_bonuses", "S_geom", "S_smooth", "S_complete", "S_color", "Q_raw",
        "Q_norm", "raw")


def test_write_csv_header_order(golden, tmp_path):
    from mqr.evaluation import compute_quality_scores, write_csv
    scores = compute_quality_scores([raw_from_golden(golden, c) for c in CASES])
    out = tmp_path / "sub" / "quality_scores.csv"
    write_csv(scores, out)
    rows = list(csv.reader(out.open()))
    assert rows[0] == ["name", "path", "Q_raw", "Q_norm", "S_geom", "S_smooth", "S_complete", "S_color", "S_shape",
                       "S_topology", "S_bonuses"] + list(qr.FIELDS)
    assert len(rows) == 1 + len(CASES) and rows[1][0] == "mixed"
    assert float(rows[2][2]) == scores[1].Q_raw and rows[2][rows[0].index("is_watertight")] == "True"


def test_c_entry_point_rejects_empty_and_oversized_meshes_before_touching_a_device():
    import ctypes

    from mqr import _lib
    out = (ctypes.c_double * 21)()
    buf = np.zeros(3, np.float32)
    idx = np.zeros(3, np.int32)
    for nv, nt, word in ((0, 1, "no geometry"), (1, 0, "no geometry"), (3, (2 ** 31) // 3 + 1, "too large")):
        with pytest.raises(_lib.MqrError) as e:
            _lib.call("mqr_mesh_quality", 0, _lib.ptr(buf), nv, None, _lib.ptr(idx), nt, _lib.MQR_HOST, out)
        assert word in str(e.value)
    assert ctypes.sizeof(__import__("mqr.evaluation", fromlist=["_Metrics"])._Metrics) == 21 * 8
