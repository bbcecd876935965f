"""bench.py's run modes: a plain run keeps only the timed steps (every leg with runs of its own is
behind --full), and --dump-outputs writes the last timed step's volume in key order, within 64 MB,
identically from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (stdlib-only at import time)


def test_plain_run_switches_every_extra_leg_off():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    assert a.no_cpu and a.no_parity and a.no_extras and a.no_c4 and a.no_c5
    assert (a.extract_reps, a.touch_steps, a.weak_steps, a.e2e_frames) == (0, 0, 0, 0)


def test_full_run_keeps_the_legs_and_their_switches():
    a = bench.parse(["--full"])
    assert a.full and not (a.no_cpu or a.no_parity or a.no_extras or a.no_c4 or a.no_c5)
    assert (a.extract_reps, a.touch_steps, a.weak_steps, a.e2e_frames) == (3, 20, 50, 500)
    b = bench.parse(["--full", "--no-c5", "--touch-steps", "4"])
    assert b.no_c5 and not b.no_c4 and b.touch_steps == 4
    c = bench.parse(["--c5-only"])  # a leg of its own: parity as asked
    assert not (c.no_cpu or c.no_parity)


class _Volume:
    def __init__(self, n, R, seed):
        rng = np.random.default_rng(seed)
        self.block_resolution = R
        self.keys = rng.permutation(np.stack(np.meshgrid(np.arange(-3, n // 16 + 1), np.arange(-2, 2), np.arange(4),
                                                         indexing="ij"), -1).reshape(-1, 3))[:n].astype(np.int32)
        self.tsdf = rng.random((n, R, R, R), dtype=np.float32)
        self.wgt = rng.integers(0, 9, (n, R, R, R)).astype(np.float32)

    def export(self):
        return self.keys, self.tsdf, self.wgt


def _load(d):
    return {k: np.load(os.path.join(d, k + ".npy")) for k in ("keys", "tsdf", "weight", "blocks")}


def test_dump_outputs_key_order_and_dtypes(tmp_path):
    v = _Volume(40, 4, 0)
    rec = bench.dump_outputs(str(tmp_path / "o"), v)
    got = _load(rec["dir"])
    order = np.lexsort(v.keys.T[::-1])
    assert rec["blocks"] == rec["blocks_written"] == 40 and got["blocks"].tolist() == [40.0]
    assert got["keys"].dtype == np.float64 and got["tsdf"].dtype == got["weight"].dtype == np.float32
    assert np.array_equal(got["keys"], v.keys[order])
    assert np.array_equal(got["tsdf"], v.tsdf[order]) and np.array_equal(got["weight"], v.wgt[order])
    # the same volume in another buffer order (another run's hash-insert order): the same files
    p = np.random.default_rng(1).permutation(40)
    w = _Volume(40, 4, 0)
    w.keys, w.tsdf, w.wgt = v.keys[p], v.tsdf[p], v.wgt[p]
    again = _load(bench.dump_outputs(str(tmp_path / "p"), w)["dir"])
    assert all(np.array_equal(got[k], again[k]) for k in got)
    # N > 1: only the owned slice
    own = _load(bench.dump_outputs(str(tmp_path / "q"), v, owned=10)["dir"])
    assert np.array_equal(own["keys"], v.keys[:10][np.lexsort(v.keys[:10].T[::-1])]) and own["blocks"][0] == 10


def test_dump_outputs_samples_within_the_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 64 << 10)
    v = _Volume(200, 4, 2)  # 200 blocks of 536 B against a 64 KiB budget
    rec = bench.dump_outputs(str(tmp_path / "a"), v)
    a = _load(rec["dir"])
    assert rec["blocks"] == 200 and a["blocks"][0] == 200 and 0 < rec["blocks_written"] < 200
    assert sum(os.path.getsize(os.path.join(rec["dir"], f)) for f in os.listdir(rec["dir"])) <= 64 << 10
    keys = [tuple(k) for k in a["keys"]]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    full = {tuple(k): (t, w) for k, t, w in zip(v.keys.tolist(), v.tsdf, v.wgt)}
    assert all(np.array_equal(full[tuple(int(x) for x in k)][0], t) and
               np.array_equal(full[tuple(int(x) for x in k)][1], w) for k, t, w in zip(a["keys"], a["tsdf"], a["weight"]))
    b = _load(bench.dump_outputs(str(tmp_path / "b"), v)["dir"])  # the sample is fixed
    assert all(np.array_equal(a[k], b[k]) for k in a)


@pytest.mark.gpu
def test_plain_bench_run_line_and_repeatable_outputs(tmp_path):
    """Two plain runs of a small sequence: the line's headline fields, no extra leg, and the same
    output files bit for bit (same inputs, same volume)."""
    outs = []
    for name in ("a", "b"):
        d = str(tmp_path / name)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup",
                            "1", "--frames", "40", "--height", "120", "--width", "160", "--block-count", "4096",
                            "--dump-outputs", d], capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = r.stdout.strip().splitlines()
        assert len(lines) == 1, r.stdout[-2000:]
        line = json.loads(lines[0])
        assert line["steps"] == 3 and line["warmup"] == 1 and line["unit"] == "frames/s" and line["dtype"] == "f32"
        assert line["higher_is_better"] is True and line["metric"] == bench.METRIC and line["full"] is False
        assert line["ms_per_step"] > 0 and line["value"] == pytest.approx(40 / (line["ms_per_step"] * 1e-3))
        assert line["roofline"]["launches"] == 3  # 40 frames: one batch per timed step, nothing else profiled
        assert all(line[k] is None for k in ("cpu_baseline", "parity", "extract_ms", "confidence", "c3", "c4", "c5",
                                             "dropin_e2e", "host_input_frames_per_s"))
        got = _load(d)
        assert line["outputs"]["blocks"] == got["blocks"][0] == len(got["keys"]) > 0
        assert got["weight"].max() > 0 and got["tsdf"].shape == got["weight"].shape == (len(got["keys"]), 16, 16, 16)
        outs.append(got)
    assert all(np.array_equal(outs[0][k], outs[1][k]) for k in outs[0])
