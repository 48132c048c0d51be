"""bench.py's command line: --dump-outputs (the metric arrays of the last timed step, at most 64 MB, the same inputs from run to
run) and the plain run, which times the steps and prints the line without the --full legs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402
from _util import assert_close, assert_roc  # noqa: E402


def _blocks(m, K, dtype):
    rng = np.random.default_rng(3)
    return [rng.standard_normal((m, K) if i < 8 and K else m).astype(dtype) for i in range(10)]


def test_dump_outputs_writes_every_metric(tmp_path):
    blocks = _blocks(1000, 0, np.float32)
    blocks[2][5] = np.nan
    bench.dump_outputs(str(tmp_path), blocks)
    assert sorted(os.listdir(tmp_path)) == sorted(n + ".npy" for n in bench.DUMP_NAMES)
    for name, b in zip(bench.DUMP_NAMES, blocks):
        got = np.load(os.path.join(tmp_path, name + ".npy"))
        assert got.dtype == np.float32 and got.shape == b.shape
        assert (got.view(np.uint32) == b.view(np.uint32)).all(), name


def test_dump_outputs_samples_a_fixed_set_of_users_beyond_the_limit(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 200_000)
    blocks = _blocks(3000, 5, np.float64)                    # cumulative layout: eight [m, K] blocks, two [m]
    total = 0
    for sub in ("a", "b"):
        bench.dump_outputs(str(tmp_path / sub), blocks)
    users = np.load(tmp_path / "a" / "sampled_users.npy")
    assert users.dtype == np.float64 and (np.diff(users) > 0).all() and 0 < users.shape[0] < 3000
    assert (np.load(tmp_path / "b" / "sampled_users.npy") == users).all()
    idx = users.astype(np.int64)
    for name, b in zip(bench.DUMP_NAMES, blocks):
        got = np.load(tmp_path / "a" / (name + ".npy"))
        assert got.dtype == np.float64 and (got == b[idx]).all(), name
        total += got.nbytes
    assert total + users.nbytes <= 200_000


def test_the_benchmark_inputs_are_the_same_from_run_to_run():
    from recometrics_amd.synth import CONFIGS
    m, n, k, dtype, K, mean_c, seed = CONFIGS["C1"]
    a, b = (bench.host_problem(m, n, k, mean_c, seed, dtype) for _ in range(2))
    assert (a["A"] == b["A"]).all() and (a["B"] == b["B"]).all()
    for x, y in zip(a["train"] + a["test"], b["train"] + b["test"]):
        assert x.dtype == y.dtype and (x == y).all()


@pytest.mark.gpu
def test_plain_run_dumps_what_the_timed_steps_computed(tmp_path):
    """A plain run: the headline line with --steps timed steps and nothing of --full; its dump holds the metric block of the
    workload it timed, within 1e-5 of the oracle on the same inputs (ROC-AUC: within a float ulp, _util.roc_tol)"""
    from oracle.oracle import NAMES, Oracle
    from recometrics_amd.synth import CONFIGS
    out = tmp_path / "dump"
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "C1", "--steps", "3", "--warmup", "1",
                          "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    line = json.loads(lines[0])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in line, key
    assert line["steps"] == 3 and line["dtype"] == "f32" and line["unit"] == "users/s"
    assert abs(line["value"] - 1000 * 3 / (line["ms_per_step"] * 3e-3)) < 1e-6 * line["value"]
    for key in ("parity", "e2e_host", "noise_on", "north_star_shape", "tutorial", "no_auc", "other_configs"):
        assert key not in line, key
    assert line["cpu_baseline"] is None
    m, n, k, dtype, K, mean_c, seed = CONFIGS["C1"]
    host = bench.host_problem(m, n, k, mean_c, seed, dtype)
    want = Oracle().calc(host["A"], host["B"], host["train"], host["test"], K, nthreads=4)
    for short, name in zip(("p", "tp", "r", "ap", "tap", "ndcg", "hit", "rr", "roc", "pr"), bench.DUMP_NAMES):
        got = np.load(out / (name + ".npy"))
        w = want[NAMES[short]]
        assert got.dtype == np.float32, name
        if short == "roc":
            assert_roc(got, w, np.float32, name)
        else:
            assert_close(got, w, 1e-5, name)
