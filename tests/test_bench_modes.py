"""bench.py's two modes.  A plain run times exactly the K steps asked for and prints the contract's line; --dump-outputs DIR
writes what the last timed step left in the solver state (float64 .npy, seeded samples of long vectors, 64 MB at most);
--full (off by default) adds every other measurement.  The CPU tests cover the options and the dump; the GPU test runs
the plain command on a small LP and checks the dump against the same steps taken in this process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("primal", "dual", "dual_product", "primal_average", "dual_average")


def _parse(argv, monkeypatch):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    return bench.parse()


def test_full_is_off_and_nothing_is_dumped_by_default(monkeypatch):
    args = _parse(["--gpus", "1", "--steps", "5", "--warmup", "2"], monkeypatch)
    assert args.full is False and args.dump_outputs is None and args.steps == 5 and args.warmup == 2
    args = _parse(["--full", "--dump-outputs", "out"], monkeypatch)
    assert args.full is True and args.dump_outputs == "out"


def test_zero_steps_is_refused():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, timeout=120)
    assert r.returncode != 0 and b"--steps" in r.stderr


def test_sample_index_is_fixed_sorted_and_bounded():
    import bench
    assert np.array_equal(bench.sample_index(10), np.arange(10))
    assert np.array_equal(bench.sample_index(bench.DUMP_SAMPLE), np.arange(bench.DUMP_SAMPLE))
    n = 3 * bench.DUMP_SAMPLE + 17
    a, b = bench.sample_index(n), bench.sample_index(n)
    assert np.array_equal(a, b) and len(a) == bench.DUMP_SAMPLE
    assert a[0] >= 0 and a[-1] < n and np.all(np.diff(a) > 0)
    # five float64 vectors and the scalars stay within the 64 MB the dump may take
    assert 5 * 8 * bench.DUMP_SAMPLE + 8 * 5 <= 64_000_000


class _FakeEngine:
    def __init__(self, n, m):
        rng = np.random.default_rng(3)
        self.x, self.y, self.aty = rng.standard_normal(n), rng.standard_normal(m), rng.standard_normal(n)
        self.xa, self.ya = rng.standard_normal(n), rng.standard_normal(m)

    def get_current(self):
        return self.x.copy(), self.y.copy()

    def get_dual_product(self):
        return self.aty.copy()

    def get_average(self):
        return self.xa.copy(), self.ya.copy()


class _State:
    step_size, primal_weight, total_number_iterations, cumulative_kkt_passes, numerical_error = 0.5, 2.0, 31, 31.0, False


def test_dump_writes_float64_samples_and_scalars(tmp_path):
    import bench
    n, m = bench.DUMP_SAMPLE + 1000, 700
    eng = _FakeEngine(n, m)
    bench.dump_outputs(str(tmp_path / "out"), eng, _State())
    got = {f[:-4]: np.load(tmp_path / "out" / f) for f in os.listdir(tmp_path / "out")}
    assert sorted(got) == sorted(NAMES + ("scalars",))
    assert all(v.dtype == np.float64 for v in got.values())
    assert sum(v.nbytes for v in got.values()) <= 64_000_000
    idx = bench.sample_index(n)
    assert np.array_equal(got["primal"], eng.x[idx]) and np.array_equal(got["dual_product"], eng.aty[idx])
    assert np.array_equal(got["primal_average"], eng.xa[idx])
    assert np.array_equal(got["dual"], eng.y) and np.array_equal(got["dual_average"], eng.ya)
    assert got["scalars"].tolist() == [0.5, 2.0, 31.0, 31.0, 0.0]
    bench.dump_outputs(str(tmp_path / "not_written"), eng, _State(), write=False)
    assert not (tmp_path / "not_written").exists()


@pytest.mark.gpu
@pytest.mark.short_rows
def test_plain_run_times_k_steps_and_dumps_their_outputs(gpu_required, tmp_path):
    """The plain command on a small LP: the line reports exactly K timed steps and nothing of --full; the dump is the
    state after W + K steps taken the way bench.py takes them, reproduced here from the same seeded LP."""
    import bench
    from firstorderlp_jl_amd import HipPdhgEngine
    from firstorderlp_jl_amd.generators import random_lp
    from firstorderlp_jl_amd.primal_dual_hybrid_gradient import AdaptiveStepsizeParams, PdhgSolverState, take_steps
    m, n, per_row, seed, steps, warmup = 3000, 2500, 7, 11, 7, 3
    out_dir = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", str(warmup), "--rows", str(m), "--cols", str(n), "--nnz-per-row", str(per_row),
                        "--seed", str(seed), "--dump-outputs", str(out_dir)],
                       cwd=ROOT, capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    d = json.loads(r.stdout.decode().rstrip("\n").split("\n")[-1])
    assert d["steps"] == steps and d["warmup"] == warmup and d["n_gpus"] == 1
    assert d["metric"] == "pdhg_iterations_per_sec" and d["unit"] == "iterations/s" and d["higher_is_better"] is True
    assert d["dtype"] == "f64" and d["ms_per_step"] > 0
    assert abs(d["value"] - 1e3 / d["ms_per_step"]) <= 1e-3 * d["value"]
    assert d["roofline"] is None and d["cpu_baseline"] is None and "other_configs" not in d

    p = random_lp(m, n, per_row, seed)
    eng = HipPdhgEngine.from_problem(p)
    step0, pw0 = bench.initial_scalars(p)
    state = PdhgSolverState(eng, step_size=step0, primal_weight=pw0)
    policy = AdaptiveStepsizeParams(0.3, 0.6)
    for k in (warmup, steps):
        done = 0
        while done < k:
            done += take_steps(policy, state, k - done)
    x, y = eng.get_current()
    want = {"primal": x, "dual": y, "dual_product": eng.get_dual_product()}
    want["primal_average"], want["dual_average"] = eng.get_average()
    eng.close()
    for name in NAMES:
        got = np.load(out_dir / (name + ".npy"))
        assert got.dtype == np.float64
        np.testing.assert_allclose(got, want[name], rtol=1e-12, atol=1e-15, err_msg=name)
    s = np.load(out_dir / "scalars.npy")
    assert s[2] == state.total_number_iterations and s[4] == float(state.numerical_error)
    np.testing.assert_allclose(s[[0, 1, 3]], [state.step_size, state.primal_weight, state.cumulative_kkt_passes], rtol=1e-12)
