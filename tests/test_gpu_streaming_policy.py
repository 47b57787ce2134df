"""The plain-launch kernels read their once-per-launch operands with non-temporal loads: the sweep's row epilogue
(spmv_tiled_kernel<MODE_DUAL, .> / <MODE_ATY, .>: y, b, sum_y / x', x, A'y) and primal_kernel (x, c, A'y, sum_x and the
words of a SPARSE bound view).  Only the cache policy of a load changes, never an operand, an order or a rounding, so
everything here is bitwise: the engine with the policy on against the same engine with the dev switches off
(PDHG_EPI_STREAM=0, PDHG_PRIMAL_STREAM=0: read per launch, so one process holds both), and against the oracle.  Left
alone the library streams only where a sweep has more workgroups than the device holds at once (millions of rows), so
"on" is the switches at 1 here.

Sweep epilogue: the geometry of tests/test_gpu_tiled_epilogue_edges.py (m = 8 R + R + 1 rows: a full workgroup, a full
wave, a wave of one row, dead waves; both products).  Primal step: the odd tail, fewer columns than a wave covers, one
mask block of a SPARSE view and one more, every mode of either bound vector.  Each script runs a trial with nothing
pending, one that carries the deferred average term in the single form, and take_steps through the C loop that stage
the paired form.  A stream-layout LP and a two-shard group do not take the new path: unchanged layouts, the same bits.

(Non-temporal STORES of the same kernels were measured too and made the products behind them slower -- NOTEBOOK
section 14 -- so the stores are the plain ones and there is nothing of theirs to test.)"""
import os

import numpy as np
import pytest
import scipy.sparse as sp

from firstorderlp_jl_amd import HipPdhgEngine, linear_programming_problem
from firstorderlp_jl_amd.generators import random_lp
from firstorderlp_jl_amd.primal_dual_hybrid_gradient import AdaptiveStepsizeParams, PdhgSolverState, take_step, take_steps
from tests import helpers as H

pytestmark = pytest.mark.gpu

TILE_COLS = 97
INF = np.inf
POLICY = AdaptiveStepsizeParams(0.3, 0.6)
SWITCHES = ("PDHG_EPI_STREAM", "PDHG_PRIMAL_STREAM")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b, label):
    assert len(a) == len(b), label
    for k, (u, v) in enumerate(zip(a, b)):
        assert np.array_equal(_bits(u), _bits(v)), f"{label}: array {k} differs between policy on and switch off"


def _policy(monkeypatch, on):
    for k in SWITCHES:
        monkeypatch.setenv(k, "1" if on else "0")


def _forced_sweep(monkeypatch, tw_rows=None):
    monkeypatch.setenv("PDHG_GRAPH", "0")              # launch by launch: the kernels that know the policy
    monkeypatch.setenv("PDHG_SPMV", "tiled")
    monkeypatch.setenv("PDHG_TILE_COLS", str(TILE_COLS))
    if tw_rows is not None:
        monkeypatch.setenv("PDHG_TW_ROWS", str(tw_rows))


def _counters(eng):
    d = eng.layout_describe()["average_update"]
    return d["form"], d["paired_accepts"], d["dropped_stagings"]


def _longest_run_in_a_tile(M):
    M = sp.csr_matrix(M)
    if M.nnz == 0:
        return 0
    rows = np.repeat(np.arange(M.shape[0], dtype=np.int64), np.diff(M.indptr))
    ntile = M.shape[1] // TILE_COLS + 1
    return int(np.unique(rows * ntile + M.indices // TILE_COLS, return_counts=True)[1].max())


def _trials(eng, st, p, label, bitwise, monkeypatch, check):
    """Two trials with an accept between them (the second carries the deferred sum_x / sum_y terms in the single form),
    another accept, then two take_steps through the C loop, the first of which stages the paired form.  check: against
    the oracle `st` as tests/test_gpu_tiled_epilogue_edges.py does.  Returns every array read from the device."""
    A = p.constraint_matrix
    step, pw = H.initial_step_and_weight(p)
    seen = []
    raw = eng.trial_step(step, pw, 1.0)
    seen += list(eng.get_trial()) + [np.array(raw)]
    if check:
        H.assert_trial_matches_oracle(raw, eng.get_trial(), st, step, pw, A, label=label + ", first trial")
    eng.accept(step)
    if check:
        st.step_size = step
        st.accept(st.x_next, st.y_next, st.aty_next)
        if not bitwise:                                 # the second trial starts from the device's own iterate
            st.x, st.y = eng.get_current()
            st.aty = eng.get_dual_product()
    raw = eng.trial_step(0.9 * step, pw, 1.0)
    seen += list(eng.get_trial()) + [np.array(raw)]
    if check:
        H.assert_trial_matches_oracle(raw, eng.get_trial(), st, 0.9 * step, pw, A, label=label + ", second trial")
    xa, ya = eng.get_average()
    seen += [xa, ya]
    if check:
        wxa, wya = st.compute_average()
        if bitwise:
            assert np.array_equal(_bits(xa), _bits(wxa)) and np.array_equal(_bits(ya), _bits(wya)), label + ": average"
        else:
            np.testing.assert_allclose(xa, wxa, rtol=1e-9, atol=1e-12)
            np.testing.assert_allclose(ya, wya, rtol=1e-9, atol=1e-12)
    # the accept leaves its term pending on both sums: the first take_step of the C loop stages the paired form
    eng.accept(0.9 * step)
    state = PdhgSolverState(eng, step_size=0.9 * step, primal_weight=pw)
    before = _counters(eng)
    assert take_steps(POLICY, state, 2) == 2
    form, paired, _ = _counters(eng)
    assert form == "paired" and paired > before[1], (label, before, (form, paired))
    seen += list(eng.get_trial()) + list(eng.get_average()) + list(eng.get_current())
    seen.append(np.array([state.step_size, state.total_number_iterations], dtype=np.float64))
    return seen


def _free_running(p, label, bitwise, steps=4):
    """take_steps through the C loop from the start against the oracle's: every second one stages."""
    eng = HipPdhgEngine.from_problem(p)
    step, pw = H.initial_step_and_weight(p)
    st = PdhgSolverState(eng, step_size=step, primal_weight=pw)
    for _ in range(steps):
        take_step(POLICY, st)
    x, y = eng.get_current()
    xa, ya = eng.get_average()
    counters = _counters(eng)
    eng.close()
    o = H.oracle_from_problem(p)
    o.exact_sums = True
    o.step_size, o.primal_weight, o.ratio_step_sizes = step, pw, 1.0
    for _ in range(steps):
        o.take_step_adaptive(POLICY.reduction_exponent, POLICY.growth_exponent)
    oxa, oya = o.compute_average()
    assert counters[0] == "paired" and counters[1] >= 1, (label, counters)
    assert st.total_number_iterations == o.total_number_iterations, label + ": accept / reject decisions differ"
    for got, want, name in ((x, o.x, "x"), (y, o.y, "y"), (xa, oxa, "average x"), (ya, oya, "average y")):
        if bitwise:
            assert np.array_equal(_bits(got), _bits(want)), f"{label}: {name} after {steps} take_steps"
        else:
            np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-12)
    assert (st.step_size == o.step_size) if bitwise else np.isclose(st.step_size, o.step_size, rtol=1e-9), label
    o.close()


# ---- the sweep's row epilogue ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("swap", [False, True], ids=["rows_of_A", "rows_of_At"])
@pytest.mark.parametrize("R", [1, 64, 65, 300])
def test_streaming_row_epilogue_is_bitwise_the_plain_one(gpu_required, monkeypatch, R, swap):
    _forced_sweep(monkeypatch, R)
    long_side, short_side = 8 * R + R + 1, 500
    m, n = (short_side, long_side) if swap else (long_side, short_side)
    p = random_lp(m, n, 5, seed=R)
    A = p.constraint_matrix
    label = f"R = {R}, {'A transposed' if swap else 'A'}"
    bitwise = os.environ.get("PDHG_ROW_ORDER") == "strict" or max(_longest_run_in_a_tile(A), _longest_run_in_a_tile(A.T)) <= 8
    assert bitwise or (R == 1 and swap), label          # the one case tests/test_gpu_tiled_epilogue_edges.py names
    if not bitwise:
        monkeypatch.setattr(H, "bitexact_row_limit", lambda: 8)
    runs, infos = [], []
    for on in (True, False):
        _policy(monkeypatch, on)
        eng = HipPdhgEngine.from_problem(p)
        info = eng.layout_info()
        assert info["A_tiled_waves"] > 0 and info["At_tiled_waves"] > 0
        assert info["At_tiled_waves" if swap else "A_tiled_waves"] == 10, info
        st = H.oracle_from_problem(p)
        runs.append(_trials(eng, st, p, label + (", policy on" if on else ", switch off"), bitwise, monkeypatch, check=True))
        infos.append(info)
        eng.close()
        st.close()
    assert infos[0] == infos[1], label
    _same(runs[0], runs[1], label)
    _policy(monkeypatch, True)
    _free_running(p, label, bitwise)


# ---- the primal step -------------------------------------------------------------------------------------------------

def _lp(n, lb, ub, seed):
    """m = ceil(n / 2) equality rows of (up to) 3 entries: row i holds columns 2i, 2i + 1 and a random one, so every column
    has an entry and xbar shows in y' (tests/test_gpu_primal_bounds.py)."""
    rng = np.random.default_rng(seed)
    m = (n + 1) // 2
    rows = np.repeat(np.arange(m), 3)
    cols = np.stack([(2 * np.arange(m)) % n, (2 * np.arange(m) + 1) % n, rng.integers(0, n, m)], axis=1).reshape(-1)
    A = sp.coo_matrix((rng.standard_normal(3 * m), (rows, cols)), shape=(m, n)).tocsc()
    A.sum_duplicates()
    A.sort_indices()
    assert (np.diff(A.indptr) > 0).all()
    return linear_programming_problem(lb, ub, rng.standard_normal(n), 0.0, A, rng.standard_normal(m), m)


def _patterns(n, seed):
    """name -> (lb, ub, the modes expected at n >= 127); lb <= ub everywhere."""
    rng = np.random.default_rng(seed)
    inf_ub = np.full(n, INF)

    def finite_ub(share):
        ub = inf_ub.copy()
        k = int(round(share * n))
        ub[rng.choice(n, size=k, replace=False)] = 4.0 + rng.random(k)
        return ub
    one = np.zeros(n)
    one[min(n - 1, 64)] = -1.25
    tail = np.zeros(n)                                  # exceptions in the last (partial) block and the odd tail element
    tail[n - 1] = -0.5
    return {
        "const / const": (np.zeros(n), inf_ub, ("const", "const")),
        "const / sparse": (np.full(n, -INF), finite_ub(0.2), ("const", "sparse")),
        "sparse / sparse": (one, finite_ub(0.2), ("sparse", "sparse")),
        "sparse (last column) / const": (tail, inf_ub, ("sparse", "const")),
        "dense / dense": (-1.0 - rng.random(n), 4.0 + rng.random(n), ("dense", "dense")),
        "sparse / dense": (one, 4.0 + rng.random(n), ("sparse", "dense")),
    }


@pytest.mark.parametrize("n", [1, 2, 3, 127, 128, 129, 1001])
def test_streaming_primal_step_is_bitwise_the_plain_one(gpu_required, monkeypatch, n):
    _forced_sweep(monkeypatch)
    for name, (lb, ub, modes) in _patterns(n, seed=n).items():
        label = f"n = {n}, {name}"
        p = _lp(n, lb, ub, seed=n + 1)
        runs, infos = [], []
        for on in (True, False):
            _policy(monkeypatch, on)
            eng = HipPdhgEngine.from_problem(p)
            info = eng.layout_info()
            if n >= 127:
                assert (info["lb_mode"], info["ub_mode"]) == modes, (label, info["lb_mode"], info["ub_mode"])
            st = H.oracle_from_problem(p)
            # x' on its own first (trial_primal: nothing pending, no xbar consumer)
            step, pw = H.initial_step_and_weight(p)
            eng.trial_primal(step, pw)
            gx = eng.get_trial()[0]
            assert np.array_equal(_bits(gx), _bits(st.trial_primal(step, pw))), label + ": x' (trial_primal)"
            runs.append([gx] + _trials(eng, st, p, label + (", policy on" if on else ", switch off"), True, monkeypatch, check=True))
            infos.append(info)
            eng.close()
            st.close()
        assert infos[0] == infos[1], label
        _same(runs[0], runs[1], label)
        _policy(monkeypatch, True)
        _free_running(p, label, True)


# ---- handles that do not take the new path ---------------------------------------------------------------------------

OTHERS = {
    "stream_layout_lp": (lambda: random_lp(700, 901, 6, seed=3), False, {}),
    "two_shard_group": (lambda: random_lp(1300, 1111, 6, seed=4), True, {"device_ids": [0, 0]}),
}


@pytest.mark.parametrize("name", sorted(OTHERS))
def test_other_layouts_are_unchanged(gpu_required, monkeypatch, name):
    maker, sweep, kw = OTHERS[name]
    p = maker()
    for k in ("PDHG_GRAPH", "PDHG_COOP", "PDHG_SPMV", "PDHG_TILE_COLS", "PDHG_TW_ROWS"):
        monkeypatch.delenv(k, raising=False)
    if sweep:
        monkeypatch.setenv("PDHG_SPMV", "tiled")
        monkeypatch.setenv("PDHG_TILE_COLS", "256")
    outs = []
    for on in (True, False):
        _policy(monkeypatch, on)
        eng = HipPdhgEngine.from_problem(p, **kw)
        info = eng.layout_info()
        if not sweep:
            assert info["A_tiled_waves"] == 0 and info["At_tiled_waves"] == 0, info
        step, pw = H.initial_step_and_weight(p)
        st = PdhgSolverState(eng, step_size=step, primal_weight=pw)
        assert take_steps(POLICY, st, 5) == 5
        first = np.concatenate(eng.get_average())
        st.step_size *= 64.0
        for _ in range(4):
            take_step(POLICY, st)
        outs.append((info, st.total_number_iterations, st.step_size, _counters(eng),
                     [first, np.concatenate(eng.get_average()), np.concatenate(eng.get_current())]))
        eng.close()
    assert outs[0][:4] == outs[1][:4], name
    assert outs[0][3] == ("single", 0, 0), outs[0][3]
    _same(outs[0][4], outs[1][4], name)
