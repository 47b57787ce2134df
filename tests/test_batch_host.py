"""optimize_batch on the host: argument checks (before any library call) and the driver's lockstep logic through
``batch_factory`` -- a batch adapter over K CPU oracle engines must give exactly what K runs of
``optimize(..., engine_factory=OracleEngine...)`` give."""
import dataclasses
import math

import numpy as np
import pytest
import scipy.sparse as sp

import folp_loader

folp = folp_loader.load()
from firstorderlp_jl_amd import _lib, optimize_batch  # noqa: E402
from firstorderlp_jl_amd import batch as batch_mod  # noqa: E402
from firstorderlp_jl_amd.generators import l1_svm_regularization_path, personalized_pagerank_lps  # noqa: E402
from firstorderlp_jl_amd.primal_dual_hybrid_gradient import (AdaptiveStepsizeParams, ConstantStepsizeParams,  # noqa: E402
                                                             MalitskyPockStepsizeParameters, PdhgParameters, optimize)
from firstorderlp_jl_amd.quadratic_programming import linear_programming_problem  # noqa: E402
from firstorderlp_jl_amd.saddle_point import (RestartScheme, RestartToCurrentMetric,  # noqa: E402
                                              construct_restart_parameters)
from firstorderlp_jl_amd.termination import construct_termination_criteria  # noqa: E402
from tests.oracle_engine import OracleEngine  # noqa: E402


def _params(tol=1e-6, limit=3000, policy=None, freq=40):
    tc = construct_termination_criteria(eps_optimal_absolute=tol, eps_optimal_relative=tol, iteration_limit=limit)
    rp = construct_restart_parameters(RestartScheme.ADAPTIVE_NORMALIZED, RestartToCurrentMetric.GAP_OVER_DISTANCE_SQUARED,
                                      1000, 0.5, 0.1, 0.9, 0.5, False)
    return PdhgParameters(10, False, 1.0, 1.0, True, 0, True, freq, tc, rp, policy or AdaptiveStepsizeParams(0.3, 0.6))


_A = sp.csc_matrix(np.array([[1.0, 1.0, 1.0, 0.0, 2.0],
                             [1.0, -1.0, 0.0, 0.5, 0.0],
                             [0.0, 2.0, -1.0, 1.0, 1.0],
                             [3.0, 0.0, 1.0, 0.0, -1.0]]))


def _lp(b, c, ub=10.0):
    n = _A.shape[1]
    return linear_programming_problem(np.zeros(n), np.full(n, ub), np.asarray(c, float), 0.0, _A.copy(),
                                      np.asarray(b, float), 1)


def _members():
    return [_lp([1.0, 0.0, -1.0, 0.5], [1.0, 2.0, 0.5, 1.0, 3.0]),
            _lp([2.0, -0.5, 0.0, 1.0], [0.3, 1.0, 2.0, 1.5, 0.2]),
            _lp([3.0, 1.0, 0.5, -1.0], [2.0, 0.1, 0.7, 3.0, 1.0]),
            _lp([-1.0, 0.0, 0.0, 0.0], [1.0, 1.0, 1.0, 1.0, 1.0])]      # x >= 0 with sum(x[:3]) + 2 x4 = -1: infeasible


class _ZeroMovementAfter:
    """An oracle engine whose trials report zero movement from trial `after` on: raises numerical_error in the
    middle of a run of steps (the same wrapper drives the solo solve)."""

    def __init__(self, eng, after):
        self._eng, self._after, self._trials = eng, after, 0

    def __getattr__(self, name):
        return getattr(self._eng, name)

    def trial_step(self, step_size, primal_weight, theta=1.0):
        raw = self._eng.trial_step(step_size, primal_weight, theta)
        self._trials += 1
        return np.zeros(5) if self._trials >= self._after else raw


def _engine_factory(k):
    def make(p):
        eng = OracleEngine.from_problem(p)
        return _ZeroMovementAfter(eng, 57) if k == 4 else eng
    return make


class _OracleBatch:
    """The batch interface of HipPdhgBatch over K oracle engines (trial_step / accept per active member)."""

    def __init__(self, problems):
        self.members = [_engine_factory(k)(p) for k, p in enumerate(problems)]
        self.K = len(problems)

    def trial_step(self, step_sizes, primal_weights, theta=1.0, active=None):
        out = np.full((self.K, 5), np.nan)
        for k, eng in enumerate(self.members):
            if active[k]:
                out[k] = eng.trial_step(step_sizes[k], primal_weights[k], theta)
        return out

    def accept(self, accept, avg_weights):
        for k, eng in enumerate(self.members):
            if accept[k]:
                eng.accept(avg_weights[k])

    def close(self):
        for eng in self.members:
            eng.close()


def _stats_key(s):
    d = dataclasses.asdict(s)
    d.pop("cumulative_time_sec")
    d["method_specific_stats"] = {k: v for k, v in d["method_specific_stats"].items() if "time" not in k}
    return repr(d)


def _assert_same(got, want):
    assert got.termination_reason == want.termination_reason
    assert got.iteration_count == want.iteration_count
    assert np.array_equal(got.primal_solution, want.primal_solution, equal_nan=True)
    assert np.array_equal(got.dual_solution, want.dual_solution, equal_nan=True)
    assert [_stats_key(s) for s in got.iteration_stats] == [_stats_key(s) for s in want.iteration_stats]


def _no_library(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("a library call was made")
    monkeypatch.setattr(_lib, "lib", refuse)


def test_lockstep_driver_matches_solo_solves():
    problems = _members() + [_lp([1.5, 0.5, 0.0, 0.0], [1.0, 0.5, 0.5, 2.0, 1.0])]
    params = _params(freq=3)
    want = [optimize(params, p, _engine_factory(k)) for k, p in enumerate(problems)]
    got = optimize_batch(params, problems, batch_factory=_OracleBatch)
    assert len(got) == len(problems)
    for g, w in zip(got, want):
        _assert_same(g, w)
    counts = {w.iteration_count for w in want[:3]}
    assert len(counts) == 3, "the feasible members should converge at different iterations"
    assert want[3].termination_string == "PRIMAL_INFEASIBLE"
    assert want[4].termination_string == "NUMERICAL_ERROR"


def test_constant_policy_matches_solo_solves():
    problems = _members()[:2]
    params = _params(limit=200, policy=ConstantStepsizeParams())
    want = [optimize(params, p, OracleEngine.from_problem) for p in problems]
    got = optimize_batch(params, problems, batch_factory=_OracleBatch)
    for g, w in zip(got, want):
        _assert_same(g, w)


@pytest.mark.parametrize("case", ["pattern", "values", "num_equalities", "qp", "malitsky_pock", "empty", "too_many", "shape"])
def test_refused_before_any_library_call(monkeypatch, case):
    _no_library(monkeypatch)
    problems = _members()[:2]
    params = _params()
    if case == "pattern":
        A = _A.toarray()
        A[0, 3] = 1.0
        problems[1].constraint_matrix = sp.csc_matrix(A)
    elif case == "values":
        A = _A.copy()
        A.data[0] = 7.0
        problems[1].constraint_matrix = A
    elif case == "num_equalities":
        problems[1].num_equalities = 2
    elif case == "qp":
        problems[1].objective_matrix = sp.identity(_A.shape[1], format="csc")
    elif case == "malitsky_pock":
        params = _params(policy=MalitskyPockStepsizeParameters(0.7, 1.0, 0.9))
    elif case == "empty":
        problems = []
    elif case == "too_many":
        problems = [_members()[0] for _ in range(33)]
    elif case == "shape":
        problems[1] = linear_programming_problem(np.zeros(4), np.ones(4), np.ones(4), 0.0, _A[:, :4], np.ones(4), 1)

    def factory(ps):
        raise AssertionError("the batch was created")
    factory.takes_original_problem = True
    with pytest.raises(ValueError):
        optimize_batch(params, problems, batch_factory=factory)
    with pytest.raises(ValueError):
        optimize_batch(params, problems)


def test_generators_share_the_matrix():
    n = 300
    rng = np.random.default_rng(0)
    tele = [np.full(n, 1.0 / n)] + [rng.dirichlet(np.ones(n)) for _ in range(2)]
    pps = personalized_pagerank_lps(n, tele, seed=1)
    assert len(pps) == 3
    base = folp.generators.pagerank_lp(n, seed=1)
    assert np.allclose(pps[0].right_hand_side, base.right_hand_side, rtol=1e-14, atol=0)
    assert (pps[0].constraint_matrix != pps[2].constraint_matrix).nnz == 0
    assert np.array_equal(pps[1].right_hand_side[1:], (1.0 - 0.99) * tele[1])
    batch_mod.check_batch(pps)
    X = sp.random(40, 12, density=0.3, random_state=1, format="csc")
    y = np.where(np.arange(40) % 2 == 0, 1.0, -1.0)
    path = l1_svm_regularization_path(X, y, [0.1, 1.0, 10.0])
    assert [p.objective_vector[-1] for p in path] == [0.1, 1.0, 10.0]
    batch_mod.check_batch(path)
    assert not math.isnan(path[2].objective_vector.sum())
