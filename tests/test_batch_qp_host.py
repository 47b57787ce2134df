"""optimize_batch for QPs that share the objective matrix, on the host: what check_batch accepts and refuses (before any
library call), the lockstep driver over a batch adapter of CPU oracle engines against K solo solves, and the
random_qp_family generator.  The scheme of tests/test_batch_host.py, restated for QPs."""
import dataclasses

import numpy as np
import pytest
import scipy.sparse as sp

import folp_loader

folp = folp_loader.load()
from firstorderlp_jl_amd import _lib, optimize_batch  # noqa: E402
from firstorderlp_jl_amd import batch as batch_mod  # noqa: E402
from firstorderlp_jl_amd.generators import random_qp_family  # noqa: E402
from firstorderlp_jl_amd.primal_dual_hybrid_gradient import (AdaptiveStepsizeParams, ConstantStepsizeParams,  # noqa: E402
                                                             MalitskyPockStepsizeParameters, PdhgParameters, optimize)
from firstorderlp_jl_amd.quadratic_programming import QuadraticProgrammingProblem  # noqa: E402
from firstorderlp_jl_amd.saddle_point import (RestartScheme, RestartToCurrentMetric,  # noqa: E402
                                              construct_restart_parameters)
from firstorderlp_jl_amd.termination import construct_termination_criteria  # noqa: E402
from tests.oracle_engine import OracleEngine  # noqa: E402


def _params(tol=1e-6, limit=3000, policy=None, freq=40):
    tc = construct_termination_criteria(eps_optimal_absolute=tol, eps_optimal_relative=tol, iteration_limit=limit)
    rp = construct_restart_parameters(RestartScheme.ADAPTIVE_NORMALIZED, RestartToCurrentMetric.GAP_OVER_DISTANCE_SQUARED,
                                      1000, 0.5, 0.1, 0.9, 0.5, False)
    return PdhgParameters(10, False, 1.0, 1.0, True, 0, True, freq, tc, rp, policy or AdaptiveStepsizeParams(0.3, 0.6))


# the constraint matrix of tests/test_batch_host.py
_A = sp.csc_matrix(np.array([[1.0, 1.0, 1.0, 0.0, 2.0],
                             [1.0, -1.0, 0.0, 0.5, 0.0],
                             [0.0, 2.0, -1.0, 1.0, 1.0],
                             [3.0, 0.0, 1.0, 0.0, -1.0]]))
# a small positive definite Q (diagonally dominant, symmetric)
_Q = sp.csc_matrix(np.array([[2.0, 0.5, 0.0, 0.0, 0.0],
                             [0.5, 1.0, 0.0, 0.25, 0.0],
                             [0.0, 0.0, 0.5, 0.0, 0.0],
                             [0.0, 0.25, 0.0, 1.5, -0.5],
                             [0.0, 0.0, 0.0, -0.5, 1.0]]))


def _qp(b, c, ub=10.0, Q=None):
    n = _A.shape[1]
    return QuadraticProgrammingProblem(np.zeros(n), np.full(n, ub), (_Q if Q is None else Q).copy(), np.asarray(c, float),
                                       0.0, _A.copy(), np.asarray(b, float), 1)


def _members():
    return [_qp([1.0, 0.0, -1.0, 0.5], [1.0, 2.0, 0.5, 1.0, 3.0]),
            _qp([2.0, -0.5, 0.0, 1.0], [0.3, 1.0, 2.0, 1.5, 0.2]),
            _qp([3.0, 1.0, 0.5, -1.0], [2.0, 0.1, 0.7, 3.0, 1.0]),
            _qp([1.5, 0.5, 0.0, 0.0], [1.0, 0.5, 0.5, 2.0, 1.0], ub=4.0)]


class _OracleBatch:
    """The batch interface of HipPdhgBatch over K oracle engines (trial_step / accept per active member)."""

    def __init__(self, problems):
        self.members = [OracleEngine.from_problem(p) for p in problems]
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


def test_shared_q_is_accepted_in_any_storage(monkeypatch):
    """The same matrix given sorted, with unsorted indices, and with duplicate entries that sum to it."""
    _no_library(monkeypatch)
    problems = _members()[:3]
    # every column's entries in descending row order
    unsorted = sp.csc_matrix((_Q.data.copy(), _Q.indices.copy(), _Q.indptr.copy()), shape=_Q.shape)
    for j in range(_Q.shape[1]):
        lo, hi = unsorted.indptr[j], unsorted.indptr[j + 1]
        unsorted.indices[lo:hi] = unsorted.indices[lo:hi][::-1].copy()
        unsorted.data[lo:hi] = unsorted.data[lo:hi][::-1].copy()
    assert np.any(np.diff(unsorted.indices)[np.diff(np.repeat(np.arange(5), np.diff(unsorted.indptr))) == 0] < 0)
    # every entry stored twice, as two halves (exact in binary)
    dup = sp.csc_matrix((np.repeat(_Q.data * 0.5, 2), np.repeat(_Q.indices, 2), 2 * _Q.indptr), shape=_Q.shape)
    assert dup.nnz == 2 * _Q.nnz and (dup.toarray() == _Q.toarray()).all()
    problems[1].objective_matrix = unsorted
    problems[2].objective_matrix = dup
    assert batch_mod.check_batch(problems, _params()) == problems
    # stored zeros only, or no matrix at all: an LP batch
    lps = _members()[:2]
    lps[0].objective_matrix = sp.csc_matrix(_Q.shape)
    lps[1].objective_matrix = sp.csc_matrix((np.zeros(2), ([0, 1], [0, 1])), shape=_Q.shape)
    batch_mod.check_batch(lps, _params())


@pytest.mark.parametrize("case", ["pattern", "values", "lp_among_qps", "qp_among_lps", "malitsky_pock"])
def test_refused_before_any_library_call(monkeypatch, case):
    _no_library(monkeypatch)
    problems = _members()[:3]
    params = _params()
    where = 2
    if case == "pattern":
        Q = _Q.toarray()
        Q[0, 2] = Q[2, 0] = 0.125
        problems[2].objective_matrix = sp.csc_matrix(Q)
    elif case == "values":
        Q = _Q.copy()
        Q.data[0] = 2.5
        problems[2].objective_matrix = Q
    elif case == "lp_among_qps":
        problems[2].objective_matrix = sp.csc_matrix(_Q.shape)
    elif case == "qp_among_lps":
        for p in problems[:2]:
            p.objective_matrix = sp.csc_matrix(_Q.shape)
    elif case == "malitsky_pock":
        params = _params(policy=MalitskyPockStepsizeParameters(0.7, 1.0, 0.9))
        where = None

    def factory(ps):
        raise AssertionError("the batch was created")
    factory.takes_original_problem = True
    for kw in ({"batch_factory": factory}, {}):
        with pytest.raises(ValueError) as err:
            optimize_batch(params, problems, **kw)
        if where is not None:
            assert f"problem {where}" in str(err.value)


@pytest.mark.parametrize("policy", ["adaptive", "constant"])
def test_lockstep_driver_matches_solo_qp_solves(policy):
    """Fails before QP batches with check_batch's ValueError ("problem 0 is a QP")."""
    problems = _members()
    if policy == "adaptive":
        params = _params(freq=3)
    else:
        params = _params(limit=400, policy=ConstantStepsizeParams(), freq=7)
    want = [optimize(params, p, OracleEngine.from_problem) for p in problems]
    got = optimize_batch(params, problems, batch_factory=_OracleBatch)
    assert len(got) == len(problems)
    for g, w in zip(got, want):
        _assert_same(g, w)
    if policy == "adaptive":
        assert all(w.termination_string == "OPTIMAL" for w in want), [w.termination_string for w in want]
        assert len({w.iteration_count for w in want}) > 1, "one member should terminate at another iteration"
    # the QP term took part: the same members without Q run differently
    lp = _members()[0]
    lp.objective_matrix = sp.csc_matrix(_Q.shape)
    assert not np.array_equal(optimize(params, lp, OracleEngine.from_problem).primal_solution, want[0].primal_solution)


def test_random_qp_family():
    fam = random_qp_family(30, 40, 5, seed=3)
    assert len(fam) == 5
    assert batch_mod.check_batch(fam, _params()) == fam
    Q = fam[0].objective_matrix
    assert Q.shape == (40, 40) and (abs(Q - Q.T)).nnz == 0 and (Q.diagonal() > 0).all()
    assert np.linalg.eigvalsh(Q.toarray()).min() > 0
    for p in fam[1:]:
        assert (p.constraint_matrix != fam[0].constraint_matrix).nnz == 0
        assert not np.array_equal(p.objective_vector, fam[0].objective_vector)
        assert not np.array_equal(p.right_hand_side, fam[0].right_hand_side)
        assert not np.array_equal(p.variable_upper_bound, fam[0].variable_upper_bound)
    again = random_qp_family(30, 40, 5, seed=3)
    assert all(np.array_equal(a.objective_vector, b.objective_vector) for a, b in zip(fam, again))
