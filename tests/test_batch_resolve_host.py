"""Re-solves of a batch on the host: the exports of include/pdhg_hip_batch_resolve.h, ``optimize_batch(...,
initial_solutions=)`` over a batch of CPU oracle engines, and ``PdhgBatchSession`` over an oracle batch whose members
implement ``update_problem_vectors`` / ``warm_start`` in numpy -- a session's solve after an update must be, bit for bit,
``optimize`` on the updated problem."""
import ctypes
import dataclasses
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import folp_loader

folp = folp_loader.load()
from firstorderlp_jl_amd import PdhgBatchSession, _lib, optimize_batch  # noqa: E402
from firstorderlp_jl_amd.primal_dual_hybrid_gradient import (AdaptiveStepsizeParams, ConstantStepsizeParams,  # noqa: E402
                                                             MalitskyPockStepsizeParameters, PdhgParameters, optimize)
from firstorderlp_jl_amd.quadratic_programming import linear_programming_problem  # noqa: E402
from firstorderlp_jl_amd.saddle_point import (RestartScheme, RestartToCurrentMetric,  # noqa: E402
                                              construct_restart_parameters)
from firstorderlp_jl_amd.termination import construct_termination_criteria  # noqa: E402
from tests.helpers import ResolveOracleEngine, assert_same_output as _assert_same  # noqa: E402
from tests.oracle_engine import OracleEngine  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ["pdhg_batch_resolve_info", "pdhg_batch_resolve_retain", "pdhg_batch_update_problem_vectors",
               "pdhg_batch_warm_start"]


def _params(policy=None, tol=1e-7, limit=300, freq=5):
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


def _family():
    return [_lp([1.0, 0.0, -1.0, 0.5], [1.0, 2.0, 0.5, 1.0, 3.0]),
            _lp([2.0, -0.5, 0.0, 1.0], [0.3, 1.0, 2.0, 1.5, 0.2]),
            _lp([3.0, 1.0, 0.5, -1.0], [2.0, 0.1, 0.7, 3.0, 1.0])]


class _OracleBatch:
    """The batch interface of HipPdhgBatch over K oracle engines (trial_step / accept per active member); it has none
    of the batch's own re-solve calls, so a session serves it member by member."""
    engine = OracleEngine

    def __init__(self, problems):
        self.members = [self.engine.from_problem(p) for p in problems]
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


class _ResolveOracleBatch(_OracleBatch):
    engine = ResolveOracleEngine


# ---- the exports ----

def test_the_batch_resolve_header_declares_exactly_the_new_exports_and_the_library_has_them():
    header = open(os.path.join(ROOT, "include", "pdhg_hip_batch_resolve.h")).read()
    declared = sorted(set(re.findall(r"\b(pdhg_[a-z_0-9]+)\s*\(", header)))
    assert declared == NEW_EXPORTS == sorted(_lib.BATCH_RESOLVE_EXPORTS)
    L = ctypes.CDLL(_lib.LIB_PATH)       # loads without a GPU
    for name in declared:
        assert hasattr(L, name), f"{name} not exported by libpdhg_hip.so"
    # the lists the existing tests pin are as they were
    assert len(_lib.EXPORTS) == 69 and len(_lib.RESOLVE_EXPORTS) == 6
    assert not set(_lib.BATCH_RESOLVE_EXPORTS) & (set(_lib.EXPORTS) | set(_lib.RESOLVE_EXPORTS))
    assert _lib.lib().pdhg_abi_version() == _lib.ABI_VERSION == 11
    for name in ("pdhg_hip.h", "pdhg_hip_resolve.h"):
        other = open(os.path.join(ROOT, "include", name)).read()
        assert not set(re.findall(r"\b(pdhg_[a-z_0-9]+)\s*\(", other)) & set(NEW_EXPORTS), name


def test_null_handles_are_refused_without_a_gpu():
    L = _lib.lib()
    out = np.zeros(4, dtype=np.int64)
    calls = {"pdhg_batch_resolve_retain": (), "pdhg_batch_update_problem_vectors": (None, None, None, None),
             "pdhg_batch_warm_start": (None, None), "pdhg_batch_resolve_info": (out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),)}
    assert sorted(calls) == NEW_EXPORTS
    for name, args in calls.items():
        assert getattr(L, name)(None, *args) == -1, name
        assert b"null handle" in L.pdhg_last_error(), name
    assert L.pdhg_batch_resolve_info(None, None) == -1
    assert not out.any()


# ---- optimize_batch(..., initial_solutions=) over the oracle ----

@pytest.mark.parametrize("policy", [AdaptiveStepsizeParams(0.3, 0.6), ConstantStepsizeParams()], ids=["adaptive", "constant"])
def test_optimize_batch_takes_a_point_per_problem(policy):
    problems = _family()
    params = _params(policy, limit=150)
    rng = np.random.default_rng(3)
    points = [(rng.uniform(0, 1, 5), rng.uniform(0, 1, 4)) for _ in problems]
    points[1] = None
    points[2] = (points[2][0], None)
    want = [optimize(params, p, OracleEngine.from_problem, *(pt or (None, None))) for p, pt in zip(problems, points)]
    got = optimize_batch(params, problems, batch_factory=_OracleBatch, initial_solutions=points)
    for g, w in zip(got, want):
        _assert_same(g, w)
    # a dual point alone, and a solve from its own solution, which ends at once
    cold = optimize_batch(params, problems, batch_factory=_OracleBatch)
    for g, w in zip(optimize_batch(params, problems, batch_factory=_OracleBatch, initial_solutions=[None] * 3), cold):
        _assert_same(g, w)
    points = [(None, rng.uniform(0, 1, 4)), (cold[1].primal_solution, cold[1].dual_solution), None]
    want = [optimize(params, p, OracleEngine.from_problem, *(pt or (None, None))) for p, pt in zip(problems, points)]
    for g, w in zip(optimize_batch(params, problems, batch_factory=_OracleBatch, initial_solutions=points), want):
        _assert_same(g, w)


def test_initial_solutions_are_checked_before_the_factory_is_called():
    problems = _family()

    def factory(ps):
        raise AssertionError("the batch was created")
    ok = (np.zeros(5), np.zeros(4))
    for bad in ([ok, ok], [ok, ok, ok, ok], [ok, (np.zeros(4), None), None], [None, (None, np.zeros(5)), None],
                [(np.array([0.0, np.nan, 0.0, 0.0, 0.0]), None), None, None], [None, None, (None, np.array([0.0, np.inf, 0.0, 0.0]))],
                [None, (np.zeros((5, 1)), np.zeros(4)), None]):
        with pytest.raises(ValueError):
            optimize_batch(_params(), problems, batch_factory=factory, initial_solutions=bad)
    with pytest.raises(AssertionError):              # ... and a good list reaches it
        optimize_batch(_params(), problems, batch_factory=factory, initial_solutions=[ok, None, ok])


# ---- sessions over the oracle ----

def _updates(problems):
    """New right-hand sides and one moved bound for members 0 and 2, a new objective vector for member 1."""
    ub = problems[2].variable_upper_bound.copy()
    ub[0] = 7.5
    return [{"right_hand_side": problems[0].right_hand_side * 1.01 + 0.003}, {"objective_vector": problems[1].objective_vector * 1.5},
            {"right_hand_side": problems[2].right_hand_side * 0.99, "variable_upper_bound": ub}]


@pytest.mark.parametrize("policy", [AdaptiveStepsizeParams(0.3, 0.6), ConstantStepsizeParams()], ids=["adaptive", "constant"])
def test_a_batch_session_is_optimize_per_problem(policy):
    problems = _family()
    params = _params(policy)
    with PdhgBatchSession(params, problems, _ResolveOracleBatch) as session:
        for g, p in zip(session.solve(), problems):
            _assert_same(g, optimize(params, p, OracleEngine.from_problem))
        updates = _updates(problems)
        updates[1] = None
        session.update(updates)
        updated = [p if u is None else dataclasses.replace(p.copy(), **u) for p, u in zip(problems, updates)]
        assert all(np.array_equal(a.right_hand_side, b.right_hand_side) for a, b in zip(session.problems, updated))
        want = [optimize(params, p, OracleEngine.from_problem) for p in updated]
        for g, w in zip(session.solve(), want):
            _assert_same(g, w)
        for g, w in zip(session.solve(), optimize_batch(params, updated, batch_factory=_OracleBatch)):
            _assert_same(g, w)
        # warm: points (one whole, one kept at zeros, one partial), then the last solutions
        warm = [(want[0].primal_solution * 0.9, want[0].dual_solution * 1.1), None, (None, want[2].dual_solution)]
        got = session.solve(warm_start=warm)
        for g, p, pt in zip(got, updated, warm):
            _assert_same(g, optimize(params, p, OracleEngine.from_problem, *(pt or (None, None))))
        for g, w in zip(got, optimize_batch(params, updated, batch_factory=_OracleBatch, initial_solutions=warm)):
            _assert_same(g, w)
        last = session.solve()
        for g, p, w in zip(session.solve(warm_start=True), updated, last):
            _assert_same(g, optimize(params, p, OracleEngine.from_problem, w.primal_solution, w.dual_solution))


def test_a_batch_session_has_the_preconditions_of_optimize_batch():
    problems = _family()

    def factory(ps):
        raise AssertionError("the batch was created")
    with pytest.raises(ValueError, match="Malitsky"):
        PdhgBatchSession(_params(MalitskyPockStepsizeParameters(0.7, 0.99, 1.0)), problems, factory)
    other = _lp([1.0, 0.0, 0.0, 0.0], [1.0, 1.0, 1.0, 1.0, 1.0])
    other.constraint_matrix = (other.constraint_matrix * 2.0).tocsc()
    with pytest.raises(ValueError, match="other values"):
        PdhgBatchSession(_params(), problems + [other], factory)
    with pytest.raises(ValueError):
        PdhgBatchSession(_params(), [], factory)


@pytest.mark.parametrize("bad", [{"variable_lower_bound": np.array([0.0, 0.0, 11.0, 0.0, 0.0])},        # lb[2] = 11 > ub[2] = 10
                                 {"right_hand_side": np.array([12.0, np.nan, 1.0, 0.0])},
                                 {"variable_lower_bound": np.array([0.0, np.inf, 0.0, 0.0, 0.0])},
                                 {"objective_vector": np.zeros(3)}],
                         ids=["lb_above_ub", "nan_rhs", "inf_lb", "wrong_length"])
def test_an_update_that_fails_validation_leaves_the_session_as_it_was(bad):
    problems = _family()
    params = _params(limit=200)
    with PdhgBatchSession(params, problems, _ResolveOracleBatch) as session:
        before = session.solve()
        calls = []
        for eng in session.batch.members:
            eng.update_problem_vectors = lambda **kw: calls.append(kw)      # no device work may be reached
        good = _updates(problems)
        with pytest.raises(ValueError):
            session.update([good[0], good[1], bad])                         # the members before the bad one are not updated either
        with pytest.raises(ValueError):
            session.update([good[0]])
        assert not calls
        for eng in session.batch.members:
            del eng.update_problem_vectors
        for g, w in zip(session.solve(), before):
            _assert_same(g, w)
        for got, p in zip(session.problems, problems):
            assert np.array_equal(got.right_hand_side, p.right_hand_side) and np.array_equal(got.objective_vector, p.objective_vector)
        with pytest.raises(ValueError):
            session.solve(warm_start=[None, None])
        with pytest.raises(ValueError):
            session.solve(warm_start=[None, (np.zeros(4), None), None])
    for call in (session.solve, lambda: session.update([None] * 3), lambda: session.batch, lambda: session.problems):
        with pytest.raises(RuntimeError, match="closed"):
            call()
