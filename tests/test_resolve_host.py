"""Re-solves on the host: the exports of include/pdhg_hip_resolve.h, warm starts of ``optimize`` over the CPU oracle, and
``PdhgSession`` / ``PdhgFleetSession`` over an oracle engine that implements ``update_problem_vectors`` / ``warm_start``
in numpy -- a session's solve after an update must be, bit for bit, ``optimize`` on the updated problem."""
import ctypes
import dataclasses
import os
import re

import numpy as np
import pytest

import folp_loader

folp = folp_loader.load()
from firstorderlp_jl_amd import PdhgFleetSession, PdhgSession, _lib, optimize_many  # noqa: E402
from firstorderlp_jl_amd.generators import random_lp  # noqa: E402
from firstorderlp_jl_amd.primal_dual_hybrid_gradient import (AdaptiveStepsizeParams, ConstantStepsizeParams,  # noqa: E402
                                                             MalitskyPockStepsizeParameters, PdhgParameters, optimize)
from firstorderlp_jl_amd.saddle_point import (RestartScheme, RestartToCurrentMetric,  # noqa: E402
                                              construct_restart_parameters)
from firstorderlp_jl_amd.solve_log import TerminationReason  # noqa: E402
from firstorderlp_jl_amd.termination import construct_termination_criteria  # noqa: E402
from tests import helpers as H  # noqa: E402
from tests.helpers import ResolveOracleEngine, assert_same_output as _assert_same  # noqa: E402
from tests.oracle_engine import OracleEngine  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _params(policy=None, tol=1e-8, limit=2000, freq=5, ruiz=10, pc=1.0):
    tc = construct_termination_criteria(eps_optimal_absolute=tol, eps_optimal_relative=tol, iteration_limit=limit)
    rp = construct_restart_parameters(RestartScheme.ADAPTIVE_NORMALIZED, RestartToCurrentMetric.GAP_OVER_DISTANCE_SQUARED,
                                      1000, 0.5, 0.1, 0.9, 0.5, False)
    return PdhgParameters(ruiz, False, pc, 1.0, True, 0, True, freq, tc, rp, policy or AdaptiveStepsizeParams(0.3, 0.6))


class _ResolveOracleFleet:
    def __init__(self, problems):
        self.members = [ResolveOracleEngine.from_problem(p) for p in problems]

    def close(self):
        for eng in self.members:
            eng.close()


def _small_problems():
    return {"example_lp": H.example_lp(), "lp_without_bounds": H.example_lp_without_bounds(),
            "dependent_rows": H.example_lp_dependent_rows(), "cc_star": H.example_cc_star_lp(), "example_qp": H.example_qp()}


# ---- the exports ----

def test_the_resolve_header_declares_exactly_the_resolve_exports_and_the_library_has_them():
    header = open(os.path.join(ROOT, "include", "pdhg_hip_resolve.h")).read()
    declared = sorted(set(re.findall(r"\b(pdhg_[a-z_0-9]+)\s*\(", header)))
    assert declared == sorted(_lib.RESOLVE_EXPORTS) and len(declared) == 6
    L = ctypes.CDLL(_lib.LIB_PATH)       # loads without a GPU
    for name in declared:
        assert hasattr(L, name), f"{name} not exported by libpdhg_hip.so"
    assert len(_lib.EXPORTS) == 69 and not set(_lib.EXPORTS) & set(_lib.RESOLVE_EXPORTS)
    assert _lib.lib().pdhg_abi_version() == _lib.ABI_VERSION == 11
    for name in ("pdhg_resolve_retain", "pdhg_update_problem_vectors", "pdhg_warm_start"):      # no GPU is needed to be refused
        assert getattr(_lib.lib(), name)(None, *([None] * {"pdhg_resolve_retain": 0, "pdhg_update_problem_vectors": 4,
                                                           "pdhg_warm_start": 2}[name])) == -1
        assert b"null handle" in _lib.lib().pdhg_last_error()


# ---- optimize(..., initial_*) over the oracle ----

@pytest.mark.parametrize("name", sorted(_small_problems()))
def test_a_solve_from_its_own_solution_ends_at_once(name):
    """The average is empty at the first check, so it evaluates the current point: the starting point itself."""
    problem = _small_problems()[name]
    params = _params(tol=1e-8)
    cold = optimize(params, problem, OracleEngine.from_problem)
    assert cold.termination_reason == TerminationReason.TERMINATION_REASON_OPTIMAL and cold.iteration_count > 0
    warm = optimize(params, problem, OracleEngine.from_problem, initial_primal_solution=cold.primal_solution,
                    initial_dual_solution=cold.dual_solution)
    assert warm.termination_reason == TerminationReason.TERMINATION_REASON_OPTIMAL
    assert warm.iteration_count == 0
    # (the point went through one multiplication and one division by the rescaling factors: at most an ulp each)
    assert np.allclose(warm.primal_solution, cold.primal_solution, rtol=4e-16, atol=0)
    assert np.allclose(warm.dual_solution, cold.dual_solution, rtol=4e-16, atol=0)


def test_initial_points_are_checked_before_any_device_work():
    problem = H.example_lp()

    def factory(p):
        raise AssertionError("the engine was created")
    for kw in ({"initial_primal_solution": np.zeros(5)}, {"initial_dual_solution": np.zeros(2)},
               {"initial_primal_solution": np.array([0.0, np.nan, 0.0, 0.0])},
               {"initial_dual_solution": np.array([0.0, np.inf, 0.0])},
               {"initial_primal_solution": np.zeros(4), "initial_dual_solution": np.zeros((3, 1))}):
        with pytest.raises(ValueError):
            optimize(_params(), problem, factory, **kw)
    with pytest.raises(ValueError):
        optimize_many(_params(), [problem, problem], lambda ps: factory(ps), initial_solutions=[None])
    with pytest.raises(ValueError):
        optimize_many(_params(), [problem], lambda ps: factory(ps), initial_solutions=[(np.zeros(3), None)])


@pytest.mark.parametrize("name", ["example_lp", "example_qp"])
def test_no_initial_point_is_the_call_without_the_arguments(name):
    problem = _small_problems()[name]
    params = _params(limit=120)
    _assert_same(optimize(params, problem, OracleEngine.from_problem, None, None), optimize(params, problem, OracleEngine.from_problem))
    got = optimize_many(params, [problem], _ResolveOracleFleet, initial_solutions=[None])
    _assert_same(got[0], optimize(params, problem, OracleEngine.from_problem))


def test_optimize_many_takes_a_point_per_problem():
    problems = [H.example_lp(), H.example_qp(), random_lp(30, 30, 3, seed=1)]
    params = _params(limit=150)
    rng = np.random.default_rng(3)
    points = [(rng.uniform(0, 1, p.num_variables), rng.uniform(0, 1, p.num_constraints)) for p in problems]
    points[1] = None
    points[2] = (points[2][0], None)
    want = [optimize(params, p, OracleEngine.from_problem, *(pt or (None, None))) for p, pt in zip(problems, points)]
    got = optimize_many(params, problems, _ResolveOracleFleet, initial_solutions=points)
    for g, w in zip(got, want):
        _assert_same(g, w)


# ---- sessions over the oracle ----

def _update_of(problem):
    """A new right-hand side and one moved bound (still a feasible, bounded problem for the examples used here)."""
    b = problem.right_hand_side * 1.01 + 0.003
    ub = problem.variable_upper_bound.copy()
    ub[0] = ub[0] * 0.75 + 0.5 if np.isfinite(ub[0]) else 7.0
    return {"right_hand_side": b, "variable_upper_bound": ub}


_POLICIES = {"adaptive": AdaptiveStepsizeParams(0.3, 0.6), "constant": ConstantStepsizeParams(),
             "malitsky_pock": MalitskyPockStepsizeParameters(0.7, 0.99, 1.0)}


# (Malitsky and Pock's linesearch takes LPs only)
@pytest.mark.parametrize("name,policy_name", [(n, p) for n in ("example_lp", "dependent_rows", "example_qp") for p in _POLICIES
                                              if not (n == "example_qp" and p == "malitsky_pock")])
def test_a_session_cold_resolve_is_a_fresh_solve(name, policy_name):
    policy = _POLICIES[policy_name]
    problem = _small_problems()[name]
    params = _params(policy, limit=300, tol=1e-7)
    with PdhgSession(params, problem, ResolveOracleEngine.from_problem) as session:
        _assert_same(session.solve(), optimize(params, problem, OracleEngine.from_problem))
        update = _update_of(problem)
        session.update(**update)
        updated = dataclasses.replace(problem.copy(), **update)
        want = optimize(params, updated, OracleEngine.from_problem)
        _assert_same(session.solve(), want)
        # ... and warm, from a point and from the last solution
        x0, y0 = want.primal_solution * 0.9, want.dual_solution * 1.1
        _assert_same(session.solve(warm_start=(x0, y0)),
                     optimize(params, updated, OracleEngine.from_problem, initial_primal_solution=x0, initial_dual_solution=y0))
        last = session.solve()
        _assert_same(session.solve(warm_start=True),
                     optimize(params, updated, OracleEngine.from_problem, initial_primal_solution=last.primal_solution,
                              initial_dual_solution=last.dual_solution))


def test_a_fleet_session_is_optimize_per_problem():
    problems = [H.example_lp(), H.example_lp_dependent_rows(), H.example_qp(), random_lp(30, 30, 3, seed=1)]
    params = _params(limit=200, tol=1e-6, freq=7)
    with PdhgFleetSession(params, problems, _ResolveOracleFleet) as session:
        for g, p in zip(session.solve(), problems):
            _assert_same(g, optimize(params, p, OracleEngine.from_problem))
        updates = [_update_of(problems[0]), None, {"objective_vector": problems[2].objective_vector * 1.5}, _update_of(problems[3])]
        session.update(updates)
        updated = [p if u is None else dataclasses.replace(p.copy(), **u) for p, u in zip(problems, updates)]
        want = [optimize(params, p, OracleEngine.from_problem) for p in updated]
        got = session.solve()
        for g, w in zip(got, want):
            _assert_same(g, w)
        warm = [(want[0].primal_solution, want[0].dual_solution), None, (None, want[2].dual_solution), (want[3].primal_solution, None)]
        got = session.solve(warm_start=warm)
        for g, p, pt in zip(got, updated, warm):
            _assert_same(g, optimize(params, p, OracleEngine.from_problem, *(pt or (None, None))))
        last = session.solve()
        for g, p, w in zip(session.solve(warm_start=True), updated, last):
            _assert_same(g, optimize(params, p, OracleEngine.from_problem, w.primal_solution, w.dual_solution))


@pytest.mark.parametrize("bad", [{"variable_lower_bound": np.array([0.0, 0.0, 7.0, 0.0])},          # lb[2] = 7 > ub[2] = 6
                                 {"right_hand_side": np.array([12.0, np.nan, 1.0])},
                                 {"variable_lower_bound": np.array([0.0, np.inf, 0.0, 0.0])},
                                 {"objective_vector": np.zeros(3)}],
                         ids=["lb_above_ub", "nan_rhs", "inf_lb", "wrong_length"])
def test_an_update_that_fails_validation_leaves_the_session_as_it_was(bad):
    problem = H.example_lp()
    params = _params(limit=200)
    with PdhgSession(params, problem, ResolveOracleEngine.from_problem) as session:
        before = session.solve()
        calls = []
        session.engine.update_problem_vectors = lambda **kw: calls.append(kw)      # no device work may be reached
        with pytest.raises(ValueError):
            session.update(**bad)
        assert not calls
        del session.engine.update_problem_vectors
        _assert_same(session.solve(), before)
        assert np.array_equal(session.problem.right_hand_side, problem.right_hand_side)
    with pytest.raises(RuntimeError):
        session.solve()
