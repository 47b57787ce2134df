"""optimize_many on the host: the driver's logic through ``fleet_factory`` -- a fleet adapter over K CPU oracle engines
must give exactly what K runs of ``optimize(..., engine_factory=OracleEngine...)`` give, for problems of different
shapes that end for different reasons, under every step-size policy -- its argument check, and the four exports."""
import ctypes
import dataclasses
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import folp_loader

folp = folp_loader.load()
from firstorderlp_jl_amd import _lib, optimize_many  # noqa: E402
from firstorderlp_jl_amd.generators import random_lp  # noqa: E402
from firstorderlp_jl_amd.primal_dual_hybrid_gradient import (AdaptiveStepsizeParams, ConstantStepsizeParams,  # noqa: E402
                                                             MalitskyPockStepsizeParameters, PdhgParameters, optimize)
from firstorderlp_jl_amd.quadratic_programming import linear_programming_problem  # noqa: E402
from firstorderlp_jl_amd.saddle_point import (RestartScheme, RestartToCurrentMetric,  # noqa: E402
                                              construct_restart_parameters)
from firstorderlp_jl_amd.termination import construct_termination_criteria  # noqa: E402
from tests import helpers as H  # noqa: E402
from tests.oracle_engine import OracleEngine  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLEET_EXPORTS = ("pdhg_create_fleet", "pdhg_fleet_add", "pdhg_fleet_take_steps_adaptive", "pdhg_fleet_info")


def _params(policy, tol=1e-6, limit=400, freq=7):
    tc = construct_termination_criteria(eps_optimal_absolute=tol, eps_optimal_relative=tol, iteration_limit=limit)
    rp = construct_restart_parameters(RestartScheme.ADAPTIVE_NORMALIZED, RestartToCurrentMetric.GAP_OVER_DISTANCE_SQUARED,
                                      1000, 0.5, 0.1, 0.9, 0.5, False)
    return PdhgParameters(10, False, 1.0, 1.0, True, 0, True, freq, tc, rp, policy)


def _problems():
    """Different shapes, different ends: two that reach optimality (4 x 5 and 3 x 4, at different iterations), a 3 x 3
    one whose rows contradict each other (x0 + x1 = 1 and x0 + x1 >= 2: found infeasible after some tens of
    iterations), and a 30 x 30 one that is still on its way at the iteration limit."""
    A = sp.csc_matrix(np.array([[1.0, 1.0, 1.0, 0.0, 2.0], [1.0, -1.0, 0.0, 0.5, 0.0], [0.0, 2.0, -1.0, 1.0, 1.0],
                                [3.0, 0.0, 1.0, 0.0, -1.0]]))
    first = linear_programming_problem(np.zeros(5), np.full(5, 10.0), np.array([1.0, 2.0, 0.5, 1.0, 3.0]), 0.0, A,
                                       np.array([1.0, 0.0, -1.0, 0.5]), 1)
    bad = linear_programming_problem(np.zeros(3), np.full(3, 10.0), np.array([1.0, 2.0, 1.0]), 0.0,
                                     sp.csc_matrix(np.array([[1.0, 1.0, 0.0], [1.0, 1.0, 0.0], [0.0, 1.0, 1.0]])),
                                     np.array([1.0, 2.0, 1.0]), 1)
    return [first, H.example_lp_dependent_rows(), bad, random_lp(30, 30, 3, seed=1)]


class _OracleFleet:
    """What optimize_many needs of a fleet, over oracle engines: ``members`` and ``close`` -- no native multi-step call,
    so every member is stepped through ``take_steps``."""

    def __init__(self, problems):
        self.members = [OracleEngine.from_problem(p) for p in problems]

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


@pytest.mark.parametrize("policy", [AdaptiveStepsizeParams(0.3, 0.6), ConstantStepsizeParams(),
                                    MalitskyPockStepsizeParameters(0.7, 1.0, 0.9)],
                         ids=["adaptive", "constant", "malitsky_pock"])
def test_optimize_many_is_optimize_per_problem(policy):
    problems = _problems()
    params = _params(policy)
    want = [optimize(params, p, OracleEngine.from_problem) for p in problems]
    got = optimize_many(params, problems, fleet_factory=_OracleFleet)
    assert len(got) == len(problems)
    for g, w in zip(got, want):
        _assert_same(g, w)
    reasons = [w.termination_string for w in want]
    assert reasons == ["OPTIMAL", "OPTIMAL", "PRIMAL_INFEASIBLE", "ITERATION_LIMIT"], reasons
    assert want[0].iteration_count != want[1].iteration_count and want[2].iteration_count > 1


def test_an_empty_list_is_refused_before_any_device_work(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("a library call was made")
    monkeypatch.setattr(_lib, "lib", refuse)

    def factory(ps):
        raise AssertionError("the fleet was created")
    factory.takes_original_problem = True
    with pytest.raises(ValueError):
        optimize_many(_params(AdaptiveStepsizeParams(0.3, 0.6)), [], fleet_factory=factory)
    with pytest.raises(ValueError):
        optimize_many(_params(AdaptiveStepsizeParams(0.3, 0.6)), [])


def test_the_fleet_exports_are_declared_and_built():
    header = open(os.path.join(ROOT, "include", "pdhg_hip.h")).read()
    declared = set(re.findall(r"\b(pdhg_[a-z_0-9]+)\s*\(", header))
    L = ctypes.CDLL(_lib.LIB_PATH)       # loads without a GPU
    for name in FLEET_EXPORTS:
        assert name in _lib.EXPORTS, name
        assert name in declared, name
        assert hasattr(L, name), f"{name} not exported by libpdhg_hip.so"
    assert _lib.lib().pdhg_abi_version() == 11
