"""New matrix values on a kept sparsity pattern, on the host: the export of include/pdhg_hip_matrix_update.h, and
``PdhgSession.update(constraint_matrix_values=...)`` over an oracle engine that implements ``update_matrix_values`` by
rebuilding its matrices -- a session's solve after such an update must be, bit for bit, ``optimize`` on the updated
problem -- and the refusals, each of which leaves the session as it was."""
import ctypes
import dataclasses
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import folp_loader

folp = folp_loader.load()
from firstorderlp_jl_amd import PdhgBatchSession, PdhgFleetSession, PdhgSession, _lib  # noqa: E402
from firstorderlp_jl_amd.generators import random_lp  # noqa: E402
from firstorderlp_jl_amd.primal_dual_hybrid_gradient import (AdaptiveStepsizeParams, ConstantStepsizeParams,  # noqa: E402
                                                             MalitskyPockStepsizeParameters, PdhgParameters, optimize)
from firstorderlp_jl_amd.saddle_point import (RestartScheme, RestartToCurrentMetric,  # noqa: E402
                                              construct_restart_parameters)
from firstorderlp_jl_amd.termination import construct_termination_criteria  # noqa: E402
from tests import helpers as H  # noqa: E402
from tests.helpers import ResolveOracleEngine, assert_same_output as _assert_same, raises_naming as _raises_naming  # noqa: E402
from tests.oracle_engine import OracleEngine  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

POLICIES = {"adaptive": AdaptiveStepsizeParams(0.3, 0.6), "constant": ConstantStepsizeParams(),
            "malitsky_pock": MalitskyPockStepsizeParameters(0.7, 0.99, 1.0)}


def _params(policy=None, tol=1e-8, limit=150, freq=5):
    tc = construct_termination_criteria(eps_optimal_absolute=tol, eps_optimal_relative=tol, iteration_limit=limit)
    rp = construct_restart_parameters(RestartScheme.ADAPTIVE_NORMALIZED, RestartToCurrentMetric.GAP_OVER_DISTANCE_SQUARED,
                                      1000, 0.5, 0.1, 0.9, 0.5, False)
    return PdhgParameters(10, False, 1.0, 1.0, True, 0, True, freq, tc, rp, policy or POLICIES["adaptive"])


class MatrixOracleEngine(ResolveOracleEngine):
    """``ResolveOracleEngine`` with ``update_matrix_values``: the oracle has no setter for its matrices, so the call
    builds a new oracle state from matrices of the old pattern with the new values, in the engine's own problem's space
    (a factory without ``takes_original_problem``: the session hands it host-rescaled values and vectors)."""

    def update_matrix_values(self, constraint_matrix_values, objective_matrix_values, objective_vector, right_hand_side,
                             variable_lower_bound, variable_upper_bound):
        A = sp.csc_matrix(self._A)
        assert np.shape(constraint_matrix_values) == A.data.shape
        self._A = sp.csc_matrix((np.array(constraint_matrix_values, dtype=np.float64), A.indices, A.indptr), shape=A.shape)
        if objective_matrix_values is not None:
            Q = sp.csc_matrix(self._Qm)
            assert np.shape(objective_matrix_values) == Q.data.shape
            self._Qm = sp.csc_matrix((np.array(objective_matrix_values, dtype=np.float64), Q.indices, Q.indptr), shape=Q.shape)
        self._vectors = [np.array(v, dtype=np.float64) for v in (objective_vector, right_hand_side, variable_lower_bound,
                                                                 variable_upper_bound)]
        self._rebuild()


class _MatrixOracleFleet:
    def __init__(self, problems):
        self.members = [MatrixOracleEngine.from_problem(p) for p in problems]

    def close(self):
        for eng in self.members:
            eng.close()


def _problems():
    return {"example_lp": H.example_lp(), "example_qp": H.example_qp(), "random_lp": random_lp(27, 32, 4, seed=1)}


def _new_values(matrix, seed):
    rng = np.random.default_rng(seed)
    return matrix.data * (1.0 + 0.1 * rng.uniform(-1, 1, matrix.nnz))


def _with_values(problem, a_values=None, q_values=None):
    changes = {}
    for field, values in (("constraint_matrix", a_values), ("objective_matrix", q_values)):
        if values is not None:
            old = getattr(problem, field)
            changes[field] = sp.csc_matrix((values, old.indices, old.indptr), shape=old.shape)
    return dataclasses.replace(problem.copy(), **changes)


# ---- the export ----

def test_the_header_declares_exactly_the_matrix_update_exports_and_the_library_has_them():
    header = open(os.path.join(ROOT, "include", "pdhg_hip_matrix_update.h")).read()
    declared = sorted(set(re.findall(r"\b(pdhg_[a-z_0-9]+)\s*\(", header)))
    assert declared == sorted(_lib.MATRIX_UPDATE_EXPORTS) == ["pdhg_update_matrix_values"]
    L = ctypes.CDLL(_lib.LIB_PATH)       # loads without a GPU
    for name in declared:
        assert hasattr(L, name), f"{name} not exported by libpdhg_hip.so"
    assert len(_lib.EXPORTS) == 69 and len(_lib.RESOLVE_EXPORTS) == 6 and len(_lib.BATCH_RESOLVE_EXPORTS) == 4
    assert not set(_lib.MATRIX_UPDATE_EXPORTS) & set(_lib.EXPORTS + _lib.RESOLVE_EXPORTS + _lib.BATCH_RESOLVE_EXPORTS)
    assert _lib.lib().pdhg_abi_version() == _lib.ABI_VERSION == 11
    assert _lib.lib().pdhg_update_matrix_values(None, 0, None, 0, None, None, None, None, None) == -1      # no GPU is needed to be refused
    assert b"null handle" in _lib.lib().pdhg_last_error()


# ---- the session's logic over the oracle ----

@pytest.mark.parametrize("policy", sorted(POLICIES))
@pytest.mark.parametrize("name", sorted(_problems()))
def test_a_solve_after_new_matrix_values_is_optimize_on_the_updated_problem(name, policy):
    problem = _problems()[name]
    params = _params(POLICIES[policy])
    is_qp = problem.objective_matrix.nnz > 0
    a_new = _new_values(problem.constraint_matrix, seed=3)
    q_new = _new_values(problem.objective_matrix, seed=4) if is_qp else None
    updated = _with_values(problem, a_new, q_new)
    rng = np.random.default_rng(5)
    x0, y0 = rng.uniform(0, 1, problem.num_variables), rng.standard_normal(problem.num_constraints)
    with PdhgSession(params, problem, MatrixOracleEngine.from_problem) as session:
        if is_qp and policy == "malitsky_pock":
            # the linesearch is for LPs only (pdhg.jl:555-647): the session says so exactly as optimize does, also after
            # an update
            session.update(constraint_matrix_values=a_new, objective_matrix_values=q_new)
            _raises_naming(ValueError, ["only supported for linear programming"], session.solve)
            _raises_naming(ValueError, ["only supported for linear programming"],
                           lambda: optimize(params, updated, OracleEngine.from_problem))
            return
        session.solve()
        session.update(constraint_matrix_values=a_new, **({"objective_matrix_values": q_new} if is_qp else {}))
        assert np.array_equal(session.problem.constraint_matrix.data, a_new)
        _assert_same(session.solve(), optimize(params, updated, OracleEngine.from_problem))
        _assert_same(session.solve(warm_start=(x0, y0)),
                     optimize(params, updated, OracleEngine.from_problem, initial_primal_solution=x0, initial_dual_solution=y0))


def test_values_and_vectors_in_one_update_and_a_whole_matrix_of_the_same_pattern():
    problem = _problems()["random_lp"]
    params = _params()
    a_new = _new_values(problem.constraint_matrix, seed=6)
    b_new = problem.right_hand_side * 1.01
    updated = dataclasses.replace(_with_values(problem, a_new), right_hand_side=b_new)
    with PdhgSession(params, problem, MatrixOracleEngine.from_problem) as session:
        session.update(constraint_matrix=updated.constraint_matrix.tocsr(), right_hand_side=b_new)      # (canonicalised like the problem's)
        _assert_same(session.solve(), optimize(params, updated, OracleEngine.from_problem))


def test_explicit_zeros_among_the_new_values_stay_stored_entries():
    problem = _problems()["random_lp"]
    a_new = _new_values(problem.constraint_matrix, seed=7)
    a_new[::5] = 0.0
    with PdhgSession(_params(), problem, MatrixOracleEngine.from_problem) as session:
        session.update(constraint_matrix_values=a_new)
        A = session.problem.constraint_matrix
        assert A.nnz == problem.constraint_matrix.nnz and np.array_equal(A.indices, problem.constraint_matrix.indices)
        session.update(constraint_matrix_values=problem.constraint_matrix.data)          # the pattern is still there to be filled
        _assert_same(session.solve(), optimize(_params(), problem, OracleEngine.from_problem))


@pytest.mark.parametrize("name", ["example_qp", "random_lp"])
def test_two_updates_in_a_row_then_back_reproduces_the_first_solve(name):
    problem = _problems()[name]
    params = _params(limit=90)
    A = problem.constraint_matrix
    with PdhgSession(params, problem, MatrixOracleEngine.from_problem) as session:
        first = session.solve()
        session.update(constraint_matrix_values=_new_values(A, seed=8))
        session.update(constraint_matrix_values=_new_values(A, seed=9))
        second = session.solve()
        assert not np.array_equal(second.primal_solution, first.primal_solution)
        session.update(constraint_matrix_values=A.data)
        _assert_same(session.solve(), first)


def test_a_fleet_session_serves_matrix_updates_member_by_member():
    problems = [H.example_lp(), H.example_qp(), random_lp(27, 32, 4, seed=1), random_lp(20, 24, 3, seed=2)]
    params = _params(limit=80)
    a_new = [_new_values(p.constraint_matrix, seed=10 + k) for k, p in enumerate(problems)]
    updates = [{"constraint_matrix_values": a_new[0]}, None, {"right_hand_side": problems[2].right_hand_side * 1.02},
               {"constraint_matrix_values": a_new[3], "objective_vector": problems[3].objective_vector * 0.9}]
    updated = [_with_values(problems[0], a_new[0]), problems[1],
               dataclasses.replace(problems[2].copy(), right_hand_side=problems[2].right_hand_side * 1.02),
               dataclasses.replace(_with_values(problems[3], a_new[3]), objective_vector=problems[3].objective_vector * 0.9)]
    with PdhgFleetSession(params, problems, _MatrixOracleFleet) as session:
        session.solve()
        session.update(updates)
        for got, p in zip(session.solve(), updated):
            _assert_same(got, optimize(params, p, OracleEngine.from_problem))


# ---- refusals on the host: the session is as it was ----

def _other_pattern(A):
    """``A`` with its last stored entry moved to a row its column does not hold yet; returns (matrix, that column)."""
    A = sp.csc_matrix(A, copy=True)
    column = int(np.searchsorted(A.indptr, A.nnz - 1, side="right")) - 1
    held = set(A.indices[A.indptr[column]:A.indptr[column + 1]].tolist())
    A.indices[A.nnz - 1] = next(r for r in range(A.shape[0] - 1, -1, -1) if r not in held)
    A.has_sorted_indices = False
    return A, column


def test_host_refusals_leave_the_session_as_it_was():
    lp, qp = _problems()["random_lp"], H.example_qp()
    params = _params(limit=60)

    class Counting(MatrixOracleEngine):
        calls = 0

        def update_matrix_values(self, *a):
            Counting.calls += 1
            super().update_matrix_values(*a)

    with PdhgSession(params, lp, Counting.from_problem) as session:
        want = session.solve()
        nnz = lp.constraint_matrix.nnz
        bad_nan = lp.constraint_matrix.data.copy()
        bad_nan[3] = np.nan
        other, column = _other_pattern(lp.constraint_matrix)
        _raises_naming(ValueError, ["shape"], lambda: session.update(constraint_matrix_values=np.ones(nnz + 1)))
        _raises_naming(ValueError, ["NaN"], lambda: session.update(constraint_matrix_values=bad_nan))
        _raises_naming(ValueError, ["without an objective matrix"], lambda: session.update(objective_matrix_values=np.ones(0)))
        _raises_naming(ValueError, [f"column {column} "], lambda: session.update(constraint_matrix=other))
        fewer = sp.csc_matrix(lp.constraint_matrix, copy=True)
        fewer.data[0] = 0.0
        fewer.eliminate_zeros()
        _raises_naming(ValueError, ["column 0 "], lambda: session.update(constraint_matrix=fewer))
        _raises_naming(ValueError, ["not both"], lambda: session.update(constraint_matrix_values=np.ones(nnz), constraint_matrix=lp.constraint_matrix))
        # a good matrix with a bad vector: nothing of the update is applied
        _raises_naming(ValueError, ["above"], lambda: session.update(constraint_matrix_values=np.ones(nnz),
                                                                     variable_lower_bound=np.full(32, 5.0),
                                                                     variable_upper_bound=np.full(32, 1.0)))
        assert Counting.calls == 0
        assert np.array_equal(session.problem.constraint_matrix.data, lp.constraint_matrix.data)
        _assert_same(session.solve(), want)

    with PdhgSession(params, qp, Counting.from_problem) as session:
        want = session.solve()
        _raises_naming(ValueError, ["all zero"], lambda: session.update(objective_matrix_values=np.zeros(qp.objective_matrix.nnz)))
        _raises_naming(ValueError, ["shape"], lambda: session.update(objective_matrix_values=np.ones(qp.objective_matrix.nnz + 2)))
        assert Counting.calls == 0
        _assert_same(session.solve(), want)


def test_a_batch_session_refuses_matrix_values_before_any_device_work():
    base = random_lp(27, 32, 4, seed=1)
    family = [base, dataclasses.replace(base.copy(), objective_vector=base.objective_vector * 2)]

    class Batch:
        def __init__(self, problems):
            self.members = [MatrixOracleEngine.from_problem(p) for p in problems]

        def close(self):
            for eng in self.members:
                eng.close()

    params = _params(limit=60)
    with PdhgBatchSession(params, family, Batch) as session:
        touched = []
        for eng in session.batch.members:
            eng.update_problem_vectors = eng.update_matrix_values = lambda *a, **k: touched.append(1)
        values = base.constraint_matrix.data * 1.1
        for key, value in (("constraint_matrix_values", values), ("objective_matrix_values", np.ones(0)),
                           ("constraint_matrix", base.constraint_matrix), ("objective_matrix", base.objective_matrix)):
            _raises_naming(ValueError, ["batch session"], lambda: session.update([{"right_hand_side": base.right_hand_side * 2}, {key: value}]))
        assert not touched
        for p, q in zip(session.problems, family):
            assert np.array_equal(p.right_hand_side, q.right_hand_side)
        # (the keys are looked at before anything is staged: the good vector update beside them was not applied either)
        session.update([{"right_hand_side": base.right_hand_side * 2}, None])
        assert len(touched) == 1
