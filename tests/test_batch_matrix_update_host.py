"""New matrix values for a batch on its kept sparsity pattern, on the host: the export of
include/pdhg_hip_batch_matrix_update.h, and ``PdhgBatchSession.update_matrix`` over a batch of CPU oracle engines that
implement ``update_matrix_values`` by rebuilding their matrices (the engine of tests/test_matrix_update_host.py, restated)
-- a session's solve after such an update must be, field for field, ``optimize_batch`` on the updated problems over the
same oracle batch -- and the refusals, each of which leaves the session as it was and touches no engine."""
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
from firstorderlp_jl_amd.generators import random_lp, random_qp_family  # noqa: E402
from firstorderlp_jl_amd.primal_dual_hybrid_gradient import (AdaptiveStepsizeParams, ConstantStepsizeParams,  # noqa: E402
                                                             PdhgParameters)
from firstorderlp_jl_amd.quadratic_programming import linear_programming_problem  # noqa: E402
from firstorderlp_jl_amd.saddle_point import (RestartScheme, RestartToCurrentMetric,  # noqa: E402
                                              construct_restart_parameters)
from firstorderlp_jl_amd.termination import construct_termination_criteria  # noqa: E402
from tests.helpers import ResolveOracleEngine, assert_same_output as _assert_same, raises_naming as _raises_naming  # noqa: E402
from tests.oracle_engine import OracleEngine  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POLICIES = {"adaptive": AdaptiveStepsizeParams(0.3, 0.6), "constant": ConstantStepsizeParams()}
MATRIX_KEYS = ("constraint_matrix_values", "objective_matrix_values", "constraint_matrix", "objective_matrix")


def _params(policy=None, tol=1e-8, limit=60, freq=5):
    tc = construct_termination_criteria(eps_optimal_absolute=tol, eps_optimal_relative=tol, iteration_limit=limit)
    rp = construct_restart_parameters(RestartScheme.ADAPTIVE_NORMALIZED, RestartToCurrentMetric.GAP_OVER_DISTANCE_SQUARED,
                                      1000, 0.5, 0.1, 0.9, 0.5, False)
    return PdhgParameters(10, False, 1.0, 1.0, True, 0, True, freq, tc, rp, policy or POLICIES["adaptive"])


class MatrixOracleEngine(ResolveOracleEngine):
    """``ResolveOracleEngine`` with ``update_matrix_values``: the oracle has no setter for its matrices, so the call
    builds a new oracle state from matrices of the old pattern with the new values, in the engine's own problem's space
    (a factory without ``takes_original_problem``: the session hands it host-rescaled values and vectors)."""
    calls = 0

    def update_matrix_values(self, constraint_matrix_values, objective_matrix_values, objective_vector, right_hand_side,
                             variable_lower_bound, variable_upper_bound):
        MatrixOracleEngine.calls += 1
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

    def update_problem_vectors(self, **vectors):
        MatrixOracleEngine.calls += 1
        super().update_problem_vectors(**vectors)


class _OracleBatch:
    """The batch interface of HipPdhgBatch over K oracle engines (trial_step / accept per active member); it has none of
    the batch's own re-solve calls, so a session serves it member by member."""
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


class _MatrixOracleBatch(_OracleBatch):
    engine = MatrixOracleEngine


class _VectorsOnlyBatch(_OracleBatch):
    engine = ResolveOracleEngine                 # (no update_matrix_values)


def _lp_family(K=3):
    p = random_lp(27, 32, 4, seed=1)
    rng = np.random.default_rng(2)
    out = []
    for k in range(K):
        c = p.objective_vector * (1.0 + 0.5 * rng.random(32)) if k else p.objective_vector.copy()
        b = p.right_hand_side * (1.0 + 0.05 * rng.random(27)) if k else p.right_hand_side.copy()
        out.append(linear_programming_problem(p.variable_lower_bound.copy(), p.variable_upper_bound + k, c, 0.0,
                                              p.constraint_matrix, b, p.num_equalities))
    return out


FAMILIES = {"lp": _lp_family, "qp": lambda: random_qp_family(27, 32, 2, seed=3, nnz_per_row=4)}


def _new_values(matrix, seed):
    rng = np.random.default_rng(seed)
    return matrix.data * (1.0 + 0.1 * rng.uniform(-1, 1, matrix.nnz))


def _matrix_update(problems, seed):
    """New values of A; of a QP family's Q one factor (it stays symmetric positive definite)."""
    update = {"constraint_matrix_values": _new_values(problems[0].constraint_matrix, seed)}
    if problems[0].objective_matrix.nnz:
        update["objective_matrix_values"] = problems[0].objective_matrix.data * 1.07
    return update


def _applied(problems, update, vectors=None):
    out = []
    for k, p in enumerate(problems):
        changes = dict((vectors or [None] * len(problems))[k] or {})
        for field in ("constraint_matrix", "objective_matrix"):
            if field + "_values" in update:
                old = getattr(p, field)
                changes[field] = sp.csc_matrix((update[field + "_values"], old.indices, old.indptr), shape=old.shape)
        out.append(dataclasses.replace(p.copy(), **changes))
    return out


def _assert_all_same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        _assert_same(g, w)


def _points(problems, seed):
    rng = np.random.default_rng(seed)
    return [(rng.uniform(0, 1, p.num_variables), rng.standard_normal(p.num_constraints)) for p in problems]


# ---- the export ----

def test_the_header_declares_exactly_the_new_export_and_the_library_has_it():
    header = open(os.path.join(ROOT, "include", "pdhg_hip_batch_matrix_update.h")).read()
    declared = sorted(set(re.findall(r"\b(pdhg_[a-z_0-9]+)\s*\(", header)))
    assert declared == sorted(_lib.BATCH_MATRIX_UPDATE_EXPORTS) == ["pdhg_batch_update_matrix_values"]
    L = ctypes.CDLL(_lib.LIB_PATH)       # loads without a GPU
    assert hasattr(L, "pdhg_batch_update_matrix_values")
    # the lists the existing tests pin are as they were
    assert len(_lib.EXPORTS) == 69 and len(_lib.RESOLVE_EXPORTS) == 6 and len(_lib.BATCH_RESOLVE_EXPORTS) == 4
    assert _lib.MATRIX_UPDATE_EXPORTS == ["pdhg_update_matrix_values"]
    assert _lib.lib().pdhg_abi_version() == _lib.ABI_VERSION == 11
    for name in ("pdhg_hip.h", "pdhg_hip_resolve.h", "pdhg_hip_batch_resolve.h", "pdhg_hip_matrix_update.h"):
        other = open(os.path.join(ROOT, "include", name)).read()
        assert "pdhg_batch_update_matrix_values" not in re.findall(r"\b(pdhg_[a-z_0-9]+)\s*\(", other), name


def test_a_null_handle_is_refused_without_a_gpu():
    L = _lib.lib()
    assert L.pdhg_batch_update_matrix_values(None, 0, None, 0, None, None, None, None, None) == -1
    assert b"null handle" in L.pdhg_last_error()


# ---- the session's logic over the oracle ----

@pytest.mark.parametrize("policy", sorted(POLICIES))
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_update_matrix_then_solve_is_optimize_batch_on_the_updated_problems(family, policy):
    problems = FAMILIES[family]()
    params = _params(POLICIES[policy])
    update = _matrix_update(problems, seed=3)
    updated = _applied(problems, update)
    with PdhgBatchSession(params, problems, _MatrixOracleBatch) as session:
        session.solve()
        session.update_matrix(**update)
        for got, want in zip(session.problems, updated):
            assert np.array_equal(got.constraint_matrix.data, want.constraint_matrix.data)
            assert np.array_equal(got.objective_matrix.data, want.objective_matrix.data)
        _assert_all_same(session.solve(), optimize_batch(params, updated, batch_factory=_OracleBatch))
        # warm, from points and from the last solutions
        points = _points(updated, seed=5)
        points[-1] = (points[-1][0], None)
        got = session.solve(warm_start=points)
        _assert_all_same(got, optimize_batch(params, updated, batch_factory=_OracleBatch, initial_solutions=points))
        last = [(g.primal_solution, g.dual_solution) for g in got]
        _assert_all_same(session.solve(warm_start=True),
                         optimize_batch(params, updated, batch_factory=_OracleBatch, initial_solutions=last))


@pytest.mark.parametrize("policy", sorted(POLICIES))
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_vector_updates_of_the_members_ride_the_same_call(family, policy):
    problems = FAMILIES[family]()
    K = len(problems)
    params = _params(POLICIES[policy])
    update = _matrix_update(problems, seed=6)
    ub = problems[0].variable_upper_bound.copy()
    ub[::5] = np.where(np.isfinite(ub[::5]), ub[::5] * 1.25, 12.0)
    vectors = [{"right_hand_side": problems[0].right_hand_side * 1.01, "variable_upper_bound": ub}] + [None] * (K - 2) + \
              [{"objective_vector": problems[-1].objective_vector * 0.9}]
    updated = _applied(problems, update, vectors)
    whole = updated[0].constraint_matrix.tocsr()               # (canonicalised like the problems')
    as_matrix = {"constraint_matrix": whole}
    if "objective_matrix_values" in update:
        as_matrix["objective_matrix"] = updated[0].objective_matrix
    for matrix in (update, as_matrix):
        with PdhgBatchSession(params, problems, _MatrixOracleBatch) as session:
            session.update_matrix(updates=vectors, **matrix)
            assert np.array_equal(session.problems[0].right_hand_side, updated[0].right_hand_side)
            assert np.array_equal(session.problems[-1].objective_vector, updated[-1].objective_vector)
            _assert_all_same(session.solve(), optimize_batch(params, updated, batch_factory=_OracleBatch))
            points = _points(updated, seed=7)
            _assert_all_same(session.solve(warm_start=points),
                             optimize_batch(params, updated, batch_factory=_OracleBatch, initial_solutions=points))
            # two updates in a row with a vector-only update between them, then back: the first problems again
            session.update_matrix(**_matrix_update(problems, seed=8))
            session.update([{k: getattr(p, k) for k in ("objective_vector", "right_hand_side", "variable_lower_bound",
                                                        "variable_upper_bound")} for p in problems])
            back = {"constraint_matrix_values": problems[0].constraint_matrix.data}
            if "objective_matrix_values" in update:
                back["objective_matrix_values"] = problems[0].objective_matrix.data
            session.update_matrix(**back)
            _assert_all_same(session.solve(), optimize_batch(params, problems, batch_factory=_OracleBatch))


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_the_constant_policys_estimate_is_computed_again(family):
    problems = FAMILIES[family]()
    params = _params(POLICIES["constant"])
    # (entry by entry: the rescaling undoes one factor for all of them, and the scaled matrix's norm would stay)
    A = problems[0].constraint_matrix
    update = {"constraint_matrix_values": A.data * np.random.default_rng(11).uniform(0.2, 3.0, A.nnz)}
    if problems[0].objective_matrix.nnz:
        update["objective_matrix_values"] = problems[0].objective_matrix.data * 2.0
    updated = _applied(problems, update)

    def power_method(outputs):
        """(number_of_power_iterations -- the KKT passes counted before the first step -- and the step size it gave)"""
        assert all(o.iteration_stats[0].iteration_number == 0 for o in outputs)
        return [(o.iteration_stats[0].cumulative_kkt_matrix_passes, o.iteration_stats[0].step_size) for o in outputs]

    with PdhgBatchSession(params, problems, _MatrixOracleBatch) as session:
        first = session.solve()
        session.update_matrix(**update)
        second = session.solve()
        want = optimize_batch(params, updated, batch_factory=_OracleBatch)
        _assert_all_same(second, want)
        assert power_method(second) == power_method(want)
        assert all(a[1] != b[1] for a, b in zip(power_method(first), power_method(second)))      # (a kept estimate would show)
        # ... and once per matrix: a vector update keeps it
        session.update([{"right_hand_side": updated[0].right_hand_side * 1.01}] + [None] * (len(problems) - 1))
        _assert_all_same(session.solve(), optimize_batch(params, session.problems, batch_factory=_OracleBatch))


# ---- refusals on the host: the session is as it was ----

def _other_pattern(A):
    """``A`` with its last stored entry moved to a row its column does not hold yet; returns (matrix, that column)."""
    A = sp.csc_matrix(A, copy=True)
    column = int(np.searchsorted(A.indptr, A.nnz - 1, side="right")) - 1
    held = set(A.indices[A.indptr[column]:A.indptr[column + 1]].tolist())
    A.indices[A.nnz - 1] = next(r for r in range(A.shape[0] - 1, -1, -1) if r not in held)
    A.has_sorted_indices = False
    return A, column


def test_host_refusals_leave_the_session_as_it_was_and_touch_no_engine():
    params = _params()
    lps, qps = FAMILIES["lp"](), FAMILIES["qp"]()
    A = lps[0].constraint_matrix
    nnz = A.nnz

    with PdhgBatchSession(params, lps, _MatrixOracleBatch) as session:
        want = session.solve()
        MatrixOracleEngine.calls = 0
        bad_nan = A.data.copy()
        bad_nan[3] = np.nan
        other, column = _other_pattern(A)
        good = A.data * 1.1
        _raises_naming(ValueError, [f"column {column} "], lambda: session.update_matrix(constraint_matrix=other))
        _raises_naming(ValueError, ["NaN"], lambda: session.update_matrix(constraint_matrix_values=bad_nan))
        _raises_naming(ValueError, ["shape"], lambda: session.update_matrix(constraint_matrix_values=np.ones(nnz + 1)))
        _raises_naming(ValueError, ["not both"], lambda: session.update_matrix(constraint_matrix_values=good, constraint_matrix=A))
        _raises_naming(ValueError, ["without an objective matrix"], lambda: session.update_matrix(objective_matrix_values=np.ones(0)))
        # a good matrix with a bad vector of the last member: nothing of the update is applied, to any member
        _raises_naming(ValueError, ["above"], lambda: session.update_matrix(
            constraint_matrix_values=good, updates=[{"right_hand_side": lps[0].right_hand_side * 2}, None,
                                                    {"variable_lower_bound": np.full(32, 50.0), "variable_upper_bound": np.full(32, 1.0)}]))
        _raises_naming(ValueError, ["entries"], lambda: session.update_matrix(constraint_matrix_values=good, updates=[None, None]))
        _raises_naming(ValueError, ["needs new values"], lambda: session.update_matrix(updates=[None, None, None]))
        # the matrix keys stay out of the per-member dicts, here and in update
        for key, value in zip(MATRIX_KEYS, (good, np.ones(0), A, lps[0].objective_matrix)):
            _raises_naming(ValueError, ["batch session"], lambda: session.update_matrix(constraint_matrix_values=good,
                                                                                        updates=[None, {key: value}, None]))
            _raises_naming(ValueError, ["batch session"], lambda: session.update([{"right_hand_side": lps[0].right_hand_side * 2},
                                                                                  {key: value}, None]))
        assert MatrixOracleEngine.calls == 0
        for got, p in zip(session.problems, lps):
            assert np.array_equal(got.constraint_matrix.data, p.constraint_matrix.data)
            assert np.array_equal(got.right_hand_side, p.right_hand_side)
        _assert_all_same(session.solve(), want)

    with PdhgBatchSession(params, qps, _MatrixOracleBatch) as session:
        want = session.solve()
        MatrixOracleEngine.calls = 0
        q_nnz = qps[0].objective_matrix.nnz
        _raises_naming(ValueError, ["all zero"], lambda: session.update_matrix(objective_matrix_values=np.zeros(q_nnz)))
        _raises_naming(ValueError, ["shape"], lambda: session.update_matrix(objective_matrix_values=np.ones(q_nnz + 2)))
        assert MatrixOracleEngine.calls == 0
        _assert_all_same(session.solve(), want)

    # engines without update_matrix_values, on a batch that has none either
    with PdhgBatchSession(params, lps, _VectorsOnlyBatch) as session:
        want = session.solve()
        touched = []
        for eng in session.batch.members:
            eng.update_problem_vectors = lambda *a, **k: touched.append(1)
        _raises_naming(ValueError, ["update_matrix_values"], lambda: session.update_matrix(
            constraint_matrix_values=A.data * 1.1, updates=[{"right_hand_side": lps[0].right_hand_side * 2}, None, None]))
        assert not touched
        for eng in session.batch.members:
            del eng.update_problem_vectors
        assert np.array_equal(session.problems[0].constraint_matrix.data, A.data)
        assert np.array_equal(session.problems[0].right_hand_side, lps[0].right_hand_side)
        _assert_all_same(session.solve(), want)
    _raises_naming(RuntimeError, ["closed"], lambda: session.update_matrix(constraint_matrix_values=A.data))

    # a batch whose engines live in the original space (it rescales them together on the device) and that offers no
    # update_matrix_values for all of them: nothing could rescale the members together again.  (The oracle batch is
    # turned into one by its members' flag: no engine of that kind exists outside the library.)
    with PdhgBatchSession(params, lps, _MatrixOracleBatch) as session:
        want = session.solve()
        MatrixOracleEngine.calls = 0
        for mb in session._held:
            mb.on_device = True
        _raises_naming(ValueError, ["rescales on the device"], lambda: session.update_matrix(constraint_matrix_values=A.data * 1.1))
        for mb in session._held:
            mb.on_device = False
        assert MatrixOracleEngine.calls == 0
        assert np.array_equal(session.problems[0].constraint_matrix.data, A.data)
        _assert_all_same(session.solve(), want)
