"""New matrix values on a kept sparsity pattern, on the device (include/pdhg_hip_matrix_update.h, csrc/abi_matrix_update.hpp,
csrc/matrix_update_kernels.hpp, firstorderlp.jl_amd/session.py).

* placement: after ``update_matrix_values`` every device array of every layout holds, bit for bit, what a fresh engine
  created from the updated problem in the same environment holds -- the 32 layout checksums, the problem vectors and
  the two products (which read the sliced jagged copies the checksums do not see) -- in every layout of
  ``tests/test_gpu_property.py`` and as row segments, on patterns with every search length and both ends of a
  searched run, a row of two full long-row chunks and a tail, and the degenerate shapes;
* the same after the rescaling that follows, at 0, 1 and 12 steps, and after a second update (the record is reset);
* a session's cold or warm solve after such an update is ``optimize`` on the updated problem, on every step path;
* a fleet session serves matrix updates member by member beside the shared vector launch; refusals launch nothing.

Every comparison is bitwise.  PDHG_TUNE=0 throughout: no timing at create, so two engines of one pattern make the
same choices."""
import ctypes
import dataclasses

import numpy as np
import pytest
import scipy.sparse as sp

from firstorderlp_jl_amd import (HipPdhgBatch, HipPdhgEngine, PdhgFleetSession, PdhgSession, _lib,
                                 linear_programming_problem, optimize_many)
from firstorderlp_jl_amd.engine import _MemberEngine
from firstorderlp_jl_amd.generators import random_lp, random_qp_family
from firstorderlp_jl_amd.primal_dual_hybrid_gradient import (AdaptiveStepsizeParams, ConstantStepsizeParams,
                                                             MalitskyPockStepsizeParameters, PdhgParameters, optimize)
from firstorderlp_jl_amd.quadratic_programming import QuadraticProgrammingProblem
from firstorderlp_jl_amd.saddle_point import (RestartScheme, RestartToCurrentMetric,
                                              construct_restart_parameters)
from firstorderlp_jl_amd.termination import construct_termination_criteria
from tests.helpers import (assert_same_output as _assert_same, bits as _bits, raises_naming as _raises_naming,
                           same_bits as _same_bits)

pytestmark = pytest.mark.gpu

RESCALINGS = {0: (0, False, None), 1: (1, False, None), 12: (10, True, 1.0)}      # applied steps -> (Ruiz, L2, Pock-Chambolle alpha)

# the layout table of tests/test_gpu_property.py::_engine (the single-handle entries), and row segments
LAYOUTS = {"default": {},
           "stream_nograph": {"PDHG_SPMV": "stream", "PDHG_GRAPH": "0"},
           "pipe": {"PDHG_SPMV": "stream", "PDHG_STREAM_PIPE": "1"},
           "slabs": {"PDHG_SPMV": "stream", "PDHG_SLABS": "1", "PDHG_SLAB_MB": "0.00005"},
           "sj_narrow": {"PDHG_SPMV": "stream", "PDHG_SJ": "1", "PDHG_SJ_WIDE": "0"},
           "sj_wide": {"PDHG_SPMV": "stream", "PDHG_SJ": "1", "PDHG_SJ_WIDE": "1"},
           "sj_hub": {"PDHG_SPMV": "stream", "PDHG_SJ": "1", "PDHG_SJ_MAXLEN": "3"},
           "tiled6": {"PDHG_SPMV": "tiled", "PDHG_TILE_SHIFT": "6"},
           "tiled8": {"PDHG_SPMV": "tiled", "PDHG_TILE_SHIFT": "8"},
           "tiled_cols96": {"PDHG_SPMV": "tiled", "PDHG_TILE_COLS": "96"},
           "tiled_var": {"PDHG_SPMV": "tiled", "PDHG_TILE_COLS": "64", "PDHG_VAR_TILES": "1"},
           # the layouts built on the device (the builders of large matrices), also under the sweep and as segments
           "device": {"PDHG_DEVICE_LAYOUT": "1"},
           "device_tiled6": {"PDHG_DEVICE_LAYOUT": "1", "PDHG_SPMV": "tiled", "PDHG_TILE_SHIFT": "6"},
           "segments": {"PDHG_MAX_SHARD_NNZ": None},                      # nnz // 4, set per problem
           "device_segments": {"PDHG_DEVICE_LAYOUT": "1", "PDHG_MAX_SHARD_NNZ": None}}
# ("slabs" is restated as it stands there; at these sizes the builders decline column slabs, which need a million
#  entries: test_column_slabs_take_the_new_values below builds them)
_LAYOUT_KEYS = sorted({k for env in LAYOUTS.values() for k in env})


@pytest.fixture(autouse=True)
def _no_tuning(monkeypatch):
    monkeypatch.setenv("PDHG_TUNE", "0")


def _layout_env(monkeypatch, layout, nnz):
    for k in _LAYOUT_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in LAYOUTS[layout].items():
        monkeypatch.setenv(k, str(max(1, nnz // 4)) if v is None else v)


# ---- patterns ----

def _edges_mask():
    """70 x 200: an empty row, an empty column, rows of 1, 63, 64 and 65 entries (the wave stride), columns of 1, 2 and
    65 entries (search lengths; both ends of a searched column are looked up), the rest at density 0.15."""
    rng = np.random.default_rng(70200)
    mask = rng.random((70, 200)) < 0.15
    mask[:, :4] = False
    mask[10, 1] = True                         # a column of one entry
    mask[[10, 69], 2] = True                   # ... of two
    mask[5:70, 3] = True                       # ... of 65: rows 5 and 69 are the ends of the searched run
    mask[:5, :] = False
    for row, count in ((1, 1), (2, 63), (3, 64), (4, 65)):
        mask[row, 4 + rng.choice(196, size=count, replace=False)] = True
    assert mask[0].sum() == 0 and mask[:, 0].sum() == 0
    assert [int(mask[r].sum()) for r in (1, 2, 3, 4)] == [1, 63, 64, 65]
    assert [int(mask[:, c].sum()) for c in (1, 2, 3)] == [1, 2, 65]
    return mask


def _long_row_mask():
    """30 x 4 100 with one dense row: two full 2 048-entry chunks and a tail in CSR(A), a hub of 30-entry columns for the
    transpose lookup."""
    rng = np.random.default_rng(304100)
    mask = rng.random((30, 4100)) < 0.15
    mask[7, :] = True
    return mask


def _masks():
    long_row = _long_row_mask()
    return {"edges": _edges_mask(), "long_row": long_row, "long_column": long_row.T.copy(),      # a 4 100-entry column: a 12-step search
            "no_entries": np.zeros((3, 4), dtype=bool), "no_rows": np.zeros((0, 5), dtype=bool), "one_by_one": np.ones((1, 1), dtype=bool)}


MASKS = _masks()


def _distinct_values(nnz, seed):
    """Every value distinct (k + 0.5 with random signs, shuffled), so that two swapped entries change a checksum."""
    rng = np.random.default_rng(seed)
    return rng.permutation(np.arange(nnz) + 0.5) * rng.choice([-1.0, 1.0], nnz)


def _pattern(mask):
    A = sp.csc_matrix(mask.astype(np.float64))
    A.sort_indices()
    return A.indices.astype(np.int64), A.indptr.astype(np.int64)


def _problem(name, seed, values=None, Q=None):
    """The LP (or, with ``Q``, QP) of pattern ``name`` with vectors drawn from ``seed``; ``values``: the matrix's stored
    values in CSC order (default: distinct ones drawn from ``seed``)."""
    mask = MASKS[name]
    m, n = mask.shape
    indices, indptr = _pattern(mask)
    rng = np.random.default_rng(seed)
    if values is None:
        values = _distinct_values(len(indices), seed)
    A = sp.csc_matrix((values, indices, indptr), shape=(m, n))
    lb = np.where(rng.random(n) < 0.25, -np.inf, rng.integers(-2, 1, n).astype(float))
    ub = np.where(rng.random(n) < 0.4, np.inf, np.maximum(lb, 0.0) + rng.integers(0, 3, n))
    c, b = rng.standard_normal(n), rng.standard_normal(m)
    if Q is None:
        return linear_programming_problem(lb, ub, c, 0.0, A, b, m // 3)
    return QuadraticProgrammingProblem(lb, ub, Q, c, 0.0, A, b, m // 3)


def _vectors(p):
    return p.objective_vector, p.right_hand_side, p.variable_lower_bound, p.variable_upper_bound


def _update(eng, p):
    q = p.objective_matrix.data if p.objective_matrix.nnz else None
    eng.update_matrix_values(p.constraint_matrix.data, q, *_vectors(p))


def _probe_vectors(p):
    rng = np.random.default_rng(p.num_variables + 7 * p.num_constraints)
    return rng.standard_normal(p.num_variables), rng.standard_normal(p.num_constraints)


def _assert_same_device_state(got, want, p, layout, label, rescaled=None):
    """``got`` and ``want``: two engines of one pattern in one environment."""
    _same_bits(got.get_problem_vectors(), want.get_problem_vectors(), label)
    if not layout.endswith("segments") or max(p.constraint_matrix.nnz // 4, 1) >= p.constraint_matrix.nnz:
        a, b = got.layout_checksums(), want.layout_checksums()            # (not defined for a matrix held as row segments)
        assert np.array_equal(a, b), (label, np.nonzero(a != b)[0])
    else:
        assert got.layout_describe()["A"]["segments"] > 1 and got.layout_describe()["At"]["segments"] > 1, label
    x, y = _probe_vectors(p)
    assert np.array_equal(_bits(got.spmv(x)), _bits(want.spmv(x))), f"{label}: A x"
    assert np.array_equal(_bits(got.spmv_t(y)), _bits(want.spmv_t(y))), f"{label}: A' y"
    if rescaled is not None:
        (E_got, D_got), (E_want, D_want) = rescaled
        assert np.array_equal(_bits(E_got), _bits(E_want)) and np.array_equal(_bits(D_got), _bits(D_want)), f"{label}: E, D"
        assert _bits(got.matrix_max_abs()) == _bits(want.matrix_max_abs()), f"{label}: max |a|"


def _retained(p):
    eng = HipPdhgEngine.from_problem(p)
    eng.retain_rescaling()
    return eng


def _trial_bits(eng, point, step=0.3, weight=1.1):
    eng.set_current(*point)
    raw = eng.trial_step(step, weight, 1.0)
    return [_bits(raw)] + [_bits(v) for v in eng.get_trial()]


# ---- placement in every layout ----

@pytest.mark.parametrize("name", sorted(MASKS))
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_every_copy_holds_the_new_values(gpu_required, monkeypatch, layout, name):
    old, new = _problem(name, seed=1), _problem(name, seed=2)
    _layout_env(monkeypatch, layout, old.constraint_matrix.nnz)
    got, want = _retained(old), _retained(new)
    try:
        _update(got, new)
        _assert_same_device_state(got, want, new, layout, f"{layout} {name}")
    finally:
        got.close()
        want.close()


def test_the_layout_describe_key_names(gpu_required, monkeypatch):
    """(what ``_assert_same_device_state`` reads for the segments layout)"""
    p = _problem("edges", seed=1)
    _layout_env(monkeypatch, "segments", p.constraint_matrix.nnz)
    eng = _retained(p)
    try:
        d = eng.layout_describe()
        assert d["A"]["segments"] >= 4 and d["At"]["segments"] >= 4, d
    finally:
        eng.close()


def _scattered_lp(seed):
    """49 152 x 49 152 with 23 scattered entries per row: over a million entries and 1.5 slab widths (of a quarter MiB)
    of gathered vector, the smallest at which both copies are built as column slabs."""
    n = 49152
    rng = np.random.default_rng(49152)                           # (the pattern: the same for every seed)
    cols = rng.integers(0, n, size=(n, 23))
    A = sp.csr_matrix((np.ones(cols.size), cols.reshape(-1), np.arange(0, cols.size + 1, 23)), shape=(n, n)).tocsc()
    A.sum_duplicates()
    A.sort_indices()
    A.data = _distinct_values(A.nnz, seed)
    rng = np.random.default_rng(seed)
    return linear_programming_problem(np.zeros(n), np.full(n, np.inf), rng.standard_normal(n), 0.0, A, rng.standard_normal(n), n // 3)


@pytest.mark.short_rows
@pytest.mark.parametrize("sliced_jagged", ["0", "1"])
def test_column_slabs_take_the_new_values(gpu_required, monkeypatch, sliced_jagged):
    for k in _LAYOUT_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in {"PDHG_SPMV": "stream", "PDHG_SLABS": "2", "PDHG_SLAB_MB": "0.25", "PDHG_SJ": sliced_jagged}.items():
        monkeypatch.setenv(k, v)
    old, new = _scattered_lp(seed=1), _scattered_lp(seed=2)
    assert old.constraint_matrix.nnz >= 1 << 20
    got, want = _retained(old), _retained(new)
    try:
        info = got.layout_info()
        assert info["A_slabs"] >= 2 and info["At_slabs"] >= 2, info
        _update(got, new)
        _assert_same_device_state(got, want, new, "slabs", "column slabs")
        rescaled = got.rescale(*RESCALINGS[12]), want.rescale(*RESCALINGS[12])
        _assert_same_device_state(got, want, new, "slabs", "column slabs rescaled", rescaled)
    finally:
        got.close()
        want.close()


def _edges_qp(seed, scale=1.0):
    rng = np.random.default_rng(99)
    B = sp.random(40, 200, density=0.05, format="csc", random_state=np.random.RandomState(5), data_rvs=rng.standard_normal)
    Q = sp.csc_matrix(B.T @ B + sp.diags(np.linspace(0.5, 2.0, 200)))
    Q.sort_indices()
    q_values = _distinct_values(Q.nnz, seed + 100) * scale
    return _problem("edges", seed, Q=sp.csc_matrix((q_values, Q.indices, Q.indptr), shape=Q.shape))


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_the_objective_matrix_takes_new_values_too(gpu_required, monkeypatch, layout):
    old, new = _edges_qp(seed=1), _edges_qp(seed=2)
    _layout_env(monkeypatch, layout, old.constraint_matrix.nnz)
    got, want = _retained(old), _retained(new)
    try:
        _update(got, new)
        _assert_same_device_state(got, want, new, layout, f"{layout} qp")
        point = _probe_vectors(new)
        for g, w in zip(_trial_bits(got, point), _trial_bits(want, point)):
            assert np.array_equal(g, w), layout
        for steps in (12,):
            rescaled = got.rescale(*RESCALINGS[steps]), want.rescale(*RESCALINGS[steps])
            _assert_same_device_state(got, want, new, layout, f"{layout} qp rescaled", rescaled)
            for g, w in zip(_trial_bits(got, point), _trial_bits(want, point)):
                assert np.array_equal(g, w), layout
    finally:
        got.close()
        want.close()


@pytest.mark.parametrize("layout", ["default", "sj_narrow", "tiled6", "device", "segments"])
def test_zeros_of_both_signs_are_stored_as_given(gpu_required, monkeypatch, layout):
    old = _problem("edges", seed=1)
    values = _distinct_values(old.constraint_matrix.nnz, seed=3)
    values[::7] = 0.0
    values[3::11] = -0.0
    A = sp.csc_matrix((values, old.constraint_matrix.indices, old.constraint_matrix.indptr), shape=old.constraint_matrix.shape)
    _layout_env(monkeypatch, layout, old.constraint_matrix.nnz)
    got = _retained(old)
    want = HipPdhgEngine(A, *_vectors(old), old.num_equalities)         # (from the arrays themselves: nothing canonicalises them)
    try:
        assert np.array_equal(_bits(A.data), _bits(values)) and np.signbit(A.data[3])
        got.update_matrix_values(values, None, *_vectors(old))
        _assert_same_device_state(got, want, old, layout, f"{layout} zeros")
    finally:
        got.close()
        want.close()


# ---- after the rescale ----

@pytest.mark.parametrize("steps", sorted(RESCALINGS))
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_the_rescale_after_an_update_is_a_fresh_rescale(gpu_required, monkeypatch, layout, steps):
    for name in ("edges", "long_row"):
        old, new, newer = (_problem(name, seed=s) for s in (1, 2, 3))
        _layout_env(monkeypatch, layout, old.constraint_matrix.nnz)
        got, want, want2 = _retained(old), _retained(new), _retained(newer)
        try:
            got.rescale(*RESCALINGS[steps])                  # the record holds the old matrix's steps
            _update(got, new)
            rescaled = got.rescale(*RESCALINGS[steps]), want.rescale(*RESCALINGS[steps])
            _assert_same_device_state(got, want, new, layout, f"{layout} {name} S={steps}", rescaled)
            # a second update on the same engine: the record was reset, not appended to
            _update(got, newer)
            rescaled = got.rescale(*RESCALINGS[steps]), want2.rescale(*RESCALINGS[steps])
            _assert_same_device_state(got, want2, newer, layout, f"{layout} {name} S={steps} second", rescaled)
            # ... and the replay of new vectors reads the new record
            other = _problem(name, seed=4)
            got.update_problem_vectors(*_vectors(other))
            want2.update_problem_vectors(*_vectors(other))
            _same_bits(got.get_problem_vectors(), want2.get_problem_vectors(), f"{layout} {name} S={steps} replay")
            fresh = HipPdhgEngine.from_problem(dataclasses.replace(newer.copy(), **dict(zip(
                ("objective_vector", "right_hand_side", "variable_lower_bound", "variable_upper_bound"), _vectors(other)))))
            try:
                fresh.rescale(*RESCALINGS[steps])
                _same_bits(got.get_problem_vectors(), fresh.get_problem_vectors(), f"{layout} {name} S={steps} replay against create")
            finally:
                fresh.close()
        finally:
            for eng in (got, want, want2):
                eng.close()


# ---- solves ----

def _params(policy=None, tol=1e-6, limit=64, freq=8):
    tc = construct_termination_criteria(eps_optimal_absolute=tol, eps_optimal_relative=tol, iteration_limit=limit)
    rp = construct_restart_parameters(RestartScheme.ADAPTIVE_NORMALIZED, RestartToCurrentMetric.GAP_OVER_DISTANCE_SQUARED,
                                      1000, 0.5, 0.1, 0.9, 0.5, False)
    return PdhgParameters(10, True, 1.0, 1.0, True, 0, True, freq, tc, rp, policy or AdaptiveStepsizeParams(0.3, 0.6))


def _medium():
    return random_lp(3000, 2500, 4, seed=2)


def _small_qp():
    return random_qp_family(40, 48, 1, seed=3, nnz_per_row=4)[0]


# restated from tests/test_gpu_resolve.py: name -> (environment, problem, what the session's engine must report
# afterwards: (steps_info, trial_graph) -> bool)
PATHS = {"small_lp": ({}, lambda: random_lp(27, 32, 4, seed=1), lambda si, tg: si[0] > 0),
         "small_lp_off": ({"PDHG_SMALL_LP": "0"}, lambda: random_lp(27, 32, 4, seed=1), lambda si, tg: si[0] == 0),
         "steps_kernel": ({"PDHG_DEVICE_LOOP": "1", "PDHG_SMALL_LP": "0"}, _medium, lambda si, tg: si[0] == 0 and si[1] > 0 and tg == 2),
         "device_loop_off": ({"PDHG_DEVICE_LOOP": "0", "PDHG_SMALL_LP": "0"}, _medium, lambda si, tg: si[:2] == [0, 0] and tg == 2),
         "graph": ({"PDHG_DEVICE_LOOP": "0", "PDHG_COOP": "0", "PDHG_SMALL_LP": "0"}, _medium, lambda si, tg: si[:2] == [0, 0] and tg == 1),
         "qp": ({}, _small_qp, lambda si, tg: si[0] == 0),
         "small_qp": ({"PDHG_SMALL_QP": "1"}, _small_qp, lambda si, tg: si[0] > 0)}


def _matrix_update(problem, seed=0):
    """Every stored value of A times 1 + 0.01 N(0, 1); a QP's Q times 1.05 (it stays symmetric positive semidefinite)."""
    rng = np.random.default_rng(seed)
    A = problem.constraint_matrix
    update = {"constraint_matrix_values": A.data * (1.0 + 0.01 * rng.standard_normal(A.nnz))}
    if problem.objective_matrix.nnz:
        update["objective_matrix_values"] = problem.objective_matrix.data * 1.05
    return update


def _applied(problem, update):
    changes = {k: v for k, v in update.items() if not k.endswith("_values")}
    for field in ("constraint_matrix", "objective_matrix"):
        if field + "_values" in update:
            old = getattr(problem, field)
            changes[field] = sp.csc_matrix((update[field + "_values"], old.indices, old.indptr), shape=old.shape)
    return dataclasses.replace(problem.copy(), **changes)


def _series(params, problem, warm_points=()):
    """solve; update the matrix values; solve cold (and warm from each of ``warm_points``) against ``optimize`` on the
    updated problem.  Returns the session engine's (steps_info, trial_graph)."""
    update = _matrix_update(problem)
    updated = _applied(problem, update)
    with PdhgSession(params, problem) as session:
        session.solve()
        session.update(**update)
        _assert_same(session.solve(), optimize(params, updated))
        for x0, y0 in warm_points:
            _assert_same(session.solve(warm_start=(x0, y0)),
                         optimize(params, updated, initial_primal_solution=x0, initial_dual_solution=y0))
        return session.engine.steps_info(), session.engine.layout_info()["trial_graph"]


@pytest.mark.short_rows
@pytest.mark.parametrize("path", sorted(PATHS))
def test_a_solve_after_new_matrix_values_is_a_fresh_solve_on_every_step_path(gpu_required, monkeypatch, path):
    env, maker, took_the_path = PATHS[path]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    problem = maker()
    rng = np.random.default_rng(9)
    point = (rng.uniform(0, 1, problem.num_variables), rng.standard_normal(problem.num_constraints))
    steps_info, trial_graph = _series(_params(), problem, warm_points=[point])
    assert took_the_path(steps_info, trial_graph), (path, steps_info, trial_graph)


@pytest.mark.short_rows
@pytest.mark.parametrize("policy", [AdaptiveStepsizeParams(0.3, 0.6), ConstantStepsizeParams(), MalitskyPockStepsizeParameters(0.7, 0.99, 1.0)],
                         ids=["adaptive", "constant", "malitsky_pock"])
def test_every_step_size_policy(gpu_required, policy):
    rng = np.random.default_rng(10)
    _series(_params(policy), random_lp(27, 32, 4, seed=1), warm_points=[(rng.uniform(0, 1, 32), rng.standard_normal(27))])


@pytest.mark.short_rows
@pytest.mark.parametrize("maker", [lambda: random_lp(27, 32, 4, seed=1), _small_qp, _medium], ids=["small_lp", "qp", "medium"])
def test_an_update_and_the_update_back_leave_no_state(gpu_required, maker):
    problem = maker()
    params = _params()
    back = {"constraint_matrix_values": problem.constraint_matrix.data}
    if problem.objective_matrix.nnz:
        back["objective_matrix_values"] = problem.objective_matrix.data
    with PdhgSession(params, problem) as session:
        first = session.solve()
        session.update(**_matrix_update(problem, seed=4))
        assert not np.array_equal(session.solve().primal_solution, first.primal_solution)
        session.update(**_matrix_update(problem, seed=5))
        session.update(**back)
        _assert_same(session.solve(), first)
    _assert_same(first, optimize(params, problem))


@pytest.mark.short_rows
def test_the_host_rescale_route_hands_scaled_values_to_the_same_call(gpu_required, monkeypatch):
    monkeypatch.setenv("PDHG_HOST_RESCALE", "1")
    for problem in (random_lp(27, 32, 4, seed=1), _small_qp()):
        params = _params()
        update = _matrix_update(problem, seed=6)
        with PdhgSession(params, problem) as session:
            session.solve()
            session.update(**update)
            _assert_same(session.solve(), optimize(params, _applied(problem, update)))


# ---- a fleet ----

@pytest.mark.short_rows
def test_a_fleet_session_serves_matrix_updates_beside_the_shared_vector_launch(gpu_required):
    problems = [random_lp(27, 32, 4, seed=1), random_lp(40, 30, 3, seed=2), _small_qp(), random_lp(300, 260, 4, seed=3),
                random_lp(20, 24, 3, seed=4)]
    params = _params(limit=40)
    b2 = problems[2].right_hand_side * 1.02
    b3 = problems[3].right_hand_side * 0.98
    updates = [_matrix_update(problems[0], seed=1), _matrix_update(problems[1], seed=2), {"right_hand_side": b2},
               dict(_matrix_update(problems[3], seed=3), right_hand_side=b3), None]
    updated = [p if u is None else _applied(p, u) for p, u in zip(problems, updates)]
    with PdhgFleetSession(params, problems) as session:
        session.solve()
        launches = session.fleet.resolve_info()["shared_launches"]
        session.update(updates)
        info = session.fleet.resolve_info()
        assert info["shared_launches"] == launches + 1 and info["carried"] == 1, info      # the vector-only member rode it
        for got, want in zip(session.solve(), optimize_many(params, updated)):
            _assert_same(got, want)
        for got, p in zip(session.solve(), updated):
            _assert_same(got, optimize(params, p))


# ---- refusals ----

def _raw_update(eng, nnz, values, q_nnz, q_values, c, b, lb, ub):
    dp = ctypes.POINTER(ctypes.c_double)
    keep = [None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in (values, q_values, c, b, lb, ub)]
    args = [None if a is None else a.ctypes.data_as(dp) for a in keep]          # (``keep`` outlives the call)
    rc = _lib.lib().pdhg_update_matrix_values(eng._h, nnz, args[0], q_nnz, *args[1:])
    return rc, _lib.lib().pdhg_last_error().decode()


def _refused(eng, words, *args):
    rc, message = _raw_update(eng, *args)
    assert rc == -1 and any(w in message for w in words), (rc, message)


@pytest.mark.short_rows
def test_refusals_launch_nothing_and_leave_the_handle_usable(gpu_required, monkeypatch):
    monkeypatch.setenv("PDHG_SMALL_LP", "0")          # (trial_step through the ordinary kernels)
    problem = random_lp(27, 32, 4, seed=1)
    A = problem.constraint_matrix
    c, b, lb, ub = _vectors(problem)
    rng = np.random.default_rng(3)
    point = (rng.uniform(0, 1, 32), rng.standard_normal(27))
    good = (A.nnz, A.data * 1.5, 0, None, c, b, lb, ub)

    def usable_as_before(eng, before, label):
        _same_bits(eng.get_problem_vectors(), before[0], label)
        for g, w in zip(_trial_bits(eng, point), before[1]):
            assert np.array_equal(g, w), label

    eng = HipPdhgEngine.from_problem(problem)
    try:
        eng.rescale(*RESCALINGS[12])
        before = eng.get_problem_vectors(), _trial_bits(eng, point)
        _refused(eng, ["pdhg_resolve_retain"], *good)
        usable_as_before(eng, before, "not retained")
    finally:
        eng.close()
    _raises_naming(_lib.PdhgHipError, ["closed"], lambda: eng.update_matrix_values(A.data, None, c, b, lb, ub))

    eng = _retained(problem)
    try:
        eng.rescale(*RESCALINGS[12])
        before = eng.get_problem_vectors(), _trial_bits(eng, point)
        _refused(eng, ["nnz"], A.nnz - 1, A.data[:-1], 0, None, c, b, lb, ub)
        _refused(eng, ["nzval"], A.nnz, None, 0, None, c, b, lb, ub)
        for k in range(4):
            vectors = [c, b, lb, ub]
            vectors[k] = None
            _refused(eng, ["all needed"], A.nnz, A.data, 0, None, *vectors)
        _refused(eng, ["without an objective matrix"], A.nnz, A.data, 3, np.ones(3), c, b, lb, ub)
        _raises_naming(ValueError, ["entries"], lambda: eng.update_matrix_values(A.data, None, c[:-1], b, lb, ub))
        usable_as_before(eng, before, "bad arguments")
    finally:
        eng.close()

    qp = _small_qp()
    eng = _retained(qp)
    try:
        before = eng.get_problem_vectors(), _trial_bits(eng, (np.ones(qp.num_variables), np.ones(qp.num_constraints)))
        QA = qp.constraint_matrix
        _refused(eng, ["q_nzval == NULL"], QA.nnz, QA.data, 0, None, *_vectors(qp))
        _refused(eng, ["q_nnz"], QA.nnz, QA.data, qp.objective_matrix.nnz - 1, qp.objective_matrix.data[:-1], *_vectors(qp))
        _same_bits(eng.get_problem_vectors(), before[0], "qp")
        for g, w in zip(_trial_bits(eng, (np.ones(qp.num_variables), np.ones(qp.num_constraints))), before[1]):
            assert np.array_equal(g, w)
    finally:
        eng.close()

    group = HipPdhgEngine.from_problem(problem, device_ids=[0, 0])
    try:
        before = group.get_problem_vectors(), _trial_bits(group, point)
        _refused(group, ["shard group"], *good)
        usable_as_before(group, before, "shard group")
    finally:
        group.close()

    family = [problem, dataclasses.replace(problem.copy(), objective_vector=problem.objective_vector * 2)]
    batch = HipPdhgBatch.from_problems(family)
    try:
        batch.retain_rescaling()
        whole = _MemberEngine._wrap(batch._L, batch._h, batch.m, batch.n)          # (a view: the batch frees the handle)
        before = batch.members[0].get_problem_vectors()
        _refused(whole, ["batch handle"], *good)
        _refused(batch.members[0], ["batch member"], *good)
        _same_bits(batch.members[0].get_problem_vectors(), before, "batch member")
        assert batch.members[0].steps_info() == [0, 0, 0, 0]
    finally:
        batch.close()


@pytest.mark.short_rows
def test_a_handle_created_from_unsorted_or_duplicate_columns_is_refused(gpu_required):
    """``pdhg_create`` keeps such columns in the caller's order; the placement searches need ascending runs, so the
    update refuses the handle (the one refusal that looks at the device: a read-only pass) and leaves it usable."""
    m, n = 6, 4
    c, b, lb, ub = np.ones(n), np.ones(m), np.zeros(n), np.full(n, 5.0)
    point = (np.linspace(0.1, 1, n), np.linspace(-1, 1, m))
    cases = {"unsorted": (np.array([0, 2, 4, 5, 7]), np.array([3, 1, 0, 2, 5, 1, 4])),
             "duplicate": (np.array([0, 2, 4, 5, 7]), np.array([1, 1, 0, 2, 5, 1, 4])),
             "sorted": (np.array([0, 2, 4, 5, 7]), np.array([1, 3, 0, 2, 5, 1, 4]))}
    for label, (indptr, indices) in cases.items():
        values = np.arange(7) + 1.5
        A = sp.csc_matrix((values, indices, indptr), shape=(m, n))
        assert np.array_equal(A.indices, indices)               # (nothing sorted or summed them)
        eng = HipPdhgEngine(A, c, b, lb, ub, 2)
        try:
            eng.retain_rescaling()
            before = eng.get_problem_vectors(), _trial_bits(eng, point)
            if label == "sorted":
                eng.update_matrix_values(values[::-1].copy(), None, c, b, lb, ub)
                want = HipPdhgEngine(sp.csc_matrix((values[::-1].copy(), indices, indptr), shape=(m, n)), c, b, lb, ub, 2)
                try:
                    assert np.array_equal(eng.layout_checksums(), want.layout_checksums())
                finally:
                    want.close()
                continue
            for _ in range(2):                                  # (the second call is answered from the remembered look)
                _refused(eng, ["ascend"], 7, values * 2, 0, None, c, b, lb, ub)
            _same_bits(eng.get_problem_vectors(), before[0], label)
            for g, w in zip(_trial_bits(eng, point), before[1]):
                assert np.array_equal(g, w), label
        finally:
            eng.close()


# ---- untouched callers ----

@pytest.mark.short_rows
def test_a_session_that_never_updates_its_matrix_is_as_before(gpu_required):
    for problem in (random_lp(27, 32, 4, seed=1), _medium()):
        params = _params()
        fresh = HipPdhgEngine.from_problem(problem)
        try:
            describe = fresh.layout_describe()
        finally:
            fresh.close()
        with PdhgSession(params, problem) as session:
            eng = session.engine
            assert [eng.layout_describe()[k] for k in ("A", "At", "bounds")] == [describe[k] for k in ("A", "At", "bounds")]
            got = session.solve()
            steps_info = eng.steps_info()
            session.update(right_hand_side=problem.right_hand_side)
            _assert_same(session.solve(), got)
            assert eng.steps_info()[:2] == [2 * v for v in steps_info[:2]]       # the same launches again
        _assert_same(got, optimize(params, problem))
