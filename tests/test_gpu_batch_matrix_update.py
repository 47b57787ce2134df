"""New matrix values for a batch on its kept sparsity pattern, on the device (include/pdhg_hip_batch_matrix_update.h,
csrc/abi_batch_matrix_update.hpp, ``HipPdhgBatch.update_matrix_values``, ``PdhgBatchSession.update_matrix``).

* placement and rescale: after ``update_matrix_values`` and the ``rescale`` that must follow it the batch holds, bit for
  bit, what a fresh retained batch created from the updated problems in the same environment and rescaled the same way
  holds -- the 32 layout checksums (read through member 0: a member's layouts are the batch handle's device arrays), the
  rescaling factors, every member's four vectors and two products, one trial of all members -- on the patterns and in
  the layouts of tests/test_gpu_matrix_update.py (restated), at K = 1, 3 (one padded lane) and 32, at 0, 1 and 12
  rescaling steps, update after update on one batch;
* the rescale of a batch that awaits it ends in ONE replay launch that carries all K members;
* between the update and the rescale every other call is refused and changes nothing;
* a session's cold or warm solve after ``update_matrix`` is ``optimize_batch`` on the updated problems;
* the refusals of the C call launch nothing and change nothing.

Every comparison is bitwise.  PDHG_TUNE=0 throughout: no timing at create, so two batches of one pattern make the same
choices."""
import dataclasses

import numpy as np
import pytest
import scipy.sparse as sp

from firstorderlp_jl_amd import (HipPdhgBatch, HipPdhgEngine, HipPdhgFleet, PdhgBatchSession, _lib,
                                 linear_programming_problem, optimize_batch)
from firstorderlp_jl_amd.generators import random_lp, random_qp_family
from firstorderlp_jl_amd.primal_dual_hybrid_gradient import (AdaptiveStepsizeParams, ConstantStepsizeParams,
                                                             PdhgParameters)
from firstorderlp_jl_amd.saddle_point import (RestartScheme, RestartToCurrentMetric,
                                              construct_restart_parameters)
from firstorderlp_jl_amd.termination import construct_termination_criteria
from tests.helpers import (assert_same_output as _assert_same, bits as _bits, raises_naming as _raises_naming,
                           same_bits as _same_bits)

pytestmark = pytest.mark.gpu

RESCALINGS = {0: (0, False, None), 1: (1, False, None), 12: (10, True, 1.0)}      # applied steps -> (Ruiz, L2, Pock-Chambolle alpha)
NAMES = ("objective_vector", "right_hand_side", "variable_lower_bound", "variable_upper_bound")
RESCALE_FIRST = ["rescale the batch first"]

# the layouts of tests/test_gpu_matrix_update.py that a batch can be held in (it refuses row segments)
LAYOUTS = {"default": {},
           "stream_nograph": {"PDHG_SPMV": "stream", "PDHG_GRAPH": "0"},
           "pipe": {"PDHG_SPMV": "stream", "PDHG_STREAM_PIPE": "1"},
           "sj_narrow": {"PDHG_SPMV": "stream", "PDHG_SJ": "1", "PDHG_SJ_WIDE": "0"},
           "sj_wide": {"PDHG_SPMV": "stream", "PDHG_SJ": "1", "PDHG_SJ_WIDE": "1"},
           "sj_hub": {"PDHG_SPMV": "stream", "PDHG_SJ": "1", "PDHG_SJ_MAXLEN": "3"},
           "tiled6": {"PDHG_SPMV": "tiled", "PDHG_TILE_SHIFT": "6"},
           "tiled_cols96": {"PDHG_SPMV": "tiled", "PDHG_TILE_COLS": "96"},
           "device": {"PDHG_DEVICE_LAYOUT": "1"}}
_LAYOUT_KEYS = sorted({k for env in LAYOUTS.values() for k in env} | {"PDHG_SLABS", "PDHG_SLAB_MB", "PDHG_TILE_SHIFT", "PDHG_VAR_TILES",
                                                                      "PDHG_MAX_SHARD_NNZ"})


@pytest.fixture(autouse=True)
def _no_tuning(monkeypatch):
    monkeypatch.setenv("PDHG_TUNE", "0")


def _layout_env(monkeypatch, layout):
    for k in _LAYOUT_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in LAYOUTS[layout].items():
        monkeypatch.setenv(k, v)


# ---- patterns (tests/test_gpu_matrix_update.py's, restated) ----

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
    """30 x 4 100 with one dense row: beyond both row orders' sequential limit (mu_long_kernel, the batch's chunk pair),
    a hub of 30-entry columns for the transpose lookup."""
    rng = np.random.default_rng(304100)
    mask = rng.random((30, 4100)) < 0.15
    mask[7, :] = True
    return mask


def _masks():
    long_row = _long_row_mask()
    return {"edges": _edges_mask(), "long_row": long_row, "long_column": long_row.T.copy(),      # a 4 100-entry column
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


def _member_vectors(m, n, rng):
    lb = np.where(rng.random(n) < 0.25, -np.inf, rng.integers(-2, 1, n).astype(float))
    ub = np.where(rng.random(n) < 0.4, np.inf, np.maximum(lb, 0.0) + rng.integers(0, 3, n))
    return lb, ub, rng.standard_normal(n), rng.standard_normal(m)


def _family_on(A, K, seed, num_eq, Q=None):
    """K problems on the matrix A (and Q) with vectors of their own, drawn from ``seed``."""
    m, n = A.shape
    rng = np.random.default_rng([int(seed), 17])
    out = []
    for _ in range(K):
        lb, ub, c, b = _member_vectors(m, n, rng)
        p = linear_programming_problem(lb, ub, c, 0.0, A, b, num_eq)
        out.append(p if Q is None else dataclasses.replace(p, objective_matrix=Q))
    return out


def _family(name, K, seed):
    """The LP family of pattern ``name``: distinct matrix values and K members' vectors, all drawn from ``seed``."""
    mask = MASKS[name]
    indices, indptr = _pattern(mask)
    A = sp.csc_matrix((_distinct_values(len(indices), seed), indices, indptr), shape=mask.shape)
    return _family_on(A, K, seed, mask.shape[0] // 3)


def _qp_family(K, seed):
    """``random_qp_family``'s 27 x 32 patterns of A and Q with distinct values drawn from ``seed`` (nothing is solved:
    Q need not be semidefinite here)."""
    base = random_qp_family(27, 32, 1, seed=3, nnz_per_row=4)[0]
    A0, Q0 = base.constraint_matrix, base.objective_matrix
    A = sp.csc_matrix((_distinct_values(A0.nnz, seed), A0.indices, A0.indptr), shape=A0.shape)
    Q = sp.csc_matrix((_distinct_values(Q0.nnz, seed + 100), Q0.indices, Q0.indptr), shape=Q0.shape)
    return _family_on(A, K, seed, base.num_equalities, Q=Q)


def _retained(problems):
    batch = HipPdhgBatch.from_problems(problems)
    try:
        batch.retain_rescaling()
    except Exception:
        batch.close()
        raise
    return batch


def _update(batch, problems):
    p0 = problems[0]
    q = p0.objective_matrix.data if p0.objective_matrix.nnz else None
    batch.update_matrix_values(p0.constraint_matrix.data, q, *[[getattr(p, name) for p in problems] for name in NAMES])


def _points(batch, seed):
    rng = np.random.default_rng(seed)
    return [(rng.standard_normal(batch.n), rng.standard_normal(batch.m)) for _ in range(batch.K)]


def _trial(batch, points):
    """One trial of all members from ``points``: the (K, 5) sums and every member's trial point, as bits."""
    for eng, point in zip(batch.members, points):
        eng.set_current(*point)
    raw = batch.trial_step(0.3, 1.1)
    return [_bits(raw)] + [_bits(v) for eng in batch.members for v in eng.get_trial()]


def _assert_same_batch(got, want, label, rescaled=None):
    """``got`` and ``want``: two batches of one pattern in one environment."""
    a, b = got.members[0].layout_checksums(), want.members[0].layout_checksums()
    assert np.array_equal(a, b), (label, np.nonzero(a != b)[0])
    points = _points(got, 5)
    for k, (g, w) in enumerate(zip(got.members, want.members)):
        _same_bits(g.get_problem_vectors(), w.get_problem_vectors(), f"{label} member {k}")
        x, y = points[k]
        assert np.array_equal(_bits(g.spmv(x)), _bits(w.spmv(x))), f"{label} member {k}: A x"
        assert np.array_equal(_bits(g.spmv_t(y)), _bits(w.spmv_t(y))), f"{label} member {k}: A' y"
    for q, (g, w) in enumerate(zip(_trial(got, points), _trial(want, points))):
        assert np.array_equal(g, w), f"{label}: trial, array {q}"
    if rescaled is not None:
        (E_got, D_got), (E_want, D_want) = rescaled
        assert np.array_equal(_bits(E_got), _bits(E_want)) and np.array_equal(_bits(D_got), _bits(D_want)), f"{label}: E, D"
        assert _bits(got.members[0].matrix_max_abs()) == _bits(want.members[0].matrix_max_abs()), f"{label}: max |a|"


def _updates_in_a_row(make_family, K, label):
    """One batch given new values again and again, rescaled by 12, 0, 1 and 12 steps: after each update + rescale it is
    the fresh retained batch of those problems rescaled the same way.  What is observed of the record: ``resolve_info``
    counts exactly one shared launch per update + rescale with ``carried == K`` -- the ABI exposes neither the record's
    step count nor its capacity -- and the members' vectors are the fresh batch's, which a record that grew from update
    to update could not give: its replay would apply the steps of the updates before as well."""
    got = _retained(make_family(K, 1))
    try:
        got.rescale(*RESCALINGS[12])                      # the record holds the first matrix's steps
        for round_, steps in enumerate((12, 0, 1, 12)):
            new = make_family(K, 2 + round_)
            launches = got.resolve_info()["shared_launches"]
            _update(got, new)
            assert got.resolve_info()["shared_launches"] == launches              # the replay is the rescale's
            factors = got.rescale(*RESCALINGS[steps])
            info = got.resolve_info()
            assert info["shared_launches"] == launches + 1 and info["carried"] == K and info["single"] == 0, info
            want = _retained(new)
            try:
                _assert_same_batch(got, want, f"{label} update {round_} S={steps}", (factors, want.rescale(*RESCALINGS[steps])))
            finally:
                want.close()
    finally:
        got.close()


# ---- placement and rescale ----

LONG = ("long_column", "long_row")            # a row of A or of A' beyond both row orders' sequential limit


@pytest.mark.short_rows
@pytest.mark.parametrize("K", [1, 3, 32])
@pytest.mark.parametrize("name", sorted(set(MASKS) - set(LONG)))
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_an_updated_and_rescaled_batch_is_a_fresh_one(gpu_required, monkeypatch, layout, name, K):
    _layout_env(monkeypatch, layout)
    _updates_in_a_row(lambda K, seed: _family(name, K, seed), K, f"{layout} {name} K={K}")


@pytest.mark.parametrize("K", [1, 3, 32])
@pytest.mark.parametrize("name", LONG)
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_an_updated_and_rescaled_batch_with_a_long_row_is_a_fresh_one(gpu_required, monkeypatch, layout, name, K):
    """(in both row orders: the placement's long-row kernel, the batch's chunk pair, the members' own long-row products)"""
    _layout_env(monkeypatch, layout)
    _updates_in_a_row(lambda K, seed: _family(name, K, seed), K, f"{layout} {name} K={K}")


@pytest.mark.short_rows
@pytest.mark.parametrize("K", [1, 3, 32])
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_the_objective_matrix_of_a_qp_batch_takes_new_values_too(gpu_required, monkeypatch, layout, K):
    """(the trial's five sums read every copy of Q and Q' the batch and its members multiply by)"""
    _layout_env(monkeypatch, layout)
    _updates_in_a_row(_qp_family, K, f"{layout} qp K={K}")
    # ... and a member's own trial, which multiplies by the member's (borrowed) layouts of Q
    old, new = _qp_family(2, 1), _qp_family(2, 2)
    got, want = _retained(old), _retained(new)
    try:
        _update(got, new)
        got.rescale(*RESCALINGS[12])
        want.rescale(*RESCALINGS[12])
        for g, w, point in zip(got.members, want.members, _points(got, 6)):
            for eng in (g, w):
                eng.set_current(*point)
            assert np.array_equal(_bits(g.trial_step(0.3, 1.1, 1.0)), _bits(w.trial_step(0.3, 1.1, 1.0)))
            for a, b in zip(g.get_trial(), w.get_trial()):
                assert np.array_equal(_bits(a), _bits(b))
    finally:
        got.close()
        want.close()


def _scattered_family(K, seed):
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
    return [linear_programming_problem(np.zeros(n), np.full(n, np.inf), rng.standard_normal(n), 0.0, A, rng.standard_normal(n), n // 3)
            for _ in range(K)]


@pytest.mark.short_rows
def test_column_slabs_take_the_new_values(gpu_required, monkeypatch):
    for k in _LAYOUT_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in {"PDHG_SPMV": "stream", "PDHG_SLABS": "2", "PDHG_SLAB_MB": "0.25", "PDHG_SJ": "0"}.items():
        monkeypatch.setenv(k, v)
    old, new = _scattered_family(2, seed=1), _scattered_family(2, seed=2)
    assert old[0].constraint_matrix.nnz >= 1 << 20
    got, want = _retained(old), _retained(new)
    try:
        info = got.members[0].layout_info()
        assert info["A_slabs"] >= 2 and info["At_slabs"] >= 2, info
        _update(got, new)
        rescaled = got.rescale(*RESCALINGS[12]), want.rescale(*RESCALINGS[12])
        _assert_same_batch(got, want, "column slabs", rescaled)
    finally:
        got.close()
        want.close()


# ---- the mark ----

@pytest.mark.short_rows
@pytest.mark.parametrize("kind", ["lp", "qp"])
def test_between_the_update_and_the_rescale_everything_else_is_refused(gpu_required, kind):
    make = (lambda K, seed: _family("edges", K, seed)) if kind == "lp" else _qp_family
    K = 3
    old, new = make(K, 1), make(K, 2)
    got, want = _retained(old), _retained(new)
    try:
        got.rescale(*RESCALINGS[12])
        points = _points(got, 8)
        for eng, point in zip(got.members, points):
            eng.set_current(*point)
        _update(got, new)
        member = got.members[1]
        vectors = [[getattr(p, name) for p in old] for name in NAMES]
        q = new[0].objective_matrix.data if kind == "qp" else None
        refused = {"trial_step": lambda: got.trial_step(0.3, 1.1),
                   "accept": lambda: got.accept(np.ones(K, dtype=np.int32), 1.0),
                   "take_steps": lambda: got.take_steps_adaptive(2, 0.3, 0.6, 0.1, 1.0, 0, 0.0),
                   "eval_point": lambda: member.eval_point(_lib.POINT_CURRENT),
                   "eval_points": lambda: got.eval_points(_lib.POINT_CURRENT),
                   "eval_points of nobody": lambda: got.eval_points(-1),
                   "point_products": lambda: got.point_products([(0, _lib.POINT_CURRENT)]),
                   "warm_start": lambda: got.warm_start(None, None),
                   "update_problem_vectors": lambda: got.update_problem_vectors(*vectors),
                   "another update": lambda: _update(got, old),
                   "a member's trial": lambda: member.trial_step(0.3, 1.1, 1.0),
                   "a member's vectors": member.get_problem_vectors,
                   "a member's point": lambda: member.set_current(*points[1]),
                   "a member's update": lambda: member.update_matrix_values(new[0].constraint_matrix.data, q, *[v[1] for v in vectors])}
        info, checks = got.resolve_info(), got.check_info()
        for label, call in refused.items():
            with pytest.raises(_lib.PdhgHipError) as caught:
                call()
            assert RESCALE_FIRST[0] in str(caught.value), (label, str(caught.value))
        assert got.resolve_info() == info and got.check_info() == checks           # (the info calls proceed, and nothing was counted)
        # the rescale proceeds; the batch is the fresh one, as if nothing had been tried
        rescaled = got.rescale(*RESCALINGS[12]), want.rescale(*RESCALINGS[12])
        _assert_same_batch(got, want, f"{kind} after the refusals", rescaled)
        # ... and everything works again
        for batch, problems in ((got, new), (want, new)):
            for eng, p in zip(batch.members, problems):
                eng.set_original_problem(*rescaled[0], *[getattr(p, name) for name in NAMES])
            batch.warm_start([x for x, _ in points], [y for _, y in points])
        assert np.array_equal(_bits(got.eval_points(_lib.POINT_CURRENT)), _bits(want.eval_points(_lib.POINT_CURRENT)))
        assert np.array_equal(_bits(got.members[1].eval_point(_lib.POINT_CURRENT)), _bits(want.members[1].eval_point(_lib.POINT_CURRENT)))
        assert np.array_equal(_bits(got.trial_step(0.3, 1.1)), _bits(want.trial_step(0.3, 1.1)))
        for batch in (got, want):
            batch.update_problem_vectors(*vectors)
        for k, (g, w) in enumerate(zip(got.members, want.members)):
            _same_bits(g.get_problem_vectors(), w.get_problem_vectors(), f"{kind} member {k} after a vector update")
    finally:
        got.close()
        want.close()


# ---- sessions ----

def _params(policy=None, tol=1e-6, limit=200, freq=25):
    tc = construct_termination_criteria(eps_optimal_absolute=tol, eps_optimal_relative=tol, iteration_limit=limit)
    rp = construct_restart_parameters(RestartScheme.ADAPTIVE_NORMALIZED, RestartToCurrentMetric.GAP_OVER_DISTANCE_SQUARED,
                                      1000, 0.5, 0.1, 0.9, 0.5, False)
    return PdhgParameters(10, True, 1.0, 1.0, True, 0, True, freq, tc, rp, policy or AdaptiveStepsizeParams(0.3, 0.6))


def _lp_family(K, seed=2):
    """K LPs on ``random_lp(27, 32)``'s matrix with their own c, b and upper bounds."""
    p = random_lp(27, 32, 4, seed=1)
    rng = np.random.default_rng(seed)
    out = []
    for k in range(K):
        c = p.objective_vector * (1.0 + 0.5 * rng.random(p.num_variables)) if k else p.objective_vector.copy()
        b = p.right_hand_side * (1.0 + 0.05 * rng.random(p.num_constraints)) if k else p.right_hand_side.copy()
        out.append(linear_programming_problem(p.variable_lower_bound.copy(), p.variable_upper_bound + k % 4, c, 0.0,
                                              p.constraint_matrix, b, p.num_equalities))
    return out


FAMILIES = {"lp_K1": lambda: _lp_family(1), "lp_K3": lambda: _lp_family(3), "lp_K32": lambda: _lp_family(32),
            "qp_K3": lambda: random_qp_family(27, 32, 3, seed=3, nnz_per_row=4)}


def _matrix_update(problems, seed=0):
    """Every stored value of A times 1 + 0.01 N(0, 1); a QP family's Q times 1.05 (it stays symmetric positive definite)."""
    rng = np.random.default_rng(seed)
    A = problems[0].constraint_matrix
    update = {"constraint_matrix_values": A.data * (1.0 + 0.01 * rng.standard_normal(A.nnz))}
    if problems[0].objective_matrix.nnz:
        update["objective_matrix_values"] = problems[0].objective_matrix.data * 1.05
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


@pytest.mark.short_rows
@pytest.mark.parametrize("checks", ["member_checks", "batch_checks"])
@pytest.mark.parametrize("policy", [AdaptiveStepsizeParams(0.3, 0.6), ConstantStepsizeParams()], ids=["adaptive", "constant"])
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_update_matrix_then_solve_is_optimize_batch_on_the_updated_problems(gpu_required, monkeypatch, family, policy, checks):
    if checks == "batch_checks":
        monkeypatch.setenv("PDHG_BATCH_CHECKS", "1")
    else:
        monkeypatch.delenv("PDHG_BATCH_CHECKS", raising=False)
    problems = FAMILIES[family]()
    K = len(problems)
    params = _params(policy)
    update = _matrix_update(problems)
    updated = _applied(problems, update)
    rng = np.random.default_rng(9)
    with PdhgBatchSession(params, problems) as session:
        session.solve()
        launches = session.batch.resolve_info()["shared_launches"]
        session.update_matrix(**update)
        info = session.batch.resolve_info()
        assert info["shared_launches"] == launches + 1 and info["carried"] == K, info        # the one replay launch
        _assert_all_same(session.solve(), optimize_batch(params, updated))
        points = [(rng.uniform(0, 1, p.num_variables), rng.standard_normal(p.num_constraints)) for p in updated]
        _assert_all_same(session.solve(warm_start=points), optimize_batch(params, updated, initial_solutions=points))


@pytest.mark.short_rows
@pytest.mark.parametrize("family", ["lp_K3", "qp_K3"])
def test_two_matrix_updates_in_a_row_with_a_vector_update_between_them(gpu_required, family):
    problems = FAMILIES[family]()
    params = _params()
    first, second = _matrix_update(problems, seed=1), _matrix_update(problems, seed=2)
    ub = problems[0].variable_upper_bound.copy()
    ub[::7] = np.where(np.isfinite(ub[::7]), ub[::7] * 1.25, 12.0)
    vectors = [{"right_hand_side": problems[0].right_hand_side * 1.01, "variable_upper_bound": ub}, None,
               {"objective_vector": problems[2].objective_vector * 1.1}]
    ride = [None, {"right_hand_side": problems[1].right_hand_side * 0.99}, None]
    with PdhgBatchSession(params, problems) as session:
        session.solve()
        session.update_matrix(**first)
        session.update(vectors)
        session.update_matrix(updates=ride, **second)                 # (member 1's new vector rides the matrix update)
        want = _applied(_applied(problems, second, vectors), {}, ride)
        for got, p in zip(session.problems, want):
            for name in NAMES:
                assert np.array_equal(getattr(got, name), getattr(p, name)), name
            assert np.array_equal(got.constraint_matrix.data, p.constraint_matrix.data)
        cold = session.solve()
        _assert_all_same(cold, optimize_batch(params, want))
        last = [(g.primal_solution, g.dual_solution) for g in cold]
        _assert_all_same(session.solve(warm_start=True), optimize_batch(params, want, initial_solutions=last))


# ---- the C call's refusals ----

def _table(rows):
    """None -> a NULL table; a list of K arrays / None -> an array of K pointers (NULL entries for None), and what it points to."""
    if rows is None:
        return None, []
    keep = [None if r is None else np.ascontiguousarray(r, dtype=np.float64) for r in rows]
    table = (_lib._dp * len(rows))()
    for k, r in enumerate(keep):
        if r is not None:
            table[k] = r.ctypes.data_as(_lib._dp)
    return table, keep


def _raw_update(handle, nnz, values, q_nnz, q_values, c, b, lb, ub):
    flat = [None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in (values, q_values)]
    tables = [_table(rows) for rows in (c, b, lb, ub)]                   # (they outlive the call)
    rc = _lib.lib().pdhg_batch_update_matrix_values(handle, nnz, None if flat[0] is None else flat[0].ctypes.data_as(_lib._dp), q_nnz,
                                                    None if flat[1] is None else flat[1].ctypes.data_as(_lib._dp), *[t for t, _ in tables])
    return rc, _lib.lib().pdhg_last_error().decode()


def _refused(handle, words, *args):
    rc, message = _raw_update(handle, *args)
    assert rc == -1 and any(w in message for w in words), (rc, message)


def _state(batch):
    return ([eng.get_problem_vectors() for eng in batch.members], batch.members[0].layout_checksums(), batch.resolve_info(),
            [eng.steps_info() for eng in batch.members], batch.check_info())


def _assert_state(batch, before, label):
    after = _state(batch)
    for k, (g, w) in enumerate(zip(after[0], before[0])):
        _same_bits(g, w, f"{label} member {k}")
    assert np.array_equal(after[1], before[1]), label
    assert after[2:] == before[2:], label


@pytest.mark.short_rows
def test_refusals_launch_nothing_and_leave_the_batch_usable(gpu_required):
    problems = _lp_family(3)
    A = problems[0].constraint_matrix
    K = len(problems)
    c, b, lb, ub = ([getattr(p, name) for p in problems] for name in NAMES)
    good = (A.nnz, A.data * 1.5, 0, None, c, b, lb, ub)
    points = None

    def usable(batch, before, trial, label):
        _assert_state(batch, before, label)
        for g, w in zip(_trial(batch, points), trial):
            assert np.array_equal(g, w), label

    _refused(None, ["null handle"], *good)

    batch = HipPdhgBatch.from_problems(problems)
    try:
        batch.rescale(*RESCALINGS[12])
        points = _points(batch, 3)
        before, trial = _state(batch), _trial(batch, points)
        _refused(batch._h, ["pdhg_batch_resolve_retain"], *good)
        usable(batch, before, trial, "not retained")
    finally:
        batch.close()
    _raises_naming(_lib.PdhgHipError, ["closed"], lambda: _update(batch, problems))

    batch = _retained(problems)
    try:
        batch.rescale(*RESCALINGS[12])
        before, trial = _state(batch), _trial(batch, points)
        _refused(batch._h, ["nnz"], A.nnz - 1, A.data[:-1], 0, None, c, b, lb, ub)
        _refused(batch._h, ["nnz"], A.nnz + 1, np.ones(A.nnz + 1), 0, None, c, b, lb, ub)
        _refused(batch._h, ["nzval"], A.nnz, None, 0, None, c, b, lb, ub)
        for q in range(4):
            tables = [c, b, lb, ub]
            tables[q] = None
            _refused(batch._h, ["all needed"], A.nnz, A.data, 0, None, *tables)            # a NULL table
            for k in (0, K - 1):
                tables[q] = [None if j == k else v for j, v in enumerate((c, b, lb, ub)[q])]
                _refused(batch._h, [f"member {k}"], A.nnz, A.data, 0, None, *tables)       # a NULL entry
        _refused(batch._h, ["LP batch"], A.nnz, A.data, 3, np.ones(3), c, b, lb, ub)
        _refused(batch._h, ["LP batch"], A.nnz, A.data, 0, np.ones(3), c, b, lb, ub)
        _raises_naming(ValueError, ["entries"], lambda: batch.update_matrix_values(A.data, None, [v[:-1] for v in c], b, lb, ub))
        _raises_naming(ValueError, ["entries", "needed"], lambda: batch.update_matrix_values(A.data, None, c[:-1], b, lb, ub))
        _raises_naming(ValueError, ["needed"], lambda: batch.update_matrix_values(A.data, None, c, [b[0], None, b[2]], lb, ub))
        # the call of one handle keeps refusing a member, and a member handle is no batch
        _refused(batch.members[0]._h, ["not a batch handle"], *good)
        usable(batch, before, trial, "bad arguments")
        # ... and the batch still takes a good update
        batch.update_matrix_values(A.data * 1.5, None, c, b, lb, ub)
        batch.rescale(*RESCALINGS[12])
        want = _retained(_applied(problems, {"constraint_matrix_values": A.data * 1.5}))
        try:
            want.rescale(*RESCALINGS[12])
            _assert_same_batch(batch, want, "after the refusals")
        finally:
            want.close()
    finally:
        batch.close()

    qps = random_qp_family(27, 32, 2, seed=3, nnz_per_row=4)
    QA, Q = qps[0].constraint_matrix, qps[0].objective_matrix
    vectors = [[getattr(p, name) for p in qps] for name in NAMES]
    batch = _retained(qps)
    try:
        points = _points(batch, 4)
        before, trial = _state(batch), _trial(batch, points)
        _refused(batch._h, ["q_nzval == NULL"], QA.nnz, QA.data, 0, None, *vectors)
        _refused(batch._h, ["q_nzval == NULL"], QA.nnz, QA.data, Q.nnz, None, *vectors)
        _refused(batch._h, ["q_nnz"], QA.nnz, QA.data, Q.nnz - 1, Q.data[:-1], *vectors)
        usable(batch, before, trial, "qp")
    finally:
        batch.close()

    # a plain handle and a fleet handle
    plain = HipPdhgEngine.from_problem(problems[0])
    fleet = HipPdhgFleet.from_problems(problems[:2])
    try:
        plain.retain_rescaling()
        for handle, eng in ((plain._h, plain), (fleet._h, fleet.members[0])):
            at_start = eng.get_problem_vectors(), eng.steps_info()
            _refused(handle, ["not a batch handle"], *good)
            _same_bits(eng.get_problem_vectors(), at_start[0], "no batch")
            assert eng.steps_info() == at_start[1]
    finally:
        plain.close()
        fleet.close()


@pytest.mark.short_rows
def test_a_batch_created_from_unsorted_columns_is_refused(gpu_required):
    """``pdhg_create_batch`` keeps such columns in the caller's order; the placement searches need ascending runs, so the
    update refuses the batch (the one refusal that looks at the device: a read-only pass) and leaves it usable.  The call
    is made twice and refused twice with the same words and the same state afterwards; that the second answer comes
    from the remembered look and not from a second pass is not observable through the ABI (no counter sees that
    kernel) and is not asserted here."""
    m, n, K = 6, 4, 2
    cs, bs = [np.ones(n), np.arange(n) + 1.0], [np.ones(m), np.linspace(-1, 1, m)]
    lbs, ubs = [np.zeros(n)] * K, [np.full(n, 5.0), np.full(n, 4.0)]
    indptr = np.array([0, 2, 4, 5, 7])
    cases = {"swapped": np.array([3, 1, 0, 2, 5, 1, 4]), "sorted": np.array([1, 3, 0, 2, 5, 1, 4])}
    values = np.arange(7) + 1.5
    for label, indices in cases.items():
        A = sp.csc_matrix((values, indices, indptr), shape=(m, n))
        assert np.array_equal(A.indices, indices)               # (nothing sorted them)
        batch = HipPdhgBatch(A, cs, bs, lbs, ubs, 2)
        try:
            batch.retain_rescaling()
            points = _points(batch, 2)
            before, trial = _state(batch), _trial(batch, points)
            if label == "sorted":
                batch.update_matrix_values(values[::-1].copy(), None, cs, bs, lbs, ubs)
                batch.rescale(*RESCALINGS[1])
                want = HipPdhgBatch(sp.csc_matrix((values[::-1].copy(), indices, indptr), shape=(m, n)), cs, bs, lbs, ubs, 2)
                try:
                    want.retain_rescaling()
                    want.rescale(*RESCALINGS[1])
                    _assert_same_batch(batch, want, "sorted")
                finally:
                    want.close()
                continue
            for _ in range(2):
                _refused(batch._h, ["ascend"], 7, values * 2, 0, None, cs, bs, lbs, ubs)
            _assert_state(batch, before, label)
            for g, w in zip(_trial(batch, points), trial):
                assert np.array_equal(g, w), label
        finally:
            batch.close()
