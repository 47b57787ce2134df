"""A fleet's rescaling in one shared launch (include/pdhg_hip_fleet_rescale.h, csrc/fleet_rescale_kernels.hpp,
csrc/abi_fleet_rescale.hpp, ``HipPdhgFleet.rescale``).

Every case builds two fleets from the same problems: one is rescaled by ``fleet.rescale``, its twin member by member
with ``eng.rescale`` and ``eng.matrix_max_abs``.  Compared bit for bit: E, D and max |a|; the problem vectors; the 32
layout checksums; both products on a probe vector and a trial step from a probe point (which reads Q x on a QP, and the
compact bound views the shared call leaves to their next reader).  No tolerance and no skipped member, and
``rescale_info()`` must say which members rode the launch: a silent fall-back cannot pass.

Shapes: the lane-stride tails of a row and of a column (0, 1, 2, 63, 64, 65, 127, 128, 129 entries and 2 048, the longest
row that is not a long row), a column of stored zeros, a stored -0.0, bounds of +-inf and 0; 1 x 1, no rows, n + m = 4 096
(carried) and 4 097 (served by its own calls, the same bits), a row beyond the long-row threshold (its own calls); every
step alone and all together; 1, 3 and 300 members, LPs and QPs mixed, an ``active`` mask; retained members; refusals;
whole solves with the switch on and off.  PDHG_TUNE=0 throughout: two fleets of one pattern make the same choices."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

from firstorderlp_jl_amd import HipPdhgFleet, PdhgFleetSession, _lib, linear_programming_problem, optimize_many
from firstorderlp_jl_amd.evaluation import POINT_CURRENT
from firstorderlp_jl_amd.generators import random_lp
from firstorderlp_jl_amd.quadratic_programming import QuadraticProgrammingProblem
from tests.helpers import assert_same_output as _assert_same, bits as _bits, same_bits as _same_bits
from tests.test_gpu_matrix_update import _applied, _distinct_values, _matrix_update, _params

pytestmark = pytest.mark.gpu

ALL = (10, True, 1.0)        # solve_qp's defaults: 11 steps
# every step alone, so that a wrong order or a step that reads another one's vector shows; then together
STEPS = {"none": (0, False, None), "ruiz1": (1, False, None), "ruiz10": (10, False, None), "l2": (0, True, None),
         "pc0": (0, False, 0.0), "pc1": (0, False, 1.0), "pc2": (0, False, 2.0), "ruiz1_l2_pc0": (1, True, 0.0), "all": ALL}
LENGTHS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 2048)


@pytest.fixture(autouse=True)
def _no_tuning(monkeypatch):
    monkeypatch.setenv("PDHG_TUNE", "0")
    monkeypatch.delenv("PDHG_FLEET_RESCALE", raising=False)


# ---- problems ----

def _lp_of(A, seed, Q=None):
    """The LP (QP) over ``A`` with vectors drawn from ``seed``: bounds of -inf, +inf, 0 and finite values."""
    m, n = A.shape
    rng = np.random.default_rng(seed)
    lb = np.where(rng.random(n) < 0.25, -np.inf, rng.integers(-2, 1, n).astype(float))
    ub = np.where(rng.random(n) < 0.4, np.inf, np.maximum(lb, 0.0) + rng.integers(0, 3, n))
    c, b = rng.standard_normal(n), rng.standard_normal(m)
    if Q is None:
        return linear_programming_problem(lb, ub, c, 0.0, A, b, m // 3)
    return QuadraticProgrammingProblem(lb, ub, Q, c, 0.0, A, b, m // 3)


def _valued(mask, seed):
    """``mask`` as a canonical CSC whose stored values are all distinct."""
    A = sp.csc_matrix(mask.astype(np.float64))
    A.sort_indices()
    return sp.csc_matrix((_distinct_values(A.nnz, seed), A.indices, A.indptr), shape=A.shape)


def _lengths_matrix(seed):
    """12 x 2 050: row i holds LENGTHS[i] entries for i < 10 -- the last a row of 2 048, the longest that is not a long
    row -- none of them in column 5 or in column 2 049, which stays empty; column 5 holds stored zeros in rows 10 and
    11, and one stored value becomes -0.0."""
    rng = np.random.default_rng(seed)
    mask = np.zeros((12, 2050), dtype=bool)
    free = np.array([j for j in range(2049) if j != 5])
    for i, count in enumerate(LENGTHS):
        mask[i, rng.choice(free, size=count, replace=False)] = True
    mask[10:, 5] = True
    A = _valued(mask, seed)
    lo, hi = A.indptr[5], A.indptr[6]
    A.data[lo:hi] = 0.0                       # a column of stored zeros: its factor becomes 1, pow(0, 0) its Pock-Chambolle term
    A.data[A.indptr[7]] = -0.0                # ... and a stored -0.0
    assert A.nnz == mask.sum()
    return A


def _lengths_lp(seed=11):
    return _lp_of(_lengths_matrix(seed), seed)


def _lengths_lp_transposed(seed=12):
    """2 050 x 12: the same lengths as COLUMNS (rows of CSR(A')), an empty row."""
    return _lp_of(sp.csc_matrix(_lengths_matrix(seed).T), seed)


def _random_qp(m, n, seed, nnz_per_row=4):
    """random_lp plus Q = B'B + diag (tests/test_gpu_small_qp.py: _random_qp)."""
    p = random_lp(m, n, min(nnz_per_row, n), seed=seed)
    B = sp.random(max(n // 3, 1), n, density=3.0 / n, format="csr", random_state=seed + 1)
    Q = sp.csc_matrix(B.T @ B + sp.diags(np.linspace(0.0, 0.5, n)))
    Q.sort_indices()
    return QuadraticProgrammingProblem(p.variable_lower_bound, p.variable_upper_bound, Q, p.objective_vector, 0.0,
                                       p.constraint_matrix, p.right_hand_side, p.num_equalities)


def _sized(m, n, seed):
    """m x n with about three entries per row and a few empty rows and columns."""
    rng = np.random.default_rng(seed)
    rows = np.repeat(np.arange(m), 3)
    mask = sp.csc_matrix((np.ones(rows.size), (rows, rng.integers(0, n, rows.size))), shape=(m, n)).toarray() > 0
    mask[::97, :] = False
    return _lp_of(_valued(mask, seed), seed)


def _long_row_lp(seed=13):
    """10 x 2 100 with a row of 2 049 entries: beyond the long-row threshold, so not in the class."""
    rng = np.random.default_rng(seed)
    mask = rng.random((10, 2100)) < 0.01
    mask[4, :] = False
    mask[4, :2049] = True
    return _lp_of(_valued(mask, seed), seed)


def _one_by_one():
    return _lp_of(sp.csc_matrix(np.array([[-3.5]])), 14)


def _no_rows():
    return _lp_of(sp.csc_matrix((0, 5)), 15)


# ---- the comparison ----

def _probe(p):
    rng = np.random.default_rng(p.num_variables + 7 * p.num_constraints)
    return rng.standard_normal(p.num_variables), rng.standard_normal(p.num_constraints)


def _assert_same_member(got, want, p, label):
    _same_bits(got.get_problem_vectors(), want.get_problem_vectors(), label)
    a, b = got.layout_checksums(), want.layout_checksums()
    assert np.array_equal(a, b), (label, np.nonzero(a != b)[0])
    x, y = _probe(p)
    assert np.array_equal(_bits(got.spmv(x)), _bits(want.spmv(x))), f"{label}: A x"
    assert np.array_equal(_bits(got.spmv_t(y)), _bits(want.spmv_t(y))), f"{label}: A' y"
    if p.num_constraints == 0:
        return
    # a trial step from the probe point: Q x on a QP, and lb / ub through the bound views
    for eng in (got, want):
        eng.set_current(x, y)
    raw = [eng.trial_step(0.3, 1.1, 1.0) for eng in (got, want)]
    assert np.array_equal(_bits(raw[0]), _bits(raw[1])), f"{label}: trial step"
    _same_bits(got.get_trial(), want.get_trial(), f"{label}: trial point")


def _rescale_both(fleet, twin, steps, members=None):
    """``fleet.rescale`` against the twin's member calls: asserts E, D and max |a|, returns the members named."""
    named = list(range(fleet.K)) if members is None else list(members)
    factors, max_abs = fleet.rescale(*steps, members=members)
    assert len(factors) == len(max_abs) == len(named)
    for k, (E, D), a in zip(named, factors, max_abs):
        E_want, D_want = twin.members[k].rescale(*steps)
        assert np.array_equal(_bits(E), _bits(E_want)), f"member {k}: E"
        assert np.array_equal(_bits(D), _bits(D_want)), f"member {k}: D"
        assert _bits(a) == _bits(twin.members[k].matrix_max_abs()), f"member {k}: max |a|"
    return named


def _compare(problems, steps, single=(), retain=False):
    """Both routes on twins of ``problems``; ``single``: the members expected outside the class."""
    fleet, twin = HipPdhgFleet.from_problems(problems), HipPdhgFleet.from_problems(problems)
    try:
        if retain:
            for eng in fleet.members + twin.members:
                eng.retain_rescaling()
        launches = fleet.rescale_info()["shared_launches"]
        _rescale_both(fleet, twin, steps)
        info = fleet.rescale_info()
        assert info["carried"] == len(problems) - len(single) and info["single"] == len(single), info
        assert info["shared_launches"] == launches + (1 if info["carried"] else 0), info
        for k, p in enumerate(problems):
            _assert_same_member(fleet.members[k], twin.members[k], p, f"member {k}")
        return fleet, twin
    except Exception:
        fleet.close()
        twin.close()
        raise


def _closed(pair):
    for f in pair:
        f.close()


# ---- lengths, values, steps ----

@pytest.mark.parametrize("steps", sorted(STEPS))
def test_every_step_alone_and_together_on_the_row_and_column_lengths(gpu_required, steps):
    _closed(_compare([_lengths_lp(), _lengths_lp_transposed(), _random_qp(40, 48, 3)], STEPS[steps]))


def test_the_lengths_member_holds_what_it_is_meant_to():
    A = _lengths_lp().constraint_matrix
    rows, cols = np.diff(A.tocsr().indptr), np.diff(A.indptr)
    assert rows.tolist() == list(LENGTHS) + [1, 1] and cols[2049] == 0 and cols.max() <= 12
    assert np.all(A.data[A.indptr[5]:A.indptr[6]] == 0.0) and cols[5] == 2
    assert np.signbit(A.data[A.indptr[7]]) and A.data[A.indptr[7]] == 0.0
    live = A.data[A.data != 0.0]
    assert len(np.unique(live)) == len(live)
    p = _lengths_lp()
    for v in (-np.inf, 0.0):
        assert v in p.variable_lower_bound
    assert np.inf in p.variable_upper_bound and 0.0 in p.variable_upper_bound


# ---- shapes, and who is carried ----

def test_the_shapes_at_the_edges_of_the_class(gpu_required):
    problems = [_one_by_one(), _no_rows(), _sized(1000, 3096, 21), _sized(1000, 3097, 22), _long_row_lp()]
    assert [p.num_variables + p.num_constraints for p in problems[2:4]] == [4096, 4097]
    fleet, twin = _compare(problems, ALL, single=(3, 4))
    try:
        # which members: one at a time
        for k, carried in enumerate([1, 1, 1, 0, 0]):
            _rescale_both(fleet, twin, STEPS["ruiz1"], members=[k])
            info = fleet.rescale_info()
            assert (info["carried"], info["single"]) == (carried, 1 - carried), (k, info)
            _assert_same_member(fleet.members[k], twin.members[k], problems[k], f"member {k}, alone")
    finally:
        _closed((fleet, twin))


# ---- member counts ----

def _mixed(K, seed=0):
    """LPs and QPs of different small shapes."""
    shapes = [(27, 32), (5, 9), (40, 30), (56, 97), (1, 3), (33, 17), (64, 64), (13, 65)]
    return [(_random_qp if k % 3 == 2 else lambda m, n, s: random_lp(m, n, min(4, n), seed=s))(*shapes[k % len(shapes)], seed + k)
            for k in range(K)]


@pytest.mark.parametrize("K", [1, 3, 300])
def test_one_three_and_more_members_than_compute_units(gpu_required, K):
    _closed(_compare(_mixed(K), ALL))


def test_an_active_mask_leaves_the_other_members_as_they_are(gpu_required):
    problems = _mixed(6, seed=50)
    fleet, twin = HipPdhgFleet.from_problems(problems), HipPdhgFleet.from_problems(problems)
    try:
        for f in (fleet, twin):
            for eng, p in zip(f.members, problems):
                eng.set_original_problem(np.ones(eng.m), np.ones(eng.n), p.objective_vector, p.right_hand_side,
                                         p.variable_lower_bound, p.variable_upper_bound)
        before = [(eng.get_problem_vectors(), eng.layout_checksums(), eng.matrix_max_abs()) for eng in fleet.members]
        rows = fleet.eval_points(np.full(fleet.K, POINT_CURRENT, dtype=np.int32))
        named = _rescale_both(fleet, twin, ALL, members=[4, 1, 2])
        assert named == [4, 1, 2]
        info = fleet.rescale_info()
        assert (info["carried"], info["single"]) == (3, 0), info
        # versions: the evaluation the fleet stored in an untouched member still answers; a rescaled member computes
        misses = fleet.check_info()["misses"]
        for k in (0, 3, 5):
            assert np.array_equal(_bits(fleet.members[k].eval_point(POINT_CURRENT)), _bits(rows[k])), k
        assert fleet.check_info()["misses"] == misses
        for j, k in enumerate(named):
            fleet.members[k].eval_point(POINT_CURRENT)
            assert fleet.check_info()["misses"] == misses + j + 1, k
        for k in named:
            _assert_same_member(fleet.members[k], twin.members[k], problems[k], f"member {k}")
        for k in (0, 3, 5):
            vectors, sums, max_abs = before[k]
            _same_bits(fleet.members[k].get_problem_vectors(), vectors, f"member {k}")
            assert np.array_equal(fleet.members[k].layout_checksums(), sums) and _bits(fleet.members[k].matrix_max_abs()) == _bits(max_abs)
    finally:
        _closed((fleet, twin))


# ---- retained members ----

def _fresh_vectors(p, seed):
    rng = np.random.default_rng(seed)
    n, m = p.num_variables, p.num_constraints
    lb = np.where(rng.random(n) < 0.3, -np.inf, -rng.integers(0, 3, n).astype(float))
    return rng.standard_normal(n), rng.standard_normal(m), lb, np.where(rng.random(n) < 0.3, np.inf, lb.clip(-5, 0) + 4.0)


def _update_vectors_and_compare(fleet, twin, problems, seed):
    """New vectors through the retained record (the fleet's one launch against the twin's member calls), a warm start
    through the running products."""
    vectors = [_fresh_vectors(p, seed + k) for k, p in enumerate(problems)]
    fleet.update_problem_vectors(*[[v[q] for v in vectors] for q in range(4)])
    points = [_probe(p) for p in problems]
    fleet.warm_start([x for x, _ in points], [y for _, y in points])
    for k, (eng, v, (x, y)) in enumerate(zip(twin.members, vectors, points)):
        eng.update_problem_vectors(*v)
        eng.warm_start(x, y)
        _same_bits(fleet.members[k].get_problem_vectors(), eng.get_problem_vectors(), f"member {k}: replayed vectors")
        _same_bits(fleet.members[k].get_current(), eng.get_current(), f"member {k}: warm start")


def test_retained_members_record_the_steps_and_take_a_second_rescaling_after_new_values(gpu_required):
    problems = _mixed(5, seed=70) + [_lengths_lp_transposed()]
    fleet, twin = _compare(problems, ALL, retain=True)
    try:
        _update_vectors_and_compare(fleet, twin, problems, seed=1)
        # new matrix values reset the record; the rescaling that follows writes it again from its first step
        for round_ in (2, 3):
            updated = [_applied(p, _matrix_update(p, seed=round_)) for p in problems]
            for f in (fleet, twin):
                for eng, p in zip(f.members, updated):
                    q = p.objective_matrix.data if p.objective_matrix.nnz else None
                    eng.update_matrix_values(p.constraint_matrix.data, q, p.objective_vector, p.right_hand_side,
                                             p.variable_lower_bound, p.variable_upper_bound)
            _rescale_both(fleet, twin, ALL)
            assert fleet.rescale_info()["single"] == 0
            for k, p in enumerate(updated):
                _assert_same_member(fleet.members[k], twin.members[k], p, f"round {round_}, member {k}")
            _update_vectors_and_compare(fleet, twin, updated, seed=10 * round_)
    finally:
        _closed((fleet, twin))


# ---- refusals ----

def test_refusals_launch_nothing_and_leave_every_member_as_it_was(gpu_required):
    problems = _mixed(3, seed=90)
    fleet = HipPdhgFleet.from_problems(problems)
    try:
        for eng, p in zip(fleet.members, problems):
            eng.set_original_problem(np.ones(eng.m), np.ones(eng.n), p.objective_vector, p.right_hand_side,
                                     p.variable_lower_bound, p.variable_upper_bound)
        rows = fleet.eval_points(np.full(fleet.K, POINT_CURRENT, dtype=np.int32))
        before = [(eng.get_problem_vectors(), eng.layout_checksums()) for eng in fleet.members]
        info = fleet.rescale_info()
        with pytest.raises(_lib.PdhgHipError, match="pock_chambolle_alpha"):
            fleet.rescale(10, True, 2.5)
        with pytest.raises(_lib.PdhgHipError, match="l_inf_ruiz_iterations"):
            fleet.rescale(-1, True, 1.0)
        dpp = ctypes.POINTER(ctypes.c_double)
        assert _lib.lib().pdhg_fleet_rescale(fleet.members[0]._h, None, 10, 1, 1, 1.0, None, None, ctypes.cast(None, dpp)) == -1
        assert b"not a fleet handle" in _lib.lib().pdhg_last_error()
        assert fleet.rescale_info() == info
        misses = fleet.check_info()["misses"]
        for k, eng in enumerate(fleet.members):
            _same_bits(eng.get_problem_vectors(), before[k][0], f"member {k}")
            assert np.array_equal(eng.layout_checksums(), before[k][1])
            assert np.array_equal(_bits(eng.eval_point(POINT_CURRENT)), _bits(rows[k]))      # (its versions have not moved)
        assert fleet.check_info()["misses"] == misses
        factors, max_abs = fleet.rescale(*ALL)                                               # usable as before
        assert len(factors) == 3 and fleet.rescale_info()["carried"] == 3
    finally:
        fleet.close()


# ---- whole solves ----

def _eight():
    return _mixed(7, seed=30) + [random_lp(300, 260, 4, seed=3)]


def test_optimize_many_gives_the_same_outputs_with_the_switch_on(gpu_required, monkeypatch):
    problems = _eight()
    params = _params(limit=48)
    want = optimize_many(params, problems)
    monkeypatch.setenv("PDHG_FLEET_RESCALE", "1")
    calls = []
    inner = HipPdhgFleet.rescale
    monkeypatch.setattr(HipPdhgFleet, "rescale", lambda self, *a, **k: calls.append(1) or inner(self, *a, **k))
    for got, w in zip(optimize_many(params, problems), want):
        _assert_same(got, w)
    assert calls == [1]


def test_a_fleet_session_tick_with_a_matrix_update_gives_the_same_outputs_with_the_switch_on(gpu_required, monkeypatch):
    problems = _eight()
    params = _params(limit=40)
    updates = [_matrix_update(p, seed=k) if k % 2 == 0 else None for k, p in enumerate(problems)]
    updates[1] = {"right_hand_side": problems[1].right_hand_side * 1.02}

    def tick():
        with PdhgFleetSession(params, problems) as session:
            first = session.solve()
            session.update(updates)
            return first + session.solve(warm_start=True), session.fleet.rescale_info()
    want, info_off = tick()
    assert info_off["shared_launches"] == 0
    monkeypatch.setenv("PDHG_FLEET_RESCALE", "1")
    got, info_on = tick()
    assert info_on["shared_launches"] == 2 and (info_on["carried"], info_on["single"]) == (4, 0), info_on
    for g, w in zip(got, want):
        _assert_same(g, w)
