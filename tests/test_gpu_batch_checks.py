"""A batch's checks in shared launches on the device (include/pdhg_hip_batch_checks.h, ``HipPdhgBatch.point_products`` /
``eval_points`` / ``check_info``, ``PDHG_BATCH_CHECKS=1``).

The yardstick everywhere is a TWIN batch handle on the same problems that takes the same steps and never uses the new
calls: its members compute every product, evaluation and search on their own.  Every comparison is bitwise.

Shapes: 700 x 500 with six entries per row (three evaluation blocks per member; neither dimension a multiple of 64 or
256), a 37 x 1 matrix, a matrix with empty rows and empty columns, and the QP form of the first (Q = B'B + diag).  Member
counts 1, 3 (a padded lane: the interleave is four wide) and 32.  State: 10 adaptive batched steps, the restart point
saved on every member, 10 more."""
import ctypes
import dataclasses

import numpy as np
import pytest
import scipy.sparse as sp

from firstorderlp_jl_amd import HipPdhgBatch, PdhgBatchSession, _lib, linear_programming_problem, optimize_batch
from firstorderlp_jl_amd.generators import (l1_svm_regularization_path, personalized_pagerank_lps,
                                            preprocess_training_data, random_lp, random_qp_family, synthetic_rcv1_like)
from firstorderlp_jl_amd.primal_dual_hybrid_gradient import AdaptiveStepsizeParams, PdhgParameters
from firstorderlp_jl_amd.saddle_point import RestartScheme, RestartToCurrentMetric, construct_restart_parameters
from firstorderlp_jl_amd.termination import construct_termination_criteria
from tests import helpers as H

pytestmark = pytest.mark.gpu

RED, GROW = 0.3, 0.6
CURRENT, AVERAGE, RESTART = _lib.POINT_CURRENT, _lib.POINT_AVERAGE, _lib.POINT_RESTART
POINTS = (CURRENT, AVERAGE, RESTART)
_int_p = ctypes.POINTER(ctypes.c_int)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _family(base, K, seed):
    """K LPs on ``base``'s matrix: member 0 is ``base``, the others move c, the inequalities' right-hand sides (into the
    feasible side) and the finite upper bounds."""
    rng = np.random.default_rng(seed)
    m, n, ne = base.num_constraints, base.num_variables, base.num_equalities
    out = []
    for k in range(K):
        c = base.objective_vector + (0.1 * rng.standard_normal(n) if k else 0.0)
        b = base.right_hand_side.copy()
        if k:
            b[ne:] -= 0.1 * rng.random(m - ne)
        out.append(linear_programming_problem(base.variable_lower_bound.copy(), base.variable_upper_bound + 0.25 * k, c, 0.0,
                                              base.constraint_matrix, b, ne))
    return out


def _column_lp():
    """37 x 1: one variable, every row one entry."""
    rng = np.random.default_rng(5)
    A = sp.csc_matrix(rng.uniform(0.5, 2.0, (37, 1)) * rng.choice([-1.0, 1.0], (37, 1)))
    x0 = 0.7
    b = (A @ np.array([x0])).reshape(-1)
    b[5:] -= rng.random(32)
    return linear_programming_problem(np.array([0.0]), np.array([3.0]), np.array([1.0]), 0.0, A, b, 5)


def _holes_lp():
    """60 x 50 with rows 0, 17, 59 and columns 0, 23, 49 empty."""
    p = random_lp(60, 50, 4, seed=21)
    A = sp.lil_matrix(p.constraint_matrix)
    for r in (0, 17, 59):
        A[r, :] = 0.0
    for c in (0, 23, 49):
        A[:, c] = 0.0
    A = sp.csc_matrix(A)
    A.eliminate_zeros()
    b = p.right_hand_side.copy()
    b[[0, 17]] = 0.0                             # (an empty equality row must read 0 = 0)
    b[59] = -1.0                                 # (an empty inequality row: 0 >= -1)
    return linear_programming_problem(p.variable_lower_bound, p.variable_upper_bound, p.objective_vector, 0.0, A, b,
                                      p.num_equalities)


def _long_lp(transpose):
    """One row (``transpose``: one column) of one entry more than the row order's sequential limit; everything else has
    three entries per row."""
    lim = H.bitexact_row_limit()
    rng = np.random.default_rng(lim + int(transpose))
    short, long_ = 48, lim + 40
    rows = np.concatenate([np.repeat(np.arange(short), 3), np.full(lim + 1, short)])
    cols = np.concatenate([np.concatenate([rng.choice(long_, 3, replace=False) for _ in range(short)]),
                           rng.choice(long_, lim + 1, replace=False)])
    A = sp.csc_matrix((rng.uniform(0.2, 1.5, len(rows)) * rng.choice([-1.0, 1.0], len(rows)), (rows, cols)), shape=(short + 1, long_))
    if transpose:
        A = sp.csc_matrix(A.T)
    m, n = A.shape
    x0 = rng.random(n)
    b = A @ x0
    ne = m // 2
    b[ne:] -= rng.random(m - ne)
    return linear_programming_problem(np.zeros(n), np.full(n, 2.0), rng.standard_normal(n), 0.0, A, b, ne)


SHAPES = {
    "700x500": lambda K: _family(random_lp(700, 500, 6, seed=11), K, seed=12),
    "37x1": lambda K: _family(_column_lp(), K, seed=13),
    "holes": lambda K: _family(_holes_lp(), K, seed=14),
    "qp700x500": lambda K: random_qp_family(700, 500, K, seed=15, nnz_per_row=6),
}
CASES = [(s, K) for s in SHAPES for K in (1, 3, 32)]


class _Rig:
    """A batch and its twin on the same problems: retained, rescaled the same way, the original problems set, stepped side
    by side.  Only ``batch`` ever sees the new calls."""

    def __init__(self, problems):
        self.problems = problems
        self.K = len(problems)
        self.batch = self.twin = None
        try:
            self.batch = self._make()
            self.twin = self._make()
        except Exception:
            self.close()
            raise
        sw = [H.initial_step_and_weight(p) for p in problems]
        self.ss = np.array([s for s, _ in sw])
        self.pw = np.array([w if np.isfinite(w) and w > 0 else 1.0 for _, w in sw])
        self.it = np.zeros(self.K, dtype=np.int64)
        self.kkt = np.zeros(self.K)

    def _make(self):
        b = HipPdhgBatch.from_problems(self.problems)
        try:
            b.retain_rescaling()
            E, D = b.rescale(4, False, 1.0)
            self.scaling = (E, D)
            for p, eng in zip(self.problems, b.members):
                self.set_original(eng, p)
        except Exception:
            b.close()
            raise
        return b

    def set_original(self, eng, p):
        E, D = self.scaling
        eng.set_original_problem(E, D, p.objective_vector, p.right_hand_side, p.variable_lower_bound, p.variable_upper_bound)

    def close(self):
        for b in (self.batch, self.twin):
            if b is not None:
                b.close()

    def step(self, n):
        args = (n, RED, GROW, self.ss, self.pw, self.it, self.kkt)
        self.twin.take_steps_adaptive(*args)
        self.ss, self.it, self.kkt, _, _ = self.batch.take_steps_adaptive(*args)

    def advance(self):
        """10 steps, the restart point saved on every member, 10 more."""
        self.step(10)
        for eng in list(self.batch.members) + list(self.twin.members):
            eng.save_restart_point()
        self.step(10)
        return self

    def have_average(self, k):
        cx, cy, _, _ = self.twin.members[k].average_info()
        return cx > 0 and cy > 0

    def mixed_points(self):
        """AVERAGE, CURRENT and -1 across the members (every member once where K allows); a member whose average is
        empty is asked for CURRENT."""
        pts = np.array([(AVERAGE, CURRENT, -1)[k % 3] for k in range(self.K)], dtype=np.int32)
        for k in range(self.K):
            if pts[k] == AVERAGE and not self.have_average(k):
                pts[k] = CURRENT
        return pts


@pytest.fixture
def rig_of(gpu_required):
    rigs = []

    def make(problems):
        rigs.append(_Rig(problems))
        return rigs[-1]
    yield make
    for r in rigs:
        r.close()


def _delta(batch, before):
    now = batch.check_info()
    return {k: now[k] - before[k] for k in now}


# ---- eval_points ----

def _check_eval(rig, points, label):
    batch, twin = rig.batch, rig.twin
    before = batch.check_info()
    rows = batch.eval_points(points)
    asked = [k for k in range(rig.K) if points[k] >= 0]
    d = _delta(batch, before)
    assert d["calls"] == 1 and d["carried"] == len(asked) and d["misses"] == 0 and d["served"] == 0, (label, d)
    for k in range(rig.K):
        if points[k] < 0:
            assert not rows[k].any(), label                   # the row of a member left alone keeps the binding's zeros
            continue
        mem, tw, pt = batch.members[k], twin.members[k], int(points[k])
        want = tw.eval_point(pt)
        assert _same(rows[k], want), f"{label}: member {k}: {rows[k]} != {want}"
        for q in ([AVERAGE, CURRENT] if rig.have_average(k) else [CURRENT]):
            assert _same(mem.distance_to_restart(q), tw.distance_to_restart(q)), f"{label}: member {k}: distance {q}"
        assert _same(mem.point_sumsq(pt), tw.point_sumsq(pt)), f"{label}: member {k}: sumsq"
        assert _same(mem.eval_point(pt), want), f"{label}: member {k}: its own eval_point"
    d = _delta(batch, before)
    assert d["served"] == len(asked) and d["misses"] == 0 and d["calls"] == 1, (label, d)


@pytest.mark.parametrize("shape,K", CASES)
def test_eval_points_are_the_twin_members_eval_points(rig_of, shape, K):
    rig = rig_of(SHAPES[shape](K)).advance()
    points = rig.mixed_points()
    _check_eval(rig, points, f"{shape} K={K}")
    # the members left alone evaluate as their twins, through their own call: a miss each
    alone = [k for k in range(K) if points[k] < 0]
    before = rig.batch.check_info()
    for k in alone:
        assert _same(rig.batch.members[k].eval_point(CURRENT), rig.twin.members[k].eval_point(CURRENT)), k
    assert _delta(rig.batch, before)["misses"] == len(alone)
    # -1 through the raw call: the rows of out keep what they held
    sentinel = np.full(24 * K, 12345.678)
    raw = sentinel.copy()
    nobody = np.full(K, -1, dtype=np.int32)
    _lib.check(_lib.lib().pdhg_batch_eval_points(rig.batch._h, nobody.ctypes.data_as(_int_p),
                                                 raw.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))
    assert _same(raw, sentinel)
    # every member at CURRENT next (the products of another point kind, the average only for the distances)
    rig.step(3)
    _check_eval(rig, np.full(K, CURRENT, dtype=np.int32), f"{shape} K={K}, all current")


# ---- point_products, then the members' trust-region searches ----

TR_RADII, TR_RANGES = [0.0, 0.3, 1e6], [0, 1, 2]


def _searches(eng, have_avg):
    pts = [CURRENT, AVERAGE if have_avg else CURRENT, RESTART]
    return [eng.trust_region_bounds(pts, 1.7, 0.6, TR_RADII, TR_RANGES, approximate) for approximate in (False, True)]


def _all_items(rig):
    return [(k, p) for k in range(rig.K) for p in POINTS if p != AVERAGE or rig.have_average(k)]


@pytest.mark.parametrize("shape,K", CASES)
def test_point_products_feed_the_members_searches(rig_of, shape, K):
    rig = rig_of(SHAPES[shape](K)).advance()
    batch, twin = rig.batch, rig.twin
    items = _all_items(rig)
    before = batch.check_info()
    batch.point_products(items)
    d = _delta(batch, before)
    assert d["calls"] == 1 and d["batched"] == len(items) and d["own"] == 0 and d["cached"] == 0, d
    launches = len({p for _, p in items}) * (1 + (3 if shape.startswith("qp") else 2))
    assert d["launches"] == launches, d                     # per point kind: the pack kernel and one launch per matrix
    batch.point_products(items)                             # a second identical call finds every item cached
    d = _delta(batch, before)
    assert d["calls"] == 2 and d["cached"] == len(items) and d["batched"] == len(items) and d["launches"] == launches, d
    for k in range(K):
        got, want = _searches(batch.members[k], rig.have_average(k)), _searches(twin.members[k], rig.have_average(k))
        for g, w in zip(got, want):
            assert _same(g, w), f"{shape} K={K}: member {k}: {g} != {w}"
    # ... and the evaluation after the products finds them cached and still gives the twin's bits
    _check_eval(rig, rig.mixed_points(), f"{shape} K={K} after point_products")


@pytest.mark.parametrize("transpose", [False, True], ids=["long_row", "long_column"])
def test_a_product_with_a_long_row_is_served_per_member(rig_of, transpose):
    K = 3
    rig = rig_of(_family(_long_lp(transpose), K, seed=31)).advance()
    batch, twin = rig.batch, rig.twin
    A = rig.problems[0].constraint_matrix
    lim = H.bitexact_row_limit()
    assert (np.diff(sp.csr_matrix(A).indptr).max() == lim + 1) != transpose and (np.diff(sp.csc_matrix(A).indptr).max() == lim + 1) == transpose
    items = _all_items(rig)
    before = batch.check_info()
    batch.point_products(items)
    d = _delta(batch, before)
    # every item: one product in the batched launch, the one with the long row by the member's own launch
    assert d["batched"] == len(items) and d["own"] == len(items) and d["cached"] == 0, d
    assert d["launches"] == len({p for _, p in items}) * (1 + 1) + len(items), d     # per point kind: pack + the batched product; one own launch per item
    for k in range(K):
        for g, w in zip(_searches(batch.members[k], rig.have_average(k)), _searches(twin.members[k], rig.have_average(k))):
            assert _same(g, w), f"member {k}: {g} != {w}"
    rig.step(2)
    _check_eval(rig, rig.mixed_points(), "long " + ("column" if transpose else "row"))


# ---- the average materialised as a side effect ----

TINY = {
    "lp2x3": lambda: _family(random_lp(2, 3, 2, seed=41), 2, seed=42),
    "qp2x3": lambda: random_qp_family(2, 3, 2, seed=43, nnz_per_row=2),
}


@pytest.mark.parametrize("shape", sorted(TINY))
def test_an_average_materialised_for_the_distances_is_the_members_own(rig_of, shape):
    """An evaluation at CURRENT asks for no products at AVERAGE, yet materialises the average (for the distances) and
    marks it fresh.  What the member then does at AVERAGE on its own -- the point, the distances, a search, whose
    products it computes itself from that average -- is the twin's, and its products are then fresh for the batch too,
    until the next step."""
    K = 2
    rig = rig_of(TINY[shape]())
    p = rig.problems[0]
    assert (p.num_constraints, p.num_variables, p.num_equalities) == (2, 3, 1) and rig.K == K
    rig.step(4)
    batch, twin = rig.batch, rig.twin
    assert all(rig.have_average(k) for k in range(K))
    before = batch.check_info()
    batch.eval_points(np.full(K, CURRENT, dtype=np.int32))
    assert _delta(batch, before)["carried"] == K
    bound = (AVERAGE, 1.7, 0.6, 0.3, 0)
    for k in range(K):
        mem, tw = batch.members[k], twin.members[k]
        for g, w in zip(mem.get_point(AVERAGE), tw.get_point(AVERAGE)):
            assert _same(g, w), f"{shape}: member {k}: the average {g} != {w}"
        assert _same(mem.distance_to_restart(AVERAGE), tw.distance_to_restart(AVERAGE)), f"{shape}: member {k}: distance"
        for approximate in (False, True):
            got, want = mem.trust_region_bound(*bound, approximate), tw.trust_region_bound(*bound, approximate)
            assert _same(got, want), f"{shape}: member {k}: {got} != {want}"
        before = batch.check_info()
        batch.point_products([(k, AVERAGE)])                 # (the member's own bound has just computed them)
        d = _delta(batch, before)
        assert d["cached"] == 1 and d["launches"] == 0, (shape, k, d)
    rig.step(1)
    for k in range(K):
        before = batch.check_info()
        batch.point_products([(k, AVERAGE)])
        d = _delta(batch, before)
        assert d["cached"] == 0 and d["launches"] > 0, (shape, k, d)
        got, want = batch.members[k].trust_region_bound(*bound), twin.members[k].trust_region_bound(*bound)
        assert _same(got, want), f"{shape}: member {k} after a step: {got} != {want}"


# ---- invalidation ----

def _expect_miss(rig, k, point, label):
    before = rig.batch.check_info()
    got, want = rig.batch.members[k].eval_point(point), rig.twin.members[k].eval_point(point)
    assert _same(got, want), f"{label}: {got} != {want}"
    d = _delta(rig.batch, before)
    assert d["misses"] == 1 and d["served"] == 0, (label, d)


@pytest.mark.parametrize("shape", ["700x500", "qp700x500"])
def test_a_stored_result_is_forgotten_when_the_member_moves(rig_of, shape):
    K = 3
    rig = rig_of(SHAPES[shape](K)).advance()
    batch, twin = rig.batch, rig.twin
    everyone = np.full(K, AVERAGE, dtype=np.int32)
    for k in range(K):
        assert rig.have_average(k)

    def store():
        before = batch.check_info()
        batch.eval_points(everyone)
        for k in range(K):
            assert _same(batch.members[k].eval_point(AVERAGE), twin.members[k].eval_point(AVERAGE))
        d = _delta(batch, before)
        assert d["served"] == K and d["misses"] == 0, d
    store()
    rig.step(1)                                               # another batched step
    for k in range(K):
        _expect_miss(rig, k, AVERAGE, f"after a step, member {k}")
    store()
    for b in (batch, twin):                                    # new vectors of member 1 alone
        b.update_problem_vectors(right_hand_sides=[None, rig.problems[1].right_hand_side * 1.01, None])
    _expect_miss(rig, 1, AVERAGE, "after an update")
    before = batch.check_info()
    assert _same(batch.members[0].eval_point(AVERAGE), twin.members[0].eval_point(AVERAGE))
    assert _delta(batch, before)["served"] == 1                # (a member the update did not touch keeps its result)
    store()
    for eng, p in ((b.members[2], rig.problems[2]) for b in (batch, twin)):   # the original problem of member 2 again
        rig.set_original(eng, dataclasses.replace(p.copy(), objective_vector=p.objective_vector * 1.5))
    _expect_miss(rig, 2, AVERAGE, "after set_original_problem")
    store()
    rng = np.random.default_rng(3)
    n, m = rig.problems[0].num_variables, rig.problems[0].num_constraints
    xs, ys = [rng.random(n), None, None], [rng.standard_normal(m), None, None]
    for b in (batch, twin):                                    # a warm start of member 0 alone
        b.warm_start(xs, ys)
    _expect_miss(rig, 0, CURRENT, "after a warm start")
    before = batch.check_info()
    assert _same(batch.members[1].eval_point(AVERAGE), twin.members[1].eval_point(AVERAGE))
    assert _delta(batch, before)["served"] == 1
    # the batch goes on as the twin does
    rig.step(4)
    pts = np.array([CURRENT, AVERAGE, AVERAGE], dtype=np.int32)
    _check_eval(rig, pts, shape + " after the warm start")


# ---- refusals ----

def _refused(call, words):
    with pytest.raises(_lib.PdhgHipError) as info:
        call()
    assert "error -1" in str(info.value) and any(w in str(info.value) for w in words), str(info.value)


def test_refusals_leave_the_handle_as_it_was(rig_of):
    K = 3
    rig = rig_of(SHAPES["700x500"](K))
    batch, twin = rig.batch, rig.twin
    L = _lib.lib()
    before = batch.check_info()
    # not a batch handle: a member
    member = batch.members[0]._h
    ints = np.zeros(3, dtype=np.int32)
    out = np.zeros(24 * K)
    for rc in (L.pdhg_batch_point_products(member, 1, ints.ctypes.data_as(_int_p), ints.ctypes.data_as(_int_p)),
               L.pdhg_batch_eval_points(member, ints.ctypes.data_as(_int_p), out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))),
               L.pdhg_batch_check_info(member, np.zeros(8, dtype=np.int64).ctypes.data_as(ctypes.POINTER(ctypes.c_int64)))):
        assert rc == -1 and b"not a batch handle" in L.pdhg_last_error()
    # the average is empty before the first step
    _refused(lambda: batch.point_products([(0, CURRENT), (1, AVERAGE)]), ["average is empty"])
    _refused(lambda: batch.eval_points([CURRENT, AVERAGE, -1]), ["average is empty"])
    rig.advance()
    _refused(lambda: batch.point_products([(0, CURRENT), (K, CURRENT)]), ["member index out of range"])
    _refused(lambda: batch.point_products([(0, CURRENT), (-1, CURRENT)]), ["member index out of range"])
    _refused(lambda: batch.point_products([(0, CURRENT), (1, 3)]), ["unknown point selector"])
    _refused(lambda: batch.point_products([(0, CURRENT), (1, -1)]), ["unknown point selector"])
    _refused(lambda: batch.eval_points([CURRENT, 7, -1]), ["unknown point selector"])
    _refused(lambda: batch.point_products([(k % K, CURRENT) for k in range(3 * 32 + 1)]), ["count must be 1..96"])
    for count in (0, -1):
        assert L.pdhg_batch_point_products(batch._h, count, ints.ctypes.data_as(_int_p), ints.ctypes.data_as(_int_p)) == -1
        assert b"count must be 1..96" in L.pdhg_last_error()
    # a member without its original problem: a fresh batch
    fresh = HipPdhgBatch.from_problems(rig.problems)
    try:
        _refused(lambda: fresh.eval_points([CURRENT, -1, -1]), ["pdhg_set_original_problem has not been called"])
        assert not any(fresh.check_info().values())
    finally:
        fresh.close()
    assert batch.check_info() == before                       # nothing was counted, launched or stored
    # a valid call of each kind next: the twin's bits
    _check_eval(rig, rig.mixed_points(), "after the refusals")
    batch.point_products(_all_items(rig))
    for k in range(K):
        for g, w in zip(_searches(batch.members[k], True), _searches(twin.members[k], True)):
            assert _same(g, w), k


@pytest.mark.parametrize("switch", ["PDHG_EVAL_PREFETCH", "PDHG_EVAL_HOST_WORD"])
def test_with_a_development_switch_of_the_evaluation_every_member_is_served_by_its_own_call(rig_of, monkeypatch, switch):
    """The shared launches restate the one-handle form with its prefetched distances; with that form switched off the
    call serves every member through the member's own ``pdhg_eval_point`` (no miss of the caller's) and stores nothing
    that could answer for another form."""
    K = 3
    rig = rig_of(SHAPES["700x500"](K)).advance()
    monkeypatch.setenv(switch, "0")
    points = rig.mixed_points()
    before = rig.batch.check_info()
    rows = rig.batch.eval_points(points)
    d = _delta(rig.batch, before)
    assert d["calls"] == 1 and d["carried"] == 0 and d["misses"] == 0 and d["launches"] == 0, d
    for k in range(K):
        if points[k] >= 0:
            want = rig.twin.members[k].eval_point(int(points[k]))
            assert _same(rows[k], want), k
            assert _same(rig.batch.members[k].eval_point(int(points[k])), want), k
    monkeypatch.delenv(switch)
    _check_eval(rig, points, "after the switch is gone")


# ---- whole solves ----

def _params(limit=400, tol=1e-6, freq=40):
    tc = construct_termination_criteria(eps_optimal_absolute=tol, eps_optimal_relative=tol, iteration_limit=limit)
    rp = construct_restart_parameters(RestartScheme.ADAPTIVE_NORMALIZED, RestartToCurrentMetric.GAP_OVER_DISTANCE_SQUARED,
                                      1000, 0.5, 0.1, 0.9, 0.5, False)
    return PdhgParameters(10, False, 1.0, 1.0, True, 0, True, freq, tc, rp, AdaptiveStepsizeParams(RED, GROW))


def _pagerank(K=3, n=300):
    rng = np.random.default_rng(2)
    return personalized_pagerank_lps(n, [np.full(n, 1.0 / n)] + [rng.dirichlet(np.ones(n)) for _ in range(K - 1)], seed=3)


def _svm_path():
    X, y = synthetic_rcv1_like(600, 900, 20, seed=3)
    return l1_svm_regularization_path(preprocess_training_data(X), y, [0.1, 0.5, 1.0, 4.0])


FAMILIES = {"pagerank_300": _pagerank, "l1_svm_path": _svm_path, "qp_200x150": lambda: random_qp_family(200, 150, 3, seed=7)}


class _Kept:
    """The default factory with the batch kept open until the test has read its counters."""
    takes_original_problem = True

    def __init__(self):
        self.batch = None

    def __call__(self, problems):
        self.batch = HipPdhgBatch.from_problems(problems)
        self.info = None
        close = self.batch.close

        def closing():
            self.info = self.batch.check_info()
            close()
        self.batch.close = closing
        return self.batch


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_a_solve_with_the_switch_on_is_the_solve_with_it_off(gpu_required, monkeypatch, family):
    problems = FAMILIES[family]()
    params = _params()
    monkeypatch.delenv("PDHG_BATCH_CHECKS", raising=False)
    off_factory = _Kept()
    off = optimize_batch(params, problems, batch_factory=off_factory)
    assert not any(off_factory.info.values()), off_factory.info     # switched off: none of the new calls, no stored result
    monkeypatch.setenv("PDHG_BATCH_CHECKS", "1")
    on_factory = _Kept()
    on = optimize_batch(params, problems, batch_factory=on_factory)
    assert len(on) == len(off) == len(problems)
    for g, w in zip(on, off):
        H.assert_same_output(g, w)
    info = on_factory.info
    assert info["misses"] == 0 and info["calls"] > 0 and info["carried"] > 0 and info["served"] == info["carried"], info
    assert info["batched"] + info["own"] > 0, info


@pytest.mark.parametrize("family", ["pagerank_300", "qp_200x150"])
def test_a_session_with_the_switch_on_is_the_session_with_it_off(gpu_required, monkeypatch, family):
    problems = FAMILIES[family]()
    params = _params(limit=200)
    update = [{"right_hand_side": p.right_hand_side * (1.0 + 0.01 * (k + 1))} if k != 1 else None for k, p in enumerate(problems)]

    def run(value):
        if value is None:
            monkeypatch.delenv("PDHG_BATCH_CHECKS", raising=False)
        else:
            monkeypatch.setenv("PDHG_BATCH_CHECKS", value)
        with PdhgBatchSession(params, problems) as session:
            first = session.solve()
            session.update(update)
            cold = session.solve()
            warm = session.solve(warm_start=True)
            return first, cold, warm, session.batch.check_info()
    *off, info_off = run(None)
    *on, info_on = run("1")
    assert not any(info_off.values()), info_off
    for got, want in zip(on, off):
        for g, w in zip(got, want):
            H.assert_same_output(g, w)
    assert info_on["misses"] == 0 and info_on["carried"] > 0 and info_on["served"] == info_on["carried"], info_on
