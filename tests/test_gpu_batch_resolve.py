"""Re-solves of a batch on the device (include/pdhg_hip_batch_resolve.h, ``HipPdhgBatch``, ``PdhgBatchSession``).

* replay: after ``update_problem_vectors`` every member's working vectors are, bit for bit, those of a fresh rescaled
  ``HipPdhgBatch`` built from the updated problems -- at 0, 1 and 12 rescaling steps, at member counts around the
  replay's tile of four and the interleave's power of two, at sizes around the wave and the workgroup, for every
  given / kept combination side by side in one call, with bounds that hold +-inf, +-0.0 and lb == ub;
* warm start: the scaled point and A'y bitwise, through the batched product where every column is within the row
  order's sequential limit and through the members' own products where one is not; subsets;
* a session's cold or warm solve after an update is ``optimize_batch`` on the updated problems, bit for bit;
* refusals that launch nothing."""
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
from tests import helpers as H
from tests.helpers import (assert_same_output as _assert_same, bits as _bits, edge_bounds as _edge_bounds,
                           raises_naming as _raises_naming, same_bits as _same_bits)

pytestmark = pytest.mark.gpu

RESCALINGS = {0: (0, False, None), 1: (0, False, 1.0), 12: (10, True, 1.0)}      # applied steps -> (Ruiz, L2, Pock-Chambolle alpha)
EW_FIRST_SECOND_TRIP = 2048 * 256 + 1          # EW_MAX_BLOCKS * TPB + 1: an elementwise thread's second grid-stride trip
NAMES = ("objective_vector", "right_hand_side", "variable_lower_bound", "variable_upper_bound")
PLURAL = ("objective_vectors", "right_hand_sides", "variable_lower_bounds", "variable_upper_bounds")


def _params(policy=None, tol=1e-6, limit=64, freq=8, steps=12):
    ruiz, l2, pc = RESCALINGS[steps]
    tc = construct_termination_criteria(eps_optimal_absolute=tol, eps_optimal_relative=tol, iteration_limit=limit)
    rp = construct_restart_parameters(RestartScheme.ADAPTIVE_NORMALIZED, RestartToCurrentMetric.GAP_OVER_DISTANCE_SQUARED,
                                      1000, 0.5, 0.1, 0.9, 0.5, False)
    return PdhgParameters(ruiz, l2, pc, 1.0, True, 0, True, freq, tc, rp, policy or AdaptiveStepsizeParams(0.3, 0.6))


def _assert_all_same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        _assert_same(g, w)


def _edge_vectors(m, n, rng):
    lb, ub = _edge_bounds(n, rng)
    return {"objective_vector": rng.standard_normal(n), "right_hand_side": rng.standard_normal(m),
            "variable_lower_bound": lb, "variable_upper_bound": ub}


def _edge_matrix(m, n, rng):
    """m x n (m may be 0) with up to three entries per row."""
    k = min(3, n)
    rows = np.repeat(np.arange(m), k)
    cols = np.concatenate([rng.choice(n, size=k, replace=False) for _ in range(m)]) if m else np.zeros(0, dtype=np.int64)
    return sp.csc_matrix((rng.uniform(0.2, 3.0, m * k) * rng.choice([-1.0, 1.0], m * k), (rows, cols)), shape=(m, n))


def _family_on(A, K, rng, num_eq=None):
    m, n = A.shape
    out = []
    for _ in range(K):
        v = _edge_vectors(m, n, rng)
        out.append(linear_programming_problem(v["variable_lower_bound"], v["variable_upper_bound"], v["objective_vector"], 0.0,
                                              A, v["right_hand_side"], m // 2 if num_eq is None else num_eq))
    return out


def _replaced(problems, updates):
    return [p if not u else dataclasses.replace(p.copy(), **u) for p, u in zip(problems, updates)]


def _retained(problems, steps):
    batch = HipPdhgBatch.from_problems(problems)
    try:
        batch.retain_rescaling()
        batch.retain_rescaling()                  # (a second call is a no-op)
        E, D = batch.rescale(*RESCALINGS[steps])
    except Exception:
        batch.close()
        raise
    return batch, E, D


def _fresh_vectors(problems, steps):
    """Every member's working vectors in a fresh batch of ``problems`` rescaled the same way."""
    batch = HipPdhgBatch.from_problems(problems)
    try:
        batch.rescale(*RESCALINGS[steps])
        return [eng.get_problem_vectors() for eng in batch.members]
    finally:
        batch.close()


def _update(batch, updates):
    """``updates``: one dict (or None) per member, keyed like ``dataclasses.replace`` takes them."""
    batch.update_problem_vectors(**{plural: [None if not u else u.get(name) for u in updates] for name, plural in zip(NAMES, PLURAL)})


# ---- replay ----

SHAPES = [(0, 5), (1, 257), (63, 64), (65, 255), (257, 256)]      # (rows, columns)


@pytest.mark.short_rows
@pytest.mark.parametrize("K", [1, 2, 3, 5, 32])
@pytest.mark.parametrize("steps", [0, 1, 12])
def test_updated_members_hold_the_vectors_of_a_fresh_rescaled_batch(gpu_required, steps, K):
    for m, n in SHAPES:
        rng = np.random.default_rng(1000 * K + 100 * m + n)
        problems = _family_on(_edge_matrix(m, n, rng), K, rng)
        batch, _, _ = _retained(problems, steps)
        try:
            label = f"{m}x{n} K={K} S={steps}"
            for got, want in zip([e.get_problem_vectors() for e in batch.members], _fresh_vectors(problems, steps)):
                _same_bits(got, want, label + " retained")              # (retention changes nothing)
            updates = [_edge_vectors(m, n, rng) for _ in range(K)]
            _update(batch, updates)
            info = batch.resolve_info()
            assert info["shared_launches"] == 1 and info["carried"] == K, info
            fresh = _fresh_vectors(_replaced(problems, updates), steps)
            for k, eng in enumerate(batch.members):
                _same_bits(eng.get_problem_vectors(), fresh[k], f"{label} member {k}")
        finally:
            batch.close()


@pytest.mark.short_rows
def test_every_combination_of_given_and_kept_vectors_side_by_side(gpu_required):
    """Sixteen members, member k given the vectors of mask k in ONE call (mask 0: not carried, untouched), then the
    masks rotated, so that every combination also meets other neighbours in its tile."""
    m, n, K = 65, 255, 16
    rng = np.random.default_rng(5)
    problems = _family_on(_edge_matrix(m, n, rng), K, rng)
    new = [_edge_vectors(m, n, rng) for _ in range(K)]
    old_scaled = _fresh_vectors(problems, 12)
    new_scaled = _fresh_vectors(_replaced(problems, new), 12)
    batch, _, _ = _retained(problems, 12)
    try:
        launches = 0
        for shift in (0, 5, 11):
            masks = [(k + shift) % 16 for k in range(K)]
            _update(batch, [{name: new[k][name] for q, name in enumerate(NAMES) if masks[k] >> q & 1} for k in range(K)])
            launches += 1
            info = batch.resolve_info()
            assert info["shared_launches"] == launches and info["carried"] == 15, info
            for k, eng in enumerate(batch.members):
                want = [(new_scaled if masks[k] >> q & 1 else old_scaled)[k][q] for q in range(4)]
                _same_bits(eng.get_problem_vectors(), want, f"shift {shift} member {k} mask {masks[k]}")
            _update(batch, [{name: getattr(p, name) for name in NAMES} for p in problems])          # back to the start
            launches += 1
            for k, eng in enumerate(batch.members):
                _same_bits(eng.get_problem_vectors(), old_scaled[k], f"shift {shift} member {k} restored")
        _update(batch, [None] * K)                                           # nothing given: nothing launched
        info = batch.resolve_info()
        assert info["shared_launches"] == launches and info["carried"] == 0, info
    finally:
        batch.close()


@pytest.mark.short_rows
def test_the_first_length_with_a_second_grid_stride_trip(gpu_required):
    n, K = EW_FIRST_SECOND_TRIP, 2
    rng = np.random.default_rng(11)
    A = sp.diags(rng.uniform(0.5, 4.0, n) * rng.choice([-1.0, 1.0], n)).tocsc()          # one entry per row
    problems = [linear_programming_problem(np.zeros(n), np.full(n, np.inf), rng.standard_normal(n), 0.0, A, rng.standard_normal(n), n // 2)
                for _ in range(K)]
    updates = [{"objective_vector": rng.standard_normal(n), "right_hand_side": rng.standard_normal(n),
                "variable_lower_bound": rng.choice([-np.inf, 0.0, -2.0], n), "variable_upper_bound": rng.choice([np.inf, 0.0, 5.0], n)}
               for _ in range(K)]
    batch, E, D = _retained(problems, 12)
    try:
        _update(batch, updates)
        fresh = _fresh_vectors(_replaced(problems, updates), 12)
        for k, eng in enumerate(batch.members):
            _same_bits(eng.get_problem_vectors(), fresh[k], f"n = {n} member {k}")
        xs, ys = [rng.standard_normal(n) for _ in range(K)], [rng.standard_normal(n) for _ in range(K)]
        batch.warm_start(xs, ys)
        assert batch.resolve_info()["batched_product"] == 1
        for k, eng in enumerate(batch.members):
            x, y = eng.get_current()
            assert np.array_equal(_bits(x), _bits(xs[k] * D)) and np.array_equal(_bits(y), _bits(ys[k] * E)), k
            assert np.array_equal(_bits(eng.get_dual_product()), _bits(eng.spmv_t(ys[k] * E))), k
    finally:
        batch.close()


# ---- warm starts ----

def _column_matrix(m, counts, rng):
    """m rows; column j holds counts[j] entries in random rows."""
    rows = np.concatenate([rng.choice(m, size=c, replace=False) for c in counts]) if sum(counts) else np.zeros(0, dtype=np.int64)
    cols = np.repeat(np.arange(len(counts)), counts)
    vals = rng.uniform(0.2, 3.0, len(rows)) * rng.choice([-1.0, 1.0], len(rows))
    return sp.csc_matrix((vals, (rows, cols)), shape=(m, len(counts)))


def _assert_warm_point(batch, E, D, xs, ys):
    for k, eng in enumerate(batch.members):
        x, y = eng.get_current()
        want_x = np.zeros(batch.n) if xs[k] is None else xs[k] * D
        want_y = np.zeros(batch.m) if ys[k] is None else ys[k] * E
        assert np.array_equal(_bits(x), _bits(want_x)), f"member {k}: x"
        assert np.array_equal(_bits(y), _bits(want_y)), f"member {k}: y"
        want_aty = np.zeros(batch.n) if ys[k] is None else eng.spmv_t(want_y)
        assert np.array_equal(_bits(eng.get_dual_product()), _bits(want_aty)), f"member {k}: A'y"
        assert eng.average_info() == (0, 0, 0.0, 0.0), k


@pytest.mark.parametrize("steps", [0, 12])
def test_columns_within_the_sequential_limit_take_the_batched_product(gpu_required, steps):
    rng = np.random.default_rng(21)
    m, K = 300, 3
    A = _column_matrix(m, [0, 1, 7, 8, 9, 256] * 7, rng)
    problems = _family_on(A, K, rng)
    batch, E, D = _retained(problems, steps)
    try:
        xs = [rng.standard_normal(batch.n) for _ in range(K)]
        ys = [rng.standard_normal(m) for _ in range(K)]
        batch.warm_start(xs, ys)
        info = batch.resolve_info()
        assert info == {"shared_launches": 2, "carried": K, "single": 0, "batched_product": 1}, info
        _assert_warm_point(batch, E, D, xs, ys)
        # a mask of some members: member 1 gets x only (no product: +0.0), member 2 y only
        xs, ys = [xs[0], rng.standard_normal(batch.n), None], [ys[0] * 0.5, None, rng.standard_normal(m)]
        batch.warm_start(xs, ys)
        info = batch.resolve_info()
        assert info == {"shared_launches": 4, "carried": K, "single": 0, "batched_product": 1}, info
        _assert_warm_point(batch, E, D, xs, ys)
        batch.warm_start(None, None)                               # everyone from zeros: no product at all
        info = batch.resolve_info()
        assert info == {"shared_launches": 5, "carried": K, "single": 0, "batched_product": 0}, info
        _assert_warm_point(batch, E, D, [None] * K, [None] * K)
    finally:
        batch.close()


def test_a_column_beyond_the_sequential_limit_takes_the_members_own_products(gpu_required):
    rng = np.random.default_rng(22)
    m, K = 2100, 3
    A = _column_matrix(m, [3, 2049, 1, 0, 40, 8], rng)
    problems = _family_on(A, K, rng)
    batch, E, D = _retained(problems, 12)
    try:
        xs = [rng.standard_normal(batch.n), None, rng.standard_normal(batch.n)]
        ys = [rng.standard_normal(m), rng.standard_normal(m), None]
        batch.warm_start(xs, ys)
        info = batch.resolve_info()
        assert info == {"shared_launches": 1, "carried": K, "single": 2, "batched_product": 0}, info
        _assert_warm_point(batch, E, D, xs, ys)
    finally:
        batch.close()


@pytest.mark.short_rows
def test_a_warm_start_of_a_subset_leaves_the_others_as_they_are(gpu_required):
    problems = _lp_family(random_lp(27, 32, 4, seed=1), 4, seed=2)
    rng = np.random.default_rng(23)
    batch, E, D = _retained(problems, 12)
    try:
        batch.warm_start([rng.uniform(0, 1, 32) for _ in range(4)], [rng.standard_normal(27) for _ in range(4)])
        batch.take_steps_adaptive(5, 0.3, 0.6, np.full(4, 0.05), np.ones(4), np.zeros(4, dtype=np.int64), np.zeros(4))
        state = [eng.get_current() + (eng.get_dual_product(), eng.average_info()) for eng in batch.members]
        assert all(s[3][0] > 0 for s in state), [s[3] for s in state]              # (the averages are not empty)
        x1, y3 = rng.uniform(0, 1, 32), rng.standard_normal(27)
        batch.warm_start([None, x1, None, None], [None, None, None, y3])
        info = batch.resolve_info()
        assert info["carried"] == 2 and info["single"] == 0 and info["batched_product"] == 1, info
        for k in (0, 2):
            eng = batch.members[k]
            now = eng.get_current() + (eng.get_dual_product(), eng.average_info())
            assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(now[:3], state[k][:3])) and now[3] == state[k][3], k
        _assert_warm_point(_Members(batch, [1, 3]), E, D, [x1, None], [None, y3])
        assert not _bits(batch.members[1].get_dual_product()).any()                 # +0.0, bit for bit
    finally:
        batch.close()


class _Members:
    """Some members of a batch where ``_assert_warm_point`` expects a batch."""

    def __init__(self, batch, which):
        self.members, self.n, self.m = [batch.members[k] for k in which], batch.n, batch.m


# ---- a cold re-solve is a fresh solve; a warm one a fresh warm solve ----

def _lp_family(p, K, seed):
    """K LPs on p's matrix with their own c, b and upper bounds."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(K):
        c = p.objective_vector * (1.0 + 0.5 * rng.random(p.num_variables)) if k else p.objective_vector.copy()
        b = p.right_hand_side * (1.0 + 0.05 * rng.random(p.num_constraints)) if k else p.right_hand_side.copy()
        out.append(linear_programming_problem(p.variable_lower_bound.copy(), p.variable_upper_bound + k, c, 0.0,
                                              p.constraint_matrix, b, p.num_equalities))
    return out


def _perturbed(problem, seed, bound=True):
    rng = np.random.default_rng(seed)
    update = {"right_hand_side": problem.right_hand_side * (1 + 0.01 * rng.uniform(-1, 1, problem.num_constraints))}
    if bound:
        ub = problem.variable_upper_bound.copy()
        ub[::7] = np.where(np.isfinite(ub[::7]), ub[::7] * 1.25, 12.0)
        update["variable_upper_bound"] = ub
    return update


FAMILIES = {"lp_27x32": lambda: _lp_family(random_lp(27, 32, 4, seed=1), 3, seed=2),
            "lp_3000x2500": lambda: _lp_family(random_lp(3000, 2500, 4, seed=2), 2, seed=3),
            "qp_40x48": lambda: random_qp_family(40, 48, 3, seed=3, nnz_per_row=4)}


@pytest.mark.parametrize("policy", [AdaptiveStepsizeParams(0.3, 0.6), ConstantStepsizeParams()], ids=["adaptive", "constant"])
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_a_session_solve_is_optimize_batch_on_the_updated_problems(gpu_required, family, policy):
    problems = FAMILIES[family]()
    K = len(problems)
    params = _params(policy, limit=48, freq=8)
    rng = np.random.default_rng(9)
    with PdhgBatchSession(params, problems) as session:
        _assert_all_same(session.solve(), optimize_batch(params, problems))
        updates = [_perturbed(p, seed=k) for k, p in enumerate(problems)]
        updates[-1] = {"objective_vector": problems[-1].objective_vector * 1.1}          # (no bound: its views stay)
        session.update(updates)
        info = session.batch.resolve_info()
        assert info["shared_launches"] == 2 and info["carried"] == K, info               # (the first solve's warm start, the update)
        updated = _replaced(problems, updates)
        _assert_all_same(session.solve(), optimize_batch(params, updated))
        points = [(rng.uniform(0, 1, p.num_variables), rng.standard_normal(p.num_constraints)) for p in updated]
        points[0] = (points[0][0], None)
        if K > 2:
            points[1] = None
        got = session.solve(warm_start=points)
        info = session.batch.resolve_info()
        assert info["carried"] == K and info["single"] == 0 and info["batched_product"] == 1, info
        _assert_all_same(got, optimize_batch(params, updated, initial_solutions=points))
        last = [(g.primal_solution, g.dual_solution) for g in got]
        _assert_all_same(session.solve(warm_start=True), optimize_batch(params, updated, initial_solutions=last))
        # an update of one member alone
        session.update([None] * (K - 1) + [_perturbed(updated[-1], seed=77)])
        assert session.batch.resolve_info()["carried"] == 1
        _assert_all_same(session.solve(), optimize_batch(params, session.problems))


@pytest.mark.short_rows
def test_no_state_is_left_over_from_the_solve_before(gpu_required):
    """The first solve ends PRIMAL_INFEASIBLE for one member, and at the iteration limit inside a batch of steps for
    all; the next solve, of an update, is the fresh solve of those problems."""
    good = H.example_lp()
    bad = good.copy()
    bad.right_hand_side = good.right_hand_side.copy()
    bad.right_hand_side[2] = 8
    other = dataclasses.replace(good.copy(), objective_vector=good.objective_vector * 1.5)
    params = _params(limit=800, freq=5, tol=1e-8)
    with PdhgBatchSession(params, [bad, good, other]) as session:
        first = session.solve()
        assert first[0].termination_string == "PRIMAL_INFEASIBLE"
        session.update([{"right_hand_side": np.array([12.0, 7.0, 1.0])}, None, {"right_hand_side": np.array([12.1, 6.9, 1.0])}])
        cold = session.solve()
        _assert_all_same(cold, optimize_batch(params, session.problems))
        _assert_all_same(session.solve(warm_start=True), optimize_batch(
            params, session.problems, initial_solutions=[(g.primal_solution, g.dual_solution) for g in cold]))
    problems = _lp_family(random_lp(27, 32, 4, seed=1), 3, seed=2)
    params = _params(limit=43, freq=8)                        # 43 = 5 * 8 + 3: the limit falls inside a batch of steps
    with PdhgBatchSession(params, problems) as session:
        first = session.solve()
        assert all(f.termination_string == "ITERATION_LIMIT" and f.iteration_count == 43 for f in first)
        session.update([_perturbed(p, seed=k) for k, p in enumerate(problems)])
        _assert_all_same(session.solve(), optimize_batch(params, session.problems))


def _view_problem(n=300, m=40, seed=3):
    p = random_lp(m, n, 4, seed=seed)
    p.variable_lower_bound = np.zeros(n)
    p.variable_upper_bound = np.full(n, np.inf)
    return p


def _view_updates(n):
    """Bounds that move lb / ub between the CONST, SPARSE and DENSE views, both ways."""
    rng = np.random.default_rng(2)
    few, many = np.zeros(n), rng.uniform(-1.0, 0.0, n)
    few[rng.choice(n, n // 10, replace=False)] = -0.5
    ufew, umany = np.full(n, np.inf), rng.uniform(1.0, 2.0, n)
    ufew[rng.choice(n, n // 8, replace=False)] = 4.0
    return [("sparse", few, ufew), ("dense", many, umany), ("sparse", few, ufew), ("const", np.zeros(n), np.full(n, np.inf)),
            ("dense", many, umany), ("const", np.zeros(n), np.full(n, np.inf))]


def _trial_bits(eng, point, step=0.3, weight=1.1):
    eng.set_current(*point)
    raw = eng.trial_step(step, weight, 1.0)
    return [_bits(raw)] + [_bits(v) for v in eng.get_trial()]


@pytest.mark.short_rows
def test_the_bound_views_of_a_member_follow_its_bounds(gpu_required, monkeypatch):
    """The batch's update marks a member's views stale; the member's OWN trial (primal_kernel reads the views) rebuilds
    them first and gives the bits of a fresh batch's member."""
    monkeypatch.setenv("PDHG_DEVICE_LOOP", "0")
    base = _view_problem()
    problems = [base, dataclasses.replace(base.copy(), objective_vector=base.objective_vector * 2.0)]
    rng = np.random.default_rng(4)
    point = (rng.standard_normal(base.num_variables), rng.standard_normal(base.num_constraints))
    batch, _, _ = _retained(problems, 12)
    try:
        for k, (mode, lb, ub) in enumerate(_view_updates(base.num_variables)):
            update = {"variable_lower_bound": lb, "variable_upper_bound": ub}
            _update(batch, [update, None])
            fresh = HipPdhgBatch.from_problems(_replaced(problems, [update, None]))
            try:
                fresh.rescale(*RESCALINGS[12])
                a, b = batch.members[0].layout_info(), fresh.members[0].layout_info()
                for key in ("lb_mode", "ub_mode", "lb_exceptions", "ub_exceptions"):
                    assert a[key] == b[key], (k, key, a[key], b[key])
                assert a["lb_mode"] == mode == a["ub_mode"], (k, mode, a["lb_mode"], a["ub_mode"])
                assert batch.members[1].layout_info()["lb_mode"] == "const"                   # (member 1's bounds never move)
                for g, w in zip(_trial_bits(batch.members[0], point), _trial_bits(fresh.members[0], point)):
                    assert np.array_equal(g, w), f"update {k} -> {mode}"
                # ... and the batched trial, which reads the dense arrays
                for eng in batch.members + fresh.members:
                    eng.set_current(*point)
                assert np.array_equal(_bits(batch.trial_step(0.3, 1.1)), _bits(fresh.trial_step(0.3, 1.1))), k
            finally:
                fresh.close()
    finally:
        batch.close()


# ---- refusals launch nothing ----

@pytest.mark.short_rows
def test_refusals_launch_nothing_and_leave_the_batch_usable(gpu_required):
    problems = _lp_family(random_lp(27, 32, 4, seed=1), 3, seed=2)
    b, x = problems[0].right_hand_side, np.zeros(32)
    L = _lib.lib()

    def counters(batch):
        return batch.resolve_info(), [eng.steps_info() for eng in batch.members]

    batch = HipPdhgBatch.from_problems(problems)
    try:
        batch.rescale(*RESCALINGS[12])
        before = [eng.get_problem_vectors() for eng in batch.members], counters(batch)
        _raises_naming(_lib.PdhgHipError, ["pdhg_batch_resolve_retain"], lambda: batch.update_problem_vectors(right_hand_sides=[b, b, b]))
        _raises_naming(_lib.PdhgHipError, ["pdhg_batch_resolve_retain"], lambda: batch.warm_start(None, None))
        _raises_naming(_lib.PdhgHipError, ["pdhg_batch_resolve_retain"], lambda: batch.warm_start([x, None, None], None))
        for eng, want in zip(batch.members, before[0]):
            _same_bits(eng.get_problem_vectors(), want, "not retained")
        assert counters(batch) == before[1]
    finally:
        batch.close()
    _raises_naming(_lib.PdhgHipError, ["closed"], lambda: batch.update_problem_vectors(right_hand_sides=[b, b, b]))
    _raises_naming(_lib.PdhgHipError, ["closed"], lambda: batch.warm_start(None, None))
    _raises_naming(_lib.PdhgHipError, ["closed"], batch.retain_rescaling)
    _raises_naming(_lib.PdhgHipError, ["closed"], batch.resolve_info)

    params = _params(limit=40, freq=8)
    want = optimize_batch(params, problems)
    with PdhgBatchSession(params, problems) as session:
        batch = session.batch
        before = counters(batch)
        for kw in ({"right_hand_sides": [b, b]}, {"objective_vectors": [None] * 4}, {"right_hand_sides": [b, np.zeros(26), None]},
                   {"objective_vectors": [np.zeros(33), None, None]}, {"variable_lower_bounds": [None, None, np.zeros((32, 1))]}):
            _raises_naming(ValueError, ["entries"], lambda: batch.update_problem_vectors(**kw))
        _raises_naming(ValueError, ["entries"], lambda: batch.warm_start([x, x], None))
        _raises_naming(ValueError, ["entries"], lambda: batch.warm_start([np.zeros(31), None, None], None))
        _raises_naming(ValueError, ["entries"], lambda: batch.warm_start(None, [None, np.zeros(28), None]))
        _raises_naming(ValueError, ["entries"], lambda: session.update([None, None]))
        _raises_naming(ValueError, ["shape"], lambda: session.update([{"right_hand_side": np.zeros(5)}, None, None]))
        _raises_naming(ValueError, ["shape"], lambda: session.solve(warm_start=[(np.zeros(5), None), None, None]))
        assert counters(batch) == before
        _assert_all_same(session.solve(), want)                   # the batch still solves
        # the calls of one handle keep refusing the batch and its members, now with a pointer to the batch's calls
        _raises_naming(_lib.PdhgHipError, ["batch member"], lambda: batch.members[0].warm_start(None, None))
        _raises_naming(_lib.PdhgHipError, ["batch member"], batch.members[0].retain_rescaling)
    _raises_naming(RuntimeError, ["closed"], session.solve)

    # a plain handle and a fleet handle passed to the batch's calls
    table = (_lib._dp * 3)()
    info = np.zeros(4, dtype=np.int64)
    plain = HipPdhgEngine.from_problem(problems[0])
    fleet = HipPdhgFleet.from_problems(problems[:2])
    try:
        plain.retain_rescaling()
        plain.rescale(*RESCALINGS[12])
        for handle, steps_info in ((plain._h, plain.steps_info), (fleet._h, fleet.members[0].steps_info)):
            at_start = steps_info()
            for rc in (L.pdhg_batch_resolve_retain(handle), L.pdhg_batch_update_problem_vectors(handle, table, table, None, None),
                       L.pdhg_batch_warm_start(handle, None, None), L.pdhg_batch_warm_start(handle, table, table),
                       L.pdhg_batch_resolve_info(handle, info.ctypes.data_as(_lib._ip))):
                assert rc == -1 and b"not a batch handle" in L.pdhg_last_error()
            assert steps_info() == at_start and not info.any()
    finally:
        plain.close()
        fleet.close()
