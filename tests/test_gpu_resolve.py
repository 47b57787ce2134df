"""Re-solves on the device (include/pdhg_hip_resolve.h, firstorderlp.jl_amd/session.py).

* replay: after ``update_problem_vectors`` the working vectors are, bit for bit, those of a fresh engine created from the
  updated problem and rescaled with the same parameters -- at 0, 1 and 12 rescaling steps, at the sizes around the wave
  and the workgroup, at the first length with a second grid-stride trip, for every NULL / given combination, with
  bounds that hold +-inf, +-0.0 and lb == ub, and with the compact bound views following the bounds;
* a session's cold or warm solve after an update is ``optimize`` on the updated problem, bit for bit, on every step path;
* ``optimize(..., initial_*)`` on the device against the CPU oracle;
* a fleet session in shared launches; refusals that launch nothing."""
import dataclasses

import numpy as np
import pytest
import scipy.sparse as sp

from firstorderlp_jl_amd import (HipPdhgBatch, HipPdhgEngine, HipPdhgFleet, PdhgFleetSession, PdhgSession, _lib,
                                 linear_programming_problem, optimize_many)
from firstorderlp_jl_amd.engine import _MemberEngine
from firstorderlp_jl_amd.generators import pagerank_lp, random_lp, random_qp_family
from firstorderlp_jl_amd.primal_dual_hybrid_gradient import (AdaptiveStepsizeParams, ConstantStepsizeParams,
                                                             MalitskyPockStepsizeParameters, PdhgParameters, optimize)
from firstorderlp_jl_amd.saddle_point import (RestartScheme, RestartToCurrentMetric,
                                              construct_restart_parameters)
from firstorderlp_jl_amd.solve_log import RestartChoice
from firstorderlp_jl_amd.termination import construct_termination_criteria
from tests import helpers as H
from tests.helpers import (assert_same_output as _assert_same, bits as _bits, edge_bounds as _edge_bounds,
                           raises_naming as _raises_naming, same_bits as _same_bits)
from tests.oracle_engine import OracleEngine

pytestmark = pytest.mark.gpu

RESCALINGS = {0: (0, False, None), 1: (0, False, 1.0), 12: (10, True, 1.0)}      # applied steps -> (Ruiz, L2, Pock-Chambolle alpha)
EW_FIRST_SECOND_TRIP = 2048 * 256 + 1          # EW_MAX_BLOCKS * TPB + 1: an elementwise thread's second grid-stride trip


def _params(policy=None, tol=1e-6, limit=64, freq=8, steps=12):
    ruiz, l2, pc = RESCALINGS[steps]
    tc = construct_termination_criteria(eps_optimal_absolute=tol, eps_optimal_relative=tol, iteration_limit=limit)
    rp = construct_restart_parameters(RestartScheme.ADAPTIVE_NORMALIZED, RestartToCurrentMetric.GAP_OVER_DISTANCE_SQUARED,
                                      1000, 0.5, 0.1, 0.9, 0.5, False)
    return PdhgParameters(ruiz, l2, pc, 1.0, True, 0, True, freq, tc, rp, policy or AdaptiveStepsizeParams(0.3, 0.6))


def _edge_lp(m, n, seed):
    """An m x n LP (m may be 0) with up to three entries per row and bounds that hold -inf, +inf, +0.0, -0.0 and
    lb == ub."""
    rng = np.random.default_rng(seed)
    k = min(3, n)
    rows = np.repeat(np.arange(m), k)
    cols = np.concatenate([rng.choice(n, size=k, replace=False) for _ in range(m)]) if m else np.zeros(0, dtype=np.int64)
    A = sp.csc_matrix((rng.uniform(0.2, 3.0, m * k) * rng.choice([-1.0, 1.0], m * k), (rows, cols)), shape=(m, n))
    lb, ub = _edge_bounds(n, rng)
    return linear_programming_problem(lb, ub, rng.standard_normal(n), 0.0, A, rng.standard_normal(m), m // 2)


def _new_vectors(problem, seed):
    rng = np.random.default_rng(seed)
    lb, ub = _edge_bounds(problem.num_variables, rng)
    return {"objective_vector": rng.standard_normal(problem.num_variables), "right_hand_side": rng.standard_normal(problem.num_constraints),
            "variable_lower_bound": lb, "variable_upper_bound": ub}


def _fresh_vectors(problem, steps):
    eng = HipPdhgEngine.from_problem(problem)
    try:
        eng.rescale(*RESCALINGS[steps])
        return eng.get_problem_vectors()
    finally:
        eng.close()


def _retained(problem, steps):
    eng = HipPdhgEngine.from_problem(problem)
    eng.retain_rescaling()
    E, D = eng.rescale(*RESCALINGS[steps])
    return eng, E, D


# ---- replay and views ----

SHAPES = [(0, 5), (1, 257), (63, 64), (64, 1), (65, 255), (255, 63), (256, 65), (257, 256)]      # (rows, columns)


@pytest.mark.parametrize("steps", [0, 1, 12])
def test_updated_vectors_are_those_of_a_fresh_rescale(gpu_required, steps):
    for m, n in SHAPES:
        problem = _edge_lp(m, n, seed=100 * m + n)
        eng, _, _ = _retained(problem, steps)
        try:
            _same_bits(eng.get_problem_vectors(), _fresh_vectors(problem, steps), f"{m}x{n} retained")      # (retention changes nothing)
            new = _new_vectors(problem, seed=m + 7 * n)
            eng.update_problem_vectors(**new)
            _same_bits(eng.get_problem_vectors(), _fresh_vectors(dataclasses.replace(problem.copy(), **new), steps), f"{m}x{n} S={steps}")
        finally:
            eng.close()


def test_every_combination_of_given_and_kept_vectors(gpu_required):
    problem = _edge_lp(65, 255, seed=5)
    new = _new_vectors(problem, seed=6)
    names = ("objective_vector", "right_hand_side", "variable_lower_bound", "variable_upper_bound")
    old_scaled = dict(zip(names, _fresh_vectors(problem, 12)))
    new_scaled = dict(zip(names, _fresh_vectors(dataclasses.replace(problem.copy(), **new), 12)))
    eng, _, _ = _retained(problem, 12)
    try:
        for mask in range(16):
            given = {k: new[k] for q, k in enumerate(names) if mask >> q & 1}
            eng.update_problem_vectors(**given)
            want = [(new_scaled if k in given else old_scaled)[k] for k in names]
            _same_bits(eng.get_problem_vectors(), want, f"mask {mask}")
            eng.update_problem_vectors(**{k: getattr(problem, k) for k in names})       # back to the start
            _same_bits(eng.get_problem_vectors(), [old_scaled[k] for k in names], f"mask {mask} restored")
    finally:
        eng.close()


@pytest.mark.short_rows
def test_the_first_length_with_a_second_grid_stride_trip(gpu_required):
    n = EW_FIRST_SECOND_TRIP
    rng = np.random.default_rng(11)
    A = sp.diags(rng.uniform(0.5, 4.0, n) * rng.choice([-1.0, 1.0], n)).tocsc()          # one entry per row
    problem = linear_programming_problem(np.zeros(n), np.full(n, np.inf), rng.standard_normal(n), 0.0, A, rng.standard_normal(n), n // 2)
    new = {"objective_vector": rng.standard_normal(n), "right_hand_side": rng.standard_normal(n),
           "variable_lower_bound": rng.choice([-np.inf, 0.0, -2.0], n), "variable_upper_bound": rng.choice([np.inf, 0.0, 5.0], n)}
    eng, E, D = _retained(problem, 12)
    try:
        eng.update_problem_vectors(**new)
        _same_bits(eng.get_problem_vectors(), _fresh_vectors(dataclasses.replace(problem.copy(), **new), 12), "n = 524289")
        x0, y0 = rng.standard_normal(n), rng.standard_normal(n)
        eng.warm_start(x0, y0)
        x, y = eng.get_current()
        assert np.array_equal(_bits(x), _bits(x0 * D)) and np.array_equal(_bits(y), _bits(y0 * E))
        assert np.array_equal(_bits(eng.get_dual_product()), _bits(eng.spmv_t(y0 * E)))
    finally:
        eng.close()


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


def _assert_views_and_trial(eng, fresh_problem, point, want_mode, label):
    fresh = HipPdhgEngine.from_problem(fresh_problem)
    try:
        fresh.rescale(*RESCALINGS[12])
        a, b = eng.layout_info(), fresh.layout_info()
        for key in ("lb_mode", "ub_mode", "lb_exceptions", "ub_exceptions"):
            assert a[key] == b[key], (label, key, a[key], b[key])
        assert a["lb_mode"] == want_mode == a["ub_mode"], (label, a["lb_mode"], a["ub_mode"])
        for g, w in zip(_trial_bits(eng, point), _trial_bits(fresh, point)):
            assert np.array_equal(g, w), label
    finally:
        fresh.close()


def test_the_bound_views_follow_the_bounds(gpu_required, monkeypatch):
    monkeypatch.setenv("PDHG_COOP", "0")             # the trial through primal_kernel, which reads the views
    monkeypatch.setenv("PDHG_DEVICE_LOOP", "0")
    problem = _view_problem()
    rng = np.random.default_rng(4)
    point = (rng.standard_normal(problem.num_variables), rng.standard_normal(problem.num_constraints))
    eng, _, _ = _retained(problem, 12)
    try:
        for k, (mode, lb, ub) in enumerate(_view_updates(problem.num_variables)):
            eng.update_problem_vectors(variable_lower_bound=lb, variable_upper_bound=ub)
            updated = dataclasses.replace(problem.copy(), variable_lower_bound=lb, variable_upper_bound=ub)
            _assert_views_and_trial(eng, updated, point, mode, f"update {k} -> {mode}")
    finally:
        eng.close()


def test_a_fleet_update_rebuilds_the_views_where_they_are_next_read(gpu_required, monkeypatch):
    monkeypatch.setenv("PDHG_COOP", "0")
    monkeypatch.setenv("PDHG_DEVICE_LOOP", "0")
    problems = [_view_problem(seed=3), _view_problem(seed=4), _view_problem(n=200, m=30, seed=5)]
    rng = np.random.default_rng(4)
    fleet = HipPdhgFleet.from_problems(problems)
    try:
        for eng in fleet.members:
            eng.retain_rescaling()
            eng.rescale(*RESCALINGS[12])
        rebuilt = 0
        for k, (mode, lb, ub) in enumerate(_view_updates(300)):
            # members 0 and 1 get new bounds, member 2 a new objective vector only: its views stay
            fleet.update_problem_vectors(objective_vectors=[None, None, problems[2].objective_vector * (k + 2)],
                                         variable_lower_bounds=[lb, lb, None], variable_upper_bounds=[ub, ub, None])
            info = fleet.resolve_info()
            assert info["shared_launches"] == k + 1 and info["carried"] == 3 and info["view_rebuilds"] == rebuilt
            updated = dataclasses.replace(problems[0].copy(), variable_lower_bound=lb, variable_upper_bound=ub)
            point = (rng.standard_normal(300), rng.standard_normal(40))
            _assert_views_and_trial(fleet.members[0], updated, point, mode, f"fleet update {k} -> {mode}")
            rebuilt += 1                         # member 0's views, at its layout_info / trial; member 1's wait
            assert fleet.resolve_info()["view_rebuilds"] == rebuilt
        a = fleet.members[1].layout_info()       # member 1: six updates, one rebuild
        assert a["lb_mode"] == a["ub_mode"] == "const" and fleet.resolve_info()["view_rebuilds"] == rebuilt + 1
        c2 = fleet.members[2].get_problem_vectors()
        want = _fresh_vectors(dataclasses.replace(problems[2].copy(), objective_vector=problems[2].objective_vector * 7), 12)
        _same_bits(c2, want, "member 2")
        assert fleet.resolve_info()["view_rebuilds"] == rebuilt + 1
    finally:
        fleet.close()


# ---- a cold re-solve is a fresh solve; a warm one a fresh warm solve ----

def _perturbed(problem, seed=7, bound=True):
    rng = np.random.default_rng(seed)
    update = {"right_hand_side": problem.right_hand_side * (1 + 0.01 * rng.uniform(-1, 1, problem.num_constraints))}
    if bound:
        ub = problem.variable_upper_bound.copy()
        ub[::7] = np.where(np.isfinite(ub[::7]), ub[::7] * 1.25, 12.0)
        update["variable_upper_bound"] = ub
    return update


def _series(params, problem, update=None, warm_points=()):
    """solve; update; solve cold (and warm from each of ``warm_points``) against ``optimize`` on the updated problem.
    Returns (first output, the fresh solve's output, the session engine's [steps_info, trial_graph])."""
    update = update if update is not None else _perturbed(problem)
    updated = dataclasses.replace(problem.copy(), **update)
    with PdhgSession(params, problem) as session:
        first = session.solve()
        session.update(**update)
        want = optimize(params, updated)
        _assert_same(session.solve(), want)
        for x0, y0 in warm_points:
            _assert_same(session.solve(warm_start=(x0, y0)),
                         optimize(params, updated, initial_primal_solution=x0, initial_dual_solution=y0))
        return first, want, (session.engine.steps_info(), session.engine.layout_info()["trial_graph"])


def _medium():
    return random_lp(3000, 2500, 4, seed=2)


def _small_qp():
    return random_qp_family(40, 48, 1, seed=3, nnz_per_row=4)[0]


# name -> (environment, problem, what the session's engine must report afterwards: (steps_info, trial_graph) -> bool)
PATHS = {"small_lp": ({}, lambda: random_lp(27, 32, 4, seed=1), lambda si, tg: si[0] > 0),
         "small_lp_off": ({"PDHG_SMALL_LP": "0"}, lambda: random_lp(27, 32, 4, seed=1), lambda si, tg: si[0] == 0),
         "steps_kernel": ({"PDHG_DEVICE_LOOP": "1", "PDHG_SMALL_LP": "0"}, _medium, lambda si, tg: si[0] == 0 and si[1] > 0 and tg == 2),
         "device_loop_off": ({"PDHG_DEVICE_LOOP": "0", "PDHG_SMALL_LP": "0"}, _medium, lambda si, tg: si[:2] == [0, 0] and tg == 2),
         "graph": ({"PDHG_DEVICE_LOOP": "0", "PDHG_COOP": "0", "PDHG_SMALL_LP": "0"}, _medium, lambda si, tg: si[:2] == [0, 0] and tg == 1),
         "qp": ({}, _small_qp, lambda si, tg: si[0] == 0),
         "small_qp": ({"PDHG_SMALL_QP": "1"}, _small_qp, lambda si, tg: si[0] > 0)}


@pytest.mark.parametrize("path", sorted(PATHS))
def test_a_cold_resolve_is_a_fresh_solve_on_every_step_path(gpu_required, monkeypatch, path):
    env, maker, took_the_path = PATHS[path]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    problem = maker()
    rng = np.random.default_rng(9)
    point = (rng.uniform(0, 1, problem.num_variables), rng.standard_normal(problem.num_constraints))
    _, _, (steps_info, trial_graph) = _series(_params(limit=60, freq=8), problem, warm_points=[point])
    assert took_the_path(steps_info, trial_graph), (path, steps_info, trial_graph)


@pytest.mark.parametrize("policy", [AdaptiveStepsizeParams(0.3, 0.6), ConstantStepsizeParams(), MalitskyPockStepsizeParameters(0.7, 0.99, 1.0)],
                         ids=["adaptive", "constant", "malitsky_pock"])
def test_every_step_size_policy(gpu_required, policy):
    problem = random_lp(27, 32, 4, seed=1)
    rng = np.random.default_rng(10)
    point = (rng.uniform(0, 1, 32), rng.standard_normal(27))
    _series(_params(policy, limit=90, freq=8), problem, warm_points=[point])


def test_no_state_is_left_over_from_the_solve_before(gpu_required):
    """The first solve ends PRIMAL_INFEASIBLE / at the iteration limit inside a batch of steps / after restarts to the
    average; the second solve, of a feasible update, is the fresh solve of that problem."""
    bad = H.example_lp()
    bad.right_hand_side[2] = 8
    params = _params(limit=800, freq=5, tol=1e-8)
    first, _, _ = _series(params, bad, update={"right_hand_side": np.array([12.0, 7.0, 1.0])})
    assert first.termination_string == "PRIMAL_INFEASIBLE"
    params = _params(limit=43, freq=8)                        # 43 = 5 * 8 + 3: the limit falls inside a batch
    first, _, _ = _series(params, random_lp(27, 32, 4, seed=1))
    assert first.termination_string == "ITERATION_LIMIT" and first.iteration_count == 43
    params = _params(limit=600, freq=5, tol=1e-9)
    first, second, _ = _series(params, H.example_lp(), update={"right_hand_side": np.array([12.1, 6.9, 1.0])})
    assert any(s.restart_used == RestartChoice.RESTART_CHOICE_RESTART_TO_AVERAGE for s in first.iteration_stats)


@pytest.mark.parametrize("which", ["x_only", "y_only", "neither"])
def test_partial_starting_points(gpu_required, which):
    problem = random_lp(27, 32, 4, seed=1)
    update = _perturbed(problem)
    updated = dataclasses.replace(problem.copy(), **update)
    rng = np.random.default_rng(12)
    x0 = rng.uniform(0, 1, 32) if which == "x_only" else None
    y0 = rng.standard_normal(27) if which == "y_only" else None
    params = _params(limit=60, freq=8)
    with PdhgSession(params, problem) as session:
        session.solve()
        session.update(**update)
        if which == "neither":
            session.engine.warm_start(None, None)
            fresh = HipPdhgEngine.from_problem(updated)
            try:
                fresh.rescale(*RESCALINGS[12])
                for g, w in zip(session.engine.get_current() + (session.engine.get_dual_product(),),
                                fresh.get_current() + (fresh.get_dual_product(),)):
                    assert np.array_equal(_bits(g), _bits(w))               # (+0.0 everywhere, the dual product included)
            finally:
                fresh.close()
            _assert_same(session.solve(warm_start=(None, None)), optimize(params, updated))
        else:
            _assert_same(session.solve(warm_start=(x0, y0)),
                         optimize(params, updated, initial_primal_solution=x0, initial_dual_solution=y0))


@pytest.mark.parametrize("name,maker", [("pagerank300", lambda: pagerank_lp(300, seed=3)), ("example_lp", H.example_lp)])
def test_a_warm_start_from_the_last_solution_takes_fewer_iterations(gpu_required, name, maker):
    """Chosen on the CPU with the oracle engine (1 % perturbation of b, seed 7, tolerance 1e-6): cold 368 / warm 144
    iterations for the PageRank LP, 560 / 168 for the reference's example LP."""
    problem = maker()
    params = dataclasses.replace(_params(tol=1e-6, limit=40000, freq=8), l2_norm_rescaling=False)     # (as chosen on the CPU)
    update = _perturbed(problem, seed=7, bound=False)
    counts = []
    for warm in (None, True):
        with PdhgSession(params, problem) as session:
            session.solve()
            session.update(**update)
            out = session.solve(warm_start=warm)
            assert out.termination_string == "OPTIMAL"
            counts.append(out.iteration_count)
    print(f"{name}: cold {counts[0]} iterations, warm {counts[1]}")
    assert counts[1] < counts[0]


# ---- against the oracle ----

@pytest.mark.parametrize("name,maker", [("random", lambda: random_lp(300, 280, 4, seed=42)), ("pagerank", lambda: pagerank_lp(2000, seed=3))])
def test_a_warm_device_solve_matches_the_warm_host_solve(gpu_required, name, maker):
    tol = 1e-6
    problem = maker()
    rough = optimize(_params(tol=1e-2, limit=40000, freq=40, steps=1), problem, OracleEngine.from_problem)
    x0, y0 = rough.primal_solution, rough.dual_solution
    params = _params(tol=tol, limit=60000, freq=40, steps=1)
    params = dataclasses.replace(params, l_inf_ruiz_iterations=10)
    dev = optimize(params, problem, initial_primal_solution=x0, initial_dual_solution=y0)
    host = optimize(params, problem, OracleEngine.from_problem, initial_primal_solution=x0, initial_dual_solution=y0)
    assert dev.termination_string == host.termination_string == "OPTIMAL"
    cd, ch = dev.iteration_stats[-1].convergence_information[0], host.iteration_stats[-1].convergence_information[0]
    scale = 1.0 + abs(ch.primal_objective)
    print(f"{name}: iterations device {dev.iteration_count} host {host.iteration_count}; objectives {cd.primal_objective} {ch.primal_objective}")
    assert abs(cd.primal_objective - ch.primal_objective) <= 50 * tol * scale
    assert abs(cd.dual_objective - ch.dual_objective) <= 50 * tol * scale
    assert 0.5 <= dev.iteration_count / host.iteration_count <= 2.0, (dev.iteration_count, host.iteration_count)
    assert np.linalg.norm(dev.primal_solution - host.primal_solution) <= 0.05 * (1.0 + np.linalg.norm(host.primal_solution))


# ---- fleets ----

def _mixed_problems():
    """Twelve members: small LPs, two beyond the check class (n + m > 4096), one without rows, a QP."""
    out = [random_lp(27, 32, 4, seed=s) for s in range(1, 6)]
    out += [random_lp(56, 97, 4, seed=6), random_lp(2500, 2000, 4, seed=7), H.example_lp()]
    n = 12
    out.append(linear_programming_problem(np.zeros(n), np.arange(1.0, n + 1), np.linspace(-1, 1, n), 0.0, sp.csc_matrix((0, n)), np.zeros(0), 0))
    out += [random_qp_family(40, 48, 1, seed=3, nnz_per_row=4)[0], random_lp(2300, 2100, 4, seed=8), random_lp(100, 120, 5, seed=9)]
    return out


def _fleet_update(p, seed):
    if p.num_constraints == 0:
        return {"objective_vector": p.objective_vector * 0.5, "variable_upper_bound": p.variable_upper_bound + 1.0}
    return _perturbed(p, seed=seed)


def test_a_fleet_session_of_mixed_members(gpu_required):
    problems = _mixed_problems()
    K = len(problems)
    assert K == 12
    params = _params(limit=40, freq=8)
    rng = np.random.default_rng(21)
    with PdhgFleetSession(params, problems) as session:
        fleet = session.fleet
        first = session.solve()
        # update all, solve warm from points
        updates = [_fleet_update(p, seed=k) for k, p in enumerate(problems)]
        session.update(updates)
        info = fleet.resolve_info()
        assert info["shared_launches"] == 2 and info["carried"] == K, info      # (the first solve's warm start, the update)
        updated = [dataclasses.replace(p.copy(), **u) for p, u in zip(problems, updates)]
        points = [(rng.uniform(0, 1, p.num_variables), rng.standard_normal(p.num_constraints)) for p in updated]
        got = session.solve(warm_start=points)
        info = fleet.resolve_info()
        assert info["shared_launches"] == 3 and info["carried"] == K and info["single"] >= 2, info
        for g, p, (x0, y0) in zip(got, updated, points):
            _assert_same(g, optimize(params, p, initial_primal_solution=x0, initial_dual_solution=y0))
        # views are rebuilt lazily, at most once per member whose bounds an update wrote
        rebuilds = fleet.resolve_info()["view_rebuilds"]
        assert rebuilds <= K, rebuilds
        # update a subset; the others are untouched
        subset = [_fleet_update(p, seed=50 + k) if k % 3 == 0 else None for k, p in enumerate(updated)]
        before = [eng.get_problem_vectors() for eng in fleet.members]
        session.update(subset)
        assert fleet.resolve_info()["carried"] == sum(u is not None for u in subset)
        for k, (eng, u) in enumerate(zip(fleet.members, subset)):
            if u is None:
                _same_bits(eng.get_problem_vectors(), before[k], f"member {k} untouched")
        updated2 = [p if u is None else dataclasses.replace(p.copy(), **u) for p, u in zip(updated, subset)]
        got = session.solve()
        for g, p in zip(got, updated2):
            _assert_same(g, optimize(params, p))
        rebuilds2 = fleet.resolve_info()["view_rebuilds"]
        assert rebuilds2 - rebuilds <= sum(u is not None for u in subset), (rebuilds, rebuilds2)
        # an update that writes no bound leaves every view alone
        session.update([{"objective_vector": p.objective_vector * 1.01} for p in updated2])
        session.solve()
        assert fleet.resolve_info()["view_rebuilds"] == rebuilds2
        updated2 = session.problems
        # warm start a subset through the fleet's own call: the others keep their state
        state = [eng.get_current() + (eng.get_dual_product(), eng.average_info()) for eng in fleet.members]
        xs = [rng.uniform(0, 1, p.num_variables) if k % 2 == 0 else None for k, p in enumerate(updated2)]
        ys = [rng.standard_normal(p.num_constraints) if k % 4 == 0 else None for k, p in enumerate(updated2)]
        fleet.warm_start(xs, ys)
        assert fleet.resolve_info()["carried"] == K // 2
        for k, eng in enumerate(fleet.members):
            now = eng.get_current() + (eng.get_dual_product(), eng.average_info())
            if k % 2:
                assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(now[:3], state[k][:3])) and now[3] == state[k][3], k
            else:
                assert now[3] == (0, 0, 0.0, 0.0), k
    assert len(first) == K


@pytest.mark.parametrize("K", [1, 300])
def test_fleet_sessions_of_one_and_of_more_members_than_compute_units(gpu_required, K):
    base = random_lp(27, 32, 4, seed=1)
    rng = np.random.default_rng(K)
    problems = [dataclasses.replace(base.copy(), objective_vector=base.objective_vector + 0.05 * rng.standard_normal(32)) for _ in range(K)]
    params = _params(limit=40, freq=8)
    with PdhgFleetSession(params, problems) as session:
        session.solve()
        updates = [_perturbed(p, seed=k) for k, p in enumerate(problems)]
        session.update(updates)
        got = session.solve(warm_start=True)
        info = session.fleet.resolve_info()
        assert info["shared_launches"] == 3 and info["carried"] == K and info["single"] == 0 and info["view_rebuilds"] <= K, info
        last = [(g.primal_solution, g.dual_solution) for g in session.solve()]
        again = session.solve(warm_start=True)
    updated = [dataclasses.replace(p.copy(), **u) for p, u in zip(problems, updates)]
    want = optimize_many(params, updated, initial_solutions=last)
    for g, w in zip(again, want):
        _assert_same(g, w)
    assert len(got) == K


# ---- refusals launch nothing ----

def test_refusals_launch_nothing_and_leave_the_handle_usable(gpu_required):
    problem = random_lp(27, 32, 4, seed=1)
    params = _params(limit=40, freq=8)
    want = optimize(params, problem)
    eng = HipPdhgEngine.from_problem(problem)
    try:
        eng.rescale(*RESCALINGS[12])
        before = eng.get_problem_vectors(), eng.steps_info()
        _raises_naming(_lib.PdhgHipError, ["pdhg_resolve_retain"], lambda: eng.update_problem_vectors(right_hand_side=problem.right_hand_side))
        _raises_naming(_lib.PdhgHipError, ["pdhg_resolve_retain"], lambda: eng.warm_start(None, None))
        _same_bits(eng.get_problem_vectors(), before[0], "not retained")
        assert eng.steps_info() == before[1]
    finally:
        eng.close()
    _raises_naming(_lib.PdhgHipError, ["closed"], lambda: eng.update_problem_vectors(right_hand_side=problem.right_hand_side))
    _raises_naming(_lib.PdhgHipError, ["closed"], lambda: eng.warm_start(None, None))
    _raises_naming(_lib.PdhgHipError, ["closed"], eng.retain_rescaling)

    with PdhgSession(params, problem) as session:
        eng = session.engine
        for kw in ({"right_hand_side": np.zeros(26)}, {"objective_vector": np.zeros(33)}, {"variable_lower_bound": np.zeros((32, 1))}):
            _raises_naming(ValueError, ["entries", "shape"], lambda: eng.update_problem_vectors(**kw))
        _raises_naming(ValueError, ["entries"], lambda: eng.warm_start(np.zeros(31), None))
        _raises_naming(ValueError, ["entries"], lambda: eng.warm_start(None, np.zeros(28)))
        _raises_naming(ValueError, ["shape"], lambda: session.update(right_hand_side=np.zeros(5)))
        _raises_naming(ValueError, ["shape"], lambda: session.solve(warm_start=(np.zeros(5), None)))
        assert eng.steps_info() == [0, 0, 0, 0]
        _assert_same(session.solve(), want)                   # the handle still solves
    _raises_naming(RuntimeError, ["closed"], session.solve)
    _raises_naming(RuntimeError, ["closed"], lambda: session.update(right_hand_side=problem.right_hand_side))

    family = [problem, dataclasses.replace(problem.copy(), objective_vector=problem.objective_vector * 2)]
    batch = HipPdhgBatch.from_problems(family)
    try:
        whole = _MemberEngine._wrap(batch._L, batch._h, batch.m, batch.n)          # (a view: the batch frees the handle)
        for target, word in ((whole, "batch handle"), (batch.members[0], "batch member")):
            _raises_naming(_lib.PdhgHipError, [word], target.retain_rescaling)
            _raises_naming(_lib.PdhgHipError, [word], lambda: target.update_problem_vectors(right_hand_side=problem.right_hand_side))
            _raises_naming(_lib.PdhgHipError, [word], lambda: target.warm_start(None, None))
        assert batch.members[0].steps_info() == [0, 0, 0, 0]
    finally:
        batch.close()

    group = HipPdhgEngine.from_problem(problem, device_ids=[0, 0])
    try:
        _raises_naming(_lib.PdhgHipError, ["shard group"], group.retain_rescaling)
        _raises_naming(_lib.PdhgHipError, ["shard group"], lambda: group.warm_start(None, None))
        assert group.steps_info() == [0, 0, 0, 0]
    finally:
        group.close()

    fleet = HipPdhgFleet.from_problems(family)
    try:
        fleet.members[0].retain_rescaling()
        for eng in fleet.members:
            eng.rescale(*RESCALINGS[12])
        counters = fleet.info(), fleet.resolve_info()
        b = problem.right_hand_side
        _raises_naming(_lib.PdhgHipError, ["member 1", "pdhg_resolve_retain"], lambda: fleet.update_problem_vectors(right_hand_sides=[b, b]))
        _raises_naming(_lib.PdhgHipError, ["member 1"], lambda: fleet.warm_start(None, None))
        _raises_naming(ValueError, ["entries"], lambda: fleet.update_problem_vectors(right_hand_sides=[b]))
        _raises_naming(ValueError, ["entries"], lambda: fleet.warm_start([np.zeros(31), None], None))
        _raises_naming(_lib.PdhgHipError, ["fleet"], lambda: _MemberEngine._wrap(fleet._L, fleet._h, 27, 32).warm_start(None, None))
        assert (fleet.info(), fleet.resolve_info()) == counters
        fleet.update_problem_vectors(right_hand_sides=[b * 1.01, None])           # member 0 alone is fine
        assert fleet.resolve_info()["carried"] == 1
    finally:
        fleet.close()
    _raises_naming(_lib.PdhgHipError, ["closed"], lambda: fleet.warm_start(None, None))
    _raises_naming(_lib.PdhgHipError, ["closed"], fleet.resolve_info)
