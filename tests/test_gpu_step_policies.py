"""The constant and the Malitsky-Pock policy in batches on the device (pdhg_take_steps_constant / _malitsky_pock, their
fleet forms).  Three paths must give the same bits -- the Python loops (PDHG_PY_TAKE_STEP=1), the host loop in C
(PDHG_SMALL_LP=0) and the one-workgroup LDS kernel (PDHG_SMALL_LP=1; csrc/small_lp_kernel.hpp) -- at the kernel's own
edges, and the LDS kernel must match the oracle in exact-sums mode.  Every comparison is np.array_equal."""
import numpy as np
import pytest

from firstorderlp_jl_amd import HipPdhgEngine, _lib, linear_programming_problem
from firstorderlp_jl_amd.fleet import HipPdhgFleet, optimize_many
from firstorderlp_jl_amd.generators import random_lp
from firstorderlp_jl_amd.primal_dual_hybrid_gradient import (ConstantStepsizeParams, MalitskyPockStepsizeParameters,
                                                             PdhgParameters, PdhgSolverState, optimize, take_step,
                                                             take_steps)
from tests import helpers as H

pytestmark = pytest.mark.gpu

CONSTANT = ConstantStepsizeParams()
MALITSKY_POCK = MalitskyPockStepsizeParameters(0.7, 0.99, 1.0)
POLICIES = pytest.mark.parametrize("policy", [CONSTANT, MALITSKY_POCK], ids=["constant", "malitsky_pock"])
PATHS = ("py", "c", "lds")
BATCHES = [1, 2, 3, 64, 200]


def _start(p, policy):
    """(step size, primal weight): pdhg.jl:821-826 for the line search; for the constant policy a step size that is safe
    whatever the matrix, 1 / sqrt(|A|_1 |A|_inf) <= 1 / |A|_2 (the iterates stay finite, so bits can be compared)."""
    step, pw = H.initial_step_and_weight(p)
    if isinstance(policy, ConstantStepsizeParams):
        A = abs(p.constraint_matrix)
        step = 1.0 / np.sqrt(A.sum(axis=0).max() * A.sum(axis=1).max())
    return float(step), float(pw)


def _set_path(monkeypatch, path):
    monkeypatch.setenv("PDHG_PY_TAKE_STEP", "1" if path == "py" else "0")
    monkeypatch.setenv("PDHG_SMALL_LP", "1" if path == "lds" else "0")
    monkeypatch.setenv("PDHG_DEVICE_LOOP", "0")


def _snapshot(eng, st, sizes=()):
    x, y = eng.get_current()
    xa, ya = eng.get_average()
    return (np.array(sizes), np.float64(st.step_size), np.float64(st.ratio_step_sizes), x, y, xa, ya,
            np.array(eng.average_info()), st.total_number_iterations, st.cumulative_kkt_passes, st.numerical_error)


def _run(p, policy, batches, monkeypatch, path, mix=False, step_scale=1.0):
    """Step sizes per batch, step size, ratio, x, y, both averages, average_info, total_number_iterations,
    cumulative_kkt_passes, numerical_error -- and the small-LP launches the engine made."""
    _set_path(monkeypatch, path)
    eng = HipPdhgEngine.from_problem(p)
    step, pw = _start(p, policy)
    st = PdhgSolverState(eng, step_size=step * step_scale, primal_weight=pw, ratio_step_sizes=1.0)
    sizes = []
    for i, k in enumerate(batches):
        if mix and i % 2 == 1:
            for _ in range(k):                 # single steps between the batches: the lazy average update crosses the paths
                take_step(policy, st)
        else:
            done = take_steps(policy, st, k)
            assert done == k or st.numerical_error
        sizes.append(st.step_size)
        if st.numerical_error:
            break
    out = _snapshot(eng, st, sizes)
    launches = eng.steps_info()[0]
    eng.close()
    return out, launches


def _assert_same(ref, got, label):
    for k, (a, b) in enumerate(zip(ref, got)):
        assert np.array_equal(a, b), (label, k)


def _with_num_eq(p, num_eq):
    return linear_programming_problem(p.variable_lower_bound, p.variable_upper_bound, p.objective_vector, 0.0,
                                      p.constraint_matrix, p.right_hand_side, num_eq)


# (maker, does the one-workgroup kernel take it?)  random_lp(m, n, ...): m rows, n columns
SHAPES = {
    "1x1": (lambda: random_lp(1, 1, 1, seed=1), True),
    "1x30": (lambda: random_lp(1, 30, 3, seed=2), True),
    "30x30": (lambda: random_lp(30, 30, 3, seed=1), True),
    "max256": (lambda: random_lp(200, 256, 4, seed=3), True),              # the last shape with 256 threads
    "max257": (lambda: random_lp(257, 200, 4, seed=4), True),              # the first with 1024
    "n1024": (lambda: random_lp(600, 1024, 5, seed=5), True),
    "n1025": (lambda: random_lp(600, 1025, 5, seed=6), True),              # a second stride trip at 1024 threads
    "no_equalities": (lambda: _with_num_eq(random_lp(40, 50, 4, seed=7), 0), True),
    "all_equalities": (lambda: _with_num_eq(random_lp(40, 50, 4, seed=8), 40), True),
    "row256": (lambda: H.rows_with_lens([256] + [4] * 59, 300, seed=9), True),
    "row257": (lambda: H.rows_with_lens([257] + [4] * 59, 300, seed=10), False),   # one entry too many: the C loop
    "lds_full": (lambda: random_lp(1458, 1400, 4, seed=11), True),         # 9n + 4m = 18 432 doubles: 144 KiB
    "lds_over": (lambda: random_lp(1459, 1400, 4, seed=12), False),        # one double past it
}


@POLICIES
@pytest.mark.parametrize("shape", list(SHAPES))
def test_three_paths_give_the_same_bits(gpu_required, monkeypatch, policy, shape):
    maker, eligible = SHAPES[shape]
    p = maker()
    ref, n_py = _run(p, policy, BATCHES, monkeypatch, "py")
    host, n_c = _run(p, policy, BATCHES, monkeypatch, "c")
    lds, n_lds = _run(p, policy, BATCHES, monkeypatch, "lds")
    mixed, _ = _run(p, policy, BATCHES, monkeypatch, "lds", mix=True)
    assert np.all(np.isfinite(ref[3])) and np.all(np.isfinite(ref[4]))
    assert ref[7][1] == sum(BATCHES)
    _assert_same(ref, host, "C loop")
    _assert_same(ref, lds, "LDS kernel")
    _assert_same(ref, mixed, "LDS kernel, single steps in between")
    assert n_py == 0 and n_c == 0
    assert (n_lds > 0) == eligible, n_lds


def test_malitsky_pock_downscales_inside_a_launch(gpu_required, monkeypatch):
    """A first step 300 times too long: the line search rejects trials inside the launches."""
    p = random_lp(300, 250, 5, seed=2)
    ref, _ = _run(p, MALITSKY_POCK, [40, 40, 40], monkeypatch, "py", step_scale=300.0)
    host, _ = _run(p, MALITSKY_POCK, [40, 40, 40], monkeypatch, "c", step_scale=300.0)
    lds, launches = _run(p, MALITSKY_POCK, [40, 40, 40], monkeypatch, "lds", step_scale=300.0)
    _assert_same(ref, host, "C loop")
    _assert_same(ref, lds, "LDS kernel")
    assert ref[8] > 120 and launches == 3        # rejected trials; [first step singly, 39], [40], [40]


def test_sixty_rejections_end_the_call_and_leave_the_state(gpu_required, monkeypatch):
    """breaking_factor = 0 rejects every trial: numerical_error, +60 iterations, +30.5 KKT passes, step size, ratio, x
    and y as they came -- on all three paths."""
    p = random_lp(60, 50, 4, seed=3)
    never = MalitskyPockStepsizeParameters(0.7, 0.0, 1.0)
    outs = []
    for path in PATHS:
        _set_path(monkeypatch, path)
        eng = HipPdhgEngine.from_problem(p)
        step, pw = _start(p, MALITSKY_POCK)
        st = PdhgSolverState(eng, step_size=step, primal_weight=pw, ratio_step_sizes=1.0)
        assert take_steps(MALITSKY_POCK, st, 5) == 5
        before = _snapshot(eng, st)
        assert take_steps(never, st, 4) == 1          # the failing take_step counts, the call ends there
        after = _snapshot(eng, st)
        assert st.numerical_error and not before[10]
        assert after[8] == before[8] + 60 and after[9] == before[9] + 30.5
        _assert_same(before[:8], after[:8], path)
        outs.append(after)
        eng.close()
    _assert_same(outs[0], outs[1], "C loop")
    _assert_same(outs[0], outs[2], "LDS kernel")


def test_the_first_accept_into_an_empty_average_adds_the_current_x(gpu_required, monkeypatch):
    """pdhg.jl:621-627: at the start, after reset_average() in mid-run and after a restart to the average the counts
    come out (k + 1, k), whichever path takes the steps."""
    p = random_lp(80, 70, 4, seed=4)
    outs = []
    for path in PATHS:
        _set_path(monkeypatch, path)
        eng = HipPdhgEngine.from_problem(p)
        step, pw = _start(p, MALITSKY_POCK)
        st = PdhgSolverState(eng, step_size=step, primal_weight=pw, ratio_step_sizes=1.0)
        seen = []
        assert take_steps(MALITSKY_POCK, st, 5) == 5
        seen.append(_snapshot(eng, st))
        assert tuple(eng.average_info()[:2]) == (6, 5)
        eng.reset_average()
        assert take_steps(MALITSKY_POCK, st, 7) == 7
        seen.append(_snapshot(eng, st))
        assert tuple(eng.average_info()[:2]) == (8, 7)
        eng.restart_to_average()
        eng.reset_average()
        assert take_steps(MALITSKY_POCK, st, 4) == 4
        seen.append(_snapshot(eng, st))
        assert tuple(eng.average_info()[:2]) == (5, 4)
        outs.append(seen)
        eng.close()
    for other, label in ((outs[1], "C loop"), (outs[2], "LDS kernel")):
        for a, b in zip(outs[0], other):
            _assert_same(a, b, label)


def test_malitsky_pock_refuses_a_qp_and_launches_nothing(gpu_required, monkeypatch):
    _set_path(monkeypatch, "lds")
    eng = HipPdhgEngine.from_problem(H.example_qp())
    x0, y0 = eng.get_current()
    info0 = eng.steps_info()
    with pytest.raises(_lib.PdhgHipError, match="-2.*linear programming"):
        eng.take_steps_malitsky_pock(8, 0.7, 0.99, 1.0, 0.1, 1.0, 1.0, 0, 0.0)
    x1, y1 = eng.get_current()
    assert np.array_equal(x0, x1) and np.array_equal(y0, y1)
    assert eng.steps_info() == info0 and tuple(eng.average_info()[:2]) == (0, 0)
    # the constant policy takes a QP (launch by launch: a QP is no small LP)
    kkt, done = eng.take_steps_constant(8, 0.05, 1.0, 0.0)
    assert (kkt, done) == (8.0, 8) and eng.steps_info()[0] == 0
    eng.close()


@POLICIES
def test_which_path_ran(gpu_required, monkeypatch, policy):
    p = random_lp(120, 100, 4, seed=5)
    step, pw = _start(p, policy)
    for path, per_batch in (("lds", 1), ("c", 0)):
        _set_path(monkeypatch, path)
        eng = HipPdhgEngine.from_problem(p)
        st = PdhgSolverState(eng, step_size=step, primal_weight=pw, ratio_step_sizes=1.0)
        assert take_steps(policy, st, 64) == 64          # (Malitsky-Pock: from an empty average -- one single step first)
        assert eng.steps_info()[0] == per_batch
        assert eng.average_info()[0] > 0
        assert take_steps(policy, st, 64) == 64          # the average is not empty: the whole batch in one launch
        assert eng.steps_info()[0] == 2 * per_batch
        assert take_steps(policy, st, 1) == 1            # a single step is taken launch by launch
        assert eng.steps_info() == [2 * per_batch, 0, 0, 0]
        eng.close()


@POLICIES
@pytest.mark.parametrize("maker", [lambda: random_lp(800, 600, 7, seed=5), lambda: random_lp(30, 30, 3, seed=1)],
                         ids=["800x600", "30x30"])
def test_the_lds_kernel_matches_the_oracle(gpu_required, monkeypatch, policy, maker):
    """600 free-running steps in batches of 64 against oracle.take_step_constant() / take_step_malitsky_pock(0.7, 0.99,
    1.0) with exact sums: x, y, the step size and total_number_iterations bitwise.  The constant policy reads no sums, so
    it matches the oracle's plain sums too."""
    p = maker()
    got, launches = _run(p, policy, [64] * 9 + [24], monkeypatch, "lds")
    assert launches == 10
    for exact in ((True, False) if policy is CONSTANT else (True,)):
        st = H.oracle_from_problem(p)
        st.exact_sums = exact
        st.step_size, st.primal_weight = _start(p, policy)
        st.ratio_step_sizes = 1.0
        for _ in range(600):
            if policy is CONSTANT:
                st.take_step_constant()
            else:
                st.take_step_malitsky_pock(0.7, 0.99, 1.0)
        assert not st.numerical_error and not got[10]
        assert np.array_equal(got[3], st.x) and np.array_equal(got[4], st.y), exact
        assert st.step_size == got[1] and st.total_number_iterations == got[8]
        assert st.cumulative_kkt_passes == got[9]


# ---- a fleet: every member bitwise a twin handle stepped by its own solo call --------------------------------------------

def _fleet_problems(K, policy):
    """K problems of mixed shapes: both thread-count classes, one LP with a row of 257 entries and, for the constant
    policy, one QP; the rest small."""
    special = [lambda: random_lp(30, 30, 3, seed=1), lambda: random_lp(300, 280, 4, seed=2),
               lambda: H.rows_with_lens([257] + [4] * 39, 300, seed=3)]
    if policy is CONSTANT:
        special.append(H.example_qp)
    rng = np.random.default_rng(K)
    out = [mk() for mk in special[:K]]
    while len(out) < K:
        m, n = int(rng.integers(4, 40)), int(rng.integers(4, 40))
        out.append(random_lp(m, n, min(3, n), seed=100 + len(out)))
    return out


@POLICIES
@pytest.mark.parametrize("K", [1, 3, 70])
def test_a_fleet_steps_every_member_as_its_solo_call_would(gpu_required, monkeypatch, policy, K):
    _set_path(monkeypatch, "lds")
    problems = _fleet_problems(K, policy)
    fleet = HipPdhgFleet.from_problems(problems)
    twins = [HipPdhgEngine.from_problem(p) for p in problems]
    start = [_start(p, policy) for p in problems]
    ss, pw = np.array([s for s, _ in start]), np.array([w for _, w in start])
    ratio, it, kkt = np.ones(K), np.zeros(K, dtype=np.int64), np.zeros(K)
    rng = np.random.default_rng(7 * K)
    eligible = [eng.layout_info()["small_lp"] == 1 for eng in fleet.members]
    assert eligible == [eng.layout_info()["small_lp"] == 1 for eng in twins]
    # a first call that leaves every average non-empty, then n_steps[k] drawn from {0, 1, 2, 64}
    rounds = [np.full(K, 3, dtype=np.int64), rng.choice([0, 1, 2, 64], size=K).astype(np.int64)]
    if K >= 3:
        rounds[1][:3] = [64, 2, 64]              # both thread-count classes and the long-row LP take part
    for r, ns in enumerate(rounds):
        launches0 = fleet.info()["shared_launches"]
        ss_in, ratio_in, it_in, kkt_in = ss.copy(), ratio.copy(), it.copy(), kkt.copy()
        if policy is CONSTANT:
            kkt, done = fleet.take_steps_constant(ns, ss, pw, kkt)
            err = np.zeros(K, dtype=bool)
        else:
            ss, ratio, it, kkt, err, done = fleet.take_steps_malitsky_pock(ns, 0.7, 0.99, 1.0, ss, ratio, pw, it, kkt)
        info = fleet.info()
        nonempty = r > 0 or policy is CONSTANT
        assert info["carried"] == sum(1 for k in range(K) if eligible[k] and ns[k] >= 2 and nonempty)
        assert info["carried"] + info["single"] == int((ns > 0).sum())
        assert info["shared_launches"] - launches0 <= 2
        assert (info["shared_launches"] > launches0) == (info["carried"] > 0)
        assert np.array_equal(done, ns) and not err.any()
        for k, tw in enumerate(twins):
            if ns[k] == 0:                           # neither read nor written
                assert (ss[k], ratio[k], it[k], kkt[k]) == (ss_in[k], ratio_in[k], it_in[k], kkt_in[k]), k
            elif policy is CONSTANT:
                assert tw.take_steps_constant(int(ns[k]), ss_in[k], pw[k], kkt_in[k]) == (kkt[k], ns[k]), k
            else:
                solo = tw.take_steps_malitsky_pock(int(ns[k]), 0.7, 0.99, 1.0, ss_in[k], ratio_in[k], pw[k], int(it_in[k]),
                                                   kkt_in[k])
                assert solo == (ss[k], ratio[k], it[k], kkt[k], False, ns[k]), k
    for k, (mb, tw) in enumerate(zip(fleet.members, twins)):
        for a, b in zip(mb.get_current() + mb.get_average(), tw.get_current() + tw.get_average()):
            assert np.array_equal(a, b), k
        assert np.array_equal(np.array(mb.average_info()), np.array(tw.average_info())), k
    # n_steps[k] < 0: refused before anything is launched
    bad = np.full(K, -1, dtype=np.int64)
    with pytest.raises(_lib.PdhgHipError, match="-2"):
        fleet.take_steps_constant(bad, ss, pw, kkt)
    with pytest.raises(_lib.PdhgHipError, match="-2"):
        fleet.take_steps_malitsky_pock(bad, 0.7, 0.99, 1.0, ss, ratio, pw, it, kkt)
    for tw in twins:
        tw.close()
    fleet.close()


def test_solo_calls_refuse_a_fleet_handle_and_fleet_calls_a_solo_handle(gpu_required):
    import ctypes
    from firstorderlp_jl_amd.engine import _int_p, _pd, _pi
    fleet = HipPdhgFleet.from_problems([random_lp(30, 30, 3, seed=1)])
    solo = HipPdhgEngine.from_problem(random_lp(30, 30, 3, seed=1))
    L = fleet._L
    ss, ratio, kkt, it, err, done = (ctypes.c_double(0.1), ctypes.c_double(1.0), ctypes.c_double(0.0), ctypes.c_int64(0),
                                     ctypes.c_int(0), ctypes.c_int64(0))
    ref = ctypes.byref
    assert L.pdhg_take_steps_constant(fleet._h, 4, 0.1, 1.0, ref(kkt), ref(done)) == -1
    assert L.pdhg_take_steps_malitsky_pock(fleet._h, 4, 0.7, 0.99, 1.0, ref(ss), ref(ratio), 1.0, ref(it), ref(kkt), ref(err),
                                           ref(done)) == -1
    ns, one, zero = np.array([4], dtype=np.int64), np.ones(1), np.zeros(1)
    its, errs, dones = np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int64)
    assert L.pdhg_fleet_take_steps_constant(solo._h, _pi(ns), _pd(one), _pd(one), _pd(zero), _pi(dones)) == -1
    assert L.pdhg_fleet_take_steps_malitsky_pock(solo._h, _pi(ns), 0.7, 0.99, 1.0, _pd(one), _pd(one), _pd(one), _pi(its),
                                                 _pd(zero), errs.ctypes.data_as(_int_p), _pi(dones)) == -1
    assert (kkt.value, it.value, done.value, zero[0], dones[0]) == (0.0, 0, 0, 0.0, 0)
    assert fleet.members[0].steps_info() == [0, 0, 0, 0] and solo.steps_info() == [0, 0, 0, 0]
    solo.close()
    fleet.close()


# ---- whole solves ---------------------------------------------------------------------------------------------------------

def _params(policy):
    from firstorderlp_jl_amd.saddle_point import RestartScheme, RestartToCurrentMetric, construct_restart_parameters
    from firstorderlp_jl_amd.termination import construct_termination_criteria
    tc = construct_termination_criteria(eps_optimal_absolute=1e-6, eps_optimal_relative=1e-6, iteration_limit=4000)
    rp = construct_restart_parameters(RestartScheme.ADAPTIVE_NORMALIZED, RestartToCurrentMetric.GAP_OVER_DISTANCE_SQUARED,
                                      1000, 0.5, 0.1, 0.9, 0.5, False)
    return PdhgParameters(10, False, 1.0, 1.0, True, 0, True, 40, tc, rp, policy)


def _solution(o):
    return o.iteration_count, o.termination_reason, o.primal_solution, o.dual_solution


def _assert_same_solve(a, b, label):
    assert a[0] == b[0] and a[1] == b[1], label
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]), label


@POLICIES
def test_a_whole_solve_is_the_python_loops_solve(gpu_required, monkeypatch, policy):
    q = random_lp(900, 700, 6, seed=11)
    monkeypatch.setenv("PDHG_PY_TAKE_STEP", "1")
    want = _solution(optimize(_params(policy), q))
    monkeypatch.delenv("PDHG_PY_TAKE_STEP")
    got = _solution(optimize(_params(policy), q))
    _assert_same_solve(want, got, "optimize")
    assert want[0] > 100


@POLICIES
def test_optimize_many_is_the_loop_of_optimize(gpu_required, monkeypatch, policy):
    monkeypatch.delenv("PDHG_PY_TAKE_STEP", raising=False)
    problems = [random_lp(900, 700, 6, seed=11), random_lp(30, 30, 3, seed=1), random_lp(300, 280, 4, seed=2),
                random_lp(120, 200, 5, seed=3), random_lp(257, 100, 4, seed=4)]
    params = _params(policy)
    want = [_solution(optimize(params, p)) for p in problems]
    got = [_solution(o) for o in optimize_many(params, problems)]
    for k, (a, b) in enumerate(zip(want, got)):
        _assert_same_solve(a, b, k)
