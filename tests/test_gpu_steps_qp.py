"""The QP form of the multi-step persistent kernel (csrc/trial_kernel.hpp: steps_kernel<LOCAL, true>, all-XCD and
XCD-local), reached through pdhg_take_steps_adaptive under PDHG_DEVICE_LOOP=1 by QPs whose Q and Q' are in the stream
layout.

Per trial the kernel must compute what one trial_kernel QP launch followed by the host's rule computes, so every case is
held BITWISE to a twin handle that takes the same steps launch by launch (PDHG_DEVICE_LOOP=0): step sizes and counters
after every batch, iterate, A'y, trial buffers, averages and average_info after every op (_assert_same_record).  The
single trials between the launches are held to the CPU oracle by _drive itself.  The shapes sit where the QP phases
branch: an odd n (the pairs' tail), a long row and column of Q (two chunks, tickets across launches of both kernels),
more dot-product blocks than workgroups, more items in Q than in A, n round 2 TPB, launches that end inside a take_step,
a first trial without movement.  Every case runs in both row orders."""
import numpy as np
import pytest
import scipy.sparse as sp

from firstorderlp_jl_amd import HipPdhgEngine, HipPdhgFleet, QuadraticProgrammingProblem
from firstorderlp_jl_amd.generators import random_lp, random_qp_family
from firstorderlp_jl_amd.primal_dual_hybrid_gradient import optimize
from tests import helpers as H
from tests.test_gpu_small_qp import _solve_qp_default_params, _stats_key
from tests.test_gpu_trial_kernel_edges import (BASE_ENV, KNOBS, LOCAL_MAX_GRID, TPB, _arrow_qp, _assert_same_record, _drive,
                                               _expected)

pytestmark = pytest.mark.gpu

RED, GROW = 0.3, 0.6
SCRIPT = [("trial", 1.0), ("trial", 0.5), ("accept",), ("steps", 5), ("trial", 1.0), ("steps", 1), ("scale", 300.0),
          ("steps", 7), ("mp", 1.2, 0.84), ("accept",), ("steps", 9), ("averages",)]
# n, PDHG_XCD_REMAP, the grid coop_prepare gives (_expected restates it: under the remap every product's row blocks count
# in eights -- 16 + 2 chunks for Q at n = 8193, a grid of 24)
ARROWS = {"5001_no_remap": (5001, "0", 16), "8193_remap": (8193, "1", 24)}

_PROBLEMS, _TWINS = {}, {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _problem(name, maker):
    if name not in _PROBLEMS:
        _PROBLEMS[name] = maker()
    return _PROBLEMS[name]


def _twin(monkeypatch, row_order_mode, name, p, script, env, **kw):
    """The launch-by-launch run (PDHG_DEVICE_LOOP=0) of a case: once per row order, left unchanged."""
    key = (row_order_mode, name, tuple(sorted(env.items())))
    if key not in _TWINS:
        _TWINS[key] = _drive(p, script, monkeypatch, device_loop=False, env=env, check=False, label="twin", **kw)
        assert _TWINS[key].info["device_loop"] == 0
    return _TWINS[key]


def _with_q(base, Q):
    Q = sp.csc_matrix(Q)
    Q.sort_indices()
    return QuadraticProgrammingProblem(
        variable_lower_bound=base.variable_lower_bound, variable_upper_bound=base.variable_upper_bound, objective_matrix=Q,
        objective_vector=base.objective_vector, objective_constant=0.0, constraint_matrix=base.constraint_matrix,
        right_hand_side=base.right_hand_side, num_equalities=base.num_equalities)


# ---- 1 and 2: the arrow QP through both kernel forms, whole take_steps and launches that end inside them -----------
@pytest.mark.parametrize("table", [None, "3"], ids=["whole_take_steps", "launches_end_inside_take_steps"])
@pytest.mark.parametrize("local", [1, 0], ids=["xcd_local", "all_xcd"])
@pytest.mark.parametrize("shape", list(ARROWS))
def test_arrow_qp_is_bitwise_the_single_launches(gpu_required, row_order_mode, monkeypatch, capfd, shape, local, table):
    """A trial, the same trial at half the step, an accept (its average update rides into the first launch), five
    take_steps in one launch, a trial, one take_step, seven from a step size 300 times too long (rejections inside the
    launch: the kept Q x is used again), a Malitsky-Pock step (phase 0 is xbar alone, Q x untouched), an accept whose
    update rides into nine more.  With PDHG_STEPS_TEST_TABLE=3 the launches end inside take_steps and the host finishes
    them with trial_kernel launches that draw from the same tickets."""
    n, remap, grid = ARROWS[shape]
    p = _problem(f"arrow_{n}", lambda: _arrow_qp(n))
    A, Q = p.constraint_matrix, p.objective_matrix
    want = _expected(A, Q=Q, remap=remap == "1")
    q_blocks = -(-n // TPB)
    assert n % 2 == 1 and want["grid"] == grid <= LOCAL_MAX_GRID and q_blocks > grid
    assert want["Q_long_rows"] == 1 and want["Q_long_chunks"] == 2 and want["Q_items"] > want["A_items"]
    env = {"PDHG_XCD_REMAP": remap}
    if table:
        env["PDHG_STEPS_TEST_TABLE"] = table
    twin = _twin(monkeypatch, row_order_mode, shape, p, SCRIPT, env)
    if not local:
        env = dict(env, PDHG_COOP_LOCAL="0")
    got = _drive(p, SCRIPT, monkeypatch, device_loop=True, env=env, capfd=capfd, local=local, label=f"QP {shape} local={local}")
    assert got.grid == grid
    _assert_same_record(got, twin, "the QP multi-step kernel against single trial_kernel launches")
    assert got.rec[-1][1] > 5 + 1 + 7 + 9      # iterations: more trials than take_steps -- the launches rejected some


# ---- 3: the elementwise phases' pairs and tail, the dot product's blocks ---------------------------------------------
def _diagonal_qp(n):
    """A of 8-entry rows and Q a diagonal alone; at n = 2 TPB the diagonal has holes (empty rows and columns of Q) and
    stored zeros."""
    base = H.rows_with_lens([8] * 40, n, 90 + n)
    d = np.linspace(0.5, 2.0, n)
    idx = np.arange(n)
    if n == 2 * TPB:
        keep = np.ones(n, dtype=bool)
        keep[[0, 7, TPB - 1, TPB, n - 1]] = False
        idx, d = idx[keep], d[keep]
        d[[3, 100, 300]] = 0.0
    Q = sp.csc_matrix((d, (idx, idx)), shape=(n, n))
    assert Q.nnz == len(d)
    return _with_q(base, Q)


@pytest.mark.parametrize("n", [2 * TPB - 1, 2 * TPB, 2 * TPB + 1])
def test_elementwise_edges(gpu_required, row_order_mode, monkeypatch, n):
    """n = 2 TPB - 1, 2 TPB, 2 TPB + 1: one pair short of a workgroup's threads and an odd tail, exactly the threads,
    one element more (a tail again); the partials of dx . (Q'dx) are 2, 2 and 3 blocks."""
    p = _problem(f"diagonal_{n}", lambda: _diagonal_qp(n))
    Q = p.objective_matrix
    assert -(-n // TPB) == (3 if n > 2 * TPB else 2)
    if n == 2 * TPB:
        assert (np.diff(Q.indptr) == 0).sum() == 5 and (Q.data == 0.0).sum() == 3
    want = _expected(p.constraint_matrix, Q=Q)
    assert want["grid"] == 16      # under the XCD remap A and Q' count eight row blocks each, and share phase 1
    script = [("trial", 1.0), ("accept",), ("trial", 1.0), ("averages",), ("accept",), ("steps", 3), ("steps", 9)]
    twin = _twin(monkeypatch, row_order_mode, f"diagonal_{n}", p, script, {})
    got = _drive(p, script, monkeypatch, device_loop=True, local=1, label=f"diagonal QP, n = {n}")
    _assert_same_record(got, twin, "the QP multi-step kernel against single trial_kernel launches")


# ---- 4: numerical error ----------------------------------------------------------------------------------------------
def test_a_first_trial_without_movement_ends_with_numerical_error(gpu_required, row_order_mode, monkeypatch):
    """c = 0, b = 0, the start at the origin inside its bounds: x' = x, y' = y, movement 0 -- the launch ends through
    the numerical-error result word with the step size it came with."""
    n = 600
    base = H.rows_with_lens([8] * 40, n, 97, num_eq=40)
    rng = np.random.default_rng(98)
    zero = QuadraticProgrammingProblem(
        variable_lower_bound=-1.0 - rng.random(n), variable_upper_bound=1.0 + rng.random(n),
        objective_matrix=sp.csc_matrix(sp.diags(np.linspace(0.5, 2.0, n))), objective_vector=np.zeros(n), objective_constant=0.0,
        constraint_matrix=base.constraint_matrix, right_hand_side=np.zeros(40), num_equalities=40)
    script = [("steps", 4)]
    twin = _drive(zero, script, monkeypatch, device_loop=False, check=False, start_seed=None, step_pw=(0.3, 1.0))
    got = _drive(zero, script, monkeypatch, device_loop=True, start_seed=None, step_pw=(0.3, 1.0), local=1, label="no movement")
    assert got.numerical_error and twin.numerical_error
    _assert_same_record(got, twin, "numerical error inside the launch against the single launches")


# ---- 5: the switch ---------------------------------------------------------------------------------------------------
def _six_steps(monkeypatch, p, setting):
    for k in KNOBS + ("PDHG_DEVICE_LOOP",):
        monkeypatch.delenv(k, raising=False)
    for k, v in BASE_ENV.items():
        monkeypatch.setenv(k, v)
    if setting is not None:
        monkeypatch.setenv("PDHG_DEVICE_LOOP", setting)
    eng = HipPdhgEngine.from_problem(p)
    try:
        step, pw = H.initial_step_and_weight(p)
        info0 = eng.layout_info()["device_loop"]
        ss, it, kkt, err, done = eng.take_steps_adaptive(6, RED, GROW, step, pw, 0, 0.0)
        assert done == 6 and not err
        return info0, eng.layout_info()["device_loop"], eng.steps_info(), it, (ss,) + eng.get_current()
    finally:
        eng.close()


def test_the_switch(gpu_required, row_order_mode, monkeypatch):
    """Unset, a QP goes launch by launch as before; PDHG_DEVICE_LOOP=1 takes it into the loop, and every trial of the
    six take_steps is one of the launches'.  An LP reports the loop in both settings."""
    p = _problem("arrow_5001", lambda: _arrow_qp(5001))
    before, after, info, it, state_unset = _six_steps(monkeypatch, p, None)
    assert (before, after) == (0, 0) and info[1] == 0 and info[2] == 0
    before, after, info, it, state_on = _six_steps(monkeypatch, p, "1")
    assert (before, after) == (1, 1) and info[1] >= 1 and info[2] == it
    for a, b in zip(state_unset, state_on):
        assert np.array_equal(_bits(a), _bits(b))
    before, after, info, it, _ = _six_steps(monkeypatch, p, "0")
    assert (before, after) == (0, 0) and info[1] == 0
    lp = H.rows_with_lens([8] * 300, 5001, 81)
    for setting in (None, "1"):
        before, after, info, it, _ = _six_steps(monkeypatch, lp, setting)
        assert (before, after) == (1, 1) and info[1] >= 1 and info[2] == it, setting


# ---- 6: bitwise against the oracle -----------------------------------------------------------------------------------
def test_short_row_qp_matches_the_oracle_in_exact_sums_mode(gpu_required, row_order_mode, monkeypatch):
    """Every row of A, A', Q and Q' within bitexact_row_limit(): batches of 3 and 9 take_steps in the loop are the
    exact-sums oracle's trajectory, bit for bit."""
    p = _problem("family_600x500", lambda: random_qp_family(600, 500, 1, 3)[0])
    A, Q = sp.csc_matrix(p.constraint_matrix), sp.csc_matrix(p.objective_matrix)
    longest = max(np.diff(M.indptr).max() for M in (A, A.tocsr(), Q, Q.tocsr()))
    assert longest <= H.bitexact_row_limit()
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in dict(BASE_ENV, PDHG_DEVICE_LOOP="1").items():
        monkeypatch.setenv(k, v)
    step, pw = H.initial_step_and_weight(p)
    st = H.oracle_from_problem(p)
    eng = HipPdhgEngine.from_problem(p)
    try:
        assert eng.layout_info()["device_loop"] == 1
        st.exact_sums = True
        st.step_size, st.primal_weight = step, pw
        ss, it, kkt = step, 0, 0.0
        for batch in (3, 9):
            ss, it, kkt, err, done = eng.take_steps_adaptive(batch, RED, GROW, ss, pw, it, kkt)
            assert done == batch and not err
            for _ in range(batch):
                st.take_step_adaptive(RED, GROW)
            x, y = eng.get_current()
            assert it == st.total_number_iterations and _bits(ss) == _bits(st.step_size), batch
            assert np.array_equal(_bits(x), _bits(st.x)) and np.array_equal(_bits(y), _bits(st.y)), batch
        assert eng.steps_info()[1] >= 2
    finally:
        eng.close()
        st.close()


# ---- 7: a whole solve ------------------------------------------------------------------------------------------------
def test_a_whole_solve_is_the_same_in_the_loop(gpu_required, row_order_mode, monkeypatch):
    """Rescaling, evaluations, restarts and primal-weight updates between the batches: termination reason, iteration
    count, KKT passes, solutions and every statistic but the times are those of the launch-by-launch solve."""
    p = _problem("family_300x240", lambda: random_qp_family(300, 240, 1, 11)[0])
    params = _solve_qp_default_params(20000)
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in BASE_ENV.items():
        monkeypatch.setenv(k, v)
    launches = {}

    def solve(setting):
        monkeypatch.setenv("PDHG_DEVICE_LOOP", setting)

        def factory(problem):
            eng = HipPdhgEngine.from_problem(problem)
            close = eng.close

            def closing():
                launches[setting] = eng.steps_info()[1]
                close()
            eng.close = closing
            return eng
        factory.takes_original_problem = True
        return optimize(params, p, engine_factory=factory)
    want, got = solve("0"), solve("1")
    assert launches["0"] == 0 and launches["1"] > 0, launches
    assert got.termination_reason == want.termination_reason and got.iteration_count == want.iteration_count
    assert np.array_equal(_bits(got.primal_solution), _bits(want.primal_solution))
    assert np.array_equal(_bits(got.dual_solution), _bits(want.dual_solution))
    assert [_stats_key(s) for s in got.iteration_stats] == [_stats_key(s) for s in want.iteration_stats]
    assert got.iteration_stats[-1].cumulative_kkt_matrix_passes == want.iteration_stats[-1].cumulative_kkt_matrix_passes


# ---- 8: a fleet's singly stepped member ------------------------------------------------------------------------------
def test_a_fleets_medium_qp_member_steps_in_the_loop(gpu_required, row_order_mode, monkeypatch):
    """A small LP (carried in the fleet's shared launch) beside the arrow QP, which the fleet steps singly: under
    PDHG_DEVICE_LOOP=1 that member's eight take_steps are the multi-step kernel's, bitwise those under 0."""
    problems = [random_lp(40, 50, 3, seed=41), _problem("arrow_5001", lambda: _arrow_qp(5001))]
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("PDHG_GRAPH", "1")
    monkeypatch.setenv("PDHG_COOP", "1")
    monkeypatch.delenv("PDHG_SMALL_LP", raising=False)
    sw = [H.initial_step_and_weight(q) for q in problems]
    out = {}
    for setting in ("0", "1"):
        monkeypatch.setenv("PDHG_DEVICE_LOOP", setting)
        fleet = HipPdhgFleet.from_problems(problems, device_id=0)
        try:
            ss, it, kkt, err, done = fleet.take_steps_adaptive([8, 8], RED, GROW, np.array([s for s, _ in sw]), np.array([w for _, w in sw]),
                                                               np.zeros(2, dtype=np.int64), np.zeros(2))
            assert list(done) == [8, 8] and not np.any(err)
            rec = [ss, it, kkt]
            for mb in fleet.members:
                rec += list(mb.get_current()) + [mb.get_dual_product()] + list(mb.get_average()) + [np.array(mb.average_info())]
            out[setting] = (rec, [int(mb.steps_info()[1]) for mb in fleet.members], fleet.info())
        finally:
            fleet.close()
    assert out["0"][1][1] == 0 and out["1"][1][1] > 0, (out["0"][1], out["1"][1])
    assert out["1"][2]["carried"] == 1 and out["1"][2]["single"] == 1, out["1"][2]
    for a, b in zip(out["0"][0], out["1"][0]):
        assert np.array_equal(_bits(a), _bits(b))
