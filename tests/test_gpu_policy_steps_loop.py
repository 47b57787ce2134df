"""The constant and the Malitsky-Pock policy in the persistent multi-step kernel (csrc/trial_kernel.hpp:
policy_steps_kernel, all-XCD and XCD-local), reached through pdhg_take_steps_constant / _malitsky_pock under
PDHG_DEVICE_LOOP=1 by problems too large for the one-workgroup class (PDHG_SMALL_LP=0 here).

Per step the kernel must compute what the launch-by-launch host loops compute, so every case is held BITWISE
(np.array_equal on the 64-bit patterns) to a twin handle that takes the same operations under PDHG_DEVICE_LOOP=0: after
every operation step size, ratio, total_number_iterations, cumulative_kkt_passes, numerical_error and steps_done, the
iterate, A'y and average_info; at the end both averages.  Under the constant policy the step size is
1 / sqrt(|A|_1 |A|_inf) (divided further for a QP), for which the iterates stay finite over every script.  Every case
runs in both row orders."""
import numpy as np
import pytest
import scipy.sparse as sp

from firstorderlp_jl_amd import HipPdhgEngine, HipPdhgFleet, _lib
from firstorderlp_jl_amd.generators import random_lp, random_qp_family
from firstorderlp_jl_amd.primal_dual_hybrid_gradient import (ConstantStepsizeParams, MalitskyPockStepsizeParameters,
                                                             PdhgParameters, PdhgSolverState, optimize, take_step,
                                                             take_steps)
from tests import helpers as H
from tests.test_gpu_small_qp import _stats_key
from tests.test_gpu_steps_qp import _diagonal_qp
from tests.test_gpu_trial_kernel_edges import BASE_ENV, KNOBS, LOCAL_MAX_GRID, TPB, _arrow_qp, _expected

pytestmark = pytest.mark.gpu

CONSTANT = ConstantStepsizeParams()
MALITSKY_POCK = MalitskyPockStepsizeParameters(0.7, 0.99, 1.0)
POLICIES = {"constant": CONSTANT, "malitsky_pock": MALITSKY_POCK}
MAX_TRIALS = 60                         # MALITSKY_POCK_MAX_TRIALS, csrc/common.hpp

_PROBLEMS, _TWINS = {}, {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b):
    if isinstance(a, (float, np.floating)) or (isinstance(a, np.ndarray) and a.dtype == np.float64):
        return np.array_equal(_bits(a), _bits(b))
    return np.array_equal(a, b)


def _problem(name, maker):
    if name not in _PROBLEMS:
        _PROBLEMS[name] = maker()
    return _PROBLEMS[name]


def _lp_5001():
    return _problem("lp_5001", lambda: H.rows_with_lens([8] * 300, 5001, 81))


def _arrow_lp():
    """block_diag(L, L'), L's first row of 2100 entries: a long row and a long column of A, two chunks each, in both
    products -- the rows the long ladder of test_ticket_bookkeeping_across_launches_and_kernels has, on a grid small
    enough for the XCD-local form (16 workgroups without the XCD remap, 24 with it)."""
    return _problem("arrow_lp", lambda: H.ladder_lp([2100] + [16] * 700, seed=7))


def _start(p, policy):
    """(step size, primal weight).  Malitsky-Pock: pdhg.jl:821-826.  Constant: 1 / sqrt(|A|_1 |A|_inf) <= 1 / |A|_2; a QP
    with primal weight 1 and half of 1 / (sqrt(|A|_1 |A|_inf) + |Q|_inf), so that tau |Q| + tau sigma |A|^2 < 1."""
    step, pw = H.initial_step_and_weight(p)
    if policy is CONSTANT:
        A = abs(sp.csr_matrix(p.constraint_matrix))
        norm = float(np.sqrt(A.sum(axis=0).max() * A.sum(axis=1).max()))
        step = 1.0 / norm
        Q = p.objective_matrix
        if Q is not None and Q.nnz > 0:
            step, pw = 0.5 / (norm + float(abs(sp.csr_matrix(Q)).sum(axis=1).max())), 1.0
    return float(step), float(pw)


def _set_env(monkeypatch, setting, env=None, base=BASE_ENV):
    for k in KNOBS + ("PDHG_DEVICE_LOOP", "PDHG_PY_TAKE_STEP"):
        monkeypatch.delenv(k, raising=False)
    for k, v in dict(base, **(env or {})).items():
        monkeypatch.setenv(k, v)
    if setting is not None:
        monkeypatch.setenv("PDHG_DEVICE_LOOP", setting)


class _Out:
    pass


def _drive(p, policy, script, monkeypatch, setting, env=None, step_scale=1.0, fresh=False):
    """One handle through `script`, a list of
      ("trial", f)     trial_step at f times the step size (one trial_kernel launch; no accept),
      ("accept",)      accept the last trial with the step size as weight (its average update is left pending),
      ("steps", k)     take_steps(policy, k): one library call,
      ("single", k)    k times take_step(policy): trial and accept launch by launch, whatever the setting,
      ("scale", f)     the step size times f,
      ("policy", q)    go on with policy q.
    fresh: start from the problem's own start with an empty average; else from a random point.  Returns the record
    (.rec), steps_info() and layout_info() at the end (.steps_info, .info)."""
    _set_env(monkeypatch, setting, env)
    out = _Out()
    out.rec = []
    eng = HipPdhgEngine.from_problem(p)
    try:
        assert eng.layout_info()["trial_graph"] == 2 and eng.layout_info()["small_lp"] == 0
        step, pw = _start(p, policy)
        st = PdhgSolverState(eng, step_size=step * step_scale, primal_weight=pw, ratio_step_sizes=1.0)
        if not fresh:
            m, n = p.constraint_matrix.shape
            rng = np.random.default_rng(5)
            eng.set_current(rng.random(n), rng.standard_normal(m))
        for op in script:
            done = -1
            if op[0] == "trial":
                out.rec.append((np.array(eng.trial_step(st.step_size * op[1], pw, 1.0)),) + tuple(eng.get_trial()))
            elif op[0] == "accept":
                eng.accept(st.step_size)
            elif op[0] == "steps":
                done = take_steps(policy, st, op[1])
            elif op[0] == "single":
                for _ in range(op[1]):
                    take_step(policy, st)
            elif op[0] == "scale":
                st.step_size *= op[1]
            elif op[0] == "policy":
                policy = op[1]
            x, y = eng.get_current()
            out.rec.append((np.float64(st.step_size), np.float64(st.ratio_step_sizes), st.total_number_iterations,
                            np.float64(st.cumulative_kkt_passes), bool(st.numerical_error), done, x, y, eng.get_dual_product(),
                            np.array(eng.average_info())))
            if st.numerical_error:
                break
        out.iterations, out.numerical_error = st.total_number_iterations, bool(st.numerical_error)
        out.steps_info, out.info = eng.steps_info(), eng.layout_info()
        out.rec.append(tuple(eng.get_average()) + (np.array(eng.average_info()),))
        out.finite = all(np.all(np.isfinite(v)) for v in eng.get_current() + eng.get_average())
    finally:
        eng.close()
    return out


def _twin(monkeypatch, row_order_mode, name, p, policy, script, env=None, **kw):
    """The launch-by-launch run (PDHG_DEVICE_LOOP=0) of a case: once per row order, left unchanged."""
    key = (row_order_mode, name, tuple(sorted((env or {}).items())))
    if key not in _TWINS:
        _TWINS[key] = _drive(p, policy, script, monkeypatch, "0", env=env, **kw)
        assert _TWINS[key].steps_info[:3] == [0, 0, 0]
    return _TWINS[key]


def _assert_same_record(a, b, label):
    assert len(a.rec) == len(b.rec), label
    for k, (u, v) in enumerate(zip(a.rec, b.rec)):
        assert len(u) == len(v), (label, k)
        for j, (s, t) in enumerate(zip(u, v)):
            assert _same(s, t), f"{label}: entry {k}.{j} of the record differs"


def _script(policy):
    """A single trial; an accept, whose average update rides into the first launch; batches of 2, 3 and 64 with single
    take_steps between them (the pending update crosses the paths both ways); a trial_kernel launch after the batches
    (the long rows' tickets go on from where the launches left them).  Malitsky-Pock: the last batch starts from a step
    size 300 times too long, so that the launch rejects trials and draws a ticket per DUAL TRIAL."""
    long_step = [("scale", 300.0)] if policy is MALITSKY_POCK else []
    return ([("trial", 1.0), ("accept",), ("steps", 2), ("single", 1), ("steps", 3), ("single", 2)] + long_step +
            [("steps", 64), ("trial", 1.0), ("single", 1), ("steps", 2), ("trial", 0.5)])


# ---- 1: both kernel forms, both policies --------------------------------------------------------------------------
@pytest.mark.parametrize("policy", list(POLICIES))
@pytest.mark.parametrize("remap", ["0", "1"], ids=["no_remap", "remap"])
@pytest.mark.parametrize("local", [1, 0], ids=["xcd_local", "all_xcd"])
@pytest.mark.parametrize("shape", ["lp", "arrow"])
def test_both_forms_both_policies(gpu_required, row_order_mode, monkeypatch, shape, local, remap, policy):
    p = _lp_5001() if shape == "lp" else _arrow_lp()
    pol = POLICIES[policy]
    want = _expected(p.constraint_matrix, remap=remap == "1")
    if shape == "arrow":
        assert want["A_long_rows"] == 1 and want["A_long_chunks"] == 2 and want["At_long_rows"] == 1 and want["At_long_chunks"] == 2
        assert want["grid"] == (24 if remap == "1" else 16)
    assert want["grid"] <= LOCAL_MAX_GRID
    env = {"PDHG_XCD_REMAP": remap}
    script = _script(pol)
    twin = _twin(monkeypatch, row_order_mode, f"{shape}_{policy}", p, pol, script, env)
    got = _drive(p, pol, script, monkeypatch, "1", env=dict(env, **({} if local else {"PDHG_COOP_LOCAL": "0"})))
    assert got.finite and twin.finite
    assert got.steps_info[0] == 0 and got.steps_info[1] >= 4 and got.info["steps_local"] == local
    _assert_same_record(got, twin, f"{policy} on the {shape}: the loop against launch by launch")
    if pol is MALITSKY_POCK:
        assert got.iterations > 2 + 1 + 3 + 2 + 64 + 1 + 2       # the launch from the long step rejected trials
        assert 0 < got.steps_info[2] < got.iterations            # ... and the single take_steps' trials are the host's


# ---- 2: the constant policy on a QP ---------------------------------------------------------------------------------
@pytest.mark.parametrize("local", [1, 0], ids=["xcd_local", "all_xcd"])
@pytest.mark.parametrize("n,remap,grid", [(5001, "0", 16), (8193, "1", 24)], ids=["5001_no_remap", "8193_remap"])
def test_constant_policy_on_the_arrow_qp(gpu_required, row_order_mode, monkeypatch, n, remap, grid, local):
    """Q x is kept for the iterate and the trial point and flips with x: an odd and an even number of steps per launch, a
    single take_step in between (its trial_kernel launch computes Q x itself), and a single trial after the batches."""
    p = _problem(f"arrow_qp_{n}", lambda: _arrow_qp(n))
    want = _expected(p.constraint_matrix, Q=p.objective_matrix, remap=remap == "1")
    assert want["grid"] == grid and want["Q_long_rows"] == 1 and want["Q_long_chunks"] == 2
    env = {"PDHG_XCD_REMAP": remap}
    script = _script(CONSTANT)
    twin = _twin(monkeypatch, row_order_mode, f"arrow_qp_{n}", p, CONSTANT, script, env)
    got = _drive(p, CONSTANT, script, monkeypatch, "1", env=dict(env, **({} if local else {"PDHG_COOP_LOCAL": "0"})))
    assert got.finite and twin.finite
    assert got.steps_info[0] == 0 and got.steps_info[1] >= 4 and got.info["steps_local"] == local
    assert got.steps_info[2] == 2 + 3 + 64 + 2
    _assert_same_record(got, twin, "the constant policy on a QP: the loop against launch by launch")


# ---- 3: the elementwise phases' pairs and tail ------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["constant_lp", "constant_qp", "malitsky_pock_lp"])
@pytest.mark.parametrize("n", [2 * TPB - 1, 2 * TPB, 2 * TPB + 1])
def test_elementwise_edges(gpu_required, row_order_mode, monkeypatch, n, kind):
    """n = 2 TPB - 1, 2 TPB, 2 TPB + 1 with m = 40: one pair short of a workgroup's threads and an odd tail, exactly the
    threads, one element more -- the pairs and the tail of primal_body and of xbar_pairs_body."""
    if kind == "constant_qp":
        p = _problem(f"diagonal_{n}", lambda: _diagonal_qp(n))
    else:
        p = _problem(f"rows8_{n}", lambda: H.rows_with_lens([8] * 40, n, 90 + n))
    pol = MALITSKY_POCK if kind == "malitsky_pock_lp" else CONSTANT
    assert p.constraint_matrix.shape == (40, n)
    script = [("trial", 1.0), ("accept",), ("steps", 3), ("single", 1), ("steps", 9), ("trial", 1.0)]
    twin = _twin(monkeypatch, row_order_mode, f"{kind}_{n}", p, pol, script)
    got = _drive(p, pol, script, monkeypatch, "1")
    assert got.finite and got.steps_info[1] == 2 and got.info["steps_local"] == 1
    _assert_same_record(got, twin, f"{kind}, n = {n}")


# ---- 4: the row partition ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", list(POLICIES))
@pytest.mark.parametrize("eq", ["none", "all"])
def test_row_partition(gpu_required, row_order_mode, monkeypatch, eq, policy):
    """num_equalities = 0 (every y' is projected) and = m (none is)."""
    p = _problem(f"lp_5001_{eq}", lambda: H.rows_with_lens([8] * 300, 5001, 81, num_eq=0 if eq == "none" else 300))
    assert p.num_equalities == (0 if eq == "none" else 300)
    pol = POLICIES[policy]
    script = [("trial", 1.0), ("accept",), ("steps", 3), ("steps", 9)]
    twin = _twin(monkeypatch, row_order_mode, f"eq_{eq}_{policy}", p, pol, script)
    got = _drive(p, pol, script, monkeypatch, "1")
    assert got.finite and got.steps_info[1] == 2
    _assert_same_record(got, twin, f"{policy}, num_equalities {eq}")


# ---- 5: Malitsky-Pock rejections inside a launch ----------------------------------------------------------------------
def test_malitsky_pock_downscales_inside_a_launch(gpu_required, row_order_mode, monkeypatch):
    """A first step 300 times too long: the first take_step (an empty average) is the host's, the three batches of 40 are
    three launches, and every dual trial after the first take_step is one of theirs."""
    p = _problem("random_300x250", lambda: random_lp(300, 250, 5, seed=2))
    script = [("steps", 1), ("steps", 40), ("steps", 40), ("steps", 40)]
    twin = _twin(monkeypatch, row_order_mode, "downscale", p, MALITSKY_POCK, script, step_scale=300.0, fresh=True)
    got = _drive(p, MALITSKY_POCK, script, monkeypatch, "1", step_scale=300.0, fresh=True)
    _assert_same_record(got, twin, "rejections inside the launches")
    first = got.rec[0][2]                                       # total_number_iterations after the host's take_step
    assert got.iterations > 121 and got.steps_info[1] == 3
    assert got.steps_info[2] == got.iterations - first


# ---- 6: sixty rejections ----------------------------------------------------------------------------------------------
def test_sixty_rejections_end_the_launch_and_leave_the_state(gpu_required, row_order_mode, monkeypatch):
    """breaking_factor = 0 rejects every trial (A'(y' - y) is not zero on this LP): numerical_error, +60 iterations, +30.5
    KKT passes; step size, ratio and the iterate as they came; the failing take_step counts as taken."""
    p = _problem("random_300x240", lambda: random_lp(300, 240, 5, seed=3))
    never = MalitskyPockStepsizeParameters(0.7, 0.0, 1.0)
    script = [("steps", 5), ("policy", never), ("steps", 4)]
    twin = _twin(monkeypatch, row_order_mode, "sixty", p, MALITSKY_POCK, script, fresh=True)
    got = _drive(p, MALITSKY_POCK, script, monkeypatch, "1", fresh=True)
    assert got.numerical_error and twin.numerical_error and got.steps_info[1] == 2
    before, after = got.rec[0], got.rec[2]
    assert after[5] == 1 and after[4] and not before[4]
    assert after[2] == before[2] + MAX_TRIALS and after[3] == before[3] + 0.5 + 0.5 * MAX_TRIALS
    for j in (0, 1, 6, 7, 8):                                   # step size, ratio, x, y, A'y
        assert _same(before[j], after[j]), j
    _assert_same_record(got, twin, "sixty rejections inside the launch")


# ---- 7: the first accept into an empty average stays on the host ------------------------------------------------------
def test_the_first_take_step_into_an_empty_average_is_the_hosts(gpu_required, row_order_mode, monkeypatch):
    p = _lp_5001()
    script = [("steps", 5)]
    twin = _twin(monkeypatch, row_order_mode, "quirk", p, MALITSKY_POCK, script, fresh=True)
    got = _drive(p, MALITSKY_POCK, script, monkeypatch, "1", fresh=True)
    _assert_same_record(got, twin, "five take_steps from an empty average")
    assert tuple(got.rec[0][9][:2]) == (6, 5)                   # pdhg.jl:621-627: the current x went in first
    assert got.steps_info[1] >= 1 and got.steps_info[2] < got.iterations


# ---- 8: the switch ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", list(POLICIES))
def test_the_switch(gpu_required, row_order_mode, monkeypatch, policy):
    """Unset and 0: launch by launch, as before; 1: the persistent kernel -- with the same bits in all three."""
    p, pol = _lp_5001(), POLICIES[policy]
    script = [("trial", 1.0), ("accept",), ("steps", 6)]
    runs = {setting: _drive(p, pol, script, monkeypatch, setting) for setting in (None, "0", "1")}
    assert runs[None].steps_info[:3] == [0, 0, 0] and runs["0"].steps_info[:3] == [0, 0, 0]
    assert runs["1"].steps_info[0] == 0 and runs["1"].steps_info[1] >= 1
    _assert_same_record(runs[None], runs["0"], "unset against 0")
    _assert_same_record(runs["1"], runs["0"], "1 against 0")


@pytest.mark.parametrize("setting", [None, "0", "1"], ids=["unset", "0", "1"])
def test_malitsky_pock_still_refuses_a_qp(gpu_required, monkeypatch, setting):
    _set_env(monkeypatch, setting)
    eng = HipPdhgEngine.from_problem(_problem("arrow_qp_5001", lambda: _arrow_qp(5001)))
    try:
        with pytest.raises(_lib.PdhgHipError, match="-2.*linear programming"):
            eng.take_steps_malitsky_pock(8, 0.7, 0.99, 1.0, 0.1, 1.0, 1.0, 0, 0.0)
        assert eng.steps_info() == [0, 0, 0, 0] and tuple(eng.average_info()[:2]) == (0, 0)
    finally:
        eng.close()


# ---- 9: bitwise against the oracle -------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", list(POLICIES))
def test_short_row_lp_matches_the_oracle_in_exact_sums_mode(gpu_required, row_order_mode, monkeypatch, policy):
    """Every row of A and A' within bitexact_row_limit(): batches of 3 and 9 take_steps in the loop are the exact-sums
    oracle's trajectory (take_step_constant / take_step_malitsky_pock(0.7, 0.99, 1.0)), bit for bit."""
    p = _problem("rows8_2000", lambda: H.rows_with_lens([8] * 300, 2000, 83))
    A = sp.csc_matrix(p.constraint_matrix)
    assert max(np.diff(A.indptr).max(), np.diff(A.tocsr().indptr).max()) <= H.bitexact_row_limit()
    pol = POLICIES[policy]
    _set_env(monkeypatch, "1")
    st = H.oracle_from_problem(p)
    eng = HipPdhgEngine.from_problem(p)
    try:
        st.exact_sums = True
        st.step_size, st.primal_weight = _start(p, pol)
        st.ratio_step_sizes = 1.0
        dev = PdhgSolverState(eng, step_size=st.step_size, primal_weight=st.primal_weight, ratio_step_sizes=1.0)
        for batch in (3, 9):
            assert take_steps(pol, dev, batch) == batch and not dev.numerical_error
            for _ in range(batch):
                if pol is CONSTANT:
                    st.take_step_constant()
                else:
                    st.take_step_malitsky_pock(0.7, 0.99, 1.0)
            x, y = eng.get_current()
            assert dev.total_number_iterations == st.total_number_iterations, batch
            assert _same(np.float64(dev.step_size), np.float64(st.step_size)), batch
            assert dev.cumulative_kkt_passes == st.cumulative_kkt_passes, batch
            assert _same(x, st.x) and _same(y, st.y), batch
        assert eng.steps_info()[0] == 0 and eng.steps_info()[1] >= 2
    finally:
        eng.close()
        st.close()


# ---- 10: a fleet's singly stepped medium members -----------------------------------------------------------------------
@pytest.mark.parametrize("policy", list(POLICIES))
def test_a_fleets_medium_members_step_in_the_loop(gpu_required, row_order_mode, monkeypatch, policy):
    """A small LP (the fleet's shared launch may carry it) beside the 5001-column LP and, for the constant policy, the
    arrow QP, which the fleet steps singly: under PDHG_DEVICE_LOOP=1 those members' take_steps are the persistent
    kernel's, bitwise those under 0, and the fleet carries and steps singly whom it did."""
    pol = POLICIES[policy]
    problems = [random_lp(40, 50, 3, seed=41), _lp_5001()]
    if pol is CONSTANT:
        problems.append(_problem("arrow_qp_5001", lambda: _arrow_qp(5001)))
    K = len(problems)
    start = [_start(q, pol) for q in problems]
    ss0, pw = np.array([s for s, _ in start]), np.array([w for _, w in start])
    ns = np.full(K, 8, dtype=np.int64)
    out = {}
    for setting in ("0", "1"):
        _set_env(monkeypatch, setting, base={"PDHG_GRAPH": "1", "PDHG_COOP": "1"})
        fleet = HipPdhgFleet.from_problems(problems, device_id=0)
        try:
            if pol is CONSTANT:
                kkt, done = fleet.take_steps_constant(ns, ss0, pw, np.zeros(K))
                rec = [kkt]
            else:
                ss, ratio, it, kkt, err, done = fleet.take_steps_malitsky_pock(ns, 0.7, 0.99, 1.0, ss0, np.ones(K), pw,
                                                                               np.zeros(K, dtype=np.int64), np.zeros(K))
                assert not np.any(err)
                rec = [ss, ratio, it, kkt]
            assert list(done) == [8] * K
            for mb in fleet.members:
                rec += list(mb.get_current()) + [mb.get_dual_product()] + list(mb.get_average()) + [np.array(mb.average_info())]
            info = fleet.info()
            out[setting] = (rec, [int(mb.steps_info()[1]) for mb in fleet.members], (info["carried"], info["single"]))
        finally:
            fleet.close()
    assert all(v == 0 for v in out["0"][1]), out["0"][1]
    assert out["1"][1][0] == 0 and all(v > 0 for v in out["1"][1][1:]), out["1"][1]
    assert out["0"][2] == out["1"][2] and out["1"][2][0] + out["1"][2][1] == K
    for a, b in zip(out["0"][0], out["1"][0]):
        assert _same(a, b)


# ---- 11: whole solves ----------------------------------------------------------------------------------------------------
def _params(policy, limit=300):
    from firstorderlp_jl_amd.saddle_point import RestartScheme, RestartToCurrentMetric, construct_restart_parameters
    from firstorderlp_jl_amd.termination import construct_termination_criteria
    tc = construct_termination_criteria(eps_optimal_absolute=1e-6, eps_optimal_relative=1e-6, iteration_limit=limit)
    rp = construct_restart_parameters(RestartScheme.ADAPTIVE_NORMALIZED, RestartToCurrentMetric.GAP_OVER_DISTANCE_SQUARED,
                                      1000, 0.5, 0.1, 0.9, 0.5, False)
    return PdhgParameters(10, False, 1.0, 1.0, True, 0, True, 40, tc, rp, policy)


@pytest.mark.parametrize("case", ["constant_lp", "malitsky_pock_lp", "constant_qp"])
def test_a_whole_solve_is_the_same_in_the_loop(gpu_required, row_order_mode, monkeypatch, case):
    """Rescaling, evaluations, restarts and primal-weight updates between the batches: termination reason, iteration
    count, KKT passes, solutions and every statistic but the times are those of the launch-by-launch solve."""
    if case == "constant_qp":
        p = _problem("family_300x240", lambda: random_qp_family(300, 240, 1, 11)[0])
    else:
        p = _problem("random_300x240_whole", lambda: random_lp(300, 240, 5, seed=11))
    params = _params(MALITSKY_POCK if case == "malitsky_pock_lp" else CONSTANT)
    _set_env(monkeypatch, None)
    launches = {}

    def solve(setting):
        monkeypatch.setenv("PDHG_DEVICE_LOOP", setting)

        def factory(problem):
            eng = HipPdhgEngine.from_problem(problem)
            close = eng.close

            def closing():
                launches[setting] = eng.steps_info()[:2]
                close()
            eng.close = closing
            return eng
        factory.takes_original_problem = True
        return optimize(params, p, engine_factory=factory)
    want, got = solve("0"), solve("1")
    assert launches["0"] == [0, 0] and launches["1"][0] == 0 and launches["1"][1] > 0, launches
    assert got.termination_reason == want.termination_reason and got.iteration_count == want.iteration_count
    assert _same(got.primal_solution, want.primal_solution) and _same(got.dual_solution, want.dual_solution)
    assert [_stats_key(s) for s in got.iteration_stats] == [_stats_key(s) for s in want.iteration_stats]
    assert got.iteration_stats[-1].cumulative_kkt_matrix_passes == want.iteration_stats[-1].cumulative_kkt_matrix_passes
