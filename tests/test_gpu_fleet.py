"""Fleets on the device (pdhg_create_fleet / pdhg_fleet_*): many independent small LPs stepped by one launch, one
workgroup per LP (csrc/small_lp_kernel.hpp: small_lp_fleet_kernel).  Every assertion is bitwise unless it says otherwise,
and is made against solo ``HipPdhgEngine``s on the same problems stepped with ``take_steps_adaptive``: step sizes,
iterates, averages, counters, whole solves; the members that cannot ride the shared launch; the fleet's lifetime and
argument checks."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

import folp_loader

folp = folp_loader.load()
from firstorderlp_jl_amd import HipPdhgEngine, HipPdhgFleet, _lib, optimize_many  # noqa: E402
from firstorderlp_jl_amd.generators import random_lp  # noqa: E402
from firstorderlp_jl_amd.primal_dual_hybrid_gradient import (AdaptiveStepsizeParams, PdhgParameters,  # noqa: E402
                                                             optimize)
from firstorderlp_jl_amd.quadratic_programming import (QuadraticProgrammingProblem,  # noqa: E402
                                                       linear_programming_problem)
from firstorderlp_jl_amd.saddle_point import (RestartScheme, RestartToCurrentMetric,  # noqa: E402
                                              construct_restart_parameters)
from firstorderlp_jl_amd.termination import construct_termination_criteria  # noqa: E402
from tests import helpers as H  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.short_rows]

RED, GROW = 0.3, 0.6


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


class _Scalars:
    """The host scalars of K members side by side (what the arrays of a fleet call hold)."""

    def __init__(self, problems):
        sw = [H.initial_step_and_weight(p) for p in problems]
        self.ss = np.array([s for s, _ in sw])
        self.pw = np.array([w for _, w in sw])
        self.it = np.zeros(len(problems), dtype=np.int64)
        self.kkt = np.zeros(len(problems))


def _fleet_call(fleet, sc, n_steps):
    sc.ss, sc.it, sc.kkt, err, done = fleet.take_steps_adaptive(n_steps, RED, GROW, sc.ss, sc.pw, sc.it, sc.kkt)
    return err, done


def _solo_call(eng, sc, k, n):
    """pdhg_take_steps_adaptive on a solo engine with member k's scalars (n == 0: no call, as the fleet leaves it)."""
    if n == 0:
        return False, 0
    sc.ss[k], sc.it[k], sc.kkt[k], err, done = eng.take_steps_adaptive(int(n), RED, GROW, float(sc.ss[k]), float(sc.pw[k]),
                                                                        int(sc.it[k]), float(sc.kkt[k]))
    return err, done


def _single_step(eng, sc, k):
    sc.ss[k], sc.it[k], sc.kkt[k], _ = eng.take_step_adaptive(RED, GROW, float(sc.ss[k]), float(sc.pw[k]), int(sc.it[k]),
                                                               float(sc.kkt[k]))


def _state(eng, trial=False):
    """Iterate, A'y, averages and their counters; trial=True: the trial buffers too (scratch of whichever launch path
    ran last, so only comparable where both sides took the same paths)."""
    x, y = eng.get_current()
    xa, ya = eng.get_average()
    out = dict(x=x, y=y, aty=eng.get_dual_product(), x_avg=xa, y_avg=ya, average_info=np.array(eng.average_info()))
    if trial:
        xn, yn, an = eng.get_trial()
        out.update(x_trial=xn, y_trial=yn, aty_trial=an)
    return out


def _assert_same_state(got, want, label):
    for key in want:
        assert np.array_equal(_bits(got[key]), _bits(want[key])), f"{label}: {key}"


def _assert_same_scalars(a, b, k, label):
    assert _bits(a.ss[k]) == _bits(b.ss[k]), f"{label}: step size {a.ss[k]!r} != {b.ss[k]!r}"
    assert a.it[k] == b.it[k], f"{label}: total_number_iterations {a.it[k]} != {b.it[k]}"
    assert _bits(a.kkt[k]) == _bits(b.kkt[k]), f"{label}: cumulative_kkt_passes"


def _mixed_problems():
    return [random_lp(30, 30, 3, seed=1), random_lp(1200, 900, 6, seed=7), random_lp(700, 1400, 9, seed=3), H.example_lp(),
            H.example_cc_lp()]           # the last: zero movement, numerical_error inside a call


def _run_mixed(problems, calls, singles_between, check_info=None):
    """Three (or more) fleet calls in a row with single take_steps between them on some members, against solo engines
    driven the same way."""
    K = len(problems)
    fleet = HipPdhgFleet.from_problems(problems, device_id=0)
    solos = [HipPdhgEngine.from_problem(p, device_id=0) for p in problems]
    try:
        fs, ss = _Scalars(problems), _Scalars(problems)
        for c, n_steps in enumerate(calls):
            err, done = _fleet_call(fleet, fs, n_steps)
            if check_info:
                check_info(c, fleet.info())
            for k in range(K):
                e, d = _solo_call(solos[k], ss, k, n_steps[k])
                label = f"call {c}, member {k}"
                assert (bool(err[k]), int(done[k])) == (bool(e), int(d)), f"{label}: (numerical_error, steps_done)"
                _assert_same_scalars(fs, ss, k, label)
            if c + 1 < len(calls):
                for k in singles_between:        # the deferred average update crosses the paths
                    _single_step(fleet.members[k], fs, k)
                    _single_step(solos[k], ss, k)
                    _assert_same_scalars(fs, ss, k, f"single step after call {c}, member {k}")
        for k in range(K):
            _assert_same_state(_state(fleet.members[k]), _state(solos[k]), f"member {k}")
    finally:
        fleet.close()
        for e in solos:
            e.close()


def test_mixed_fleet_is_the_solo_runs_bitwise(gpu_required):
    seen = []

    def check_info(c, info):
        seen.append(info)
        assert info["members"] == 5

    _run_mixed(_mixed_problems(), [[2, 64, 40, 3, 200], [64, 7, 40, 50, 5], [300, 200, 40, 50, 2]], singles_between=[0, 2, 3],
               check_info=check_info)
    # every member takes the solo small-LP path and asked for >= 2 steps: all five carried, by two launches per call
    # (256 threads for the three of up to 256 rows, 1024 for the other two)
    assert [i["carried"] for i in seen] == [5, 5, 5] and [i["single"] for i in seen] == [0, 0, 0]
    assert [i["shared_launches"] for i in seen] == [2, 4, 6]


def _three_hundred():
    out = []
    for k in range(300):
        if k % 3 == 0:
            out.append(random_lp(280 + 20 * (k % 7), 260 + 10 * (k % 5), 4, seed=1000 + k))     # beyond 256 rows: 1024 threads
        else:
            out.append(random_lp(20 + k % 50, 30 + k % 40, 3, seed=1000 + k))
    return out


def test_more_members_than_compute_units(gpu_required):
    problems = _three_hundred()
    fleet = HipPdhgFleet.from_problems(problems, device_id=0)
    try:
        fs, ss = _Scalars(problems), _Scalars(problems)
        err, done = _fleet_call(fleet, fs, np.full(300, 64))
        info = fleet.info()
        assert info == dict(members=300, shared_launches=2, carried=300, single=0), info
        for k, p in enumerate(problems):
            solo = HipPdhgEngine.from_problem(p, device_id=0)
            try:
                e, d = _solo_call(solo, ss, k, 64)
                assert (bool(err[k]), int(done[k])) == (bool(e), int(d)), k
                _assert_same_scalars(fs, ss, k, f"member {k}")
                _assert_same_state(_state(fleet.members[k]), _state(solo), f"member {k}")
            finally:
                solo.close()
    finally:
        fleet.close()


def test_a_member_with_zero_steps_is_untouched(gpu_required):
    problems = [random_lp(40, 50, 3, seed=21), random_lp(300, 280, 4, seed=22), random_lp(60, 30, 3, seed=23)]
    fleet = HipPdhgFleet.from_problems(problems, device_id=0)
    try:
        fs = _Scalars(problems)
        _fleet_call(fleet, fs, [10, 10, 10])
        before = _state(fleet.members[1], trial=True)
        scal = (fs.ss[1], fs.it[1], fs.kkt[1])
        err, done = _fleet_call(fleet, fs, [20, 0, 20])
        assert fleet.info()["carried"] == 2 and fleet.info()["single"] == 0
        _assert_same_state(_state(fleet.members[1], trial=True), before, "the member with n_steps == 0")
        assert (fs.ss[1], fs.it[1], fs.kkt[1]) == scal and done[1] == 0 and not err[1]
        assert done[0] == 20 and done[2] == 20
    finally:
        fleet.close()


def test_launches_that_end_inside_a_take_step(gpu_required, monkeypatch):
    """PDHG_STEPS_TEST_TABLE=3: a table of powers of 3 entries, so the shared launch returns after 3 trials, mostly inside
    a take_step (the first step is far too long: rejections); the member's step size on entry goes to the per-member
    continuation.  The solo engines run with the ordinary tables."""
    problems = [random_lp(300, 250, 5, seed=2), random_lp(40, 50, 3, seed=5), random_lp(600, 500, 5, seed=6)]
    K = len(problems)

    def scalars():
        sc = _Scalars(problems)
        sc.ss = sc.ss * 300.0
        return sc

    solos = [HipPdhgEngine.from_problem(p, device_id=0) for p in problems]
    want = []
    try:
        ss = scalars()
        for n in ([40, 12, 25], [40, 40, 40]):
            for k in range(K):
                _solo_call(solos[k], ss, k, n[k])
        want = [_state(e) for e in solos]
    finally:
        for e in solos:
            e.close()
    monkeypatch.setenv("PDHG_STEPS_TEST_TABLE", "3")
    fleet = HipPdhgFleet.from_problems(problems, device_id=0)
    try:
        fs = scalars()
        for n in ([40, 12, 25], [40, 40, 40]):
            err, done = _fleet_call(fleet, fs, n)
            assert list(done) == n and not err.any()
            assert fleet.info()["carried"] == 3
        for k in range(K):
            _assert_same_scalars(fs, ss, k, f"member {k}")
            _assert_same_state(_state(fleet.members[k]), want[k], f"member {k}")
        assert (fs.it > np.array([80, 52, 65])).all(), fs.it       # there were rejected trials
    finally:
        fleet.close()


def _long_row_lp():
    """300 x 900 with one dense row (900 entries) and one dense column: beyond the small-LP kernel's rows."""
    return H.skewed_lp(300, 900, seed=7, dense_rows=1, dense_cols=1, base_nnz=3)


def _qp():
    p = random_lp(60, 50, 4, seed=31)
    n = 50
    Q = sp.diags(np.linspace(0.5, 2.0, n)).tocsc()
    return QuadraticProgrammingProblem(p.variable_lower_bound, p.variable_upper_bound, Q, p.objective_vector, 0.0,
                                       p.constraint_matrix, p.right_hand_side, p.num_equalities)


@pytest.mark.parametrize("order", ["strict", "relaxed"])
def test_ineligible_members_are_stepped_singly(gpu_required, monkeypatch, order):
    """A QP and an LP with a row of 900 entries among small LPs: the shared launch carries the small ones, the call
    steps the other two with the per-member loop.  The QP and the small members are bitwise the solo runs in both row
    orders; the long-row member is bitwise in strict order, and in relaxed order (rows beyond 256 entries are summed
    wave-parallel, within 1e-13 * sum |a x| of the sequential sum per row) it is held to the tolerance
    tests/test_gpu_batch.py holds two runs to that sum such rows in that order: rtol 1e-9, atol 1e-12 * (1 + max |v|)."""
    monkeypatch.setenv("PDHG_ROW_ORDER", order)
    problems = [random_lp(40, 50, 3, seed=41), _qp(), random_lp(400, 300, 4, seed=42), _long_row_lp(),
                random_lp(25, 25, 3, seed=43)]
    K = len(problems)
    n_steps = [30, 12, 30, 6, 30]
    fleet = HipPdhgFleet.from_problems(problems, device_id=0)
    solos = [HipPdhgEngine.from_problem(p, device_id=0) for p in problems]
    try:
        fs, ss = _Scalars(problems), _Scalars(problems)
        err, done = _fleet_call(fleet, fs, n_steps)
        info = fleet.info()
        assert info["carried"] == 3 and info["single"] == 2, info
        for k in range(K):
            e, d = _solo_call(solos[k], ss, k, n_steps[k])
            assert (bool(err[k]), int(done[k])) == (bool(e), int(d)), k
            got, want = _state(fleet.members[k]), _state(solos[k])
            if k == 3 and order == "relaxed":
                assert fs.it[k] == ss.it[k]
                assert np.isclose(fs.ss[k], ss.ss[k], rtol=1e-9, atol=0)
                for key in ("x", "y", "aty", "x_avg", "y_avg"):
                    assert np.allclose(got[key], want[key], rtol=1e-9, atol=1e-12 * (1.0 + np.abs(want[key]).max())), key
            else:
                _assert_same_scalars(fs, ss, k, f"member {k} ({order})")
                _assert_same_state(got, want, f"member {k} ({order})")
    finally:
        fleet.close()
        for e in solos:
            e.close()


def _params(limit=20000, tol=1e-6):
    tc = construct_termination_criteria(eps_optimal_absolute=tol, eps_optimal_relative=tol, iteration_limit=limit)
    rp = construct_restart_parameters(RestartScheme.ADAPTIVE_NORMALIZED, RestartToCurrentMetric.GAP_OVER_DISTANCE_SQUARED,
                                      1000, 0.5, 0.1, 0.9, 0.5, False)
    return PdhgParameters(10, False, 1.0, 1.0, True, 0, True, 64, tc, rp, AdaptiveStepsizeParams(RED, GROW))


def _twelve():
    """Netlib-like shapes (27 x 32, 56 x 97 and neighbours), one infeasible; with the iteration limit of the test some
    stop there."""
    out = []
    for k in range(11):
        m, n = [(27, 32), (56, 97), (40, 60), (90, 120)][k % 4]
        out.append(random_lp(m, n, 4, seed=300 + k))
    bad = linear_programming_problem(np.zeros(3), np.full(3, 10.0), np.array([1.0, 2.0, 1.0]), 0.0,
                                     sp.csc_matrix(np.array([[1.0, 1.0, 0.0], [1.0, 1.0, 0.0], [0.0, 1.0, 1.0]])),
                                     np.array([1.0, 2.0, 1.0]), 1)
    out.insert(5, bad)
    return out


def _stats_key(s):
    import dataclasses
    d = dataclasses.asdict(s)
    d.pop("cumulative_time_sec")
    d["method_specific_stats"] = {k: v for k, v in d["method_specific_stats"].items() if "time" not in k}
    return repr(d)


def test_optimize_many_is_optimize_per_problem(gpu_required):
    problems = _twelve()
    params = _params(limit=1500)          # low enough that some members stop at it
    infos = []

    def factory(ps):
        fleet = HipPdhgFleet.from_problems(ps, device_id=0)
        inner = fleet.take_steps_adaptive

        def spy(*a, **k):
            out = inner(*a, **k)
            infos.append(fleet.info())
            return out
        fleet.take_steps_adaptive = spy
        return fleet
    factory.takes_original_problem = True

    want = [optimize(params, p) for p in problems]
    got = optimize_many(params, problems, fleet_factory=factory)
    assert len(got) == 12
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.termination_reason == w.termination_reason, k
        assert g.iteration_count == w.iteration_count, k
        assert np.array_equal(_bits(g.primal_solution), _bits(w.primal_solution)), k
        assert np.array_equal(_bits(g.dual_solution), _bits(w.dual_solution)), k
        assert [_stats_key(s) for s in g.iteration_stats] == [_stats_key(s) for s in w.iteration_stats], k
    reasons = {w.termination_string for w in want}
    assert {"OPTIMAL", "PRIMAL_INFEASIBLE", "ITERATION_LIMIT"} <= reasons, reasons
    assert infos and infos[-1]["shared_launches"] > 0 and max(i["carried"] for i in infos) >= 10, infos[-1]
    # the default factory gives the same
    again = optimize_many(params, problems[:3])
    for g, w in zip(again, want[:3]):
        assert g.iteration_count == w.iteration_count and np.array_equal(_bits(g.primal_solution), _bits(w.primal_solution))


def test_fleet_lifetime(gpu_required):
    problems = [random_lp(40, 50, 3, seed=51), random_lp(300, 280, 4, seed=52)]
    fleet = HipPdhgFleet.from_problems(problems, device_id=0)
    fs = _Scalars(problems)
    fleet.members[0].close()                               # a view: forgets its handle, frees nothing
    assert fleet.members[0]._h is None
    L = _lib.lib()
    mh = fleet.members[1]._h
    L.pdhg_destroy(mh)                                     # a member's destroy does nothing
    err, done = _fleet_call(fleet, fs, [16, 16])
    assert list(done) == [16, 16] and fleet.info()["carried"] == 2
    x, y = fleet.members[1].get_current()
    assert np.isfinite(x).all() and np.isfinite(y).all()
    fleet.close()
    fleet.close()                                          # harmless
    assert fleet._h is None and all(e._h is None for e in fleet.members)


def test_argument_errors_launch_nothing(gpu_required):
    problems = [random_lp(40, 50, 3, seed=61), random_lp(30, 20, 3, seed=62)]
    fleet = HipPdhgFleet.from_problems(problems, device_id=0)
    try:
        L = _lib.lib()
        dp, ip, cp = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int)
        sc = _Scalars(problems)
        ns = np.array([5, -1], dtype=np.int64)
        err = np.zeros(2, dtype=np.int32)
        done = np.zeros(2, dtype=np.int64)
        before = [_state(e) for e in fleet.members]

        def call(handle, ns_p=ns.ctypes.data_as(ip), ss_p=sc.ss.ctypes.data_as(dp), done_p=done.ctypes.data_as(ip)):
            return L.pdhg_fleet_take_steps_adaptive(handle, ns_p, RED, GROW, ss_p, sc.pw.ctypes.data_as(dp),
                                                    sc.it.ctypes.data_as(ip), sc.kkt.ctypes.data_as(dp),
                                                    err.ctypes.data_as(cp), done_p)
        assert call(fleet._h) < 0                                          # n_steps[1] < 0
        ns[1] = 5
        assert call(fleet._h, ns_p=None) < 0 and call(fleet._h, ss_p=None) < 0 and call(fleet._h, done_p=None) < 0
        assert call(None) < 0
        assert call(fleet.members[0]._h) < 0                               # a member where the fleet is expected
        out = np.zeros(5)
        assert L.pdhg_trial_step(fleet._h, 0.1, 1.0, 1.0, out.ctypes.data_as(dp)) < 0     # the fleet where a member is expected
        info = np.zeros(8, dtype=np.int64)
        assert L.pdhg_fleet_info(fleet.members[0]._h, info.ctypes.data_as(ip)) < 0
        mh = ctypes.c_void_p()
        assert L.pdhg_fleet_add(fleet.members[0]._h, 0, 0, 0, None, None, None, 0, None, None, None, None, 0, ctypes.byref(mh)) < 0
        # nothing was launched, nothing moved
        assert fleet.info() == dict(members=2, shared_launches=0, carried=0, single=0)
        assert (sc.it == 0).all() and (done == 0).all()
        for e, b in zip(fleet.members, before):
            _assert_same_state(_state(e), b, "after the refused calls")
    finally:
        fleet.close()
