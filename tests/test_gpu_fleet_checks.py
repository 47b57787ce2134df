"""A fleet's checks in shared launches (pdhg_fleet_eval_points / pdhg_fleet_trust_region_bounds; csrc/fleet_check_kernels.hpp):
termination evaluations and trust-region problems of many members in one call, one workgroup per member or problem.  Every
comparison is bitwise and made against solo ``HipPdhgEngine``s on the same problems driven the same way: the rows the fleet
calls return, what they leave in the members (the prefetched distances, the stored results that answer the member's own
calls without a launch), the split into carried and per-member items, staleness, argument errors, whole solves."""
import ctypes
import dataclasses
import math

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

pytestmark = [pytest.mark.gpu]

RED, GROW = 0.3, 0.6
CURRENT, AVERAGE, RESTART = _lib.POINT_CURRENT, _lib.POINT_AVERAGE, _lib.POINT_RESTART


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _qp():
    p = random_lp(60, 50, 4, seed=31)
    Q = sp.diags(np.linspace(0.5, 2.0, 50)).tocsc()
    return QuadraticProgrammingProblem(p.variable_lower_bound, p.variable_upper_bound, Q, p.objective_vector, 0.0,
                                       p.constraint_matrix, p.right_hand_side, p.num_equalities)


def _with_equalities(p, num_eq):
    return linear_programming_problem(p.variable_lower_bound, p.variable_upper_bound, p.objective_vector, 0.0,
                                      p.constraint_matrix, p.right_hand_side, num_eq)


# name, problem, rides in the shared check launches?  The smallest shapes at which each branch can go wrong:
def _members():
    return [
        ("1x1", H.example_lp_without_bounds(), True),                              # degenerate shape, infinite bounds on both sides
        ("30x30", random_lp(30, 30, 3, seed=1), True),                             # n + m = 60: less than one wave
        ("255x256", random_lp(255, 256, 3, seed=2), True),                         # n + m = 511: the last size with one virtual block
        ("256x256", random_lp(256, 256, 3, seed=3), True),                         # n + m = 512: the first with two
        ("2048x2048", random_lp(2048, 2048, 3, seed=4), True),                     # n + m = TRS_MAX, 9 virtual blocks; no small-LP steps
        ("2048x2049", random_lp(2048, 2049, 3, seed=5), False),                    # first size beyond TRS_MAX
        ("row256", H.ladder_lp([3] * 30 + [256], seed=6), True),                   # a row and a column of 256 entries
        ("row257", H.ladder_lp([3] * 30 + [257], seed=7), False),                  # ... of 257
        ("example_lp", H.example_lp(), True),
        ("no_equalities", _with_equalities(random_lp(40, 50, 3, seed=8), 0), True),
        ("all_equalities", _with_equalities(random_lp(40, 50, 3, seed=9), 40), True),
        ("qp", _qp(), False),
        # no edge of its own: the member that test_eval_points_are_the_solo_eval_points leaves alone (-1), so that every
        # member above is compared at every state
        ("spare", random_lp(20, 25, 3, seed=10), True),
    ]


class _Rig:
    """A fleet and solo engines on the same problems, rescaled the same way, with the original problem set, stepped
    side by side."""

    def __init__(self, members=None):
        self.members = members if members is not None else _members()
        self.names = [n for n, _, _ in self.members]
        self.problems = [p for _, p, _ in self.members]
        self.eligible = [e for _, _, e in self.members]
        self.K = len(self.problems)
        self.fleet = HipPdhgFleet.from_problems(self.problems, device_id=0)
        self.solos = [HipPdhgEngine.from_problem(p, device_id=0) for p in self.problems]
        self.scaling = []
        for p, a, b in zip(self.problems, self.fleet.members, self.solos):
            for eng in (a, b):
                E, D = eng.rescale(4, False, 1.0)
                self.scaling.append((E, D))
                eng.set_original_problem(E, D, p.objective_vector, p.right_hand_side, p.variable_lower_bound,
                                         p.variable_upper_bound)
        sw = [H.initial_step_and_weight(p) for p in self.problems]
        self.ss = np.array([s for s, _ in sw])
        self.pw = np.array([w for _, w in sw])
        self.it = np.zeros(self.K, dtype=np.int64)
        self.kkt = np.zeros(self.K)

    def close(self):
        self.fleet.close()
        for e in self.solos:
            e.close()

    def step(self, n):
        """n adaptive take_steps of every member through the fleet, and of every solo engine with the same scalars."""
        before = (self.ss.copy(), self.it.copy(), self.kkt.copy())
        self.ss, self.it, self.kkt, _, _ = self.fleet.take_steps_adaptive(n, RED, GROW, self.ss, self.pw, self.it, self.kkt)
        for k, e in enumerate(self.solos):
            e.take_steps_adaptive(n, RED, GROW, float(before[0][k]), float(self.pw[k]), int(before[1][k]), float(before[2][k]))

    def restart(self):
        for e in list(self.fleet.members) + self.solos:
            e.restart_to_average()
            e.reset_average()
            e.save_restart_point()

    def weights(self, k):
        """define_norms' uniform entries for member k's scalars."""
        return 1.0 / self.ss[k] * self.pw[k], 1.0 / self.ss[k] / self.pw[k]

    def have_average(self, k):
        cx, cy, _, _ = self.solos[k].average_info()
        return cx > 0 and cy > 0

    def points(self, k):
        return [CURRENT, RESTART] + ([AVERAGE] if self.have_average(k) else [])

    def states(self):
        """fresh -> 5 steps -> 40 steps -> restart + 8 steps; yields the state's name at each."""
        yield "fresh"
        self.step(5)
        yield "after 5 steps"
        self.step(35)
        yield "after 40 steps"
        self.restart()
        self.step(8)
        yield "after a restart and 8 steps"


@pytest.fixture
def rig(gpu_required):
    r = _Rig()
    yield r
    r.close()


def test_eval_points_are_the_solo_eval_points(rig):
    fleet = rig.fleet
    alone = rig.names.index("spare")                      # the member left alone
    for state in rig.states():
        for point in (AVERAGE, CURRENT):
            if point == AVERAGE and state == "fresh":
                continue                                  # (the empty average: test_argument_errors_change_nothing)
            label = f"{state}, point {point}"
            # (a member whose average is empty is asked for CURRENT: the 1x1 LP reaches its optimum in one step, every
            #  later step ends in a numerical error, and so no step is accepted after the restart has emptied the average)
            points = np.array([point if point != AVERAGE or rig.have_average(k) else CURRENT for k in range(rig.K)], dtype=np.int32)
            points[alone] = -1
            sentinel = np.full(24, 12345.678)
            before = fleet.members[alone].get_current()
            launches = fleet.check_info()["check_launches"]
            rows = fleet.eval_points(points)
            info = fleet.check_info()
            assert 1 <= info["check_launches"] - launches <= 3, (label, info)
            assert info["carried"] == sum(rig.eligible) - 1 and info["single"] == rig.K - sum(rig.eligible), (label, info)
            assert not rows[alone].any(), label               # the row of the skipped member is untouched (the binding's zeros)
            misses = info["misses"]
            for k in range(rig.K):
                if k == alone:
                    continue
                mem, solo, point_k = fleet.members[k], rig.solos[k], int(points[k])
                want = solo.eval_point(point_k)
                assert _same(rows[k], want), f"{label}: member {rig.names[k]}: {rows[k]} != {want}"
                # what the evaluation leaves for the rest of a check
                for pt in ([AVERAGE, CURRENT] if rig.have_average(k) else [CURRENT]):
                    assert _same(mem.distance_to_restart(pt), solo.distance_to_restart(pt)), f"{label}: {rig.names[k]}: distance {pt}"
                assert _same(mem.point_sumsq(point_k), solo.point_sumsq(point_k)), f"{label}: {rig.names[k]}: sumsq"
                # the member's own call answers from the stored result
                assert _same(mem.eval_point(point_k), want), f"{label}: member {rig.names[k]}: its own eval_point"
            assert fleet.check_info()["misses"] == misses, label
            # -1 through the raw call: the row of out keeps what it held
            raw = np.tile(sentinel, rig.K)
            nobody = np.full(rig.K, -1, dtype=np.int32)
            _lib.check(_lib.lib().pdhg_fleet_eval_points(fleet._h, nobody.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
                                                         raw.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))
            assert _same(raw, np.tile(sentinel, rig.K)), label
            x, y = fleet.members[alone].get_current()
            assert _same(x, before[0]) and _same(y, before[1])
        # the skipped member still evaluates as its solo twin (through its own call: a miss)
        misses = fleet.check_info()["misses"]
        assert _same(fleet.members[alone].eval_point(CURRENT), rig.solos[alone].eval_point(CURRENT)), state
        assert fleet.check_info()["misses"] == misses + 1, state
    # info() keeps its four keys, and its launches count the step launches only: one call of the final batch of steps
    # carried the small-LP members, the check launches are counted apart
    info = fleet.info()
    assert set(info) == {"members", "shared_launches", "carried", "single"} and info["members"] == rig.K, info
    assert info["carried"] + info["single"] == rig.K and 0 < info["shared_launches"] <= 2 * 4, info


def _tr_items(rig, k):
    """The trust-region problems of one member at its present state: (point, wp, wd, radius, range, approximate)."""
    wp, wd = rig.weights(k)
    solo = rig.solos[k]
    items = []
    for point in rig.points(k):
        if point == RESTART:
            radius = 0.75
        else:
            dx2, dy2 = solo.distance_to_restart(point)
            radius = math.sqrt(wp * dx2 + wd * dy2)       # compute_localized_duality_gaps' radius
        items.append((point, wp, wd, radius, 0, False))
    point = AVERAGE if rig.have_average(k) else CURRENT
    sx2, sy2 = solo.point_sumsq(point)
    px, py = max(1e-8, math.sqrt(wp * sx2)), max(1e-8, math.sqrt(wd * sy2))
    for rng in (1, 2):                                    # update_objective_bound_estimates: the two MAX_NORM halves
        items.append((point, wp / px ** 2, wd / py ** 2, 1.0, rng, False))
    items.append((CURRENT, wp, wd, 0.0, 0, False))        # radius 0
    items.append((CURRENT, wp, wd, 0.5, 0, True))         # the approximate form
    items.append((RESTART, 2.0 * wp, 0.5 * wd, 0.3, 2, True))
    return items


def test_trust_region_bounds_are_the_solo_bounds(rig):
    fleet = rig.fleet
    for state in rig.states():
        per_member = [_tr_items(rig, k) for k in range(rig.K)]
        # interleaved: items of different members, with different weights, side by side
        order = [(k, j) for j in range(max(len(v) for v in per_member)) for k in range(rig.K) if j < len(per_member[k])]
        items = [(k,) + per_member[k][j] for k, j in order]
        launches = fleet.check_info()["check_launches"]
        rows = fleet.trust_region_bounds(items)
        info = fleet.check_info()
        assert 1 <= info["check_launches"] - launches <= 3, (state, info)
        assert info["carried"] == sum(1 for it in items if rig.eligible[it[0]]), (state, info)
        assert info["single"] == sum(1 for it in items if not rig.eligible[it[0]]), (state, info)
        misses = info["misses"]
        for row, it in zip(rows, items):
            k = it[0]
            want = rig.solos[k].trust_region_bound(*it[1:])
            assert _same(row, want), f"{state}: member {rig.names[k]}, item {it[1:]}: {row} != {want}"
        # the members' own calls answer from the stored results -- a member holds at least six (here up to eight)
        for it in items:
            k = it[0]
            assert _same(fleet.members[k].trust_region_bound(*it[1:]), rig.solos[k].trust_region_bound(*it[1:])), (state, it)
        assert fleet.check_info()["misses"] == misses, state
        # ... and the three-at-once call reduces to them on small handles
        k = 1
        three = per_member[k][:2] + [per_member[k][-3]]
        got = fleet.members[k].trust_region_bounds([t[0] for t in three], three[0][1], three[0][2], [t[3] for t in three],
                                                   [t[4] for t in three], False)
        for g, t in zip(got, three):
            assert _same(g, rig.solos[k].trust_region_bound(*t)), state
        assert fleet.check_info()["misses"] == misses, state


def test_five_problems_of_one_member_in_one_call(rig):
    rig.step(12)
    fleet, k = rig.fleet, 2
    items = [(k,) + it for it in _tr_items(rig, k)[:5]]
    assert sorted(it[5] for it in items) == [0, 0, 0, 1, 2]
    rows = fleet.trust_region_bounds(items)
    info = fleet.check_info()
    assert info["carried"] == 5 and info["single"] == 0 and info["check_launches"] == 2, info   # products of three points, the searches
    for row, it in zip(rows, items):
        assert _same(row, rig.solos[k].trust_region_bound(*it[1:])), it
    assert fleet.info()["shared_launches"] >= 1 and set(fleet.info()) == {"members", "shared_launches", "carried", "single"}


def _tiny_members():
    """n = 3, m = 2 with one equality row: an LP, and the QP it becomes with a diagonal Q."""
    lp = random_lp(2, 3, 2, seed=41)
    qp = QuadraticProgrammingProblem(lp.variable_lower_bound, lp.variable_upper_bound, sp.diags([0.5, 1.0, 2.0]).tocsc(),
                                     lp.objective_vector, 0.0, lp.constraint_matrix, lp.right_hand_side, lp.num_equalities)
    return [("lp2x3", lp, True), ("qp2x3", qp, True)]


def test_an_average_materialised_for_the_distances_is_the_members_own(gpu_required, monkeypatch):
    """An evaluation at CURRENT asks for no products at AVERAGE, yet materialises the average (for the distances) and
    marks it fresh.  What the member then does at AVERAGE on its own -- the point, the distances, a search, whose
    products it computes itself from that average -- is the solo engine's, which never saw a shared call."""
    monkeypatch.setenv("PDHG_SMALL_QP", "1")                 # (the QP rides in the shared launches too)
    rig = _Rig(_tiny_members())
    try:
        for p in rig.problems:
            assert (p.num_constraints, p.num_variables, p.num_equalities) == (2, 3, 1)
        rig.step(4)
        assert all(rig.have_average(k) for k in range(rig.K))
        rig.fleet.eval_points(np.full(rig.K, CURRENT, dtype=np.int32))
        info = rig.fleet.check_info()
        assert info["carried"] == rig.K and info["single"] == 0, info
        for k, name in enumerate(rig.names):
            mem, solo = rig.fleet.members[k], rig.solos[k]
            for g, w in zip(mem.get_point(AVERAGE), solo.get_point(AVERAGE)):
                assert _same(g, w), f"{name}: the average {g} != {w}"
            assert _same(mem.distance_to_restart(AVERAGE), solo.distance_to_restart(AVERAGE)), f"{name}: distance"
            wp, wd = rig.weights(k)
            for approximate in (False, True):
                bound = (AVERAGE, wp, wd, 0.3, 0, approximate)
                got, want = mem.trust_region_bound(*bound), solo.trust_region_bound(*bound)
                assert _same(got, want), f"{name}: {got} != {want}"
    finally:
        rig.close()


def test_stored_results_go_stale_with_the_member(rig):
    rig.step(10)
    rig.restart()
    rig.step(6)
    fleet = rig.fleet
    k = 1
    mem, solo = fleet.members[k], rig.solos[k]
    wp, wd = rig.weights(k)
    tr_restart = (RESTART, wp, wd, 0.4, 0, False)
    tr_current = (CURRENT, wp, wd, 0.4, 0, False)

    def fleet_calls():
        fleet.eval_points(np.full(rig.K, CURRENT, dtype=np.int32))
        fleet.trust_region_bounds([(k,) + tr_restart, (k,) + tr_current])
        return fleet.check_info()["misses"]

    def step_both():
        out = []
        for e in (mem, solo):
            out.append(e.take_step_adaptive(RED, GROW, float(rig.ss[k]), float(rig.pw[k]), int(rig.it[k]), float(rig.kkt[k])))
        rig.ss[k], rig.it[k], rig.kkt[k] = out[0][0], out[0][1], out[0][2]

    # a step moves the state: the next calls compute again (misses) and equal the solo engine's
    misses = fleet_calls()
    assert _same(mem.eval_point(CURRENT), solo.eval_point(CURRENT)) and fleet.check_info()["misses"] == misses
    step_both()
    assert _same(mem.eval_point(CURRENT), solo.eval_point(CURRENT))
    assert _same(mem.trust_region_bound(*tr_current), solo.trust_region_bound(*tr_current))
    assert fleet.check_info()["misses"] == misses + 2
    # a new restart point: the result at the RESTART point is stale
    misses = fleet_calls()
    for e in (mem, solo):
        e.save_restart_point()
    assert _same(mem.trust_region_bound(*tr_restart), solo.trust_region_bound(*tr_restart))
    assert fleet.check_info()["misses"] == misses + 1
    # a rescaled matrix
    misses = fleet_calls()
    for e in (mem, solo):
        e.rescale(1, True, None)
    assert _same(mem.trust_region_bound(*tr_restart), solo.trust_region_bound(*tr_restart))
    assert _same(mem.eval_point(CURRENT), solo.eval_point(CURRENT))
    assert fleet.check_info()["misses"] == misses + 2
    # another original problem: the evaluation reads it, none of the three versions sees it
    misses = fleet_calls()
    p = rig.problems[k]
    E, D = rig.scaling[2 * k]
    for e in (mem, solo):
        e.set_original_problem(E, D, 2.0 * p.objective_vector, p.right_hand_side + 1.0, p.variable_lower_bound,
                               p.variable_upper_bound)
    assert _same(mem.eval_point(CURRENT), solo.eval_point(CURRENT))
    assert fleet.check_info()["misses"] == misses + 1
    # different bits of an argument are another problem
    misses = fleet_calls()
    other = (RESTART, wp, wd, float(np.nextafter(0.4, 1.0)), 0, False)
    assert _same(mem.trust_region_bound(*other), solo.trust_region_bound(*other))
    assert fleet.check_info()["misses"] == misses + 1
    # the member becomes a QP: nothing stored for the LP answers, and the fleet serves it by its own calls from now on
    misses = fleet_calls()
    Q = sp.diags(np.linspace(0.5, 2.0, p.num_variables)).tocsc()
    for e in (mem, solo):
        e._upload_objective_matrix(Q)
    assert _same(mem.trust_region_bound(*tr_current), solo.trust_region_bound(*tr_current))
    assert _same(mem.eval_point(CURRENT), solo.eval_point(CURRENT))
    assert fleet.check_info()["misses"] == misses + 2
    rows = fleet.eval_points(np.full(rig.K, CURRENT, dtype=np.int32))
    assert _same(rows[k], solo.eval_point(CURRENT))
    info = fleet.check_info()
    assert info["single"] == rig.K - sum(rig.eligible) + 1 and info["misses"] == misses + 2, info


def _snapshot(rig):
    out = []
    for e in rig.fleet.members:
        x, y = e.get_current()
        xa, ya = e.get_average()
        out.append((x, y, xa, ya, np.array(e.average_info())))
    return out


def test_argument_errors_change_nothing(rig):
    fleet, L = rig.fleet, _lib.lib()
    ip, dp = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double)
    K = rig.K
    before = _snapshot(rig)
    info = (fleet.info(), fleet.check_info())
    out = np.zeros(24 * K)

    def eval_rc(handle, pts):
        pts = np.ascontiguousarray(pts, dtype=np.int32)
        return L.pdhg_fleet_eval_points(handle, pts.ctypes.data_as(ip), out.ctypes.data_as(dp))

    def tr_rc(handle, member, point, rng):
        one = lambda v, t: np.array([v], dtype=t)
        tout = np.zeros(8)
        return L.pdhg_fleet_trust_region_bounds(
            handle, 1, one(member, np.int32).ctypes.data_as(ip), one(point, np.int32).ctypes.data_as(ip),
            one(1.0, np.float64).ctypes.data_as(dp), one(1.0, np.float64).ctypes.data_as(dp), one(0.5, np.float64).ctypes.data_as(dp),
            one(rng, np.int32).ctypes.data_as(ip), one(0, np.int32).ctypes.data_as(ip), tout.ctypes.data_as(dp))

    def last():
        return L.pdhg_last_error().decode()

    pts = np.full(K, CURRENT)
    pts[4] = AVERAGE
    assert eval_rc(fleet._h, pts) == -1 and "average is empty" in last() and "member 4" in last()
    pts[4] = 7
    assert eval_rc(fleet._h, pts) == -1 and "unknown point selector" in last() and "member 4" in last()
    assert eval_rc(fleet.members[0]._h, np.full(K, CURRENT)) == -1 and "not a fleet" in last()
    assert eval_rc(None, np.full(K, CURRENT)) == -1
    assert tr_rc(fleet._h, 2, CURRENT, 3) == -1 and "range must be 0, 1 or 2" in last() and "item 0" in last()
    assert tr_rc(fleet._h, 2, AVERAGE, 0) == -1 and "average is empty" in last()
    assert tr_rc(fleet._h, 2, 5, 0) == -1 and "unknown point selector" in last()
    assert tr_rc(fleet._h, K, CURRENT, 0) == -1
    assert tr_rc(fleet.members[0]._h, 0, CURRENT, 0) == -1 and "not a fleet" in last()
    with pytest.raises(_lib.PdhgHipError):
        fleet.eval_points(np.full(K, 3))
    assert (fleet.info(), fleet.check_info()) == info
    for a, b in zip(_snapshot(rig), before):
        assert all(_same(u, v) for u, v in zip(a, b))
    # a member without the original problem
    bare = HipPdhgFleet.from_problems([random_lp(20, 20, 3, seed=3)], device_id=0)
    try:
        assert eval_rc(bare._h, [CURRENT]) == -1 and "pdhg_set_original_problem" in last() and "member 0" in last()
        assert bare.check_info() == dict(check_launches=0, carried=0, single=0, misses=0)
    finally:
        bare.close()


def _params(record, scheme, tol=1e-6, limit=400, freq=7):
    tc = construct_termination_criteria(eps_optimal_absolute=tol, eps_optimal_relative=tol, iteration_limit=limit)
    rp = construct_restart_parameters(scheme, RestartToCurrentMetric.GAP_OVER_DISTANCE_SQUARED, 1000, 0.5, 0.1, 0.9, 0.5, False)
    return PdhgParameters(10, False, 1.0, 1.0, True, 0, record, freq, tc, rp, AdaptiveStepsizeParams(RED, GROW))


def _stats_key(s):
    d = dataclasses.asdict(s)
    d.pop("cumulative_time_sec")
    d["method_specific_stats"] = {k: v for k, v in d["method_specific_stats"].items() if "time" not in k}
    return repr(d)


def _solve_many(params, problems):
    infos = []

    def factory(ps):
        fleet = HipPdhgFleet.from_problems(ps, device_id=0)
        inner = fleet.close

        def close():
            if fleet._h:
                infos.append(fleet.check_info())
            inner()
        fleet.close = close
        return fleet
    factory.takes_original_problem = True
    return optimize_many(params, problems, fleet_factory=factory), infos[-1]


_WANT = {}


def _want(record, scheme, names):
    """optimize() per problem, computed once per parameter set and shared."""
    import os
    key = (record, scheme, os.environ.get("PDHG_ROW_ORDER"))
    if key not in _WANT:
        _WANT[key] = {n: optimize(_params(record, scheme), p) for n, p, _ in _members()}
    return [_WANT[key][n] for n in names]


@pytest.mark.parametrize("scheme", [RestartScheme.ADAPTIVE_NORMALIZED, RestartScheme.NO_RESTARTS], ids=["adaptive_normalized", "no_restarts"])
@pytest.mark.parametrize("record", [True, False], ids=["recorded", "unrecorded"])
def test_whole_solves_are_optimize_per_problem(gpu_required, record, scheme):
    members = _members()
    params = _params(record, scheme)
    for only_eligible in (True, False):
        # (the all-eligible list: a few of the shapes, so that the case stays short)
        chosen = [(n, p) for n, p, e in members if (n in ("30x30", "256x256", "row256", "example_lp") if only_eligible else
                                                    (e or n in ("qp", "2048x2049")))]
        names, problems = [n for n, _ in chosen], [p for _, p in chosen]
        want = _want(record, scheme, names)
        got, info = _solve_many(params, problems)
        for n, g, w in zip(names, got, want):
            assert g.termination_reason == w.termination_reason, n
            assert g.iteration_count == w.iteration_count, n
            assert _same(g.primal_solution, w.primal_solution) and _same(g.dual_solution, w.dual_solution), n
            assert [_stats_key(s) for s in g.iteration_stats] == [_stats_key(s) for s in w.iteration_stats], n
        assert info["check_launches"] > 0, info
        if only_eligible:
            # every device request of every check went through a shared launch
            assert info["misses"] == 0, info
