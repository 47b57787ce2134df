"""Small QPs in a fleet's shared check launches (PDHG_SMALL_QP=1; csrc/fleet_check_kernels.hpp: fleet_qp_point_products_kernel,
fleet_qp_eval_kernel, and fleet_tr_kernel with Q x): pdhg_fleet_eval_points / pdhg_fleet_trust_region_bounds carry a QP member
whose CSR(Q) is plain with rows of at most 256 entries, beside the LPs.  Every comparison is bitwise and made against solo
``HipPdhgEngine``s on the same problems driven the same way (the rig of tests/test_gpu_fleet_checks.py, built with the switch
on): the rows, what they leave in the members, the split into carried and per-member items, the switch read per call, an LP
that becomes a QP, argument errors, whole solves against ``optimize`` with the switch off.  Both row orders."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

from firstorderlp_jl_amd import _lib
from firstorderlp_jl_amd.generators import random_lp
from firstorderlp_jl_amd.primal_dual_hybrid_gradient import optimize
from firstorderlp_jl_amd.saddle_point import RestartScheme
from tests import helpers as H
from tests import test_gpu_fleet_checks as FC
from tests.test_gpu_small_qp import _diag_qp, _long_row_qp, _nonsym_qp, _with_q

pytestmark = [pytest.mark.gpu]

CURRENT, AVERAGE = _lib.POINT_CURRENT, _lib.POINT_AVERAGE
_same = FC._same


def _diag(n):
    return sp.diags(np.linspace(0.5, 2.0, n))


def _gappy_qp():
    """Q holds an entry on every other column's diagonal alone, the first of them a stored 0.0: empty rows, a stored zero."""
    p = random_lp(60, 50, 4, seed=33)
    idx = np.arange(0, 50, 2)
    vals = np.linspace(0.5, 2.0, len(idx))
    vals[0] = 0.0
    q = _with_q(p, sp.csc_matrix((vals, (idx, idx)), shape=(50, 50)))
    Q = sp.csr_matrix(q.objective_matrix)
    assert Q.nnz == 25 and Q.data[0] == 0.0 and (np.diff(Q.indptr) == 0).sum() == 25
    return q


# name, problem, rides in the shared check launches with the switch on?  The smallest shapes at which each branch can go wrong:
def _members():
    return [
        ("example_qp", H.example_qp(), True),                                      # n = 2, m = 1
        ("example_qp2", H.example_qp2(), True),
        ("diag_60x50", _diag_qp(60, 50, 31), True),                                # less than one virtual block
        ("diag_255x256", _diag_qp(255, 256, 2, nnz_per_row=3), True),              # n + m = 511: the last size with one virtual block
        ("diag_256x256", _diag_qp(256, 256, 3, nnz_per_row=3), True),              # n + m = 512: the first with two
        ("diag_2048x2048", _diag_qp(2048, 2048, 4, nnz_per_row=3), True),          # n + m = TRS_MAX, nine virtual blocks
        ("diag_2048x2049", _diag_qp(2048, 2049, 5, nnz_per_row=3), False),         # first size beyond TRS_MAX
        ("q_row_256", _long_row_qp(256, False), True),                             # a row of Q with 256 entries
        ("q_row_257", _long_row_qp(257, False), False),                            # ... with 257
        ("q_col_257", _long_row_qp(257, True), True),                              # a 257-entry COLUMN of Q: Q' is not read by a check
        ("a_row_257", _with_q(H.ladder_lp([3] * 30 + [257], seed=7), _diag(288)), False),   # the LP condition still applies
        ("nonsym_90x120", _nonsym_qp(90, 120, 9), True),                           # a swap of Q and Q' shows in the bits
        ("gappy", _gappy_qp(), True),                                              # empty rows of Q, a stored zero
        ("lds_8x1700", _diag_qp(8, 1700, 71, nnz_per_row=40), True),               # 11 n + 4 m doubles > 144 KiB: steps per launch, checks shared
        ("lp_30x30", random_lp(30, 30, 3, seed=1), True),                          # LPs beside the QPs
        ("lp_400x300", random_lp(400, 300, 4, seed=42), True),
        # the member that test_eval_points_are_the_solo_eval_points leaves alone (-1)
        ("spare", random_lp(20, 25, 3, seed=10), True),
    ]


def _is_qp(p):
    return p.objective_matrix is not None and sp.csr_matrix(p.objective_matrix).nnz > 0


@pytest.fixture
def switch_on(monkeypatch):
    monkeypatch.setenv("PDHG_SMALL_QP", "1")


@pytest.fixture
def rig(gpu_required, switch_on):
    r = FC._Rig(_members())
    yield r
    r.close()


def _small_rig(members):
    return FC._Rig(members)


def test_the_shapes_sit_where_the_table_says():
    by_name = {n: p for n, p, _ in _members()}
    p = by_name["a_row_257"]
    assert p.num_variables == 288 and np.diff(sp.csr_matrix(p.constraint_matrix).indptr).max() == 257
    p = by_name["q_col_257"]
    assert np.diff(sp.csr_matrix(p.objective_matrix).indptr).max() <= 16 and np.diff(sp.csc_matrix(p.objective_matrix).indptr).max() == 257
    p = by_name["lds_8x1700"]
    assert 8 * (11 * p.num_variables + 4 * p.num_constraints) > 144 * 1024 and p.num_variables + p.num_constraints <= 4096


def _point_x(eng, point):
    return (eng.get_current() if point == CURRENT else eng.get_average())[0]


# ---- 1. (fails without the feature: every QP counts as `single`)
def test_eval_points_are_the_solo_eval_points(rig, row_order_mode):
    fleet = rig.fleet
    alone = rig.names.index("spare")
    for state in rig.states():
        for point in (AVERAGE, CURRENT):
            if point == AVERAGE and state == "fresh":
                continue
            label = f"{state}, point {point}"
            points = np.array([point if point != AVERAGE or rig.have_average(k) else CURRENT for k in range(rig.K)], dtype=np.int32)
            points[alone] = -1
            launches = fleet.check_info()["check_launches"]
            rows = fleet.eval_points(points)
            info = fleet.check_info()
            # LP points, QP points, LP evaluations, QP evaluations; a part without stale products issues nothing
            assert 2 <= info["check_launches"] - launches <= 4, (label, info)
            assert info["carried"] == sum(rig.eligible) - 1 and info["single"] == rig.K - sum(rig.eligible), (label, info)
            assert not rows[alone].any(), label
            misses = info["misses"]
            with_qx = 0
            for k in range(rig.K):
                if k == alone:
                    continue
                mem, solo, point_k = fleet.members[k], rig.solos[k], int(points[k])
                want = solo.eval_point(point_k)
                assert _same(rows[k], want), f"{label}: member {rig.names[k]}: {rows[k]} != {want}"
                p = rig.problems[k]
                if _is_qp(p):
                    # x'Qx and |Qx|inf of the unscaled point are there whenever Q_o x_o is not zero
                    D = rig.scaling[2 * k][1]
                    qx = p.objective_matrix @ (_point_x(solo, point_k) / D)
                    if np.abs(qx).max() > 1e-9:
                        with_qx += 1
                        assert rows[k][20] != 0.0 and rows[k][21] > 0.0, f"{label}: member {rig.names[k]}: {rows[k][20:22]}"
                else:
                    assert rows[k][20] == 0.0 and rows[k][21] == 0.0, f"{label}: member {rig.names[k]}"
                for pt in ([AVERAGE, CURRENT] if rig.have_average(k) else [CURRENT]):
                    assert _same(mem.distance_to_restart(pt), solo.distance_to_restart(pt)), f"{label}: {rig.names[k]}: distance {pt}"
                assert _same(mem.point_sumsq(point_k), solo.point_sumsq(point_k)), f"{label}: {rig.names[k]}: sumsq"
                assert _same(mem.eval_point(point_k), want), f"{label}: member {rig.names[k]}: its own eval_point"
            assert fleet.check_info()["misses"] == misses, label
            assert state == "fresh" or with_qx > 0, label


# ---- 2.
def test_trust_region_bounds_are_the_solo_bounds(rig, row_order_mode):
    fleet = rig.fleet
    for state in rig.states():
        per_member = [FC._tr_items(rig, k) for k in range(rig.K)]
        order = [(k, j) for j in range(max(len(v) for v in per_member)) for k in range(rig.K) if j < len(per_member[k])]
        items = [(k,) + per_member[k][j] for k, j in order]
        assert {it[5] for it in items} == {0, 1, 2} and {bool(it[6]) for it in items} == {False, True}
        launches = fleet.check_info()["check_launches"]
        rows = fleet.trust_region_bounds(items)
        info = fleet.check_info()
        # LP points, QP points, ONE trust-region launch for all problems
        assert 1 <= info["check_launches"] - launches <= 3, (state, info)
        assert info["carried"] == sum(1 for it in items if rig.eligible[it[0]]), (state, info)
        assert info["single"] == sum(1 for it in items if not rig.eligible[it[0]]), (state, info)
        misses = info["misses"]
        for row, it in zip(rows, items):
            k = it[0]
            want = rig.solos[k].trust_region_bound(*it[1:])
            assert _same(row, want), f"{state}: member {rig.names[k]}, item {it[1:]}: {row} != {want}"
        for it in items:
            k = it[0]
            assert _same(fleet.members[k].trust_region_bound(*it[1:]), rig.solos[k].trust_region_bound(*it[1:])), (state, it)
        assert fleet.check_info()["misses"] == misses, state


def test_five_problems_of_one_qp_member_in_one_call(rig, row_order_mode):
    rig.step(12)
    fleet, k = rig.fleet, rig.names.index("nonsym_90x120")
    items = [(k,) + it for it in FC._tr_items(rig, k)[:5]]
    assert sorted(it[5] for it in items) == [0, 0, 0, 1, 2]
    launches = fleet.check_info()["check_launches"]
    rows = fleet.trust_region_bounds(items)
    info = fleet.check_info()
    # the products of three points of a QP (one launch of the QP point kernel; the LP part is empty: nothing), the searches
    assert info["carried"] == 5 and info["single"] == 0 and info["check_launches"] - launches == 2, info
    for row, it in zip(rows, items):
        assert _same(row, rig.solos[k].trust_region_bound(*it[1:])), it


# ---- 3.
def test_the_switch_is_read_at_every_call(rig, row_order_mode, monkeypatch):
    rig.step(9)
    fleet = rig.fleet
    qps = sum(1 for p, e in zip(rig.problems, rig.eligible) if e and _is_qp(p))
    assert qps > 0
    points = np.full(rig.K, CURRENT, dtype=np.int32)
    k = rig.names.index("nonsym_90x120")
    wp, wd = rig.weights(k)
    trs = [(k, CURRENT, wp, wd, 0.4, 0, False), (k, AVERAGE, wp, wd, 0.7, 1, False), (rig.names.index("lp_30x30"), CURRENT, 1.0, 1.0, 0.5, 0, True)]
    want = [s.eval_point(CURRENT) for s in rig.solos]
    want_tr = [rig.solos[it[0]].trust_region_bound(*it[1:]) for it in trs]
    for switch, riding in (("1", True), ("0", False), ("1", True)):
        monkeypatch.setenv("PDHG_SMALL_QP", switch)
        for e in (rig.fleet.members[k], rig.solos[k]):     # (new bits of the state: nothing cached or stored answers)
            e.take_step_adaptive(FC.RED, FC.GROW, float(rig.ss[k]), float(rig.pw[k]), int(rig.it[k]), float(rig.kkt[k]))
        want[k] = rig.solos[k].eval_point(CURRENT)
        want_tr[:2] = [rig.solos[k].trust_region_bound(*it[1:]) for it in trs[:2]]
        rows = fleet.eval_points(points)
        info = fleet.check_info()
        assert info["carried"] == sum(rig.eligible) - (0 if riding else qps), (switch, info)
        assert info["single"] == rig.K - info["carried"], (switch, info)
        for j in range(rig.K):
            assert _same(rows[j], want[j]), (switch, rig.names[j])
        got = fleet.trust_region_bounds(trs)
        info = fleet.check_info()
        assert (info["carried"], info["single"]) == ((3, 0) if riding else (1, 2)), (switch, info)
        for g, w in zip(got, want_tr):
            assert _same(g, w), switch


# ---- 4.
def test_an_lp_that_becomes_a_qp(gpu_required, switch_on, row_order_mode):
    rig = _small_rig([("lp_40x50", random_lp(40, 50, 3, seed=8), True), ("lp_30x30", random_lp(30, 30, 3, seed=1), True)])
    try:
        rig.step(10)
        fleet, k = rig.fleet, 0
        mem, solo = fleet.members[k], rig.solos[k]
        points = np.full(rig.K, CURRENT, dtype=np.int32)
        wp, wd = rig.weights(k)
        tr = (k, CURRENT, wp, wd, 0.4, 0, False)
        rows = fleet.eval_points(points)
        assert _same(rows[k], solo.eval_point(CURRENT)) and rows[k][21] == 0.0
        as_lp = rows[k].copy()
        tr_lp = fleet.trust_region_bounds([tr])[0].copy()
        assert fleet.check_info()["carried"] == 1
        Q = sp.csc_matrix(_nonsym_qp(40, 50, 8).objective_matrix)
        for e in (mem, solo):
            e._upload_objective_matrix(Q)
        for again in (False, True):
            if again:                                     # ... and the same after a second rescale
                for e in (mem, solo):
                    e.rescale(1, True, None)
            launches = fleet.check_info()["check_launches"]
            rows = fleet.eval_points(points)
            info = fleet.check_info()
            assert info["carried"] == 2 and info["single"] == 0, info
            assert info["check_launches"] - launches == 3, info        # QP points, LP evaluation, QP evaluation (the LP's products are fresh)
            want = solo.eval_point(CURRENT)
            assert _same(rows[k], want) and rows[k][20] != 0.0 and rows[k][21] > 0.0, (again, rows[k], want)
            assert not _same(rows[k], as_lp)
            got = fleet.trust_region_bounds([tr])[0]
            assert fleet.check_info()["carried"] == 1
            assert _same(got, solo.trust_region_bound(*tr[1:])) and not _same(got, tr_lp), again
            misses = fleet.check_info()["misses"]
            assert _same(mem.eval_point(CURRENT), want) and _same(mem.trust_region_bound(*tr[1:]), got)
            assert fleet.check_info()["misses"] == misses
    finally:
        rig.close()


# ---- 5.
def test_argument_errors_change_nothing(gpu_required, switch_on, row_order_mode):
    rig = _small_rig([("diag_60x50", _diag_qp(60, 50, 31), True), ("example_qp", H.example_qp(), True),
                      ("lp_30x30", random_lp(30, 30, 3, seed=1), True)])
    try:
        fleet, L, K = rig.fleet, _lib.lib(), rig.K
        ip, dp = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double)
        rig.step(6)
        rig.restart()                                     # the averages are empty again, the iterates are not zero
        want = fleet.eval_points(np.full(K, CURRENT, dtype=np.int32))
        wp, wd = rig.weights(0)
        tr = (0, CURRENT, wp, wd, 0.4, 0, False)
        want_tr = fleet.trust_region_bounds([tr])[0]
        before = FC._snapshot(rig)
        info = (fleet.info(), fleet.check_info())
        out = np.zeros(24 * K)

        def eval_rc(pts):
            pts = np.ascontiguousarray(pts, dtype=np.int32)
            return L.pdhg_fleet_eval_points(fleet._h, pts.ctypes.data_as(ip), out.ctypes.data_as(dp))

        def tr_rc(member, point, rng):
            one = lambda v, t: np.array([v], dtype=t)     # noqa: E731
            tout = np.zeros(8)
            return L.pdhg_fleet_trust_region_bounds(
                fleet._h, 1, one(member, np.int32).ctypes.data_as(ip), one(point, np.int32).ctypes.data_as(ip),
                one(1.0, np.float64).ctypes.data_as(dp), one(1.0, np.float64).ctypes.data_as(dp), one(0.5, np.float64).ctypes.data_as(dp),
                one(rng, np.int32).ctypes.data_as(ip), one(0, np.int32).ctypes.data_as(ip), tout.ctypes.data_as(dp))

        def last():
            return L.pdhg_last_error().decode()

        assert eval_rc([CURRENT, AVERAGE, CURRENT]) == -1 and "average is empty" in last() and "member 1" in last()
        assert eval_rc([CURRENT, CURRENT, 7]) == -1 and "unknown point selector" in last() and "member 2" in last()
        assert eval_rc([7, CURRENT, CURRENT]) == -1 and "unknown point selector" in last() and "member 0" in last()
        assert tr_rc(0, AVERAGE, 0) == -1 and "average is empty" in last()
        assert tr_rc(0, 5, 0) == -1 and "unknown point selector" in last()
        assert tr_rc(0, CURRENT, 3) == -1 and "range must be 0, 1 or 2" in last()
        assert not out.any()
        assert (fleet.info(), fleet.check_info()) == info
        for a, b in zip(FC._snapshot(rig), before):
            assert all(_same(u, v) for u, v in zip(a, b))
        # the stored results still answer, without a launch or a miss
        for k in range(K):
            assert _same(fleet.members[k].eval_point(CURRENT), want[k]) and _same(want[k], rig.solos[k].eval_point(CURRENT)), k
        assert _same(fleet.members[0].trust_region_bound(*tr[1:]), want_tr)
        assert (fleet.info(), fleet.check_info()) == info
    finally:
        rig.close()


# ---- 6.
_RIDING = ("example_qp", "diag_60x50", "nonsym_90x120", "q_col_257", "gappy")
_LPS = ("lp_30x30", "lp_400x300")
_NOT_RIDING = ("q_row_257", "a_row_257")
_WANT = {}


def _want(monkeypatch, record, scheme, row_order_mode, names):
    """optimize() per problem with the switch off, computed once per parameter set and row order and shared."""
    key = (record, scheme, row_order_mode)
    if key not in _WANT:
        monkeypatch.setenv("PDHG_SMALL_QP", "0")
        by_name = {n: p for n, p, _ in _members()}
        _WANT[key] = {n: optimize(FC._params(record, scheme), by_name[n]) for n in _RIDING + _LPS + _NOT_RIDING}
    return [_WANT[key][n] for n in names]


@pytest.mark.parametrize("scheme", [RestartScheme.ADAPTIVE_NORMALIZED, RestartScheme.NO_RESTARTS], ids=["adaptive_normalized", "no_restarts"])
@pytest.mark.parametrize("record", [True, False], ids=["recorded", "unrecorded"])
def test_whole_solves_are_optimize_per_problem(gpu_required, monkeypatch, row_order_mode, record, scheme):
    by_name = {n: p for n, p, _ in _members()}
    params = FC._params(record, scheme)
    for names in (_RIDING + _LPS, _RIDING + _LPS + _NOT_RIDING):
        want = _want(monkeypatch, record, scheme, row_order_mode, names)
        monkeypatch.setenv("PDHG_SMALL_QP", "1")
        got, info = FC._solve_many(params, [by_name[n] for n in names])
        for n, g, w in zip(names, got, want):
            assert g.termination_reason == w.termination_reason, n
            assert g.iteration_count == w.iteration_count, n
            assert _same(g.primal_solution, w.primal_solution) and _same(g.dual_solution, w.dual_solution), n
            assert [FC._stats_key(s) for s in g.iteration_stats] == [FC._stats_key(s) for s in w.iteration_stats], n
        assert info["check_launches"] > 0, info
        if names == _RIDING + _LPS:
            assert info["misses"] == 0, info               # every device request of every check went through a shared launch
