"""The one-workgroup LDS kernel (csrc/small_lp_kernel.hpp: small_lp_steps_body) against the CPU oracle at its edges:
degenerate shapes, the three eligibility bounds of small_lp_eligible (LDS bytes, entries per row, entries per column) on
both sides, the thread-count boundary, the 8-entry loop and tail of small_row_sum, and the equality split at its ends.

Every LP runs twice: as a member of a HipPdhgFleet stepped by take_steps_adaptive with n_steps >= 2 (the shared launch,
small_lp_fleet_kernel, carries the eligible ones: info()["carried"] / ["single"] are asserted) and through a solo
HipPdhgEngine with take_steps (small_lp_steps_kernel: layout_info()["small_lp"] is asserted).  Both are compared, bit
for bit, with an exact-sums oracle trajectory of as many take_step_adaptive calls -- step size, counters,
numerical_error, steps done, x, y, A'y and the averages.  Ineligible LPs take the other launch paths and must equal the
oracle all the same (strict row order, which the file runs in: every row here is summed left to right)."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import folp_loader

folp = folp_loader.load()
from firstorderlp_jl_amd import HipPdhgEngine, HipPdhgFleet  # noqa: E402
from firstorderlp_jl_amd.primal_dual_hybrid_gradient import AdaptiveStepsizeParams, PdhgSolverState, take_steps  # noqa: E402
from firstorderlp_jl_amd.quadratic_programming import linear_programming_problem  # noqa: E402
from tests import helpers as H  # noqa: E402
from tests.test_gpu_edge_shapes import CASES  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.own_row_order]

RED, GROW = 0.3, 0.6
POLICY = AdaptiveStepsizeParams(RED, GROW)
_CSRC = os.path.join(os.path.dirname(os.path.abspath(folp.__file__)), "csrc")


def _const(name):
    with open(os.path.join(_CSRC, "small_lp_kernel.hpp")) as f:
        return int(re.search(r"constexpr int %s = (\d+);" % name, f.read()).group(1))


SMALL_MAX_ROW = _const("SMALL_MAX_ROW")        # 256 entries per row and per column
SMALL_FEW_ROWS = _const("SMALL_FEW_ROWS")      # 256 threads up to max(n, m) = 256, 1024 beyond
LDS_DOUBLES = 144 * 1024 // 8                  # host_small_lp.hpp: 8 * (9 n + 4 m) <= 144 KiB


def _lds_doubles(p):
    m, n = p.constraint_matrix.shape
    return 9 * n + 4 * m


def _max_row_and_col(p):
    A = p.constraint_matrix
    if A.nnz == 0:
        return 0, 0
    return int(np.diff(sp.csr_matrix(A).indptr).max()), int(np.diff(sp.csc_matrix(A).indptr).max())


def _eligible(p):
    """small_lp_eligible restated from the matrix (LPs on one device, none large enough for a tiled or slab layout)."""
    m, n = p.constraint_matrix.shape
    r, c = _max_row_and_col(p)
    return n > 0 and m > 0 and r <= SMALL_MAX_ROW and c <= SMALL_MAX_ROW and _lds_doubles(p) <= LDS_DOUBLES


def _same(a, b):
    """Bit for bit, NaNs in the same places (0 / 0 of an average without weight carries either sign)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(H._bits64(a[~nan]), H._bits64(b[~nan]))


def _oracle_run(p, n_steps, step, weight):
    o = H.oracle_from_problem(p)
    try:
        o.exact_sums = True
        o.step_size, o.primal_weight = step, weight
        done = 0
        while done < n_steps and not o.numerical_error:
            o.take_step_adaptive(RED, GROW)
            done += 1
        xa, ya = o.compute_average()
        return dict(step_size=o.step_size, total_number_iterations=o.total_number_iterations,
                    cumulative_kkt_passes=o.cumulative_kkt_passes, numerical_error=o.numerical_error, steps_done=done,
                    x=o.x, y=o.y, aty=o.aty, x_avg=xa, y_avg=ya)
    finally:
        o.close()


def _vectors(eng):
    x, y = eng.get_current()
    xa, ya = eng.get_average()
    return dict(x=x, y=y, aty=eng.get_dual_product(), x_avg=xa, y_avg=ya)


def _assert_is_oracle(got, want, label):
    assert H._bits64(got["step_size"]) == H._bits64(want["step_size"]), \
        f"{label}: step size {got['step_size']!r} != {want['step_size']!r}"
    for key in ("total_number_iterations", "cumulative_kkt_passes", "numerical_error", "steps_done"):
        assert got[key] == want[key], f"{label}: {key} {got[key]} != {want[key]}"
    for key in ("x", "y", "aty", "x_avg", "y_avg"):
        assert _same(got[key], want[key]), f"{label}: {key}"


def _check(problems, n_steps, starts=None, launches=None):
    """problems: the fleet's members; starts: (step size, primal weight) per member (default: the solver's own initial
    ones).  Eligibility is derived from each matrix; returns it per member."""
    K = len(problems)
    starts = starts or [H.initial_step_and_weight(p) for p in problems]
    ss0 = np.array([s for s, _ in starts])
    pw0 = np.array([w for _, w in starts])
    eligible = [_eligible(p) for p in problems]
    want = [_oracle_run(p, n_steps, ss0[k], pw0[k]) for k, p in enumerate(problems)]
    assert n_steps >= 2
    fleet = HipPdhgFleet.from_problems(problems, device_id=0)
    try:
        launches0 = fleet.info()["shared_launches"]
        ss, it, kkt, err, done = fleet.take_steps_adaptive(n_steps, RED, GROW, ss0, pw0, np.zeros(K, dtype=np.int64), np.zeros(K))
        info = fleet.info()
        assert info["members"] == K
        assert (info["carried"], info["single"]) == (sum(eligible), K - sum(eligible)), (info, eligible)
        if launches is not None:
            assert info["shared_launches"] - launches0 == launches, info
        for k in range(K):
            got = dict(step_size=ss[k], total_number_iterations=int(it[k]), cumulative_kkt_passes=float(kkt[k]),
                       numerical_error=bool(err[k]), steps_done=int(done[k]), **_vectors(fleet.members[k]))
            _assert_is_oracle(got, want[k], f"fleet member {k}")
    finally:
        fleet.close()
    for k, p in enumerate(problems):
        eng = HipPdhgEngine.from_problem(p, device_id=0)
        try:
            assert eng.layout_info()["small_lp"] == int(eligible[k]), f"solo {k}: small_lp"
            st = PdhgSolverState(eng, step_size=float(ss0[k]), primal_weight=float(pw0[k]))
            steps = take_steps(POLICY, st, n_steps)
            got = dict(step_size=st.step_size, total_number_iterations=st.total_number_iterations,
                       cumulative_kkt_passes=st.cumulative_kkt_passes, numerical_error=st.numerical_error, steps_done=steps,
                       **_vectors(eng))
            _assert_is_oracle(got, want[k], f"solo {k}")
        finally:
            eng.close()
    return eligible, want


def test_degenerate_shapes(gpu_required):
    """1 x 1, an all-zero 3 x 3 matrix, empty rows and columns, a single column and a single row ride the shared launch;
    no_constraints (m = 0) is ineligible and stepped singly.  A member that raises numerical_error inside the launch
    stops where the oracle stops."""
    names = sorted(CASES)
    problems = [CASES[k]() for k in names]
    eligible, want = _check(problems, 12, starts=[(0.3, 1.0)] * len(names))
    assert dict(zip(names, eligible)) == {"all_zero_matrix": True, "empty_rows_and_columns": True, "no_constraints": False,
                                          "one_by_one": True, "single_column": True, "single_row": True}
    # what the oracle's trajectories hold: a carried member (single_row) raises numerical_error before its 12 steps are
    # over, others reject trials on the way (more trials than steps)
    by_name = dict(zip(names, want))
    assert by_name["single_row"]["numerical_error"] and 0 < by_name["single_row"]["steps_done"] < 12
    assert any(not w["numerical_error"] and w["total_number_iterations"] > w["steps_done"] for w in want)


def _sparse_lp(m, n, seed, num_eq=None):
    """A random LP on an m x n matrix whose rows and columns stay well under SMALL_MAX_ROW entries whatever the shape:
    about six entries per row or column of the longer side, at most 200 per row or column of the shorter one on average."""
    rng = np.random.default_rng(seed)
    k = min(6 * max(m, n), 200 * min(m, n))
    A = sp.coo_matrix((rng.standard_normal(k), (rng.integers(0, m, k), rng.integers(0, n, k))), shape=(m, n)).tocsc()
    A.sum_duplicates()
    A.sort_indices()
    num_eq = m // 3 if num_eq is None else num_eq
    x0 = rng.random(n)
    b = A @ x0
    b[num_eq:] -= rng.random(m - num_eq)
    y0 = rng.standard_normal(m)
    y0[num_eq:] = np.abs(y0[num_eq:])
    c = A.T @ y0 + rng.random(n) * (rng.random(n) < 0.5)
    lb = np.where(rng.random(n) < 0.2, -np.inf, 0.0)
    ub = np.where(rng.random(n) < 0.5, np.inf, 2.0)
    return linear_programming_problem(lb, ub, c, 0.0, A, b, num_eq)


def test_lds_boundary(gpu_required):
    """9 n + 4 m = 18 432 doubles exactly, three ways (the 9 n part, the 4 m part, both): eligible and carried.  One row
    more is 4 doubles over: ineligible, stepped singly."""
    shapes = [(1600, 1008), (2044, 9), (4, 4599), (1600, 1009)]
    problems = [_sparse_lp(m, n, seed=20 + i) for i, (n, m) in enumerate(shapes)]
    assert [_lds_doubles(p) for p in problems[:3]] == [LDS_DOUBLES] * 3
    assert _lds_doubles(problems[3]) == LDS_DOUBLES + 4
    for p in problems:
        assert max(_max_row_and_col(p)) <= SMALL_MAX_ROW, _max_row_and_col(p)
    eligible, _ = _check(problems, 40)
    assert eligible == [True, True, True, False]


def test_row_length_boundary(gpu_required, monkeypatch):
    """A row of exactly SMALL_MAX_ROW = 256 entries is carried, one of 257 is not; the same for a column.  The ladder
    0, 1, 7, 8, 9, 16, 255, 256 walks small_row_sum's 8-entry loop and its tail: none, a tail alone, a full step alone,
    a step and a tail, whole steps only."""
    monkeypatch.setenv("PDHG_ROW_ORDER", "strict")
    lens = (0, 1, 7, 8, 9, 16, 255, 256)
    problems = [H.ladder_lp(lens, 31, blocks="rows"), H.ladder_lp(lens + (257,), 32, blocks="rows"),
                H.ladder_lp(lens, 33, blocks="cols"), H.ladder_lp(lens + (257,), 34, blocks="cols"),
                H.ladder_lp(lens, 35)]
    assert [_max_row_and_col(p) for p in problems[:4]] == [(256, 4), (257, 5), (4, 256), (5, 257)]
    assert _max_row_and_col(problems[4]) == (256, 256)
    A = problems[4].constraint_matrix
    assert set(lens) <= set(np.diff(sp.csr_matrix(A).indptr).tolist()) and set(lens) <= set(np.diff(A.indptr).tolist())
    eligible, _ = _check(problems, 30)
    assert eligible == [True, False, True, False, True]


def test_thread_count_boundary(gpu_required):
    """max(n, m) = 256 runs the 256-thread instantiation, 257 the 1024-thread one: one fleet, two shared launches."""
    problems = [_sparse_lp(200, 256, seed=41), _sparse_lp(256, 120, seed=42), _sparse_lp(257, 100, seed=43),
                _sparse_lp(150, 257, seed=44)]
    sizes = [max(p.constraint_matrix.shape) for p in problems]
    assert sizes == [SMALL_FEW_ROWS, SMALL_FEW_ROWS, SMALL_FEW_ROWS + 1, SMALL_FEW_ROWS + 1]
    eligible, _ = _check(problems, 40, launches=2)
    assert all(eligible)


def test_equality_split_at_its_ends(gpu_required):
    """num_eq = 0: row 0 is an inequality whose right-hand side is out of reach, so its y is projected to 0 at every
    step; num_eq = m: the last row is an equality with such a right-hand side, and its y must go negative."""
    problems = []
    for which in ("none", "all"):
        base = H.ladder_lp((0, 1, 7, 8, 9, 15, 16, 17, 40), seed=51)
        m = base.constraint_matrix.shape[0]
        b = base.right_hand_side.copy()
        b[0 if which == "none" else m - 1] = -50.0
        problems.append(linear_programming_problem(base.variable_lower_bound, base.variable_upper_bound, base.objective_vector,
                                                   0.0, base.constraint_matrix, b, 0 if which == "none" else m))
    eligible, want = _check(problems, 20)
    assert all(eligible)
    assert want[0]["y"][0] == 0.0 and (want[0]["y"] >= 0.0).all()
    assert want[1]["y"][-1] < 0.0
