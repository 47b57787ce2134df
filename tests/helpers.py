"""Shared test helpers: the reference's test LPs
(test/shared_test_qp_problems.jl) restated as data, and glue between the
product's problem type and the CPU oracle."""
import dataclasses

import numpy as np
import pytest
import scipy.sparse as sp

from firstorderlp_jl_amd import (QuadraticProgrammingProblem,
                                 linear_programming_problem)
from oracle.oracle import OracleState
from tests.oracle_engine import OracleEngine

INF = np.inf


def example_lp():
    """test/shared_test_qp_problems.jl:30-44; optimum x=[1,0,6,2], y=[.5,4,0]."""
    return linear_programming_problem(
        [0.0, 0.0, 0.0, 0.0], [2.0, 4.0, 6.0, 3.0], [5.0, 2.0, 1.0, 1.0], -14.0,
        [[2.0, 1.0, 1.0, 2.0], [1.0, 0.0, 1.0, 0.0], [0.0, 0.0, 1.0, -1.0]],
        [12.0, 7.0, 1.0], 1)


def example_lp_without_bounds():
    """shared_test_qp_problems.jl:55-65; optimum x=[2], y=[1]."""
    return linear_programming_problem([-INF], [INF], [-1.0], 0.0, [[-1.0]],
                                      [-2.0], 0)


def example_qp():
    """shared_test_qp_problems.jl:79-93; optimum x=[.2,.8], y=[.2]."""
    return QuadraticProgrammingProblem(
        [0.0, 0.0], [1.0, 1.0], [[4.0, 0.0], [0.0, 1.0]], [-1.0, -1.0], -0.0,
        [[-1.0, -1.0]], [-1.0], 0)


def example_qp2():
    """shared_test_qp_problems.jl:107-121; optimum x=[.25,0], y=[0]."""
    return QuadraticProgrammingProblem(
        [0.0, 0.0], [1.0, 1.0], [[4.0, 0.0], [0.0, 1.0]], [-1.0, 1.0], -0.0,
        [[-1.0, -1.0]], [-1.0], 0)


def example_cc_lp():
    """shared_test_qp_problems.jl:139-153."""
    return linear_programming_problem(
        [0.0] * 6, [1.0] * 6, [-1.0, -1.0, 1.0, -1.0, 1.0, -1.0], 4.0,
        [[0.0, -1.0, 1.0, 0.0, 0.0, -1.0], [0.0, 0.0, 0.0, -1.0, 1.0, -1.0],
         [-1.0, -1.0, 0.0, 1.0, 0.0, 0.0]], [-1.0, -1.0, -1.0], 0)


def example_cc_star_lp():
    """shared_test_qp_problems.jl:160-174."""
    return linear_programming_problem(
        [0.0] * 6, [1.0] * 6, [-1.0, -1.0, -1.0, 1.0, 1.0, 1.0], 3.0,
        [[-1.0, -1.0, 0.0, 1.0, 0.0, 0.0], [-1.0, 0.0, -1.0, 0.0, 1.0, 0.0],
         [0.0, -1.0, -1.0, 0.0, 0.0, 1.0]], [-1.0, -1.0, -1.0], 0)


def example_lp_dependent_rows():
    """shared_test_qp_problems.jl:192-206."""
    return linear_programming_problem(
        [0.0] * 4, [INF] * 4, [1.0, 2.0, 3.0, 4.0], 0.0,
        [[1.0, 1.0, 1.0, 1.0], [1.0, 1.0, 1.0, 1.0], [1.0, 0.0, 0.0, 1.0]],
        [2.0, 2.0, 1.0], 3)


def oracle_from_problem(p):
    A, Q = p.constraint_matrix, p.objective_matrix
    return OracleState(A.shape[0], A.shape[1], A.indptr, A.indices, A.data,
                       p.objective_vector, p.right_hand_side,
                       p.variable_lower_bound, p.variable_upper_bound,
                       p.num_equalities, Q.indptr, Q.indices, Q.data)


def initial_step_and_weight(p):
    """pdhg.jl:821-826 (1/norm(A, Inf) = 1/max|A_ij|) and
    select_initial_primal_weight (saddle_point.jl:1049-1075, unit norms)."""
    A = p.constraint_matrix
    step = 1.0 / np.abs(A.data).max()
    cn = np.sqrt(np.sum(p.objective_vector ** 2))
    bn = np.sqrt(np.sum(p.right_hand_side ** 2))
    pw = cn / bn if cn > 0 and bn > 0 else 1.0
    return step, pw


def sparse_uniform(m, n, density, seed, fmt="csc"):
    """A random sparse matrix with uniform(0, 1) entries like sp.random's default, its cells drawn WITH replacement
    (repeats summed): sp.random draws without replacement from the m * n cells, seconds at 12 000 x 12 000."""
    rng = np.random.default_rng(seed)
    k = int(round(density * m * n))
    A = sp.coo_matrix((rng.random(k), (rng.integers(0, m, k), rng.integers(0, n, k))), shape=(m, n)).asformat(fmt)
    A.sum_duplicates()
    A.sort_indices()
    return A


def skewed_lp(m, n, seed, dense_rows=1, dense_cols=1, base_nnz=4):
    """Random LP with a few very long rows/columns (exercises the long-row
    split path, like the PageRank LP's dense equality row and the L1-SVM
    intercept column)."""
    rng = np.random.default_rng(seed)
    # the sparse part as triplets drawn with replacement (sp.random draws WITHOUT replacement from the m * n cells: 40-100 s
    # at 30 000 x 40 000; the few repeated cells are summed by the constructor below)
    k = int(round(min(1.0, base_nnz / n) * m * n))
    br, bc, bv = rng.integers(0, m, k), rng.integers(0, n, k), rng.standard_normal(k)
    # the dense rows 0 .. dense_rows - 1 and the dense columns n - 1, n - 2, ... replace what the sparse part holds there
    keep = (br >= dense_rows) & (bc < n - dense_cols)
    rows, cols, vals = [br[keep]], [bc[keep]], [bv[keep]]
    for r in range(dense_rows):
        rows.append(np.full(n, r)); cols.append(np.arange(n)); vals.append(rng.standard_normal(n))
    for c in range(dense_cols):
        rows.append(np.arange(dense_rows, m)); cols.append(np.full(m - dense_rows, n - 1 - c)); vals.append(rng.standard_normal(m - dense_rows))
    A = sp.csc_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(m, n))
    A.sort_indices()
    x0 = rng.random(n)
    num_eq = m // 3
    b = A @ x0
    b[num_eq:] -= rng.random(m - num_eq)
    y0 = rng.standard_normal(m)
    y0[num_eq:] = np.abs(y0[num_eq:])
    c = A.T @ y0 + rng.random(n) * (rng.random(n) < 0.5)
    lb = np.where(rng.random(n) < 0.2, -INF, 0.0)
    ub = np.where(rng.random(n) < 0.5, INF, 2.0)
    return linear_programming_problem(lb, ub, c, 0.0, A, b, num_eq)


def with_dense_rows_and_columns(m, n, k, seed):
    """random_lp plus two dense rows and two dense columns (long rows in both layouts)."""
    from firstorderlp_jl_amd import linear_programming_problem
    from firstorderlp_jl_amd.generators import random_lp
    p = random_lp(m, n, k, seed)
    rng = np.random.default_rng(seed + 1)
    A = p.constraint_matrix.tocsr()
    A = sp.vstack([sp.csr_matrix(rng.standard_normal((2, n))), A[2:]]).tocsc()
    A = sp.hstack([sp.csc_matrix(rng.standard_normal((m, 2))), A[:, 2:]]).tocsc()
    A.sort_indices()
    return linear_programming_problem(p.variable_lower_bound, p.variable_upper_bound, p.objective_vector, 0.0,
                                      A, p.right_hand_side, p.num_equalities)


def bitexact_row_limit():
    """Rows of at most this many entries are bit-identical to the oracle's sequential sums in the row order the test runs
    in (conftest.row_order_mode sets PDHG_ROW_ORDER): 2048 (BLOCK_NNZ) in strict order, 256 (RELAXED_MIN_ROW) in the
    shipped relaxed order; longer rows are within 1e-13 * sum |a x| of them (spmv_kernels.hpp)."""
    import os
    return 256 if os.environ.get("PDHG_ROW_ORDER", "relaxed") == "relaxed" else 2048


def assert_rows_match_oracle(got, want, row_nnz, abs_scale, label=""):
    """got / want: a product's rows on the device / from the oracle; row_nnz: entries per row; abs_scale: sum |a x| per
    row (or any bound of it).  Short rows bitwise, long rows within 1e-13 of the scale."""
    short = row_nnz <= bitexact_row_limit()
    assert np.array_equal(got[short], want[short]), label + ": short rows differ"
    if np.any(~short):
        assert np.all(np.abs(got[~short] - want[~short]) <= 1e-13 * abs_scale[~short] + 1e-300), label + ": long rows beyond 1e-13 * sum|a x|"


def assert_products_match_oracle(eng, A, x, y, forced_sweep=False, label=""):
    """A x and A'y of `eng` against the oracle's sequential loops in the row order the test runs in: rows up to the
    bit-exact limit bitwise, longer rows within 1e-13 * sum |a x| (and never worse than that anywhere).
    forced_sweep: PDHG_SPMV=tiled put the sweep on a matrix whose rows have long runs inside one tile (the builder itself
    would stream it).  In relaxed order a CHUNK holding a same-row run of more than 8 entries is tree-reduced as a whole
    (tiled_chunk_relaxed), so only rows of at most 8 entries are then guaranteed bitwise; strict order is unaffected."""
    import os
    from oracle import oracle as orc
    import scipy.sparse as sp
    A = sp.csc_matrix(A)
    m, n = A.shape
    relaxed = os.environ.get("PDHG_ROW_ORDER", "relaxed") == "relaxed"
    limit = (8 if forced_sweep else 256) if relaxed else 2048
    absA = abs(A).tocsr()
    for got, want, nnz_per, scale, name in (
            (eng.spmv(x), orc.spmv(m, n, A.indptr, A.indices, A.data, x), np.diff(A.tocsr().indptr), absA @ np.abs(x), "A x"),
            (eng.spmv_t(y), orc.spmv_t(m, n, A.indptr, A.indices, A.data, y), np.diff(A.indptr), absA.T @ np.abs(y), "A'y")):
        short = nnz_per <= limit
        assert np.array_equal(got[short], want[short]), f"{label} {name}: rows of <= {limit} entries differ from the oracle"
        assert np.all(np.abs(got - want) <= 1e-13 * scale + 1e-300), f"{label} {name}: beyond 1e-13 * sum |a x|"


LADDER_LENS = (0, 1, 7, 8, 9, 15, 16, 17, 127, 128, 129, 255, 256, 257, 384, 1024, 1025, 1152, 2047, 2048, 2049, 2176)


def ladder_lp(lens, seed, num_eq=None, blocks="both"):
    """An LP whose constraint matrix is block_diag(L, L'): row i of L has exactly lens[i] entries (distinct sorted columns,
    standard-normal values), so A's rows AND A's columns hold every length of `lens`: both products of a trial, A xbar
    and A'y', see every row length.  Bounds mix -inf / finite below, +inf / finite above and some lb == ub; b and c are
    random; num_eq defaults to m // 3.  blocks="rows": A = L alone (the lengths are A's rows', its columns stay short);
    blocks="cols": A = L' alone."""
    rng = np.random.default_rng(seed)
    lens = [int(v) for v in lens]
    rows_l, cols_l = len(lens), max(max(lens), 1)
    ri = np.repeat(np.arange(rows_l), lens)
    ci = np.concatenate([np.sort(rng.choice(cols_l, size=k, replace=False)) for k in lens] + [np.zeros(0, dtype=np.int64)])
    L = sp.csr_matrix((rng.standard_normal(len(ci)), (ri, ci.astype(np.int64))), shape=(rows_l, cols_l))
    A = {"both": lambda: sp.block_diag([L, L.T], format="csc"), "rows": L.tocsc, "cols": lambda: L.T.tocsc()}[blocks]()
    A.sort_indices()
    m, n = A.shape
    lb = np.where(rng.random(n) < 0.25, -INF, -rng.random(n))
    ub = np.where(rng.random(n) < 0.25, INF, 1.0 + rng.random(n))
    fixed = rng.random(n) < 0.1
    lb[fixed] = ub[fixed] = rng.standard_normal(int(fixed.sum()))
    b = rng.standard_normal(m)
    c = rng.standard_normal(n)
    return linear_programming_problem(lb, ub, c, 0.0, A, b, m // 3 if num_eq is None else int(num_eq))


_MATRIX_PARTS = []      # the last matrix assert_trial_matches_oracle saw, and what it derives from it


def _matrix_parts(A):
    """(|A| in CSR, |A|' in CSR, entries per row, entries per column) of A, kept for the next call with the same matrix
    object."""
    if not (_MATRIX_PARTS and _MATRIX_PARTS[0] is A):
        Ar = sp.csr_matrix(A)
        Aa = abs(Ar)
        _MATRIX_PARTS[:] = [A, Aa, sp.csr_matrix(Aa.T), np.diff(Ar.indptr), np.diff(sp.csc_matrix(A).indptr)]
    return _MATRIX_PARTS[1:]


def _bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def assert_trial_matches_oracle(got_raw, got_trial, oracle_state, step, weight, A, label="", theta=1.0, dual_only=False,
                                Q=None):
    """One trial of a device path against the CPU oracle's from the same state.  got_raw: the five sums the device
    returned; got_trial: its (x', y', A'y'); oracle_state: an OracleState holding the iterate the device trial started
    from (left holding its own trial vectors); A: the constraint matrix.  The oracle runs trial_step(step, weight, theta)
    with exact sums -- with dual_only (the retries of a Malitsky-Pock step) trial_dual(step, weight, theta) from the x' its
    own trial_primal left.  x' bitwise; y' bitwise on rows of at most bitexact_row_limit() entries, longer rows within
    1e-13 * sigma * sum |a xbar| + 4 eps |y'| (sigma = weight * step); A'y' bitwise on columns of at most the limit whose
    rows are all short, elsewhere within |A|'|dy'| + 1e-13 |A|'|y'| + 4 eps |A'y'|; the four sums bitwise when every row
    and column is short, else to rtol 1e-9; out[4] == 0.  Returns (long rows, long columns) of A.

    Q: the objective matrix of a QP (the oracle state was built with it).  A row of Q beyond the limit puts the same
    1e-13 * sum |q x| on that entry of Q x, so x' is bitwise on the other entries and within
    tau * 1e-13 * sum |q x| + 4 eps |x'| there (tau = step / weight); what x' differs by reaches y' through
    sigma (1 + theta) |A| |dx'|, which joins its bar, and only rows that touch no such entry stay bitwise.  The fifth sum,
    0.5 dx'Q dx, is held like the other four: bitwise when every row and column of A and of Q is short, else rtol 1e-9."""
    eps = np.finfo(np.float64).eps
    lim = bitexact_row_limit()
    Aa, AaT, row_nnz, col_nnz = _matrix_parts(A)
    oracle_state.exact_sums = True
    x_prev = oracle_state.x
    if dual_only:
        want_raw, wx, wy, wa = oracle_state.trial_dual(step, weight, theta)
    else:
        want_raw, wx, wy, wa = oracle_state.trial_step(step, weight, theta)
    gx, gy, ga = got_trial
    got_raw = np.asarray(got_raw, dtype=np.float64)
    q_short = True
    loose_x = np.zeros(len(wx), dtype=bool)
    if Q is not None:
        Qr = sp.csr_matrix(Q)
        loose_x = np.diff(Qr.indptr) > lim
        q_short = not loose_x.any() and (np.diff(sp.csc_matrix(Q).indptr) <= lim).all()
        tol_x = 1e-13 * (step / weight) * (abs(Qr) @ np.abs(x_prev)) + 4 * eps * np.abs(wx)
        assert np.all(np.abs(gx - wx)[loose_x] <= tol_x[loose_x]), label + ": x' on long rows of Q"
    assert np.array_equal(_bits64(gx[~loose_x]), _bits64(wx[~loose_x])), label + ": x'"
    dx = np.abs(gx - wx)
    short_r = row_nnz <= lim
    clean_r = short_r & (Aa @ loose_x.astype(float) == 0)
    assert np.array_equal(_bits64(gy[clean_r]), _bits64(wy[clean_r])), label + ": y' on short rows"
    sigma = weight * step
    xbar = wx + theta * (wx - x_prev)
    tol_y = 1e-13 * sigma * (Aa @ np.abs(xbar)) + 4 * eps * np.abs(wy) + sigma * (1.0 + abs(theta)) * (Aa @ dx)
    assert np.all(np.abs(gy - wy) <= tol_y), label + ": y' on long rows beyond 1e-13 * sigma * sum |a xbar|"
    short_c = col_nnz <= lim
    clean = short_c & (AaT @ (~clean_r).astype(float) == 0)
    assert np.array_equal(_bits64(ga[clean]), _bits64(wa[clean])), label + ": A'y' on short columns of short rows"
    tol_a = AaT @ np.abs(gy - wy) + 1e-13 * (AaT @ np.abs(wy)) + 4 * eps * np.abs(wa)
    assert np.all(np.abs(ga - wa) <= tol_a), label + ": A'y' beyond the relaxed bar"
    bitwise_sums = short_r.all() and short_c.all() and q_short
    if bitwise_sums:
        assert np.array_equal(_bits64(got_raw[:4]), _bits64(want_raw[:4])), label + ": sums"
    else:
        assert np.allclose(got_raw[:4], want_raw[:4], rtol=1e-9, atol=0), label + ": sums"
    if Q is None:
        assert got_raw[4] == 0.0, label + ": out[4]"
    elif bitwise_sums:
        assert _bits64(got_raw[4]) == _bits64(want_raw[4]), label + ": 0.5 dx'Q dx"
    else:
        assert np.isclose(got_raw[4], want_raw[4], rtol=1e-9, atol=0), label + ": 0.5 dx'Q dx"
    return int((~short_r).sum()), int((~short_c).sum())


def rows_with_lens(lens, n, seed, num_eq=None):
    """An LP with len(lens) rows over n columns: row i holds exactly lens[i] entries, a window of consecutive columns
    (wrapped) from a random start, standard-normal values.  Bounds mix -inf / finite below, +inf / finite above and some
    lb == ub; b and c are random; num_eq defaults to m // 3."""
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens, dtype=np.int64)
    m = len(lens)
    assert lens.max(initial=0) <= n
    start = rng.integers(0, n, m)
    ci = np.concatenate([(s + np.arange(k)) % n for s, k in zip(start, lens)] + [np.zeros(0, dtype=np.int64)])
    A = sp.csr_matrix((rng.standard_normal(len(ci)), ci, np.concatenate([[0], np.cumsum(lens)])), shape=(m, n)).tocsc()
    A.sort_indices()
    lb = np.where(rng.random(n) < 0.25, -INF, -rng.random(n))
    ub = np.where(rng.random(n) < 0.25, INF, 1.0 + rng.random(n))
    fixed = rng.random(n) < 0.1
    lb[fixed] = ub[fixed] = rng.standard_normal(int(fixed.sum()))
    return linear_programming_problem(lb, ub, rng.standard_normal(n), 0.0, A, rng.standard_normal(m),
                                      m // 3 if num_eq is None else int(num_eq))


# ---- what the re-solve tests share (test_resolve_host, test_batch_resolve_host, test_gpu_resolve, test_gpu_batch_resolve) ----
def stats_key(s):
    d = dataclasses.asdict(s)
    d.pop("cumulative_time_sec")
    d["method_specific_stats"] = {k: v for k, v in d["method_specific_stats"].items() if "time" not in k}
    return repr(d)


def assert_same_output(got, want):
    assert got.termination_reason == want.termination_reason
    assert got.iteration_count == want.iteration_count
    assert np.array_equal(got.primal_solution, want.primal_solution, equal_nan=True)
    assert np.array_equal(got.dual_solution, want.dual_solution, equal_nan=True)
    assert [stats_key(s) for s in got.iteration_stats] == [stats_key(s) for s in want.iteration_stats]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(got, want, label=""):
    for name, g, w in zip(("c", "b", "lb", "ub"), got, want):
        assert np.array_equal(bits(g), bits(w)), f"{label}: {name} differs at {np.nonzero(bits(g) != bits(w))[0][:5]}"


def edge_bounds(n, rng):
    """Bounds that hold -inf, +inf, +0.0, -0.0 and lb == ub."""
    lb = rng.choice([-np.inf, 0.0, -0.0, -1.5, 0.25], size=n)
    free = np.isneginf(lb)
    ub = np.where(free, 0.0, lb) + rng.choice([np.inf, 0.0, 2.0, 0.125], size=n)
    ub[free] = rng.choice([np.inf, 0.0, -0.0, 3.0], size=int(free.sum()))
    return lb, ub


def raises_naming(exc, words, call):
    with pytest.raises(exc) as info:
        call()
    assert any(w in str(info.value) for w in words), str(info.value)


class ResolveOracleEngine(OracleEngine):
    """``OracleEngine`` with the two calls a session needs, in numpy: the oracle holds the problem's vectors in its own
    state and has no setter for them, so an update builds a new oracle state over the same matrix; a warm start is a new
    state too (everything empty) at the given point."""

    def __init__(self, constraint_matrix, objective_vector, right_hand_side, variable_lower_bound, variable_upper_bound,
                 num_equalities, objective_matrix=None):
        super().__init__(constraint_matrix, objective_vector, right_hand_side, variable_lower_bound, variable_upper_bound,
                         num_equalities, objective_matrix)
        self._vectors = [np.array(v, dtype=np.float64) for v in (objective_vector, right_hand_side, variable_lower_bound,
                                                                 variable_upper_bound)]
        self._num_eq, self._Qm = num_equalities, objective_matrix

    def _rebuild(self):
        self.st.close()
        OracleEngine.__init__(self, self._A, *self._vectors, self._num_eq, self._Qm)

    def update_problem_vectors(self, objective_vector=None, right_hand_side=None, variable_lower_bound=None,
                               variable_upper_bound=None):
        for k, v in enumerate((objective_vector, right_hand_side, variable_lower_bound, variable_upper_bound)):
            if v is not None:
                assert np.shape(v) == self._vectors[k].shape
                self._vectors[k] = np.array(v, dtype=np.float64)
        self._rebuild()

    def warm_start(self, x=None, y=None):
        self._rebuild()
        if x is not None or y is not None:
            self.set_current(x, y)
