"""Small QPs in the one-workgroup LDS kernel (csrc/small_lp_kernel.hpp: the QP form of small_lp_steps_body behind
small_qp_steps_kernel / small_qp_constant_kernel and their fleet forms), switched on by PDHG_SMALL_QP=1.

A QP step is the LP step plus Q x in the gradient, Q' dx and one more double-double sum; the element arithmetic, the
left-to-right row sums and the step rule are those of the per-launch path, so every result must be BITWISE what the same
library gives with PDHG_SMALL_QP=0 (one launch per trial) -- step sizes, iterates, A'y, averages, counters -- and what
the CPU oracle gives in exact-sums mode.  Every test runs in both row orders (the row_order_mode fixture).  The shapes
sit on the edges of the class: the LDS bound 8 (11 n + 4 m) <= 144 KiB, rows of Q and of Q' of 256 / 257 entries, the
thread classes (max(n, m) = 256 / 257), more than one element per thread, the 8-entry step of the row sum."""
import numpy as np
import pytest
import scipy.sparse as sp

from firstorderlp_jl_amd import HipPdhgEngine, HipPdhgFleet, optimize_many
from firstorderlp_jl_amd.generators import random_lp
from firstorderlp_jl_amd.primal_dual_hybrid_gradient import optimize
from firstorderlp_jl_amd.quadratic_programming import QuadraticProgrammingProblem
from tests import helpers as H

pytestmark = pytest.mark.gpu

RED, GROW = 0.3, 0.6
BATCHES = (2, 7, 51)          # 60 adaptive steps
CONSTANT = 40


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---------------------------------------------------------------------------------------------------------- problems
def _with_q(p, Q):
    Q = sp.csc_matrix(Q)
    Q.sort_indices()
    return QuadraticProgrammingProblem(p.variable_lower_bound, p.variable_upper_bound, Q, p.objective_vector, 0.0,
                                       p.constraint_matrix, p.right_hand_side, p.num_equalities)


def _diag_qp(m, n, seed, nnz_per_row=4):
    return _with_q(random_lp(m, n, nnz_per_row, seed=seed), sp.diags(np.linspace(0.5, 2.0, n)))


def _random_qp(m, n, seed, nnz_per_row=5):
    """random_lp plus Q = B'B + diag (tests/test_gpu_native_take_step.py: _random_qp), at small n."""
    B = sp.random(max(n // 3, 1), n, density=3.0 / n, format="csr", random_state=seed + 1)
    return _with_q(random_lp(m, n, nnz_per_row, seed=seed), B.T @ B + sp.diags(np.linspace(0.0, 0.5, n)))


def _window_matrix(lens, n, seed, scale, span=None):
    """n x n, row i holds lens[i % len(lens)] entries: a window of consecutive columns (wrapped inside the first `span`
    columns) from a random start.  Not symmetric."""
    rng = np.random.default_rng(seed)
    span = n if span is None else span
    lens = np.array([lens[i % len(lens)] for i in range(n)], dtype=np.int64)
    assert lens.max() <= span
    start = rng.integers(0, span, n)
    ci = np.concatenate([np.sort((s + np.arange(k)) % span) for s, k in zip(start, lens)] + [np.zeros(0, dtype=np.int64)])
    return sp.csr_matrix((scale * rng.standard_normal(len(ci)), ci, np.concatenate([[0], np.cumsum(lens)])), shape=(n, n))


def _nonsym_qp(m, n, seed, lens=(3, 5, 2), scale=0.05, transpose=False, span=None):
    """A sparse NON-SYMMETRIC Q (the library does not ask for symmetry): small off-diagonal windows plus a positive
    diagonal.  A swap of Q and Q' shows."""
    W = _window_matrix(lens, n, seed + 7, scale, span)
    Q = (W.T if transpose else W) + sp.diags(np.linspace(0.2, 1.0, n))
    return _with_q(random_lp(m, n, min(5, n), seed=seed), Q)


def _long_row_qp(row_len, transpose, seed=61):
    """300 columns, one row of Q (transpose: one column) with exactly `row_len` entries, the others short."""
    n = 300
    lens = [row_len] + [3] * (n - 1)
    W = _window_matrix(lens, n, seed, 0.01).tolil()
    W.setdiag(0.0)                 # the diagonal comes back below: the long row keeps exactly row_len entries
    W = sp.csr_matrix(W)
    W.eliminate_zeros()
    # the window of row 0 may have held its diagonal: count again and top up
    row0 = set(W[0].indices.tolist())
    free = [j for j in range(1, n) if j not in row0]
    need = row_len - 1 - len(row0)
    W = W.tolil()
    for j in free[:max(need, 0)]:
        W[0, j] = 0.01
    W = sp.csr_matrix(W) + sp.diags(np.linspace(0.2, 1.0, n))
    W = sp.csr_matrix(W)
    assert np.diff(W.indptr)[0] == row_len and np.diff(W.indptr)[1:].max() <= 8
    return _with_q(random_lp(40, n, 5, seed=seed), W.T if transpose else W)


def _lds_edge_qp(n):
    """m = 8: 11 n + 32 doubles of LDS.  Q: a diagonal plus a few entries off it."""
    rng = np.random.default_rng(n)
    off = sp.coo_matrix((0.05 * rng.standard_normal(6), (rng.integers(0, n, 6), rng.integers(0, n, 6))), shape=(n, n))
    return _with_q(random_lp(8, n, 40, seed=n), sp.diags(np.linspace(0.5, 2.0, n)) + off)


# ------------------------------------------------------------------------------------------------------------- runs
def _state(eng):
    x, y = eng.get_current()
    xa, ya = eng.get_average()
    return dict(x=x, y=y, aty=eng.get_dual_product(), x_avg=xa, y_avg=ya, average_info=np.array(eng.average_info()))


def _run(monkeypatch, p, switch, batches=BATCHES, constant=CONSTANT, step_scale=1.0, single_first=False, table=None,
         lp_steps_first=0):
    """An engine made and stepped with PDHG_SMALL_QP=switch: the adaptive batches, then `constant` constant steps with
    the step size they left.  lp_steps_first: the engine starts as the LP (no Q), takes that many steps, and gets Q by
    pdhg_set_objective_matrix.  Returns (state, small launches per batch incl. the constant one, small_lp bit)."""
    monkeypatch.setenv("PDHG_SMALL_QP", switch)
    if table is None:
        monkeypatch.delenv("PDHG_STEPS_TEST_TABLE", raising=False)
    else:
        monkeypatch.setenv("PDHG_STEPS_TEST_TABLE", str(table))
    step, pw = H.initial_step_and_weight(p)
    ss, it, kkt, err = step * step_scale, 0, 0.0, False
    if lp_steps_first:
        eng = HipPdhgEngine(p.constraint_matrix, p.objective_vector, p.right_hand_side, p.variable_lower_bound,
                            p.variable_upper_bound, p.num_equalities)
    else:
        eng = HipPdhgEngine.from_problem(p)
    try:
        if lp_steps_first:
            assert eng.layout_info()["small_lp"] == 1                 # an LP of the class whatever the switch says
            ss, it, kkt, err, _ = eng.take_steps_adaptive(lp_steps_first, RED, GROW, ss, pw, it, kkt)
            eng._upload_objective_matrix(p.objective_matrix)
        bit = eng.layout_info()["small_lp"]
        sizes, launches = [], []
        if single_first:
            ss, it, kkt, err = eng.take_step_adaptive(RED, GROW, ss, pw, it, kkt)
        for k in batches:
            if err:
                break
            before = eng.steps_info()[0]
            ss, it, kkt, err, done = eng.take_steps_adaptive(k, RED, GROW, ss, pw, it, kkt)
            assert done == k or err
            sizes.append(ss)
            launches.append(eng.steps_info()[0] - before)
        if constant and not err:
            before = eng.steps_info()[0]
            kkt, done = eng.take_steps_constant(constant, ss, pw, kkt)
            assert done == constant
            launches.append(eng.steps_info()[0] - before)
        out = _state(eng)
        out.update(step_sizes=np.array(sizes), total_number_iterations=np.array(it), cumulative_kkt_passes=np.array(kkt),
                   numerical_error=np.array(int(err)))
        return out, launches, bit
    finally:
        eng.close()


def _assert_same(got, want, label=""):
    assert got.keys() == want.keys()
    for key in want:
        assert np.array_equal(_bits(got[key]), _bits(want[key])), f"{label}: {key}"


_TWINS = {}


def _twin(monkeypatch, row_order_mode, name, maker, **kw):
    """The per-launch run (PDHG_SMALL_QP=0) of a problem, computed once per row order and left unchanged."""
    key = (row_order_mode, name, tuple(sorted(kw.items())))
    if key not in _TWINS:
        p = maker()
        want, launches, bit = _run(monkeypatch, p, "0", **kw)
        assert bit == 0 and launches == [0] * len(launches), (name, bit, launches)
        _TWINS[key] = (p, want)
    return _TWINS[key]


SHAPES = {
    "example_qp": H.example_qp,                                     # n = 2, m = 1
    "diagonal_60x50": lambda: _diag_qp(60, 50, 31),
    "btb_300x280": lambda: _random_qp(300, 280, 4),
    "nonsymmetric_90x120": lambda: _nonsym_qp(90, 120, 9),
}


# ---- 1. the same bits as the per-launch path
@pytest.mark.parametrize("name", list(SHAPES))
def test_small_qp_batches_are_bitwise_the_per_launch_path(gpu_required, monkeypatch, row_order_mode, name):
    p, want = _twin(monkeypatch, row_order_mode, name, SHAPES[name])
    got, launches, bit = _run(monkeypatch, p, "1")
    assert bit == 1 and launches == [1] * len(launches), (bit, launches)
    _assert_same(got, want, name)


def test_a_swap_of_q_and_its_transpose_would_show(gpu_required, monkeypatch, row_order_mode):
    """The non-symmetric shape against its transpose, per launch: other bits -- the case above can tell the copies apart."""
    _, a = _twin(monkeypatch, row_order_mode, "nonsymmetric_90x120", SHAPES["nonsymmetric_90x120"])
    _, b = _twin(monkeypatch, row_order_mode, "nonsymmetric_90x120'", lambda: _nonsym_qp(90, 120, 9, transpose=True))
    assert not np.array_equal(_bits(a["x"]), _bits(b["x"]))


# ---- 2. the same bits as the oracle in exact-sums mode
@pytest.mark.parametrize("name", ["diagonal_60x50", "btb_300x280"])
def test_small_qp_matches_the_oracle_in_exact_sums_mode(gpu_required, monkeypatch, row_order_mode, name):
    p = SHAPES[name]()
    got, launches, bit = _run(monkeypatch, p, "1", batches=(64, 64, 64, 8), constant=0)
    assert bit == 1 and launches == [1, 1, 1, 1]
    st = H.oracle_from_problem(p)
    st.exact_sums = True
    st.step_size, st.primal_weight = H.initial_step_and_weight(p)
    for _ in range(200):
        st.take_step_adaptive(RED, GROW)
    assert st.total_number_iterations == int(got["total_number_iterations"])
    assert _bits(st.step_size) == _bits(got["step_sizes"][-1])
    assert np.array_equal(_bits(got["x"]), _bits(st.x)) and np.array_equal(_bits(got["y"]), _bits(st.y))


# ---- 3. which path ran (fails without the feature)
def test_the_switch_decides_which_path_runs(gpu_required, monkeypatch, row_order_mode):
    p = SHAPES["diagonal_60x50"]()
    on, launches_on, bit_on = _run(monkeypatch, p, "1", batches=(1, 2, 1, 7, 51))
    assert bit_on == 1 and launches_on == [0, 1, 0, 1, 1, 1], launches_on      # a single step launches nothing new
    off, launches_off, bit_off = _run(monkeypatch, p, "0", batches=(1, 2, 1, 7, 51))
    assert bit_off == 0 and launches_off == [0] * 6, launches_off
    _assert_same(on, off)
    monkeypatch.delenv("PDHG_SMALL_QP")                                          # the default is off
    eng = HipPdhgEngine.from_problem(p)
    try:
        assert eng.layout_info()["small_lp"] == 0 and eng.layout_describe()["small_lp"] is False
    finally:
        eng.close()
    monkeypatch.setenv("PDHG_SMALL_QP", "1")
    eng = HipPdhgEngine.from_problem(p)
    try:
        assert eng.layout_describe()["small_lp"] == "qp"
    finally:
        eng.close()
    monkeypatch.setenv("PDHG_SMALL_LP", "0")                                    # ... and PDHG_SMALL_LP=0 switches the class off
    _, launches_none, bit_none = _run(monkeypatch, p, "1")
    assert bit_none == 0 and launches_none == [0] * 4


# ---- 4. the edges of the class, both sides
EDGES = {
    # LDS: 11 * 1672 + 32 = 18 424 <= 18 432 doubles; 1673 is beyond (9 n + 4 m would still admit it as an LP)
    "lds_1672": (lambda: _lds_edge_qp(1672), 1),
    "lds_1673": (lambda: _lds_edge_qp(1673), 0),
    "q_row_256": (lambda: _long_row_qp(256, False), 1),
    "q_row_257": (lambda: _long_row_qp(257, False), 0),
    "q_col_256": (lambda: _long_row_qp(256, True), 1),
    "q_col_257": (lambda: _long_row_qp(257, True), 0),
    # thread classes: 256 threads up to max(n, m) = 256, 1024 beyond
    "threads_256": (lambda: _nonsym_qp(200, 256, 13), 1),
    "threads_257": (lambda: _nonsym_qp(200, 257, 13), 1),
    "threads_m_257": (lambda: _nonsym_qp(257, 100, 14), 1),
    # more than one element per thread
    "stride_1025": (lambda: _nonsym_qp(30, 1025, 15), 1),
    # the 8-entry step of the row sum: rows of Q with 0, 1, 7, 8, 9, 16 and 17 entries; no diagonal, the last column empty
    "row_steps": (lambda: _with_q(random_lp(40, 70, 5, seed=16), _window_matrix((0, 1, 7, 8, 9, 16, 17), 70, 17, 0.05, span=69)), 1),
    "col_steps": (lambda: _with_q(random_lp(40, 70, 5, seed=16), _window_matrix((0, 1, 7, 8, 9, 16, 17), 70, 17, 0.05, span=69).T), 1),
}


@pytest.mark.parametrize("name", list(EDGES))
def test_edges_of_the_class(gpu_required, monkeypatch, row_order_mode, name):
    maker, eligible = EDGES[name]
    kw = dict(batches=(2, 30), constant=8)
    p, want = _twin(monkeypatch, row_order_mode, name, maker, **kw)
    if name.startswith("row_steps"):
        Q = sp.csr_matrix(p.objective_matrix)
        assert set(np.diff(Q.indptr).tolist()) == {0, 1, 7, 8, 9, 16, 17} and np.diff(sp.csc_matrix(Q).indptr)[-1] == 0
    got, launches, bit = _run(monkeypatch, p, "1", **kw)
    assert bit == eligible and launches == [eligible] * 3, (bit, launches)
    _assert_same(got, want, name)


# ---- 5. degenerate Q
def test_stored_zeros(gpu_required, monkeypatch, row_order_mode):
    base = random_lp(60, 50, 4, seed=31)
    # every stored entry 0.0: pdhg_set_objective_matrix keeps the handle an LP (all_zero), whatever the switch says
    zeros = _with_q(base, sp.csc_matrix((np.zeros(50), (np.arange(50), np.arange(50))), shape=(50, 50)))
    assert zeros.objective_matrix.nnz == 50
    lp, lp_launches, lp_bit = _run(monkeypatch, base, "0")
    for switch in ("0", "1"):
        got, launches, bit = _run(monkeypatch, zeros, switch)
        assert bit == 1 and launches == lp_launches == [1] * 4
        _assert_same(got, lp, f"all-zero Q, switch {switch}")
    # some stored zeros among the nonzeros
    Q = sp.csc_matrix(_nonsym_qp(60, 50, 31).objective_matrix)
    Q.data[::3] = 0.0
    assert Q.nnz == len(Q.data) and (Q.data == 0.0).sum() > 10
    some = _with_q(base, Q)
    want, _, _ = _run(monkeypatch, some, "0")
    got, launches, bit = _run(monkeypatch, some, "1")
    assert bit == 1 and launches == [1] * 4
    _assert_same(got, want, "stored zeros among nonzeros")


def test_objective_matrix_set_after_lp_steps(gpu_required, monkeypatch, row_order_mode):
    """pdhg_set_objective_matrix on a handle that has stepped as an LP (in the LDS kernel): the class is decided again."""
    p = SHAPES["nonsymmetric_90x120"]()
    want, launches_off, bit_off = _run(monkeypatch, p, "0", lp_steps_first=10)
    got, launches_on, bit_on = _run(monkeypatch, p, "1", lp_steps_first=10)
    assert (bit_off, launches_off) == (0, [0] * 4) and (bit_on, launches_on) == (1, [1] * 4)
    _assert_same(got, want)


# ---- 6. launches that end inside a take_step, and a pending average
def test_a_launch_that_ends_inside_a_take_step(gpu_required, monkeypatch, row_order_mode):
    """A table of powers of 3 entries and a first step far too long: launches end after rejections, the take_step they
    end in is finished launch by launch with its step size on entry as the average's weight."""
    p = SHAPES["btb_300x280"]()
    kw = dict(batches=(20, 20), constant=0, step_scale=300.0)
    want, _, _ = _run(monkeypatch, p, "0", **kw)
    got, launches, bit = _run(monkeypatch, p, "1", table=3, **kw)
    assert bit == 1 and min(launches) >= 2, launches
    assert int(got["total_number_iterations"]) > 40                  # there were rejected trials
    _assert_same(got, want)


def test_a_batch_entered_with_a_pending_average_update(gpu_required, monkeypatch, row_order_mode):
    p = SHAPES["nonsymmetric_90x120"]()
    kw = dict(batches=(7, 20), constant=5, single_first=True)
    want, _, _ = _run(monkeypatch, p, "0", **kw)
    got, launches, bit = _run(monkeypatch, p, "1", **kw)
    assert bit == 1 and launches == [1, 1, 1]
    _assert_same(got, want)


# ---- 7. the fleet
def _fleet_problems():
    return [random_lp(40, 50, 3, seed=41),                        # 0 LP, 256 threads
            random_lp(400, 300, 4, seed=42),                      # 1 LP, 1024 threads
            _diag_qp(60, 50, 31),                                 # 2 QP, 256 threads
            _random_qp(300, 280, 4),                              # 3 QP, 1024 threads
            _long_row_qp(257, False),                             # 4 QP with a 257-entry row of Q: not of the class
            H.rows_with_lens([257] + [5] * 30, 300, seed=44),     # 5 LP with a 257-entry row: not of the class
            _nonsym_qp(90, 120, 9),                               # 6 QP, 256 threads, not symmetric
            _nonsym_qp(100, 400, 10)]                             # 7 QP, 1024 threads, not symmetric
FLEET_QPS, FLEET_CLASS_LP, FLEET_CLASS_QP = (2, 3, 4, 6, 7), (0, 1), (2, 3, 6, 7)
FLEET_CALLS = ([64, 2, 64, 64, 2, 64, 1, 0], [2, 64, 0, 1, 64, 2, 64, 64], [0, 0, 64, 0, 0, 0, 2, 0])


class _Scalars:
    def __init__(self, problems):
        sw = [H.initial_step_and_weight(p) for p in problems]
        self.ss = np.array([s for s, _ in sw])
        self.pw = np.array([w for _, w in sw])
        self.it = np.zeros(len(problems), dtype=np.int64)
        self.kkt = np.zeros(len(problems))


def _expected_fleet_counts(n_steps, switch):
    klass = FLEET_CLASS_LP + (FLEET_CLASS_QP if switch == "1" else ())
    carried = [k for k, n in enumerate(n_steps) if n >= 2 and k in klass]
    single = [k for k, n in enumerate(n_steps) if n >= 1 and k not in carried]
    few = {0, 2, 6}
    parts = {(k in FLEET_QPS, k in few) for k in carried}
    return len(carried), len(single), len(parts)


@pytest.mark.parametrize("policy", ["adaptive", "constant"])
@pytest.mark.parametrize("switch", ["1", "0"])
def test_fleet_carries_small_qps_beside_the_lps(gpu_required, monkeypatch, row_order_mode, policy, switch):
    problems = _fleet_problems()
    K = len(problems)
    # the solo twins: every member stepped by its own calls, per launch for the QPs
    monkeypatch.setenv("PDHG_SMALL_QP", "0")
    solos = [HipPdhgEngine.from_problem(p, device_id=0) for p in problems]
    for e in solos:
        e.layout_info()                  # (the class is decided here, under the twins' setting)
    monkeypatch.setenv("PDHG_SMALL_QP", switch)
    fleet = HipPdhgFleet.from_problems(problems, device_id=0)
    try:
        for k, mb in enumerate(fleet.members):
            assert mb.layout_info()["small_lp"] == int(k in FLEET_CLASS_LP or (switch == "1" and k in FLEET_CLASS_QP)), k
        fs, ss = _Scalars(problems), _Scalars(problems)
        launches = 0
        for c, n_steps in enumerate(FLEET_CALLS):
            if policy == "adaptive":
                fs.ss, fs.it, fs.kkt, err, done = fleet.take_steps_adaptive(n_steps, RED, GROW, fs.ss, fs.pw, fs.it, fs.kkt)
            else:
                fs.kkt, done = fleet.take_steps_constant(n_steps, fs.ss, fs.pw, fs.kkt)
                err = np.zeros(K, dtype=bool)
            carried, single, parts = _expected_fleet_counts(n_steps, switch)
            launches += parts
            info = fleet.info()
            assert (info["carried"], info["single"], info["shared_launches"]) == (carried, single, launches), (c, info)
            for k, n in enumerate(n_steps):
                if n == 0:
                    assert done[k] == 0
                    continue
                if policy == "adaptive":
                    ss.ss[k], ss.it[k], ss.kkt[k], e, d = solos[k].take_steps_adaptive(n, RED, GROW, float(ss.ss[k]), float(ss.pw[k]),
                                                                                       int(ss.it[k]), float(ss.kkt[k]))
                else:
                    ss.kkt[k], d = solos[k].take_steps_constant(n, float(ss.ss[k]), float(ss.pw[k]), float(ss.kkt[k]))
                    e = False
                label = f"call {c}, member {k}"
                assert (bool(err[k]), int(done[k])) == (bool(e), int(d)), label
                assert _bits(fs.ss[k]) == _bits(ss.ss[k]) and fs.it[k] == ss.it[k] and _bits(fs.kkt[k]) == _bits(ss.kkt[k]), label
        for k in range(K):
            _assert_same(_state(fleet.members[k]), _state(solos[k]), f"member {k}")
    finally:
        fleet.close()
        for e in solos:
            e.close()


def test_fleet_malitsky_pock_still_refuses_a_qp_before_any_launch(gpu_required, monkeypatch, row_order_mode):
    monkeypatch.setenv("PDHG_SMALL_QP", "1")
    problems = [random_lp(40, 50, 3, seed=41), _diag_qp(60, 50, 31)]
    fleet = HipPdhgFleet.from_problems(problems, device_id=0)
    try:
        sc = _Scalars(problems)
        before = [_state(mb) for mb in fleet.members]
        with pytest.raises(Exception, match="only supported for linear programming"):
            fleet.take_steps_malitsky_pock([8, 8], 0.7, 0.99, 1.0, sc.ss, np.ones(2), sc.pw, sc.it, sc.kkt)
        assert fleet.info()["shared_launches"] == 0
        assert [mb.steps_info()[0] for mb in fleet.members] == [0, 0]
        for k, mb in enumerate(fleet.members):
            _assert_same(_state(mb), before[k], f"member {k}")
    finally:
        fleet.close()


# ---- 8. whole solves
def _stats_key(s):
    import dataclasses
    d = dataclasses.asdict(s)
    d.pop("cumulative_time_sec")
    d["method_specific_stats"] = {k: v for k, v in d["method_specific_stats"].items() if "time" not in k}
    return repr(d)


def _solve_qp_default_params(iteration_limit):
    """scripts/solve_qp.py's defaults (tools/fleet_bench.py states them the same way): Ruiz-10 + Pock-Chambolle, adaptive
    steps, adaptive-normalised restarts, an evaluation every 40 iterations, tolerance 1e-6."""
    from firstorderlp_jl_amd.primal_dual_hybrid_gradient import AdaptiveStepsizeParams, PdhgParameters
    from firstorderlp_jl_amd.saddle_point import RestartScheme, RestartToCurrentMetric, construct_restart_parameters
    from firstorderlp_jl_amd.termination import construct_termination_criteria
    tc = construct_termination_criteria(eps_optimal_absolute=1e-6, eps_optimal_relative=1e-6, iteration_limit=iteration_limit)
    rp = construct_restart_parameters(RestartScheme.ADAPTIVE_NORMALIZED, RestartToCurrentMetric.GAP_OVER_DISTANCE_SQUARED,
                                      1000, 0.5, 0.1, 0.9, 0.5, False)
    return PdhgParameters(10, False, 1.0, 1.0, True, 0, False, 40, tc, rp, AdaptiveStepsizeParams(RED, GROW))


def test_optimize_many_with_small_qps_is_optimize_per_problem(gpu_required, monkeypatch, row_order_mode):
    """Rescaling, evaluations and restarts between the batches: the rescaled copies of Q go through the kernel."""
    params = _solve_qp_default_params(2000)
    problems = [H.example_qp(), H.example_qp2(), _random_qp(60, 50, 21), _random_qp(300, 280, 4), random_lp(40, 50, 3, seed=41),
                random_lp(400, 300, 4, seed=42)]
    monkeypatch.setenv("PDHG_SMALL_QP", "0")
    want = [optimize(params, p) for p in problems]
    monkeypatch.setenv("PDHG_SMALL_QP", "1")
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
    got = optimize_many(params, problems, fleet_factory=factory)
    assert len(got) == 6
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.termination_reason == w.termination_reason, k
        assert g.iteration_count == w.iteration_count, k
        assert np.array_equal(_bits(g.primal_solution), _bits(w.primal_solution)), k
        assert np.array_equal(_bits(g.dual_solution), _bits(w.dual_solution)), k
        assert [_stats_key(s) for s in g.iteration_stats] == [_stats_key(s) for s in w.iteration_stats], k
    assert infos and max(i["carried"] for i in infos) == 6, infos[:3]      # the four QPs rode in the shared launches
