"""Batched solves on the device (pdhg_create_batch / pdhg_batch_*): every member's trial, masking, free-running
adaptive steps and whole solves against solo handles on the same LP; the batch's lifetime."""
import numpy as np
import pytest
import scipy.sparse as sp

import folp_loader

folp = folp_loader.load()
from firstorderlp_jl_amd import HipPdhgBatch, HipPdhgEngine, optimize_batch  # noqa: E402
from firstorderlp_jl_amd.generators import (l1_svm_regularization_path,  # noqa: E402
                                            personalized_pagerank_lps, random_lp, synthetic_rcv1_like,
                                            preprocess_training_data)
from firstorderlp_jl_amd.primal_dual_hybrid_gradient import (AdaptiveStepsizeParams, PdhgParameters,  # noqa: E402
                                                             optimize)
from firstorderlp_jl_amd.quadratic_programming import linear_programming_problem  # noqa: E402
from firstorderlp_jl_amd.saddle_point import (RestartScheme, RestartToCurrentMetric,  # noqa: E402
                                              construct_restart_parameters)
from firstorderlp_jl_amd.termination import construct_termination_criteria  # noqa: E402

pytestmark = pytest.mark.gpu


def _variants(p, K, seed):
    """K LPs on p's matrix with their own c, b and bounds."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(K):
        c = p.objective_vector * (1.0 + 0.5 * rng.random(len(p.objective_vector))) if k else p.objective_vector.copy()
        b = p.right_hand_side * (1.0 + 0.3 * rng.random(len(p.right_hand_side))) if k else p.right_hand_side.copy()
        lb = p.variable_lower_bound.copy()
        ub = p.variable_upper_bound + k
        out.append(linear_programming_problem(lb, ub, c, 0.0, p.constraint_matrix, b, p.num_equalities))
    return out


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


_EPS = np.finfo(np.float64).eps


def _trial_case(problems, mask=None, seed=5):
    """A batch and one solo handle per member, all from the same random warm start.  Round 1: one trial of every active
    member from that start, then an accept on both sides; round 2 (returned in `raw`) then starts from the accepted
    nonzero iterate, with the deferred average update riding on the batched kernels."""
    K = len(problems)
    batch = HipPdhgBatch.from_problems(problems, device_id=0)
    solos = [HipPdhgEngine.from_problem(p, device_id=0) for p in problems]
    try:
        m, n = problems[0].constraint_matrix.shape
        rng = np.random.default_rng(seed)
        states = [(rng.random(n), rng.standard_normal(m)) for _ in range(K)]
        for e, s in zip(batch.members, states):
            e.set_current(*s)
        for e, s in zip(solos, states):
            e.set_current(*s)
        ss = 0.5 / (1.0 + np.arange(K))
        pw = 1.0 + np.arange(K) * 0.25
        act = np.ones(K, dtype=np.int32) if mask is None else np.asarray(mask, dtype=np.int32)
        before = {k: batch.members[k].get_trial() + batch.members[k].get_current() + batch.members[k].get_average()
                  for k in range(K) if not act[k]}
        raw1 = batch.trial_step(ss, pw, 1.0, act)
        first = {}
        for k in np.flatnonzero(act):
            want = solos[k].trial_step(ss[k], pw[k], 1.0)
            first[k] = (raw1[k], want, batch.members[k].get_trial(), solos[k].get_trial(), states[k][0])
        batch.accept(act, ss)
        for k in np.flatnonzero(act):
            solos[k].accept(ss[k])
        prev = {k: first[k][3][0] for k in first}          # x' of round 1 = x at the start of round 2
        raw = batch.trial_step(ss, pw, 1.0, act)
        return dict(batch=batch, solos=solos, raw=raw, first=first, prev=prev, before=before, ss=ss, pw=pw, act=act)
    except Exception:
        batch.close()
        for e in solos:
            e.close()
        raise


def _close(c):
    c["batch"].close()
    for e in c["solos"]:
        e.close()


def _compare_trial(A, got_raw, want_raw, got, want, x_prev, sigma, label):
    """One member's trial against the solo handle's: x' bitwise; y' bitwise on rows the single path sums sequentially,
    within 2e-13 * sigma * sum |a xbar| elsewhere; A'y' bitwise on such columns whose rows are all such rows, elsewhere
    within what the y' differences and 2e-13 * sum |a y'| explain; the sums bitwise when every row and column is such
    a row, else to 1e-9."""
    from tests.helpers import bitexact_row_limit
    lim = bitexact_row_limit()
    Ar = sp.csr_matrix(A)
    Aa = abs(Ar)
    row_nnz = np.diff(Ar.indptr)
    col_nnz = np.diff(sp.csc_matrix(A).indptr)
    gx, gy, ga = got
    wx, wy, wa = want
    assert np.array_equal(_bits(gx), _bits(wx)), label + ": x'"
    short_r = row_nnz <= lim
    assert np.array_equal(_bits(gy[short_r]), _bits(wy[short_r])), label + ": y' on short rows"
    xbar = 2.0 * wx - x_prev
    tol_y = sigma * 2e-13 * (Aa @ np.abs(xbar)) + 4 * _EPS * np.abs(wy)
    assert np.all(np.abs(gy - wy) <= tol_y), label + ": y' on long rows beyond the relaxed bar"
    clean = (col_nnz <= lim) & (Aa.T @ (~short_r).astype(float) == 0)
    assert np.array_equal(_bits(ga[clean]), _bits(wa[clean])), label + ": A'y' on short columns"
    tol_a = Aa.T @ np.abs(gy - wy) + 2e-13 * (Aa.T @ np.abs(wy)) + 4 * _EPS * np.abs(wa)
    assert np.all(np.abs(ga - wa) <= tol_a), label + ": A'y' beyond the relaxed bar"
    if short_r.all() and (col_nnz <= lim).all():
        assert np.array_equal(_bits(got_raw), _bits(want_raw)), label + ": sums"
    else:
        assert np.allclose(got_raw, want_raw, rtol=1e-9, atol=0), label + ": sums"
    return int((~short_r).sum()), int((col_nnz > lim).sum())


def _check_case(c, A, k):
    raw1, want1, got1, sol1, x0 = c["first"][k]
    sigma = c["pw"][k] * c["ss"][k]
    counts = _compare_trial(A, raw1, want1, got1, sol1, x0, sigma, f"member {k}, trial 1")
    same = all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(got1, sol1))
    want = c["solos"][k].trial_step(c["ss"][k], c["pw"][k], 1.0)
    got2, sol2 = c["batch"].members[k].get_trial(), c["solos"][k].get_trial()
    avg_b, avg_s = c["batch"].members[k].get_average(), c["solos"][k].get_average()
    if same:
        # the same state after trial 1: trial 2 (with the pending average update on the batched kernels) compares like
        # trial 1, and the averages bitwise
        _compare_trial(A, c["raw"][k], want, got2, sol2, c["prev"][k], sigma, f"member {k}, trial 2")
        for a, b in zip(avg_b, avg_s):
            assert np.array_equal(_bits(a), _bits(b)), f"member {k}: averages"
    else:
        # trial 1's long rows differed within the bar, so the two sides start trial 2 from states that differ by as much
        for a, b in zip(got2 + avg_b, sol2 + avg_s):
            assert np.allclose(a, b, rtol=1e-9, atol=1e-12 * (1.0 + np.abs(b).max())), f"member {k}: trial 2"
        assert np.allclose(c["raw"][k], want, rtol=1e-6, atol=0), f"member {k}: trial 2 sums"
    return counts


@pytest.mark.parametrize("K", [1, 3, 8, 32])
def test_batched_trial_is_the_solo_trial_bitwise(gpu_required, K):
    p = random_lp(3000, 2500, 8, seed=11)
    c = _trial_case(_variants(p, K, 1))
    try:
        for k in range(K):
            _check_case(c, p.constraint_matrix, k)
    finally:
        _close(c)


def _svm_members():
    X, y = synthetic_rcv1_like(600, 900, 20, seed=3)
    return l1_svm_regularization_path(preprocess_training_data(X), y, [0.1, 1.0, 4.0])


def _pagerank_20000():
    n = 20000
    rng = np.random.default_rng(2)
    return personalized_pagerank_lps(n, [np.full(n, 1.0 / n)] + [rng.dirichlet(np.ones(n)) for _ in range(2)], seed=3)


@pytest.mark.parametrize("case", ["pagerank", "l1_svm"])
def test_batched_trial_long_rows_and_columns(gpu_required, row_order_mode, case):
    """Matrices with rows and columns beyond the sequential limit (both orders): the chunked long-row kernels of both
    products against the single path, from a nonzero iterate."""
    probs = _pagerank_20000() if case == "pagerank" else _svm_members()
    A = probs[0].constraint_matrix
    c = _trial_case(probs)
    try:
        counts = [_check_case(c, A, k) for k in range(len(probs))]
    finally:
        _close(c)
    long_rows, long_cols = counts[0]
    # the chunked paths ran: A xbar's (PageRank's row 0 and hub rows, in both orders) and, in the shipped relaxed order,
    # A'y''s (PageRank hub columns, the SVM's frequent feature columns)
    if case == "pagerank":
        assert long_rows > 0, long_rows
    if row_order_mode == "relaxed":
        assert long_cols > 0, long_cols


def test_masked_members_are_untouched(gpu_required):
    p = random_lp(2000, 1800, 6, seed=4)
    probs = _variants(p, 6, 9)
    mask = np.array([1, 0, 1, 1, 0, 1], dtype=np.int32)
    c = _trial_case(probs, mask)
    try:
        for k in range(6):
            if mask[k]:
                _check_case(c, p.constraint_matrix, k)
            else:
                after = c["batch"].members[k].get_trial() + c["batch"].members[k].get_current() + \
                    c["batch"].members[k].get_average()
                for a, b in zip(after, c["before"][k]):
                    assert np.array_equal(_bits(a), _bits(b))
                assert np.isnan(c["raw"][k]).all()
        # the active members' bits do not depend on the mask (a trial of every member from the same state)
        raw_all = c["batch"].trial_step(c["ss"], c["pw"], 1.0, np.ones(6, dtype=np.int32))
        for k in np.flatnonzero(mask):
            assert np.array_equal(_bits(raw_all[k]), _bits(c["raw"][k]))
    finally:
        _close(c)


def test_free_running_adaptive_steps_match_solo_handles(gpu_required):
    """Five members with their own c / b / bounds (one warm-started) take 300 adaptive steps in lockstep; a sixth, with
    c = 0 and b = 0 at the origin, has zero movement on its first trial: it raises numerical_error, stops after that
    step and takes no further trials while the others go on.  Every member equals a solo handle's take_steps_adaptive."""
    p = random_lp(4000, 3500, 8, seed=21)
    probs = _variants(p, 5, 3)
    m0, n0 = p.constraint_matrix.shape
    probs.append(linear_programming_problem(p.variable_lower_bound, p.variable_upper_bound, np.zeros(n0), 0.0,
                                            p.constraint_matrix, np.zeros(m0), p.num_equalities))
    batch = HipPdhgBatch.from_problems(probs, device_id=0)
    solos = [HipPdhgEngine.from_problem(q, device_id=0) for q in probs]
    try:
        m, n = p.constraint_matrix.shape
        rng = np.random.default_rng(8)
        x0, y0 = rng.random(n), rng.standard_normal(m)
        batch.members[2].set_current(x0, y0)
        solos[2].set_current(x0, y0)
        step0 = 1.0 / batch.members[0].matrix_max_abs()
        ss = np.full(6, step0)
        pw = np.array([1.0, 0.5, 2.0, 1.5, 0.8, 1.0])
        it = np.zeros(6, dtype=np.int64)
        kkt = np.zeros(6)
        ss, it, kkt, err, done = batch.take_steps_adaptive(300, 0.3, 0.6, ss, pw, it, kkt)
        assert (done[:5] == 300).all() and not err[:5].any()
        assert done[5] == 1 and err[5] and it[5] == 1
        for k, e in enumerate(solos):
            s, i, c, er, d = e.take_steps_adaptive(300, 0.3, 0.6, step0, pw[k], 0, 0.0)
            assert (s, i, c, er, d) == (ss[k], it[k], kkt[k], bool(err[k]), done[k])
            for a, b in zip(batch.members[k].get_current() + batch.members[k].get_average(),
                            e.get_current() + e.get_average()):
                assert np.array_equal(_bits(a), _bits(b))
            assert batch.members[k].average_info() == e.average_info()
    finally:
        batch.close()
        for e in solos:
            e.close()


def _params(tol=1e-6, limit=20000):
    tc = construct_termination_criteria(eps_optimal_absolute=tol, eps_optimal_relative=tol, iteration_limit=limit)
    rp = construct_restart_parameters(RestartScheme.ADAPTIVE_NORMALIZED, RestartToCurrentMetric.GAP_OVER_DISTANCE_SQUARED,
                                      1000, 0.5, 0.1, 0.9, 0.5, False)
    return PdhgParameters(10, False, 1.0, 1.0, True, 0, True, 64, tc, rp, AdaptiveStepsizeParams(0.3, 0.6))


def _assert_same_solve(got, want, bitwise):
    assert got.termination_reason == want.termination_reason
    if bitwise:
        assert got.iteration_count == want.iteration_count
        assert np.array_equal(_bits(got.primal_solution), _bits(want.primal_solution))
        assert np.array_equal(_bits(got.dual_solution), _bits(want.dual_solution))
    else:
        # rows or columns beyond the sequential limit: the two runs sum them in different fixed orders (each within
        # 1e-13 of the exact sum), so their trajectories part after many steps, as a solo solve's do between the two row
        # orders (the L1-SVM path here: 21 056 / 17 216 / 1 728 iterations in strict order, 18 816 / 14 336 / 2 304 in
        # relaxed); both must reach the same answer, in a comparable number of iterations
        assert want.iteration_count / 1.5 <= got.iteration_count <= 1.5 * want.iteration_count + 128
        cg = got.iteration_stats[-1].convergence_information[0]
        cw = want.iteration_stats[-1].convergence_information[0]
        scale = 1.0 + abs(cw.primal_objective)
        assert abs(cg.primal_objective - cw.primal_objective) <= 50 * 1e-6 * scale
        assert abs(cg.dual_objective - cw.dual_objective) <= 50 * 1e-6 * scale


def _pagerank_members():
    n = 5000
    rng = np.random.default_rng(6)
    return personalized_pagerank_lps(n, [np.full(n, 1.0 / n)] + [rng.dirichlet(np.ones(n)) for _ in range(3)], seed=7)


def _with_infeasible():
    p = random_lp(800, 700, 5, seed=13)
    probs = _variants(p, 3, 2)
    n = len(p.objective_vector)
    bad = linear_programming_problem(np.zeros(n), np.zeros(n), p.objective_vector, 0.0, p.constraint_matrix,
                                     np.abs(p.right_hand_side) + 1.0, p.num_equalities)
    return probs + [bad]


@pytest.mark.parametrize("case", ["pagerank", "l1_svm", "infeasible", "single"])
def test_optimize_batch_is_optimize_per_member(gpu_required, row_order_mode, case):
    """optimize_batch against optimize per member in both row orders: bitwise where every row and column is summed
    sequentially by both paths (conftest sets the order)."""
    from tests.helpers import bitexact_row_limit
    probs = {"pagerank": _pagerank_members, "l1_svm": _svm_members, "infeasible": _with_infeasible,
             "single": lambda: [random_lp(1500, 1200, 6, seed=5)]}[case]()
    params = _params(limit=5000 if case == "infeasible" else 40000)
    want = [optimize(params, p) for p in probs]
    got = optimize_batch(params, probs)
    A = sp.csr_matrix(probs[0].constraint_matrix)
    short = max(np.diff(A.indptr).max(), np.diff(sp.csc_matrix(A).indptr).max()) <= bitexact_row_limit()
    for g, w in zip(got, want):
        _assert_same_solve(g, w, bitwise=short)


def test_batch_lifetime(gpu_required):
    import torch
    p = random_lp(20000, 18000, 8, seed=2)
    probs = _variants(p, 8, 4)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(0)[0]
    batch = HipPdhgBatch.from_problems(probs, device_id=0)
    m0 = batch.members[0]
    folp._lib.lib().pdhg_destroy(m0._h)        # a member's destroy does nothing
    out = optimize_batch(_params(limit=200), probs[:1])
    assert out[0].iteration_count > 0
    raw = batch.trial_step(np.full(8, 0.1), np.ones(8))
    assert np.isfinite(raw).all()
    batch.close()
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info(0)[0]
    assert abs(free1 - free0) <= (1 << 20), (free0, free1)
