"""QP batches (pdhg_batch_set_objective_matrix; csrc/batch_kernels.hpp: the pack kernel, Q X, the QP primal kernel, Q' DX
and the five-sum final kernel) against the CPU oracle at the places where the kernels branch, and against solo QP
handles where the claim is "the same bits".

The scheme of tests/test_gpu_batch_edges.py, restated for QPs: every active member is compared with its OWN oracle state
(tests/helpers.py: assert_trial_matches_oracle(..., Q=Q), the project's existing bars) over two rounds -- a trial from a
random nonzero start, an accept on both sides, then a second trial on which the deferred average update rides.  The
objective matrices are NOT symmetric wherever convexity is not needed: the library keeps Q and Q' as two layouts, and only
then is a swap of the two visible."""
import copy
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import folp_loader

folp = folp_loader.load()
from firstorderlp_jl_amd import HipPdhgBatch, HipPdhgEngine, _lib, optimize_batch  # noqa: E402
from firstorderlp_jl_amd.generators import random_qp_family  # noqa: E402
from firstorderlp_jl_amd.primal_dual_hybrid_gradient import AdaptiveStepsizeParams, PdhgParameters, optimize  # noqa: E402
from firstorderlp_jl_amd.quadratic_programming import QuadraticProgrammingProblem, linear_programming_problem  # noqa: E402
from firstorderlp_jl_amd.saddle_point import (RestartScheme, RestartToCurrentMetric,  # noqa: E402
                                              construct_restart_parameters)
from firstorderlp_jl_amd.termination import construct_termination_criteria  # noqa: E402
from tests import helpers as H  # noqa: E402

pytestmark = pytest.mark.gpu

_CSRC = os.path.join(os.path.dirname(os.path.abspath(folp.__file__)), "csrc")


def _const(header, name):
    """An integer constant of the kernels' headers (`constexpr int NAME = 256 * 8;`)."""
    with open(os.path.join(_CSRC, header)) as f:
        expr = re.search(r"constexpr int %s = ([0-9 *]+);" % name, f.read()).group(1)
    return int(np.prod([int(t) for t in expr.split("*")]))


TPB = _const("common.hpp", "TPB")
EW_MAX_BLOCKS = _const("common.hpp", "EW_MAX_BLOCKS")
BATCH_CHUNK = _const("batch_kernels.hpp", "BATCH_CHUNK")
BATCH_MAX_GRID = _const("batch_kernels.hpp", "BATCH_MAX_GRID")
BATCH_U = _const("batch_kernels.hpp", "BATCH_U")


def _gpb(K):
    """Lane groups per workgroup: TPB >> shift, Kp = 1 << shift the member count rounded up to a power of two."""
    return TPB // (1 << max(0, int(K - 1).bit_length()))


def _same(a, b):
    """Bit for bit, NaNs in the same places (0 / 0 of an average without weight carries either sign)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(H._bits64(a[~nan]), H._bits64(b[~nan]))


def _csc(Q):
    Q = sp.csc_matrix(Q)
    Q.sum_duplicates()
    Q.sort_indices()
    return Q


def _qp_members(p, Q, K, seed):
    """K QPs on p's constraint matrix and on Q (the same objects: no copies of large ones) with their own c, b and
    bounds; fixed variables stay fixed, at another value."""
    rng = np.random.default_rng(seed)
    n, m = len(p.objective_vector), len(p.right_hand_side)
    out = []
    for k in range(K):
        c = p.objective_vector * (1.0 + 0.5 * rng.random(n)) if k else p.objective_vector.copy()
        b = p.right_hand_side * (1.0 + 0.3 * rng.random(m)) if k else p.right_hand_side.copy()
        fixed = p.variable_lower_bound == p.variable_upper_bound
        lb = p.variable_lower_bound - np.where(fixed, 0.125 * k, 0.0)
        ub = np.where(fixed, lb, p.variable_upper_bound + k)
        q = QuadraticProgrammingProblem(lb, ub, sp.csc_matrix((n, n)), c, 0.0, sp.csc_matrix((m, n)), b, p.num_equalities)
        q.constraint_matrix, q.objective_matrix = p.constraint_matrix, Q
        out.append(q)
    return out


def _nnz(M):
    return np.diff(sp.csr_matrix(M).indptr), np.diff(sp.csc_matrix(M).indptr)


def _two_rounds(problems, mask=None, seed=5, set_q_late=False):
    """The device does both rounds first (its vectors are taken to the host after each trial); then every active member
    is verified against an oracle state of its own, one at a time.  set_q_late: the batch is created as an LP batch, takes
    a trial and an accept as one, and only then gets its objective matrix (the iterates are set again afterwards)."""
    K = len(problems)
    A, Q = problems[0].constraint_matrix, problems[0].objective_matrix
    m, n = A.shape
    col_nnz = np.diff(sp.csc_matrix(A).indptr)
    absA = abs(sp.csr_matrix(A))
    rng = np.random.default_rng(seed)
    states = [(rng.random(n), rng.standard_normal(m)) for _ in range(K)]
    ss = 0.5 / (1.0 + np.arange(K))
    pw = 1.0 + np.arange(K) * 0.25
    act = np.ones(K, dtype=np.int32) if mask is None else np.asarray(mask, dtype=np.int32)
    if set_q_late:
        lps = []
        for p in problems:
            q = copy.copy(p)
            q.objective_matrix = sp.csc_matrix((n, n))
            lps.append(q)
        batch = HipPdhgBatch.from_problems(lps, device_id=0)
    else:
        batch = HipPdhgBatch.from_problems(problems, device_id=0)
    try:
        if set_q_late:
            raw = batch.trial_step(ss, pw, 1.0, act)
            assert (raw[act != 0, 4] == 0.0).all()
            batch.accept(act, ss)
            batch.set_objective_matrix(Q)
            for e in batch.members:
                e.reset_average()
        for e, s in zip(batch.members, states):
            e.set_current(*s)
        aty0 = [e.get_dual_product() for e in batch.members]

        def snapshot(k):
            e = batch.members[k]
            return e.get_trial() + e.get_current() + e.get_average()

        before = {k: snapshot(k) for k in range(K) if not act[k]}
        raw1 = batch.trial_step(ss, pw, 1.0, act)
        trial1 = {k: batch.members[k].get_trial() for k in np.flatnonzero(act)}
        batch.accept(act, ss)
        raw2 = batch.trial_step(ss, pw, 1.0, act)
        trial2 = {k: batch.members[k].get_trial() for k in np.flatnonzero(act)}
        avg = {k: batch.members[k].get_average() for k in np.flatnonzero(act)}
        after = {k: snapshot(k) for k in before}
        # an all-zero mask returns without touching anything
        everything = [snapshot(k) for k in range(K)]
        raw0 = batch.trial_step(ss, pw, 1.0, np.zeros(K, dtype=np.int32))
        assert np.isnan(raw0).all()
        for k in range(K):
            for a, b in zip(snapshot(k), everything[k]):
                assert _same(a, b), f"member {k}: an empty trial wrote something"
    finally:
        batch.close()
    for k in range(K):
        if not act[k]:
            for a, b in zip(after[k], before[k]):
                assert _same(a, b), f"inactive member {k} was written"
            assert np.isnan(raw1[k]).all() and np.isnan(raw2[k]).all(), f"inactive member {k}: raw"
            continue
        o = H.oracle_from_problem(problems[k])
        try:
            o.x, o.y = states[k]
            o.recompute_dual_product()
            # set_current's A'y is the single path's product (not a batched kernel): held to its own bar, then taken over
            H.assert_rows_match_oracle(aty0[k], o.aty, col_nnz, absA.T @ np.abs(states[k][1]), f"member {k}: A'y of the start")
            o.aty = aty0[k]
            H.assert_trial_matches_oracle(raw1[k], trial1[k], o, ss[k], pw[k], A, f"member {k}, trial 1", Q=Q)
            assert raw1[k][4] != 0.0, f"member {k}: the QP term is missing"
            o.step_size = ss[k]
            o.accept(*trial1[k])
            H.assert_trial_matches_oracle(raw2[k], trial2[k], o, ss[k], pw[k], A, f"member {k}, trial 2", Q=Q)
            for a, b, name in zip(avg[k], o.compute_average(), ("x", "y")):
                assert _same(a, b), f"member {k}: average of {name}"
        finally:
            o.close()


def _ladder_q(lens, seed):
    """A non-symmetric n x n matrix, n = len(lens) + max(lens): block_diag(L, L') of another ladder, so its rows AND its
    columns hold every length of `lens` (the same shape as ladder_lp's constraint matrix)."""
    Q = _csc(H.ladder_lp(lens, seed=seed).constraint_matrix)
    assert Q.shape[0] == Q.shape[1] and (Q != Q.T).nnz > 0
    return Q


def _assert_both_sides_of_the_threshold(M):
    """Rows and columns of M at long_thr and at long_thr + 1 entries; no entry at all, the shortest and the longest masked
    tail alone and after a full step, no tail after one and two full steps; whole chunks with and without one entry more,
    below the threshold and beyond it."""
    thr = H.bitexact_row_limit()
    for nnz in _nnz(M):
        have = set(nnz.tolist())
        assert {thr, thr + 1} <= have, "no rows on both sides of the long-row threshold"
        assert {0, 1, BATCH_U - 1, BATCH_U, BATCH_U + 1, 2 * BATCH_U - 1, 2 * BATCH_U, 2 * BATCH_U + 1} <= have
        assert {BATCH_CHUNK - 1, BATCH_CHUNK, BATCH_CHUNK + 1} <= have
        long_ = nnz[nnz > thr]
        assert np.any(long_ % BATCH_CHUNK == 0) and np.any(long_ % BATCH_CHUNK == 1), "no long row of 128 c and 128 c + 1 entries"


@pytest.mark.parametrize("K", [1, 2, 5, 32])
def test_row_length_ladder(gpu_required, row_order_mode, K):
    """Kp = 1, 2, 8, 32 over rows and columns of every length of the ladder, in A and in Q, in both row orders.  At
    K = 32 (gpb = 8) this is also the second trip through the chunk sums of batch_long_final_kernel for Q and Q': a long
    row of more than gpb * BATCH_CHUNK = 1024 entries (1025 and more in relaxed order, 2049 and 2176 in strict order)."""
    p = H.ladder_lp(H.LADDER_LENS, seed=3)
    Q = _ladder_q(H.LADDER_LENS, seed=21)
    assert Q.shape == (p.constraint_matrix.shape[1],) * 2
    _assert_both_sides_of_the_threshold(p.constraint_matrix)
    _assert_both_sides_of_the_threshold(Q)
    if K == 32:
        thr, gpb = H.bitexact_row_limit(), _gpb(K)
        assert gpb == 8
        for nnz in _nnz(Q):
            chunks = -(-nnz[nnz > thr] // BATCH_CHUNK)
            assert np.any(chunks > gpb), (gpb, chunks.max())
    _two_rounds(_qp_members(p, Q, K, 1))


@pytest.mark.parametrize("mask", [[0, 0, 0, 0, 0, 1], [1, 0, 1, 0, 1, 0]], ids=["last", "alternating"])
def test_masks_with_long_rows(gpu_required, row_order_mode, mask):
    """Inactive members keep the bits of their trial, current and average vectors and their raw rows stay NaN; active
    members match the oracle on short and long rows of A and Q; an all-zero mask touches nothing (_two_rounds).  (A
    member's qx has no getter: a write to an inactive member's would go unseen here; it is recomputed by every trial.)"""
    p = H.ladder_lp(H.LADDER_LENS, seed=6)
    Q = _ladder_q(H.LADDER_LENS, seed=22)
    thr = H.bitexact_row_limit()
    assert all(np.any(nnz > thr) for nnz in _nnz(Q))
    _two_rounds(_qp_members(p, Q, 6, 3), mask=mask)


def _small_q(n, seed, kind):
    rng = np.random.default_rng(seed)
    if kind == "diagonal":
        return _csc(sp.diags(0.25 + rng.random(n)))
    Q = sp.random(n, n, density=0.2, random_state=seed, format="lil", data_rvs=rng.standard_normal)
    if kind == "empty_row_and_column":
        Q[3, :] = 0.0
        Q[:, 5] = 0.0
    Q = _csc(sp.csc_matrix(Q))
    Q.eliminate_zeros()
    return Q


@pytest.mark.short_rows
@pytest.mark.parametrize("case", ["no_constraints", "empty_row_and_column", "diagonal", "q_set_after_lp_steps"])
def test_degenerate_shapes(gpu_required, row_order_mode, case):
    """m = 0 (the products of A are skipped, the Q products are not); a Q with an empty row and an empty column; a
    diagonal Q; an objective matrix that arrives after the batch has stepped as an LP batch."""
    n = 37
    if case == "no_constraints":
        rng = np.random.default_rng(31)
        p = linear_programming_problem(-rng.random(n), 1.0 + rng.random(n), rng.standard_normal(n), 0.0, sp.csc_matrix((0, n)),
                                       np.zeros(0), 0)
    else:
        p = H.rows_with_lens([0, 1, 7, 8, 9, 15, 16, 17, 3, 5], n, seed=32)
    kind = case if case in ("empty_row_and_column", "diagonal") else "general"
    Q = _small_q(n, 33, kind)
    row_nnz, col_nnz = _nnz(Q)
    if case == "empty_row_and_column":
        assert row_nnz[3] == 0 and col_nnz[5] == 0 and row_nnz.max() > 1 and (Q != Q.T).nnz > 0
    if case == "diagonal":
        assert (row_nnz == 1).all() and (Q - sp.diags(Q.diagonal())).nnz == 0
    _two_rounds(_qp_members(p, Q, 3, 4), set_q_late=(case == "q_set_after_lp_steps"))


@pytest.mark.short_rows
def test_all_zero_objective_matrix_keeps_an_lp_batch(gpu_required, row_order_mode):
    """Stored values that are all 0.0: the batch stays an LP batch -- out[4] == 0.0 and every bit of two rounds equal to a
    batch that never had a Q -- also when the zeros replace a real Q."""
    n = 37
    p = H.rows_with_lens([0, 1, 7, 8, 9, 15, 16, 17, 3, 5], n, seed=34)
    Q = _small_q(n, 35, "general")
    zeros = sp.csc_matrix((np.zeros(Q.nnz), Q.indices, Q.indptr), shape=Q.shape)
    probs = _qp_members(p, sp.csc_matrix((n, n)), 3, 5)
    rng = np.random.default_rng(6)
    states = [(rng.random(n), rng.standard_normal(len(p.right_hand_side))) for _ in range(3)]
    ss, pw = np.array([0.5, 0.25, 0.125]), np.array([1.0, 1.5, 2.0])

    def run(prepare):
        batch = HipPdhgBatch.from_problems(probs, device_id=0)
        try:
            prepare(batch)
            for e, s in zip(batch.members, states):
                e.set_current(*s)
            raw1 = batch.trial_step(ss, pw)
            out = [raw1] + [v for e in batch.members for v in e.get_trial()]
            batch.accept(np.ones(3, dtype=np.int32), ss)
            raw2 = batch.trial_step(ss, pw)
            out += [raw2] + [v for e in batch.members for v in e.get_trial() + e.get_average()]
            assert (raw1[:, 4] == 0.0).all() and (raw2[:, 4] == 0.0).all()
            return out
        finally:
            batch.close()

    def call(batch, M):
        # (HipPdhgBatch.set_objective_matrix passes any matrix with stored entries on to the library)
        batch.set_objective_matrix(M)

    want = run(lambda batch: None)
    for label, prepare in (("zeros", lambda b: call(b, zeros)), ("Q, then zeros", lambda b: (call(b, Q), call(b, zeros)))):
        got = run(prepare)
        for a, b in zip(got, want):
            assert _same(a, b), label


@pytest.mark.short_rows
def test_members_borrow_q(gpu_required, row_order_mode):
    """A member's own pdhg_trial_step gives the batched trial's bits from the same state (it multiplies by the batch's Q and
    Q' through its borrowed copies; a swap of the two would show: Q is not symmetric).  eval_point and a trust-region
    bound on a member equal a solo QP handle's; so do both after pdhg_rescale on the batch, which must reach Q."""
    n = 41
    p = H.rows_with_lens([0, 1, 7, 8, 9, 15, 16, 17, 3, 5, 12], n, seed=36)
    m = len(p.right_hand_side)
    Q = _small_q(n, 37, "general")
    assert (Q != Q.T).nnz > 0
    probs = _qp_members(p, Q, 3, 6)
    rng = np.random.default_rng(7)
    states = [(rng.random(n), rng.standard_normal(m)) for _ in range(3)]
    ss, pw = np.array([0.5, 0.25, 0.125]), np.array([1.0, 1.5, 2.0])

    def original(eng, q):
        eng.set_original_problem(np.ones(m), np.ones(n), q.objective_vector, q.right_hand_side, q.variable_lower_bound,
                                 q.variable_upper_bound)

    for rescale in (False, True):
        batch = HipPdhgBatch.from_problems(probs, device_id=0)
        solos = [HipPdhgEngine.from_problem(q, device_id=0) for q in probs]
        try:
            if rescale:
                E, D = batch.rescale(4, True, 1.0)
                for s in solos:
                    Es, Ds = s.rescale(4, True, 1.0)
                    assert _same(E, Es) and _same(D, Ds), "the batch's rescaling is not the solo QP handle's"
            for e, s, st in zip(batch.members, solos, states):
                e.set_current(*st)
                s.set_current(*st)
            raw = batch.trial_step(ss, pw)
            assert (raw[:, 4] != 0.0).all()
            for k, (e, s, q) in enumerate(zip(batch.members, solos, probs)):
                label = f"member {k}, rescale={rescale}"
                trial = e.get_trial()
                own = e.trial_step(ss[k], pw[k], 1.0)
                assert _same(own, raw[k]), label + ": the member's own trial's sums"
                for a, b in zip(e.get_trial(), trial):
                    assert _same(a, b), label + ": the member's own trial's vectors"
                solo = s.trial_step(ss[k], pw[k], 1.0)
                assert _same(solo, raw[k]), label + ": the solo QP handle's sums"
                for a, b in zip(s.get_trial(), trial):
                    assert _same(a, b), label + ": the solo QP handle's trial vectors"
                if not rescale:
                    original(e, q)
                    original(s, q)
                    assert _same(e.eval_point(0), s.eval_point(0)), label + ": eval_point"
                    assert _same(e.trust_region_bound(0, 1.7, 0.6, 0.5, 0, False), s.trust_region_bound(0, 1.7, 0.6, 0.5, 0, False)), \
                        label + ": trust-region bound"
        finally:
            batch.close()
            for s in solos:
                s.close()


def _rows_of_q(n, per_row, seed):
    """An n x n matrix whose every row has exactly per_row entries (consecutive columns from a random start, wrapped)."""
    rng = np.random.default_rng(seed)
    start = rng.integers(0, n, n)
    ci = (start[:, None] + np.arange(per_row)[None, :]) % n
    return _csc(sp.csr_matrix((rng.standard_normal(n * per_row), ci.ravel(), np.arange(n + 1) * per_row), shape=(n, n)))


def _sparse_lp(m, n, per_row, seed):
    rng = np.random.default_rng(seed)
    ci = np.sort(rng.choice(n, size=(m, per_row), replace=True), axis=1)
    A = _csc(sp.csr_matrix((rng.standard_normal(m * per_row), ci.ravel(), np.arange(m + 1) * per_row), shape=(m, n)))
    lb = np.where(rng.random(n) < 0.25, -np.inf, 0.0)
    ub = np.where(rng.random(n) < 0.25, np.inf, 2.0)
    return linear_programming_problem(lb, ub, rng.standard_normal(n), 0.0, A, rng.standard_normal(m), m // 3)


@pytest.mark.short_rows
def test_q_products_grid_stride(gpu_required, row_order_mode):
    """Both Q products at K = 32 deal BATCH_MAX_GRID * gpb = 32 768 rows per trip: n = 33 000 with Q rows of 3 entries over
    a small constraint matrix."""
    K, n = 32, 33000
    p = _sparse_lp(50, n, 6, seed=41)
    Q = _rows_of_q(n, 3, seed=42)
    row_nnz, col_nnz = _nnz(Q)
    assert n > BATCH_MAX_GRID * _gpb(K) and row_nnz.max() == 3 and col_nnz.max() < 256 and (Q != Q.T).nnz > 0
    _two_rounds(_qp_members(p, Q, K, 8))


@pytest.mark.short_rows
def test_elementwise_kernels_grid_stride(gpu_required, row_order_mode):
    """batch_pack_kernel and the QP primal kernel cover EW_MAX_BLOCKS * TPB = 524 288 columns per trip (one grid row per
    member), and at K = 2 (gpb = 128) the Q products as many rows: n = 524 588 with one entry per row of Q (a cyclic
    shift with values: not symmetric)."""
    K = 2
    n = EW_MAX_BLOCKS * TPB + 300
    p = _sparse_lp(64, n, 8, seed=43)
    rng = np.random.default_rng(44)
    Q = _csc(sp.csr_matrix((0.5 + rng.random(n), (np.arange(n) + 7) % n, np.arange(n + 1)), shape=(n, n)))
    row_nnz, col_nnz = _nnz(Q)
    assert n > EW_MAX_BLOCKS * TPB and n > BATCH_MAX_GRID * _gpb(K) and (row_nnz == 1).all() and (col_nnz == 1).all()
    _two_rounds(_qp_members(p, Q, K, 9))


@pytest.mark.short_rows
def test_free_running_matches_solo_qp_handles(gpu_required, row_order_mode):
    """40 adaptive take_steps of a K = 3 QP batch (pdhg_batch_take_steps_adaptive) against three solo QP handles
    (pdhg_take_steps_adaptive): step sizes, counts and iterates bit for bit (every row within the bit-exact limit)."""
    probs = random_qp_family(60, 80, 3, seed=11)
    assert max(max(nnz.max() for nnz in _nnz(M)) for M in (probs[0].constraint_matrix, probs[0].objective_matrix)) < 256
    ss0 = 1.0 / abs(probs[0].constraint_matrix).max()
    pw = np.array([1.0, 0.7, 1.4])
    batch = HipPdhgBatch.from_problems(probs, device_id=0)
    try:
        ss, it, kkt, err, done = batch.take_steps_adaptive(40, 0.3, 0.6, np.full(3, ss0), pw, np.zeros(3, dtype=np.int64), np.zeros(3))
        got = [e.get_current() + e.get_average() for e in batch.members]
    finally:
        batch.close()
    assert (np.asarray(it) > 40).any(), "no member rejected a trial"
    for k, q in enumerate(probs):
        s = HipPdhgEngine.from_problem(q, device_id=0)
        try:
            want = s.take_steps_adaptive(40, 0.3, 0.6, ss0, float(pw[k]), 0, 0.0)
            vecs = s.get_current() + s.get_average()
        finally:
            s.close()
        assert H._bits64(ss[k]) == H._bits64(want[0]) and it[k] == want[1] and kkt[k] == want[2], (k, ss[k], it[k], want)
        assert bool(err[k]) == want[3] and done[k] == want[4] == 40, (k, err[k], done[k], want)
        for a, b, name in zip(got[k], vecs, ("x", "y", "x average", "y average")):
            assert _same(a, b), f"member {k}: {name}"


def _solve_params():
    tc = construct_termination_criteria(eps_optimal_absolute=1e-6, eps_optimal_relative=1e-6, iteration_limit=4000)
    rp = construct_restart_parameters(RestartScheme.ADAPTIVE_NORMALIZED, RestartToCurrentMetric.GAP_OVER_DISTANCE_SQUARED,
                                      1000, 0.5, 0.1, 0.9, 0.5, False)
    return PdhgParameters(10, False, 1.0, 1.0, True, 0, True, 40, tc, rp, AdaptiveStepsizeParams(0.3, 0.6))


@pytest.mark.strict_rows
@pytest.mark.parametrize("host_rescale", [False, True], ids=["device_rescale", "host_rescale"])
def test_whole_solves_match_optimize(gpu_required, row_order_mode, monkeypatch, host_rescale):
    """optimize_batch on a family of four QPs against optimize per member: reason, iteration count and solutions bit for
    bit (strict order), rescaled on the device and with PDHG_HOST_RESCALE=1 (the factory then receives four host-scaled
    problems whose scaled objective matrices must pass as one)."""
    if host_rescale:
        monkeypatch.setenv("PDHG_HOST_RESCALE", "1")
    probs = random_qp_family(60, 80, 4, seed=12)
    params = _solve_params()
    got = optimize_batch(params, probs)
    for k, (g, q) in enumerate(zip(got, probs)):
        w = optimize(params, q)
        assert g.termination_reason == w.termination_reason, k
        assert g.iteration_count == w.iteration_count, (k, g.iteration_count, w.iteration_count)
        assert _same(g.primal_solution, w.primal_solution) and _same(g.dual_solution, w.dual_solution), k
    assert {g.termination_string for g in got} == {"OPTIMAL"}, [g.termination_string for g in got]


@pytest.mark.short_rows
def test_lifetime(gpu_required, row_order_mode):
    """Create, set Q, rescale, close; create with Q and close without ever stepping; replace Q by another and close."""
    probs = random_qp_family(30, 40, 2, seed=13)
    batch = HipPdhgBatch.from_problems(probs, device_id=0)
    batch.rescale(2, True, 1.0)
    batch.close()
    batch = HipPdhgBatch.from_problems(probs, device_id=0)
    batch.close()
    batch = HipPdhgBatch.from_problems(probs, device_id=0)
    try:
        batch.set_objective_matrix(_small_q(40, 14, "general"))
        raw = batch.trial_step(np.full(2, 0.1), np.ones(2))
        assert np.isfinite(raw).all()
        with pytest.raises(_lib.PdhgHipError):     # the solo setter keeps refusing a member
            batch.members[0]._upload_objective_matrix(probs[0].objective_matrix)
    finally:
        batch.close()
