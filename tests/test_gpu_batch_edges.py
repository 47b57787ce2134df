"""The batched-trial kernels (csrc/batch_kernels.hpp, behind HipPdhgBatch) against the CPU oracle at the places where
they branch: every row length around the 8-entry step, the 128-entry chunk and the long-row threshold of the order in use,
the second trip through a row's chunk sums, every member count's lane-group width, masks over long rows, the equality
split at its ends, fixed variables, degenerate shapes and each kernel's grid-stride loop.

Every member is compared with its OWN oracle state (tests/helpers.py: assert_trial_matches_oracle, the project's existing
bars).  A case runs two rounds: a trial from a random nonzero start, an accept on both sides, then a second trial on which
the deferred average update rides.  The oracle accepts the trial point the device returned (just verified against its
own), so the second round starts from the same bits on both sides and is held to the same bars as the first, and the
averages are then the oracle's bit for bit, long rows or not.  Every test asserts from the matrix that the branch it is
named for is taken."""
import copy
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import folp_loader

folp = folp_loader.load()
from firstorderlp_jl_amd import HipPdhgBatch  # noqa: E402
from firstorderlp_jl_amd.quadratic_programming import linear_programming_problem  # noqa: E402
from tests import helpers as H  # noqa: E402
from tests.test_gpu_edge_shapes import CASES  # noqa: E402

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


def _members(p, K, seed):
    """K LPs on p's matrix (the same object: no copies of a large one) with their own c, b and bounds; fixed variables
    stay fixed, at another value."""
    rng = np.random.default_rng(seed)
    n, m = len(p.objective_vector), len(p.right_hand_side)
    out = []
    for k in range(K):
        c = p.objective_vector * (1.0 + 0.5 * rng.random(n)) if k else p.objective_vector.copy()
        b = p.right_hand_side * (1.0 + 0.3 * rng.random(m)) if k else p.right_hand_side.copy()
        fixed = p.variable_lower_bound == p.variable_upper_bound
        lb = p.variable_lower_bound - np.where(fixed, 0.125 * k, 0.0)
        ub = np.where(fixed, lb, p.variable_upper_bound + k)
        q = copy.copy(p)
        q.objective_vector, q.right_hand_side, q.variable_lower_bound, q.variable_upper_bound = c, b, lb, ub
        out.append(q)
    return out


def _row_and_col_nnz(A):
    return np.diff(sp.csr_matrix(A).indptr), np.diff(sp.csc_matrix(A).indptr)


def _two_rounds(problems, mask=None, seed=5):
    """The device does both rounds first (its vectors are taken to the host after each trial); then every active member
    is verified against an oracle state of its own, one at a time.  Returns the entries per row and per column of the
    matrix and, per active member, the ORACLE's y' of the first trial."""
    K = len(problems)
    A = problems[0].constraint_matrix
    m, n = A.shape
    row_nnz, col_nnz = _row_and_col_nnz(A)
    absA = abs(sp.csr_matrix(A))
    rng = np.random.default_rng(seed)
    states = [(rng.random(n), rng.standard_normal(m)) for _ in range(K)]
    ss = 0.5 / (1.0 + np.arange(K))
    pw = 1.0 + np.arange(K) * 0.25
    act = np.ones(K, dtype=np.int32) if mask is None else np.asarray(mask, dtype=np.int32)
    batch = HipPdhgBatch.from_problems(problems, device_id=0)
    try:
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
    oracle_y1 = {}
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
            H.assert_trial_matches_oracle(raw1[k], trial1[k], o, ss[k], pw[k], A, f"member {k}, trial 1")
            oracle_y1[k] = o.y_next
            o.step_size = ss[k]
            o.accept(*trial1[k])
            H.assert_trial_matches_oracle(raw2[k], trial2[k], o, ss[k], pw[k], A, f"member {k}, trial 2")
            for a, b, name in zip(avg[k], o.compute_average(), ("x", "y")):
                assert _same(a, b), f"member {k}: average of {name}"
        finally:
            o.close()
    return row_nnz, col_nnz, oracle_y1


def _assert_both_sides_of_the_threshold(row_nnz, col_nnz):
    """Rows of A (for A xbar) and columns of A (the rows of A'y') at long_thr and at long_thr + 1 entries; no entry at all,
    the shortest and the longest masked tail alone and after a full step, no tail after one and two full steps; whole
    chunks with and without one entry more, below the threshold and beyond it."""
    thr = H.bitexact_row_limit()
    for nnz in (row_nnz, col_nnz):
        have = set(nnz.tolist())
        assert {thr, thr + 1} <= have, "no rows on both sides of the long-row threshold"
        assert {0, 1, BATCH_U - 1, BATCH_U, BATCH_U + 1, 2 * BATCH_U - 1, 2 * BATCH_U, 2 * BATCH_U + 1} <= have
        assert {BATCH_CHUNK - 1, BATCH_CHUNK, BATCH_CHUNK + 1} <= have
        long_ = nnz[nnz > thr]
        assert np.any(long_ % BATCH_CHUNK == 0) and np.any(long_ % BATCH_CHUNK == 1), "no long row of 128 c and 128 c + 1 entries"


@pytest.mark.parametrize("K", [1, 2, 5, 16, 17, 32])
def test_row_length_ladder(gpu_required, row_order_mode, K):
    """Kp = 1, 2, 8, 16, 32, 32 (K = 5 and 17 with padding lanes) over rows and columns of every length of the ladder,
    in both row orders."""
    p = H.ladder_lp(H.LADDER_LENS, seed=3)
    row_nnz, col_nnz, _ = _two_rounds(_members(p, K, 1))
    _assert_both_sides_of_the_threshold(row_nnz, col_nnz)
    assert np.any(p.variable_lower_bound == p.variable_upper_bound) and np.any(np.isinf(p.variable_lower_bound)) \
        and np.any(np.isinf(p.variable_upper_bound))


@pytest.mark.parametrize("K,giant", [(32, False), (1, True)], ids=["K32", "K1_33000"])
def test_second_trip_through_the_chunk_sums(gpu_required, row_order_mode, K, giant):
    """batch_long_final_kernel's lane group adds chunk sums g, g + gpb, ...: a second one only for a row of more than gpb
    chunks -- more than 1024 entries at K = 32, more than 32 768 at K = 1 (the 33 000-entry row and column)."""
    lens = H.LADDER_LENS + ((33000,) if giant else ())
    p = H.ladder_lp(lens, seed=4)
    row_nnz, col_nnz, _ = _two_rounds(_members(p, K, 2))
    thr, gpb = H.bitexact_row_limit(), _gpb(K)
    for nnz in (row_nnz, col_nnz):
        chunks = -(-nnz[nnz > thr] // BATCH_CHUNK)
        assert np.any(chunks > gpb), (gpb, chunks.max())


@pytest.mark.parametrize("mask", [[1, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 1], [1, 0, 1, 0, 1, 0]], ids=["first", "last", "alternating"])
def test_masks_with_long_rows(gpu_required, row_order_mode, mask):
    """Inactive members keep the bits of their trial, current and average vectors and their raw rows stay NaN; active
    members match the oracle on short and long rows; an all-zero mask touches nothing (_two_rounds)."""
    p = H.ladder_lp(H.LADDER_LENS, seed=6)
    row_nnz, col_nnz, _ = _two_rounds(_members(p, 6, 3), mask=mask)
    thr = H.bitexact_row_limit()
    assert np.any(row_nnz > thr) and np.any(col_nnz > thr)


@pytest.mark.short_rows
@pytest.mark.parametrize("which", ["none", "all"])
def test_equality_split_at_its_ends(gpu_required, row_order_mode, which):
    """num_eq = 0 (row 0 is the first inequality) and num_eq = m (no inequality) on a ladder of short rows.  With
    num_eq = 0 row 0's right-hand side is far below what the row can reach, so its y' is projected to 0 in every member;
    with num_eq = m the last row's is as far below, and its y' must stay negative."""
    lens = (0, 1, 7, 8, 9, 15, 16, 17, 127, 128, 129, 255)
    base = H.ladder_lp(lens, seed=8)
    m = base.constraint_matrix.shape[0]
    num_eq = 0 if which == "none" else m
    row = 0 if which == "none" else m - 1
    b = base.right_hand_side.copy()
    b[row] = -1e4
    p = linear_programming_problem(base.variable_lower_bound, base.variable_upper_bound, base.objective_vector, 0.0,
                                   base.constraint_matrix, b, num_eq)
    probs = _members(p, 3, 4)
    row_nnz, col_nnz, oracle_y1 = _two_rounds(probs)
    assert max(row_nnz.max(), col_nnz.max()) < 256
    # the precondition, from the oracle alone: the projection acts on that row (num_eq = 0) or must not (num_eq = m)
    for k in range(3):
        assert (oracle_y1[k][row] == 0.0) if which == "none" else (oracle_y1[k][row] < 0.0)


@pytest.mark.short_rows
@pytest.mark.parametrize("name", sorted(CASES))
def test_degenerate_shapes(gpu_required, row_order_mode, name):
    """No constraints (the dual product is skipped and the last kernel reads no slots of it), an all-zero matrix, 1 x 1,
    empty rows and columns, a single column, a single row: three members with their own c and bounds take 12 lockstep
    adaptive steps; every scalar and vector is the exact-sums oracle's bit for bit, a member that raises
    numerical_error included."""
    base = CASES[name]()
    probs = []
    for k in range(3):
        c = base.objective_vector * (1.0 + 0.5 * k)
        probs.append(linear_programming_problem(base.variable_lower_bound - 0.25 * k, base.variable_upper_bound + k, c, 0.0,
                                                base.constraint_matrix, base.right_hand_side * (1.0 + 0.5 * k),
                                                base.num_equalities))
    batch = HipPdhgBatch.from_problems(probs, device_id=0)
    try:
        ss, it, kkt, err, done = batch.take_steps_adaptive(12, 0.3, 0.6, np.full(3, 0.3), np.ones(3), np.zeros(3, dtype=np.int64),
                                                           np.zeros(3))
        got = [e.get_current() + e.get_average() for e in batch.members]
    finally:
        batch.close()
    for k, p in enumerate(probs):
        o = H.oracle_from_problem(p)
        o.exact_sums = True
        o.step_size, o.primal_weight = 0.3, 1.0
        steps = 0
        while steps < 12 and not o.numerical_error:
            o.take_step_adaptive(0.3, 0.6)
            steps += 1
        label = f"{name}, member {k}"
        assert H._bits64(ss[k]) == H._bits64(o.step_size), f"{label}: step size {ss[k]!r} != {o.step_size!r}"
        assert it[k] == o.total_number_iterations, label
        assert bool(err[k]) == o.numerical_error, label
        assert done[k] == steps, label
        assert kkt[k] == o.cumulative_kkt_passes, label
        for a, b, what in zip(got[k], (o.x, o.y) + o.compute_average(), ("x", "y", "x average", "y average")):
            assert _same(a, b), f"{label}: {what}"
        o.close()


def _rows_of(m, n, per_row, seed):
    """An m x n LP whose every row has exactly per_row entries (a window of consecutive columns, wrapped), with mixed
    bounds."""
    rng = np.random.default_rng(seed)
    start = rng.integers(0, n, m)
    ci = (start[:, None] + np.arange(per_row)[None, :]) % n
    A = sp.csr_matrix((rng.standard_normal(m * per_row), ci.ravel(), np.arange(m + 1) * per_row), shape=(m, n)).tocsc()
    A.sort_indices()
    lb = np.where(rng.random(n) < 0.25, -np.inf, 0.0)
    ub = np.where(rng.random(n) < 0.25, np.inf, 2.0)
    return linear_programming_problem(lb, ub, rng.standard_normal(n), 0.0, A, rng.standard_normal(m), m // 3)


@pytest.mark.short_rows
def test_spmv_grid_stride(gpu_required, row_order_mode):
    """batch_spmv_kernel at K = 32 deals BATCH_MAX_GRID * gpb = 32 768 rows per trip: 33 000 rows of 3 entries."""
    K = 32
    p = _rows_of(33000, 3000, 3, seed=12)
    row_nnz, col_nnz = _row_and_col_nnz(p.constraint_matrix)
    assert len(row_nnz) > BATCH_MAX_GRID * _gpb(K) and row_nnz.max() == 3 and col_nnz.max() < 256
    _two_rounds(_members(p, K, 5))


@pytest.mark.short_rows
def test_primal_and_transposed_grid_stride(gpu_required, row_order_mode):
    """batch_primal_kernel covers EW_MAX_BLOCKS * TPB = 524 288 columns per trip, and at K = 2 (gpb = 128)
    batch_spmv_kernel's transposed product as many rows of A': 524 588 columns of one entry each over 70 000 rows."""
    K = 2
    n, m = EW_MAX_BLOCKS * TPB + 300, 70000
    rng = np.random.default_rng(13)
    A = sp.csc_matrix((rng.standard_normal(n), np.arange(n) % m, np.arange(n + 1)), shape=(m, n))
    lb = np.where(rng.random(n) < 0.25, -np.inf, 0.0)
    ub = np.where(rng.random(n) < 0.25, np.inf, 2.0)
    p = linear_programming_problem(lb, ub, rng.standard_normal(n), 0.0, A, rng.standard_normal(m), m // 3)
    row_nnz, col_nnz = _row_and_col_nnz(A)
    assert n > EW_MAX_BLOCKS * TPB and n > BATCH_MAX_GRID * _gpb(K) and (col_nnz == 1).all() and row_nnz.max() <= 8
    _two_rounds(_members(p, K, 6))


@pytest.mark.own_row_order
def test_long_row_kernels_grid_stride(gpu_required, row_order_mode, monkeypatch):
    """batch_long_final_kernel takes BATCH_MAX_GRID = 4096 long rows per trip and batch_long_partial_kernel
    BATCH_MAX_GRID * gpb = 32 768 chunks at K = 32 (the member count with the fewest lane groups).  The smallest matrix
    beyond both bounds has the shortest long rows: BATCH_MAX_GRID * gpb / 3 + 1 = 10 923 rows of 257 entries, three
    chunks each (128, 128 and 1 entries), 2.8 M entries in relaxed order, where a row is long beyond 256 entries.  (4100
    rows of 1100 entries cross the same two bounds with 4.5 M entries; the 32 members' oracle states and trials on them
    take 7 s on the host alone.)  In strict order a row is long beyond 2048 entries, so the same coverage needs 4097 rows
    of 2049 entries -- an 8.4 M-entry matrix for each of 32 members' oracle trials, outside what a test of a few seconds
    can carry: relaxed order only."""
    monkeypatch.setenv("PDHG_ROW_ORDER", "relaxed")
    K = 32
    thr = H.bitexact_row_limit()
    assert thr == 256
    p = _rows_of(BATCH_MAX_GRID * _gpb(K) // 3 + 1, 16000, thr + 1, seed=14)
    row_nnz, col_nnz = _row_and_col_nnz(p.constraint_matrix)
    long_rows = row_nnz > thr
    assert long_rows.sum() > BATCH_MAX_GRID
    assert (-(-row_nnz[long_rows] // BATCH_CHUNK)).sum() > BATCH_MAX_GRID * _gpb(K)
    _two_rounds(_members(p, K, 7))
