"""The two persistent kernels of csrc/trial_kernel.hpp -- trial_kernel (one launch per trial) and steps_kernel (whole
batches of adaptive take_steps per launch, all-XCD and XCD-local) -- and the shard-group kernel that runs the same
product_phase, at the places where their code branches: long rows of two, three and four chunks and the tickets that
finish them across launches of both kernels, row-block counts that leave a tail in the XCD remap, products of different
item counts, several items per workgroup, the XCD-local threshold, the elementwise phases' pairs, tail and stride, row
blocks closed by their row count, degenerate shapes and the QP phases.

Every handle is made with PDHG_GRAPH=1, PDHG_COOP=1 and PDHG_SMALL_LP=0 and must report trial_graph == 2; every test
asserts from layout_info() (held to the restatement of the layout rule below) that its matrix takes the branch it is
named for.

SINGLE trials (trial_step, trial_primal + trial_dual) are held to the CPU oracle from the device's own current state
(tests/helpers.py: assert_trial_matches_oracle, the project's existing bars); the oracle accepts the trial point the
device returned, so the averages must then be the oracle's bit for bit.  MULTI-STEP launches cannot be stopped trial by
trial: they are held bitwise to a twin handle that takes the same steps as single trial_kernel launches
(PDHG_DEVICE_LOOP=0) -- step sizes and counters after every batch, iterate, dual product, trial buffers, averages -- and,
where every row and column stays within bitexact_row_limit(), bitwise to the exact-sums oracle as well."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import folp_loader

folp = folp_loader.load()
from firstorderlp_jl_amd import HipPdhgEngine, QuadraticProgrammingProblem  # noqa: E402
from firstorderlp_jl_amd.primal_dual_hybrid_gradient import AdaptiveStepsizeParams, PdhgSolverState, take_steps  # noqa: E402
from firstorderlp_jl_amd.quadratic_programming import linear_programming_problem  # noqa: E402
from tests import helpers as H  # noqa: E402
from tests.test_gpu_batch_edges import _const, _row_and_col_nnz, _same  # noqa: E402
from tests.test_gpu_edge_shapes import CASES  # noqa: E402

pytestmark = pytest.mark.gpu

TPB = _const("common.hpp", "TPB")
BLOCK_NNZ = _const("common.hpp", "BLOCK_NNZ")
NUM_XCD = _const("common.hpp", "NUM_XCD")
LONG_CHUNK = BLOCK_NNZ                 # common.hpp: constexpr int LONG_CHUNK = BLOCK_NNZ
with open(os.path.join(os.path.dirname(os.path.abspath(folp.__file__)), "csrc", "common.hpp")) as _f:
    MAX_ROWS_PER_BLOCK = int(re.search(r"#define PDHG_MAX_ROWS_PER_BLOCK \((\d+) \* TPB\)", _f.read()).group(1)) * TPB
LOCAL_MAX_GRID = 32                    # host_trial_coop.hpp, steps_local_prepare: the XCD-local mode up to this grid

POLICY = AdaptiveStepsizeParams(0.3, 0.6)
BASE_ENV = {"PDHG_GRAPH": "1", "PDHG_COOP": "1", "PDHG_SMALL_LP": "0"}
KNOBS = ("PDHG_COOP_WGS", "PDHG_COOP_FORCE", "PDHG_COOP_LOCAL", "PDHG_XCD_REMAP", "PDHG_BLOCK_CAP", "PDHG_STEPS_TEST_TABLE",
         "PDHG_GROUP_COOP", "PDHG_VERBOSE")

LENS = H.LADDER_LENS + (4096, 4097, 6145)      # long rows of 2, 2, 2, 3 and 4 chunks (2049, 2176, 4096, 4097, 6145)
TWO_ROUNDS = [("trial", 1.0), ("accept",), ("trial", 1.0), ("averages",), ("accept",)]


def _stream_layout(row_nnz, cap=BLOCK_NNZ):
    """(row blocks, long rows, long-row chunks) of a product whose rows hold row_nnz entries: build_stream_tables
    (csrc/layout.hpp) restated.  A row beyond BLOCK_NNZ entries is long, one chunk per LONG_CHUNK entries; a block takes
    consecutive rows while it stays within BLOCK_NNZ entries and MAX_ROWS_PER_BLOCK rows, and is closed once a further row
    would bring it beyond `cap` (PDHG_BLOCK_CAP).  (The equal-cost re-cut applies only beyond one item per compute
    unit: no matrix of this file comes near.)"""
    blocks = longs = chunks = 0
    r, rows = 0, len(row_nnz)
    while r < rows:
        if row_nnz[r] > BLOCK_NNZ:
            longs, chunks, r = longs + 1, chunks + -(-int(row_nnz[r]) // LONG_CHUNK), r + 1
            continue
        r0, nn = r, 0
        while r < rows and r - r0 < MAX_ROWS_PER_BLOCK:
            k = int(row_nnz[r])
            if k > BLOCK_NNZ - nn or (nn > 0 and k > cap - nn):
                break
            nn, r = nn + k, r + 1
        blocks += 1
    return blocks, longs, chunks


def _expected(A, Q=None, cap=BLOCK_NNZ, remap=True, wgs=None):
    """What layout_info() must say of A, the items of each product (row blocks -- a whole number of eights under the
    XCD remap -- plus long-row chunks) and the grid of the persistent launch (coop_prepare, host_trial_coop.hpp)."""
    out = {}

    def items(nnz):
        b, l, c = _stream_layout(nnz, cap)
        return (b, l, c), (-(-b // NUM_XCD) * NUM_XCD if remap else b) + c

    for key, nnz in zip(("A", "At"), _row_and_col_nnz(A)):
        (out[key + "_blocks"], out[key + "_long_rows"], out[key + "_long_chunks"]), out[key + "_items"] = items(nnz)
    most = max(out["A_items"], out["At_items"])
    if Q is not None:
        (out["Q_blocks"], out["Q_long_rows"], out["Q_long_chunks"]), out["Q_items"] = items(np.diff(sp.csr_matrix(Q).indptr))
        _, qt_items = items(np.diff(sp.csc_matrix(Q).indptr))
        most = max(most, out["Q_items"], out["A_items"] + qt_items)
    out["grid"] = max(8, -(-most // 8) * 8)
    if wgs is not None:
        out["grid"] = max(8, min(out["grid"], wgs // 8 * 8))
    return out


def _assert_layout(info, want):
    for key in ("A_blocks", "A_long_rows", "A_long_chunks", "At_blocks", "At_long_rows", "At_long_chunks"):
        assert info[key] == want[key], (key, info[key], want[key])


class _Out:
    pass


def _sync(o, eng):
    o.x, o.y = eng.get_current()
    o.aty = eng.get_dual_product()


def _drive(p, script, monkeypatch, device_loop, env=None, check=True, start_seed=5, step_pw=None, capfd=None, graph=2,
           local=None, label="", **engine_kw):
    """One handle through `script`, a list of
      ("trial", f)        trial_step at f times the current step size (no accept: the next trial repeats it),
      ("accept",)         accept the last trial, weight = the current step size,
      ("mp", f1, f2, ..)  trial_primal, then trial_dual at f times the step size with theta = f for each f,
      ("scale", f)        the current step size times f,
      ("steps", k)        take_steps(k): the multi-step kernel with device_loop, else single trial_kernel launches,
      ("averages",)       read the averages (this flushes a deferred update: placed where none must ride on).
    check: every single trial against the oracle from the device's own state; the oracle accepts what the device
    accepted, so at ("averages",) and at the end the averages must be its own, bitwise, for as long as it has seen every
    accept; where every row and column is within bitexact_row_limit() it takes the ("steps", k) too, with exact sums, and
    step size, counters and iterate must be its own bitwise after every batch.  Returns the record to compare with a
    twin's (.rec), layout_info() before and after (.info0, .info) and the launch's grid (.grid, with capfd)."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in dict(BASE_ENV, PDHG_DEVICE_LOOP="1" if device_loop else "0", **(env or {})).items():
        monkeypatch.setenv(k, v)
    if capfd is not None:
        monkeypatch.setenv("PDHG_VERBOSE", "1")
        capfd.readouterr()
    A = p.constraint_matrix
    m, n = A.shape
    Q = p.objective_matrix if p.objective_matrix is not None and p.objective_matrix.nnz > 0 else None
    row_nnz, col_nnz = _row_and_col_nnz(A)
    lim = H.bitexact_row_limit()
    exact = check and Q is None and max(row_nnz.max(initial=0), col_nnz.max(initial=0)) <= lim
    out = _Out()
    out.rec, out.exact, out.grid = [], exact, None
    eng = HipPdhgEngine.from_problem(p, **engine_kw)
    o = None
    try:
        out.info0 = eng.layout_info()
        out.describe = eng.layout_describe() if Q is not None else None
        if capfd is not None:
            out.grid = int(re.search(r"one-launch trial: (\d+) workgroups", capfd.readouterr().err).group(1))
        if graph is not None:
            assert out.info0["trial_graph"] == graph, out.info0["trial_graph"]
        step, pw = step_pw or H.initial_step_and_weight(p)
        st = PdhgSolverState(eng, step_size=step, primal_weight=pw)
        if start_seed is not None:
            rng = np.random.default_rng(start_seed)
            x0, y0 = rng.random(n), rng.standard_normal(m)
            eng.set_current(x0, y0)
        if check:
            o = H.oracle_from_problem(p)
            o.exact_sums = True
            o.primal_weight = pw
            if start_seed is not None:
                o.x, o.y = x0, y0
                o.recompute_dual_product()
                # set_current's A'y is the separate product kernel's: held to its own bar, then taken over
                H.assert_rows_match_oracle(eng.get_dual_product(), o.aty, col_nnz, abs(sp.csr_matrix(A)).T @ np.abs(y0),
                                           label + ": A'y of the start")
        follows, accepts, last = check, 0, None       # follows: the oracle has seen every accept so far

        def averages(where):
            got = eng.get_average()
            out.rec.append(got)
            if follows and accepts:
                for a, b, name in zip(got, o.compute_average(), ("x", "y")):
                    assert _same(a, b), f"{label} {where}: average of {name} is not the oracle's"

        for k, op in enumerate(script):
            what = f"{label} op {k} {op}"
            if op[0] == "trial":
                s = st.step_size * op[1]
                raw = eng.trial_step(s, pw, 1.0)
                last = eng.get_trial()
                out.rec.append((raw,) + last)
                if check:
                    _sync(o, eng)
                    H.assert_trial_matches_oracle(raw, last, o, s, pw, A, what, Q=Q)
            elif op[0] == "mp":
                s = st.step_size
                eng.trial_primal(s, pw)
                if check:
                    _sync(o, eng)
                    o.trial_primal(s, pw)
                for f in op[1:]:
                    raw = eng.trial_dual(s * f, pw, f)
                    last = eng.get_trial()
                    out.rec.append((raw,) + last)
                    if check:
                        H.assert_trial_matches_oracle(raw, last, o, s * f, pw, A, what, theta=f, dual_only=True, Q=Q)
            elif op[0] == "accept":
                eng.accept(st.step_size)
                accepts += 1
                if check:
                    o.step_size = st.step_size
                    o.accept(*last)
            elif op[0] == "scale":
                st.step_size *= op[1]
            elif op[0] == "averages":
                averages(what)
            elif op[0] == "steps":
                if exact and follows:
                    _sync(o, eng)
                    o.step_size = st.step_size
                    before, want_done = o.total_number_iterations, 0
                    while want_done < op[1] and not o.numerical_error:
                        o.take_step_adaptive(POLICY.reduction_exponent, POLICY.growth_exponent)
                        want_done += 1
                it0 = st.total_number_iterations
                done = take_steps(POLICY, st, op[1])
                assert done == op[1] or st.numerical_error, what
                accepts += done
                now = eng.get_current()
                out.rec.append((st.step_size, st.total_number_iterations, st.cumulative_kkt_passes, st.numerical_error, done)
                               + now + (eng.get_dual_product(),) + eng.get_trial())
                if exact and follows:
                    assert done == want_done and st.numerical_error == o.numerical_error, what
                    assert st.total_number_iterations - it0 == o.total_number_iterations - before, what
                    assert H._bits64(st.step_size) == H._bits64(o.step_size), f"{what}: step size {st.step_size!r} != {o.step_size!r}"
                    for a, b, name in zip(now, (o.x, o.y), ("x", "y")):
                        assert _same(a, b), f"{what}: {name} is not the exact-sums oracle's"
                else:
                    follows = False
            out.rec.append(np.array(eng.average_info()))
            if st.numerical_error:
                break
        out.info = eng.layout_info()
        averages(label + " at the end")
        out.rec.append((st.step_size, st.total_number_iterations, st.cumulative_kkt_passes, st.numerical_error))
        out.numerical_error = st.numerical_error
        if device_loop and graph == 2:
            assert out.info["device_loop"] == 1, label
            if local is not None:
                assert out.info["steps_local"] == local, (label, out.info["steps_local"], local)
    finally:
        eng.close()
        if o is not None:
            o.close()
    return out


def _assert_same_record(a, b, label):
    assert len(a.rec) == len(b.rec), label
    for k, (u, v) in enumerate(zip(a.rec, b.rec)):
        u, v = (u, v) if isinstance(u, tuple) else ((u,), (v,))
        assert len(u) == len(v), (label, k)
        for j, (s, t) in enumerate(zip(u, v)):
            assert _same(s, t), f"{label}: entry {k}.{j} of the record differs"


# ---- 1: the row-length ladder through trial_kernel ----------------------------------------------------------------
@pytest.mark.parametrize("eq", ["none", "third", "all"])
@pytest.mark.parametrize("blocks", ["both", "rows", "cols"])
def test_row_length_ladder(gpu_required, row_order_mode, monkeypatch, blocks, eq):
    """Rows of every length round the 256-entry and the 2048-entry thresholds and long rows of 2, 3 and 4 chunks: in
    both products, in A xbar alone (blocks="rows") and in A'y' alone ("cols"), where the two products have different
    item counts (a workgroup's prefetched first item is a chunk in one phase and a row block or nothing in the next); no
    equality, a third, every row."""
    m = H.ladder_lp(LENS, seed=3, blocks=blocks).constraint_matrix.shape[0]
    p = H.ladder_lp(LENS, seed=3, num_eq={"none": 0, "third": m // 3, "all": m}[eq], blocks=blocks)
    A = p.constraint_matrix
    want = _expected(A)
    for key, nnz in zip(("A", "At"), _row_and_col_nnz(A)):
        chunk_counts = set((-(-nnz[nnz > BLOCK_NNZ] // LONG_CHUNK)).tolist())
        has_long = blocks == "both" or (key == "A") == (blocks == "rows")
        assert (want[key + "_long_rows"] >= 3 and {2, 3, 4} <= chunk_counts) if has_long else want[key + "_long_rows"] == 0
    assert want["A_items"] != want["At_items"] or blocks == "both"
    out = _drive(p, TWO_ROUNDS, monkeypatch, device_loop=False, label=f"ladder {blocks} {eq}")
    _assert_layout(out.info0, want)


# ---- 2: the long rows' tickets across launches of both kernels ------------------------------------------------------
TICKET_SCRIPT = [("trial", 1.0), ("trial", 0.5), ("accept",), ("steps", 5), ("trial", 1.0), ("steps", 1), ("scale", 300.0),
                 ("steps", 7), ("mp", 1.2, 0.84), ("accept",), ("trial", 1.0)]


@pytest.mark.parametrize("table", [None, "3"], ids=["whole_take_steps", "launches_end_inside_take_steps"])
def test_ticket_bookkeeping_across_launches_and_kernels(gpu_required, row_order_mode, monkeypatch, table):
    """A long row is finished by the workgroup that draws ticket (uses + 1) * chunks of the row; `uses` is the host's
    count of the launches of EITHER kernel (CsrDev::coop_uses).  A trial, the same trial again at half the step (a
    rejection), an accept, five take_steps in one launch, a trial, one take_step, seven take_steps from a step size 300
    times too long (rejections inside the launch), a Malitsky-Pock step (trial_primal, two trial_dual), an accept and a
    last trial: if the count drifts from the tickets a long row keeps an old y' and the oracle and the twin both
    differ.  With PDHG_STEPS_TEST_TABLE=3 the launches end inside take_steps and the host finishes them."""
    p = H.ladder_lp(LENS, seed=7)
    want = _expected(p.constraint_matrix)
    assert want["A_long_rows"] >= 3 and want["At_long_rows"] >= 3 and want["grid"] > LOCAL_MAX_GRID
    env = {"PDHG_STEPS_TEST_TABLE": table} if table else {}
    got = _drive(p, TICKET_SCRIPT, monkeypatch, device_loop=True, env=env, local=0, label="device loop")
    _assert_layout(got.info0, want)
    twin = _drive(p, TICKET_SCRIPT, monkeypatch, device_loop=False, check=False, label="twin")
    _assert_same_record(got, twin, "multi-step launches against single trial_kernel launches")
    assert got.rec[-1][1] > 5 + 1 + 7   # iterations: more trials than take_steps -- the launches rejected some


# ---- 3: block counts round the XCD remap ---------------------------------------------------------------------------
def _block_matrix(kind, k, seed=21):
    """k row blocks in A and another count in A': rows of 1100 entries are one block each at the default capacity (in
    relaxed order they are summed by their wave: the helper's long-row bar); rows of 64 entries are one block each under
    PDHG_BLOCK_CAP=64 and bitwise in both orders."""
    if kind == "rows1100":
        return H.rows_with_lens([1100] * k, 1500, seed + k), {}
    return H.rows_with_lens([64] * k, 1100, seed + k), {"PDHG_BLOCK_CAP": "64"}


@pytest.mark.parametrize("remap", ["1", "0"], ids=["remap", "no_remap"])
@pytest.mark.parametrize("k", [1, 7, 8, 9, 15, 16, 17])
@pytest.mark.parametrize("kind", ["rows1100", "cap64"])
def test_block_counts_round_the_remap(gpu_required, row_order_mode, monkeypatch, kind, k, remap):
    """product_block_of: workgroup b works on block (b & 7) * per_xcd + (b >> 3) when that is a block, and stores a zero
    partial when it is not -- 1, 7, 9, 15 and 17 blocks leave such workgroups, 8 and 16 none; A' has another block
    count, so workgroups idle in one phase work in the next.  With and without the remap (PDHG_XCD_REMAP)."""
    p, env = _block_matrix(kind, k)
    env["PDHG_XCD_REMAP"] = remap
    want = _expected(p.constraint_matrix, cap=int(env.get("PDHG_BLOCK_CAP", BLOCK_NNZ)), remap=remap == "1")
    assert want["A_blocks"] == k and want["At_blocks"] != k and want["A_long_rows"] == want["At_long_rows"] == 0
    script = TWO_ROUNDS + [("steps", 20)]
    got = _drive(p, script, monkeypatch, device_loop=True, env=env, local=int(want["grid"] <= LOCAL_MAX_GRID),
                 label=f"{kind} {k} blocks")
    _assert_layout(got.info0, want)
    assert got.exact == (kind == "cap64" or H.bitexact_row_limit() >= 1100)      # cap64: the oracle, bitwise, in both orders
    twin = _drive(p, script, monkeypatch, device_loop=False, env=env, check=False)
    _assert_same_record(got, twin, "multi-step launches against single trial_kernel launches")


# ---- 4: the XCD-local threshold ------------------------------------------------------------------------------------
def _threshold_matrix(items, long):
    """`items` items in A xbar, fewer in A'y': rows of 1100 entries, one block each -- with `long`, 24 of them, a
    6145-entry row (4 chunks) and one of 6145 (32 items) or 8193 entries (5 chunks: 33 items) among them."""
    if not long:
        return H.rows_with_lens([1100] * items, 1500, 30 + items)
    lens = [1100] * 24
    lens.insert(5, 6145)
    lens.insert(20, 6145 if items == 32 else 8193)
    return H.rows_with_lens(lens, 8200, 40 + items)


@pytest.mark.parametrize("long", [False, True], ids=["blocks", "with_long_rows"])
@pytest.mark.parametrize("items", [32, 33])
def test_xcd_local_threshold(gpu_required, row_order_mode, monkeypatch, capfd, items, long):
    """A grid of 32 runs the multi-step kernel on one XCD, its workgroups numbered by ticket (another workgroup draws a
    given long-row chunk in every launch); 33 items are a grid of 40 and the all-XCD kernel.  Three batches (9, 40, 40)
    against the twin, and the XCD-local handle against one under PDHG_COOP_LOCAL=0."""
    p = _threshold_matrix(items, long)
    want = _expected(p.constraint_matrix)
    assert want["A_blocks"] + want["A_long_chunks"] == items and want["At_items"] < want["A_items"]
    assert want["grid"] == (32 if items == 32 else 40)
    assert want["A_long_rows"] == (2 if long else 0)
    script = [("trial", 1.0), ("accept",), ("steps", 9), ("steps", 40), ("steps", 40)]
    local = int(items == 32)
    got = _drive(p, script, monkeypatch, device_loop=True, capfd=capfd, local=local, label=f"{items} items")
    assert got.grid == want["grid"]
    _assert_layout(got.info0, want)
    twin = _drive(p, script, monkeypatch, device_loop=False, check=False)
    _assert_same_record(got, twin, "multi-step launches against single trial_kernel launches")
    if local:
        wide = _drive(p, script, monkeypatch, device_loop=True, env={"PDHG_COOP_LOCAL": "0"}, check=False, local=0)
        _assert_same_record(got, wide, "XCD-local against all-XCD")


# ---- 5: several items per workgroup --------------------------------------------------------------------------------
@pytest.mark.parametrize("local", ["1", "0"], ids=["xcd_local", "all_xcd"])
@pytest.mark.parametrize("which", ["ladder", "blocks17"])
def test_several_items_per_workgroup(gpu_required, row_order_mode, monkeypatch, capfd, which, local):
    """PDHG_COOP_WGS=8 with PDHG_COOP_FORCE=1: eight workgroups walk every row block and long-row chunk (on one handle
    the walk b = w, w + nwg, ... and c = nwg - 1 - w, ... otherwise takes one trip), some with chunks and blocks in one
    phase.  Partial slots are indexed by item: not a bit may differ from a handle with the default grid."""
    p = H.ladder_lp(LENS, seed=3) if which == "ladder" else _block_matrix("rows1100", 17)[0]
    env = {"PDHG_COOP_WGS": "8", "PDHG_COOP_FORCE": "1", "PDHG_COOP_LOCAL": local}
    want = _expected(p.constraint_matrix, wgs=8)
    wide = _expected(p.constraint_matrix)
    assert want["grid"] == 8 and min(want["A_items"], want["At_items"]) > 8
    if which == "ladder":
        assert want["A_long_chunks"] > 8 and want["At_long_chunks"] > 8      # more than one chunk for some workgroup, and blocks
    script = [("trial", 1.0), ("trial", 0.5), ("accept",), ("trial", 1.0), ("averages",), ("accept",), ("steps", 9),
              ("steps", 20), ("trial", 1.0)]
    got = _drive(p, script, monkeypatch, device_loop=True, env=env, capfd=capfd, local=int(local), label=f"{which} on 8 workgroups")
    assert got.grid == 8
    _assert_layout(got.info0, want)
    twin = _drive(p, script, monkeypatch, device_loop=False, env=env, check=False, capfd=capfd)
    assert twin.grid == 8
    _assert_same_record(got, twin, "multi-step launches against single trial_kernel launches")
    full = _drive(p, script, monkeypatch, device_loop=True, check=False, capfd=capfd)
    assert full.grid == wide["grid"] > 8
    _assert_same_record(got, full, "eight workgroups against the default grid")


# ---- 6: the elementwise phases' pairs, tail and stride --------------------------------------------------------------
def _one_per_column(n, transposed, seed=50):
    """Three rows, one entry per column (column j in row j mod 3) -- or its transpose: m rows of one entry, three
    columns.  Bounds of every kind at fixed places (where n allows), the rest mixed."""
    rng = np.random.default_rng(seed + n)
    A = sp.csc_matrix((rng.standard_normal(n) + 3.0, np.arange(n) % 3, np.arange(n + 1)), shape=(3, n))
    if transposed:
        A = sp.csc_matrix(A.T)
        A.sort_indices()
    m, cols = A.shape
    lb = np.where(rng.random(cols) < 0.25, -np.inf, -rng.random(cols))
    ub = np.where(rng.random(cols) < 0.25, np.inf, 1.0 + rng.random(cols))
    kinds = [(-np.inf, np.inf), (0.5, 0.5), (-np.inf, 1.0), (0.0, np.inf)]
    for j in range(min(cols, len(kinds))):      # the last elements (the odd tail among them) and the first
        lb[cols - 1 - j], ub[cols - 1 - j] = kinds[j]
    if cols > 8:
        lb[:4], ub[:4] = [k[0] for k in kinds], [k[1] for k in kinds]
    return linear_programming_problem(lb, ub, rng.standard_normal(cols), 0.0, A, rng.standard_normal(m), m // 3)


@pytest.mark.parametrize("transposed", [False, True], ids=["n", "m"])
@pytest.mark.parametrize("size", [1, 2, 3, 2047, 2048, 2049, 4097])
def test_elementwise_strides(gpu_required, row_order_mode, monkeypatch, capfd, size, transposed):
    """primal_body works on pairs (2p, 2p + 1), strided by nwg * TPB = 2048 pairs on eight workgroups, the odd tail on
    workgroup 0: n = 1 (tail alone), 2, 3, one pair short of a stride's threads, one stride of threads and one element
    more, and beyond one stride of pairs; bounds of every kind on the tail.  Transposed, the same sizes are the rows of
    the dual epilogue and of the row-block walk."""
    p = _one_per_column(size, transposed)
    A = p.constraint_matrix
    want = _expected(A)
    lb, ub = p.variable_lower_bound, p.variable_upper_bound
    assert np.isinf(lb).any() and np.isinf(ub).any() and ((lb == ub).any() or len(lb) == 1)
    if not transposed and size > 8:
        assert np.isinf(lb[-1]) and np.isinf(ub[-1]) and lb[-2] == ub[-2]
    script = TWO_ROUNDS + [("steps", 3), ("steps", 9)]
    got = _drive(p, script, monkeypatch, device_loop=True, capfd=capfd, local=1, label=f"{size} {'rows' if transposed else 'columns'}")
    assert got.grid == 8 == want["grid"]
    _assert_layout(got.info0, want)
    assert got.exact == (-(-size // 3) <= H.bitexact_row_limit())
    twin = _drive(p, script, monkeypatch, device_loop=False, check=False)
    _assert_same_record(got, twin, "multi-step launches against single trial_kernel launches")


# ---- 7: row blocks closed by their row count ------------------------------------------------------------------------
def _one_per_row(m, seed=60):
    rng = np.random.default_rng(seed + m)
    A = sp.csr_matrix((rng.standard_normal(m) + 3.0, np.arange(m) % 16, np.arange(m + 1)), shape=(m, 16)).tocsc()
    A.sort_indices()
    lb = np.where(rng.random(16) < 0.25, -np.inf, -rng.random(16))
    ub = np.where(rng.random(16) < 0.25, np.inf, 1.0 + rng.random(16))
    return linear_programming_problem(lb, ub, rng.standard_normal(16), 0.0, A, rng.standard_normal(m), m // 3)


@pytest.mark.parametrize("m,blocks", [(255, 1), (256, 1), (257, 1), (1023, 1), (1024, 1), (1025, 2), (2049, 3)])
def test_row_blocks_by_row_count(gpu_required, row_order_mode, monkeypatch, m, blocks):
    """Rows of one entry: a block is closed by MAX_ROWS_PER_BLOCK = 1024 rows, not by its entries; TPB - 1, TPB and
    TPB + 1 rows are one trip of a workgroup's threads through the epilogue and the start of a second."""
    assert MAX_ROWS_PER_BLOCK == 1024 and TPB == 256
    p = _one_per_row(m)
    want = _expected(p.constraint_matrix)
    assert want["A_blocks"] == blocks and want["At_blocks"] <= 2
    script = TWO_ROUNDS + [("steps", 3), ("steps", 9)]
    got = _drive(p, script, monkeypatch, device_loop=True, local=1, label=f"{m} rows")
    _assert_layout(got.info0, want)
    assert got.exact
    twin = _drive(p, script, monkeypatch, device_loop=False, check=False)
    _assert_same_record(got, twin, "multi-step launches against single trial_kernel launches")


def test_empty_rows_in_the_middle(gpu_required, row_order_mode, monkeypatch):
    """300 rows of three entries, 1500 rows without any, 300 more: two row blocks hold nothing but empty rows' ends, and
    an empty row's y' = proj(y + sigma b) is still projected."""
    p = H.rows_with_lens([3] * 300 + [0] * 1500 + [3] * 300, 40, 71, num_eq=100)
    A = p.constraint_matrix
    want = _expected(A)
    assert want["A_blocks"] == 3
    o = H.oracle_from_problem(p)
    y0 = np.random.default_rng(5).standard_normal(2100)
    o.x, o.y = np.random.default_rng(6).random(40), y0
    o.recompute_dual_product()
    step, pw = H.initial_step_and_weight(p)
    yn = o.trial_step(step, pw, 1.0)[2][300:1800]
    o.close()
    assert (yn == 0.0).any() and (yn > 0.0).any() and not np.array_equal(yn, y0[300:1800]), "the projection does not act on the empty rows"
    script = TWO_ROUNDS + [("steps", 3), ("steps", 9)]
    got = _drive(p, script, monkeypatch, device_loop=True, local=1, label="empty rows")
    _assert_layout(got.info0, want)
    assert got.exact
    twin = _drive(p, script, monkeypatch, device_loop=False, check=False)
    _assert_same_record(got, twin, "multi-step launches against single trial_kernel launches")


# ---- 8: degenerate shapes -------------------------------------------------------------------------------------------
DEGENERATE_SCRIPT = TWO_ROUNDS + [("steps", 5), ("steps", 7)]


@pytest.mark.short_rows
@pytest.mark.parametrize("device_loop", [False, True], ids=["trial_kernel", "steps_kernel"])
@pytest.mark.parametrize("name", sorted(k for k in CASES if k != "no_constraints"))
def test_degenerate_shapes(gpu_required, row_order_mode, monkeypatch, name, device_loop):
    """An all-zero matrix, 1 x 1, empty rows and columns, a single column, a single row through both kernels: single
    trials and twelve adaptive steps, every vector and scalar the exact-sums oracle's bit for bit, up to and including a
    step that raises numerical_error."""
    p = CASES[name]()
    got = _drive(p, DEGENERATE_SCRIPT, monkeypatch, device_loop=device_loop, start_seed=None, step_pw=(0.3, 1.0),
                 local=1 if device_loop else None, label=name)
    assert got.exact
    _assert_layout(got.info0, _expected(p.constraint_matrix))


@pytest.mark.short_rows
def test_no_constraints_stays_off_the_persistent_kernels(gpu_required, row_order_mode, monkeypatch):
    """m = 0: there is no product to fuse; the handle reports another path and still matches the oracle bit for bit."""
    p = CASES["no_constraints"]()
    got = _drive(p, DEGENERATE_SCRIPT, monkeypatch, device_loop=True, start_seed=None, step_pw=(0.3, 1.0), graph=None,
                 label="no_constraints")
    assert got.info0["trial_graph"] != 2 and got.info["trial_graph"] != 2
    assert got.exact


# ---- 9: a QP through trial_kernel -----------------------------------------------------------------------------------
def _arrow_qp(n=5001, m=300, seed=80):
    """A short-row A of few blocks and Q = diag(d) + e0 u' + u e0' + B'B: row and column 0 of Q hold 2101 entries (long:
    two chunks in the Q x and Q'dx phases), positive semidefinite because d0 = 1 + sum u_i^2 / d_i."""
    rng = np.random.default_rng(seed)
    base = H.rows_with_lens([8] * m, n, seed + 1)
    d = 0.5 + rng.random(n)
    idx = np.sort(rng.choice(np.arange(1, n), size=2100, replace=False))
    u = rng.standard_normal(2100) * 0.05
    d[0] = 1.0 + np.sum(u * u / d[idx])
    B = sp.random(150, n, density=3.0 / n, format="csr", random_state=seed + 2)
    arrow = sp.coo_matrix((np.concatenate([u, u]), (np.concatenate([np.zeros(2100, dtype=np.int64), idx]),
                                                     np.concatenate([idx, np.zeros(2100, dtype=np.int64)]))), shape=(n, n))
    Q = (sp.diags(d) + arrow + B.T @ B).tocsc()
    Q.sort_indices()
    return QuadraticProgrammingProblem(
        variable_lower_bound=base.variable_lower_bound, variable_upper_bound=base.variable_upper_bound, objective_matrix=Q,
        objective_vector=base.objective_vector, objective_constant=0.0, constraint_matrix=base.constraint_matrix,
        right_hand_side=base.right_hand_side, num_equalities=base.num_equalities)


@pytest.mark.parametrize("n,remap", [(5001, "0"), (8193, "1")], ids=["5001_no_remap", "8193_remap"])
def test_qp_through_trial_kernel(gpu_required, row_order_mode, monkeypatch, capfd, n, remap):
    """The partials of dx . (Q'dx) are more blocks than the grid has workgroups (dot_body's b += nwg takes a second
    trip), n is odd (diff_pairs_body's tail), Q has a long row and column and more items than A.  n = 5001 is 20 blocks;
    under the XCD remap every product's row blocks count in eights and the grid is 24, so that size runs with
    PDHG_XCD_REMAP=0 (a grid of 16), and n = 8193 (33 blocks on a grid of 32) with the remap.  Adaptive trials with a
    rejection, and a Malitsky-Pock step (phase 0 is xbar alone), against the oracle and bitwise against PDHG_COOP=0."""
    p = _arrow_qp(n)
    A, Q = p.constraint_matrix, p.objective_matrix
    want = _expected(A, Q=Q, remap=remap == "1")
    q_blocks = -(-n // TPB)
    assert n % 2 == 1 and q_blocks == {5001: 20, 8193: 33}[n] > want["grid"]
    assert want["Q_long_rows"] == 1 and want["Q_long_chunks"] == 2 and want["Q_items"] > want["A_items"]
    script = [("trial", 1.0), ("trial", 0.5), ("accept",), ("trial", 1.0), ("averages",), ("accept",), ("mp", 1.2, 0.84),
              ("accept",), ("trial", 1.0)]
    got = _drive(p, script, monkeypatch, device_loop=False, env={"PDHG_XCD_REMAP": remap}, capfd=capfd, label="QP")
    assert got.grid == want["grid"] < q_blocks
    _assert_layout(got.info0, want)
    desc = got.describe["Q"]
    assert desc["row_blocks"] == want["Q_blocks"] and desc["long_rows"] == 1
    plain = _drive(p, script, monkeypatch, device_loop=False, env={"PDHG_COOP": "0", "PDHG_XCD_REMAP": remap}, check=False, graph=None)
    assert plain.info0["trial_graph"] != 2
    _assert_same_record(got, plain, "trial_kernel against the separate launches")


# ---- 10: the shard-group kernel runs the same product_phase ---------------------------------------------------------
@pytest.mark.parametrize("shards", [2, 3])
@pytest.mark.parametrize("which", ["ladder", "blocks17"])
def test_shard_group_kernel(gpu_required, row_order_mode, monkeypatch, which, shards):
    """group_kernel.hpp: several shards share one device's workgroups, each walking its shard's blocks and chunks with
    product_phase(w, nwg).  20 adaptive steps, bitwise the per-launch group path (PDHG_GROUP_COOP=0)."""
    p = H.ladder_lp(LENS, seed=3) if which == "ladder" else _block_matrix("rows1100", 17)[0]
    script = [("steps", 20)]
    got = _drive(p, script, monkeypatch, device_loop=True, check=False, graph=None, device_ids=[0] * shards)
    assert got.info["group_coop_trials"] >= 20 and got.info["group_coop_fallbacks"] == 0
    ref = _drive(p, script, monkeypatch, device_loop=True, env={"PDHG_GROUP_COOP": "0"}, check=False, graph=None,
                 device_ids=[0] * shards)
    assert ref.info["group_coop_trials"] == 0
    _assert_same_record(got, ref, "group kernel against the per-launch group path")
