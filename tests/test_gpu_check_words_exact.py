"""The 22 words of ``pdhg_eval_point`` -- and the scalars that ride in the same reduction -- against plain Python
integers (tests/check_reference.py), as numbers with NO tolerance.

The original problem and the unscaled point are small integers, the rescaling vectors powers of two: every scaling,
product, partial sum and square the kernels form is then exactly representable, floating-point addition of such numbers
is exact in any order, and so every word must EQUAL the integer -- whatever the grid, the wave tree, the second stage,
the number of shards or the host path (one handle, shard group, fleet, batch) that reduced it.

The generator lands every column and every row in a chosen cell of the branch table (bounds x sign g x sign g_h x
position of x x sign x; row kind x sign(b - A x) x sign(-A x) x sign y).  ``census`` asserts from the reference's own
cells, before any device is touched, that EVERY cell of the table is occupied: over the variants (ne, scaling) of a
shape from 513 x 511 upward, over the union of the smaller shapes otherwise.

POINT_AVERAGE is left out: an average is exact only after a take_step, whose iterate is not an integer point."""
import dataclasses
import functools
from dataclasses import dataclass

import numpy as np
import pytest
import scipy.sparse as sp

from firstorderlp_jl_amd import HipPdhgBatch, HipPdhgEngine, HipPdhgFleet, _lib
from firstorderlp_jl_amd.quadratic_programming import QuadraticProgrammingProblem
from tests import check_reference as R

CURRENT, RESTART = _lib.POINT_CURRENT, _lib.POINT_RESTART
INF = np.inf

# what the generator chooses per column: (bounds, position) x sign g, 45 patterns; per row: sign(b - A x)
COLUMN_PATTERNS = [(bk, pos, sg) for bk in R.BOUNDS for pos in R.POSITIONS[bk] for sg in R.SIGNS]
SHIFT = {-1: -2, 0: 0, 1: 3}            # c_j = (A'y)_j - (Qx)_j + s_j,  b_i = (A x)_i + s_i


@dataclass
class Case:
    n: int
    m: int
    ne: int
    A: object                 # original problem, integer entries (float64 storage)
    Q: object
    c: object
    b: object
    lb: object
    ub: object
    x: object                 # the unscaled integer point, and a different one for the restart point
    y: object
    x2: object
    y2: object
    E: object
    D: object

    def reference_problem(self):
        return R.problem_from_arrays(self.A, self.c, self.b, self.lb, self.ub, self.ne, self.Q)

    def original_problem(self):
        Q = self.Q if self.Q is not None else sp.csc_matrix((self.n, self.n))
        return QuadraticProgrammingProblem(self.lb, self.ub, Q, self.c, 0.0, self.A, self.b, self.ne)

    def scaled_problem(self):
        """A_s = E^-1 A_o D^-1, Q_s = D^-1 Q_o D^-1, c_o / D, b_o / E, bounds . D: every one exact (powers of two)."""
        As = sp.csc_matrix(sp.diags(1.0 / self.E) @ self.A @ sp.diags(1.0 / self.D)) if self.m else self.A.copy()
        As = sp.csc_matrix((As.data, As.indices, As.indptr), shape=(self.m, self.n))
        Qs = sp.csc_matrix((self.n, self.n))
        if self.Q is not None:
            Qs = sp.csc_matrix(sp.diags(1.0 / self.D) @ self.Q @ sp.diags(1.0 / self.D))
        return QuadraticProgrammingProblem(self.lb * self.D, self.ub * self.D, Qs, self.c / self.D, 0.0, As,
                                           self.b / self.E, self.ne)


def _points(rng, size):
    """integers of magnitude <= 8, a third of them zero"""
    v = rng.integers(1, 9, size) * rng.choice([-1, 1], size)
    return np.where(rng.random(size) < 1.0 / 3.0, 0, v).astype(np.int64)


def _bounds_for(x, choice):
    """(lb, ub, shift of c) that land column j in pattern COLUMN_PATTERNS[choice[j]] around the point x"""
    n = len(x)
    lb, ub, shift = np.full(n, -INF), np.full(n, INF), np.zeros(n, dtype=np.int64)
    xf = x.astype(np.float64)
    for p, (bk, pos, sg) in enumerate(COLUMN_PATTERNS):
        at = choice == p
        shift[at] = SHIFT[sg]
        lo = {"below": xf + 2, "at_lb": xf, "inside": xf - 3, "at_ub": xf - 5, "above": xf - 4}[pos]
        hi = {"below": xf + 6, "at_lb": xf + 5, "inside": xf + 2, "at_ub": xf, "above": xf - 1}[pos]
        if bk == "fixed":
            hi = lo = {"below": xf + 2, "at_lb": xf, "above": xf - 1}[pos]
        if bk in ("lower", "box", "fixed"):
            lb[at] = lo[at]
        if bk in ("upper", "box", "fixed"):
            ub[at] = hi[at]
    return lb, ub, shift


def _matrix(rng, n, m, long_row):
    """A: 0, 1 or 2 entries per column, nonzero integers of magnitude <= 8; one column and one row stay empty"""
    k = rng.choice([0, 1, 2], n, p=[0.05, 0.5, 0.45]) if m >= 2 else (rng.random(n) < 0.9).astype(np.int64) * min(m, 1)
    if n >= 3:
        k[n // 2] = 0
    used = m - 1 if m >= 3 else max(m, 1)                 # m >= 3: row m // 2 stays empty
    r0 = rng.integers(0, used, n)
    r1 = (r0 + 1 + rng.integers(0, max(used - 1, 1), n)) % used       # another row than r0
    cols = np.concatenate([np.nonzero(k >= 1)[0], np.nonzero(k >= 2)[0]])
    rows = np.concatenate([r0[k >= 1], r1[k >= 2]])
    if m >= 3:
        rows = np.where(rows >= m // 2, rows + 1, rows)
    if m >= 4 * n and m >= 3:                             # a few long columns: half of the rows each, so that A x != 0 on most rows
        cols, rows = np.nonzero(rng.random((n, m)) < 0.5)
        cols, rows = cols[rows != m // 2], rows[rows != m // 2]
    vals = rng.integers(1, 9, len(rows)) * rng.choice([-1, 1], len(rows))
    if long_row:
        keep = rows != 0
        cols, rows, vals = cols[keep], rows[keep], vals[keep]
        cols = np.concatenate([cols, np.arange(long_row)])
        rows = np.concatenate([rows, np.zeros(long_row, dtype=np.int64)])
        vals = np.concatenate([vals, rng.integers(1, 9, long_row) * rng.choice([-1, 1], long_row)])
    A = sp.csc_matrix((vals.astype(np.float64), (rows, cols)), shape=(m, n))
    A.sort_indices()
    assert A.nnz == len(vals), "a duplicate entry"
    return A


def _objective_matrix(rng, n):
    """Q = B'B, B sparse with entries +-1"""
    nb = max(n // 2, 1)
    bj = np.concatenate([rng.integers(0, n, nb), rng.integers(0, n, nb // 2)])
    bi = np.concatenate([np.arange(nb), rng.choice(nb, nb // 2, replace=False) if nb >= 2 else np.zeros(0, dtype=np.int64)])
    B = sp.csc_matrix((rng.choice([-1, 1], len(bi)).astype(np.int64), (bi, bj)), shape=(nb, n))
    Q = sp.csc_matrix(B.T @ B)
    Q.eliminate_zeros()
    Q.sort_indices()
    return Q.astype(np.float64)


def make_case(n, m, ne, seed, mixed, counters, qp=False, long_row=0, without=None, shared=None):
    """``counters``: how many columns / rows each natural class (what A, x and y decide) has seen so far, shared by the
    cases of one census so that they walk through the patterns together.  ``long_row``: row 0 gets that many entries.
    ``without``: a column pattern the generator leaves out (to show that the census notices).  ``shared``: a case whose
    A, Q, E and D this one takes over (the members of a batch); the points, and so c, b and the bounds, are its own."""
    rng = np.random.default_rng(seed)
    x, y, x2, y2 = _points(rng, n), _points(rng, m), _points(rng, n), _points(rng, m)
    if n and not np.any(x != x2):
        x2[0] = x[0] + 1
    if shared is None:
        A = _matrix(rng, n, m, long_row)
        Q = _objective_matrix(rng, n) if qp else None
        E = np.exp2(rng.integers(-3, 4, m)) if mixed else np.ones(m)
        D = np.exp2(rng.integers(-3, 4, n)) if mixed else np.ones(n)
    else:
        A, Q, E, D = shared.A, shared.Q, shared.E, shared.D
    Ai = sp.csc_matrix((A.data.astype(np.int64), A.indices, A.indptr), shape=(m, n))
    ax, aty = Ai @ x, Ai.T @ y
    qx = np.zeros(n, dtype=np.int64) if Q is None else (Q @ x.astype(np.float64)).astype(np.int64)

    def walk(classes, num_classes, period, key):
        """the pattern of every element: the elements of a natural class walk through 0 .. period - 1 in turn"""
        choice = np.zeros(len(classes), dtype=np.int64)
        seen = counters.setdefault(key, np.zeros(num_classes, dtype=np.int64))
        for cl in range(num_classes):
            idx = np.nonzero(classes == cl)[0]
            choice[idx] = (seen[cl] + np.arange(len(idx))) % period
            seen[cl] += len(idx)
        return choice

    # columns: A, x and y decide (sign g_h, sign x); the generator chooses the bounds, the position and the sign of g
    choice = walk((np.sign(-aty) + 1) * 3 + np.sign(x) + 1, 9, len(COLUMN_PATTERNS), "col")
    if without is not None:
        choice = np.where(choice == COLUMN_PATTERNS.index(without), (choice + 1) % len(COLUMN_PATTERNS), choice)
    lb, ub, shift = _bounds_for(x, choice)
    c = aty - qx + shift
    # rows: A, x, y and ne decide (kind, sign(-A x), sign y); the generator chooses the sign of b - A x
    kind = (np.arange(m) < ne).astype(np.int64)
    rchoice = walk(kind * 9 + (np.sign(-ax) + 1) * 3 + np.sign(y) + 1, 18, 3, "row")
    b = ax + np.array([-2, 0, 3], dtype=np.int64)[rchoice]
    for i in (ne - 1, ne):                                # either side of the i < ne boundary: b - A x < 0, which an equality
        if 0 <= i < m:                                    # row counts and an inequality row does not
            b[i] = ax[i] - 2
    f = lambda v: v.astype(np.float64)
    return Case(n, m, ne, A, Q, f(c), f(b), lb, ub, f(x), f(y), f(x2), f(y2), E, D)


# ---- the cases: every shape at which the evaluation grid changes its walk (workgroups of 256 threads over rows and
# columns with a grid stride, ceil((n + m + 2) / 2 / 256) of them, at most 1024) ------------------------------------------
SMALL_SHAPES = [(1, 0), (1, 1), (255, 1), (256, 1), (257, 1), (1, 257), (3, 1300), (1300, 0)]
MID = (513, 511)
BIG = (400000, 130000)         # n + m > 2 * 256 * 1024: every workgroup makes more than one trip


def _variants(n, m):
    """(ne, mixed scaling): ne over 0, 1, m - 1, m (the i < ne boundary), E = D = 1 against mixed powers of two"""
    nes = sorted({0, min(1, m), max(m - 1, 0), m})
    return [(ne, mixed) for ne in nes for mixed in (False, True)]


# the largest shape: the reference takes seconds per point, so two of the eight variants -- both row kinds with mixed
# scaling, and every row an equality (ne = m) with E = D = 1; ne = 0, 1 and m - 1 are left to the smaller shapes
BIG_VARIANTS = [(BIG[1] // 2, True), (BIG[1], False)]


@functools.lru_cache(maxsize=None)
def _group(name):
    """The cases of one census, generated once with shared counters: {(n, m, ne, mixed): (case, reference words)}."""
    counters, out = {}, {}
    if name == "small":
        shapes = [s + v for s in SMALL_SHAPES for v in _variants(*s)]
    elif name == "big":
        shapes = [BIG + v for v in BIG_VARIANTS]
    else:
        shapes = [MID + v for v in _variants(*MID)]
    for seed, (n, m, ne, mixed) in enumerate(shapes):
        if name == "big" and out:
            # the first variant's data with every row an equality and E = D = 1: the census is the first variant's
            first = next(iter(out.values()))[0]
            case = dataclasses.replace(first, ne=ne, E=np.ones(m), D=np.ones(n))
        else:
            case = make_case(n, m, ne, 1000 + seed, mixed, counters, qp=(name == "mid_qp"))
        out[(n, m, ne, mixed)] = (case, _reference(case))
    return out


def _reference(case):
    """the words at the current point and at the restart point"""
    P = case.reference_problem()
    return {"P": P, CURRENT: R.words(P, case.x, case.y), RESTART: R.words(P, case.x2, case.y2)}


def census(references):
    """Every cell of the branch table is occupied by a column / row of the CURRENT points of ``references``; an empty
    column sits among the g_h == 0 cells and an empty row among the rows."""
    cols, rows = set(), set()
    empty_col = empty_row = False
    for ref in references:
        w = ref[CURRENT]
        cols.update(w.column_cells)
        rows.update(w.row_cells)
        empty_col |= any(w.column_cells[j][2] == 0 for j in w.empty_columns)
        empty_row |= bool(w.empty_rows)
    missing = sorted(R.COLUMN_CELLS - cols)
    assert not missing, f"{len(missing)} column cells are never visited, e.g. {missing[:5]}"
    missing = sorted(R.ROW_CELLS - rows)
    assert not missing, f"{len(missing)} row cells are never visited, e.g. {missing[:5]}"
    assert empty_col and empty_row


def _census_of(name):
    census([ref for _, ref in _group(name).values()])


# ---- the device side ---------------------------------------------------------------------------------------------------
def _exact(got, want, label):
    """as numbers: a zero of either sign is a zero; no tolerance"""
    got = [float(v) for v in np.atleast_1d(got)]
    want = list(want)
    assert len(got) == len(want)
    bad = [(q, g, str(w)) for q, (g, w) in enumerate(zip(got, want)) if not g == w]
    assert not bad, f"{label}: (word, device, integer reference) {bad}"


def _place(eng, case):
    """the original problem, the restart point (x2, y2) and the current point (x, y) on an engine of the scaled problem"""
    eng.set_original_problem(case.E, case.D, case.c, case.b, case.lb, case.ub)
    eng.set_current(case.x2 * case.D, case.y2 * case.E)
    eng.save_restart_point()
    eng.set_current(case.x * case.D, case.y * case.E)


def _scaled_sums(case):
    """the sums of squares of the SCALED points: (current, restart, current - restart)"""
    pts = {CURRENT: (case.x, case.y), RESTART: (case.x2, case.y2)}
    out = {p: (R.sumsq(x, case.D), R.sumsq(y, case.E)) for p, (x, y) in pts.items()}
    out["distance"] = (R.sumsq(case.x - case.x2, case.D), R.sumsq(case.y - case.y2, case.E))
    return out


def _check_riders(eng, sums, point, label):
    """what rides in the evaluation's reduction: the distances to the restart point, the sums of squares"""
    _exact(eng.distance_to_restart(CURRENT), sums["distance"], f"{label}: distance_to_restart(CURRENT)")
    _exact(eng.distance_to_restart(RESTART), (0, 0), f"{label}: distance_to_restart(RESTART)")
    _exact(eng.point_sumsq(point), sums[point], f"{label}: point_sumsq(point)")
    _exact(eng.point_sumsq(CURRENT), sums[CURRENT], f"{label}: point_sumsq(CURRENT)")


def _check_engine(eng, case, ref, label):
    _place(eng, case)
    sums = _scaled_sums(case)
    for point in (CURRENT, RESTART):
        w = eng.eval_point(point)
        _exact(w[:22], ref[point].words, f"{label}: eval_point({point})")
        _check_riders(eng, sums, point, f"{label}, after eval_point({point})")


def _ids(keys):
    return [f"{n}x{m}-ne{ne}-{'pow2' if mixed else 'unit'}" for n, m, ne, mixed in keys]


def _keys(shapes):
    return [s + v for s in shapes for v in _variants(*s)]


# PDHG_EVAL_HOST_WORD=0 (two reduction rounds) and PDHG_EVAL_PREFETCH=0 (the distances and sums of squares by their own
# launches) are selected by the environment alone: the library keeps no counter for either switch, so unlike the shard
# groups, the tiled layout, the trust-region forms, the fleet and the batch below, nothing here can prove which path ran
# (tests/test_gpu_device_eval.py, which pins the two forms to each other bit for bit, is in the same position).
FORMS = {"default": {}, "two_rounds": {"PDHG_EVAL_HOST_WORD": "0"}, "own_launches": {"PDHG_EVAL_PREFETCH": "0"}}


def _check_forms(monkeypatch, case, ref, label):
    """every form on one engine: both switches are read per call, and _check_engine sets the points anew, so that
    nothing of the previous form's results can answer"""
    eng = HipPdhgEngine.from_problem(case.scaled_problem(), device_id=0)
    for form, env in FORMS.items():
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        _check_engine(eng, case, ref, f"{label}, {form}")
        for k in env:
            monkeypatch.delenv(k)
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("key", _keys(SMALL_SHAPES), ids=_ids(_keys(SMALL_SHAPES)))
def test_one_handle_small_shapes(gpu_required, monkeypatch, key):
    _census_of("small")
    case, ref = _group("small")[key]
    _check_forms(monkeypatch, case, ref, "small")


@pytest.mark.gpu
@pytest.mark.parametrize("group", ["mid", "mid_qp"])
@pytest.mark.parametrize("key", _keys([MID]), ids=_ids(_keys([MID])))
def test_one_handle_two_blocks(gpu_required, monkeypatch, key, group):
    """513 x 511: two workgroups, the second one a partial block on both sides; as an LP and as a QP (Q = B'B: out[20],
    out[21] and the Q x term of g).  The census holds over this shape's own variants."""
    _census_of(group)
    case, ref = _group(group)[key]
    _check_forms(monkeypatch, case, ref, group)
    if group == "mid_qp":
        assert ref[CURRENT].words[20] > 0 and ref[CURRENT].words[21] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("variant", BIG_VARIANTS, ids=lambda v: f"ne{v[0]}-{'pow2' if v[1] else 'unit'}")
def test_one_handle_above_the_grid_cap(gpu_required, variant):
    """400000 x 130000: n + m > 524288, so each of the 1024 workgroups makes more than one trip on the column side.
    The census holds on the first variant alone; the second is its data with ne = m and E = D = 1."""
    _census_of("big")
    case, ref = _group("big")[BIG + variant]
    eng = HipPdhgEngine.from_problem(case.scaled_problem(), device_id=0)
    _check_engine(eng, case, ref, "big")
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("key", [(1, 1, 0, True), (1, 1, 1, False), (3, 1300, 1299, True), (257, 1, 1, True),
                                 (1300, 0, 0, True), MID + (1, True), MID + (510, False)],
                         ids=lambda k: "x".join(map(str, k[:2])) + f"-ne{k[2]}")
def test_shard_groups(gpu_required, key, world):
    """device_ids = [0, 0] and [0, 0, 0]: two reduction rounds over column slices; at 1 x 1 and 3 x 1300 a rank owns no
    column or no row."""
    group = "mid" if key[:2] == MID else "small"
    _census_of(group)
    case, ref = _group(group)[key]
    eng = HipPdhgEngine.from_problem(case.scaled_problem(), device_ids=[0] * world)
    assert eng.dist_info()["world"] == world
    _check_engine(eng, case, ref, f"world {world}")
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("world", [1, 2], ids=["one_handle", "shard_group"])
@pytest.mark.parametrize("group", ["mid", "mid_qp"])
def test_one_lit_column_and_one_lit_row(gpu_required, group, world):
    """The maxima (out[4..7], out[14..19], out[21]) of a dense point are taken over hundreds of elements of magnitude up
    to 8, so a branch that is wrong on one kind of column can hide behind the others.  Here x has ONE nonzero and y has
    ONE nonzero: every maximum is decided by that column, that row and their few neighbours in A.  The lit columns
    cover every kind of bounds with both signs of x, the lit rows both kinds with both signs of y."""
    case, ref = _group(group)[MID + (1, True)]
    cells = ref[CURRENT].column_cells
    filled = [j for j in range(case.n) if j not in set(ref[CURRENT].empty_columns)]
    lit_cols = [(j, s) for bk in R.BOUNDS for j in [j for j in filled if cells[j][0] == bk][:2] for s in (-8.0, 8.0)]
    rows = [i for i in range(case.m) if i not in set(ref[CURRENT].empty_rows)]
    lit_rows = [(i, t) for i in (0, rows[len(rows) // 2]) for t in (-8.0, 8.0)]
    assert {(cells[j][0], s) for j, s in lit_cols} == {(bk, s) for bk in R.BOUNDS for s in (-8.0, 8.0)}
    assert {(i < case.ne, t) for i, t in lit_rows} == {(k, t) for k in (True, False) for t in (-8.0, 8.0)}
    kw = {"device_id": 0} if world == 1 else {"device_ids": [0] * world}
    eng = HipPdhgEngine.from_problem(case.scaled_problem(), **kw)
    _place(eng, case)
    differing = set()
    for k, (j, s) in enumerate(lit_cols + [(0, 0.0)]):
        i, t = (lit_rows + [(0, 0.0)])[k % 5]
        x, y = np.zeros(case.n), np.zeros(case.m)
        x[j], y[i] = s, t
        want = R.words(ref["P"], x, y).words
        eng.set_current(x * case.D, y * case.E)
        _exact(eng.eval_point(CURRENT)[:22], want, f"x[{j}] = {s}, y[{i}] = {t}")
        _exact(eng.point_sumsq(CURRENT), (R.sumsq(x, case.D), R.sumsq(y, case.E)), f"x[{j}] = {s}, y[{i}] = {t}: point_sumsq")
        differing.add(tuple(want[q] for q in (5, 17, 18, 19)))
    assert len(differing) > 5          # the ray maxima do depend on which column and row is lit
    eng.close()


@pytest.mark.gpu
def test_tiled_layout(gpu_required, monkeypatch):
    """The words depend on A x and A'y of whichever product kernel serves the point: the tiled layout forced."""
    monkeypatch.setenv("PDHG_SPMV", "tiled")
    monkeypatch.setenv("PDHG_TILE_SHIFT", "6")
    _census_of("mid")
    case, ref = _group("mid")[MID + (510, True)]
    eng = HipPdhgEngine.from_problem(case.scaled_problem(), device_id=0)
    info = eng.layout_info()
    assert info["A_tiled_waves"] > 0 and info["At_tiled_waves"] > 0 and info["A_tile_shift"] == 6, info
    _check_engine(eng, case, ref, "tiled")
    eng.close()


# ---- the trust-region set-up sums: out[0] the Lagrangian value, out[3] |x|^2, out[4] |y|^2 of the SCALED point ---------
@pytest.mark.gpu
@pytest.mark.parametrize("small_eval,coop", [("1", "1"), ("0", "1"), ("0", "0")],
                         ids=["one_workgroup_kernel", "one_persistent_launch", "pass_by_pass"])
@pytest.mark.parametrize("group", ["mid", "mid_qp"])
def test_trust_region_setup_sums(gpu_required, monkeypatch, group, small_eval, coop):
    """E = D = 1, so the scaled problem is the integer problem itself and wp = 2, wd = 1/2 keep every term of the
    set-up pass exact.  Radius 0; nothing else of the call is asserted here."""
    monkeypatch.setenv("PDHG_SMALL_EVAL", small_eval)
    monkeypatch.setenv("PDHG_TR_COOP", coop)
    case, ref = _group(group)[MID + (1, False)]
    assert np.all(case.E == 1.0) and np.all(case.D == 1.0)
    eng = HipPdhgEngine.from_problem(case.scaled_problem(), device_id=0)
    _place(eng, case)
    for point, (x, y) in ((CURRENT, (case.x, case.y)), (RESTART, (case.x2, case.y2))):
        want = [R.lagrangian(ref["P"], x, y), R.sumsq(x), R.sumsq(y)]
        for rng in (0, 1, 2):
            for approximate in (False, True):
                out = eng.trust_region_bound(point, 2.0, 0.5, 0.0, rng, approximate)
                _exact(out[[0, 3, 4]], want, f"point {point}, range {rng}, approximate {approximate}")
    assert (eng.layout_info()["tr_coop_calls"] > 0) == (small_eval == "0" and coop == "1")
    eng.close()


# ---- a fleet: members of different shapes in one call ------------------------------------------------------------------
def _fleet_cases():
    """(name, case, carried by the shared launch?) -- n + m == 4096 against 4097, a row of 256 entries against 257"""
    counters = {}
    mk = lambda n, m, ne, seed, **kw: make_case(n, m, ne, seed, True, counters, **kw)
    return [("2048x2048", mk(2048, 2048, 1000, 1, ), True),
            ("2049x2048", mk(2049, 2048, 2047, 2), False),
            ("row256", mk(300, 40, 0, 3, long_row=256), True),
            ("row257", mk(300, 40, 40, 4, long_row=257), False),
            ("1x1", mk(1, 1, 1, 5), True),
            ("513x511", mk(513, 511, 1, 6), True),
            ("qp", mk(60, 50, 25, 7, qp=True), None)]      # carried only with PDHG_SMALL_QP=1


@pytest.mark.gpu
@pytest.mark.parametrize("small_qp", ["0", "1"], ids=["qp_on_its_own", "qp_carried"])
def test_fleet_eval_points(gpu_required, monkeypatch, small_qp):
    monkeypatch.setenv("PDHG_SMALL_QP", small_qp)
    members = _fleet_cases()
    refs = [_reference(case) for _, case, _ in members]
    census(refs)
    carried = [small_qp == "1" if c is None else c for _, _, c in members]
    fleet = HipPdhgFleet.from_problems([case.scaled_problem() for _, case, _ in members], device_id=0)
    for eng, (_, case, _) in zip(fleet.members, members):
        _place(eng, case)
    K = len(members)
    for point in (CURRENT, RESTART):
        # member by member (the others -1): carried by the shared launch, or served by its own call
        for k, (name, case, _) in enumerate(members):
            only = np.full(K, -1, dtype=np.int32)
            only[k] = point
            rows = fleet.eval_points(only)
            info = fleet.check_info()
            assert (info["carried"], info["single"]) == ((1, 0) if carried[k] else (0, 1)), (name, info)
            _exact(rows[k][:22], refs[k][point].words, f"fleet member {name} alone: eval_points({point})")
            fleet.members[k].set_current(None, None)      # the state moves: the next call evaluates again
        # all members in one call
        launches = fleet.check_info()["check_launches"]
        rows = fleet.eval_points(point)
        info = fleet.check_info()
        assert info["check_launches"] > launches, info
        assert info["carried"] == sum(carried) and info["single"] == K - sum(carried), info
        for eng, row, ref, (name, case, _) in zip(fleet.members, rows, refs, members):
            _exact(row[:22], ref[point].words, f"fleet member {name}: eval_points({point})")
            _check_riders(eng, _scaled_sums(case), point, f"fleet member {name}, after eval_points({point})")
    fleet.close()


# ---- a batch: members share A_o, E and D and differ in c, b, the bounds and the point -----------------------------------
BATCH_SHAPE = (3000, 1500, 750)     # n, m, ne: enough columns for every member to fill the 405 column cells on its own


def _batch_cases(K):
    """K cases on one matrix, E and D; each member has its own points and so its own c, b and bounds, steered by its
    own counters into every cell of the table"""
    n, m, ne = BATCH_SHAPE
    base = make_case(n, m, ne, 77, True, {})
    return [base] + [make_case(n, m, ne, 500 + k, True, {}, shared=base) for k in range(1, K)]


@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 3])
def test_batch_eval_points(gpu_required, K):
    cases = _batch_cases(K)
    refs = [_reference(case) for case in cases]
    for ref in refs:
        census([ref])                                     # each member has its own census
    assert all(c.A is cases[0].A for c in cases) and any(np.any(c.c != cases[0].c) for c in cases[1:]) == (K > 1)
    problems = [case.scaled_problem() for case in cases]
    batch = HipPdhgBatch.from_problems(problems, device_id=0)
    for eng, case in zip(batch.members, cases):
        _place(eng, case)
    for point in (CURRENT, RESTART):
        before = batch.check_info()
        rows = batch.eval_points(point)
        info = batch.check_info()
        assert info["carried"] - before["carried"] == K and info["misses"] == before["misses"], (before, info)
        for k, (eng, row, ref, case) in enumerate(zip(batch.members, rows, refs, cases)):
            _exact(row[:22], ref[point].words, f"batch member {k} of {K}: eval_points({point})")
            _check_riders(eng, _scaled_sums(case), point, f"batch member {k} of {K}, after eval_points({point})")
    batch.close()
