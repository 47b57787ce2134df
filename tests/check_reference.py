"""The 22 raw words of ``pdhg_eval_point`` (include/pdhg_hip.h) in plain Python integers.

Written from the reference's own definitions -- compute_primal_residual, compute_reduced_costs_from_primal_gradient,
compute_dual_stats, compute_convergence_information and compute_infeasibility_information
(iteration_stats_utils.jl:30-63, 128-148, 157-197, 228-349) and the primal gradient Q x + c - A'y
(saddle_point.jl:1093-1100) -- element by element, with ``int`` / ``fractions.Fraction`` for every finite number and
``math.inf`` for a missing bound.  Nothing is imported from the package's evaluation code.

The problem is the ORIGINAL (unscaled) one and the point the unscaled point; all entries are integers, so every word is
an integer (or a Fraction for Fraction input) and a floating-point evaluation in any order must give exactly that number
as long as every sum of magnitudes stays below 2^53 -- which ``words`` asserts on its own integers.

Beside the words, ``words`` returns for every column and every row the CELL of the branch table it falls in:

* column: (bounds, sign g, sign g_h, position, sign x) with bounds in BOUNDS, position in POSITIONS[bounds];
* row:    (kind, sign(b - A x), sign(-A x), sign y) with kind "eq" / "ineq".
"""
import math
from dataclasses import dataclass, field
from fractions import Fraction
from itertools import product

INF = math.inf
LIMIT = 2 ** 53

BOUNDS = ("free", "lower", "upper", "box", "fixed")
POSITIONS = {"free": ("inside",),
             "lower": ("below", "at_lb", "inside"),
             "upper": ("inside", "at_ub", "above"),
             "box": ("below", "at_lb", "inside", "at_ub", "above"),
             "fixed": ("below", "at_lb", "above")}        # lb == ub: at_lb is at_ub
SIGNS = (-1, 0, 1)
COLUMN_CELLS = frozenset((bk, sg, sgh, pos, sx) for bk in BOUNDS for pos in POSITIONS[bk]
                         for sg, sgh, sx in product(SIGNS, SIGNS, SIGNS))
ROW_CELLS = frozenset(product(("eq", "ineq"), SIGNS, SIGNS, SIGNS))


def sign(v):
    return (v > 0) - (v < 0)


def _num(v):
    """A finite entry as an int (or Fraction), an infinite one as +-math.inf."""
    if isinstance(v, (int, Fraction)):
        return v
    if type(v) is float and v.is_integer():
        return int(v)
    f = float(v)
    if math.isinf(f):
        return f
    if f == int(f):
        return int(f)
    return Fraction(f)            # exact: a double is a dyadic rational


@dataclass
class Problem:
    """cols[j]: the entries (row, value) of column j of A; qcols likewise for Q (None: an LP)."""
    n: int
    m: int
    ne: int
    cols: list
    c: list
    b: list
    lb: list
    ub: list
    qcols: list = None
    objective_constant: object = 0


def problem_from_arrays(A_csc, c, b, lb, ub, ne, Q_csc=None, objective_constant=0):
    """From a scipy CSC matrix (or anything with shape / indptr / indices / data) and vectors."""
    m, n = (int(s) for s in A_csc.shape)

    def columns(M):
        ptr, idx, val = M.indptr.tolist(), M.indices.tolist(), [_num(v) for v in M.data.tolist()]
        return [list(zip(idx[ptr[j]:ptr[j + 1]], val[ptr[j]:ptr[j + 1]])) for j in range(len(ptr) - 1)]

    qcols = None
    if Q_csc is not None and Q_csc.nnz > 0:
        qcols = columns(Q_csc)
    vec = lambda v: [_num(t) for t in (v.tolist() if hasattr(v, "tolist") else v)]
    return Problem(n, m, int(ne), columns(A_csc), vec(c), vec(b), vec(lb), vec(ub), qcols, _num(objective_constant))


@dataclass
class Words:
    words: list                      # 22 numbers, the layout of pdhg_eval_point
    column_cells: list
    row_cells: list
    empty_columns: list = field(default_factory=list)
    empty_rows: list = field(default_factory=list)


def _reduced(grad, lb, ub):
    """(reduced cost, its contribution bound * rc to the dual objective) of one column   iteration_stats_utils.jl:93-148"""
    bound = lb if grad > 0 else ub
    rc = grad if abs(bound) != INF else 0
    contrib = 0
    if rc != 0:
        contrib = (lb if rc > 0 else ub) * rc      # finite by construction of rc
    return rc, contrib


def words(P, x, y):
    x = [_num(v) for v in (x.tolist() if hasattr(x, "tolist") else x)]
    y = [_num(v) for v in (y.tolist() if hasattr(y, "tolist") else y)]
    n, m, ne = P.n, P.m, P.ne
    assert len(x) == n and len(y) == m and 0 <= ne <= m
    # the three products, each with its sum of magnitudes
    ax, ax_mag = [0] * m, [0] * m
    aty, aty_mag = [0] * n, [0] * n
    row_nnz = [0] * m
    for j, col in enumerate(P.cols):
        xj = x[j]
        s = mag = 0
        for i, a in col:
            t = a * xj
            ax[i] += t
            ax_mag[i] += abs(t)
            row_nnz[i] += 1
            t = a * y[i]
            s += t
            mag += abs(t)
        aty[j], aty_mag[j] = s, mag
    qx, qx_mag = [0] * n, [0] * n
    if P.qcols is not None:
        for j, col in enumerate(P.qcols):
            for i, q in col:
                t = q * x[j]
                qx[i] += t
                qx_mag[i] += abs(t)
    biggest = max([0] + ax_mag + aty_mag + qx_mag)

    # (plain local accumulators: the largest case has half a million elements.  Sums of squares are their own sums of
    #  magnitudes; the signed sums s2, s9, s11, s13, s20 keep theirs in g2, g9, g11, g13, g20.)
    row_cells, col_cells = [], []
    # rows: compute_primal_residual of the problem and of the homogeneous one (b = 0), the duals' sign constraint
    s0 = s1 = s2 = s3 = g2 = 0
    m4 = m5 = m6 = m7 = 0
    b_ = P.b
    for i in range(m):
        bi, yo = b_[i], y[i]
        rh = -ax[i]
        r = bi + rh
        if i < ne:
            viol, violh, dres, kind = r, rh, 0, "eq"
        else:
            viol, violh, dres, kind = (r if r > 0 else 0), (rh if rh > 0 else 0), (-yo if yo < 0 else 0), "ineq"
        t = bi * yo
        s0 += viol * viol; s1 += yo * yo; s2 += t; g2 += abs(t); s3 += dres * dres
        t = abs(viol)
        if t > m4: m4 = t
        t = abs(violh)
        if t > m5: m5 = t
        t = abs(yo)
        if t > m6: m6 = t
        if dres > m7: m7 = dres
        t = abs(bi) + ax_mag[i]
        if t > biggest: biggest = t
        row_cells.append((kind, sign(r), sign(rh), sign(yo)))
    # columns: reduced costs of g = Q x + c - A'y and of g_h = -A'y (the c = 0, Q = 0 problem), bound violations
    s8 = s9 = s10 = s11 = s12 = s13 = s20 = g9 = g11 = g13 = g20 = 0
    m14 = m15 = m16 = m17 = m18 = m19 = m21 = 0
    for j in range(n):
        lb, ub, xo, cj, qxj = P.lb[j], P.ub[j], x[j], P.c[j], qx[j]
        lbf, ubf = lb != -INF, ub != INF
        assert lb != INF and ub != -INF and (not (lbf and ubf) or lb <= ub)
        g = qxj + cj - aty[j]
        gh = -aty[j]
        rc, contrib = _reduced(g, lb, ub)
        rch, contribh = _reduced(gh, lb, ub)
        resid, residh = g - rc, gh - rch
        lv = lb - xo if lbf and lb > xo else 0
        uv = xo - ub if ubf and xo > ub else 0
        # the homogeneous primal: finite bounds become 0, so a negative x violates a finite lb, a positive x a finite ub
        rayv = -xo if lbf and xo < 0 else (xo if ubf and xo > 0 else 0)
        t11, t20 = cj * xo, xo * qxj
        s8 += resid * resid; s9 += contrib; g9 += abs(contrib); s10 += xo * xo; s11 += t11; g11 += abs(t11)
        s12 += lv * lv + uv * uv; s13 += contribh; g13 += abs(contribh); s20 += t20; g20 += abs(t20)
        t = abs(resid)
        if t > m14: m14 = t
        t = abs(xo)
        if t > m15: m15 = t
        if lv > m16: m16 = lv
        if uv > m16: m16 = uv
        t = abs(residh)
        if t > m17: m17 = t
        t = abs(rch)
        if t > m18: m18 = t
        if rayv > m19: m19 = rayv
        t = abs(qxj)
        if t > m21: m21 = t
        t = qx_mag[j] + abs(cj) + aty_mag[j]
        if t > biggest: biggest = t
        if lbf and ubf:
            bk = "fixed" if lb == ub else "box"
        else:
            bk = "lower" if lbf else ("upper" if ubf else "free")
        if lbf and xo < lb:
            pos = "below"
        elif ubf and xo > ub:
            pos = "above"
        elif lbf and xo == lb:
            pos = "at_lb"
        elif ubf and xo == ub:
            pos = "at_ub"
        else:
            pos = "inside"
        col_cells.append((bk, sign(g), sign(gh), pos, sign(xo)))
    out = [s0, s1, s2, s3, m4, m5, m6, m7, s8, s9, s10, s11, s12, s13, m14, m15, m16, m17, m18, m19, s20, m21]
    biggest = max([biggest, g2, g9, g11, g13, g20] + [abs(v) for v in out])
    assert biggest < LIMIT, f"a sum of magnitudes reaches {biggest} >= 2^53: the words are not exact in floating point"
    return Words(out, col_cells, row_cells, [j for j, col in enumerate(P.cols) if not col],
                 [i for i in range(m) if row_nnz[i] == 0])


def sumsq(v, scale=None, denominator=8):
    """sum (v_k scale_k)^2 as an exact number (pdhg_point_sumsq / pdhg_distance_to_restart on the scaled point).  Every
    v_k scale_k must be a multiple of 1 / denominator: the sum is taken over the integers v_k scale_k denominator
    (in int64, vector at a time: these vectors have up to half a million entries)."""
    import numpy as np
    q = np.asarray(v, dtype=np.float64) * (1.0 if scale is None else np.asarray(scale, dtype=np.float64)) * float(denominator)
    assert np.all(q == np.rint(q)), "not a multiple of 1 / denominator"
    assert q.size < 2 ** 22 and (q.size == 0 or np.abs(q).max() < 2 ** 20)       # the int64 sum cannot overflow
    total = int(np.sum(q.astype(np.int64) ** 2))
    assert total < LIMIT
    return Fraction(total, denominator * denominator)


def lagrangian(P, x, y):
    """0.5 x'Qx + c'x - x'A'y + y'b (out[0] of pdhg_trust_region_bound: without the objective constant)."""
    x = [_num(v) for v in (x.tolist() if hasattr(x, "tolist") else x)]
    y = [_num(v) for v in (y.tolist() if hasattr(y, "tolist") else y)]
    total = mag = 0
    for j, col in enumerate(P.cols):
        for i, a in col:
            total -= x[j] * a * y[i]
            mag += abs(x[j] * a * y[i])
        total += P.c[j] * x[j]
        mag += abs(P.c[j] * x[j])
    for i in range(P.m):
        total += P.b[i] * y[i]
        mag += abs(P.b[i] * y[i])
    xqx = 0
    if P.qcols is not None:
        for j, col in enumerate(P.qcols):
            for i, q in col:
                xqx += x[i] * q * x[j]
                mag += abs(x[i] * q * x[j])
    assert mag < LIMIT
    return Fraction(xqx, 2) + total


def _norm2(v):
    return math.sqrt(sum(t * t for t in v))


def information(P, w, eps_ratio=1.0):
    """(ConvergenceInformation fields, InfeasibilityInformation fields) as dicts of floats from the 22 words ``w`` of
    one point: compute_convergence_information at that point and compute_infeasibility_information with that point as
    both rays (iteration_stats_utils.jl:228-349)."""
    w = [float(v) for v in w]
    ci = {}
    ci["primal_objective"] = float(P.objective_constant) + w[11] + 0.5 * w[20]
    ci["l_inf_primal_residual"] = max(w[4], w[16])
    ci["l2_primal_residual"] = math.sqrt(w[0] + w[12])
    b_inf = max([0] + [abs(t) for t in P.b])
    c_inf = max([0] + [abs(t) for t in P.c])
    ci["relative_l_inf_primal_residual"] = ci["l_inf_primal_residual"] / (eps_ratio + b_inf)
    ci["relative_l2_primal_residual"] = ci["l2_primal_residual"] / (eps_ratio + _norm2(P.b))
    ci["l_inf_primal_variable"] = w[15]
    ci["l2_primal_variable"] = math.sqrt(w[10])
    ci["dual_objective"] = (w[2] + float(P.objective_constant) - 0.5 * w[20]) + w[9]
    ci["l_inf_dual_residual"] = max(w[7], w[14])
    ci["l2_dual_residual"] = math.sqrt(w[3] + w[8])
    ci["relative_l_inf_dual_residual"] = ci["l_inf_dual_residual"] / (eps_ratio + c_inf)
    ci["relative_l2_dual_residual"] = ci["l2_dual_residual"] / (eps_ratio + _norm2(P.c))
    ci["l_inf_dual_variable"] = w[6]
    ci["l2_dual_variable"] = math.sqrt(w[1])
    ci["corrected_dual_objective"] = ci["dual_objective"] if ci["l_inf_dual_residual"] == 0.0 else -INF
    gap = abs(ci["primal_objective"] - ci["dual_objective"])
    ci["relative_optimality_gap"] = gap / (eps_ratio + abs(ci["primal_objective"]) + abs(ci["dual_objective"]))
    ii = {}
    s = w[15] if w[15] != 0.0 else 1.0
    ii["max_primal_ray_infeasibility"] = max(w[5], w[19]) / s
    ii["primal_ray_linear_objective"] = w[11] / s
    ii["primal_ray_quadratic_norm"] = w[21] / s
    scaling = max(w[6], w[18])
    ii["max_dual_ray_infeasibility"] = max(w[7], w[17]) / scaling if scaling != 0.0 else 0.0
    ii["dual_ray_objective"] = (w[2] + w[13]) / scaling if scaling != 0.0 else 0.0
    return ci, ii
