"""primal_kernel reads lb / ub as "default + exceptions" (csrc/vector_kernels.hpp: BoundView) -- CONST: one bit pattern,
nothing read; SPARSE: a default, a mask bit per column, an exception count per 128-column block and the packed
exceptions; DENSE: the arrays.  The dense arrays stay the authority and the views are derived from them by every writer
(create, rescale).  Whatever the mode the clamp must see the operand a dense read gives it: x' and xbar bitwise the
oracle's and bitwise the same engine's under PDHG_BOUNDS=dense, at the sizes where the block / mask-word / pair / odd-tail
arithmetic can go wrong, for every mode of either vector, before and after a rescale.

xbar has no getter: it is observed through y' = y + sigma (b - A xbar) with a matrix that has an entry in EVERY column
and equality rows only (no projection that could hide a wrong operand).  Both launch paths that carry the compact views
run: separate launches (launch_primal) and the trial graph's primal node."""
import numpy as np
import pytest
import scipy.sparse as sp

from firstorderlp_jl_amd import HipPdhgEngine, linear_programming_problem
from firstorderlp_jl_amd.primal_dual_hybrid_gradient import AdaptiveStepsizeParams, PdhgSolverState, take_step
from oracle.oracle import OracleState
from tests import helpers as H

pytestmark = pytest.mark.gpu

INF = np.inf
SIZES = [1, 2, 127, 128, 129, 255, 257, 1000, 4097]
PATHS = {"plain": {"PDHG_GRAPH": "0"}, "graph": {"PDHG_GRAPH": "1", "PDHG_COOP": "0"}}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _lp(n, lb, ub, seed):
    """m = ceil(n / 2) equality rows of (up to) 3 entries: row i holds columns 2i, 2i + 1 and a random one, so every column
    has an entry."""
    rng = np.random.default_rng(seed)
    m = (n + 1) // 2
    rows = np.repeat(np.arange(m), 3)
    cols = np.stack([(2 * np.arange(m)) % n, (2 * np.arange(m) + 1) % n, rng.integers(0, n, m)], axis=1).reshape(-1)
    A = sp.coo_matrix((rng.standard_normal(3 * m), (rows, cols)), shape=(m, n)).tocsc()
    A.sum_duplicates()
    A.sort_indices()
    assert (np.diff(A.indptr) > 0).all()
    return linear_programming_problem(lb, ub, rng.standard_normal(n), 0.0, A, rng.standard_normal(m), m)


def _patterns(n, seed):
    """name -> (lb, ub); lb <= ub everywhere."""
    rng = np.random.default_rng(seed)
    inf_ub = np.full(n, INF)

    def finite_ub(share):
        ub = inf_ub.copy()
        k = int(round(share * n))
        ub[rng.choice(n, size=k, replace=False)] = 4.0 + rng.random(k)
        return ub
    tail_ub = inf_ub.copy()                       # exceptions only in the last (partial) block of 128 columns, at most n / 4
    tail0 = ((n - 1) // 128) * 128
    k = max(1, min(n - tail0, n // 4))
    tail_ub[n - k:] = 5.0 + rng.random(k)
    out = {
        "lb 0 / ub inf": (np.zeros(n), inf_ub),
        "lb -inf / ub 20%": (np.full(n, -INF), finite_ub(0.2)),
        "lb 3.5 / ub 30%": (np.full(n, 3.5), finite_ub(0.3)),
        "lb -0.0 / ub last block": (np.full(n, -0.0), tail_ub),
    }
    for k, col in enumerate(sorted({c for c in (0, 63, 64, 127, 128, n - 1) if c < n})):
        lb = np.zeros(n)
        lb[col] = -1.25
        out[f"lb 0 but column {col} / ub {'inf' if k % 2 else '20%'}"] = (lb, inf_ub if k % 2 else finite_ub(0.2))
    return out


def _expected_view(v):
    """The rule of the issue, restated on the host: the default is the most frequent of the bit patterns of the first entry,
    +inf, -inf and +0.0; no exception: const; at most a quarter: sparse; else dense (which reports no exceptions).  A tie
    between candidates leaves at least half of the entries as exceptions, i.e. dense whichever wins."""
    b = _bits(v)
    cand = [b[0], _bits(np.array([INF]))[0], _bits(np.array([-INF]))[0], np.uint64(0)]
    nexc = len(b) - max(int((b == c).sum()) for c in cand)
    if nexc == 0:
        return "const", 0
    return ("sparse", nexc) if 4 * nexc <= len(b) else ("dense", 0)


def _device_matrix(eng, A):
    """The matrix as it stands on the device (after a rescale its entries are not reproducible on the host bit for bit):
    A e_S for sets S of columns no two of which share a row gives the entries of those columns exactly."""
    A = sp.csc_matrix(A)
    m, n = A.shape
    Ar = A.tocsr()
    colour = np.full(n, -1)
    for j in range(n):
        taken = set()
        for r in A.indices[A.indptr[j]:A.indptr[j + 1]]:
            taken.update(colour[Ar.indices[Ar.indptr[r]:Ar.indptr[r + 1]]].tolist())
        c = 0
        while c in taken:
            c += 1
        colour[j] = c
    data = np.empty_like(A.data)
    for c in range(colour.max() + 1):
        sel = colour == c
        v = eng.spmv(sel.astype(np.float64))
        for j in np.nonzero(sel)[0]:
            data[A.indptr[j]:A.indptr[j + 1]] = v[A.indices[A.indptr[j]:A.indptr[j + 1]]]
    return sp.csc_matrix((data, A.indices.copy(), A.indptr.copy()), shape=(m, n))


def _oracle(eng, A):
    c, b, lb, ub = eng.get_problem_vectors()
    m, n = A.shape
    return OracleState(m, n, A.indptr, A.indices, A.data, c, b, lb, ub, m), lb, ub


def _checks(eng, A, x0, y0, step, pw, label):
    """The issue's per-case checks from the state (x0, y0) against an oracle built from the device's own vectors.  Returns
    every array read from the device, for the comparison with the engine that reads the bounds densely."""
    o, lb, ub = _oracle(eng, A)
    o.exact_sums = True
    eng.reset_average()
    eng.set_current(x0, y0)
    o.x, o.y = x0, y0
    o.recompute_dual_product()
    assert np.array_equal(_bits(eng.get_dual_product()), _bits(o.aty)), label + ": A'y of the start"
    seen = []
    eng.trial_primal(step, pw)
    gx = eng.get_trial()[0]
    assert np.array_equal(_bits(gx), _bits(o.trial_primal(step, pw))), label + ": x' (trial_primal)"
    seen.append(gx)
    raw = eng.trial_step(step, pw, 1.0)
    want_raw, wx, wy, wa = o.trial_step(step, pw, 1.0)
    gx, gy, ga = eng.get_trial()
    assert np.array_equal(_bits(gx), _bits(wx)), label + ": x'"
    assert np.array_equal(_bits(gy), _bits(wy)), label + ": y' (xbar through A xbar)"
    assert np.array_equal(_bits(ga), _bits(wa)), label + ": A'y'"
    assert np.array_equal(_bits(raw[:4]), _bits(want_raw[:4])), label + ": sums"
    seen += [gx, gy, ga, np.array(raw)]
    # three accepted take_steps: the second and third primal_kernel carry the deferred sum_x update
    st = PdhgSolverState(eng, step_size=step, primal_weight=pw, ratio_step_sizes=1.0)
    o.step_size, o.primal_weight, o.ratio_step_sizes = step, pw, 1.0
    for _ in range(3):
        take_step(AdaptiveStepsizeParams(0.3, 0.6), st)
        o.take_step_adaptive(0.3, 0.6)
    assert st.total_number_iterations == o.total_number_iterations, label + ": decisions"
    xa, ya = eng.get_average()
    wxa, wya = o.compute_average()
    assert np.array_equal(_bits(xa), _bits(wxa)) and np.array_equal(_bits(ya), _bits(wya)), label + ": average"
    seen += [xa, ya, np.concatenate(eng.get_current())]
    o.close()
    return seen


def _modes(eng, label):
    info = eng.layout_info()
    _, _, lb, ub = eng.get_problem_vectors()
    for k, v in (("lb", lb), ("ub", ub)):
        assert (info[k + "_mode"], info[k + "_exceptions"]) == _expected_view(v), f"{label}: {k} {info[k + '_mode']}"
    return info


def _script(p, x0, y0, label, rescale, expect=None):
    eng = HipPdhgEngine.from_problem(p)
    A = p.constraint_matrix
    step, pw = H.initial_step_and_weight(p)
    info = _modes(eng, label) if expect is None else eng.layout_info()
    if expect is not None:
        assert (info["lb_mode"], info["ub_mode"]) == expect, label
    seen = _checks(eng, A, x0, y0, step, pw, label)
    infos = [info]
    if rescale:
        # a trial graph built before the rescale must not keep the views of the arrays as they were
        eng.rescale(10, True, 1.0)
        info = _modes(eng, label + ", rescaled") if expect is None else eng.layout_info()
        if expect is not None:
            assert (info["lb_mode"], info["ub_mode"]) == expect, label
        Ad = _device_matrix(eng, A)
        seen += _checks(eng, Ad, x0, y0, 1.0 / np.abs(Ad.data).max(), pw, label + ", rescaled")
        infos.append(info)
    eng.close()
    return seen, infos


@pytest.mark.parametrize("path", sorted(PATHS))
@pytest.mark.parametrize("n", SIZES)
def test_compact_bounds_are_bitwise_the_dense_read(gpu_required, monkeypatch, n, path):
    for k, v in PATHS[path].items():
        monkeypatch.setenv(k, v)
    rescale = n in (1000, 4097)
    rng = np.random.default_rng(n)
    for name, (lb, ub) in _patterns(n, seed=n).items():
        label = f"n = {n}, {name}, {path}"
        p = _lp(n, lb, ub, seed=n + 1)
        m = p.constraint_matrix.shape[0]
        x0, y0 = rng.standard_normal(n), rng.standard_normal(m)
        monkeypatch.delenv("PDHG_BOUNDS", raising=False)
        seen, infos = _script(p, x0, y0, label, rescale)
        # what the patterns are there for (a case that silently ran DENSE would prove nothing)
        before = (infos[0]["lb_mode"], infos[0]["ub_mode"])
        if name == "lb 0 / ub inf":
            assert all((i["lb_mode"], i["ub_mode"]) == ("const", "const") for i in infos), label
        if name == "lb 3.5 / ub 30%" and n >= 127:
            assert before == ("const", "dense"), label
        if name == "lb -inf / ub 20%" and n >= 127:
            assert all((i["lb_mode"], i["ub_mode"]) == ("const", "sparse") for i in infos), label
            assert infos[-1]["ub_exceptions"] == infos[0]["ub_exceptions"] == int(np.isfinite(ub).sum()), label
        if name == "lb -0.0 / ub last block" and n >= 127:
            assert before == ("const", "sparse"), label
        if name.startswith("lb 0 but column") and n >= 127:
            assert all(i["lb_mode"] == "sparse" and i["lb_exceptions"] == 1 for i in infos), label
        monkeypatch.setenv("PDHG_BOUNDS", "dense")
        dense, _ = _script(p, x0, y0, label + ", PDHG_BOUNDS=dense", rescale, expect=("dense", "dense"))
        assert len(seen) == len(dense)
        for a, b in zip(seen, dense):
            assert np.array_equal(_bits(a), _bits(b)), label + ": differs from the dense read"
