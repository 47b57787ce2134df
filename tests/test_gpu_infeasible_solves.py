"""optimize() to a ray: solves that end PRIMAL_INFEASIBLE or DUAL_INFEASIBLE with everything on the device, against the
host path (the CPU oracle engine) and against the certificate itself, recomputed in numpy from the returned point alone
-- independently of both evaluators (iteration_stats_utils.jl:228-349, termination.jl:198-227).  Then the same problems as
members of a fleet and of a batch: a member that ends on a ray must not disturb the others.  Iteration counts are not
compared (the two paths reduce in different orders)."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from firstorderlp_jl_amd import optimize_batch, optimize_many
from firstorderlp_jl_amd.generators import random_lp
from firstorderlp_jl_amd.primal_dual_hybrid_gradient import optimize
from firstorderlp_jl_amd.quadratic_programming import QuadraticProgrammingProblem
from tests.oracle_engine import OracleEngine
from tests.test_gpu_end_to_end import _params

INF = np.inf
TOL, LIMIT = 1e-6, 40000          # the iteration limit leaves a factor of three over the slowest host solve (12 840)


def _problem(lb, ub, c, A, b, ne, Q=None):
    n = len(c)
    Q = sp.csc_matrix((n, n)) if Q is None else sp.csc_matrix(sp.diags(np.asarray(Q, dtype=np.float64)))
    return QuadraticProgrammingProblem(lb, ub, Q, c, 0.0, sp.csc_matrix(np.asarray(A, dtype=np.float64).reshape(len(b), n)), b, ne)


def _chain(n):
    """the rows x_i - x_{i+1} = 0"""
    A = np.zeros((n - 1, n))
    A[np.arange(n - 1), np.arange(n - 1)] = 1.0
    A[np.arange(n - 1), np.arange(1, n)] = -1.0
    return A


def _unb3(Q=None):
    """min -x1 + 0.5 x3,  x1 - x2 = 0,  x2 - x3 >= -2,  x1 free, x2 >= 0, 0 <= x3 <= 5: unbounded along (1, 1, 0)"""
    return _problem([-INF, 0.0, 0.0], [INF, INF, 5.0], [-1.0, 0.0, 0.5], [[1.0, -1.0, 0.0], [0.0, 1.0, -1.0]], [0.0, -2.0], 1, Q)


def _chain30():
    c = np.zeros(30); c[0], c[-1] = -1.0, 0.5
    lb = np.zeros(30); lb[0] = -INF
    return _problem(lb, np.full(30, INF), c, _chain(30), np.zeros(29), 29)


def _infeas_chain30():
    lb = np.zeros(30); lb[0] = 2.0
    ub = np.full(30, INF); ub[-1] = 1.0
    return _problem(lb, ub, np.ones(30), _chain(30), np.zeros(29), 29)


def _boxed_chain30():
    c = np.zeros(30); c[0], c[-1] = -1.0, 0.5
    return _problem(np.zeros(30), np.ones(30), c, _chain(30), np.zeros(29), 29)


# name -> (problem, the outcome of the host path)
PROBLEMS = {
    "unb3": (_unb3, "DUAL_INFEASIBLE"),
    "unb3_qp": (lambda: _unb3([0.0, 0.0, 2.0]), "DUAL_INFEASIBLE"),        # the ray lies in Q's null space
    "curved_qp": (lambda: _unb3([1.0, 0.0, 0.0]), "OPTIMAL"),              # curvature along the ray: primal_ray_quadratic_norm vetoes
    "chain30": (_chain30, "DUAL_INFEASIBLE"),
    "infeas_chain30": (_infeas_chain30, "PRIMAL_INFEASIBLE"),
    # a pair that ends at the first check
    "trivial_unbounded": (lambda: _problem([0.0, 0.0], [INF, INF], [-1.0, -1.0], [[-1.0, 1.0]], [-1.0], 0), "DUAL_INFEASIBLE"),
    "trivial_infeasible": (lambda: _problem([0.0, 0.0], [1.0, 1.0], [0.0, 0.0], [[1.0, 1.0]], [3.0], 1), "PRIMAL_INFEASIBLE"),
}


@functools.lru_cache(maxsize=None)
def _host(name):
    return optimize(_params(TOL, LIMIT), PROBLEMS[name][0](), OracleEngine.from_problem)


@functools.lru_cache(maxsize=None)
def _device(name):
    return optimize(_params(TOL, LIMIT), PROBLEMS[name][0]())


def check_certificate(p, out, criteria):
    """The certificate of ``out.termination_string`` from ``out``'s point and the problem, in numpy."""
    A = sp.csr_matrix(p.constraint_matrix)
    absA = abs(A)
    ne = p.num_equalities
    lbf, ubf = np.isfinite(p.variable_lower_bound), np.isfinite(p.variable_upper_bound)
    u = 64.0 * 2.0 ** -53
    if out.termination_string == "DUAL_INFEASIBLE":
        x = np.asarray(out.primal_solution)
        r = x / np.abs(x).max()
        slope = float(p.objective_vector @ r)
        assert slope < 0.0, slope
        eps = criteria.eps_dual_infeasible
        allowance = u * float((absA @ np.abs(r)).max(initial=0.0))            # the rounding of A r in this recomputation
        assert np.abs(p.objective_matrix @ r).max(initial=0.0) / -slope <= eps
        act = A @ r
        rows = np.concatenate([np.abs(act[:ne]), np.maximum(-act[ne:], 0.0)])
        ray_bounds = np.maximum(np.where(lbf, np.maximum(-r, 0.0), 0.0), np.where(ubf, np.maximum(r, 0.0), 0.0))
        worst = max(rows.max(initial=0.0), ray_bounds.max(initial=0.0))
        assert worst / -slope <= eps + allowance / -slope, (worst, slope)
    elif out.termination_string == "PRIMAL_INFEASIBLE":
        # Farkas: y with y_ineq >= 0, reduced costs of -A'y only where the bound they price is finite, and a positive
        # dual ray objective b'y + sum bound * rc
        y = np.asarray(out.dual_solution)
        gh = -(A.T @ y)
        rc = np.where(np.where(gh > 0.0, lbf, ubf), gh, 0.0)
        scale = max(np.abs(y).max(initial=0.0), np.abs(rc).max(initial=0.0))
        assert scale > 0.0
        bound = np.where(rc > 0.0, p.variable_lower_bound, p.variable_upper_bound)
        objective = (float(p.right_hand_side @ y) + float(np.sum(np.where(rc != 0.0, bound * rc, 0.0)))) / scale
        assert objective > 0.0, objective
        residual = max(np.maximum(-y[ne:], 0.0).max(initial=0.0), np.abs(gh - rc).max(initial=0.0)) / scale
        allowance = u * float((absA.T @ np.abs(y)).max(initial=0.0)) / scale
        assert residual / objective <= criteria.eps_primal_infeasible + allowance / objective, (residual, objective)
    else:
        assert out.termination_string == "OPTIMAL"


@pytest.mark.parametrize("name", list(PROBLEMS))
def test_host_path_outcomes(name):
    """no GPU: the host path ends as stated, within the iteration limit, and its point passes the certificate check"""
    host = _host(name)
    assert host.termination_string == PROBLEMS[name][1]
    check_certificate(PROBLEMS[name][0](), host, _params(TOL, LIMIT).termination_criteria)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(PROBLEMS))
def test_device_solve_ends_as_the_host_solve(gpu_required, name):
    dev, host = _device(name), _host(name)
    assert dev.termination_string == host.termination_string == PROBLEMS[name][1]
    check_certificate(PROBLEMS[name][0](), dev, _params(TOL, LIMIT).termination_criteria)


@pytest.mark.gpu
def test_fleet_members_end_as_their_solo_solves(gpu_required):
    names = ["unb3", "chain30", "infeas_chain30"]
    problems = [PROBLEMS[n][0]() for n in names] + [random_lp(30, 30, 3, seed=1)]
    solo = [_device(n).termination_string for n in names] + [optimize(_params(TOL, LIMIT), problems[-1]).termination_string]
    assert solo == ["DUAL_INFEASIBLE", "DUAL_INFEASIBLE", "PRIMAL_INFEASIBLE", "OPTIMAL"]
    outs = optimize_many(_params(TOL, LIMIT), problems)
    assert [o.termination_string for o in outs] == solo
    for p, o in zip(problems, outs):
        check_certificate(p, o, _params(TOL, LIMIT).termination_criteria)


@pytest.mark.gpu
def test_batch_members_end_as_their_solo_solves(gpu_required):
    problems = [_chain30(), _infeas_chain30(), _boxed_chain30()]
    solo = [_device("chain30").termination_string, _device("infeas_chain30").termination_string,
            optimize(_params(TOL, LIMIT), problems[2]).termination_string]
    assert solo == ["DUAL_INFEASIBLE", "PRIMAL_INFEASIBLE", "OPTIMAL"]
    outs = optimize_batch(_params(TOL, LIMIT), problems)
    assert [o.termination_string for o in outs] == solo
    for p, o in zip(problems, outs):
        check_certificate(p, o, _params(TOL, LIMIT).termination_criteria)
