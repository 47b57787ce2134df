"""tests/check_reference.py -- the integer reference of pdhg_eval_point's 22 words -- pinned without a GPU: against the
reference's known answers (tests/stats_cases.py, both halves), against the host evaluation over the CPU oracle engine
on a random integer problem (exactly), and the generator's census of the branch table (it holds, and it bites).  CPU only."""
import dataclasses
from types import SimpleNamespace

import numpy as np
import pytest

from firstorderlp_jl_amd.evaluation import POINT_CURRENT, HostEvaluator
from firstorderlp_jl_amd.primal_dual_hybrid_gradient import EngineOps, UnscaledEngineOps
from firstorderlp_jl_amd.quadratic_programming import ScaledQpProblem
from firstorderlp_jl_amd.solve_log import PointType
from firstorderlp_jl_amd.termination import cached_quadratic_program_info, construct_termination_criteria
from tests import check_reference as R
from tests import stats_cases as S
from tests import test_gpu_check_words_exact as G
from tests.oracle_engine import OracleEngine


@pytest.mark.parametrize("case", S.CASES, ids=lambda c: c[0])
def test_known_answers(case):
    """test/test_iteration_stats.jl:118-308: ConvergenceInformation at (x, y), InfeasibilityInformation at the rays"""
    name, lp, x, y, xr, yr, want_ci, want_ii = case
    P = R.problem_from_arrays(lp.constraint_matrix, lp.objective_vector, lp.right_hand_side, lp.variable_lower_bound,
                              lp.variable_upper_bound, lp.num_equalities, None, lp.objective_constant)
    ci, _ = R.information(P, R.words(P, x, y).words)          # eps_ratio = 1e-6 / 1e-6
    _, ii = R.information(P, R.words(P, xr, yr).words)
    S.check_ci(SimpleNamespace(**ci), want_ci, 1e-15)
    S.check_ii(SimpleNamespace(**ii), want_ii, 0.0)


@pytest.mark.parametrize("qp", [False, True], ids=["lp", "qp"])
@pytest.mark.parametrize("mixed", [False, True], ids=["unit", "pow2"])
def test_against_the_host_evaluator_exactly(qp, mixed):
    """Integers throughout: the host's numpy evaluation is exact as well, so every field is the same double."""
    case = G.make_case(120, 90, 40, 5 + qp, mixed, {}, qp=qp)
    assert np.abs(case.x).max() == 8.0                    # the ray's normalisation x / |x|_inf is exact
    original, scaled = case.original_problem(), case.scaled_problem()
    sp_ = ScaledQpProblem(original, scaled, case.E, case.D)
    eng = OracleEngine.from_problem(scaled)
    ev = HostEvaluator(eng, sp_, cached_quadratic_program_info(original), EngineOps(eng, scaled), UnscaledEngineOps(eng, sp_))
    eng.set_current(case.x * case.D, case.y * case.E)
    tc = construct_termination_criteria(eps_optimal_absolute=1e-6, eps_optimal_relative=1e-6)
    st = ev.iteration_stats(POINT_CURRENT, tc, True, 6, 5.0, 1.5, 1.0, 1.0, PointType.POINT_TYPE_CURRENT_ITERATE)
    P = case.reference_problem()
    w = R.words(P, case.x, case.y)
    ci, ii = R.information(P, w.words)
    for got, want in ((st.convergence_information[0], ci), (st.infeasibility_information[0], ii)):
        for f in dataclasses.fields(got):
            if f.name in want:
                assert getattr(got, f.name) == want[f.name], (f.name, getattr(got, f.name), want[f.name])
    assert set(ci) == set(S.CI_FIELDS) and set(ii) == set(S.II_FIELDS)
    assert ii["dual_ray_objective"] != 0.0 and ii["max_primal_ray_infeasibility"] != 0.0
    assert (ii["primal_ray_quadratic_norm"] != 0.0) == qp
    # the other scalars of a check: sums of squares of the scaled point, the Lagrangian value
    x_s, y_s = case.x * case.D, case.y * case.E
    assert float(x_s @ x_s) == R.sumsq(case.x, case.D) and float(y_s @ y_s) == R.sumsq(case.y, case.E)
    A, Q = original.constraint_matrix, original.objective_matrix
    lag = 0.5 * float(case.x @ (Q @ case.x)) + float(case.c @ case.x) - float(case.x @ (A.T @ case.y)) + float(case.y @ case.b)
    assert lag == R.lagrangian(P, case.x, case.y)
    eng.close()


def test_the_reference_refuses_sums_beyond_2_53():
    case = G.make_case(3, 2, 1, 1, False, {})
    P = case.reference_problem()
    P.c[0] = 2 ** 52
    with pytest.raises(AssertionError, match="2\\^53"):
        R.words(P, [8, 8, 8], [1, 1])


@pytest.mark.parametrize("group", ["small", "mid", "mid_qp", "big"])
def test_census_holds(group):
    G._census_of(group)


def test_census_bites():
    """a generator that leaves one pattern out fails the census"""
    counters, refs = {}, []
    for seed, (ne, mixed) in enumerate(G._variants(*G.MID)):
        case = G.make_case(*G.MID, ne, 1000 + seed, mixed, counters, without=("box", "at_ub", 1))
        refs.append(G._reference(case))
    with pytest.raises(AssertionError, match="column cells are never visited") as failure:
        G.census(refs)
    seen = set().union(*(ref[G.CURRENT].column_cells for ref in refs))
    assert R.COLUMN_CELLS - seen == {c for c in R.COLUMN_CELLS if (c[0], c[3], c[1]) == ("box", "at_ub", 1)}
    assert str(len(R.COLUMN_CELLS - seen)) in str(failure.value)


def test_every_batch_member_fills_the_table():
    for case in G._batch_cases(3):
        G.census([G._reference(case)])
