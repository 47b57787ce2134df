"""Host driver of the PDHG inner loop: the reference's
src/primal_dual_hybrid_gradient.jl with the n-/m-length vector work moved
behind the C ABI (``engine.HipPdhgEngine``).

What stays on the host (as the reference's north star prescribes): the scalar
step-size rules of ``take_step`` (pdhg.jl:555-767), counters, and -- in
``optimize`` -- restarts, primal-weight updates and termination.
"""
import math
import os
import time as _time
from dataclasses import dataclass
from typing import Optional

import numpy as np
import scipy.sparse as sp

from .evaluation import (POINT_AVERAGE, POINT_CURRENT, DeviceEvaluator,
                         HostEvaluator)
from .iteration_stats_utils import print_to_screen_this_iteration
from .preprocess import rescale_problem, validate
from .quadratic_programming import (QuadraticProgrammingProblem, ScaledQpProblem,
                                    is_linear_programming_problem)
from .saddle_point import (RestartParameters, answer_request, compute_new_primal_weight,
                           create_last_restart_info, drive_requests, run_restart_scheme,
                           run_restart_scheme_steps, select_initial_primal_weight,
                           unscaled_saddle_point_output,
                           update_objective_bound_estimates,
                           update_objective_bound_estimates_steps)
from .solve_log import PointType, RestartChoice, TerminationReason
from .termination import (TerminationCriteria, cached_quadratic_program_info,
                          check_termination_criteria)


# ---- step-size policy parameter structs (pdhg.jl:19-68) ----------------------

@dataclass
class MalitskyPockStepsizeParameters:
    """pdhg.jl:19-42"""
    downscaling_factor: float
    breaking_factor: float
    interpolation_coefficient: float


@dataclass
class AdaptiveStepsizeParams:
    """pdhg.jl:44-63"""
    reduction_exponent: float
    growth_exponent: float


@dataclass
class ConstantStepsizeParams:
    """pdhg.jl:65-68"""
    pass


@dataclass
class PdhgSolverState:
    """pdhg.jl:205-258.  The vector fields (current_primal_solution,
    current_dual_solution, delta_*, current_dual_product,
    solution_weighted_avg) live on the device inside ``engine``."""
    engine: object
    step_size: float = 0.0
    primal_weight: float = 1.0
    numerical_error: bool = False
    cumulative_kkt_passes: float = 0.0
    total_number_iterations: int = 0
    required_ratio: Optional[float] = None
    ratio_step_sizes: Optional[float] = None

    # convenience accessors (device -> host copies)
    @property
    def current_primal_solution(self):
        return self.engine.get_current()[0]

    @property
    def current_dual_solution(self):
        return self.engine.get_current()[1]

    @property
    def current_dual_product(self):
        return self.engine.get_dual_product()


def interaction_and_movement(raw, primal_weight):
    """compute_interaction_and_movement (pdhg.jl:527-549) from the device's raw
    sums: raw = [dx.(A'y'-A'y), sum dx^2, sum dy^2, sum dAty^2, 0.5 dx'Qdx].
    ``norm(v)^2`` is restated literally as sqrt(sum)^2."""
    interaction = abs(raw[0]) + abs(raw[4])
    nx = math.sqrt(raw[1])
    ny = math.sqrt(raw[2])
    movement = 0.5 * primal_weight * (nx * nx) + (0.5 / primal_weight) * (ny * ny)
    return interaction, movement


def julia_min(a, b):
    """Julia's ``min`` on Float64: a NaN operand gives NaN (Python's ``min`` returns
    whichever operand the comparison happens to favour).  pdhg.jl:729 uses Julia's: once a
    NaN reaches the step-size rule the reference's step size IS NaN from then on (and, since
    `step_size <= limit` is false for a NaN on either side, its retry loop never accepts
    again -- the reference relies on NaN-free data); the twins here keep the same scalars."""
    if a != a or b != b:
        return math.nan
    return a if a < b else b


def adaptive_step_rule(raw, primal_weight, step_size, total_number_iterations, step_params):
    """What the adaptive policy does with one trial's sums (pdhg.jl:691-729; ``adaptive_step_rule`` of
    csrc/common.hpp is the same statements): (accept, numerical_error, next step size).
    ``total_number_iterations`` counts this trial."""
    interaction, movement = interaction_and_movement(raw, primal_weight)
    if movement == 0.0:
        # The algorithm will terminate at the beginning of the next iteration
        return False, True, step_size
    if interaction > 0:
        step_size_limit = movement / interaction
    else:
        step_size_limit = math.inf
    k1 = float(total_number_iterations + 1)
    first_term = (1 - k1 ** (-step_params.reduction_exponent)) * step_size_limit
    second_term = (1 + k1 ** (-step_params.growth_exponent)) * step_size
    return step_size <= step_size_limit, False, julia_min(first_term, second_term)


# ---- the adaptive policy's scalars to and from the library's take_step(s) calls: one engine, or the members of a batch
# / a fleet side by side (``placed``: (slot, solver_state) pairs, the slot indexing the call's arrays of K entries)

def _native_step_args(step_params, solver_state):
    return (step_params.reduction_exponent, step_params.growth_exponent, solver_state.step_size,
            solver_state.primal_weight, solver_state.total_number_iterations, solver_state.cumulative_kkt_passes)


def _store_step_state(solver_state, step_size, total_number_iterations, cumulative_kkt_passes, numerical_error):
    solver_state.step_size = float(step_size)
    solver_state.total_number_iterations = int(total_number_iterations)
    solver_state.cumulative_kkt_passes = float(cumulative_kkt_passes)
    if numerical_error:
        solver_state.numerical_error = True


def _pack_ratios(K, placed):
    """ratio_step_sizes of a K-member Malitsky-Pock call, packed like ``_pack_step_states``' arrays."""
    ratio = np.ones(K)
    for k, st in placed:
        ratio[k] = st.ratio_step_sizes
    return ratio


def _pack_step_states(K, placed):
    """(step_sizes, primal_weights, total_number_iterations, cumulative_kkt_passes) of a K-member call; the slots that
    ``placed`` does not name hold harmless values."""
    ss, pw, kkt = np.ones(K), np.ones(K), np.zeros(K)
    it = np.zeros(K, dtype=np.int64)
    for k, st in placed:
        ss[k], pw[k], it[k], kkt[k] = st.step_size, st.primal_weight, st.total_number_iterations, st.cumulative_kkt_passes
    return ss, pw, it, kkt


def _unpack_step_states(placed, step_sizes, total_number_iterations, cumulative_kkt_passes, numerical_error, steps_done):
    """What a K-member call returned, back into the states of ``placed``; the steps each of them took."""
    for k, st in placed:
        _store_step_state(st, step_sizes[k], total_number_iterations[k], cumulative_kkt_passes[k], numerical_error[k])
    return [int(steps_done[k]) for k, _ in placed]


def take_step_adaptive(step_params, solver_state):
    """take_step(::AdaptiveStepsizeParams, ...)  pdhg.jl:653-731.

    With the HIP engine the same statements run inside the library
    (pdhg_take_step_adaptive: one call per iteration instead of two with
    Python in between; bitwise the same scalars).  PDHG_PY_TAKE_STEP=1 keeps
    the loop below, which is also what every other engine uses."""
    eng = solver_state.engine
    if hasattr(eng, "take_step_adaptive") and os.environ.get("PDHG_PY_TAKE_STEP", "0") != "1":
        _store_step_state(solver_state, *eng.take_step_adaptive(*_native_step_args(step_params, solver_state)))
        return
    step_size = solver_state.step_size
    done = False
    while not done:
        solver_state.total_number_iterations += 1
        raw = eng.trial_step(step_size, solver_state.primal_weight, 1.0)
        solver_state.cumulative_kkt_passes += 1
        done, numerical_error, step_size = adaptive_step_rule(
            raw, solver_state.primal_weight, step_size, solver_state.total_number_iterations, step_params)
        if numerical_error:
            solver_state.numerical_error = True
            break
        if done:
            # update_solution_in_solver_state: weight = solver_state.step_size,
            # the value on entry to take_step (pdhg.jl:512)
            eng.accept(solver_state.step_size)
    solver_state.step_size = step_size


def take_step_constant(step_params, solver_state):
    """take_step(::ConstantStepsizeParams, ...)  pdhg.jl:737-767."""
    eng = solver_state.engine
    eng.trial_step(solver_state.step_size, solver_state.primal_weight, 1.0)
    solver_state.cumulative_kkt_passes += 1
    eng.accept(solver_state.step_size)


def take_step_malitsky_pock(step_params, solver_state, is_lp=True):
    """take_step(::MalitskyPockStepsizeParameters, ...)  pdhg.jl:555-647."""
    if not is_lp:
        raise ValueError("Malitsky and Pock linesearch is only supported for "
                         "linear programming problems.")
    eng = solver_state.engine
    step_size = solver_state.step_size
    ratio_step_sizes = solver_state.ratio_step_sizes
    done = False
    it = 0
    eng.trial_primal(step_size, solver_state.primal_weight)
    solver_state.cumulative_kkt_passes += 0.5
    step_size = step_size + step_params.interpolation_coefficient * \
        (math.sqrt(1 + ratio_step_sizes) - 1) * step_size
    max_iter = 60
    while not done and it < max_iter:
        it += 1
        solver_state.total_number_iterations += 1
        ratio_step_sizes = step_size / solver_state.step_size
        raw = eng.trial_dual(step_size, solver_state.primal_weight,
                             ratio_step_sizes)
        solver_state.cumulative_kkt_passes += 0.5
        norm_delta_dual_product = math.sqrt(raw[3])
        norm_delta_dual = math.sqrt(raw[2])
        if step_size * norm_delta_dual_product <= \
                step_params.breaking_factor * norm_delta_dual:
            if eng.average_info()[0] == 0:
                eng.add_current_primal_to_average(step_size * ratio_step_sizes)
            eng.accept(solver_state.step_size)
            done = True
        else:
            step_size *= step_params.downscaling_factor
    if it == max_iter and not done:
        solver_state.numerical_error = True
        return
    solver_state.step_size = step_size
    solver_state.ratio_step_sizes = ratio_step_sizes


def take_step(step_params, solver_state, is_lp=True):
    """Dispatch on the policy type like the reference's three methods."""
    if isinstance(step_params, AdaptiveStepsizeParams):
        return take_step_adaptive(step_params, solver_state)
    if isinstance(step_params, MalitskyPockStepsizeParameters):
        return take_step_malitsky_pock(step_params, solver_state, is_lp)
    if isinstance(step_params, ConstantStepsizeParams):
        return take_step_constant(step_params, solver_state)
    raise TypeError(f"unknown step size policy {type(step_params)}")


def take_steps(step_params, solver_state, n_steps, is_lp=True):
    """`n_steps` consecutive take_step calls -- the iterations optimize() runs between
    two termination evaluations (pdhg.jl:862-1046: nothing else happens on them).
    With the HIP engine they are one library call under every policy
    (pdhg_take_steps_adaptive / _constant / _malitsky_pock; the same statements, so the
    same scalars bit for bit).  PDHG_PY_TAKE_STEP=1 keeps the loop below, which is also
    what every other engine uses.
    Stops after a step that raised numerical_error.  Returns the steps taken."""
    eng = solver_state.engine
    native = os.environ.get("PDHG_PY_TAKE_STEP", "0") != "1"
    if isinstance(step_params, AdaptiveStepsizeParams) and hasattr(eng, "take_steps_adaptive") and native:
        *results, done = eng.take_steps_adaptive(n_steps, *_native_step_args(step_params, solver_state))
        _store_step_state(solver_state, *results)
        return done
    if isinstance(step_params, ConstantStepsizeParams) and hasattr(eng, "take_steps_constant") and native:
        solver_state.cumulative_kkt_passes, done = eng.take_steps_constant(
            n_steps, solver_state.step_size, solver_state.primal_weight, solver_state.cumulative_kkt_passes)
        return done
    if isinstance(step_params, MalitskyPockStepsizeParameters) and hasattr(eng, "take_steps_malitsky_pock") and native:
        if not is_lp:
            raise ValueError("Malitsky and Pock linesearch is only supported for "
                             "linear programming problems.")
        step_size, ratio, *results, done = eng.take_steps_malitsky_pock(
            n_steps, step_params.downscaling_factor, step_params.breaking_factor, step_params.interpolation_coefficient,
            solver_state.step_size, solver_state.ratio_step_sizes, solver_state.primal_weight,
            solver_state.total_number_iterations, solver_state.cumulative_kkt_passes)
        _store_step_state(solver_state, step_size, *results)
        solver_state.ratio_step_sizes = float(ratio)
        return done
    done = 0
    while done < n_steps:
        take_step(step_params, solver_state, is_lp)
        done += 1
        if solver_state.numerical_error:
            break
    return done


# ==============================================================================
# optimize(): the reference's outer loop (pdhg.jl:782-1049) on the host, with
# every n-/m-length vector operation behind ``engine``.
# ==============================================================================

@dataclass
class PdhgParameters:
    """pdhg.jl:128-199 (same field names and order)."""
    l_inf_ruiz_iterations: int
    l2_norm_rescaling: bool
    pock_chambolle_alpha: Optional[float]
    primal_importance: float
    scale_invariant_initial_primal_weight: bool
    verbosity: int
    record_iteration_stats: bool
    termination_evaluation_frequency: int
    termination_criteria: TerminationCriteria
    restart_params: RestartParameters
    step_size_policy_params: object


class EngineOps:
    """A*x, A'*y of the SCALED problem on the device (pdhg_spmv / pdhg_spmv_t);
    Q*x on the host (Q is LP-empty or tiny in the reference's QPs)."""

    def __init__(self, engine, problem):
        self._eng = engine
        self._Q = problem.objective_matrix
        self._n = problem.num_variables

    def Ax(self, x):
        return self._eng.spmv(x)

    def ATy(self, y):
        return self._eng.spmv_t(y)

    def Qx(self, x):
        if self._Q.nnz == 0:
            return np.zeros(self._n)
        return self._Q @ x


class UnscaledEngineOps:
    """The ORIGINAL problem's mat-vecs through the scaled device matrix:
    A = E A_s D  =>  A x = E .* (A_s (D .* x)),  A'y = D .* (A_s' (E .* y))."""

    def __init__(self, engine, scaled_problem):
        self._eng = engine
        self._E = scaled_problem.constraint_rescaling
        self._D = scaled_problem.variable_rescaling
        self._Q = scaled_problem.original_qp.objective_matrix
        self._n = scaled_problem.original_qp.num_variables

    def Ax(self, x):
        return self._E * self._eng.spmv(self._D * x)

    def ATy(self, y):
        return self._D * self._eng.spmv_t(self._E * y)

    def Qx(self, x):
        if self._Q.nnz == 0:
            return np.zeros(self._n)
        return self._Q @ x


def power_method_failure_probability(dimension, epsilon, k):
    """pdhg.jl:378-390"""
    if k < 2 or epsilon <= 0.0:
        return 1.0
    return min(0.824, 0.354 / math.sqrt(epsilon * (k - 1))) * \
        math.sqrt(dimension) * (1.0 - epsilon) ** (k - 1 / 2)


def estimate_maximum_singular_value(ops, num_cols, probability_of_failure=0.01,
                                    desired_relative_error=0.1, seed=1):
    """pdhg.jl:414-440.  The reference draws randn(MersenneTwister(seed)); that
    stream cannot be replayed outside Julia, so parity of the constant-step
    policy is at the tolerance of the power method, not bitwise."""
    epsilon = 1.0 - (1.0 - desired_relative_error) ** 2
    x = np.random.default_rng(seed).standard_normal(num_cols)
    number_of_power_iterations = 0
    while power_method_failure_probability(num_cols, epsilon,
                                           number_of_power_iterations) > probability_of_failure:
        x = x / math.sqrt(float(x @ x))
        x = ops.ATy(ops.Ax(x))
        number_of_power_iterations += 1
    return (math.sqrt(float(x @ ops.ATy(ops.Ax(x))) / float(x @ x)),
            number_of_power_iterations)


def define_norms(primal_size, dual_size, step_size, primal_weight):
    """pdhg.jl:265-277"""
    with np.errstate(divide="ignore"):
        primal_norm_params = np.float64(1) / step_size * primal_weight * np.ones(primal_size)
        dual_norm_params = np.float64(1) / step_size / primal_weight * np.ones(dual_size)
    return primal_norm_params, dual_norm_params


def _default_engine_factory(problem):
    from .engine import HipPdhgEngine
    return HipPdhgEngine.from_problem(problem)


_default_engine_factory.takes_original_problem = True


def _check_inputs(params, problems):
    for problem in problems:
        validate(problem)
    if params.primal_importance <= 0 or not math.isfinite(params.primal_importance):
        raise ValueError("primal_importance must be positive and finite")


def _rescales_on_device(factory):
    """A factory whose ``takes_original_problem`` is true receives the ORIGINAL problem(s) and what it builds
    rescales on the device (the product path); PDHG_HOST_RESCALE=1 turns that off."""
    return getattr(factory, "takes_original_problem", False) and os.environ.get("PDHG_HOST_RESCALE", "0") != "1"


def _device_scaled_problem(original_problem, engine, constraint_rescaling, variable_rescaling):
    """The host's ``ScaledQpProblem`` of an engine that was rescaled on the device (``rescale``): only the
    n-/m-length vectors come back; the scaled constraint (and objective) matrix lives on the device only."""
    c_s, b_s, lb_s, ub_s = engine.get_problem_vectors()
    m0, n0 = original_problem.constraint_matrix.shape
    problem = QuadraticProgrammingProblem(
        lb_s, ub_s, sp.csc_matrix((n0, n0)), c_s, original_problem.objective_constant,
        sp.csc_matrix((m0, n0)), b_s, original_problem.num_equalities)
    return ScaledQpProblem(original_problem, problem, constraint_rescaling, variable_rescaling)


def _host_scaled_problem(params, original_problem):
    """``rescale_problem`` on the host: (scaled problem, norm(A, Inf) of its sparse constraint matrix)."""
    scaled_problem = rescale_problem(params.l_inf_ruiz_iterations, params.l2_norm_rescaling,
                                     params.pock_chambolle_alpha, params.verbosity, original_problem)
    data = scaled_problem.scaled_qp.constraint_matrix.data
    return scaled_problem, (float(np.max(np.abs(data))) if len(data) else 0.0)


CONSTANT_STEP_DESIRED_RELATIVE_ERROR = 0.2
KKT_PASSES_PER_TERMINATION_EVALUATION = 2.0


def _constant_step_estimate(solve):
    """The constant policy's power method on one solve's operators (pdhg.jl:829-838): what ``_Solve.start`` takes."""
    return estimate_maximum_singular_value(solve.ops, solve.problem.num_variables, probability_of_failure=0.001,
                                           desired_relative_error=CONSTANT_STEP_DESIRED_RELATIVE_ERROR)


class _Solve:
    """One problem's host-side solve: the state of the reference's ``optimize`` (pdhg.jl:782-1049) and what it does
    at an evaluation.  ``optimize`` drives one of these, ``batch.optimize_batch`` one per member; the caller takes
    the steps in between."""

    def __init__(self, params, original_problem, scaled_problem, engine, matrix_max_abs):
        self.params = params
        self.scaled_problem = scaled_problem
        self.problem = scaled_problem.scaled_qp
        self.engine = engine
        self.matrix_max_abs = matrix_max_abs
        # (from the original problem: the host copy of a device-rescaled problem carries no matrices)
        self.is_lp = is_linear_programming_problem(original_problem)
        self.qp_cache = cached_quadratic_program_info(original_problem)
        self.ops = EngineOps(engine, self.problem)
        self.original_ops = UnscaledEngineOps(engine, scaled_problem)
        self.state = PdhgSolverState(engine)   # zeros(...) state, pdhg.jl:805-819
        self.last_restart_info = create_last_restart_info()
        self.iteration = 0
        self.iteration_stats = []
        self.time_spent_doing_basic_algorithm = 0.0
        self.output = None

    def start(self, singular_value_estimate=None):
        """Initial step size and primal weight, the evaluator, the clock (pdhg.jl:821-860).  The constant policy takes
        ``singular_value_estimate`` = (maximum_singular_value, number_of_power_iterations) from the caller
        (``_constant_step_estimate``: it depends on the matrix only)."""
        params, st, problem = self.params, self.state, self.problem
        policy = params.step_size_policy_params
        inv_max_abs = math.inf if self.matrix_max_abs == 0.0 else 1.0 / self.matrix_max_abs
        if isinstance(policy, AdaptiveStepsizeParams):
            st.cumulative_kkt_passes += 0.5
            st.step_size = inv_max_abs
        elif isinstance(policy, MalitskyPockStepsizeParameters):
            st.cumulative_kkt_passes += 0.5
            st.step_size = inv_max_abs
            st.ratio_step_sizes = 1.0
        else:
            maximum_singular_value, number_of_power_iterations = singular_value_estimate
            st.step_size = (1 - CONSTANT_STEP_DESIRED_RELATIVE_ERROR) / maximum_singular_value
            st.cumulative_kkt_passes += number_of_power_iterations

        if params.scale_invariant_initial_primal_weight:
            st.primal_weight = select_initial_primal_weight(
                problem, np.ones(problem.num_variables), np.ones(problem.num_constraints),
                params.primal_importance, params.verbosity)
        else:
            st.primal_weight = params.primal_importance

        self.start_time = _time.time()
        if getattr(self.engine, "supports_device_evaluation", False):
            self.ev = DeviceEvaluator(self.engine, self.scaled_problem, self.qp_cache)
        else:
            self.ev = HostEvaluator(self.engine, self.scaled_problem, self.qp_cache, self.ops, self.original_ops)
        st.numerical_error = False

    def evaluate(self):
        """The top of one iteration of optimize's loop (pdhg.jl:862-1023).  Returns the number of take_steps to
        run before the next evaluation, or 0 once the solve has terminated (``self.output`` set)."""
        return drive_requests(self.evaluate_steps(), self.ev)

    def evaluate_steps(self):
        """``evaluate`` as a generator (saddle_point.py, "the check's device requests"): yields at the three places where
        the check asks the evaluator for device results -- the iteration stats, the bounds behind the objective-bound
        estimates, the bounds of the restart test -- and returns ``evaluate``'s step count."""
        params, st, ev = self.params, self.state, self.ev
        termination_criteria = params.termination_criteria
        iteration_limit = termination_criteria.iteration_limit
        termination_evaluation_frequency = params.termination_evaluation_frequency
        self.iteration += 1
        iteration = self.iteration
        if ((iteration - 1) % termination_evaluation_frequency == 0 or
                iteration == iteration_limit + 1 or iteration <= 10 or
                st.numerical_error):
            st.cumulative_kkt_passes += KKT_PASSES_PER_TERMINATION_EVALUATION
            count_x, count_y, _, _ = self.engine.average_info()
            if st.numerical_error or count_x == 0 or count_y == 0:
                avg_point = POINT_CURRENT
            else:
                avg_point = POINT_AVERAGE

            current_iteration_stats = yield ("iteration_stats", (
                avg_point, termination_criteria, params.record_iteration_stats, iteration,
                _time.time() - self.start_time, st.cumulative_kkt_passes,
                st.step_size, st.primal_weight, PointType.POINT_TYPE_AVERAGE_ITERATE))
            method_specific_stats = current_iteration_stats.method_specific_stats
            method_specific_stats["time_spent_doing_basic_algorithm"] = \
                self.time_spent_doing_basic_algorithm

            # define_norms (pdhg.jl:265-277): uniform weights, kept as scalars
            with np.errstate(divide="ignore"):
                primal_weight_norm = float(np.float64(1) / st.step_size * st.primal_weight)
                dual_weight_norm = float(np.float64(1) / st.step_size / st.primal_weight)
            termination_reason = check_termination_criteria(
                termination_criteria, self.qp_cache, current_iteration_stats)
            if st.numerical_error and termination_reason is False:
                termination_reason = TerminationReason.TERMINATION_REASON_NUMERICAL_ERROR
            # update_objective_bound_estimates (pdhg.jl:938-945) fills three entries of method_specific_stats that are
            # only ever read from KEPT stats (solve_log; the final log, saddle_point.jl:961-993) -- neither the
            # termination test nor the restart scheme sees them.  A check whose stats are dropped skips the two
            # trust-region problems behind them (a quarter of a check on medium LPs); the values of kept stats are
            # the reference's (both functions only read the state, so their order does not matter).
            if params.record_iteration_stats or termination_reason is not False:
                yield from update_objective_bound_estimates_steps(
                    method_specific_stats, ev, avg_point, primal_weight_norm, dual_weight_norm)
                self.iteration_stats.append(current_iteration_stats)

            if print_to_screen_this_iteration(termination_reason, iteration, params.verbosity,
                                              termination_evaluation_frequency):
                _display_iteration_stats(current_iteration_stats)

            if termination_reason is not False:
                # ** Terminate the algorithm ** (the only exit, pdhg.jl:973-992)
                if params.verbosity >= 2:
                    print(f"Terminated after {iteration - 1} iterations: "
                          f"{termination_reason.name}")
                avg_primal_solution, avg_dual_solution = ev.solution(avg_point)
                self.output = unscaled_saddle_point_output(
                    self.scaled_problem, avg_primal_solution, avg_dual_solution,
                    termination_reason, iteration - 1, self.iteration_stats)
                return 0

            current_iteration_stats.restart_used = yield from run_restart_scheme_steps(
                ev, self.last_restart_info, iteration - 1, primal_weight_norm,
                dual_weight_norm, st.primal_weight, params.verbosity,
                params.restart_params)

            if current_iteration_stats.restart_used != RestartChoice.RESTART_CHOICE_NO_RESTART:
                st.primal_weight = compute_new_primal_weight(
                    self.last_restart_info, st.primal_weight,
                    params.restart_params.primal_weight_update_smoothing, params.verbosity)
                st.ratio_step_sizes = 1.0
            # RESTART_TO_AVERAGE: A'y was recomputed inside
            # engine.restart_to_average() (pdhg.jl:1018-1022).

        # This iteration's take_step and those of the iterations up to (not including)
        # the next one the test above fires on: the reference does nothing else on them.
        next_evaluation = ((iteration - 1) // termination_evaluation_frequency + 1) * \
            termination_evaluation_frequency + 1
        if iteration < 10:
            next_evaluation = iteration + 1
        if iteration < iteration_limit + 1:
            next_evaluation = min(next_evaluation, iteration_limit + 1)
        return next_evaluation - iteration

    def stepped(self, steps_taken, seconds):
        """The caller took ``steps_taken`` take_steps since ``evaluate`` (fewer than asked after a numerical error)."""
        self.iteration += steps_taken - 1
        self.time_spent_doing_basic_algorithm += seconds


def _check_round(active, checks):
    """One round's evaluations of the active solves with their device requests gathered: every solve's
    ``evaluate_steps`` is advanced to its next request, ``checks(pending)`` -- ``pending`` = [(solve, request)] in the
    solves' order -- lets the device answer the requests of all of them at once and leave the results with the
    members, then each solve's OWN evaluator call runs unchanged (it finds the result) and its return value goes into
    the generator; until every generator has returned its step count (at most three sweeps: the iteration stats, the
    objective-bound estimates, the restart test).  Returns {id(solve): steps}."""
    steps = {}
    pending = []

    def advance(mb, gen, answer=None, first=False):
        try:
            pending.append((mb, gen, next(gen) if first else gen.send(answer)))
        except StopIteration as stop:
            steps[id(mb)] = stop.value

    for mb in active:
        advance(mb, mb.evaluate_steps(), first=True)
    while pending:
        sweep, pending = pending, []
        checks([(mb, request) for mb, _, request in sweep])
        for mb, gen, request in sweep:
            advance(mb, gen, answer_request(mb.ev, request))
    return steps


def _check_requests(pending, slot, members):
    """A sweep's ``pending`` requests (``_check_round``) as the arguments of the shared check calls: (points, tr_items)
    -- ``points[slot(solve)]`` = the point of the solve's ``"iteration_stats"`` request, -1 where it has none, over
    ``members`` slots; ``tr_items`` = (slot, point, primal weight, dual weight, radius, range, approximate) for every
    trust-region problem of the ``"bounds"`` requests, in the solves' order."""
    points = np.full(members, -1, dtype=np.int32)
    tr_items = []
    for mb, (method, arguments) in pending:
        k = slot(mb)
        if method == "iteration_stats":
            points[k] = arguments[0]
        elif method == "bounds":
            requests, primal_w, dual_w, norm, approximate = arguments
            tr_items.extend((k, point, primal_w, dual_w, radius, rng, approximate)
                            for point, radius, rng in mb.ev.tr_problems(requests, norm))
    return points, tr_items


def _drive_solves(solves, step, checks=None):
    """The outer loop of several solves side by side (``batch.optimize_batch``, ``fleet.optimize_many``): at each
    round every active solve evaluates and names its step count, a solve that terminated leaves, and
    ``step(requests)`` -- ``requests`` = [(solve, steps)] in the solves' order -- takes those steps and returns
    (solve, steps taken, seconds) for each.  ``checks``: the round's evaluations go through ``_check_round``.
    Returns the outputs in the solves' order."""
    active = list(solves)
    while active:
        requests = []
        round_steps = _check_round(active, checks) if checks is not None else None
        for mb in active:
            steps = round_steps[id(mb)] if round_steps is not None else mb.evaluate()
            if steps > 0:
                requests.append((mb, steps))
        active = [mb for mb in active if mb.output is None]
        if requests:
            for mb, done, seconds in step(requests):
                mb.stepped(done, seconds)
    return [mb.output for mb in solves]


def _initial_point(problem, initial_primal_solution, initial_dual_solution):
    """The starting point of a warm solve, checked on the host before any device work: ``(x0, y0)`` as float64
    vectors (``None`` stays ``None``: zeros), or ``None`` when neither was given.  Wrong lengths and entries that are
    not finite raise ``ValueError``."""
    if initial_primal_solution is None and initial_dual_solution is None:
        return None
    m, n = problem.constraint_matrix.shape
    point = []
    for name, value, length in (("initial_primal_solution", initial_primal_solution, n),
                                ("initial_dual_solution", initial_dual_solution, m)):
        if value is not None:
            value = np.ascontiguousarray(value, dtype=np.float64)
            if value.shape != (length,):
                raise ValueError(f"{name} has shape {value.shape}, the problem needs ({length},)")
            if not np.all(np.isfinite(value)):
                raise ValueError(f"{name} holds entries that are not finite")
        point.append(value)
    return tuple(point)


def _set_initial_point(engine, scaled_problem, point):
    """A fresh engine's iterate at ``point`` (original space): scaled on the host -- the output divides by the same
    factors -- and handed to ``engine.set_current``, which also computes A'y."""
    x0, y0 = point
    engine.set_current(None if x0 is None else x0 * scaled_problem.variable_rescaling,
                       None if y0 is None else y0 * scaled_problem.constraint_rescaling)


def _step_solves(policy, requests):
    """``_drive_solves``' step for solves that are stepped one by one through ``take_steps``."""
    out = []
    for mb, steps in requests:
        time_spent_doing_basic_algorithm_checkpoint = _time.time()
        steps_taken = take_steps(policy, mb.state, steps, mb.is_lp)
        out.append((mb, steps_taken, _time.time() - time_spent_doing_basic_algorithm_checkpoint))
    return out


def _drive_solve(solve):
    """One started solve to its end: the loop of the reference's ``optimize`` (pdhg.jl:862-1049) -- evaluate, take the
    steps up to the next evaluation, until the evaluation terminates.  ``optimize`` and ``session.PdhgSession.solve``
    run this."""
    policy = solve.params.step_size_policy_params
    return _drive_solves([solve], lambda requests: _step_solves(policy, requests))[0]


def optimize(params, original_problem, engine_factory=None, initial_primal_solution=None, initial_dual_solution=None):
    """``optimize(params::PdhgParameters, original_problem)`` -- pdhg.jl:782-1049.

    ``engine_factory(problem) -> engine`` builds the device state; the default is the HIP engine on the current GPU
    and there is no CPU fallback.  A factory whose ``takes_original_problem`` is true (the default is one) receives
    the original problem and rescales it on the device, any other one the host-rescaled problem.

    ``initial_primal_solution`` / ``initial_dual_solution``: a starting point in the ORIGINAL problem's space (either
    may be ``None``: zeros; both ``None``, the default: the reference's cold start, untouched).  The reference has no
    warm start to follow: the point replaces the zeros of ``PdhgSolverState`` (pdhg.jl:805-819) and nothing else
    changes -- the step size, the primal weight and ``cumulative_kkt_passes`` start exactly as in a cold solve, the
    averages are empty (so the first evaluation looks at the point itself), and the point is not projected: the
    first step's projections do that.  Lengths and finiteness are checked before any device work.

    Returns a ``SaddlePointOutput``.  The engine (device memory) is released on every exit path, exceptions
    included."""
    _check_inputs(params, [original_problem])
    point = _initial_point(original_problem, initial_primal_solution, initial_dual_solution)
    factory = engine_factory or _default_engine_factory
    engine = None
    try:
        if _rescales_on_device(factory):
            engine = factory(original_problem)
            constraint_rescaling, variable_rescaling = engine.rescale(
                params.l_inf_ruiz_iterations, params.l2_norm_rescaling, params.pock_chambolle_alpha)
            scaled_problem = _device_scaled_problem(original_problem, engine, constraint_rescaling,
                                                    variable_rescaling)
            matrix_max_abs = engine.matrix_max_abs()
        else:
            scaled_problem, matrix_max_abs = _host_scaled_problem(params, original_problem)
            engine = factory(scaled_problem.scaled_qp)
        solve = _Solve(params, original_problem, scaled_problem, engine, matrix_max_abs)
        if point is not None:
            _set_initial_point(engine, scaled_problem, point)
        policy = params.step_size_policy_params
        solve.start(_constant_step_estimate(solve) if isinstance(policy, ConstantStepsizeParams) else None)
        return _drive_solve(solve)
    finally:
        if engine is not None and hasattr(engine, "close"):
            engine.close()


def _display_iteration_stats(stats):
    """Condensed form of display_iteration_stats (iteration_stats_utils.jl:559-619)."""
    ci = stats.convergence_information[0]
    print("  %6d %9.1f %8.2f | %9.2e %9.2e %9.2e | %12.5e %12.5e | %9.2e %9.2e" % (
        stats.iteration_number, stats.cumulative_kkt_matrix_passes,
        stats.cumulative_time_sec, ci.relative_l2_primal_residual,
        ci.relative_l2_dual_residual, ci.relative_optimality_gap,
        ci.primal_objective, ci.dual_objective, stats.step_size,
        stats.primal_weight))
