"""Many independent small LPs at once, one workgroup per LP.

``optimize_many(params, problems)`` returns what ``optimize(params, problems[k])`` returns, for every k.  The problems
share nothing -- any mix of shapes, LPs and QPs.  What they share is the launch: an LP small enough for the solo
small-LP path (csrc/small_lp_kernel.hpp: every vector in one workgroup's LDS) takes its steps between two evaluations in
one workgroup, and ``pdhg_fleet_take_steps_adaptive`` (``_constant`` / ``_malitsky_pock`` under the two other policies)
carries one such workgroup per problem in one launch instead of one launch per problem on one of 256 compute units.
With ``PDHG_SMALL_QP=1`` in the environment (off by default) a small QP -- ``11n + 4m`` doubles of LDS, rows of ``Q`` and
``Q'`` of at most 256 entries -- belongs to that class too and rides in launches of the QP kernels beside the LPs'; without
it a QP member is stepped by its own launches inside the same call.  The members do not run in lockstep: each accepts, rejects, restarts and
terminates on its own, at the iterations ``optimize`` would.  Both drivers run the same per-problem solve object
(``primal_dual_hybrid_gradient._Solve``).  The checks between the steps go the same way: a fleet with ``eval_points`` and
``trust_region_bounds`` gets the device requests of every member's check -- the termination evaluation, the
objective-bound estimates, the restart test -- in shared launches, one workgroup per member or trust-region problem
(csrc/fleet_check_kernels.hpp), and each member then reads its own result; the restarts themselves stay per member.
Under the same ``PDHG_SMALL_QP=1`` the shared check launches carry QP members as well (rows of ``Q`` of at most 256
entries; the library decides per call, nothing changes here).  With ``PDHG_FLEET_RESCALE=1`` (off by default) the members'
rescaling before the first step goes the same way: one ``fleet.rescale`` -- one workgroup per member in one launch
(csrc/fleet_rescale_kernels.hpp) -- instead of ``rescale`` and ``matrix_max_abs`` member after member, the same bits.

``HipPdhgFleet`` is the device side: one fleet handle that owns K ordinary member handles on one stream (``.members``:
``HipPdhgEngine`` views -- every single-LP method works on them, ``rescale`` included: a member's matrix is its own).
"""
import ctypes
import os
import time as _time

import numpy as np

from . import _lib
from .engine import _dp, _int_p, _MemberEngine, _MemberOwner, _d, _i, _pd, _pi
from .primal_dual_hybrid_gradient import (AdaptiveStepsizeParams, ConstantStepsizeParams,
                                          MalitskyPockStepsizeParameters, _check_inputs, _check_requests,
                                          _constant_step_estimate, _device_scaled_problem, _drive_solves,
                                          _host_scaled_problem, _initial_point, _pack_ratios, _pack_step_states,
                                          _rescales_on_device, _set_initial_point, _Solve, _unpack_step_states,
                                          take_steps)


class HipPdhgFleet(_MemberOwner):
    """K independent problems on one GPU and one stream (``pdhg_create_fleet`` / ``pdhg_fleet_add``)."""

    takes_original_problem = True

    def __init__(self, device_id=-1, stream=None):
        self._L = _lib.lib()
        h = ctypes.c_void_p()
        _lib.check(self._L.pdhg_create_fleet(ctypes.byref(h), int(device_id), ctypes.c_void_p(stream) if stream else None))
        self._h = h
        self.members = []

    @property
    def K(self):
        return len(self.members)

    def add(self, problem):
        """A new member from a problem (``pdhg_fleet_add``; a QP's objective matrix is uploaded to the member)."""
        A = problem.constraint_matrix.tocsc()
        m, n = int(A.shape[0]), int(A.shape[1])
        colptr, rowval, nzval = _i(A.indptr), _i(A.indices), _d(A.data)
        c, b = _d(problem.objective_vector), _d(problem.right_hand_side)
        lb, ub = _d(problem.variable_lower_bound), _d(problem.variable_upper_bound)
        if c.shape != (n,) or lb.shape != (n,) or ub.shape != (n,) or b.shape != (m,):
            raise ValueError("vector lengths do not match the constraint matrix")
        mh = ctypes.c_void_p()
        _lib.check(self._L.pdhg_fleet_add(self._h, m, n, len(nzval), _pi(colptr), _pi(rowval), _pd(nzval), 0, _pd(c),
                                          _pd(b), _pd(lb), _pd(ub), int(problem.num_equalities), ctypes.byref(mh)))
        eng = _MemberEngine._wrap(self._L, mh, m, n)
        self.members.append(eng)
        eng._upload_objective_matrix(problem.objective_matrix)
        return eng

    @classmethod
    def from_problems(cls, problems, device_id=-1, stream=None):
        problems = list(problems)
        if not problems:
            raise ValueError("a fleet needs at least one problem")
        fleet = cls(device_id=device_id, stream=stream)
        try:
            for p in problems:
                fleet.add(p)
        except Exception:
            fleet.close()
            raise
        return fleet

    def take_steps_adaptive(self, n_steps, reduction_exponent, growth_exponent, step_sizes, primal_weights,
                            total_number_iterations, cumulative_kkt_passes):
        """``n_steps[k]`` take_steps of member k, for every k (0: the member is left alone); the small LPs among them in
        one launch.  Returns arrays (step_sizes, total_number_iterations, cumulative_kkt_passes, numerical_error,
        steps_done)."""
        ns = np.array(np.broadcast_to(n_steps, (self.K,)), dtype=np.int64)
        return self._take_steps_adaptive(self._L.pdhg_fleet_take_steps_adaptive, _pi(ns), reduction_exponent,
                                         growth_exponent, step_sizes, primal_weights, total_number_iterations,
                                         cumulative_kkt_passes)

    def take_steps_constant(self, n_steps, step_sizes, primal_weights, cumulative_kkt_passes):
        """``n_steps[k]`` constant-step take_steps of member k, for every k (0: left alone); the small LPs among them in
        one launch.  Returns arrays (cumulative_kkt_passes, steps_done)."""
        ns = np.array(np.broadcast_to(n_steps, (self.K,)), dtype=np.int64)
        return self._take_steps_constant(self._L.pdhg_fleet_take_steps_constant, _pi(ns), step_sizes, primal_weights,
                                         cumulative_kkt_passes)

    def take_steps_malitsky_pock(self, n_steps, downscaling_factor, breaking_factor, interpolation_coefficient,
                                 step_sizes, ratio_step_sizes, primal_weights, total_number_iterations,
                                 cumulative_kkt_passes):
        """``n_steps[k]`` Malitsky-Pock take_steps of member k (an LP), for every k (0: left alone); the small LPs among
        them in one launch.  Returns arrays (step_sizes, ratio_step_sizes, total_number_iterations,
        cumulative_kkt_passes, numerical_error, steps_done)."""
        ns = np.array(np.broadcast_to(n_steps, (self.K,)), dtype=np.int64)
        return self._take_steps_malitsky_pock(self._L.pdhg_fleet_take_steps_malitsky_pock, _pi(ns), downscaling_factor,
                                              breaking_factor, interpolation_coefficient, step_sizes, ratio_step_sizes,
                                              primal_weights, total_number_iterations, cumulative_kkt_passes)

    def info(self):
        """dict(members, shared_launches, carried, single): the last two describe the last ``take_steps_*`` call."""
        info = np.zeros(8, dtype=np.int64)
        _lib.check(self._L.pdhg_fleet_info(self._h, _pi(info)))
        return dict(zip(["members", "shared_launches", "carried", "single"], info[:4].tolist()))

    # ---- the checks in shared launches (pdhg_fleet_eval_points / pdhg_fleet_trust_region_bounds) ----
    def eval_points(self, points):
        """``members[k].eval_point(points[k])`` for every k (-1: member k is left alone, its row stays as it is), the
        members that suit it in one launch: a (K, 24) array.  Every result is also left in its member: the member's own
        ``eval_point`` with the same point answers from it until the member's state moves."""
        pts = np.ascontiguousarray(np.broadcast_to(points, (self.K,)), dtype=np.int32)
        out = np.zeros((self.K, 24))
        _lib.check(self._L.pdhg_fleet_eval_points(self._h, pts.ctypes.data_as(_int_p), _pd(out)))
        return out

    def trust_region_bounds(self, items):
        """``members[k].trust_region_bound(point, wp, wd, radius, range, approximate)`` for every item
        ``(k, point, wp, wd, radius, range, approximate)``, the members that suit it in one launch: a (len(items), 8)
        array.  Left in the members like ``eval_points``' results."""
        items = list(items)
        count = len(items)
        out = np.zeros((count, 8))
        if count == 0:
            return out
        col = list(zip(*items))
        ints = [np.ascontiguousarray(col[q], dtype=np.int32) for q in (0, 1, 5)]
        approx = np.ascontiguousarray([int(bool(a)) for a in col[6]], dtype=np.int32)
        dbl = [_d(col[q]) for q in (2, 3, 4)]
        _lib.check(self._L.pdhg_fleet_trust_region_bounds(
            self._h, count, ints[0].ctypes.data_as(_int_p), ints[1].ctypes.data_as(_int_p), _pd(dbl[0]), _pd(dbl[1]),
            _pd(dbl[2]), ints[2].ctypes.data_as(_int_p), approx.ctypes.data_as(_int_p), _pd(out)))
        return out

    def check_info(self):
        """dict(check_launches, carried, single, misses): launches of the check kernels so far; items of the last
        ``eval_points`` / ``trust_region_bounds`` carried by a shared launch / served per member; ``eval_point`` and
        ``trust_region_bound`` calls on members so far that no stored fleet result answered (the fleet's own calls
        for the members it serves one by one are not counted)."""
        info = np.zeros(8, dtype=np.int64)
        _lib.check(self._L.pdhg_fleet_info(self._h, _pi(info)))
        return dict(zip(["check_launches", "carried", "single", "misses"], info[4:8].tolist()))

    # ---- the rescaling in one shared launch (include/pdhg_hip_fleet_rescale.h) ----
    def rescale(self, l_inf_ruiz_iterations, l2_norm_rescaling, pock_chambolle_alpha, members=None):
        """``eng.rescale(...)`` and ``eng.matrix_max_abs()`` of the members named (indices; None: all), the members that
        suit it in ONE launch, one workgroup per member: ``([(E, D), ...], [max_abs, ...])`` in the order named, the
        same bits as the members' own calls.  The other members are left as they are."""
        K = self.K
        named = list(range(K)) if members is None else [int(k) for k in members]
        if len(set(named)) != len(named) or any(not 0 <= k < K for k in named):
            raise ValueError(f"members must be distinct indices below {K}")
        active = np.zeros(K, dtype=np.int32)
        active[named] = 1
        Es = [np.empty(self.members[k].m) for k in named]
        Ds = [np.empty(self.members[k].n) for k in named]
        e_table, d_table = (_dp * K)(), (_dp * K)()
        for k, E, D in zip(named, Es, Ds):
            e_table[k], d_table[k] = _pd(E), _pd(D)
        max_abs = np.zeros(K)
        use_pc = pock_chambolle_alpha is not None
        _lib.check(self._L.pdhg_fleet_rescale(self._live(), active.ctypes.data_as(_int_p), int(l_inf_ruiz_iterations),
                                              int(bool(l2_norm_rescaling)), int(use_pc),
                                              float(pock_chambolle_alpha) if use_pc else 0.0, e_table, d_table,
                                              _pd(max_abs)))
        return list(zip(Es, Ds)), [float(max_abs[k]) for k in named]

    def rescale_info(self):
        """dict(shared_launches, carried, single, view_rebuilds): shared rescale launches so far; members the last
        ``rescale`` carried in its launch / served by their own calls; lazy rebuilds of bound views so far."""
        info = np.zeros(4, dtype=np.int64)
        _lib.check(self._L.pdhg_fleet_rescale_info(self._live(), _pi(info)))
        return dict(zip(["shared_launches", "carried", "single", "view_rebuilds"], info.tolist()))

    # ---- re-solves in shared launches (include/pdhg_hip_resolve.h): ``_MemberOwner``'s, over these ----
    _noun, _resolve_other = "fleet", "view_rebuilds"

    def _resolve_calls(self):
        return (self._L.pdhg_fleet_update_problem_vectors, self._L.pdhg_fleet_warm_start, self._L.pdhg_fleet_resolve_info)


def _default_fleet_factory(problems):
    return HipPdhgFleet.from_problems(problems)


_default_fleet_factory.takes_original_problem = True


def _fleet_rescales(fleet):
    """Do the members rescale through ONE ``fleet.rescale``?  With ``PDHG_FLEET_RESCALE=1`` in the environment (read at
    every call; off by default: the path is new) and a fleet that has the method; else member by member, every call
    and launch as it always was."""
    return os.environ.get("PDHG_FLEET_RESCALE", "0") == "1" and hasattr(fleet, "rescale")


def _rescale_members(fleet, params, members=None):
    """``(E, D)`` and max |a| of the members named (None: all) after their rescaling on the device: one
    ``fleet.rescale`` (``_fleet_rescales``), or ``eng.rescale`` and ``eng.matrix_max_abs`` member after member."""
    args = (params.l_inf_ruiz_iterations, params.l2_norm_rescaling, params.pock_chambolle_alpha)
    if _fleet_rescales(fleet):
        return fleet.rescale(*args) if members is None else fleet.rescale(*args, members=members)
    factors, max_abs = [], []
    for k in (range(len(fleet.members)) if members is None else members):
        eng = fleet.members[k]
        factors.append(eng.rescale(*args))
        max_abs.append(eng.matrix_max_abs())
    return factors, max_abs


def _step_fleet(fleet, solves, policy, requests):
    """The steps the members named at this round: one ``take_steps_adaptive`` / ``_constant`` / ``_malitsky_pock`` of the
    fleet for all of them, else (PDHG_PY_TAKE_STEP=1, a fleet without the policy's native call) member by member through
    ``take_steps``.  Returns (solve, steps taken, seconds) per request."""
    call = {AdaptiveStepsizeParams: "take_steps_adaptive", ConstantStepsizeParams: "take_steps_constant",
            MalitskyPockStepsizeParameters: "take_steps_malitsky_pock"}.get(type(policy))
    if call and hasattr(fleet, call) and os.environ.get("PDHG_PY_TAKE_STEP", "0") != "1":
        K = len(solves)
        slot = {id(mb): k for k, mb in enumerate(solves)}
        placed = [(slot[id(mb)], mb.state) for mb, _ in requests]
        ns = np.zeros(K, dtype=np.int64)
        for mb, steps in requests:
            ns[slot[id(mb)]] = steps
        ss, pw, it, kkt = _pack_step_states(K, placed)
        t0 = _time.time()
        if isinstance(policy, AdaptiveStepsizeParams):
            results = fleet.take_steps_adaptive(ns, policy.reduction_exponent, policy.growth_exponent, ss, pw, it, kkt)
            taken = _unpack_step_states(placed, *results)
        elif isinstance(policy, ConstantStepsizeParams):
            kkt, done = fleet.take_steps_constant(ns, ss, pw, kkt)
            for k, st in placed:
                st.cumulative_kkt_passes = float(kkt[k])
            taken = [int(done[k]) for k, _ in placed]
        else:
            if not all(mb.is_lp for mb, _ in requests):
                raise ValueError("Malitsky and Pock linesearch is only supported for "
                                 "linear programming problems.")
            ss, ratio, *results = fleet.take_steps_malitsky_pock(
                ns, policy.downscaling_factor, policy.breaking_factor, policy.interpolation_coefficient, ss,
                _pack_ratios(K, placed), pw, it, kkt)
            taken = _unpack_step_states(placed, ss, *results)
            for k, st in placed:
                st.ratio_step_sizes = float(ratio[k])
        dt = _time.time() - t0
        return [(mb, d, dt) for (mb, _), d in zip(requests, taken)]
    out = []
    for mb, steps in requests:
        t0 = _time.time()
        done = take_steps(policy, mb.state, steps, mb.is_lp)
        out.append((mb, done, _time.time() - t0))
    return out


def _fleet_checks(fleet, solves, pending):
    """One sweep of a round's checks (``_check_round``): the members' requests -- ``pending`` = [(solve, (method,
    arguments))] -- as ONE ``fleet.eval_points`` and / or ONE ``fleet.trust_region_bounds``.  The results stay with the
    members: each member's own evaluator call, which follows, finds them."""
    slot = {id(mb): k for k, mb in enumerate(solves)}
    points, items = _check_requests(pending, lambda mb: slot[id(mb)], len(solves))
    if (points >= 0).any():
        fleet.eval_points(points)
    if items:
        fleet.trust_region_bounds(items)


def optimize_many(params, problems, fleet_factory=None, initial_solutions=None):
    """``optimize(params, problems[k])`` for every k, side by side: a list of ``SaddlePointOutput`` in input order.

    Anything ``optimize`` accepts: any mix of shapes, LPs and QPs, every step-size policy, any number of problems (an
    empty list raises ``ValueError`` before any device work).  Small LPs share the launches of their steps; small QPs do
    with ``PDHG_SMALL_QP=1`` in the environment (the library partitions the members: no argument here), and are stepped
    member by member otherwise -- the results are the same bits either way.  ``fleet_factory(problems) -> fleet`` builds the device
    side (default ``HipPdhgFleet``): an object with ``.members`` (one engine per problem, in order), ``close()`` and,
    optionally, ``take_steps_adaptive`` / ``take_steps_constant`` / ``take_steps_malitsky_pock`` and the pair
    ``eval_points`` / ``trust_region_bounds`` (the checks in shared launches); a factory whose
    ``takes_original_problem`` is true receives the original problems and every member rescales on the device, any other
    one receives the host-rescaled problems.

    ``initial_solutions``: ``None`` (every problem starts from zeros, the path as it always was) or one entry per
    problem -- ``None`` or ``(x0, y0)``, a starting point in the original problem's space with ``optimize``'s
    semantics (``initial_primal_solution`` / ``initial_dual_solution``)."""
    problems = list(problems)
    if not problems:
        raise ValueError("optimize_many needs at least one problem")
    _check_inputs(params, problems)
    points = [None] * len(problems)
    if initial_solutions is not None:
        initial_solutions = list(initial_solutions)
        if len(initial_solutions) != len(problems):
            raise ValueError(f"initial_solutions has {len(initial_solutions)} entries for {len(problems)} problems")
        points = [None if pt is None else _initial_point(p, *pt) for p, pt in zip(problems, initial_solutions)]
    policy = params.step_size_policy_params
    factory = fleet_factory or _default_fleet_factory
    fleet = None
    try:
        if _rescales_on_device(factory):
            fleet = factory(problems)
            factors, max_abs = _rescale_members(fleet, params)
            scaled = [_device_scaled_problem(p, eng, E, D) for p, eng, (E, D) in zip(problems, fleet.members, factors)]
        else:
            scaled, max_abs = zip(*[_host_scaled_problem(params, p) for p in problems])
            fleet = factory([s.scaled_qp for s in scaled])
        solves = [_Solve(params, p, s, eng, a) for p, s, eng, a in zip(problems, scaled, fleet.members, max_abs)]
        for mb, point in zip(solves, points):
            if point is not None:
                _set_initial_point(mb.engine, mb.scaled_problem, point)
        for mb in solves:
            mb.start(_constant_step_estimate(mb) if isinstance(policy, ConstantStepsizeParams) else None)
        checks = None
        if hasattr(fleet, "eval_points") and hasattr(fleet, "trust_region_bounds"):
            checks = lambda pending: _fleet_checks(fleet, solves, pending)      # noqa: E731
        return _drive_solves(solves, lambda requests: _step_fleet(fleet, solves, policy, requests), checks)
    finally:
        if fleet is not None and hasattr(fleet, "close"):
            fleet.close()
