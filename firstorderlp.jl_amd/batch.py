"""Batched PDHG solves of LPs, or of QPs that share the objective matrix as well, over one constraint matrix.

``optimize_batch(params, problems)`` returns what ``optimize(params, problems[k])`` returns, for every k, while the
batch reads the matrix once per trial for all members (``pdhg_batch_trial_step``: member-interleaved iterates,
csrc/batch_kernels.hpp); a QP batch reads the objective matrix and its transpose once per trial as well.  The members run in lockstep on accepted steps: one batch iteration is one ``take_step``
of every active member; evaluations, restarts and primal-weight updates happen per member at the iterations
``optimize`` would use, with the same helpers; a member that terminates leaves the batch.  Both drivers run the same
per-problem solve object (``primal_dual_hybrid_gradient._Solve``): only the stepping between evaluations differs.

``HipPdhgBatch`` is the device side: one ``pdhg_handle`` that owns the matrix plus K member handles that borrow it
(``.members``: ``HipPdhgEngine`` views -- every single-LP method works on them).  With ``objective_matrix`` the members
are QPs that borrow one objective matrix too (``pdhg_batch_set_objective_matrix``).  With ``PDHG_BATCH_CHECKS=1`` the
members' check products and evaluations share launches (``point_products`` / ``eval_points``,
include/pdhg_hip_batch_checks.h; ``_batch_checks``); every member's own evaluator call still runs, and finds them.  A batch that is solved again and
again keeps its handle (``retain_rescaling`` / ``update_problem_vectors`` / ``warm_start``,
include/pdhg_hip_batch_resolve.h; ``session.PdhgBatchSession`` drives them) and takes new matrix values on the kept
sparsity pattern for all members at once (``update_matrix_values`` then ``rescale``,
include/pdhg_hip_batch_matrix_update.h; ``PdhgBatchSession.update_matrix``).
"""
import ctypes
import os
import time as _time

import numpy as np
import scipy.sparse as sp

from . import _lib
from .engine import _MemberEngine, _MemberOwner, _d, _i, _int_p, _pd, _pi
from .primal_dual_hybrid_gradient import (AdaptiveStepsizeParams, ConstantStepsizeParams,
                                          MalitskyPockStepsizeParameters, _check_inputs, _check_requests,
                                          _constant_step_estimate, _device_scaled_problem, _drive_solves,
                                          _host_scaled_problem, _initial_point, _pack_step_states,
                                          _rescales_on_device, _set_initial_point, _Solve, _unpack_step_states,
                                          adaptive_step_rule)

MAX_BATCH = 32


class _BatchMember(_MemberEngine):
    def rescale(self, *args, **kw):
        raise ValueError("a batch member shares its batch's matrix: rescale the batch")


class HipPdhgBatch(_MemberOwner):
    """K LPs with one constraint matrix on one GPU (``pdhg_create_batch``); with ``objective_matrix`` (n x n, the same
    for every member) K QPs."""

    def __init__(self, constraint_matrix, objective_vectors, right_hand_sides, variable_lower_bounds,
                 variable_upper_bounds, num_equalities, device_id=-1, stream=None, objective_matrix=None):
        self._L = _lib.lib()
        A = sp.csc_matrix(constraint_matrix)
        self.m, self.n = int(A.shape[0]), int(A.shape[1])
        c = _d(np.asarray(objective_vectors, dtype=np.float64))
        K = c.shape[0]
        if not 1 <= K <= MAX_BATCH:
            raise ValueError(f"a batch holds 1..{MAX_BATCH} problems, not {K}")
        b = _d(np.asarray(right_hand_sides, dtype=np.float64))
        lb = _d(np.asarray(variable_lower_bounds, dtype=np.float64))
        ub = _d(np.asarray(variable_upper_bounds, dtype=np.float64))
        if c.shape != (K, self.n) or lb.shape != (K, self.n) or ub.shape != (K, self.n) or b.shape != (K, self.m):
            raise ValueError("vector shapes do not match K members of the constraint matrix")
        colptr, rowval, nzval = _i(A.indptr), _i(A.indices), _d(A.data)
        h = ctypes.c_void_p()
        _lib.check(self._L.pdhg_create_batch(
            ctypes.byref(h), K, self.m, self.n, len(nzval), _pi(colptr), _pi(rowval), _pd(nzval), 0,
            _pd(c), _pd(b), _pd(lb), _pd(ub), int(num_equalities), int(device_id),
            ctypes.c_void_p(stream) if stream else None))
        self._h = h
        self.K = K
        self.members = []
        try:
            self.set_objective_matrix(objective_matrix)
        except Exception:
            self.close()
            raise
        for k in range(K):
            mh = ctypes.c_void_p()
            _lib.check(self._L.pdhg_batch_member(self._h, k, ctypes.byref(mh)))
            self.members.append(_BatchMember._wrap(self._L, mh, self.m, self.n))

    def set_objective_matrix(self, objective_matrix):
        """One objective matrix for every member (``pdhg_batch_set_objective_matrix``); ``None`` or no stored entry
        leaves the batch as it is, stored entries that are all 0.0 make it an LP batch (again)."""
        if objective_matrix is None:
            return
        Q = sp.csc_matrix(objective_matrix)
        if Q.shape != (self.n, self.n):
            raise ValueError(f"the objective matrix has shape {Q.shape}, not {(self.n, self.n)}")
        if Q.nnz == 0:
            return
        qc, qr, qv = _i(Q.indptr), _i(Q.indices), _d(Q.data)
        _lib.check(self._L.pdhg_batch_set_objective_matrix(self._h, len(qv), _pi(qc), _pi(qr), _pd(qv), 0))

    @classmethod
    def from_problems(cls, problems, **kw):
        check_batch(problems)
        p0 = problems[0]
        return cls(p0.constraint_matrix, [p.objective_vector for p in problems],
                   [p.right_hand_side for p in problems], [p.variable_lower_bound for p in problems],
                   [p.variable_upper_bound for p in problems], p0.num_equalities,
                   objective_matrix=_shared_q(p0), **kw)

    takes_original_problem = True

    def _mask(self, active):
        a = np.ones(self.K, dtype=np.int32) if active is None else np.asarray(active, dtype=np.int32).copy()
        if a.shape != (self.K,):
            raise ValueError("one mask entry per member")
        return a

    def rescale(self, l_inf_ruiz_iterations, l2_norm_rescaling, pock_chambolle_alpha):
        """``rescale_problem`` once on the shared matrix, applied to every member's vectors; returns
        (constraint_rescaling, variable_rescaling), the same for every member."""
        e, dvec = np.empty(self.m), np.empty(self.n)
        use_pc = pock_chambolle_alpha is not None
        _lib.check(self._L.pdhg_rescale(self._h, int(l_inf_ruiz_iterations), int(bool(l2_norm_rescaling)), int(use_pc),
                                        float(pock_chambolle_alpha) if use_pc else 0.0, _pd(e), _pd(dvec)))
        return e, dvec

    def trial_step(self, step_sizes, primal_weights, theta=1.0, active=None):
        """One trial of every active member: a (K, 5) array of ``pdhg_trial_step``'s sums (rows of inactive
        members are NaN)."""
        a = self._mask(active)
        ss, pw = _d(np.broadcast_to(step_sizes, (self.K,))), _d(np.broadcast_to(primal_weights, (self.K,)))
        out = np.full(5 * self.K, np.nan)
        _lib.check(self._L.pdhg_batch_trial_step(self._h, _pd(ss), _pd(pw), float(theta),
                                                 a.ctypes.data_as(_int_p), _pd(out)))
        return out.reshape(self.K, 5)

    def accept(self, accept, avg_weights):
        a = self._mask(accept)
        w = _d(np.broadcast_to(avg_weights, (self.K,)))
        _lib.check(self._L.pdhg_batch_accept(self._h, a.ctypes.data_as(_int_p), _pd(w)))

    def take_steps_adaptive(self, n_steps, reduction_exponent, growth_exponent, step_sizes, primal_weights,
                            total_number_iterations, cumulative_kkt_passes, active=None):
        """``n_steps`` take_steps of every active member in lockstep.  Returns arrays (step_sizes,
        total_number_iterations, cumulative_kkt_passes, numerical_error, steps_done)."""
        a = self._mask(active)
        return self._take_steps_adaptive(self._L.pdhg_batch_take_steps_adaptive, int(n_steps), reduction_exponent,
                                         growth_exponent, step_sizes, primal_weights, total_number_iterations,
                                         cumulative_kkt_passes, a.ctypes.data_as(_int_p))

    # ---- the checks in shared launches (include/pdhg_hip_batch_checks.h) ----
    def point_products(self, items):
        """A x, A' y (and Q x) at ``point`` of member ``k`` for every item ``(k, point)``, from one read of the matrix
        per point kind, into the members' own product caches: the members' ``eval_point`` / ``trust_region_bound(s)``
        at those points then launch no product.  At most ``3 * MAX_BATCH`` items."""
        items = list(items)
        if not items:
            return
        ks = np.ascontiguousarray([k for k, _ in items], dtype=np.int32)
        pts = np.ascontiguousarray([p for _, p in items], dtype=np.int32)
        _lib.check(self._L.pdhg_batch_point_products(self._live(), len(items), ks.ctypes.data_as(_int_p),
                                                     pts.ctypes.data_as(_int_p)))

    def eval_points(self, points):
        """``members[k].eval_point(points[k])`` for every k (-1: member k is left alone, its row stays zeros), all
        members in shared launches: a (K, 24) array.  Every result is also left in its member: the member's own
        ``eval_point`` with the same point answers from it until the member's state moves."""
        pts = np.ascontiguousarray(np.broadcast_to(points, (self.K,)), dtype=np.int32)
        out = np.zeros((self.K, 24))
        _lib.check(self._L.pdhg_batch_eval_points(self._live(), pts.ctypes.data_as(_int_p), _pd(out)))
        return out

    def check_info(self):
        """``pdhg_batch_check_info`` as a dict: calls, items whose products rode a batched launch (``batched``), items
        with a product served by the member's own launch (``own``), items found ``cached``, members ``carried`` by
        ``eval_points``, member evaluations ``served`` from a stored result, ``misses`` (member evaluations that
        launched although the batch had been asked) and ``launches``; all since the batch was created."""
        info = np.zeros(8, dtype=np.int64)
        _lib.check(self._L.pdhg_batch_check_info(self._live(), _pi(info)))
        return dict(zip(["calls", "batched", "own", "cached", "carried", "served", "misses", "launches"], info.tolist()))

    # ---- re-solves on the batch handle (include/pdhg_hip_batch_resolve.h): ``_MemberOwner``'s, over these ----
    _noun, _resolve_other = "batch", "batched_product"

    def _resolve_calls(self):
        return (self._L.pdhg_batch_update_problem_vectors, self._L.pdhg_batch_warm_start, self._L.pdhg_batch_resolve_info)

    def retain_rescaling(self):
        """``pdhg_batch_resolve_retain``: to be called before ``rescale`` (and after the objective matrix is set).
        The batch keeps every rescaling step's factors once for all members (8 * steps * (n + m) bytes of device
        memory), which ``update_problem_vectors`` and ``warm_start`` need."""
        _lib.check(self._L.pdhg_batch_resolve_retain(self._live()))

    def update_matrix_values(self, constraint_matrix_values, objective_matrix_values, objective_vectors, right_hand_sides,
                             variable_lower_bounds, variable_upper_bounds):
        """``pdhg_batch_update_matrix_values`` (include/pdhg_hip_batch_matrix_update.h): new values of the shared
        constraint matrix in the order of the ``data`` the batch was created from, of the shared objective matrix
        likewise (``None`` on an LP batch), and the four vectors of every member's ORIGINAL problem (K x n or K x m, as
        in the constructor).  Call ``rescale`` next, as after create: until then every other call on the batch and on
        its members is refused.  After that ``rescale`` every device array holds, bit for bit, what a fresh batch
        created from the updated problems, retained and rescaled the same way holds."""
        h = self._live()
        a = _d(constraint_matrix_values).reshape(-1)
        q = None if objective_matrix_values is None else _d(objective_matrix_values).reshape(-1)
        ns, ms = [self.n] * self.K, [self.m] * self.K
        tables = []
        for name, rows, lens in (("objective_vectors", objective_vectors, ns), ("right_hand_sides", right_hand_sides, ms),
                                 ("variable_lower_bounds", variable_lower_bounds, ns),
                                 ("variable_upper_bounds", variable_upper_bounds, ns)):
            if rows is None or any(row is None for row in rows):
                raise ValueError(f"{name}: every member's vector is needed (the batch is rescaled afterwards)")
            tables.append(self._pointer_table(name, [_d(row) for row in rows], lens))
        _lib.check(self._L.pdhg_batch_update_matrix_values(h, len(a), _pd(a), 0 if q is None else len(q), _pd(q),
                                                           *[t for t, _ in tables]))


def _shared_q(problem):
    """A problem's objective matrix in canonical CSC form (duplicates summed, indices sorted), or None for an LP: no
    matrix, no stored entry, or stored entries that are all 0.0."""
    Q = problem.objective_matrix
    if Q is None or Q.nnz == 0:
        return None
    Q = sp.csc_matrix(Q, copy=True)
    Q.sum_duplicates()
    Q.sort_indices()
    return Q if np.any(Q.data != 0) else None


def check_batch(problems, params=None):
    """The batch's preconditions, checked before any device work (ValueError): 1..32 problems, no Malitsky-Pock, one
    constraint matrix, one ``num_equalities``, and either LPs throughout or QPs with one objective matrix."""
    problems = list(problems)
    if not 1 <= len(problems) <= MAX_BATCH:
        raise ValueError(f"optimize_batch takes 1..{MAX_BATCH} problems, not {len(problems)}")
    if params is not None and isinstance(params.step_size_policy_params, MalitskyPockStepsizeParameters):
        raise ValueError("optimize_batch supports the adaptive and constant step-size policies, not Malitsky-Pock")
    A0 = sp.csc_matrix(problems[0].constraint_matrix)
    A0.sort_indices()
    Q0 = _shared_q(problems[0])
    for k, p in enumerate(problems):
        Q = _shared_q(p) if k else Q0
        if (Q is None) != (Q0 is None):
            raise ValueError(f"problem {k} is {'an LP' if Q is None else 'a QP'}, problem 0 "
                             f"{'an LP' if Q0 is None else 'a QP'}: a batch holds LPs only or QPs that share one objective matrix")
        if Q is not None and k:
            if Q.shape != Q0.shape:
                raise ValueError(f"problem {k}'s objective matrix has shape {Q.shape}, problem 0's {Q0.shape}")
            if not (np.array_equal(Q.indptr, Q0.indptr) and np.array_equal(Q.indices, Q0.indices)):
                raise ValueError(f"problem {k}'s objective matrix has another sparsity pattern than problem 0's")
            if not np.array_equal(Q.data, Q0.data):
                raise ValueError(f"problem {k}'s objective matrix has other values than problem 0's")
        if int(p.num_equalities) != int(problems[0].num_equalities):
            raise ValueError(f"problem {k} has num_equalities {p.num_equalities}, problem 0 {problems[0].num_equalities}")
        if k == 0:
            continue
        A = sp.csc_matrix(p.constraint_matrix)
        if A.shape != A0.shape:
            raise ValueError(f"problem {k}'s constraint matrix has shape {A.shape}, problem 0's {A0.shape}")
        A.sort_indices()
        if not (np.array_equal(A.indptr, A0.indptr) and np.array_equal(A.indices, A0.indices)):
            raise ValueError(f"problem {k}'s constraint matrix has another sparsity pattern than problem 0's")
        if not np.array_equal(A.data, A0.data):
            raise ValueError(f"problem {k}'s constraint matrix has other values than problem 0's")
    return problems


def _default_batch_factory(problems):
    return HipPdhgBatch.from_problems(problems)


_default_batch_factory.takes_original_problem = True


def _take_steps_python(batch, members, n_steps, policy):
    """The lockstep loop of pdhg_batch_take_steps_adaptive (and the constant policy's) through the batch's trial /
    accept calls: for batches without a native multi-step call."""
    K = len(batch.members)
    slot = [_slot(batch, mb) for mb in members]
    live = {k: mb for k, mb in zip(slot, members)}
    done = {k: 0 for k in slot}
    for _ in range(n_steps):
        if not live:
            break
        entry = {k: mb.state.step_size for k, mb in live.items()}
        need = dict(live)
        while need:
            mask = np.zeros(K, dtype=np.int32)
            ss, pw = np.ones(K), np.ones(K)
            for k, mb in need.items():
                mask[k] = 1
                ss[k], pw[k] = mb.state.step_size, mb.state.primal_weight
                if isinstance(policy, AdaptiveStepsizeParams):
                    mb.state.total_number_iterations += 1
            raw = batch.trial_step(ss, pw, 1.0, mask)
            acc = np.zeros(K, dtype=np.int32)
            for k in list(need):
                st = need[k].state
                st.cumulative_kkt_passes += 1
                if not isinstance(policy, AdaptiveStepsizeParams):
                    acc[k] = 1
                    done[k] += 1
                    del need[k]
                    continue
                accept, numerical_error, st.step_size = adaptive_step_rule(
                    raw[k], st.primal_weight, st.step_size, st.total_number_iterations, policy)
                if numerical_error:
                    st.numerical_error = True
                    del live[k]
                if accept or numerical_error:
                    acc[k] = int(accept)
                    done[k] += 1
                    del need[k]
            weights = np.ones(K)
            for k in range(K):
                if acc[k]:
                    weights[k] = entry[k]
            batch.accept(acc, weights)
    return [done[k] for k in slot]


def _slot(batch, member):
    return next(k for k, e in enumerate(batch.members) if e is member.engine)


def _take_steps(batch, members, n_steps, policy):
    """``n_steps`` take_steps of every member in ``members`` (lockstep); returns the steps each took."""
    if (isinstance(policy, AdaptiveStepsizeParams) and isinstance(batch, HipPdhgBatch)
            and os.environ.get("PDHG_PY_TAKE_STEP", "0") != "1"):
        placed = [(_slot(batch, mb), mb.state) for mb in members]
        mask = np.zeros(batch.K, dtype=np.int32)
        mask[[k for k, _ in placed]] = 1
        return _unpack_step_states(placed, *batch.take_steps_adaptive(
            n_steps, policy.reduction_exponent, policy.growth_exponent, *_pack_step_states(batch.K, placed), mask))
    return _take_steps_python(batch, members, n_steps, policy)


def _step_batch(batch, policy, requests):
    """``_drive_solves``' step for the solves of a batch: lockstep -- the members that named the same step count step
    together, the smaller counts first.  Returns (solve, steps taken, seconds) per request."""
    groups = {}
    for mb, steps in requests:
        groups.setdefault(steps, []).append(mb)
    out = []
    for steps, group in sorted(groups.items()):
        t0 = _time.time()
        done = _take_steps(batch, group, steps, policy)
        dt = _time.time() - t0
        out.extend((mb, d, dt) for mb, d in zip(group, done))
    return out


def _batch_checks(batch, solves, pending):
    """One sweep of a round's checks (``_check_round``), the counterpart of ``fleet._fleet_checks``: the members'
    ``"iteration_stats"`` requests as ONE ``batch.eval_points``, and the points that their ``"bounds"`` requests'
    trust-region problems name as ONE ``batch.point_products``.  The results stay with the members: each member's own
    evaluator call, which follows unchanged, finds them.  (The searches themselves stay per member.)"""
    points, tr_items = _check_requests(pending, lambda mb: _slot(batch, mb), len(batch.members))
    items = list(dict.fromkeys((k, int(point)) for k, point, *_ in tr_items))       # each once, first seen first
    if (points >= 0).any():
        batch.eval_points(points)
    if items:
        batch.point_products(items)


def _checks_hook(batch, solves):
    """``_drive_solves``' ``checks`` for a batch: ``_batch_checks`` when the batch offers both calls and
    ``PDHG_BATCH_CHECKS=1`` is set (read at every solve; off by default: the path is new), else None -- every member
    checks on its own, as before."""
    if os.environ.get("PDHG_BATCH_CHECKS", "0") != "1":
        return None
    if not (hasattr(batch, "eval_points") and hasattr(batch, "point_products")):
        return None
    return lambda pending: _batch_checks(batch, solves, pending)


def _initial_points(problems, initial_solutions):
    """``initial_solutions`` of ``optimize_batch`` checked on the host: one ``_initial_point`` result per problem."""
    if initial_solutions is None:
        return [None] * len(problems)
    initial_solutions = list(initial_solutions)
    if len(initial_solutions) != len(problems):
        raise ValueError(f"initial_solutions has {len(initial_solutions)} entries for {len(problems)} problems")
    return [None if pt is None else _initial_point(p, *pt) for p, pt in zip(problems, initial_solutions)]


def optimize_batch(params, problems, batch_factory=None, initial_solutions=None):
    """``optimize(params, problems[k])`` for every k, as one batch: a list of ``SaddlePointOutput`` in input order.

    The problems must share the constraint matrix (shape, pattern, values) and ``num_equalities``, and be LPs
    throughout or QPs that share the objective matrix as well (model-predictive control, a portfolio frontier, a
    ridge or elastic-net path: c, b and the bounds differ, Q and A do not);
    ``batch_factory(problems) -> batch`` builds the device side (default ``HipPdhgBatch``; a factory whose
    ``takes_original_problem`` is true receives the original problems and rescales on the device, any other one
    receives the host-rescaled problems, whose scaled objective matrices are one matrix again).  Malitsky-Pock, a mix
    of LPs and QPs, QPs with different objective matrices, an empty list or more than 32 problems raise ``ValueError``
    before any device work.

    ``initial_solutions``: ``None`` (every problem starts from zeros, the path as it always was) or one entry per
    problem -- ``None`` or ``(x0, y0)``, a starting point in the original problem's space with ``optimize``'s
    semantics (``initial_primal_solution`` / ``initial_dual_solution``), checked before any device work.
    ``session.PdhgBatchSession`` keeps the batch across solves.

    Measured on one MI355X (README, "Batched solves"; ``profiles/batch_qp_throughput.txt``): at K = 8 a QP batch of
    ``generators.random_qp_family`` runs 1.19x the solo QP handle's member-iterations/s at 10M x 10M and 1.48x at
    1M x 1M; at 10M x 10M, K = 16 is no gain (0.98x)."""
    problems = check_batch(problems, params)
    _check_inputs(params, problems)
    policy = params.step_size_policy_params
    if not isinstance(policy, (AdaptiveStepsizeParams, ConstantStepsizeParams)):
        raise ValueError(f"optimize_batch does not support the step-size policy {type(policy).__name__}")
    points = _initial_points(problems, initial_solutions)
    factory = batch_factory or _default_batch_factory
    batch = None
    try:
        if _rescales_on_device(factory):
            batch = factory(problems)
            E, D = batch.rescale(params.l_inf_ruiz_iterations, params.l2_norm_rescaling, params.pock_chambolle_alpha)
            matrix_max_abs = batch.members[0].matrix_max_abs()
            scaled = [_device_scaled_problem(p, eng, E.copy(), D.copy()) for p, eng in zip(problems, batch.members)]
        else:
            scaled, max_abs = zip(*[_host_scaled_problem(params, p) for p in problems])
            matrix_max_abs = max_abs[0]
            batch = factory([s.scaled_qp for s in scaled])
        members = [_Solve(params, p, s, eng, matrix_max_abs) for p, s, eng in zip(problems, scaled, batch.members)]
        for mb, point in zip(members, points):
            if point is not None:
                _set_initial_point(mb.engine, mb.scaled_problem, point)

        # the constant policy's power method depends on the matrix only: run once, on member 0's operators
        estimate = _constant_step_estimate(members[0]) if isinstance(policy, ConstantStepsizeParams) else None
        for mb in members:
            mb.start(estimate)

        return _drive_solves(members, lambda requests: _step_batch(batch, policy, requests), _checks_hook(batch, members))
    finally:
        if batch is not None and hasattr(batch, "close"):
            batch.close()
