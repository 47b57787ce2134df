"""Re-solves on a live handle: the same matrix again and again with other vectors, starting near the last answer.

``optimize`` creates the device state, rescales, solves and frees everything.  A model-predictive controller with a new
right-hand side every tick, branch-and-bound nodes that differ in a few bounds, a scenario set or a regularization path
would repeat the create and the rescaling -- layout builders, create-time kernel timing, a dozen rescaling passes over
every copy of the matrix -- for work that depends on the matrix only.  A session does that work once:

    with PdhgSession(params, problem) as session:
        first = session.solve()
        session.update(right_hand_side=b_next)
        second = session.solve(warm_start=True)        # from the first solve's solution

``PdhgSession.solve()`` returns what ``optimize(params, <the problem as updated>)`` returns, bit for bit -- and
``solve(warm_start=(x0, y0))`` what ``optimize(..., initial_primal_solution=x0, initial_dual_solution=y0)`` returns: the
library replays the recorded rescaling steps on the new vectors (include/pdhg_hip_resolve.h) and empties everything a
fresh handle has empty.  ``PdhgFleetSession`` is the same over a fleet (``fleet.optimize_many``): updates and warm starts
of all members in one launch each, and ``PdhgBatchSession`` over a batch (``batch.optimize_batch``): problems that share
the matrix share the record of its rescaling too (include/pdhg_hip_batch_resolve.h).

The reference has no warm start: a warm solve differs from a cold one in the starting point alone (see ``optimize``).
"""
import copy
import dataclasses

import numpy as np
import scipy.sparse as sp

from .batch import _checks_hook, _default_batch_factory, _step_batch, check_batch
from .fleet import _default_fleet_factory, _fleet_checks, _fleet_rescales, _rescale_members, _step_fleet
from .preprocess import validate
from .quadratic_programming import as_csc
from .primal_dual_hybrid_gradient import (AdaptiveStepsizeParams, ConstantStepsizeParams, _check_inputs, _constant_step_estimate,
                                          _default_engine_factory, _device_scaled_problem, _drive_solve, _drive_solves,
                                          _host_scaled_problem, _initial_point, _rescales_on_device, _Solve)

_UPDATE_FIELDS = ("objective_vector", "right_hand_side", "variable_lower_bound", "variable_upper_bound")
# new matrix ENTRIES on the kept sparsity pattern: {the problem's field (also the key that takes a whole matrix): the key that takes its values}
_MATRIX_FIELDS = {"constraint_matrix": "constraint_matrix_values", "objective_matrix": "objective_matrix_values"}


def _has_objective_matrix(problem):
    """Does an engine created from ``problem`` hold an objective matrix?  (An all-zero one is an LP to the library.)"""
    return bool(np.any(problem.objective_matrix.data != 0.0))


def _matrix_with_values(problem, field, values, matrix):
    """``problem``'s matrix ``field`` with new values on the same pattern: ``values`` in the order of its ``data`` (the
    canonical CSC the problem keeps), or ``matrix``, canonicalised the same way, whose pattern must be the same."""
    old, name = getattr(problem, field), _MATRIX_FIELDS[field]
    if values is not None and matrix is not None:
        raise ValueError(f"give {name} or {field}, not both")
    if matrix is not None:
        name = field
        new = as_csc(matrix, old.shape)
        if not np.array_equal(new.indptr, old.indptr):
            column = int(np.nonzero(np.diff(new.indptr) != np.diff(old.indptr))[0][0])
            raise ValueError(f"{field} has another sparsity pattern: column {column} holds {int(np.diff(new.indptr)[column])} "
                             f"stored entries, the session's {int(np.diff(old.indptr)[column])}")
        if not np.array_equal(new.indices, old.indices):
            at = int(np.nonzero(new.indices != old.indices)[0][0])
            column = int(np.searchsorted(old.indptr, at, side="right")) - 1
            raise ValueError(f"{field} has another sparsity pattern: column {column} holds other row indices")
        values = new.data
    values = np.array(values, dtype=np.float64).reshape(-1)
    if values.shape != old.data.shape:
        raise ValueError(f"{name} has shape {values.shape}, the pattern holds {old.data.shape} stored entries")
    if not np.all(np.isfinite(values)):
        raise ValueError(f"NaN or Inf found in {name}")
    if field == "objective_matrix":
        if not _has_objective_matrix(problem):
            raise ValueError(f"{name} on a problem without an objective matrix: an update cannot turn an LP into a QP")
        if not np.any(values != 0.0):
            raise ValueError(f"{name} are all zero: an update cannot turn a QP into an LP")
    return sp.csc_matrix((values, old.indices.copy(), old.indptr.copy()), shape=old.shape)


def _updated_problem(problem, objective_vector=None, right_hand_side=None, variable_lower_bound=None,
                     variable_upper_bound=None, constraint_matrix_values=None, objective_matrix_values=None,
                     constraint_matrix=None, objective_matrix=None):
    """``problem`` with the given vectors replaced -- and, on the same sparsity pattern, the given matrix values (explicit
    zeros among them stay stored entries) -- validated on the host (shapes and finite values, no objective-matrix values
    on an LP and no all-zero ones on a QP, ``validate``, no lower bound above its upper bound); ``problem`` itself is not
    touched.  Returns (updated problem, {field: new vector or matrix})."""
    given = {k: v for k, v in zip(_UPDATE_FIELDS, (objective_vector, right_hand_side, variable_lower_bound,
                                                   variable_upper_bound)) if v is not None}
    changes = {}
    for name, value in given.items():
        value = np.array(value, dtype=np.float64).reshape(-1)
        if value.shape != getattr(problem, name).shape:
            raise ValueError(f"{name} has shape {value.shape}, the problem needs {getattr(problem, name).shape}")
        changes[name] = value
    for field, values, matrix in (("constraint_matrix", constraint_matrix_values, constraint_matrix),
                                  ("objective_matrix", objective_matrix_values, objective_matrix)):
        if values is not None or matrix is not None:
            changes[field] = _matrix_with_values(problem, field, values, matrix)
    updated = dataclasses.replace(problem, **changes)
    validate(updated)
    if np.any(updated.variable_lower_bound > updated.variable_upper_bound):
        raise ValueError("the update leaves a variable_lower_bound above its variable_upper_bound")
    return updated, changes


def _matrix_changed(changes):
    return any(field in changes for field in _MATRIX_FIELDS)


def _warm_point(problem, warm_start, last):
    """``solve``'s ``warm_start`` argument as ``_initial_point``'s result: None (zeros), True (``last``, the previous
    solve's solution) or (x0, y0)."""
    if warm_start is None or warm_start is False:
        return None
    if warm_start is True:
        if last is None:
            raise ValueError("warm_start=True needs a solve before it")
        warm_start = last
    x0, y0 = warm_start
    return _initial_point(problem, x0, y0)


class _Member:
    """One problem of a session on its engine: created, retained, rescaled; its current problem and scaled problem."""

    def __init__(self, params, problem, engine, on_device, host_scaled=None, rescaled=None):
        self.params, self.problem, self.engine, self.on_device = params, problem, engine, on_device
        self.last = None
        self.estimate = None
        if rescaled is not None:
            # a batch member: its batch retained and rescaled for all members -- (E, D, matrix_max_abs)
            self.E, self.D, self.matrix_max_abs = rescaled
            self.scaled_problem = _device_scaled_problem(problem, engine, self.E, self.D)
            return
        if hasattr(engine, "retain_rescaling"):
            engine.retain_rescaling()
        if on_device:
            self.E, self.D = engine.rescale(params.l_inf_ruiz_iterations, params.l2_norm_rescaling,
                                            params.pock_chambolle_alpha)
            self.scaled_problem = _device_scaled_problem(problem, engine, self.E, self.D)
            self.matrix_max_abs = engine.matrix_max_abs()
        else:
            self.scaled_problem, self.matrix_max_abs = host_scaled

    def staged_update(self, **vectors):
        """The update checked and prepared on the host, nothing changed yet: (updated problem, changes, scaled problem
        of the host route or None)."""
        updated, changes = _updated_problem(self.problem, **vectors)
        host_scaled = None if self.on_device else _host_scaled_problem(self.params, updated)[0]
        return updated, changes, host_scaled

    def engine_vectors(self, changes, host_scaled):
        """What the engine's ``update_problem_vectors`` takes for ``changes``: the new vectors themselves on the device
        route (the library replays its rescaling on them), their host-rescaled form otherwise."""
        if self.on_device:
            return {k: changes.get(k) for k in _UPDATE_FIELDS}
        return {k: (getattr(host_scaled.scaled_qp, k) if k in changes else None) for k in _UPDATE_FIELDS}

    def update_matrix(self, updated, host_scaled, rescale=True):
        """New matrix values on the engine (``update_matrix_values``: every copy of every layout, the raw vectors), the
        rescaling run again as at create, and what depends on the matrix measured again; ``committed`` follows.
        ``rescale=False`` (device route): the group rescales its updated members in one call and hands each the result
        (``rescaled``)."""
        def q(problem):              # (an update keeps the class of the problem: the engine has Q where `updated` has)
            return problem.objective_matrix.data if _has_objective_matrix(updated) else None
        if self.on_device:
            self.engine.update_matrix_values(updated.constraint_matrix.data, q(updated), updated.objective_vector,
                                             updated.right_hand_side, updated.variable_lower_bound,
                                             updated.variable_upper_bound)
            if rescale:
                self.rescaled(self.engine.rescale(self.params.l_inf_ruiz_iterations, self.params.l2_norm_rescaling,
                                                  self.params.pock_chambolle_alpha), self.engine.matrix_max_abs())
        else:
            # the host route: the engine lives in the host-rescaled problem's space and is not rescaled
            sq = host_scaled.scaled_qp
            self.engine.update_matrix_values(sq.constraint_matrix.data, q(sq), sq.objective_vector, sq.right_hand_side,
                                             sq.variable_lower_bound, sq.variable_upper_bound)
            data = sq.constraint_matrix.data
            self.matrix_max_abs = float(np.max(np.abs(data))) if len(data) else 0.0
        self.estimate = None                 # the constant policy's power method sees the matrix: it runs again

    def rescaled(self, factors, matrix_max_abs):
        """What the engine's rescaling returned: ``(E, D)`` and max |a| of the scaled matrix."""
        (self.E, self.D), self.matrix_max_abs = factors, matrix_max_abs

    def apply(self, updated, changes, host_scaled):
        """One member's staged update on its own engine."""
        if _matrix_changed(changes):
            self.update_matrix(updated, host_scaled)
        elif changes:
            self.engine.update_problem_vectors(**self.engine_vectors(changes, host_scaled))

    def committed(self, updated, host_scaled):
        self.problem = updated
        if self.on_device:
            self.scaled_problem = _device_scaled_problem(updated, self.engine, self.E, self.D)
        else:
            self.scaled_problem = host_scaled

    def engine_point(self, point):
        """``point`` (original space) as the engine's ``warm_start`` takes it: the library scales on the device route."""
        x0, y0 = point if point is not None else (None, None)
        if self.on_device:
            return x0, y0
        sp = self.scaled_problem
        return (None if x0 is None else x0 * sp.variable_rescaling, None if y0 is None else y0 * sp.constraint_rescaling)

    def new_solve(self):
        """A fresh host-side solve on the live engine (host state, ``qp_cache``, evaluator, primal weight from the
        current scaled vectors), started; the engine has been warm-started."""
        solve = _Solve(self.params, self.problem, self.scaled_problem, self.engine, self.matrix_max_abs)
        if isinstance(self.params.step_size_policy_params, ConstantStepsizeParams):
            # the power method sees the matrix only: estimated once; its passes count in every solve, as in a fresh one
            if self.estimate is None:
                self.estimate = _constant_step_estimate(solve)
            solve.start(self.estimate)
        else:
            solve.start(None)
        return solve

    def solved(self, output):
        self.last = (output.primal_solution, output.dual_solution)
        return output


class _Session:
    """What the three sessions share: ``_held`` -- the member, or the list of members; None once closed -- and ``_owner``,
    whatever ``close`` has to close (the engine, the fleet, the batch)."""

    _held = _owner = None

    def _live(self):
        if self._held is None:
            raise RuntimeError("the session is closed")
        return self._held

    def close(self):
        owner, self._owner, self._held = self._owner, None, None
        if owner is not None and hasattr(owner, "close"):
            owner.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PdhgSession(_Session):
    """One problem kept on the device across solves.

    ``PdhgSession(params, problem, engine_factory=None)`` creates the engine, retains the rescaling steps, rescales and
    measures the matrix once.  ``engine_factory`` as in ``optimize``; an engine of another kind must offer
    ``update_problem_vectors(objective_vector, right_hand_side, variable_lower_bound, variable_upper_bound)`` and
    ``warm_start(x, y)`` in ITS problem's space (a factory that does not rescale on the device gets host-rescaled
    vectors and points) -- and, for updates of the matrix values, ``update_matrix_values(constraint_matrix_values,
    objective_matrix_values, objective_vector, right_hand_side, variable_lower_bound, variable_upper_bound)`` in that
    space too: the values in the order of the ``data`` of the matrices it was created from (``None`` for the objective
    matrix of an LP) and all four vectors; an engine that rescales on the device is rescaled again afterwards."""

    def __init__(self, params, problem, engine_factory=None):
        _check_inputs(params, [problem])
        factory = engine_factory or _default_engine_factory
        self.params = params
        on_device = _rescales_on_device(factory)
        try:
            if on_device:
                self._owner = factory(problem)
                self._held = _Member(params, problem, self._owner, True)
            else:
                host_scaled = _host_scaled_problem(params, problem)
                self._owner = factory(host_scaled[0].scaled_qp)
                self._held = _Member(params, problem, self._owner, False, host_scaled)
        except Exception:
            self.close()
            raise

    @property
    def problem(self):
        """The problem as updated so far."""
        return self._live().problem

    @property
    def engine(self):
        return self._live().engine

    def update(self, objective_vector=None, right_hand_side=None, variable_lower_bound=None, variable_upper_bound=None,
               constraint_matrix_values=None, objective_matrix_values=None, constraint_matrix=None, objective_matrix=None):
        """New vectors of the problem (``None``: keep) and new matrix ENTRIES on the kept sparsity pattern:
        ``constraint_matrix_values`` / ``objective_matrix_values`` in the order of ``session.problem.constraint_matrix.data``
        / ``.objective_matrix.data`` (the canonical CSC the problem keeps; explicit zeros stay stored entries), or
        ``constraint_matrix`` / ``objective_matrix``, canonicalised the same way -- another pattern raises ``ValueError``
        naming the first column that differs.  After a matrix change the engine takes the new values in place, is
        rescaled again and its matrix measured again; no layout is built and nothing is allocated.  The updated problem
        is validated before any device work; if that raises, the session is as it was."""
        mb = self._live()
        updated, changes, host_scaled = mb.staged_update(
            objective_vector=objective_vector, right_hand_side=right_hand_side,
            variable_lower_bound=variable_lower_bound, variable_upper_bound=variable_upper_bound,
            constraint_matrix_values=constraint_matrix_values, objective_matrix_values=objective_matrix_values,
            constraint_matrix=constraint_matrix, objective_matrix=objective_matrix)
        mb.apply(updated, changes, host_scaled)
        mb.committed(updated, host_scaled)

    def solve(self, warm_start=None):
        """Solve the problem as updated so far: ``None`` from zeros, ``True`` from the previous solve's solution,
        ``(x0, y0)`` from that point (either may be ``None``: zeros).  Returns a ``SaddlePointOutput``."""
        mb = self._live()
        point = _warm_point(mb.problem, warm_start, mb.last)
        mb.engine.warm_start(*mb.engine_point(point))
        return mb.solved(_drive_solve(mb.new_solve()))


class _GroupSession(_Session):
    """A session over a group of problems on one owner (a fleet, a batch): ``update`` and the front half of ``solve``.
    A subclass opens the group in its ``__init__`` (``_owner``, ``_held``), says in ``_group_takes(call, members)``
    whether the owner itself takes the members' ``update_problem_vectors`` / ``warm_start`` calls (original-space
    vectors, one launch each) and drives the started solves in ``_drive(members)``."""

    @property
    def problems(self):
        return [mb.problem for mb in self._live()]

    def _group(self):
        self._live()
        return self._owner

    def update(self, updates):
        """``updates``: one entry per problem -- ``None`` (keep the problem) or a dict with any of ``objective_vector``,
        ``right_hand_side``, ``variable_lower_bound``, ``variable_upper_bound`` and, where the group takes them
        (``PdhgSession.update``), the matrix keys.  A member with new matrix values is served on its own engine -- it
        has a matrix of its own and rescales alone, as at create (with ``PDHG_FLEET_RESCALE=1`` and a fleet that offers
        ``rescale``: those members in one call, after their placements); the others still ride the shared vector launch.
        Every updated problem is validated before any device work; if one raises, the session is as it was."""
        members = self._live()
        updates = list(updates)
        if len(updates) != len(members):
            raise ValueError(f"updates has {len(updates)} entries for {len(members)} problems")
        self._check_update_keys(updates)
        staged = [None if u is None else mb.staged_update(**u) for mb, u in zip(members, updates)]
        changed = [k for k, st in enumerate(staged) if st is not None and _matrix_changed(st[1])]
        shared = [k for k in changed if members[k].on_device] if self._group_takes("rescale", members) else []
        for k in changed:
            members[k].update_matrix(staged[k][0], staged[k][2], rescale=k not in shared)
        if shared:       # the members given matrix values rescale in one call, after their placements
            for k, factors, max_abs in zip(shared, *_rescale_members(self._owner, self.params, shared)):
                members[k].rescaled(factors, max_abs)
        vectors = [None if st is None or not st[1] or _matrix_changed(st[1]) else mb.engine_vectors(st[1], st[2])
                   for mb, st in zip(members, staged)]
        if any(v is not None for v in vectors):
            if self._group_takes("update_problem_vectors", members):
                self._owner.update_problem_vectors(*[[None if v is None else v[k] for v in vectors] for k in _UPDATE_FIELDS])
            else:
                for mb, v in zip(members, vectors):
                    if v is not None:
                        mb.engine.update_problem_vectors(**v)
        for mb, st in zip(members, staged):
            if st is not None:
                mb.committed(st[0], st[2])

    def _check_update_keys(self, updates):
        """(a group that cannot take every key of ``update`` says so here, before anything is staged)"""

    def solve(self, warm_start=None):
        """Solve every problem as updated so far; returns what the group's one-shot driver (``optimize_many``,
        ``optimize_batch``) returns.  ``warm_start``: ``None`` (everyone from zeros), ``True`` (everyone from its
        previous solution) or a list with one entry per problem -- ``None`` (zeros) or ``(x0, y0)``."""
        members = self._live()
        if warm_start is None or warm_start is True:
            warm_start = [warm_start] * len(members)
        warm_start = list(warm_start)
        if len(warm_start) != len(members):
            raise ValueError(f"warm_start has {len(warm_start)} entries for {len(members)} problems")
        points = [mb.engine_point(_warm_point(mb.problem, w, mb.last)) for mb, w in zip(members, warm_start)]
        if self._group_takes("warm_start", members):
            if all(x is None and y is None for x, y in points):
                self._owner.warm_start(None, None)
            else:
                # a member whose two entries are None would be left as it is: zeros are given as zeros
                xs = [np.zeros(mb.engine.n) if x is None and y is None else x for mb, (x, y) in zip(members, points)]
                self._owner.warm_start(xs, [y for _, y in points])
        else:
            for mb, (x, y) in zip(members, points):
                mb.engine.warm_start(x, y)
        return [mb.solved(out) for mb, out in zip(members, self._drive(members))]


class PdhgFleetSession(_GroupSession):
    """Many independent problems kept on the device across solves: ``PdhgSession`` over a fleet
    (``fleet.optimize_many``).  A fleet with ``update_problem_vectors`` / ``warm_start`` of its own (``HipPdhgFleet``)
    takes the updates and the warm starts of all members in one launch each; any other fleet member by member."""

    def __init__(self, params, problems, fleet_factory=None):
        problems = list(problems)
        if not problems:
            raise ValueError("a fleet session needs at least one problem")
        _check_inputs(params, problems)
        factory = fleet_factory or _default_fleet_factory
        self.params = params
        members = None
        try:
            # the members rescale one by one (_Member): each has a matrix of its own -- or, with PDHG_FLEET_RESCALE=1
            # and a fleet that offers it, in one fleet.rescale after every member has retained
            if _rescales_on_device(factory):
                self._owner = factory(problems)
                if _fleet_rescales(self._owner):
                    for eng in self._owner.members:
                        if hasattr(eng, "retain_rescaling"):
                            eng.retain_rescaling()
                    factors, max_abs = _rescale_members(self._owner, params)
                    members = [_Member(params, p, eng, True, rescaled=(E, D, a))
                               for p, eng, (E, D), a in zip(problems, self._owner.members, factors, max_abs)]
                else:
                    members = [_Member(params, p, eng, True) for p, eng in zip(problems, self._owner.members)]
            else:
                host_scaled = [_host_scaled_problem(params, p) for p in problems]
                self._owner = factory([s.scaled_qp for s, _ in host_scaled])
                members = [_Member(params, p, eng, False, hs) for p, eng, hs in zip(problems, self._owner.members, host_scaled)]
            self._held = members
        except Exception:
            self.close()
            raise

    fleet = property(_GroupSession._group)

    def _group_takes(self, call, members):
        if call == "rescale":
            return _fleet_rescales(self._owner)
        return hasattr(self._owner, call)

    def _drive(self, members):
        fleet, policy = self._owner, self.params.step_size_policy_params
        solves = [mb.new_solve() for mb in members]
        checks = None
        if hasattr(fleet, "eval_points") and hasattr(fleet, "trust_region_bounds"):
            checks = lambda pending: _fleet_checks(fleet, solves, pending)      # noqa: E731
        return _drive_solves(solves, lambda requests: _step_fleet(fleet, solves, policy, requests), checks)


class PdhgBatchSession(_GroupSession):
    """Problems that share the constraint matrix (and the objective matrix) kept on the device across solves:
    ``PdhgSession`` over a batch (``batch.optimize_batch``, whose preconditions hold here: 1..32 problems, one matrix,
    the adaptive or the constant policy).  A batch with ``retain_rescaling`` / ``update_problem_vectors`` / ``warm_start``
    of its own (``HipPdhgBatch``) keeps one record of the rescaling for all members and takes the updates and the warm
    starts of all members in one launch each; a factory that does not rescale on the device, or any other batch, is
    served member by member through its engines' ``update_problem_vectors`` / ``warm_start``.  New matrix values on the
    kept sparsity pattern, one matrix for all problems, go through ``update_matrix``."""

    def __init__(self, params, problems, batch_factory=None):
        problems = check_batch(problems, params)
        _check_inputs(params, problems)
        policy = params.step_size_policy_params
        if not isinstance(policy, (AdaptiveStepsizeParams, ConstantStepsizeParams)):
            raise ValueError(f"a batch session does not support the step-size policy {type(policy).__name__}")
        factory = batch_factory or _default_batch_factory
        self.params = params
        self._estimate = None
        try:
            if _rescales_on_device(factory):
                # the batch rescales once, on the shared matrix, and hands (E, D, max_abs) to its members
                batch = self._owner = factory(problems)
                if hasattr(batch, "retain_rescaling"):
                    batch.retain_rescaling()
                E, D = batch.rescale(params.l_inf_ruiz_iterations, params.l2_norm_rescaling, params.pock_chambolle_alpha)
                max_abs = batch.members[0].matrix_max_abs()
                members = [_Member(params, p, eng, True, rescaled=(E.copy(), D.copy(), max_abs))
                           for p, eng in zip(problems, batch.members)]
            else:
                host_scaled = [_host_scaled_problem(params, p) for p in problems]
                batch = self._owner = factory([s.scaled_qp for s, _ in host_scaled])
                members = [_Member(params, p, eng, False, (s, host_scaled[0][1]))
                           for p, eng, (s, _) in zip(problems, batch.members, host_scaled)]
            self._held = members
        except Exception:
            self.close()
            raise

    batch = property(_GroupSession._group)

    def _check_update_keys(self, updates):
        # the members share one matrix, and its layouts are lent between their handles: new values for one member have
        # no meaning; new values for all of them go through update_matrix
        for k, u in enumerate(updates):
            given = [] if u is None else [key for pair in _MATRIX_FIELDS.items() for key in pair if u.get(key) is not None]
            if given:
                raise ValueError(f"updates[{k}] gives {given[0]}: a batch session cannot change matrix values per problem "
                                 "(its problems share one matrix): give the new values of all of them to update_matrix, "
                                 "or use PdhgSession / PdhgFleetSession")

    def update_matrix(self, constraint_matrix_values=None, objective_matrix_values=None, constraint_matrix=None,
                      objective_matrix=None, updates=None):
        """New ENTRIES of the one constraint matrix (and the one objective matrix) of all problems, on the kept sparsity
        pattern: values in the order of ``session.problems[0].constraint_matrix.data`` / ``.objective_matrix.data``, or
        whole matrices of the same pattern, with ``PdhgSession.update``'s checks (another pattern raises ``ValueError``
        naming the first column that differs; an LP stays an LP, a QP a QP).  ``updates``: optional vector updates per
        problem, as ``update`` takes them, applied in the same call.

        A batch that offers ``update_matrix_values`` (``HipPdhgBatch``) takes the values in place, once for all
        members, is rescaled again as at create -- the members' vectors come back in one launch -- and its matrix is
        measured again; no layout is built and nothing is allocated.  A batch without that call whose engines live in the
        host-rescaled space (a factory without ``takes_original_problem``: the oracle batches of the CPU tests) is served
        member by member through its engines' ``update_matrix_values``, in each engine's problem space
        (``PdhgSession``); any other batch raises ``ValueError`` before any work.  Every updated problem
        and the batch's preconditions (``check_batch``) are validated before any device work; if that raises, the
        session is as it was.  The solve that follows is ``optimize_batch`` on the updated problems, bit for bit."""
        members = self._live()
        matrix = {"constraint_matrix_values": constraint_matrix_values, "objective_matrix_values": objective_matrix_values,
                  "constraint_matrix": constraint_matrix, "objective_matrix": objective_matrix}
        if all(v is None for v in matrix.values()):
            raise ValueError("update_matrix needs new values of the constraint matrix or of the objective matrix "
                             "(new vectors alone go through update)")
        updates = [None] * len(members) if updates is None else list(updates)
        if len(updates) != len(members):
            raise ValueError(f"updates has {len(updates)} entries for {len(members)} problems")
        self._check_update_keys(updates)
        batch, params = self._owner, self.params
        group = self._group_takes("update_matrix_values", members) and hasattr(batch, "update_matrix_values")
        if not group:
            # member by member, in the host-rescaled space of each engine: nothing rescales such engines together
            if any(mb.on_device for mb in members):
                raise ValueError("this batch rescales on the device and offers no update_matrix_values for all its members: "
                                 "it cannot take new matrix values; open a new session")
            lacking = [k for k, mb in enumerate(members) if not hasattr(mb.engine, "update_matrix_values")]
            if lacking:
                raise ValueError(f"the engine of problem {lacking[0]} has no update_matrix_values, and the batch has none "
                                 "for all of them: this batch cannot take new matrix values; open a new session")
        given = [{k: v for k, v in (u or {}).items() if v is not None} for u in updates]
        # The matrix is checked and canonicalised ONCE, on problem 0 (the problems hold one matrix: check_batch said so when
        # the session was opened); the other problems take the same matrix objects and only their own vectors are staged.
        # A problem's constructor canonicalises both matrices again, and staging every problem through it made the tick
        # of an 8-member batch LONGER than optimize_batch again on two of three families
        # (profiles/batch_matrix_update_throughput.txt, section 1b).  The copies skip that constructor and nothing else:
        # their vectors were validated when they were last set, the matrices with problem 0, and check_batch follows.
        first = members[0].staged_update(**matrix, **given[0])
        shared = {field: first[1][field] for field in _MATRIX_FIELDS if field in first[1]}

        def staged_member(mb, vectors):
            updated, changes = _updated_problem(mb.problem, **vectors) if vectors else (copy.copy(mb.problem), {})
            for field, new in shared.items():
                setattr(updated, field, new)
            host_scaled = None if mb.on_device else _host_scaled_problem(mb.params, updated)[0]
            return updated, {**changes, **shared}, host_scaled
        staged = [first] + [staged_member(mb, vectors) for mb, vectors in zip(members[1:], given[1:])]
        check_batch([st[0] for st in staged], self.params)
        rescaling = (params.l_inf_ruiz_iterations, params.l2_norm_rescaling, params.pock_chambolle_alpha)
        if group:
            first = staged[0][0]
            q = first.objective_matrix.data if _has_objective_matrix(first) else None
            batch.update_matrix_values(first.constraint_matrix.data, q, *[[getattr(st[0], k) for st in staged] for k in _UPDATE_FIELDS])
            E, D = batch.rescale(*rescaling)
            max_abs = batch.members[0].matrix_max_abs()
            for mb in members:
                mb.rescaled((E.copy(), D.copy()), max_abs)
                mb.estimate = None
        else:
            for mb, (updated, _, host_scaled) in zip(members, staged):
                mb.update_matrix(updated, host_scaled)
        for mb, (updated, _, host_scaled) in zip(members, staged):
            mb.committed(updated, host_scaled)
        self._estimate = None                # the constant policy's power method sees the matrix: it runs again

    def _group_takes(self, call, members):
        return call != "rescale" and all(mb.on_device for mb in members) and hasattr(self._owner, "update_problem_vectors") and \
            hasattr(self._owner, "warm_start")

    def _drive(self, members):
        batch, policy = self._owner, self.params.step_size_policy_params
        solves = [_Solve(self.params, mb.problem, mb.scaled_problem, mb.engine, mb.matrix_max_abs) for mb in members]
        if isinstance(policy, ConstantStepsizeParams) and self._estimate is None:
            # the power method sees the matrix only: once per session, on member 0's operators (as optimize_batch runs
            # it); its passes count in every solve, as in a fresh one
            self._estimate = _constant_step_estimate(solves[0])
        for solve in solves:
            solve.start(self._estimate)
        return _drive_solves(solves, lambda requests: _step_batch(batch, policy, requests), _checks_hook(batch, solves))
