"""A fleet's rescaling in one shared call, on the host: the two exports of include/pdhg_hip_fleet_rescale.h, and the
switch ``PDHG_FLEET_RESCALE=1`` in ``optimize_many`` and ``PdhgFleetSession`` through a fleet over CPU oracle engines
that counts calls -- switched on, a fleet with ``rescale`` gets ONE ``fleet.rescale`` (at create; after a matrix update,
one for the members given values) and no member ``rescale`` / ``matrix_max_abs``; switched off, or a fleet without the
method, the member calls exactly as before; the outputs are the same either way.

The counting engines take the ORIGINAL problem and rescale "on the device" -- on the host, by ``rescale_problem`` -- so
that the driver takes the route of ``HipPdhgFleet``; the scaled problem the driver then asks the engine for
(``_device_scaled_problem``: vectors only on the device) is the engine's full one here, which the host evaluator needs."""
import ctypes
import dataclasses
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import folp_loader

folp = folp_loader.load()
from firstorderlp_jl_amd import PdhgFleetSession, _lib, optimize_many  # noqa: E402
from firstorderlp_jl_amd import fleet as fleet_mod, session as session_mod  # noqa: E402
from firstorderlp_jl_amd.generators import random_lp  # noqa: E402
from firstorderlp_jl_amd.preprocess import rescale_problem  # noqa: E402
from firstorderlp_jl_amd.primal_dual_hybrid_gradient import optimize  # noqa: E402
from tests import helpers as H  # noqa: E402
from tests.helpers import ResolveOracleEngine, assert_same_output as _assert_same  # noqa: E402
from tests.oracle_engine import OracleEngine  # noqa: E402
from tests.test_matrix_update_host import _params  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ["pdhg_fleet_rescale", "pdhg_fleet_rescale_info"]
SWITCH = "PDHG_FLEET_RESCALE"


# ---- the exports ----

def test_the_header_declares_exactly_the_new_exports_and_the_library_has_them():
    header = open(os.path.join(ROOT, "include", "pdhg_hip_fleet_rescale.h")).read()
    declared = sorted(set(re.findall(r"\b(pdhg_[a-z_0-9]+)\s*\(", header)))
    assert declared == NEW_EXPORTS == sorted(_lib.FLEET_RESCALE_EXPORTS)
    L = ctypes.CDLL(_lib.LIB_PATH)       # loads without a GPU
    for name in declared:
        assert hasattr(L, name), f"{name} not exported by libpdhg_hip.so"
        assert getattr(_lib.lib(), name).argtypes, f"{name} is not bound in _lib"
    taken = set(_lib.EXPORTS + _lib.RESOLVE_EXPORTS + _lib.BATCH_RESOLVE_EXPORTS + _lib.MATRIX_UPDATE_EXPORTS +
                _lib.BATCH_CHECKS_EXPORTS)
    assert not set(NEW_EXPORTS) & taken
    assert _lib.lib().pdhg_abi_version() == _lib.ABI_VERSION == 11
    for name in ("pdhg_hip.h", "pdhg_hip_resolve.h", "pdhg_hip_batch_resolve.h", "pdhg_hip_matrix_update.h",
                 "pdhg_hip_batch_checks.h"):
        other = open(os.path.join(ROOT, "include", name)).read()
        assert not set(re.findall(r"\b(pdhg_[a-z_0-9]+)\s*\(", other)) & set(NEW_EXPORTS), name


def test_null_handles_are_refused_without_a_gpu():
    L = _lib.lib()
    info = np.zeros(4, dtype=np.int64)
    max_abs = np.zeros(3)
    assert L.pdhg_fleet_rescale(None, None, 10, 1, 1, 1.0, None, None, max_abs.ctypes.data_as(ctypes.POINTER(ctypes.c_double))) == -1
    assert b"null handle" in L.pdhg_last_error()
    assert L.pdhg_fleet_rescale_info(None, info.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))) == -1
    assert b"null handle" in L.pdhg_last_error()
    assert not info.any() and not max_abs.any()


# ---- the switch ----

class _RescalingEngine(ResolveOracleEngine):
    """An oracle engine created from the ORIGINAL problem that rescales itself, as ``HipPdhgEngine`` does on the device:
    ``rescale`` / ``matrix_max_abs`` / ``get_problem_vectors``, and the session's calls in the original problem's
    space.  Every ``rescale`` and ``matrix_max_abs`` a caller makes is logged with the member's index."""

    @classmethod
    def member(cls, k, problem, log):
        eng = cls.from_problem(problem)
        eng.k, eng.log, eng.original, eng.scaled, eng.args = k, log, problem, None, None
        return eng

    def _take(self, scaled):
        q = self.scaled = scaled
        q = q.scaled_qp
        self._A, self._Qm = q.constraint_matrix, q.objective_matrix
        self._vectors = [np.array(v, dtype=np.float64) for v in (q.objective_vector, q.right_hand_side,
                                                                 q.variable_lower_bound, q.variable_upper_bound)]
        self._rebuild()

    def quiet_rescale(self, l_inf_ruiz_iterations, l2_norm_rescaling, pock_chambolle_alpha):
        self.args = (l_inf_ruiz_iterations, l2_norm_rescaling, pock_chambolle_alpha)
        self._take(rescale_problem(*self.args, 0, self.original))
        return self.scaled.constraint_rescaling, self.scaled.variable_rescaling

    def quiet_max_abs(self):
        data = self._A.data
        return float(np.max(np.abs(data))) if len(data) else 0.0

    def retain_rescaling(self):
        self.log.append(("retain", self.k))

    def rescale(self, *args):
        self.log.append(("rescale", self.k))
        return self.quiet_rescale(*args)

    def matrix_max_abs(self):
        self.log.append(("matrix_max_abs", self.k))
        return self.quiet_max_abs()

    def get_problem_vectors(self):
        return tuple(v.copy() for v in self._vectors)

    def update_problem_vectors(self, objective_vector=None, right_hand_side=None, variable_lower_bound=None,
                               variable_upper_bound=None):
        given = {"objective_vector": objective_vector, "right_hand_side": right_hand_side,
                 "variable_lower_bound": variable_lower_bound, "variable_upper_bound": variable_upper_bound}
        self.original = dataclasses.replace(self.original, **{k: np.array(v, dtype=np.float64) for k, v in given.items()
                                                              if v is not None})
        self._take(rescale_problem(*self.args, 0, self.original))       # (the factors depend on the matrices alone)

    def update_matrix_values(self, constraint_matrix_values, objective_matrix_values, objective_vector, right_hand_side,
                             variable_lower_bound, variable_upper_bound):
        self.log.append(("update_matrix_values", self.k))
        A = self.original.constraint_matrix
        changes = {"constraint_matrix": sp.csc_matrix((np.array(constraint_matrix_values, dtype=np.float64), A.indices, A.indptr),
                                                      shape=A.shape)}
        if objective_matrix_values is not None:
            Q = self.original.objective_matrix
            changes["objective_matrix"] = sp.csc_matrix((np.array(objective_matrix_values, dtype=np.float64), Q.indices, Q.indptr),
                                                        shape=Q.shape)
        self.original = dataclasses.replace(self.original, objective_vector=objective_vector, right_hand_side=right_hand_side,
                                            variable_lower_bound=variable_lower_bound,
                                            variable_upper_bound=variable_upper_bound, **changes)

    def warm_start(self, x=None, y=None):
        s = self.scaled
        super().warm_start(None if x is None else x * s.variable_rescaling, None if y is None else y * s.constraint_rescaling)


class _PlainFleet:
    """``members`` and ``close``, nothing else: the fleet of the other CPU tests, over the rescaling engines."""
    takes_original_problem = True

    def __init__(self, problems):
        self.log = []
        self.members = [_RescalingEngine.member(k, p, self.log) for k, p in enumerate(problems)]

    def close(self):
        for eng in self.members:
            eng.close()


class _CountingFleet(_PlainFleet):
    """... with ``rescale``: logged, and served without a logged member call."""

    def rescale(self, l_inf_ruiz_iterations, l2_norm_rescaling, pock_chambolle_alpha, members=None):
        named = list(range(len(self.members))) if members is None else list(members)
        self.log.append(("fleet.rescale", tuple(named)))
        factors = [self.members[k].quiet_rescale(l_inf_ruiz_iterations, l2_norm_rescaling, pock_chambolle_alpha) for k in named]
        return factors, [self.members[k].quiet_max_abs() for k in named]


@pytest.fixture(autouse=True)
def _full_scaled_problem(monkeypatch):
    for mod in (fleet_mod, session_mod):
        monkeypatch.setattr(mod, "_device_scaled_problem", lambda problem, engine, E, D: engine.scaled)
    monkeypatch.delenv(SWITCH, raising=False)
    monkeypatch.delenv("PDHG_HOST_RESCALE", raising=False)


def _problems():
    return [H.example_lp(), H.example_qp(), random_lp(27, 32, 4, seed=1), H.example_lp_dependent_rows()]


def _solve(factory, monkeypatch, switch):
    fleets = []

    def build(problems):
        fleets.append(factory(problems))
        return fleets[-1]
    build.takes_original_problem = True
    if switch is None:
        monkeypatch.delenv(SWITCH, raising=False)
    else:
        monkeypatch.setenv(SWITCH, switch)
    out = optimize_many(_params(), _problems(), fleet_factory=build)
    return out, fleets[-1].log


def _member_calls(K):
    return [(call, k) for k in range(K) for call in ("rescale", "matrix_max_abs")]


def test_switched_on_optimize_many_makes_one_fleet_rescale_and_no_member_rescale(monkeypatch):
    problems = _problems()
    want = [optimize(_params(), p, OracleEngine.from_problem) for p in problems]
    got, log = _solve(_CountingFleet, monkeypatch, "1")
    assert log == [("fleet.rescale", tuple(range(len(problems))))]
    for g, w in zip(got, want):
        _assert_same(g, w)


@pytest.mark.parametrize("value", [None, "0", ""], ids=["unset", "zero", "empty"])
def test_switched_off_the_member_calls_are_made_as_before_and_the_outputs_are_the_same(value, monkeypatch):
    on, _ = _solve(_CountingFleet, monkeypatch, "1")
    off, log = _solve(_CountingFleet, monkeypatch, value)
    assert log == _member_calls(len(on))
    for g, w in zip(off, on):
        _assert_same(g, w)


def test_a_fleet_without_the_method_is_driven_as_before(monkeypatch):
    on, _ = _solve(_CountingFleet, monkeypatch, "1")
    got, log = _solve(_PlainFleet, monkeypatch, "1")
    assert log == _member_calls(len(on))
    for g, w in zip(got, on):
        _assert_same(g, w)


def _session_run(factory, monkeypatch, switch):
    """Create, solve, a matrix update on members 0 and 2 with a vector update on member 3, solve: (outputs, log)."""
    if switch is None:
        monkeypatch.delenv(SWITCH, raising=False)
    else:
        monkeypatch.setenv(SWITCH, switch)
    problems = _problems()
    with PdhgFleetSession(_params(), problems, factory) as session:
        first = session.solve()
        updates = [None] * len(problems)
        for k in (0, 2):
            A = problems[k].constraint_matrix
            updates[k] = {"constraint_matrix_values": A.data * (1.0 + 0.05 * np.cos(np.arange(A.nnz)))}
        updates[3] = {"right_hand_side": problems[3].right_hand_side * 1.25}
        session.update(updates)
        second = session.solve(warm_start=True)
        return first + second, list(session.fleet.log)


def test_a_fleet_session_rescales_in_one_call_at_create_and_after_a_matrix_update(monkeypatch):
    K = len(_problems())
    on, log_on = _session_run(_CountingFleet, monkeypatch, "1")
    retains = [("retain", k) for k in range(K)]
    assert log_on == retains + [("fleet.rescale", tuple(range(K))), ("update_matrix_values", 0), ("update_matrix_values", 2),
                                ("fleet.rescale", (0, 2))]
    for factory, switch in ((_CountingFleet, None), (_CountingFleet, "0"), (_PlainFleet, "1")):
        off, log_off = _session_run(factory, monkeypatch, switch)
        create = [entry for k in range(K) for entry in (("retain", k), ("rescale", k), ("matrix_max_abs", k))]
        update = [entry for k in (0, 2) for entry in (("update_matrix_values", k), ("rescale", k), ("matrix_max_abs", k))]
        assert log_off == create + update, (factory.__name__, switch)
        assert len(off) == len(on) == 2 * K
        for g, w in zip(off, on):
            _assert_same(g, w)
