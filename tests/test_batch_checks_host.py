"""A batch's checks in shared launches, on the host: the three exports of include/pdhg_hip_batch_checks.h, and the
driver's hook (``batch._batch_checks``) through a recording batch over CPU oracle engines -- with ``PDHG_BATCH_CHECKS=1``
every sweep of a round makes one ``eval_points`` with exactly the active members' points and one ``point_products`` with
the points the bounds requests name; with the switch off, or a batch without the methods, no such call; the outputs are
the same either way."""
import ctypes
import os
import re

import numpy as np
import pytest

import folp_loader

folp = folp_loader.load()
from firstorderlp_jl_amd import PdhgBatchSession, _lib, optimize_batch  # noqa: E402
from firstorderlp_jl_amd import primal_dual_hybrid_gradient as pdhg  # noqa: E402
from firstorderlp_jl_amd.evaluation import POINT_AVERAGE, POINT_CURRENT, POINT_RESTART  # noqa: E402
from firstorderlp_jl_amd.primal_dual_hybrid_gradient import (AdaptiveStepsizeParams, ConstantStepsizeParams,  # noqa: E402
                                                             optimize)
from tests.helpers import ResolveOracleEngine  # noqa: E402
from tests.oracle_engine import OracleEngine  # noqa: E402
from tests.test_batch_host import _assert_same, _lp, _members, _OracleBatch, _params  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ["pdhg_batch_check_info", "pdhg_batch_eval_points", "pdhg_batch_point_products"]
POLICIES = [AdaptiveStepsizeParams(0.3, 0.6), ConstantStepsizeParams()]
POLICY_IDS = ["adaptive", "constant"]


def _problems():
    return _members()[:3] + [_lp([1.5, 0.5, 0.0, 0.0], [1.0, 0.5, 0.5, 2.0, 1.0])]


class _PlainBatch(_OracleBatch):
    def __init__(self, problems):
        self.members = [OracleEngine.from_problem(p) for p in problems]
        self.K = len(problems)


class _RecordingBatch(_PlainBatch):
    """An oracle batch with the two hook methods as no-ops that record their arguments: the members' own evaluators
    (host evaluators here) do all the work, as they do on the device after the caches have been filled."""

    def __init__(self, problems):
        super().__init__(problems)
        self.records = []

    def eval_points(self, points):
        points = np.asarray(points)
        assert points.shape == (self.K,)
        self.records.append(("eval_points", {k: int(p) for k, p in enumerate(points) if p >= 0}))

    def point_products(self, items):
        items = list(items)
        assert items and len(items) == len(set(items)) and len(items) <= 3 * 32
        assert all(0 <= k < self.K and p in (POINT_CURRENT, POINT_AVERAGE, POINT_RESTART) for k, p in items)
        self.records.append(("point_products", sorted(items)))


# ---- the exports ----

def test_the_header_declares_exactly_the_new_exports_and_the_library_has_them():
    header = open(os.path.join(ROOT, "include", "pdhg_hip_batch_checks.h")).read()
    declared = sorted(set(re.findall(r"\b(pdhg_batch_[a-z_0-9]+)\s*\(pdhg_handle", header)))
    assert declared == NEW_EXPORTS == sorted(_lib.BATCH_CHECKS_EXPORTS)
    L = ctypes.CDLL(_lib.LIB_PATH)       # loads without a GPU
    for name in declared:
        assert hasattr(L, name), f"{name} not exported by libpdhg_hip.so"
        assert getattr(_lib.lib(), name).argtypes, f"{name} is not bound in _lib"
    taken = set(_lib.EXPORTS + _lib.RESOLVE_EXPORTS + _lib.BATCH_RESOLVE_EXPORTS + _lib.MATRIX_UPDATE_EXPORTS)
    assert not set(NEW_EXPORTS) & taken
    assert _lib.lib().pdhg_abi_version() == _lib.ABI_VERSION == 11
    for name in ("pdhg_hip.h", "pdhg_hip_resolve.h", "pdhg_hip_batch_resolve.h", "pdhg_hip_matrix_update.h"):
        other = open(os.path.join(ROOT, "include", name)).read()
        assert not set(re.findall(r"\b(pdhg_[a-z_0-9]+)\s*\(", other)) & set(NEW_EXPORTS), name


def test_null_handles_are_refused_without_a_gpu():
    L = _lib.lib()
    ints = np.zeros(4, dtype=np.int32).ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    info = np.zeros(8, dtype=np.int64)
    out = np.zeros(24 * 4)
    calls = {"pdhg_batch_point_products": (1, ints, ints),
             "pdhg_batch_eval_points": (ints, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))),
             "pdhg_batch_check_info": (info.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),)}
    assert sorted(calls) == NEW_EXPORTS
    for name, args in calls.items():
        assert getattr(L, name)(None, *args) == -1, name
        assert b"null handle" in L.pdhg_last_error(), name
    assert not info.any() and not out.any()


# ---- the hook ----

def _spied_solve(monkeypatch, run):
    """``run(factory)`` with ``_check_round`` spied: (outputs, the batch, [(active members' slots, the round's records)])."""
    batches, rounds = [], []
    inner = pdhg._check_round

    def spy(active, checks):
        batch = batches[-1]
        start = len(batch.records)
        out = inner(active, checks)
        slot = {id(e): k for k, e in enumerate(batch.members)}
        rounds.append((sorted(slot[id(mb.engine)] for mb in active), batch.records[start:]))
        return out
    monkeypatch.setattr(pdhg, "_check_round", spy)

    def factory(ps):
        batches.append(_RecordingBatch(ps))
        return batches[-1]
    return run(factory), batches[-1], rounds


@pytest.mark.parametrize("policy", POLICIES, ids=POLICY_IDS)
def test_switched_on_every_sweep_makes_one_call_of_each_kind(policy, monkeypatch):
    problems = _problems()
    params = _params(freq=3, policy=policy)
    want = [optimize(params, p, OracleEngine.from_problem) for p in problems]
    monkeypatch.setenv("PDHG_BATCH_CHECKS", "1")
    got, batch, rounds = _spied_solve(monkeypatch, lambda f: optimize_batch(params, problems, batch_factory=f))
    for g, w in zip(got, want):
        _assert_same(g, w)
    assert rounds and sum(len(r) for _, r in rounds) == len(batch.records)
    kinds = set()
    for members, records in rounds:
        # at most three sweeps, each at most one call per kind; the first holds every active member's iteration stats
        assert 1 <= len(records) <= 3, records
        kind, points = records[0]
        assert kind == "eval_points" and sorted(points) == members, (records, members)
        assert set(points.values()) <= {POINT_CURRENT, POINT_AVERAGE}
        assert [kind for kind, _ in records].count("eval_points") == 1
        products = [items for kind, items in records if kind == "point_products"]
        assert len(products) <= 2                                 # the objective-bound estimates, the restart test
        for items in products:
            assert {k for k, _ in items} <= set(members)
        if products:
            # record_iteration_stats: every checking member asks for the bounds at the point it evaluated
            assert sorted(k for k, _ in products[0]) == members
            assert all(points[k] == p for k, p in products[0])
        if len(products) == 2:
            # the restart test of the members that went on: the average, the current iterate and, for the
            # adaptive-normalized scheme, the restart point
            by_member = {}
            for k, p in products[1]:
                by_member.setdefault(k, []).append(p)
            assert all(ps in ([POINT_CURRENT, POINT_AVERAGE], [POINT_CURRENT, POINT_AVERAGE, POINT_RESTART])
                       for ps in by_member.values()), by_member
        kinds.update(kind for kind, _ in records)
    assert kinds == {"eval_points", "point_products"}
    assert any(len(a) == len(problems) for a, _ in rounds) and any(len(a) < len(problems) for a, _ in rounds)
    assert any(len(r) == 3 for _, r in rounds)


@pytest.mark.parametrize("value", [None, "0", ""], ids=["unset", "zero", "empty"])
def test_switched_off_no_call_is_made_and_the_outputs_are_the_same(value, monkeypatch):
    problems = _problems()
    params = _params(freq=3)
    monkeypatch.setenv("PDHG_BATCH_CHECKS", "1")
    on, batch_on, _ = _spied_solve(monkeypatch, lambda f: optimize_batch(params, problems, batch_factory=f))
    assert batch_on.records
    if value is None:
        monkeypatch.delenv("PDHG_BATCH_CHECKS")
    else:
        monkeypatch.setenv("PDHG_BATCH_CHECKS", value)
    batches = []

    def factory(ps):
        batches.append(_RecordingBatch(ps))
        return batches[-1]
    off = optimize_batch(params, problems, batch_factory=factory)
    assert batches[-1].records == []
    for g, w in zip(off, on):
        _assert_same(g, w)


def test_a_batch_without_the_methods_is_driven_as_before(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("the hook ran for a batch without eval_points / point_products")
    monkeypatch.setattr(pdhg, "_check_round", refuse)
    monkeypatch.setenv("PDHG_BATCH_CHECKS", "1")
    problems = _problems()
    params = _params(freq=3)
    want = [optimize(params, p, OracleEngine.from_problem) for p in problems]
    for g, w in zip(optimize_batch(params, problems, batch_factory=_PlainBatch), want):
        _assert_same(g, w)

    class _Half(_PlainBatch):                # one of the two methods is not enough
        def eval_points(self, points):
            raise AssertionError("called")
    for g, w in zip(optimize_batch(params, problems, batch_factory=_Half), want):
        _assert_same(g, w)


def test_a_batch_session_takes_the_same_hook(monkeypatch):
    class _ResolveRecordingBatch(_RecordingBatch):
        def __init__(self, problems):
            self.members = [ResolveOracleEngine.from_problem(p) for p in problems]
            self.K = len(problems)
            self.records = []
    problems = _problems()
    params = _params(freq=3, limit=200)
    want = [optimize(params, p, OracleEngine.from_problem) for p in problems]
    with PdhgBatchSession(params, problems, _ResolveRecordingBatch) as session:
        for g, w in zip(session.solve(), want):               # the variable is read at every solve: off ...
            _assert_same(g, w)
        assert session.batch.records == []
        monkeypatch.setenv("PDHG_BATCH_CHECKS", "1")           # ... and on, on the same session
        for g, w in zip(session.solve(), want):
            _assert_same(g, w)
        kinds = {kind for kind, _ in session.batch.records}
        assert kinds == {"eval_points", "point_products"}
        count = len(session.batch.records)
        last = session.solve()
        warm = session.solve(warm_start=True)
        assert len(session.batch.records) > count
        for g, p, w in zip(warm, problems, last):
            _assert_same(g, optimize(params, p, OracleEngine.from_problem, w.primal_solution, w.dual_solution))
