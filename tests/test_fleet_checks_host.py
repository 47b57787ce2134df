"""The checks of optimize_many on the host: the check stated once as a generator (``_Solve.evaluate_steps``, the ``*_steps``
functions of saddle_point.py) and the driver's hook that gathers the requests of all members (``_check_round``), through
a recording fleet over CPU oracle engines; the plain functions against results recorded before they were restated; the
two exports.

The goldens: ``python tests/test_fleet_checks_host.py tests/golden/fleet_checks_plain_functions.json`` writes what
``_plain_function_results`` returns (every float as its hex string); the committed file was written that way by the
commit before the generator forms existed."""
import ctypes
import dataclasses
import json
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)

import folp_loader  # noqa: E402

folp = folp_loader.load()
from firstorderlp_jl_amd import _lib, optimize_many  # noqa: E402
from firstorderlp_jl_amd.evaluation import POINT_AVERAGE, POINT_CURRENT  # noqa: E402
from firstorderlp_jl_amd import primal_dual_hybrid_gradient as pdhg  # noqa: E402
from firstorderlp_jl_amd.primal_dual_hybrid_gradient import (AdaptiveStepsizeParams, ConstantStepsizeParams,  # noqa: E402
                                                             MalitskyPockStepsizeParameters, optimize, take_steps)
from firstorderlp_jl_amd.saddle_point import (RestartScheme, run_restart_scheme,  # noqa: E402
                                              update_objective_bound_estimates)
from tests.oracle_engine import OracleEngine  # noqa: E402
from tests.test_fleet_host import _assert_same, _OracleFleet, _params, _problems  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "fleet_checks_plain_functions.json")
CHECK_EXPORTS = ("pdhg_fleet_eval_points", "pdhg_fleet_trust_region_bounds")
POLICIES = [AdaptiveStepsizeParams(0.3, 0.6), ConstantStepsizeParams(), MalitskyPockStepsizeParameters(0.7, 1.0, 0.9)]
POLICY_IDS = ["adaptive", "constant", "malitsky_pock"]


class _RecordingFleet(_OracleFleet):
    """An oracle fleet with the two hook methods as no-ops that record (kind, member indices): the members' own
    evaluators (host evaluators here) do all the work, as they do for a member the device does not carry."""

    def __init__(self, problems):
        super().__init__(problems)
        self.records = []

    def eval_points(self, points):
        self.records.append(("eval_points", [k for k, p in enumerate(points) if p >= 0]))

    def trust_region_bounds(self, items):
        assert all(len(it) == 7 and it[5] in (0, 1, 2) for it in items)
        self.records.append(("trust_region_bounds", sorted({it[0] for it in items})))


@pytest.mark.parametrize("policy", POLICIES, ids=POLICY_IDS)
def test_the_hook_gathers_every_members_requests(policy, monkeypatch):
    problems = _problems()
    params = _params(policy)
    want = [optimize(params, p, OracleEngine.from_problem) for p in problems]
    fleets, rounds = [], []
    inner = pdhg._check_round

    def spy(active, checks):
        fleet = fleets[-1]
        start = len(fleet.records)
        out = inner(active, checks)
        rounds.append((list(active), fleet.records[start:]))
        return out
    monkeypatch.setattr(pdhg, "_check_round", spy)

    def factory(ps):
        fleets.append(_RecordingFleet(ps))
        return fleets[-1]
    got = optimize_many(params, problems, fleet_factory=factory)
    for g, w in zip(got, want):
        _assert_same(g, w)
    fleet = fleets[-1]
    slot = {id(e): k for k, e in enumerate(fleet.members)}
    assert rounds and sum(len(r) for _, r in rounds) == len(fleet.records)
    seen_kinds = set()
    for active, records in rounds:
        members = sorted(slot[id(mb.engine)] for mb in active)
        # at most three sweeps, each at most one call per kind; the first holds every active member's iteration stats
        assert 1 <= len(records) <= 3, records
        assert records[0] == ("eval_points", members), (records, members)
        assert [kind for kind, _ in records].count("eval_points") == 1
        tr = [ks for kind, ks in records if kind == "trust_region_bounds"]
        assert len(tr) <= 2                                   # the objective-bound estimates, the restart test
        for ks in tr:
            assert set(ks) <= set(members) and len(set(ks)) == len(ks)
        seen_kinds.update(kind for kind, _ in records)
        if tr:
            assert tr[0] == members
        if len(tr) == 2:
            # record_iteration_stats: every checking member asks for the objective-bound estimates; those that went on
            # (did not terminate in this round) and hold an average ask for the restart test's bounds
            assert tr[0] == members and set(tr[1]) <= set(tr[0])
    assert seen_kinds == {"eval_points", "trust_region_bounds"}
    assert any(len(a) == len(problems) for a, _ in rounds) and any(len(a) < len(problems) for a, _ in rounds)


def test_a_fleet_without_the_methods_is_driven_as_before(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("the hook ran for a fleet without eval_points / trust_region_bounds")
    monkeypatch.setattr(pdhg, "_check_round", refuse)
    problems = _problems()
    params = _params(POLICIES[0])
    want = [optimize(params, p, OracleEngine.from_problem) for p in problems]
    for g, w in zip(optimize_many(params, problems, fleet_factory=_OracleFleet), want):
        _assert_same(g, w)


def test_evaluate_is_its_generator_answered_at_once():
    """``evaluate()`` and a hand-driven ``evaluate_steps()`` on twin solves: the same requests' answers, the same step
    counts, the same stats."""
    p = _problems()[0]
    params = _params(POLICIES[0])
    twins = []
    for _ in range(2):
        scaled, max_abs = pdhg._host_scaled_problem(params, p)
        solve = pdhg._Solve(params, p, scaled, OracleEngine.from_problem(scaled.scaled_qp), max_abs)
        solve.start()
        twins.append(solve)
    a, b = twins
    kinds = []
    for _ in range(12):
        steps_a = a.evaluate()
        gen = b.evaluate_steps()
        try:
            request = next(gen)
            while True:
                kinds.append(request[0])
                request = gen.send(getattr(b.ev, request[0])(*request[1]))
        except StopIteration as stop:
            steps_b = stop.value
        assert steps_a == steps_b
        if steps_a == 0:
            break
        for s in (a, b):
            s.stepped(take_steps(params.step_size_policy_params, s.state, steps_a, True), 0.0)
    assert set(kinds) == {"iteration_stats", "bounds"}
    from tests.test_fleet_host import _stats_key
    assert [_stats_key(s) for s in a.iteration_stats] == [_stats_key(s) for s in b.iteration_stats]
    for s in twins:
        s.engine.close()


def _hex(v):
    if v is None:
        return None
    if isinstance(v, (list, tuple)):
        return [_hex(u) for u in v]
    if dataclasses.is_dataclass(v):
        return {k: _hex(u) for k, u in dataclasses.asdict(v).items()}
    if isinstance(v, dict):
        return {k: _hex(u) for k, u in v.items()}
    if isinstance(v, (float, np.floating)):
        return float(v).hex()
    if isinstance(v, (int, np.integer)):
        return int(v)
    return str(v)


def _plain_function_results():
    """``update_objective_bound_estimates`` and ``run_restart_scheme`` (the plain functions) with a ``HostEvaluator``
    over the CPU oracle, on the problems of tests/test_fleet_host.py after 3, 10 and 31 adaptive steps, under three
    restart schemes: what they return and what they leave in their arguments.  ``run_restart_scheme`` is called twice
    at each state.  First with an iteration count a thousand times the real one, so that the average is far too short
    for an artificial restart and the scheme's own test decides (with the points its ``bounds`` request named: the
    adaptive-normalized test adds the RESTART point); then with the real count, at which every average that the first
    call left is long enough for an artificial restart."""
    out = {}
    for scheme in (RestartScheme.ADAPTIVE_NORMALIZED, RestartScheme.NO_RESTARTS, RestartScheme.ADAPTIVE_DISTANCE):
        params = _params(POLICIES[0])
        params.restart_params.restart_scheme = scheme
        for k, p in enumerate(_problems()):
            scaled, max_abs = pdhg._host_scaled_problem(params, p)
            eng = OracleEngine.from_problem(scaled.scaled_qp)
            solve = pdhg._Solve(params, p, scaled, eng, max_abs)
            solve.start()
            st = solve.state
            done = 0
            asked = []
            bounds = solve.ev.bounds

            def spy(requests, *rest):
                asked.append([int(r[0]) for r in requests])
                return bounds(requests, *rest)
            solve.ev.bounds = spy
            for n in (3, 7, 21):
                done += take_steps(params.step_size_policy_params, st, n, True)
                wp = float(np.float64(1) / st.step_size * st.primal_weight)
                wd = float(np.float64(1) / st.step_size / st.primal_weight)
                stats = {}
                for point in (POINT_AVERAGE, POINT_CURRENT):
                    update_objective_bound_estimates(stats, solve.ev, point, wp, wd)
                    out[f"{scheme.name}/{k}/{done}/bounds/{point}"] = _hex(stats)
                for name, completed in (("restart_by_the_scheme", 1000 * done), ("restart", done)):
                    del asked[:]
                    choice = run_restart_scheme(solve.ev, solve.last_restart_info, completed, wp, wd, st.primal_weight, 0,
                                                params.restart_params)
                    out[f"{scheme.name}/{k}/{done}/{name}"] = _hex([choice.name, solve.last_restart_info, eng.average_info(),
                                                                  list(asked)])
            eng.close()
    return out


def test_the_plain_functions_return_what_they_returned_before():
    want = json.load(open(GOLDEN))
    got = _plain_function_results()
    assert sorted(got) == sorted(want)
    for key in want:
        assert got[key] == want[key], key
    # the recorded calls reach every exit of the scheme: its own test restarted and did not (NO_RESTART with a non-empty
    # average), with and without the RESTART point in its request; the artificial restart took the rest
    by_scheme = [v for k, v in want.items() if k.endswith("/restart_by_the_scheme")]
    assert any(v[0] == "RESTART_CHOICE_NO_RESTART" and v[2][0] > 0 for v in by_scheme)
    assert any(v[0] != "RESTART_CHOICE_NO_RESTART" for v in by_scheme)
    assert any(v[3] and len(v[3][0]) == 3 for v in by_scheme) and any(v[3] and len(v[3][0]) == 2 for v in by_scheme)
    assert any(v[0] != "RESTART_CHOICE_NO_RESTART" for k, v in want.items() if k.endswith("/restart"))


def test_the_check_exports_are_declared_built_and_bound():
    header = open(os.path.join(ROOT, "include", "pdhg_hip.h")).read()
    declared = set(re.findall(r"\b(pdhg_[a-z_0-9]+)\s*\(", header))
    julia = open(os.path.join(ROOT, "julia", "FirstOrderLpHIP.jl")).read()
    L = ctypes.CDLL(_lib.LIB_PATH)       # loads without a GPU
    for name in CHECK_EXPORTS:
        assert name in _lib.EXPORTS, name
        assert name in declared, name
        assert hasattr(L, name), f"{name} not exported by libpdhg_hip.so"
        assert f"(:{name}, LIB)" in julia, f"{name} is not bound in the Julia shim"
    assert _lib.lib().pdhg_abi_version() == 11


if __name__ == "__main__":
    with open(sys.argv[1], "w") as fh:
        json.dump(_plain_function_results(), fh, indent=0, sort_keys=True)
        fh.write("\n")
