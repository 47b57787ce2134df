"""Paired average updates: on a plain handle whose A is in the sweep layout, the first trial after an accept carries the
pending term AND, in advance, its own x' / y' with the weight its accept will have, into alternate sums beside the
running sums; pdhg_accept with that weight swaps the buffers and queues nothing.  Per element these are the additions
of two single updates in the same order with the same roundings, so every bit of the running averages -- and with them
everything else -- must be what the single form (PDHG_PAIR_AVG=0), the separate accept_kernel (PDHG_LAZY_ACCEPT=0) and
the Python take_step loop (PDHG_PY_TAKE_STEP=1, which never stages: it does not go through the C loops) produce,
through rejected trials, reads that settle the pending term, and every entry point that can come between a staging
trial and its accept.

Which take_steps pair depends on where the average is read: a read settles the pending term, so the take_step after it
carries nothing and the one after that pairs.  With reads after take_steps 1, 2, 3 (the first schedule) take_steps 5, 7, 9
and 11 pair, and take_step 6, whose step size was multiplied by 64, is a plain one with rejects; with reads after 1 and
3 alone (the second schedule) take_step 3 -- also multiplied by 64 -- is a pairing one, so its rejected trials stage
again and again with the same weight and the describe counters must show dropped stagings."""
import numpy as np
import pytest

from firstorderlp_jl_amd import HipPdhgEngine
from firstorderlp_jl_amd.evaluation import POINT_AVERAGE
from firstorderlp_jl_amd.generators import random_lp
from firstorderlp_jl_amd.primal_dual_hybrid_gradient import (AdaptiveStepsizeParams, ConstantStepsizeParams,
                                                             PdhgSolverState, take_step, take_steps)
from tests import helpers as H

pytestmark = pytest.mark.gpu

# the smallest shapes that still have the edges: odd n (primal_kernel's scalar tail), m no multiple of 64, several
# column tiles, more than one workgroup of the sweep
LPS = {
    "333x257": (lambda: random_lp(333, 257, 5, seed=1), "128"),
    "1300x1111": (lambda: random_lp(1300, 1111, 6, seed=4), "256"),
    "5000x4001": (lambda: random_lp(5000, 4001, 8, seed=7), "700"),
}
MODES = {          # environment on top of the forced sweep
    "paired": {},
    "single": {"PDHG_PAIR_AVG": "0"},
    "eager": {"PDHG_LAZY_ACCEPT": "0"},
    "python": {"PDHG_PY_TAKE_STEP": "1"},
}
KEYS = ("PDHG_GRAPH", "PDHG_COOP", "PDHG_SPMV", "PDHG_TILE_COLS", "PDHG_SLAB_MB", "PDHG_PY_TAKE_STEP", "PDHG_PAIR_AVG",
        "PDHG_LAZY_ACCEPT", "PDHG_ROW_ORDER")
POLICY = AdaptiveStepsizeParams(0.3, 0.6)


def _engine(p, monkeypatch, mode, tile_cols, sweep=True, **kw):
    for k in KEYS:
        if k != "PDHG_ROW_ORDER":
            monkeypatch.delenv(k, raising=False)
    if sweep:
        monkeypatch.setenv("PDHG_SPMV", "tiled")
        monkeypatch.setenv("PDHG_TILE_COLS", tile_cols)
    for k, v in MODES[mode].items():
        monkeypatch.setenv(k, v)
    return HipPdhgEngine.from_problem(p, **kw)


def _counters(eng):
    d = eng.layout_describe()["average_update"]
    return d["form"], d["paired_accepts"], d["dropped_stagings"]


def _adaptive_run(p, tile_cols, monkeypatch, mode, batches, reads):
    """Twelve adaptive take_steps, the step size multiplied by 64 before take_steps 3 and 6, the average read after the
    take_steps in `reads`; as take_steps batches between those events or one call per step."""
    eng = _engine(p, monkeypatch, mode, tile_cols)
    step, pw = H.initial_step_and_weight(p)
    st = PdhgSolverState(eng, step_size=step, primal_weight=pw)
    events = sorted(set(reads) | {2, 5, 12})          # a batch ends before a scaled take_step and at every read
    sizes, snaps, done = [], [], 0
    for stop in events:
        if batches:
            assert take_steps(POLICY, st, stop - done) == stop - done
        else:
            for _ in range(stop - done):
                take_step(POLICY, st)
        done = stop
        sizes.append(st.step_size)
        if stop in reads:
            snaps.append(np.concatenate(eng.get_average()))
        if stop in (2, 5):
            st.step_size *= 64.0
    out = (st.total_number_iterations, np.array(sizes), np.concatenate(eng.get_current()), snaps, _counters(eng))
    eng.close()
    return out


@pytest.mark.parametrize("reads", [(1, 2, 3, 12), (1, 3, 12)], ids=["reads_1_2_3", "reads_1_3"])
@pytest.mark.parametrize("batches", [True, False], ids=["batches", "per_step"])
@pytest.mark.parametrize("name", sorted(LPS))
def test_paired_average_is_bitwise_single_eager_and_python(gpu_required, monkeypatch, name, batches, reads):
    maker, tile_cols = LPS[name]
    p = maker()
    runs = {mode: _adaptive_run(p, tile_cols, monkeypatch, mode, batches, reads) for mode in MODES}
    ref = runs["eager"]
    assert ref[0] >= 12 + 6, ref[0]                  # both scaled take_steps rejected at least three trials each
    for mode, r in runs.items():
        assert r[0] == ref[0], (mode, r[0], ref[0])
        assert np.array_equal(r[1], ref[1]), mode
        assert np.array_equal(r[2], ref[2]), mode
        assert len(r[3]) == len(ref[3]) == len(reads)
        for a, b in zip(r[3], ref[3]):
            assert np.array_equal(a, b), mode
    form, paired, dropped = runs["paired"][4]
    assert form == "paired" and paired > 0, runs["paired"][4]
    if reads == (1, 3, 12):                          # take_step 3 pairs and rejects: its retries stage again
        assert dropped > 0, runs["paired"][4]
    assert runs["single"][4] == ("single", 0, 0)
    assert runs["eager"][4] == ("single", 0, 0)
    assert runs["python"][4][1:] == (0, 0)           # eligible, but nothing goes through the C loops


# ---- interleavings: what can come between a staging trial and its accept, and right behind a paired accept ----------

def _script(eng, p, ops):
    step, pw = H.initial_step_and_weight(p)
    rng = np.random.default_rng(5)
    st = PdhgSolverState(eng, step_size=step, primal_weight=pw)
    seen = []
    for op in ops:
        if op == "c_step":                           # one take_step through the C loop: stages when a term is pending
            take_step(POLICY, st)
        elif op == "c_steps3":
            take_steps(POLICY, st, 3)
        elif op == "trial":                          # the public entry: weight unknown, never stages
            eng.trial_step(st.step_size, pw)
        elif op == "accept":
            eng.accept(st.step_size)
        elif op == "accept_other":                   # not the weight a staging was made for
            eng.accept(0.75 * st.step_size)
        elif op == "accept_zero":                    # the weight the live staging below was made for
            eng.accept(0.0)
        elif op == "c_zero_step":
            # a staging whose accept never comes: a take_step through the C loop entered with step size 0 stages (when a
            # term is pending) with weight 0, its trial moves nothing, the loop raises numerical_error and returns
            # without an accept -- the staging stays live for whatever comes next
            zero = PdhgSolverState(eng, step_size=0.0, primal_weight=pw)
            take_step(POLICY, zero)
            assert zero.numerical_error
        elif op == "avg":
            seen.append(np.concatenate(eng.get_average()))
        elif op == "reset":
            eng.reset_average()
        elif op == "restart":
            eng.restart_to_average()
            seen.append(np.concatenate(eng.get_current()))
        elif op == "set":
            eng.set_current(rng.standard_normal(eng.n), np.abs(rng.standard_normal(eng.m)))
            seen.append(np.concatenate(eng.get_current()))
        elif op == "add_primal":
            eng.add_current_primal_to_average(0.25)
        elif op == "info":
            seen.append(np.array(eng.average_info(), dtype=float))
        elif op == "eval":
            seen.append(np.array(eng.eval_point(POINT_AVERAGE)))
            seen.append(np.array(eng.distance_to_restart(POINT_AVERAGE)))
        else:
            raise AssertionError(op)
        seen.append(np.array([st.step_size, st.total_number_iterations], dtype=float))
    seen.append(np.concatenate(eng.get_current()))
    if eng.average_info()[0] > 0 and eng.average_info()[1] > 0:
        seen.append(np.concatenate(eng.get_average()))
    return seen


# "c_step", "c_step" = a plain take_step (nothing pending) and then a pairing one; a third "c_step" is plain again;
# "c_step", "c_zero_step" leaves a LIVE staging behind
PAIRING = ["c_step", "c_step"]
PLAIN = ["c_step", "c_step", "c_step"]
LIVE = ["c_step", "c_zero_step"]
TAIL = ["c_step", "c_step", "c_step", "avg"]
SCRIPTS = {
    "raw_trial_and_accept_after_a_pairing_step": PAIRING + ["trial", "accept"] + TAIL,
    "raw_trial_and_accept_after_a_plain_step": PLAIN + ["trial", "accept"] + TAIL,
    "raw_trial_and_accept_over_a_live_staging": LIVE + ["trial", "accept"] + TAIL,
    "accept_with_another_weight_over_a_live_staging": LIVE + ["accept_other"] + TAIL,
    "accept_with_its_weight_over_a_live_staging": LIVE + ["accept_zero"] + TAIL,
    "two_accepts_in_a_row_after_a_pairing_step": PAIRING + ["accept", "accept"] + TAIL,
    "two_accepts_in_a_row_after_a_plain_step": PLAIN + ["accept", "accept"] + TAIL,
    "batches_of_three": ["c_steps3", "avg", "c_steps3", "c_steps3", "info", "c_steps3", "avg"],
}
for _op in ("avg", "reset", "restart", "set", "add_primal", "info", "eval"):
    SCRIPTS[_op + "_after_a_pairing_step"] = PAIRING + [_op] + TAIL
    SCRIPTS[_op + "_after_a_plain_step"] = PLAIN + [_op] + TAIL
    SCRIPTS[_op + "_over_a_live_staging"] = LIVE + [_op] + TAIL
# every script with a live staging must report it dropped, except the one whose accept takes it
DROPS = {k for k in SCRIPTS if "live_staging" in k and "its_weight" not in k}


@pytest.mark.parametrize("name", sorted(SCRIPTS))
def test_paired_average_interleavings(gpu_required, monkeypatch, name):
    p = random_lp(1300, 1111, 6, seed=4)
    m, n = p.constraint_matrix.shape
    results, counters = [], []
    for mode in ("eager", "paired"):
        eng = _engine(p, monkeypatch, mode, "256")
        eng.set_original_problem(np.ones(m), np.ones(n), p.objective_vector, p.right_hand_side,
                                 p.variable_lower_bound, p.variable_upper_bound)
        eng.save_restart_point()
        results.append(_script(eng, p, SCRIPTS[name]))
        counters.append(_counters(eng))
        eng.close()
    assert len(results[0]) == len(results[1]) > 0
    for a, b in zip(*results):
        assert np.array_equal(a, b)
    assert counters[0] == ("single", 0, 0)
    assert counters[1][0] == "paired" and counters[1][1] > 0, counters[1]
    if name in DROPS:
        assert counters[1][2] > 0, counters[1]


# ---- the constant policy ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("steps", [1, 2, 5, 8])
@pytest.mark.parametrize("name", sorted(LPS))
def test_paired_average_constant_policy(gpu_required, monkeypatch, name, steps):
    maker, tile_cols = LPS[name]
    p = maker()
    outs = []
    for mode in ("eager", "paired"):
        eng = _engine(p, monkeypatch, mode, tile_cols)
        step, pw = H.initial_step_and_weight(p)
        st = PdhgSolverState(eng, step_size=0.5 * step, primal_weight=pw)
        assert take_steps(ConstantStepsizeParams(), st, steps) == steps
        first = np.concatenate(eng.get_average())
        assert take_steps(ConstantStepsizeParams(), st, steps) == steps       # from a settled average again
        outs.append((first, np.concatenate(eng.get_average()), np.concatenate(eng.get_current()),
                     np.array(eng.average_info(), dtype=float), st.cumulative_kkt_passes, _counters(eng)))
        eng.close()
    for a, b in zip(outs[0][:5], outs[1][:5]):
        assert np.array_equal(a, b)
    assert outs[1][5][0] == "paired" and outs[1][5][1] == 2 * (steps // 2), outs[1][5]


# ---- free-running against the exact-sums oracle ----------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(LPS))
def test_paired_average_free_running_is_bitwise_the_oracles(gpu_required, monkeypatch, name):
    maker, tile_cols = LPS[name]
    p = maker()
    steps = 40
    monkeypatch.setenv("PDHG_ROW_ORDER", "strict")
    eng = _engine(p, monkeypatch, "paired", tile_cols)
    step, pw = H.initial_step_and_weight(p)
    st = PdhgSolverState(eng, step_size=step, primal_weight=pw)
    sizes = []
    for _ in range(steps):
        take_step(POLICY, st)
        sizes.append(st.step_size)
    x, y = eng.get_current()
    xa, ya = eng.get_average()
    counters = _counters(eng)
    eng.close()
    o = H.oracle_from_problem(p)
    o.exact_sums = True
    o.step_size, o.primal_weight, o.ratio_step_sizes = step, pw, 1.0
    osizes = []
    for _ in range(steps):
        o.take_step_adaptive(POLICY.reduction_exponent, POLICY.growth_exponent)
        osizes.append(o.step_size)
    oxa, oya = o.compute_average()
    assert st.total_number_iterations == o.total_number_iterations, "accept / reject decisions differ"
    for a, b in zip((np.array(sizes), x, y, xa, ya), (np.array(osizes), o.x, o.y, oxa, oya)):
        assert np.array_equal(a, b)
    assert counters[0] == "paired" and counters[1] == steps // 2, counters


# ---- handles that do not pair say so and compute what they computed ------------------------------------------------------

def _qp():
    p = random_lp(700, 901, 6, seed=3)
    import scipy.sparse as sp
    from firstorderlp_jl_amd import QuadraticProgrammingProblem
    n = p.constraint_matrix.shape[1]
    q = sp.diags(np.linspace(0.5, 1.5, n)).tocsc()
    return QuadraticProgrammingProblem(p.variable_lower_bound, p.variable_upper_bound, q, p.objective_vector,
                                       p.objective_constant, p.constraint_matrix, p.right_hand_side, p.num_equalities)


INELIGIBLE = {
    "stream_layout_lp": (lambda: random_lp(700, 901, 6, seed=3), False, {}),
    "qp_in_the_sweep_layout": (_qp, True, {}),
    "two_shard_group": (lambda: random_lp(1300, 1111, 6, seed=4), True, {"device_ids": [0, 0]}),
}


@pytest.mark.parametrize("name", sorted(INELIGIBLE))
def test_an_ineligible_handle_says_so_and_is_bitwise_unchanged(gpu_required, monkeypatch, name):
    maker, sweep, kw = INELIGIBLE[name]
    p = maker()
    outs = []
    for mode in ("eager", "single", "paired"):
        eng = _engine(p, monkeypatch, mode, "256", sweep=sweep, **kw)
        step, pw = H.initial_step_and_weight(p)
        st = PdhgSolverState(eng, step_size=step, primal_weight=pw)
        assert take_steps(POLICY, st, 5) == 5
        first = np.concatenate(eng.get_average())
        st.step_size *= 64.0
        for _ in range(4):
            take_step(POLICY, st)
        outs.append((st.total_number_iterations, st.step_size, first, np.concatenate(eng.get_average()),
                     np.concatenate(eng.get_current()), _counters(eng)))
        eng.close()
    for o in outs:
        assert o[5] == ("single", 0, 0), o[5]
        assert o[0] == outs[0][0] and o[1] == outs[0][1]
        for a, b in zip(o[2:5], outs[0][2:5]):
            assert np.array_equal(a, b)
