"""The constant and the Malitsky-Pock policy as library calls (pdhg_take_steps_constant / _malitsky_pock, their fleet
forms, pdhg_steps_info): what can be checked without a GPU -- the exports, the argument checks that return before any
device work, and that ``take_steps`` hands a whole batch to the engine's native call (one call, every scalar stored)
unless PDHG_PY_TAKE_STEP=1 keeps the Python loops."""
import ctypes
import os
import re

import numpy as np
import pytest

from firstorderlp_jl_amd import _lib
from firstorderlp_jl_amd.primal_dual_hybrid_gradient import (ConstantStepsizeParams, MalitskyPockStepsizeParameters,
                                                             PdhgSolverState, take_steps)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ("pdhg_take_steps_constant", "pdhg_take_steps_malitsky_pock", "pdhg_fleet_take_steps_constant",
               "pdhg_fleet_take_steps_malitsky_pock", "pdhg_steps_info")


def test_the_five_exports_are_declared_built_and_bound():
    header = open(os.path.join(ROOT, "include", "pdhg_hip.h")).read()
    declared = set(re.findall(r"\b(pdhg_[a-z_0-9]+)\s*\(", header))
    shim = open(os.path.join(ROOT, "julia", "FirstOrderLpHIP.jl")).read()
    bound = set(re.findall(r"ccall\(\(:(pdhg_[a-z_0-9]+), LIB\)", shim))
    L = ctypes.CDLL(_lib.LIB_PATH)       # loads without a GPU
    for name in NEW_EXPORTS:
        assert name in _lib.EXPORTS, name
        assert name in declared, name
        assert name in bound, name
        assert hasattr(L, name), f"{name} not exported by libpdhg_hip.so"
    assert _lib.lib().pdhg_abi_version() == _lib.ABI_VERSION == 11


def test_argument_checks_return_before_any_device_work():
    L = _lib.lib()
    d, i64, i32 = ctypes.c_double, ctypes.c_int64, ctypes.c_int
    ss, ratio, kkt, it, err, done = d(1.0), d(1.0), d(0.0), i64(0), i32(0), i64(7)
    ref = ctypes.byref
    # no handle
    assert L.pdhg_take_steps_constant(None, 3, 1.0, 1.0, ref(kkt), ref(done)) == -1
    assert done.value == 0 and kkt.value == 0.0
    assert L.pdhg_take_steps_malitsky_pock(None, 3, 0.7, 0.99, 1.0, ref(ss), ref(ratio), 1.0, ref(it), ref(kkt), ref(err),
                                           ref(done)) == -1
    assert (ss.value, ratio.value, it.value, kkt.value) == (1.0, 1.0, 0, 0.0)
    # null pointers (the handle is never looked at: any non-null value will do)
    fake = ctypes.c_void_p(8)
    assert L.pdhg_take_steps_constant(fake, 3, 1.0, 1.0, None, ref(done)) == -1
    assert L.pdhg_take_steps_constant(fake, 3, 1.0, 1.0, ref(kkt), None) == -1
    for hole in range(6):
        args = [ref(ss), ref(ratio), ref(it), ref(kkt), ref(err), ref(done)]
        args[hole] = None
        assert L.pdhg_take_steps_malitsky_pock(fake, 3, 0.7, 0.99, 1.0, args[0], args[1], 1.0, *args[2:]) == -1, hole
    # n_steps < 0
    assert L.pdhg_take_steps_constant(fake, -1, 1.0, 1.0, ref(kkt), ref(done)) == -2
    assert L.pdhg_take_steps_malitsky_pock(fake, -1, 0.7, 0.99, 1.0, ref(ss), ref(ratio), 1.0, ref(it), ref(kkt), ref(err),
                                           ref(done)) == -2
    assert b"n_steps < 0" in L.pdhg_last_error()
    # the fleet calls without a fleet
    ns = np.array([2], dtype=np.int64)
    one, zero = np.ones(1), np.zeros(1)
    its, errs, dones = np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int64)
    pd, pi = (lambda a: a.ctypes.data_as(ctypes.POINTER(d))), (lambda a: a.ctypes.data_as(ctypes.POINTER(i64)))
    assert L.pdhg_fleet_take_steps_constant(None, pi(ns), pd(one), pd(one), pd(zero), pi(dones)) == -1
    assert L.pdhg_fleet_take_steps_malitsky_pock(None, pi(ns), 0.7, 0.99, 1.0, pd(one), pd(one), pd(one), pi(its), pd(zero),
                                                 errs.ctypes.data_as(ctypes.POINTER(i32)), pi(dones)) == -1
    assert L.pdhg_steps_info(None, pi(np.zeros(4, dtype=np.int64))) == -1
    assert zero[0] == 0.0 and its[0] == 0


class _StubEngine:
    """An engine that only offers the two native calls: every other attribute access is an error."""

    def __init__(self):
        self.calls = []

    def take_steps_constant(self, n_steps, step_size, primal_weight, cumulative_kkt_passes):
        self.calls.append(("constant", n_steps, step_size, primal_weight, cumulative_kkt_passes))
        return cumulative_kkt_passes + n_steps, n_steps

    def take_steps_malitsky_pock(self, n_steps, downscaling_factor, breaking_factor, interpolation_coefficient, step_size,
                                 ratio_step_sizes, primal_weight, total_number_iterations, cumulative_kkt_passes):
        self.calls.append(("malitsky_pock", n_steps, downscaling_factor, breaking_factor, interpolation_coefficient,
                           step_size, ratio_step_sizes, primal_weight, total_number_iterations, cumulative_kkt_passes))
        return 0.25, 0.5, total_number_iterations + 70, cumulative_kkt_passes + 40.5, True, n_steps - 1


class _LoopEngine(_StubEngine):
    """The same with the per-trial entry points of the Python loops (every trial accepted)."""

    def __init__(self):
        super().__init__()
        self.trials = 0
        self.accepts = []

    def trial_step(self, step_size, primal_weight, theta=1.0):
        self.trials += 1
        return np.array([0.0, 1.0, 1.0, 0.0, 0.0])

    def trial_primal(self, step_size, primal_weight):
        pass

    def trial_dual(self, step_size, primal_weight, theta):
        self.trials += 1
        return np.array([0.0, 1.0, 1.0, 0.0, 0.0])

    def average_info(self):
        return (1, 1, 1.0, 1.0)

    def accept(self, avg_weight):
        self.accepts.append(avg_weight)


def test_take_steps_makes_one_native_call_per_batch(monkeypatch):
    monkeypatch.delenv("PDHG_PY_TAKE_STEP", raising=False)
    eng = _StubEngine()
    st = PdhgSolverState(eng, step_size=0.5, primal_weight=2.0, cumulative_kkt_passes=3.0, total_number_iterations=11,
                         ratio_step_sizes=1.0)
    assert take_steps(ConstantStepsizeParams(), st, 64) == 64
    assert eng.calls == [("constant", 64, 0.5, 2.0, 3.0)]
    assert (st.step_size, st.cumulative_kkt_passes, st.total_number_iterations, st.numerical_error) == (0.5, 67.0, 11, False)
    eng.calls.clear()
    assert take_steps(MalitskyPockStepsizeParameters(0.7, 0.99, 1.0), st, 64) == 63
    assert eng.calls == [("malitsky_pock", 64, 0.7, 0.99, 1.0, 0.5, 1.0, 2.0, 11, 67.0)]
    assert (st.step_size, st.ratio_step_sizes, st.total_number_iterations, st.cumulative_kkt_passes,
            st.numerical_error) == (0.25, 0.5, 81, 107.5, True)
    with pytest.raises(ValueError):
        take_steps(MalitskyPockStepsizeParameters(0.7, 0.99, 1.0), st, 64, is_lp=False)
    assert len(eng.calls) == 1


def test_the_python_loops_stay_behind_the_switch(monkeypatch):
    monkeypatch.setenv("PDHG_PY_TAKE_STEP", "1")
    eng = _LoopEngine()
    st = PdhgSolverState(eng, step_size=0.5, primal_weight=2.0, ratio_step_sizes=1.0)
    assert take_steps(ConstantStepsizeParams(), st, 5) == 5
    assert take_steps(MalitskyPockStepsizeParameters(0.7, 0.99, 1.0), st, 4) == 4
    assert eng.calls == [] and eng.trials == 9 and len(eng.accepts) == 9
    assert st.cumulative_kkt_passes == 5 + 4 * 1.0 and st.total_number_iterations == 4
