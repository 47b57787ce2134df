"""The three kinds of pinned result words (csrc/grid_sync.hpp: steps_res, res_host, ev_host) taking turns on one handle
against a run that uses none of them: 30 rounds of five take_steps in one call, a trial step + accept, an evaluation and a
trust-region bound (tests/workers/result_words_worker.py).  The reference is the same sequence with every one-launch
path and every host word turned off -- separate launches, device-to-host copies, stream synchronisation -- in a child
of its own (PDHG_TRIAL_HOST_WORD is read once per process).  Every step size, count, returned scalar and iterate must
be bitwise equal: a word taken from the wrong launch, or a sequence counter out of step after another buffer's
launch, would show at once."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "workers", "result_words_worker.py")

PLAIN = {"PDHG_COOP": "0", "PDHG_GRAPH": "0", "PDHG_DEVICE_LOOP": "0", "PDHG_SMALL_LP": "0", "PDHG_TRIAL_HOST_WORD": "0",
         "PDHG_EVAL_HOST_WORD": "0"}


@pytest.mark.gpu
@pytest.mark.short_rows
@pytest.mark.timeout(240)
@pytest.mark.parametrize("shape,env", [("small", {}),                            # 40 x 30: the small-LP kernel
                                       ("stream", {"PDHG_SMALL_LP": "0"})],    # 300 x 200: steps_kernel and trial_kernel
                         ids=["small_lp", "stream"])
def test_interleaved_publishers_match_a_run_without_result_words(gpu_required, tmp_path, shape, env):
    runs = {}
    for name, extra in (("words", env), ("plain", PLAIN)):
        e = dict(os.environ)
        for k in PLAIN:
            e.pop(k, None)
        e.update(extra)
        out = str(tmp_path / f"{name}.npz")
        runs[name] = (out, subprocess.Popen([sys.executable, WORKER, shape, out], cwd=ROOT, env=e, stdout=subprocess.PIPE,
                                            stderr=subprocess.STDOUT, text=True))
    got = {}
    try:
        for name, (out, proc) in runs.items():
            log, _ = proc.communicate(timeout=100)
            assert proc.returncode == 0, (name, log[-3000:])
            assert "timed out" not in log, (name, log[-3000:])       # (a barrier fallback would be bitwise equal too)
            got[name] = dict(np.load(out))
    finally:
        for _, proc in runs.values():
            if proc.poll() is None:
                proc.kill()
                proc.wait()
    assert sorted(got["words"]) == sorted(got["plain"])
    assert got["words"]["it"][-1] >= 30 * 5, got["words"]["it"]
    for k in got["plain"]:
        a, b = got["words"][k], got["plain"][k]
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), (k, a, b)
