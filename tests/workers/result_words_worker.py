#!/usr/bin/env python3
"""One run of tests/test_gpu_result_words.py: 30 rounds on ONE handle of five take_steps in one call, a trial step + accept,
and an evaluation + a trust-region bound at the current iterate -- the three kinds of pinned result words (csrc/grid_sync.hpp)
taking turns.  Which paths serve the calls is the parent's business (environment); everything the calls return and the
iterate after every round go into an .npz.

argv: <small|stream> <out.npz>"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import folp_loader  # noqa: E402

folp_loader.load()
from firstorderlp_jl_amd import HipPdhgEngine  # noqa: E402
from firstorderlp_jl_amd.evaluation import POINT_CURRENT  # noqa: E402
from firstorderlp_jl_amd.generators import random_lp  # noqa: E402
from tests import helpers as H  # noqa: E402

SHAPES = {"small": (40, 30, 3, 11), "stream": (300, 200, 8, 12)}      # rows, columns, entries per row, seed
ROUNDS, STEPS = 30, 5


def main(shape, out):
    p = random_lp(*SHAPES[shape][:3], seed=SHAPES[shape][3])
    eng = HipPdhgEngine.from_problem(p, device_id=0)
    m, n = p.constraint_matrix.shape
    eng.set_original_problem(np.ones(m), np.ones(n), p.objective_vector, p.right_hand_side, p.variable_lower_bound,
                             p.variable_upper_bound)
    step, pw = H.initial_step_and_weight(p)
    it, kkt = 0, 0.0
    rec = {k: [] for k in ("step", "it", "kkt", "err", "done", "raw", "ev", "tr", "x", "y")}
    for r in range(ROUNDS):
        step, it, kkt, err, done = eng.take_steps_adaptive(STEPS, 0.3, 0.6, step, pw, it, kkt)
        raw = eng.trial_step(step, pw, 1.0)
        eng.accept(step)
        ev = eng.eval_point(POINT_CURRENT)
        tr = eng.trust_region_bound(POINT_CURRENT, 1.7, 0.6, 0.5 + 0.25 * r, 0, False)
        x, y = eng.get_current()
        for k, v in (("step", step), ("it", it), ("kkt", kkt), ("err", float(err)), ("done", done), ("raw", raw), ("ev", ev),
                     ("tr", tr), ("x", x), ("y", y)):
            rec[k].append(np.array(v, dtype=np.float64))
    np.savez(out, **{k: np.array(v) for k, v in rec.items()})
    eng.close()


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
