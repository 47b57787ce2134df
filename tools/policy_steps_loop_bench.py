"""What a take_step of a MEDIUM problem -- too large for the one-workgroup LDS kernel -- costs under the constant and the
Malitsky-Pock policy in the persistent multi-step kernel (policy_steps_kernel, PDHG_DEVICE_LOOP=1) and launch by launch
(PDHG_DEVICE_LOOP=0), with the adaptive LP of the same shape beside it as the control (code this kernel leaves alone).

    python tools/policy_steps_loop_bench.py [--shapes qp3000x2500,qp60000x50000,l1svm] [--rows lp/adaptive,lp/constant,...]
                                            [--steps 256] [--warm 256] [--reps 5] [--settings 0,1] [--rounds 2]
                                            [--label NAME] [--out TABLE.txt]

Shapes and problems: those of tools/steps_qp_bench.py (README, "Medium QPs").  Rows: the LP under the adaptive, the
constant and the Malitsky-Pock policy (0.7, 0.99, 1.0), the QP under the constant policy.  K = 1: one HipPdhgEngine; one
call = `steps` take_steps; every repetition starts from the origin and `warm` steps (which leave the Malitsky-Pock
average non-empty); the best of `reps` wall times of one call -- the call returns after the results have arrived, so the
wall time includes the device -- and the spread (worst - best) / best.  The constant step size is
1 / sqrt(|A|_1 |A|_inf), for a QP 1 / (sqrt(|A|_1 |A|_inf) + |Q|_inf), primal weight 1.

One invocation measures ONE library (PDHG_HIP_LIB chooses that of another checkout: the tool uses only names that older
checkouts have) and alternates the settings of PDHG_DEVICE_LOOP row by row, `rounds` times, a fresh engine each time (the
library reads the variable at every call).  `loop launches` is pdhg_steps_info's count of persistent multi-step launches
during the timed calls: 0 means the row went launch by launch."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from steps_qp_bench import SHAPES, problem  # noqa: E402

ROWS = ("lp/adaptive", "lp/constant", "lp/malitsky_pock", "qp/constant")


def policy_and_step(p, name):
    import scipy.sparse as sp
    from firstorderlp_jl_amd.primal_dual_hybrid_gradient import (AdaptiveStepsizeParams, ConstantStepsizeParams,
                                                                 MalitskyPockStepsizeParameters)
    A = abs(sp.csr_matrix(p.constraint_matrix))
    if name == "constant":
        norm = float(np.sqrt(A.sum(axis=0).max() * A.sum(axis=1).max()))
        Q = p.objective_matrix
        if Q is not None and Q.nnz > 0:
            norm += float(abs(sp.csr_matrix(Q)).sum(axis=1).max())
        return ConstantStepsizeParams(), 1.0 / norm
    policy = AdaptiveStepsizeParams(0.3, 0.6) if name == "adaptive" else MalitskyPockStepsizeParameters(0.7, 0.99, 1.0)
    return policy, float(1.0 / A.data.max())


def measure(p, name, steps, warm, reps):
    import folp_loader
    from firstorderlp_jl_amd.primal_dual_hybrid_gradient import PdhgSolverState, take_steps
    pkg = folp_loader.load()
    policy, step = policy_and_step(p, name)
    eng = pkg.HipPdhgEngine.from_problem(p, device_id=0)
    try:
        times, launches, trials = [], 0, 0
        for rep in range(reps):
            eng.set_current(np.zeros(eng.n), np.zeros(eng.m))
            eng.reset_average()
            st = PdhgSolverState(eng, step_size=step, primal_weight=1.0, ratio_step_sizes=1.0)
            take_steps(policy, st, warm)
            info = getattr(eng, "steps_info", lambda: [0, 0, 0, 0])
            before, it0 = info(), st.total_number_iterations
            t0 = time.perf_counter()
            done = take_steps(policy, st, steps)
            times.append(time.perf_counter() - t0)
            if done != steps or st.numerical_error:
                raise RuntimeError(f"{name}: the engine stopped on a numerical error")
            launches += int(info()[1] - before[1])
            # (the constant policy does not count iterations: one trial per step)
            trials += int(st.total_number_iterations - it0) if name != "constant" else steps
        return {"times": times, "loop_launches": launches, "trials": trials, "steps_local": int(eng.layout_info()["steps_local"])}
    finally:
        eng.close()


HEADER = ["# tools/policy_steps_loop_bench.py: one call = `steps` take_steps of one engine (K = 1); best of `reps` calls, each from the",
          "# origin and `warm` steps; wall time includes the device; spread = (worst - best) / best; us/step = best / steps; us/trial",
          "# counts the rejected dual trials too; loop launches: persistent multi-step launches during the timed calls (0: launch by launch)",
          f"{'shape':<15} {'row':<17} {'library / setting':<34} {'call ms':>9} {'steps/s':>9} {'us/step':>8} {'us/trial':>9} {'spread':>7} {'loop launches':>14} {'local':>6}"]


def line_of(shape, row, label, r, steps, reps):
    best = min(r["times"])
    return (f"{shape:<15} {row:<17} {label:<34} {1e3 * best:>9.3f} {steps / best:>9.0f} {1e6 * best / steps:>8.2f} "
            f"{1e6 * sum(r['times']) / max(r['trials'], 1):>9.2f} {(max(r['times']) - best) / best:>7.2f} {r['loop_launches']:>14} {r['steps_local']:>6}")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--rows", default=",".join(ROWS))
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--warm", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--settings", default="0,1", help="values of PDHG_DEVICE_LOOP to alternate (`unset` leaves it out)")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--label", default="this", help="names the library in the table (PDHG_HIP_LIB chooses it)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    lines = list(HEADER)
    print("\n".join(lines), flush=True)
    for shape in args.shapes.split(","):
        problems = {}
        for row in args.rows.split(","):
            kind, name = row.split("/")
            if kind not in problems:
                problems[kind] = problem(shape, kind)
            for rnd in range(args.rounds):
                for setting in args.settings.split(","):
                    os.environ.pop("PDHG_DEVICE_LOOP", None)
                    if setting != "unset":
                        os.environ["PDHG_DEVICE_LOOP"] = setting
                    label = f"{args.label}, {'unset' if setting == 'unset' else '..=' + setting} (round {rnd + 1})"
                    try:
                        lines.append(line_of(shape, row, label, measure(problems[kind], name, args.steps, args.warm, args.reps), args.steps, args.reps))
                    except RuntimeError as e:
                        lines.append(f"{shape:<15} {row:<17} {label:<34} not measured: {e}")
                    print(lines[-1], flush=True)
            lines.append("")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
