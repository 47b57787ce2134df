"""What an adaptive take_step of a MEDIUM QP costs -- too large for the one-workgroup LDS kernel, Q and Q' in the stream
layout -- in the multi-step persistent kernel's QP form (PDHG_DEVICE_LOOP=1) and launch by launch (PDHG_DEVICE_LOOP=0),
with the LP of the same shape beside it as the control.

    python tools/steps_qp_bench.py [--shapes qp3000x2500,qp60000x50000,l1svm] [--kinds lp,qp] [--steps 256] [--warm 256]
                                   [--reps 5] [--label NAME] [--json OUT.json]
    python tools/steps_qp_bench.py --table A.json B.json ... [--out TABLE.txt]

Shapes: random_qp_family(m, n, 1, seed) at 3000 x 2500 and 60000 x 50000, and the L1-SVM generator's LP (rcv1-shaped
synthetic data) plus Q = B'B + diag (B: n/3 x n, three entries per row, the diagonal from 0.05 to 0.5).  The LP rows are
the same problems without Q.  K = 1: one HipPdhgEngine, adaptive policy (0.3, 0.6); one call = `steps` take_steps; every
repetition starts from the origin and `warm` steps (a strongly convex QP carried through thousands of steps reaches its
fixed point, where the adaptive rule stops with numerical_error); the best of `reps` wall times of one call -- the call
returns after the results have arrived, so the wall time includes the device -- and the spread (worst - best) / best.

One invocation measures ONE library under ONE setting of the environment (PDHG_DEVICE_LOOP, and PDHG_HIP_LIB for the
library of another checkout: the tool uses only names that older checkouts have); a shell loop alternates the invocations
on one device and --table puts their --json files side by side.  `loop launches` is pdhg_steps_info's count of multi-step
launches during the timed calls: 0 means the row went launch by launch whatever the setting asked for."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ("qp3000x2500", "qp60000x50000", "l1svm")


def problem(shape, kind):
    import scipy.sparse as sp
    import folp_loader
    folp_loader.load()
    from firstorderlp_jl_amd.generators import l1_svm_rcv1_like_lp, random_qp_family
    from firstorderlp_jl_amd.quadratic_programming import QuadraticProgrammingProblem, linear_programming_problem
    if shape == "l1svm":
        p = l1_svm_rcv1_like_lp()
        if kind == "lp":
            return p
        n = p.constraint_matrix.shape[1]
        rng = np.random.default_rng(4242)
        rows_b = n // 3
        B = sp.csr_matrix((rng.standard_normal(3 * rows_b), (np.repeat(np.arange(rows_b), 3), rng.integers(0, n, 3 * rows_b))),
                          shape=(rows_b, n))
        Q = (B.T @ B + sp.diags(np.linspace(0.05, 0.5, n))).tocsc()
        Q = ((Q + Q.T) * 0.5).tocsc()
        Q.sum_duplicates()
        Q.sort_indices()
        return QuadraticProgrammingProblem(p.variable_lower_bound, p.variable_upper_bound, Q, p.objective_vector, 0.0,
                                           p.constraint_matrix, p.right_hand_side, p.num_equalities)
    m, n = (int(v) for v in shape[2:].split("x"))
    p = random_qp_family(m, n, 1, 20 + m % 7)[0]
    if kind == "qp":
        return p
    return linear_programming_problem(p.variable_lower_bound, p.variable_upper_bound, p.objective_vector, 0.0,
                                      p.constraint_matrix, p.right_hand_side, p.num_equalities)


def measure(p, steps, warm, reps):
    import folp_loader
    from firstorderlp_jl_amd.primal_dual_hybrid_gradient import AdaptiveStepsizeParams, PdhgSolverState, take_steps
    pkg = folp_loader.load()
    policy = AdaptiveStepsizeParams(0.3, 0.6)
    eng = pkg.HipPdhgEngine.from_problem(p, device_id=0)
    try:
        info = eng.layout_info()
        times, launches, trials = [], 0, 0
        for rep in range(reps):
            eng.set_current(np.zeros(eng.n), np.zeros(eng.m))
            eng.reset_average()
            st = PdhgSolverState(eng, step_size=float(1.0 / abs(p.constraint_matrix).data.max()), primal_weight=1.0)
            take_steps(policy, st, warm)
            before, it0 = eng.steps_info(), st.total_number_iterations
            t0 = time.perf_counter()
            done = take_steps(policy, st, steps)
            times.append(time.perf_counter() - t0)
            if done != steps or st.numerical_error:
                raise RuntimeError("the engine stopped on a numerical error")
            launches += int(eng.steps_info()[1] - before[1])
            trials += int(st.total_number_iterations - it0)
        return {"times": times, "loop_launches": launches, "trials": trials, "trial_graph": int(info["trial_graph"]),
                "device_loop": int(info["device_loop"]), "steps_local": int(eng.layout_info()["steps_local"])}
    finally:
        eng.close()


def table(files, out):
    runs = [json.load(open(f)) for f in files]
    lines = ["# tools/steps_qp_bench.py: one call = `steps` adaptive take_steps of one engine (K = 1); best of `reps` calls, each from the origin",
             "# and `warm` steps; wall time includes the device; spread = (worst - best) / best; us/step = best / steps; us/trial counts",
             "# the rejected trials too; loop launches: multi-step launches during the timed calls (0: launch by launch)",
             f"{'shape':<15} {'kind':<4} {'library / setting':<28} {'call ms':>9} {'steps/s':>9} {'us/step':>8} {'us/trial':>9} {'spread':>7} {'loop launches':>14} {'local':>6}"]
    keys = []
    for r in runs:
        for k in r["rows"]:
            if k not in keys:
                keys.append(k)
    for k in keys:
        for r in runs:
            if k not in r["rows"]:
                continue
            row, steps, reps = r["rows"][k], r["steps"], r["reps"]
            best = min(row["times"])
            shape, kind = k.split("/")
            lines.append(f"{shape:<15} {kind:<4} {r['label']:<28} {1e3 * best:>9.3f} {steps / best:>9.0f} {1e6 * best / steps:>8.2f} "
                         f"{1e6 * best * reps / max(row['trials'], 1):>9.2f} {(max(row['times']) - best) / best:>7.2f} {row['loop_launches']:>14} {row['steps_local']:>6}")
        lines.append("")
    text = "\n".join(lines)
    print(text)
    if out:
        with open(out, "w") as fh:
            fh.write(text + "\n")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--kinds", default="lp,qp")
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--warm", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--label", default=None)
    ap.add_argument("--json", default=None)
    ap.add_argument("--table", nargs="+", default=None, help="--json files of earlier invocations: print them side by side")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if args.table:
        table(args.table, args.out)
        return
    label = args.label or f"PDHG_DEVICE_LOOP={os.environ.get('PDHG_DEVICE_LOOP', 'unset')}"
    rows = {}
    for shape in args.shapes.split(","):
        for kind in args.kinds.split(","):
            r = measure(problem(shape, kind), args.steps, args.warm, args.reps)
            rows[f"{shape}/{kind}"] = r
            best = min(r["times"])
            print(f"{shape:<15} {kind:<4} {label:<28} {1e3 * best:9.3f} ms  {args.steps / best:9.0f} steps/s  spread {(max(r['times']) - best) / best:.2f}  "
                  f"loop launches {r['loop_launches']}  trial_graph {r['trial_graph']}", flush=True)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump({"label": label, "steps": args.steps, "warm": args.warm, "reps": args.reps, "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
