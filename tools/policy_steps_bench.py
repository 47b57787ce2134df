"""What a take_step costs under each step-size policy: `take_steps(policy, state, steps)` on one engine, and the same
batch for K members through optimize_many's stepping call.

    python tools/policy_steps_bench.py [--shapes netlib27x32,netlib56x97,random1000x800] [--ks 64,256] [--steps 256]
                                       [--warm 512] [--reps 5] [--qp] [--policies adaptive,constant,malitsky_pock]
                                       [--json OUT.json] [--baseline PARENT.json] [--out TABLE.txt]

Policies: adaptive (0.3, 0.6) as the control, constant, Malitsky-Pock (0.7, 0.99, 1.0).  Shapes: those of
tools/fleet_bench.py.  Every measurement starts from a warmed state -- `warm` steps of the policy, so that the
Malitsky-Pock average is not empty -- and is the best of `reps` wall times of one call (the call returns after the
results have arrived, so the wall time includes the device); the other repetitions are kept, for the run-to-run spread.
Solo: one HipPdhgEngine.  K members: one HipPdhgFleet, stepped by fleet.py's stepping function, as optimize_many does
between two evaluations.

--qp adds QP members of the same shapes (rows `<shape>+Q`): the same random_lp seeds plus Q = B'B + diag (B: n/3 x n with
three entries per column on average), under the adaptive and the constant policy (Malitsky-Pock takes LPs only).  A
shape whose QP does not pass the one-workgroup kernel's LDS rule, 8 (11 n + 4 m) <= 144 KiB, is left out and named.  Run
it with PDHG_SMALL_QP=1 to time the one-workgroup QP kernels, without it (or at an older checkout) to time the
per-launch path.  The QP rows start every repetition from the origin and --qp-warm steps (default 64): these small strongly
convex QPs reach their fixed point to the last bit within a thousand steps or so, where the adaptive rule stops with
numerical_error (zero movement), so a state carried through 512 + 5 x 256 steps cannot be timed.

The tool uses only names that older checkouts have as well (take_steps, HipPdhgEngine, HipPdhgFleet, the fleet's stepping
function), so the same file measures a checkout from before the policies' native calls: run it there with --json, then
here with --baseline pointing at that file, and the table gains the earlier it/s and the ratio.
"""
import argparse
import json
import os
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"netlib27x32": (27, 32, 4), "netlib56x97": (56, 97, 4), "random1000x800": (1000, 800, 10)}


def qp_fits(shape):
    m, n, _ = SHAPES[shape]
    return 8 * (11 * n + 4 * m) <= 144 * 1024


def members(shape, K, qp=False):
    from firstorderlp_jl_amd.generators import random_lp
    m, n, per_row = SHAPES[shape]
    lps = [random_lp(m, n, per_row, seed=7000 + k) for k in range(K)]
    if not qp:
        return lps
    import scipy.sparse as sp
    from firstorderlp_jl_amd.quadratic_programming import QuadraticProgrammingProblem
    out = []
    for k, p in enumerate(lps):
        B = sp.random(max(n // 3, 1), n, density=3.0 / n, format="csr", random_state=8000 + k)
        Q = (B.T @ B + sp.diags(np.linspace(0.0, 0.5, n))).tocsc()
        Q.sort_indices()
        out.append(QuadraticProgrammingProblem(p.variable_lower_bound, p.variable_upper_bound, Q, p.objective_vector, 0.0,
                                               p.constraint_matrix, p.right_hand_side, p.num_equalities))
    return out


def policies():
    from firstorderlp_jl_amd.primal_dual_hybrid_gradient import (AdaptiveStepsizeParams, ConstantStepsizeParams,
                                                                 MalitskyPockStepsizeParameters)
    return {"adaptive": AdaptiveStepsizeParams(0.3, 0.6), "constant": ConstantStepsizeParams(),
            "malitsky_pock": MalitskyPockStepsizeParameters(0.7, 0.99, 1.0)}


def first_step(p, name):
    """1 / max |a_ij| (pdhg.jl:821-826) for the two policies that adapt it; for the constant one a step size that is safe
    whatever the matrix: 1 / sqrt(|A|_1 |A|_inf) <= 1 / |A|_2."""
    A = abs(p.constraint_matrix)
    if name == "constant":
        step = float(1.0 / np.sqrt(A.sum(axis=0).max() * A.sum(axis=1).max()))
        Q = p.objective_matrix
        if Q is not None and Q.nnz > 0:      # a QP: tau |Q|_2 <= 1 as well (primal weight 1: tau = step)
            Qa = abs(Q)
            step = min(step, float(1.0 / np.sqrt(Qa.sum(axis=0).max() * Qa.sum(axis=1).max())))
        return step
    return float(1.0 / A.data.max())


def new_state(eng, p, name):
    from firstorderlp_jl_amd.primal_dual_hybrid_gradient import PdhgSolverState
    return PdhgSolverState(eng, step_size=first_step(p, name), primal_weight=1.0, ratio_step_sizes=1.0)


def solo_seconds(p, name, policy, steps, warm, reps, from_origin=False):
    import folp_loader
    from firstorderlp_jl_amd.primal_dual_hybrid_gradient import take_steps
    pkg = folp_loader.load()
    eng = pkg.HipPdhgEngine.from_problem(p, device_id=0)
    try:
        st = new_state(eng, p, name)
        take_steps(policy, st, warm)
        times = []
        for rep in range(reps):
            if from_origin and rep > 0:
                eng.set_current(np.zeros(eng.n), np.zeros(eng.m))
                eng.reset_average()
                st = new_state(eng, p, name)
                take_steps(policy, st, warm)
            t0 = time.perf_counter()
            done = take_steps(policy, st, steps)
            times.append(time.perf_counter() - t0)
            if done != steps or st.numerical_error:
                raise RuntimeError(f"{name}: the engine stopped on a numerical error")
        return times
    finally:
        eng.close()


def fleet_seconds(fleet, problems, K, name, policy, steps, warm, reps, is_lp=True, from_origin=False):
    import firstorderlp_jl_amd.fleet as fl
    step_fleet = getattr(fl, "_take_member_steps", None) or fl._step_fleet
    solves = []
    for eng, p in zip(fleet.members, problems):
        eng.set_current(np.zeros(eng.n), np.zeros(eng.m))
        eng.reset_average()
        solves.append(types.SimpleNamespace(state=new_state(eng, p, name), is_lp=is_lp))
    def restart():
        for mb, eng, p in zip(solves, fleet.members, problems):
            eng.set_current(np.zeros(eng.n), np.zeros(eng.m))
            eng.reset_average()
            mb.state = new_state(eng, p, name)
        step_fleet(fleet, solves, policy, [(mb, warm) for mb in solves[:K]])

    step_fleet(fleet, solves, policy, [(mb, warm) for mb in solves[:K]])
    times = []
    for rep in range(reps):
        if from_origin and rep > 0:
            restart()
        t0 = time.perf_counter()
        got = step_fleet(fleet, solves, policy, [(mb, steps) for mb in solves[:K]])
        times.append(time.perf_counter() - t0)
        if any(done != steps for _, done, _ in got):
            raise RuntimeError(f"{name}: a member stopped on a numerical error")
    return times


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--ks", default="64,256")
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--warm", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--qp", action="store_true", help="QP members of the shapes as well (rows <shape>+Q)")
    ap.add_argument("--qp-warm", type=int, default=64, help="warming steps of the QP rows, taken from the origin before EVERY repetition")
    ap.add_argument("--policies", default="adaptive,constant,malitsky_pock")
    ap.add_argument("--json", default=None, help="write the measurements here (a later run's --baseline)")
    ap.add_argument("--baseline", default=None, help="measurements of another checkout (its --json): adds its it/s and the ratio")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    import folp_loader
    pkg = folp_loader.load()
    ks = [int(k) for k in args.ks.split(",") if k]
    base = json.load(open(args.baseline)) if args.baseline else {}
    rows = {}
    lines = [f"# tools/policy_steps_bench.py --shapes {args.shapes} --ks {args.ks} --steps {args.steps} --warm {args.warm} --reps {args.reps}"
             + (" --qp" if args.qp else "") + f" --policies {args.policies}" + f"    (PDHG_SMALL_QP={os.environ.get('PDHG_SMALL_QP', 'unset')})",
             "# one call = `steps` take_steps of each of K members (K = 1: one engine); best of `reps` calls after `warm` steps; wall time "
             "includes the device; spread = (worst - best) / best of the repetitions",
             f"{'shape':<17} {'policy':<14} {'K':>4} {'call ms':>9} {'member-it/s':>12} {'spread':>7}"
             + (f" {'baseline it/s':>14} {'ratio':>7}" if base else "")]
    print("\n".join(lines), flush=True)

    def emit(shape, name, K, times):
        best = min(times)
        rate = K * args.steps / best
        key = f"{shape}/{name}/{K}"
        rows[key] = {"times": times, "rate": rate}
        line = f"{shape:<17} {name:<14} {K:>4} {1e3 * best:>9.3f} {rate:>12.0f} {(max(times) - best) / best:>7.2f}"
        if key in base:
            line += f" {base[key]['rate']:>14.0f} {rate / base[key]['rate']:>7.2f}"
        print(line, flush=True)
        lines.append(line)

    wanted = [w for w in args.policies.split(",") if w]
    qp_warm = args.qp_warm
    for shape in args.shapes.split(","):
        for qp in ([False, True] if args.qp else [False]):
            if qp and not qp_fits(shape):
                lines.append(f"# {shape}+Q: 8 (11 n + 4 m) > 144 KiB -- not of the one-workgroup class, left out")
                print(lines[-1], flush=True)
                continue
            label = shape + ("+Q" if qp else "")
            chosen = {k: v for k, v in policies().items() if k in wanted and not (qp and k == "malitsky_pock")}
            problems = members(shape, max(ks + [1]), qp)
            for name, policy in chosen.items():
                emit(label, name, 1, solo_seconds(problems[0], name, policy, args.steps, qp_warm if qp else args.warm, args.reps, qp))
            if ks:
                fleet = pkg.HipPdhgFleet.from_problems(problems, device_id=0)
                try:
                    for name, policy in chosen.items():
                        for K in ks:
                            emit(label, name, K, fleet_seconds(fleet, problems, K, name, policy, args.steps, qp_warm if qp else args.warm, args.reps, not qp, qp))
                finally:
                    fleet.close()
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(rows, fh, indent=1)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
