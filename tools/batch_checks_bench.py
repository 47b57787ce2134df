"""Whole ``optimize_batch`` solves with a batch's checks in shared launches (PDHG_BATCH_CHECKS=1) against the same solves
with every member checking on its own (the default), and against another built checkout (the parent commit).

    python tools/batch_checks_bench.py [--families pagerank,l1svm,random,qp] [--k 8] [--reps 3]
                                       [--iteration-limit 2000] [--random-limit 200] [--against OTHER_CHECKOUT]
                                       [--out profiles/batch_checks_throughput.txt]
    python tools/batch_checks_bench.py --kernels FAMILY        (under rocprofv3 --kernel-trace --stats: see below)

Families (tools/batch_bench.py's, and one QP): "pagerank" = personalized PageRank on the 1M-node PageRank LP; "l1svm" =
the L1-SVM regularization path on the rcv1-like data; "random" = the 10M x 10M, 100M-nnz random LP with per-member c and
b, stopped at --random-limit iterations; "qp" = ``generators.random_qp_family`` 1M x 1M.  Parameters: solve_qp's defaults
(Ruiz-10 + Pock-Chambolle, adaptive steps, adaptive-normalized restarts, an evaluation every 40 iterations), tolerance
1e-6.

Per family the problems are built once; then --reps rounds, each round one solve per side, the sides alternating:
"parent" (with --against: a child process of this file over the other checkout's package and library, which keeps its
problems and waits for its turn), "off" (PDHG_BATCH_CHECKS unset) and "on" (=1), the last two in this process on one
library.  Reported per side: the best wall time per solve, the spread (worst - best) / best, the share of the best
solve's wall time spent in the checks (everything ``_Solve.evaluate`` / ``_check_round`` does, device waits included),
iterations of member 0, and for "on" the batch's ``check_info()``.  "on" must return "off"'s outputs bit for bit (checked).

--kernels FAMILY runs, in one process, one "on" solve of FAMILY and then K single plain products of the same shape per
matrix (every member's own ``eval_point`` after a step), so that one ``rocprofv3 --kernel-trace --stats -- python
tools/batch_checks_bench.py --kernels FAMILY`` shows the durations of the new kernels and of the batched plain products
beside the members' own.
"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def _root(argv):
    """The checkout whose package is imported: --root DIR (the child of --against), else this file's."""
    if "--root" in argv:
        return os.path.abspath(argv[argv.index("--root") + 1])
    return os.path.dirname(HERE)


ROOT = _root(sys.argv)
sys.path.insert(0, ROOT)
sys.path.insert(1, HERE)


def problems_of(family, K):
    import folp_loader
    folp_loader.load()            # (from ROOT, before batch_bench puts its own checkout in front)
    from batch_bench import members, qp_members
    if family == "qp":
        return qp_members("1000000x1000000", K)
    return members(family, K)


def solve_params(iteration_limit):
    from firstorderlp_jl_amd.primal_dual_hybrid_gradient import AdaptiveStepsizeParams, PdhgParameters
    from firstorderlp_jl_amd.saddle_point import RestartScheme, RestartToCurrentMetric, construct_restart_parameters
    from firstorderlp_jl_amd.termination import construct_termination_criteria
    tc = construct_termination_criteria(eps_optimal_absolute=1e-6, eps_optimal_relative=1e-6, iteration_limit=iteration_limit)
    rp = construct_restart_parameters(RestartScheme.ADAPTIVE_NORMALIZED, RestartToCurrentMetric.GAP_OVER_DISTANCE_SQUARED,
                                      1000, 0.5, 0.1, 0.9, 0.5, False)
    return PdhgParameters(10, False, 1.0, 1.0, True, 0, False, 40, tc, rp, AdaptiveStepsizeParams(0.3, 0.6))


def one_solve(problems, params, switch):
    """(wall seconds, seconds in the checks, outputs, check_info or None) of one optimize_batch."""
    import folp_loader
    folp_loader.load()
    import firstorderlp_jl_amd.primal_dual_hybrid_gradient as pd
    from firstorderlp_jl_amd import HipPdhgBatch, optimize_batch
    if switch:
        os.environ["PDHG_BATCH_CHECKS"] = "1"
    else:
        os.environ.pop("PDHG_BATCH_CHECKS", None)
    spent, depth = [0.0], [0]
    inner = {"evaluate": pd._Solve.evaluate, "round": pd._check_round}

    def timed(which):
        def run(*a):
            depth[0] += 1
            t = time.perf_counter()
            try:
                return inner[which](*a)
            finally:
                depth[0] -= 1
                if depth[0] == 0:
                    spent[0] += time.perf_counter() - t
        return run
    info = [None]

    def factory(ps):
        batch = HipPdhgBatch.from_problems(ps)
        close = batch.close

        def closing():
            if hasattr(batch, "check_info"):
                info[0] = batch.check_info()
            close()
        batch.close = closing
        return batch
    factory.takes_original_problem = True
    pd._Solve.evaluate = timed("evaluate")
    pd._check_round = timed("round")
    try:
        t0 = time.perf_counter()
        outs = optimize_batch(params, problems, batch_factory=factory)
        wall = time.perf_counter() - t0
    finally:
        pd._Solve.evaluate = inner["evaluate"]
        pd._check_round = inner["round"]
        os.environ.pop("PDHG_BATCH_CHECKS", None)
    return wall, spent[0], outs, info[0]


def serve(family, K, limit):
    """The child of --against: builds the problems, then one "off" solve per line read from stdin."""
    problems = problems_of(family, K)
    params = solve_params(limit)
    print("READY", flush=True)
    for line in sys.stdin:
        if line.strip() != "go":
            break
        wall, checks, outs, _ = one_solve(problems, params, False)
        print(f"T {wall!r} {checks!r} {outs[0].iteration_count}", flush=True)


def same_outputs(a, b):
    return all(x.termination_reason == y.termination_reason and x.iteration_count == y.iteration_count and
               np.array_equal(x.primal_solution, y.primal_solution, equal_nan=True) and
               np.array_equal(x.dual_solution, y.dual_solution, equal_nan=True) for x, y in zip(a, b))


def family_rows(family, K, reps, limit, against, emit):
    child = None
    if against:
        child = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--serve", family, "--k", str(K), "--limit", str(limit),
                                  "--root", against], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
    try:
        problems = problems_of(family, K)
        params = solve_params(limit)
        if child and child.stdout.readline().strip() != "READY":
            raise RuntimeError("the child over the other checkout did not come up")
        one_solve(problems, params, False)                     # warm-up: first-launch costs, allocations
        runs = {"parent": [], "off": [], "on": []}
        info, differ = None, 0
        for _ in range(reps):
            if child:
                child.stdin.write("go\n")
                child.stdin.flush()
                _, wall, checks, its = child.stdout.readline().split()
                runs["parent"].append((float(wall), float(checks), int(its)))
            wall, checks, off, _ = one_solve(problems, params, False)
            runs["off"].append((wall, checks, off[0].iteration_count))
            wall, checks, on, info = one_solve(problems, params, True)
            runs["on"].append((wall, checks, on[0].iteration_count))
            differ += 0 if same_outputs(on, off) else 1
        for side in ("parent", "off", "on"):
            rs = runs[side]
            if not rs:
                continue
            best = min(rs)
            spread = (max(r[0] for r in rs) - best[0]) / best[0]
            emit(f"{family:<9} {K:>3} {side:<7} {1e3 * best[0]:>10.1f} {100 * spread:>7.1f}% {100 * best[1] / best[0]:>7.1f}% "
                 f"{1e3 * best[1]:>10.1f} {best[2]:>7}")
        emit(f"#   {family}: 'on' differs from 'off' in {differ} of {reps} rounds; check_info of the last 'on' solve: {info}")
    finally:
        if child:
            try:
                child.stdin.close()
            except Exception:
                pass
            child.wait(timeout=60)


def kernels(family, K, limit):
    """One 'on' solve, then every member's own products at its current point (K single products per matrix)."""
    import folp_loader
    folp_loader.load()
    from firstorderlp_jl_amd import HipPdhgBatch, _lib
    problems = problems_of(family, K)
    one_solve(problems, solve_params(limit), True)
    batch = HipPdhgBatch.from_problems(problems)
    try:
        E, D = batch.rescale(10, False, 1.0)
        for p, eng in zip(problems, batch.members):
            eng.set_original_problem(E, D, p.objective_vector, p.right_hand_side, p.variable_lower_bound, p.variable_upper_bound)
        ss = np.full(K, 1.0 / batch.members[0].matrix_max_abs())
        batch.take_steps_adaptive(5, 0.3, 0.6, ss, np.ones(K), np.zeros(K, dtype=np.int64), np.zeros(K))
        for eng in batch.members:
            eng.eval_point(_lib.POINT_CURRENT)
    finally:
        batch.close()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--families", default="pagerank,l1svm,random,qp")
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--iteration-limit", type=int, default=2000)
    ap.add_argument("--random-limit", type=int, default=200)
    ap.add_argument("--against", default=None, help="another built checkout (the parent commit): its solves under this file, alternating")
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernels", default=None, metavar="FAMILY")
    ap.add_argument("--serve", default=None, metavar="FAMILY", help=argparse.SUPPRESS)
    ap.add_argument("--limit", type=int, default=2000, help=argparse.SUPPRESS)
    ap.add_argument("--root", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args(argv)
    if args.serve:
        return serve(args.serve, args.k, args.limit)
    if args.kernels:
        return kernels(args.kernels, args.k, args.random_limit if args.kernels == "random" else args.iteration_limit)
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    emit(f"# whole optimize_batch solves, K = {args.k}: solve_qp defaults, tolerance 1e-6, iteration limit {args.iteration_limit} "
         f"(random: {args.random_limit}); PDHG_ROW_ORDER={os.environ.get('PDHG_ROW_ORDER', 'relaxed')}")
    emit(f"# sides alternate, {args.reps} rounds: best wall ms per solve, spread (worst - best) / best, share and ms of the best solve "
         "spent in the checks; parent = the other checkout's library and package under this file")
    emit(f"{'family':<9} {'K':>3} {'side':<7} {'ms/solve':>10} {'spread':>8} {'checks':>8} {'checks ms':>10} {'it[0]':>7}")
    for family in args.families.split(","):
        limit = args.random_limit if family == "random" else args.iteration_limit
        family_rows(family, args.k, args.reps, limit, args.against, emit)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
