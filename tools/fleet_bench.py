"""Throughput of a fleet of independent small LPs (pdhg_fleet_take_steps_adaptive, optimize_many) against the
single-LP engine and a Python loop of optimize.

    python tools/fleet_bench.py [--shapes netlib27x32,netlib56x97,random1000x800] [--ks 1,8,64,256,1024] [--steps 256]
                                [--reps 5] [--solve-ks 1,8,64,256] [--qp] [--out profiles/fleet_throughput.txt]

Members: `random_lp(m, n)` of the shape, a distinct seed per member ("netlib27x32", "netlib56x97": the shapes of the
reference's smallest Netlib runs, BASELINE configs[1]; "random1000x800": near the upper end of what one workgroup holds).
`--qp`: the same LPs plus Q = B'B + diag, as tools/policy_steps_bench.py --qp builds them (run it with PDHG_SMALL_QP=1 to
have the fleet carry them in its shared step and check launches; without, they are stepped and checked member by member).

Stepping: one fleet of max(ks) members per shape; the K-member measurement passes n_steps = 0 for the others.  A timed
call takes `steps` take_steps of every member (the call returns after every member's results have arrived, so the wall
time includes the device); best of `reps`.  member-it/s = K * steps / call time; the solo figure is
pdhg_take_steps_adaptive of `steps` steps on a solo handle of member 0's LP, measured the same way in the same run.
Model: up to one workgroup per compute unit the members run side by side, so the kernel time of a shared launch should be
a solo launch's and the ratio to solo K * (solo call time / fleet call time).  Beside the wall time the table gives the
shared launch's KERNEL duration -- from a `rocprofv3 --kernel-trace --stats` run of a child process of its own (no
counters) at --profile-k members -- and the host's part of a call: the tables of powers, the argument table and its
upload, and the K result waits behind the kernel (wall - kernel).

Whole solves: optimize_many on K members against a Python loop of optimize over (at most --loop-cap of) the same
members, at solve_qp's defaults (Ruiz-10 + Pock-Chambolle, adaptive steps, adaptive-normalized restarts, an evaluation
every 40 iterations, tolerance 1e-6), solves per second, and the share of optimize_many's wall time spent inside the
evaluations -- `_check_round` where the fleet takes the checks of all members in shared launches (eval_points,
trust_region_bounds), `_Solve.evaluate` where they run member by member -- with the fleet's `check_info()` at the end of
the solve: launches of the three check kernels, and the members' own eval_point / trust_region_bound calls that no
shared launch had answered (`misses`).  `--solve-reps N` repeats every whole-solve measurement and reports the best
optimize_many time and the spread; `--check-kernels` adds the kernel durations of the three check kernels at
--profile-k members from a `rocprofv3 --kernel-trace --stats` run of a child of its own.
"""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"netlib27x32": (27, 32, 4), "netlib56x97": (56, 97, 4), "random1000x800": (1000, 800, 10)}


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


def _start(problems):
    ss = np.array([1.0 / np.abs(p.constraint_matrix.data).max() for p in problems])
    K = len(problems)
    return ss, np.ones(K), np.zeros(K, dtype=np.int64), np.zeros(K)


def solo_call_seconds(p, steps, reps):
    import folp_loader
    pkg = folp_loader.load()
    eng = pkg.HipPdhgEngine.from_problem(p, device_id=0)
    try:
        s, it, kkt = 1.0 / eng.matrix_max_abs(), 0, 0.0
        s, it, kkt, _, _ = eng.take_steps_adaptive(steps, 0.3, 0.6, s, 1.0, it, kkt)          # warm-up: the same shape of call
        best = np.inf
        for _ in range(reps):
            t0 = time.perf_counter()
            s, it, kkt, err, done = eng.take_steps_adaptive(steps, 0.3, 0.6, s, 1.0, it, kkt)
            best = min(best, time.perf_counter() - t0)
            if done != steps or err:
                raise RuntimeError("the solo handle stopped on a numerical error")
        return best
    finally:
        eng.close()


def fleet_call_seconds(fleet, problems, ks, steps, reps):
    """{K: (best call seconds, members that stopped on a numerical error)} on one fleet; every K starts its K members
    from the zero iterate, as the solo handle starts."""
    out = {}
    for K in ks:
        ss, pw, it, kkt = _start(problems)
        for eng in fleet.members[:K]:
            eng.set_current(np.zeros(eng.n), np.zeros(eng.m))
            eng.reset_average()
        ns = np.zeros(len(problems), dtype=np.int64)
        ns[:K] = steps
        ss, it, kkt, _, _ = fleet.take_steps_adaptive(ns, 0.3, 0.6, ss, pw, it, kkt)           # warm-up at this K
        best, stopped = np.inf, 0
        for _ in range(reps):
            t0 = time.perf_counter()
            ss, it, kkt, err, done = fleet.take_steps_adaptive(ns, 0.3, 0.6, ss, pw, it, kkt)
            dt = time.perf_counter() - t0
            stopped = max(stopped, int((done[:K] != steps).sum()))
            if (done[:K] == steps).all():
                best = min(best, dt)
        info = fleet.info()
        if info["carried"] != K:
            raise RuntimeError(f"the shared launch carried {info['carried']} of {K} members")
        out[K] = (best, stopped)
    return out


def child_launch(shape, K, steps, qp=False):
    """What the profiled child runs: a fleet of K members, a warm-up call and three calls of `steps` steps."""
    import folp_loader
    pkg = folp_loader.load()
    problems = members(shape, K, qp)
    fleet = pkg.HipPdhgFleet.from_problems(problems, device_id=0)
    try:
        ss, pw, it, kkt = _start(problems)
        for _ in range(4):
            ss, it, kkt, _, _ = fleet.take_steps_adaptive(np.full(K, steps), 0.3, 0.6, ss, pw, it, kkt)
    finally:
        fleet.close()


def kernel_us(shape, K, steps, qp=False, timeout=300):
    """Average duration (us) of small_lp_fleet_kernel (--qp: small_qp_fleet_kernel) in a `rocprofv3 --kernel-trace --stats`
    run of a child of its own, or a string saying why there is none."""
    kernel = "small_qp_fleet_kernel" if qp else "small_lp_fleet_kernel"
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from rocprof_summary import summarize
    rp = shutil.which("rocprofv3")
    if not rp:
        return "rocprofv3 not on PATH"
    work = tempfile.mkdtemp(prefix="pdhg_fleet_prof_", dir="/tmp")
    try:
        cmd = [rp, "--kernel-trace", "--stats", "-d", work, "--", sys.executable, os.path.abspath(__file__), "--child", shape, str(K), str(steps)] + (["--qp"] if qp else [])
        r = subprocess.run(cmd, cwd="/tmp", env=dict(os.environ, TMPDIR="/tmp"), timeout=timeout, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
        if r.returncode != 0:
            return f"profiled child failed ({r.returncode}): {r.stderr.decode(errors='replace')[-200:]}"
        rows = [k for k in summarize(work) if kernel in k["name"]]
        if not rows:
            return f"no {kernel} in the trace"
        # (the calls of one instantiation are the warm-up and three timed-like calls: their average)
        return max(k["avg_us"] for k in rows)
    except subprocess.TimeoutExpired:
        return f"profiled child timed out after {timeout} s"
    finally:
        shutil.rmtree(work, ignore_errors=True)


def solve_params(iteration_limit):
    from firstorderlp_jl_amd.primal_dual_hybrid_gradient import AdaptiveStepsizeParams, PdhgParameters
    from firstorderlp_jl_amd.saddle_point import RestartScheme, RestartToCurrentMetric, construct_restart_parameters
    from firstorderlp_jl_amd.termination import construct_termination_criteria
    tc = construct_termination_criteria(eps_optimal_absolute=1e-6, eps_optimal_relative=1e-6, iteration_limit=iteration_limit)
    rp = construct_restart_parameters(RestartScheme.ADAPTIVE_NORMALIZED, RestartToCurrentMetric.GAP_OVER_DISTANCE_SQUARED,
                                      1000, 0.5, 0.1, 0.9, 0.5, False)
    return PdhgParameters(10, False, 1.0, 1.0, True, 0, False, 40, tc, rp, AdaptiveStepsizeParams(0.3, 0.6))


def whole_solves(problems, K, loop_cap, iteration_limit, with_loop=True):
    """(optimize_many solves/s, share of its wall time in the evaluations, loop solves/s, loop members, solves that
    differ from the loop's, the fleet's check_info() at the end or None)"""
    import firstorderlp_jl_amd.primal_dual_hybrid_gradient as pd
    import firstorderlp_jl_amd.fleet as fl
    from firstorderlp_jl_amd import optimize_many
    params = solve_params(iteration_limit)
    spent = [0.0]
    depth = [0]
    inner = {"evaluate": pd._Solve.evaluate, "round": getattr(pd, "_check_round", None)}

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
        fleet = fl.HipPdhgFleet.from_problems(ps)
        close = fleet.close

        def closing():
            if getattr(fleet, "_h", None) and hasattr(fleet, "check_info"):
                info[0] = fleet.check_info()
            close()
        fleet.close = closing
        return fleet
    factory.takes_original_problem = True
    pd._Solve.evaluate = timed("evaluate")
    if inner["round"]:
        pd._check_round = timed("round")
    try:
        t0 = time.perf_counter()
        outs = optimize_many(params, problems[:K], fleet_factory=factory)
        many = time.perf_counter() - t0
        in_checks = spent[0]
    finally:
        pd._Solve.evaluate = inner["evaluate"]
        if inner["round"]:
            pd._check_round = inner["round"]
    if not with_loop:
        return K / many, in_checks / many, None, 0, 0, info[0]
    n_loop = min(K, loop_cap)
    t0 = time.perf_counter()
    solo = [pd.optimize(params, p) for p in problems[:n_loop]]
    loop = time.perf_counter() - t0
    differ = sum(1 for a, b in zip(outs, solo)
                 if a.iteration_count != b.iteration_count or not np.array_equal(a.primal_solution, b.primal_solution))
    return K / many, in_checks / many, n_loop / loop, n_loop, differ, info[0]


def child_solve(shape, K, iteration_limit, qp=False):
    """What the profiled child of --check-kernels runs: one optimize_many of K members."""
    from firstorderlp_jl_amd import optimize_many
    optimize_many(solve_params(iteration_limit), members(shape, K, qp))


CHECK_KERNELS = ("fleet_point_products_kernel", "fleet_eval_kernel", "fleet_tr_kernel", "small_lp_fleet_kernel",
                 "fleet_qp_point_products_kernel", "fleet_qp_eval_kernel", "small_qp_fleet_kernel")


def check_kernels_us(shape, K, iteration_limit, qp=False, timeout=400):
    """{kernel: (calls, average us)} of the check kernels (and the shared step kernels) in a `rocprofv3 --kernel-trace --stats` run of a child of
    its own, or a string saying why there is none."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from rocprof_summary import summarize
    rp = shutil.which("rocprofv3")
    if not rp:
        return "rocprofv3 not on PATH"
    work = tempfile.mkdtemp(prefix="pdhg_fleet_prof_", dir="/tmp")
    try:
        cmd = [rp, "--kernel-trace", "--stats", "-d", work, "--", sys.executable, os.path.abspath(__file__), "--child-solve", shape, str(K),
               str(iteration_limit)] + (["--qp"] if qp else [])
        r = subprocess.run(cmd, cwd="/tmp", env=dict(os.environ, TMPDIR="/tmp"), timeout=timeout, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
        if r.returncode != 0:
            return f"profiled child failed ({r.returncode}): {r.stderr.decode(errors='replace')[-200:]}"
        out = {}
        for k in summarize(work):
            # (a traced name is "[void ](anonymous namespace)::kernel[<256>](arguments)": the kernel and its template arguments)
            hit = re.search(r"\b(" + "|".join(CHECK_KERNELS) + r")(<[^>]*>)?\(", k["name"])
            if hit:
                out[hit.group(1) + (hit.group(2) or "")] = (k.get("calls"), k["avg_us"])
        return out or "no check kernel in the trace"
    except subprocess.TimeoutExpired:
        return f"profiled child timed out after {timeout} s"
    finally:
        shutil.rmtree(work, ignore_errors=True)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--ks", default="1,8,64,256,1024")
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--solve-ks", default="1,8,64,256")
    ap.add_argument("--loop-cap", type=int, default=16, help="the Python loop of optimize runs over at most this many members")
    ap.add_argument("--iteration-limit", type=int, default=5000)
    ap.add_argument("--profile-k", type=int, default=256)
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--solve-reps", type=int, default=1, help="repeat every whole-solve measurement; report the best and the spread")
    ap.add_argument("--check-kernels", action="store_true", help="kernel durations of the check kernels (a rocprofv3 run of its own)")
    ap.add_argument("--qp", action="store_true", help="QP members: the shape's LPs plus Q = B'B + diag (PDHG_SMALL_QP=1 lets the fleet carry them)")
    ap.add_argument("--child", nargs=3, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--child-solve", nargs=3, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args(argv)
    import folp_loader
    pkg = folp_loader.load()
    if args.child:
        child_launch(args.child[0], int(args.child[1]), int(args.child[2]), args.qp)
        return
    if args.child_solve:
        child_solve(args.child_solve[0], int(args.child_solve[1]), int(args.child_solve[2]), args.qp)
        return
    ks = [int(k) for k in args.ks.split(",") if k]
    solve_ks = [int(k) for k in args.solve_ks.split(",") if k]
    lines = [f"# tools/fleet_bench.py --shapes {args.shapes} --ks {args.ks} --steps {args.steps} --reps {args.reps} "
             f"--solve-ks {args.solve_ks} --loop-cap {args.loop_cap} --iteration-limit {args.iteration_limit} --solve-reps {args.solve_reps}"
             + (f" --qp    (PDHG_SMALL_QP={os.environ.get('PDHG_SMALL_QP', 'unset')})" if args.qp else ""),
             "# stepping: one call = `steps` take_steps of each of K members; best of `reps` calls; wall time includes the device",
             f"{'shape':<15} {'K':>5} {'call ms':>9} {'member-it/s':>12} {'solo call ms':>12} {'solo it/s':>10} {'ratio':>7}"]
    print("\n".join(lines), flush=True)

    def emit(line):
        print(line, flush=True)
        lines.append(line)

    shapes = args.shapes.split(",")
    for shape in shapes if ks else []:
        problems = members(shape, max(ks), args.qp)
        solo = solo_call_seconds(problems[0], args.steps, args.reps)
        fleet = pkg.HipPdhgFleet.from_problems(problems, device_id=0)
        try:
            calls = fleet_call_seconds(fleet, problems, ks, args.steps, args.reps)
        finally:
            fleet.close()
        stopped = {K: v[1] for K, v in calls.items() if v[1]}
        calls = {K: v[0] for K, v in calls.items()}
        for K in ks:
            rate = K * args.steps / calls[K]
            emit(f"{shape:<15} {K:>5} {1e3 * calls[K]:>9.3f} {rate:>12.0f} {1e3 * solo:>12.3f} {args.steps / solo:>10.0f} "
                 f"{rate / (args.steps / solo):>7.2f}")
        if stopped:
            emit(f"# {shape}: members that stopped on a numerical error in a timed call (those calls are not counted): {stopped}")
        if not args.no_profile:
            K = min(args.profile_k, max(ks))
            us = kernel_us(shape, K, args.steps, args.qp)
            if isinstance(us, str):
                emit(f"# {shape}: kernel duration of the shared launch at K = {K}: not measured ({us})")
            elif K in calls:
                emit(f"# {shape}: shared launch at K = {K}: kernel {1e-3 * us:.3f} ms (rocprofv3 --kernel-trace --stats, a run of its own) of "
                     f"{1e3 * calls[K]:.3f} ms wall; the rest, {1e3 * calls[K] - 1e-3 * us:.3f} ms, is the host's: tables of powers, "
                     f"argument table + upload, {K} result waits; a solo call is {1e3 * solo:.3f} ms")
            else:
                emit(f"# {shape}: shared launch at K = {K}: kernel {1e-3 * us:.3f} ms (rocprofv3 --kernel-trace --stats, a run of its own)")
        del problems
    if solve_ks:
        emit(f"# whole solves: solve_qp defaults, tolerance 1e-6, iteration limit {args.iteration_limit}; the loop of optimize runs over "
             f"the first min(K, {args.loop_cap}) members")
        emit(f"{'shape':<15} {'K':>5} {'many solves/s':>13} {'loop solves/s':>13} {'ratio':>7} {'share in checks':>15} {'loop over':>9}"
             f"   (many solves/s: best of {args.solve_reps}; check_info() of the fleet at the end of the solve)")
    for shape in shapes if solve_ks else []:
        problems = members(shape, max(solve_ks), args.qp)
        for K in solve_ks:
            many, share, loop, n_loop, differ, info = whole_solves(problems, K, args.loop_cap, args.iteration_limit)
            rates = [many]
            for _ in range(args.solve_reps - 1):
                again = whole_solves(problems, K, args.loop_cap, args.iteration_limit, with_loop=False)
                rates.append(again[0])
                if again[0] >= max(rates):
                    share = again[1]
            many = max(rates)
            emit(f"{shape:<15} {K:>5} {many:>13.2f} {loop:>13.2f} {many / loop:>7.2f} {share:>15.2f} {n_loop:>9}"
                 + (f"   # all runs: {' '.join('%.2f' % r for r in rates)}" if len(rates) > 1 else "")
                 + (f"   # check_info: {info}" if info else "")
                 + (f"   # {differ} solves differ from optimize's" if differ else ""))
        if args.check_kernels:
            K = min(args.profile_k, max(solve_ks))
            got = check_kernels_us(shape, K, args.iteration_limit, args.qp)
            if isinstance(got, str):
                emit(f"# {shape}: check kernels at K = {K}: not measured ({got})")
            else:
                emit(f"# {shape}: kernels of one optimize_many at K = {K} (rocprofv3 --kernel-trace --stats, a run of its own), calls x average us: "
                     + "; ".join(f"{n} {c} x {us:.1f}" for n, (c, us) in sorted(got.items())))
        del problems
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
