"""What a re-solve on a live handle saves: a series of ticks, each with a new right-hand side, solved three ways.

    python tools/resolve_bench.py [--shapes netlib27x32,netlib56x97,random1000x800] [--ks 64,256] [--single l1svm,pagerank1m]
                                  [--ticks 20] [--reps 5] [--iteration-limit 5000] [--profile-k 256] [--no-profile]
                                  [--out profiles/resolve_throughput.txt]
                                  [--batch pagerank,l1svm,randomqp] [--batch-k 8] [--batch-qp-shape 1000000x1000000]
                                  [--matrix] [--matrix-qp-shape 1000000x1000000]

At every tick the right-hand side of every problem is perturbed by 1 % (a fixed seed per tick and member).  Per tick:

  (a) the existing route: `optimize_many(params, updated)` for a fleet, `optimize(params, updated)` for a single problem --
      create and rescale again.  The baseline; it runs code this tool does not touch.
  (b) session update + cold solve (`PdhgFleetSession` / `PdhgSession`): what create and rescale cost.
  (c) session update + warm solve, from the previous tick's solution.

Fleet members: tools/fleet_bench.py's (`random_lp` of the shape, a distinct seed per member); single problems: the
L1-SVM substitute and the 1M-node PageRank LP of the README.  Parameters: solve_qp's defaults (Ruiz-10 +
Pock-Chambolle, adaptive steps, adaptive-normalized restarts, an evaluation every 40 iterations, tolerance 1e-6).
Reported: wall ms per tick and iterations per solve (mean over ticks and members), best of `reps` series with the
spread (worst / best) of the repetitions; routes (a) and (b) must give the same iteration counts (same bits).  The
session is created once per repetition, outside the timed ticks (its first solve is the warm-up).

Also the kernel durations of the shared update and warm-start launches (fleet_resolve_replay_kernel,
fleet_resolve_point_kernel) at --profile-k members, from a `rocprofv3 --kernel-trace --stats` run of a child process of
its own, with no counters.

--batch adds the batch legs (nothing else changes): families that share the matrix -- tools/batch_bench.py's
personalized PageRank at 1M nodes and its L1-SVM regularization path, and ``generators.random_qp_family`` at
--batch-qp-shape -- at --batch-k members, where (a) is `optimize_batch` on the updated problems and (b), (c) are a
`PdhgBatchSession`.  Their kernels (batch_resolve_replay_kernel, batch_resolve_point_kernel) are timed the same way in a
child whose updates give all four vectors of every member, so that the replay streams the whole record: its bytes per
second are tiles * 8 * S * (n + m) over the kernel's average duration (tiles = ceil(K / 4), S = 11 recorded steps).

--matrix runs the same legs (--shapes, --single, and one QP of ``generators.random_qp_family`` at --matrix-qp-shape) with
another tick: every stored value of A is multiplied by 1 + 0.01 N(0, 1), and those of Q by one factor 1 + 0.01 N(0, 1)
(it stays positive semidefinite), on the same sparsity pattern.  (a) creates and rescales again; (b), (c) are
``session.update(constraint_matrix_values=...)`` -- new values placed into every resident copy, then the rescaling -- and
a cold or warm solve.  Beside each row, timed on one engine of the row's first problem (best of three): the
``update_matrix_values`` call alone, the ``rescale`` call alone, and a create of the same problem; and the durations of
the placement kernels (mu_*_kernel, sj_fill_kernel) from a profiled child of their own.

--matrix with --batch adds the batch legs to that table: ONE matrix tick for the whole family (the members share the
matrix); (a) is `optimize_batch` again on the updated problems, (b) and (c) are ``PdhgBatchSession.update_matrix`` -- the
values placed once, the batch rescaled, the members' vectors replayed in one launch -- and a cold or warm solve.  place /
rescale / create are those of a ``HipPdhgBatch`` of the family, and the profiled child's kernels include the replay
launch (batch_resolve_replay_kernel).
"""
import argparse
import dataclasses
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

KERNELS = ("fleet_resolve_replay_kernel", "fleet_resolve_point_kernel", "resolve_replay_kernel", "resolve_point_kernel",
           "batch_resolve_replay_kernel", "batch_resolve_point_kernel")
BATCH_RESOLVE_TILE = 4          # csrc/batch_resolve_kernels.hpp
MATRIX_KERNELS = (r"\b((?:mu_[a-z]+_kernel|sj_fill_kernel|scale_csr_kernel|scale_long_kernel|scale_tiled_kernel|"
                  r"batch_resolve_replay_kernel|batch_scale_vectors_kernel)(?:<[^>]*>)?)\(")


def single_problem(name):
    from firstorderlp_jl_amd.generators import l1_svm_rcv1_like_lp, pagerank_lp
    if name == "l1svm":
        return l1_svm_rcv1_like_lp()
    if name == "pagerank1m":
        return pagerank_lp(1_000_000, seed=1)
    raise ValueError(f"unknown problem {name}")


def tick_rhs(problem, tick, member):
    rng = np.random.default_rng([tick, member, 1234])
    return problem.right_hand_side * (1.0 + 0.01 * rng.uniform(-1.0, 1.0, problem.num_constraints))


def tick_matrix(problem, tick, member):
    """The --matrix tick as ``update``'s keywords: new values on the same pattern."""
    rng = np.random.default_rng([tick, member, 4321])
    A, Q = problem.constraint_matrix, problem.objective_matrix
    update = {"constraint_matrix_values": A.data * (1.0 + 0.01 * rng.standard_normal(A.nnz))}
    if Q.nnz:
        update["objective_matrix_values"] = Q.data * (1.0 + 0.01 * float(rng.standard_normal()))
    return update


def with_matrix_values(problem, update):
    import scipy.sparse as sp
    changes = {}
    for field in ("constraint_matrix", "objective_matrix"):
        if field + "_values" in update:
            old = getattr(problem, field)
            changes[field] = sp.csc_matrix((update[field + "_values"], old.indices, old.indptr), shape=old.shape)
    return dataclasses.replace(problem, **changes)


def _iterations(outs):
    return float(np.mean([o.iteration_count for o in outs]))


def batch_problems(config, K, qp_shape):
    from batch_bench import members, qp_members
    return qp_members(qp_shape, K) if config == "randomqp" else members(config, K)


def series(problems, params, ticks, route, single, batch=False, matrix=False):
    """One series of `ticks` ticks by `route` ('a', 'b', 'c'): (seconds per tick, iterations per solve).  `matrix`: the
    tick changes the matrix values instead of the right-hand side."""
    from firstorderlp_jl_amd import PdhgBatchSession, PdhgFleetSession, PdhgSession, optimize_batch, optimize_many
    from firstorderlp_jl_amd.primal_dual_hybrid_gradient import optimize
    if batch:
        optimize_many = optimize_batch
    seconds, iterations = [], []
    session = None
    try:
        if route != "a":
            session = PdhgSession(params, problems[0]) if single else (PdhgBatchSession if batch else PdhgFleetSession)(params, problems)
            session.solve()
        for tick in range(ticks):
            if matrix and batch:             # the members share the matrix: one tick for all of them
                updates = [tick_matrix(problems[0], tick, 0)] * len(problems)
                updated = [with_matrix_values(p, u) for p, u in zip(problems, updates)] if route == "a" else None
            elif matrix:
                updates = [tick_matrix(p, tick, k) for k, p in enumerate(problems)]
                updated = [with_matrix_values(p, u) for p, u in zip(problems, updates)] if route == "a" else None
            else:
                updates = [{"right_hand_side": tick_rhs(p, tick, k)} for k, p in enumerate(problems)]
                updated = [dataclasses.replace(p, **u) for p, u in zip(problems, updates)] if route == "a" else None
            t0 = time.perf_counter()
            if route == "a":
                outs = [optimize(params, updated[0])] if single else optimize_many(params, updated)
            elif single:
                session.update(**updates[0])
                outs = [session.solve(warm_start=True if route == "c" else None)]
            else:
                if matrix and batch:
                    session.update_matrix(**updates[0])
                else:
                    session.update(updates)
                outs = session.solve(warm_start=True if route == "c" else None)
            seconds.append(time.perf_counter() - t0)
            iterations.append(_iterations(outs))
    finally:
        if session is not None:
            session.close()
    return float(np.mean(seconds)), float(np.mean(iterations))


def measure(problems, params, ticks, reps, single, batch=False, matrix=False):
    """{route: (best ms per tick, worst / best over the repetitions, iterations per solve)}, the routes alternating."""
    runs = {r: [] for r in "abc"}
    for _ in range(reps):
        for route in "abc":
            runs[route].append(series(problems, params, ticks, route, single, batch, matrix))
    out = {}
    for route, rs in runs.items():
        secs = [s for s, _ in rs]
        out[route] = (1e3 * min(secs), max(secs) / min(secs), rs[0][1])
    return out


def matrix_single_timings(problem, params):
    """(ms of ``update_matrix_values`` alone, of ``rescale`` alone, of a create of the same problem), best of three each,
    on one engine of ``problem`` (a QP's create includes its objective matrix)."""
    from firstorderlp_jl_amd import HipPdhgEngine
    rescaling = (params.l_inf_ruiz_iterations, params.l2_norm_rescaling, params.pock_chambolle_alpha)
    create, place, rescale = [], [], []
    eng = None
    try:
        for _ in range(3):
            if eng is not None:
                eng.close()
            t0 = time.perf_counter()
            eng = HipPdhgEngine.from_problem(problem)
            create.append(time.perf_counter() - t0)
        eng.retain_rescaling()
        eng.rescale(*rescaling)
        for tick in range(3):
            u = tick_matrix(problem, tick, 0)
            p = with_matrix_values(problem, u)
            t0 = time.perf_counter()
            eng.update_matrix_values(u["constraint_matrix_values"], u.get("objective_matrix_values"), p.objective_vector,
                                     p.right_hand_side, p.variable_lower_bound, p.variable_upper_bound)
            t1 = time.perf_counter()
            eng.rescale(*rescaling)
            t2 = time.perf_counter()
            place.append(t1 - t0)
            rescale.append(t2 - t1)
    finally:
        if eng is not None:
            eng.close()
    return 1e3 * min(place), 1e3 * min(rescale), 1e3 * min(create)


def matrix_batch_timings(problems, params):
    """``matrix_single_timings`` for a batch: ms of ``HipPdhgBatch.update_matrix_values`` alone, of the ``rescale`` that
    follows (it ends in the replay launch) and of a create of the same family, best of three each; and, fourth, ms of
    the ``rescale`` of a freshly created batch, which scales the members' vectors step by step (K launches and K
    rebuilds of the bound views per step): what the replay launch stands in for."""
    from firstorderlp_jl_amd import HipPdhgBatch
    rescaling = (params.l_inf_ruiz_iterations, params.l2_norm_rescaling, params.pock_chambolle_alpha)
    vectors = [[getattr(p, k) for p in problems] for k in ("objective_vector", "right_hand_side", "variable_lower_bound",
                                                           "variable_upper_bound")]
    create, place, rescale, fresh = [], [], [], []
    batch = None
    try:
        for _ in range(3):
            if batch is not None:
                batch.close()
            t0 = time.perf_counter()
            batch = HipPdhgBatch.from_problems(problems)
            create.append(time.perf_counter() - t0)
            batch.retain_rescaling()
            t0 = time.perf_counter()
            batch.rescale(*rescaling)
            fresh.append(time.perf_counter() - t0)
        for tick in range(3):
            u = tick_matrix(problems[0], tick, 0)
            t0 = time.perf_counter()
            batch.update_matrix_values(u["constraint_matrix_values"], u.get("objective_matrix_values"), *vectors)
            t1 = time.perf_counter()
            batch.rescale(*rescaling)
            t2 = time.perf_counter()
            place.append(t1 - t0)
            rescale.append(t2 - t1)
    finally:
        if batch is not None:
            batch.close()
    return 1e3 * min(place), 1e3 * min(rescale), 1e3 * min(create), 1e3 * min(fresh)


def matrix_problem(name, qp_shape):
    """A --matrix leg's single problem: --single's, or ``qp`` = one QP of ``random_qp_family`` at ``qp_shape``."""
    if name != "qp":
        return single_problem(name)
    from firstorderlp_jl_amd.generators import random_qp_family
    m, n = (int(v) for v in qp_shape.split("x"))
    return random_qp_family(m, n, 1, seed=1)[0]


def matrix_child(name, K, ticks, qp_shape):
    """What the profiled child of a --matrix leg runs: `ticks` matrix updates and warm solves with a short iteration limit."""
    from fleet_bench import members, solve_params
    from firstorderlp_jl_amd import PdhgBatchSession, PdhgFleetSession, PdhgSession
    if name.startswith("batch:"):
        problems = batch_problems(name[len("batch:"):], K, qp_shape)
        with PdhgBatchSession(solve_params(80), problems) as session:
            session.solve()
            for tick in range(ticks):
                session.update_matrix(**tick_matrix(problems[0], tick, 0))
                session.solve(warm_start=True)
        return
    if K > 1:
        problems = members(name, K)
        with PdhgFleetSession(solve_params(80), problems) as session:
            session.solve()
            for tick in range(ticks):
                session.update([tick_matrix(p, tick, k) for k, p in enumerate(problems)])
                session.solve(warm_start=True)
        return
    problem = matrix_problem(name, qp_shape)
    with PdhgSession(solve_params(80), problem) as session:
        session.solve()
        for tick in range(ticks):
            session.update(**tick_matrix(problem, tick, 0))
            session.solve(warm_start=True)


def child(shape, K, ticks):
    """What the profiled child runs: a fleet session, `ticks` updates and warm solves with a short iteration limit."""
    from fleet_bench import members, solve_params
    from firstorderlp_jl_amd import PdhgFleetSession
    problems = members(shape, K)
    with PdhgFleetSession(solve_params(80), problems) as session:
        session.solve()
        for tick in range(ticks):
            session.update([{"right_hand_side": tick_rhs(p, tick, k)} for k, p in enumerate(problems)])
            session.solve(warm_start=True)


def batch_child(config, K, ticks, qp_shape):
    """What the profiled child of a batch leg runs: a batch session, `ticks` updates of all four vectors of every member
    (b perturbed, the others as they are) and warm solves with a short iteration limit."""
    from fleet_bench import solve_params
    from firstorderlp_jl_amd import PdhgBatchSession
    problems = batch_problems(config, K, qp_shape)
    with PdhgBatchSession(solve_params(80), problems) as session:
        session.solve()
        for tick in range(ticks):
            session.update([{"objective_vector": p.objective_vector, "right_hand_side": tick_rhs(p, tick, k),
                             "variable_lower_bound": p.variable_lower_bound, "variable_upper_bound": p.variable_upper_bound}
                            for k, p in enumerate(problems)])
            session.solve(warm_start=True)


def kernel_us(shape, K, ticks=4, timeout=400, extra=(), flag="--child", pattern=None):
    """{kernel: (calls, average us)} of the re-solve kernels in a `rocprofv3 --kernel-trace --stats` run of a child of its
    own, or a string saying why there is none.  `extra`: more arguments for the child (a batch leg's); `flag`, `pattern`:
    another child and the kernels to pick from its trace (a --matrix leg's)."""
    from rocprof_summary import summarize
    rp = shutil.which("rocprofv3")
    if not rp:
        return "rocprofv3 not on PATH"
    work = tempfile.mkdtemp(prefix="pdhg_resolve_prof_", dir="/tmp")
    try:
        cmd = [rp, "--kernel-trace", "--stats", "-d", work, "--", sys.executable, os.path.abspath(__file__), flag, shape, str(K), str(ticks), *extra]
        r = subprocess.run(cmd, cwd="/tmp", env=dict(os.environ, TMPDIR="/tmp"), timeout=timeout, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
        if r.returncode != 0:
            return f"profiled child failed ({r.returncode}): {r.stderr.decode(errors='replace')[-200:]}"
        out = {}
        for k in summarize(work):
            hit = re.search(pattern or r"\b(" + "|".join(KERNELS) + r")\(", k["name"])
            if hit:
                out[hit.group(1)] = (k.get("calls"), k["avg_us"])
        return out or "no re-solve kernel in the trace"
    except subprocess.TimeoutExpired:
        return f"profiled child timed out after {timeout} s"
    finally:
        shutil.rmtree(work, ignore_errors=True)


def matrix_legs(args, params, ks, emit):
    """The --matrix table: the fleet shapes at every K, --single's problems and one QP."""
    from fleet_bench import members
    emit("# ms per tick: best series of `reps` (mean over its ticks); spread: worst / best series; it: iterations per solve")
    emit("# --matrix: per tick every stored value of A times 1 + 0.01 N(0, 1) (Q times one such factor) on the kept pattern; (a) optimize / "
         "optimize_many on the updated problems, (b) session.update(constraint_matrix_values=...) + cold solve, (c) the same + warm solve")
    emit("# place / rescale / create: ms of update_matrix_values, of rescale and of a create of the row's first problem, each alone (best of 3)")
    emit(f"{'problem':<15} {'K':>5} {'(a) ms':>9} {'spread':>6} {'it':>7} {'(b) ms':>9} {'spread':>6} {'it':>7} {'(c) ms':>9} {'spread':>6} {'it':>7} "
         f"{'a/b':>6} {'a/c':>6} {'place':>8} {'rescale':>8} {'create':>8}")

    def row(name, K, problems, single, batch=False):
        got = measure(problems, params, args.ticks, args.reps, single, batch, matrix=True)
        place, rescale, create, *fresh = matrix_batch_timings(problems, params) if batch else matrix_single_timings(problems[0], params)
        a, b, c = got["a"], got["b"], got["c"]
        ahead = a[0] / b[0] > max(a[1], b[1])
        emit(f"{name:<15} {K:>5} {a[0]:>9.2f} {a[1]:>6.2f} {a[2]:>7.1f} {b[0]:>9.2f} {b[1]:>6.2f} {b[2]:>7.1f} {c[0]:>9.2f} {c[1]:>6.2f} "
             f"{c[2]:>7.1f} {a[0] / b[0]:>6.2f} {a[0] / c[0]:>6.2f} {place:>8.2f} {rescale:>8.2f} {create:>8.2f}"
             + ("" if a[2] == b[2] else "   # (a) and (b) DIFFER in iterations") + ("" if ahead else "   # (b) is NOT ahead of (a) by more than the spread"))
        if fresh:
            emit(f"# {name}: the rescale of a freshly created batch, members scaled step by step: {fresh[0]:.2f} ms (best of 3); "
                 f"the rescale after update_matrix_values above, members replayed in one launch: {rescale:.2f} ms")

    def kernels(name, K, extra):
        if args.no_profile:
            return
        got = kernel_us(name, K, ticks=2, extra=extra, flag="--matrix-child", pattern=MATRIX_KERNELS)
        if isinstance(got, str):
            emit(f"# {name}: placement kernels at K = {K}: not measured ({got})")
        else:
            emit(f"# {name}: placement and scale kernels at K = {K} (rocprofv3 --kernel-trace --stats, a run of its own), calls x average us: "
                 + "; ".join(f"{n} {c} x {us:.1f}" for n, (c, us) in sorted(got.items())))

    for shape in [s for s in args.shapes.split(",") if s]:
        problems = members(shape, max(ks))
        for K in ks:
            row(shape, K, problems[:K], False)
        kernels(shape, min(args.profile_k, max(ks)), (args.matrix_qp_shape or "-",))
    for config in [s for s in args.batch.split(",") if s]:
        problems = batch_problems(config, args.batch_k, args.batch_qp_shape)
        row("batch:" + config, args.batch_k, problems, False, batch=True)
        del problems
        kernels("batch:" + config, args.batch_k, (args.batch_qp_shape,))
    for name in [s for s in args.single.split(",") if s] + (["qp"] if args.matrix_qp_shape else []):
        row(name, 1, [matrix_problem(name, args.matrix_qp_shape)], True)
        kernels(name, 1, (args.matrix_qp_shape or "-",))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="netlib27x32,netlib56x97,random1000x800")
    ap.add_argument("--ks", default="64,256")
    ap.add_argument("--single", default="l1svm,pagerank1m")
    ap.add_argument("--ticks", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iteration-limit", type=int, default=5000)
    ap.add_argument("--profile-k", type=int, default=256)
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch", default="", help="batch legs: any of pagerank,l1svm,randomqp")
    ap.add_argument("--batch-k", type=int, default=8)
    ap.add_argument("--batch-qp-shape", default="1000000x1000000")
    ap.add_argument("--matrix", action="store_true", help="the tick changes the matrix values on the kept pattern")
    ap.add_argument("--matrix-qp-shape", default="1000000x1000000", help="--matrix: the QP leg's shape ('' for none)")
    ap.add_argument("--child", nargs="+", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--matrix-child", nargs="+", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args(argv)
    import folp_loader
    folp_loader.load()
    from fleet_bench import members, solve_params
    if args.matrix_child:
        matrix_child(args.matrix_child[0], int(args.matrix_child[1]), int(args.matrix_child[2]), args.matrix_child[3])
        return
    if args.child and len(args.child) > 3:
        batch_child(args.child[0], int(args.child[1]), int(args.child[2]), args.child[3])
        return
    if args.child:
        child(args.child[0], int(args.child[1]), int(args.child[2]))
        return
    params = solve_params(args.iteration_limit)
    lines = []

    def emit(line):
        print(line, flush=True)
        lines.append(line)

    emit(f"# tools/resolve_bench.py --shapes {args.shapes} --ks {args.ks} --single {args.single} --ticks {args.ticks} --reps {args.reps} "
         f"--iteration-limit {args.iteration_limit}" + (f" --matrix --matrix-qp-shape {args.matrix_qp_shape}" if args.matrix else "")
         + (f" --batch {args.batch} --batch-k {args.batch_k} --batch-qp-shape {args.batch_qp_shape}" if args.batch else ""))
    ks = [int(k) for k in args.ks.split(",") if k]
    if args.matrix:
        matrix_legs(args, params, ks, emit)
        if args.out:
            with open(args.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")
        return
    emit("# per tick: b perturbed by 1 %; (a) optimize / optimize_many on the updated problems (create + rescale again), (b) session "
         "update + cold solve, (c) session update + warm solve from the last solution")
    emit("# ms per tick: best series of `reps` (mean over its ticks); spread: worst / best series; it: iterations per solve")
    emit(f"{'problem':<15} {'K':>5} {'(a) ms':>9} {'spread':>6} {'it':>7} {'(b) ms':>9} {'spread':>6} {'it':>7} {'(c) ms':>9} {'spread':>6} {'it':>7} "
         f"{'a/b':>6} {'a/c':>6}")

    def row(name, K, problems, single, batch=False):
        got = measure(problems, params, args.ticks, args.reps, single, batch)
        a, b, c = got["a"], got["b"], got["c"]
        emit(f"{name:<15} {K:>5} {a[0]:>9.2f} {a[1]:>6.2f} {a[2]:>7.1f} {b[0]:>9.2f} {b[1]:>6.2f} {b[2]:>7.1f} {c[0]:>9.2f} {c[1]:>6.2f} "
             f"{c[2]:>7.1f} {a[0] / b[0]:>6.2f} {a[0] / c[0]:>6.2f}" + ("" if a[2] == b[2] else "   # (a) and (b) DIFFER in iterations"))

    for shape in [s for s in args.shapes.split(",") if s]:
        problems = members(shape, max(ks))
        for K in ks:
            row(shape, K, problems[:K], False)
        if not args.no_profile:
            K = min(args.profile_k, max(ks))
            got = kernel_us(shape, K)
            if isinstance(got, str):
                emit(f"# {shape}: re-solve kernels at K = {K}: not measured ({got})")
            else:
                emit(f"# {shape}: re-solve kernels at K = {K} (rocprofv3 --kernel-trace --stats, a run of its own), calls x average us: "
                     + "; ".join(f"{n} {c} x {us:.1f}" for n, (c, us) in sorted(got.items())))
    for name in [s for s in args.single.split(",") if s]:
        row(name, 1, [single_problem(name)], True)
    for config in [s for s in args.batch.split(",") if s]:
        K = args.batch_k
        problems = batch_problems(config, K, args.batch_qp_shape)
        m, n = problems[0].constraint_matrix.shape
        row("batch:" + config, K, problems, False, True)
        del problems
        if args.no_profile:
            continue
        got = kernel_us(config, K, ticks=2, extra=(args.batch_qp_shape,))
        if isinstance(got, str):
            emit(f"# batch:{config}: re-solve kernels at K = {K}: not measured ({got})")
            continue
        emit(f"# batch:{config}: re-solve kernels at K = {K} (rocprofv3 --kernel-trace --stats, a run of its own), calls x average us: "
             + "; ".join(f"{name} {c} x {us:.1f}" for name, (c, us) in sorted(got.items())))
        if "batch_resolve_replay_kernel" in got:
            steps = 11                                        # solve_params: ten Ruiz passes and Pock-Chambolle
            record = -(-K // BATCH_RESOLVE_TILE) * 8 * steps * (n + m)
            emit(f"# batch:{config}: the replay reads {record / 1e6:.1f} MB of record per launch ({m} x {n}, {steps} steps, "
                 f"{-(-K // BATCH_RESOLVE_TILE)} tiles): {record / got['batch_resolve_replay_kernel'][1] / 1e3:.1f} GB/s of record")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
