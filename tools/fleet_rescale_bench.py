"""What one shared rescale launch saves a fleet (pdhg_fleet_rescale, HipPdhgFleet.rescale) against the member loop of
eng.rescale + eng.matrix_max_abs, the route of every fleet before it and the yardstick here.

    python tools/fleet_rescale_bench.py [--shapes netlib27x32,netlib56x97,random1000x800] [--ks 1,8,64,256] [--reps 5]
                                        [--solve-ks 64,256] [--solve-reps 3] [--iteration-limit 5000]
                                        [--out profiles/fleet_rescale_throughput.txt]

Members: tools/fleet_bench.py's (`random_lp` of the shape, a distinct seed per member).  Rescaling: solve_qp's defaults,
10 Ruiz steps and Pock-Chambolle with alpha = 1 (11 steps).

Calls: one fleet of max(ks) members per shape; at every K the member loop over the first K members and one
`fleet.rescale(members=first K)` are timed in turn, `reps` times each after a warm-up of each; wall ms per call, the
best and the spread (a call returns with the stream idle, so the wall time includes the device).  The matrix is rescaled
again and again: every step does the same work whatever the values.  `rescale_info()` must report every member carried.

Whole solves: `optimize_many` on K members and a `PdhgFleetSession` tick -- new matrix values for every member, then a
warm solve -- with PDHG_FLEET_RESCALE unset and set to 1 in turn, `solve-reps` times each; seconds, best and spread.

Kernel: fleet_rescale_kernel's duration at --profile-k members from a `rocprofv3 --kernel-trace --stats` run of a child
process of its own (no counters).
"""
import argparse
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from fleet_bench import SHAPES, members, solve_params  # noqa: E402

RESCALING = (10, False, 1.0)
SWITCH = "PDHG_FLEET_RESCALE"


def _spread(times):
    return f"{1e3 * min(times):>9.3f} ({1e3 * min(times):.3f} - {1e3 * max(times):.3f})"


def call_times(fleet, K, reps):
    """([member-loop seconds], [shared-call seconds]) over the first K members, alternating."""
    named = list(range(K))

    def loop():
        for eng in fleet.members[:K]:
            eng.rescale(*RESCALING)
            eng.matrix_max_abs()

    def shared():
        fleet.rescale(*RESCALING, members=named)
    loop()
    shared()
    info = fleet.rescale_info()
    if info["carried"] != K or info["single"]:
        raise RuntimeError(f"the shared launch carried {info['carried']} of {K} members")
    out = ([], [])
    for _ in range(reps):
        for which, call in enumerate((loop, shared)):
            t0 = time.perf_counter()
            call()
            out[which].append(time.perf_counter() - t0)
    return out


def child_launch(shape, K):
    """What the profiled child runs: a fleet of K members and four shared rescale calls."""
    import folp_loader
    pkg = folp_loader.load()
    fleet = pkg.HipPdhgFleet.from_problems(members(shape, K), device_id=0)
    try:
        for _ in range(4):
            fleet.rescale(*RESCALING)
    finally:
        fleet.close()


def kernel_us(shape, K, timeout=300):
    """(calls, average us) of fleet_rescale_kernel in a `rocprofv3 --kernel-trace --stats` run of a child of its own, or
    a string saying why there is none."""
    from rocprof_summary import summarize
    rp = shutil.which("rocprofv3")
    if not rp:
        return "rocprofv3 not on PATH"
    work = tempfile.mkdtemp(prefix="pdhg_fleet_rescale_prof_", dir="/tmp")
    try:
        cmd = [rp, "--kernel-trace", "--stats", "-d", work, "--", sys.executable, os.path.abspath(__file__), "--child", shape, str(K)]
        r = subprocess.run(cmd, cwd="/tmp", env=dict(os.environ, TMPDIR="/tmp"), timeout=timeout, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
        if r.returncode != 0:
            return f"profiled child failed ({r.returncode}): {r.stderr.decode(errors='replace')[-200:]}"
        rows = [k for k in summarize(work) if "fleet_rescale_kernel" in k["name"]]
        if not rows:
            return "no fleet_rescale_kernel in the trace"
        return rows[0].get("calls"), rows[0]["avg_us"]
    except subprocess.TimeoutExpired:
        return f"profiled child timed out after {timeout} s"
    finally:
        shutil.rmtree(work, ignore_errors=True)


def _switched(value, run):
    old = os.environ.pop(SWITCH, None)
    if value:
        os.environ[SWITCH] = value
    try:
        t0 = time.perf_counter()
        out = run()
        return time.perf_counter() - t0, out
    finally:
        os.environ.pop(SWITCH, None)
        if old is not None:
            os.environ[SWITCH] = old


def solve_times(problems, params, reps):
    """{"many" | "tick": ([seconds switch off], [seconds switch on])}; the outputs of the two routes must agree."""
    from firstorderlp_jl_amd import PdhgFleetSession, optimize_many
    rng = np.random.default_rng(0)
    updates = [{"constraint_matrix_values": p.constraint_matrix.data * (1.0 + 0.01 * rng.standard_normal(p.constraint_matrix.nnz))}
               for p in problems]
    out = {"many": ([], []), "tick": ([], [])}
    seen = {}

    def same(kind, outputs):
        key = [(o.iteration_count, o.primal_solution.tobytes()) for o in outputs]
        if seen.setdefault(kind, key) != key:
            raise RuntimeError(f"{kind}: the outputs differ between the two routes")
    for _ in range(reps):
        for which, value in enumerate((None, "1")):
            dt, outputs = _switched(value, lambda: optimize_many(params, problems))
            same("many", outputs)
            out["many"][which].append(dt)
            # the session is created (and solved once) outside the timed tick; the switch is read at every call
            old = os.environ.pop(SWITCH, None)
            if value:
                os.environ[SWITCH] = value
            try:
                with PdhgFleetSession(params, problems) as session:
                    session.solve()
                    t0 = time.perf_counter()
                    session.update(updates)
                    outputs = session.solve(warm_start=True)
                    out["tick"][which].append(time.perf_counter() - t0)
                same("tick", outputs)
            finally:
                os.environ.pop(SWITCH, None)
                if old is not None:
                    os.environ[SWITCH] = old
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--ks", default="1,8,64,256")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--solve-ks", default="64,256")
    ap.add_argument("--solve-reps", type=int, default=3)
    ap.add_argument("--iteration-limit", type=int, default=5000)
    ap.add_argument("--profile-k", type=int, default=256)
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", nargs=2, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args(argv)
    import folp_loader
    pkg = folp_loader.load()
    if args.child:
        child_launch(args.child[0], int(args.child[1]))
        return
    ks = [int(k) for k in args.ks.split(",") if k]
    solve_ks = [int(k) for k in args.solve_ks.split(",") if k]
    lines = []

    def emit(line):
        print(line, flush=True)
        lines.append(line)

    emit(f"# tools/fleet_rescale_bench.py --shapes {args.shapes} --ks {args.ks} --reps {args.reps} --solve-ks {args.solve_ks} "
         f"--solve-reps {args.solve_reps} --iteration-limit {args.iteration_limit}")
    emit(f"# calls: rescale{RESCALING} + matrix_max_abs of K members; wall ms per call, best of {args.reps} (best - worst), the two routes in turn")
    emit(f"{'shape':<15} {'K':>5} {'member loop ms':>32} {'one fleet.rescale ms':>32} {'loop / shared':>13}")
    shapes = args.shapes.split(",")
    for shape in shapes if ks else []:
        problems = members(shape, max(ks))
        fleet = pkg.HipPdhgFleet.from_problems(problems, device_id=0)
        try:
            for K in ks:
                loop, shared = call_times(fleet, K, args.reps)
                emit(f"{shape:<15} {K:>5} {_spread(loop):>32} {_spread(shared):>32} {min(loop) / min(shared):>13.2f}")
        finally:
            fleet.close()
        if not args.no_profile:
            K = min(args.profile_k, max(ks))
            got = kernel_us(shape, K)
            if isinstance(got, str):
                emit(f"# {shape}: fleet_rescale_kernel at K = {K}: not measured ({got})")
            else:
                emit(f"# {shape}: fleet_rescale_kernel at K = {K} (rocprofv3 --kernel-trace --stats, a run of its own): {got[0]} calls, "
                     f"{got[1]:.1f} us on average")
    if solve_ks:
        emit(f"# whole solves: solve_qp defaults, tolerance 1e-6, iteration limit {args.iteration_limit}; {SWITCH} unset and 1 in turn, "
             f"seconds, best of {args.solve_reps} (best - worst); tick: new matrix values for every member, then a warm solve")
        emit(f"{'shape':<15} {'K':>5} {'what':>14} {'switch off s':>28} {'switch on s':>28} {'off / on':>9}")
    for shape in shapes if solve_ks else []:
        problems = members(shape, max(solve_ks))
        for K in solve_ks:
            got = solve_times(problems[:K], solve_params(args.iteration_limit), args.solve_reps)
            for kind, name in (("many", "optimize_many"), ("tick", "session tick")):
                off, on = got[kind]
                emit(f"{shape:<15} {K:>5} {name:>14} {min(off):>12.3f} ({min(off):.3f} - {max(off):.3f}) "
                     f"{min(on):>12.3f} ({min(on):.3f} - {max(on):.3f}) {min(off) / min(on):>9.2f}")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
