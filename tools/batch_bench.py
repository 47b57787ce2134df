"""Throughput of batched PDHG (pdhg_batch_take_steps_adaptive) against the single-LP engine.

For every configuration and every K: member-iterations/s of the batch (accepted take_steps summed over the members,
divided by the wall time of the timed call), the solo engine's iterations/s on member 0, their ratio, and ms per
batched trial (a separate loop of pdhg_batch_trial_step).  Every timed call returns after the device has drained.  Row order: whatever PDHG_ROW_ORDER says (the shipped
default is relaxed).

    python tools/batch_bench.py [--configs pagerank,l1svm,random] [--ks 1,2,4,8,16] [--steps 300] [--warmup 50]
                                [--qp] [--qp-shape 10000000x10000000] [--against OTHER_CHECKOUT] [--reps 3]
                                [--out profiles/batch_throughput.txt]

Configurations: "pagerank" = personalized PageRank on the 1M-node PageRank LP (BASELINE configs[2]), one Dirichlet
teleport vector per member; "l1svm" = L1-SVM regularization path on the rcv1-like data (configs[3]), weights 0.25 ..
4; "random" = the 10M x 10M, 100M-nnz random LP (configs[4]) with per-member c and b.

--qp adds the QP leg (rows "random+Q"): ``generators.random_qp_family`` at --qp-shape (default: the random config's
shape), QPs that share Q = B'B + diag as well as A, against the solo QP engine on member 0 in the same run.

--against OTHER_CHECKOUT (a built checkout of another commit, e.g. the parent) runs the LP legs --reps times with that
checkout's own tools/batch_bench.py and with this one's, alternating, each in a fresh process, and prints per config and
K the median member-it/s of both and the spread (worst - best) / best of each side's repetitions.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def members(config, K, seed=0):
    from firstorderlp_jl_amd.generators import (l1_svm_regularization_path, personalized_pagerank_lps,
                                                preprocess_training_data, random_lp, synthetic_rcv1_like)
    from firstorderlp_jl_amd.quadratic_programming import linear_programming_problem
    rng = np.random.default_rng(seed)
    if config == "pagerank":
        n = 1_000_000
        tele = [np.full(n, 1.0 / n)] + [rng.dirichlet(np.full(n, 0.5)) for _ in range(K - 1)]
        return personalized_pagerank_lps(n, tele, 4 * n, 0.99, seed=0)
    if config == "l1svm":
        X, y = synthetic_rcv1_like(seed=0)
        return l1_svm_regularization_path(preprocess_training_data(X), y, list(np.geomspace(0.25, 4.0, K)))
    p = random_lp(10_000_000, 10_000_000, 10, 12345)
    out = [p]
    for _ in range(K - 1):
        c = p.objective_vector * (1.0 + 0.2 * rng.random(len(p.objective_vector)))
        b = p.right_hand_side * (1.0 + 0.2 * rng.random(len(p.right_hand_side)))
        out.append(linear_programming_problem(p.variable_lower_bound, p.variable_upper_bound, c, 0.0,
                                              p.constraint_matrix, b, p.num_equalities))
    return out


def qp_members(shape, K):
    from firstorderlp_jl_amd.generators import random_qp_family
    m, n = (int(v) for v in shape.lower().split("x"))
    return random_qp_family(m, n, K, 12345)


def solo_rate(p, steps, warmup):
    import folp_loader
    pkg = folp_loader.load()
    eng = pkg.HipPdhgEngine.from_problem(p, device_id=0)
    try:
        s, it, kkt = 1.0 / eng.matrix_max_abs(), 0, 0.0
        s, it, kkt, _, _ = eng.take_steps_adaptive(warmup, 0.3, 0.6, s, 1.0, it, kkt)
        t0 = time.perf_counter()
        s, it, kkt, err, done = eng.take_steps_adaptive(steps, 0.3, 0.6, s, 1.0, it, kkt)
        return done / (time.perf_counter() - t0)
    finally:
        eng.close()


def batch_rates(problems, steps, warmup, trials=20):
    import folp_loader
    pkg = folp_loader.load()
    K = len(problems)
    batch = pkg.HipPdhgBatch.from_problems(problems, device_id=0)
    try:
        ss = np.full(K, 1.0 / batch.members[0].matrix_max_abs())
        pw, it, kkt = np.ones(K), np.zeros(K, dtype=np.int64), np.zeros(K)
        ss, it, kkt, _, _ = batch.take_steps_adaptive(warmup, 0.3, 0.6, ss, pw, it, kkt)
        it0 = it.copy()
        t0 = time.perf_counter()
        ss, it, kkt, err, done = batch.take_steps_adaptive(steps, 0.3, 0.6, ss, pw, it, kkt)
        elapsed = time.perf_counter() - t0
        rate = float(done.sum()) / elapsed
        member_trials = int((it - it0).sum())
        t1 = time.perf_counter()
        for _ in range(trials):
            batch.trial_step(ss, pw)
        ms_trial = 1e3 * (time.perf_counter() - t1) / trials
        return rate, ms_trial, member_trials / float(done.sum())
    finally:
        batch.close()


def _table_rows(path):
    """{(config, K): member-it/s} of a table this tool wrote."""
    out = {}
    with open(path) as fh:
        for line in fh:
            t = line.split()
            if len(t) == 7 and t[1].isdigit():
                out[(t[0], int(t[1]))] = float(t[2])
    return out


def against(args):
    """The LP legs with another checkout's tool and library and with this one's, alternating, a fresh process each."""
    import subprocess
    import tempfile
    sides = (("other", os.path.abspath(args.against)), ("this", ROOT))
    runs = {name: [] for name, _ in sides}
    for r in range(args.reps):
        for name, root in sides:
            with tempfile.NamedTemporaryFile(suffix=".txt") as tmp:
                subprocess.check_call([sys.executable, os.path.join(root, "tools", "batch_bench.py"), "--configs", args.configs,
                                       "--ks", args.ks, "--steps", str(args.steps), "--warmup", str(args.warmup),
                                       "--out", tmp.name], cwd=root, stdout=subprocess.DEVNULL)
                runs[name].append(_table_rows(tmp.name))
            print(f"# repetition {r + 1} of {args.reps}, {name}: done", flush=True)
    lines = [f"# tools/batch_bench.py --against {args.against} --configs {args.configs} --ks {args.ks} --steps {args.steps} "
             f"--warmup {args.warmup} --reps {args.reps}  (PDHG_ROW_ORDER={os.environ.get('PDHG_ROW_ORDER', 'relaxed')})",
             "# member-it/s: median of the repetitions; spread = (worst - best) / best of one side's repetitions",
             f"{'config':<10} {'K':>3} {'other':>12} {'spread':>7} {'this':>12} {'spread':>7} {'this/other':>10}"]
    for key in sorted(runs["this"][0], key=lambda k: (args.configs.split(",").index(k[0]), k[1])):
        col = {}
        for name, _ in sides:
            v = sorted(run[key] for run in runs[name])
            col[name] = (float(np.median(v)), (v[-1] - v[0]) / v[-1])
        lines.append(f"{key[0]:<10} {key[1]:>3} {col['other'][0]:>12.1f} {col['other'][1]:>7.3f} {col['this'][0]:>12.1f} "
                     f"{col['this'][1]:>7.3f} {col['this'][0] / col['other'][0]:>10.3f}")
    print("\n".join(lines), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="pagerank,l1svm,random")
    ap.add_argument("--ks", default="1,2,4,8,16")
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--out", default=None)
    ap.add_argument("--qp", action="store_true", help="the QP leg as well (rows random+Q)")
    ap.add_argument("--qp-shape", default="10000000x10000000", help="m x n of the QP leg's family")
    ap.add_argument("--against", default=None, help="another built checkout: its LP legs and this one's, alternating")
    ap.add_argument("--reps", type=int, default=3, help="repetitions per side of --against")
    args = ap.parse_args(argv)
    if args.against:
        return against(args)
    import folp_loader
    folp_loader.load()
    ks = [int(k) for k in args.ks.split(",")]
    lines = [f"# tools/batch_bench.py --configs {args.configs} --ks {args.ks} --steps {args.steps} --warmup {args.warmup}"
             f"  (PDHG_ROW_ORDER={os.environ.get('PDHG_ROW_ORDER', 'relaxed')})",
             f"{'config':<10} {'K':>3} {'member-it/s':>12} {'solo it/s':>10} {'ratio':>7} {'ms/batched trial':>17} "
             f"{'trials/step':>11}"]
    print("\n".join(lines), flush=True)
    legs = [c for c in args.configs.split(",") if c] + (["random+Q"] if args.qp else [])
    if args.qp:
        lines.insert(1, f"# random+Q: random_qp_family at {args.qp_shape}; solo it/s = the solo QP engine on member 0")
    for config in legs:
        probs = qp_members(args.qp_shape, max(ks)) if config == "random+Q" else members(config, max(ks))
        solo = solo_rate(probs[0], args.steps, args.warmup)
        for K in ks:
            rate, ms_trial, tps = batch_rates(probs[:K], args.steps, args.warmup)
            line = f"{config:<10} {K:>3} {rate:>12.1f} {solo:>10.1f} {rate / solo:>7.2f} {ms_trial:>17.3f} {tps:>11.2f}"
            print(line, flush=True)
            lines.append(line)
        del probs
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
