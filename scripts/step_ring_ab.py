#!/usr/bin/env python3
"""Ring launches (csrc/step_mh_ring.hip): what a launch boundary costs, and the A/B.

  step_ring_ab.py --parent /path/libquadswarm.so --rounds 5 --out-dir DIR [--dump DIR] [-- bench args]

Two measurements in one GPU job, both on plain `bench.py --gpus 1` (scripts/step_hot_ab.py
runs the children: a fresh process each under its own time limit, the whole run ending at
the first child that fails):

 1. `DIR/step_ring_depths.json`: the parent library under QS_MAX_FUSED_STEPS = 32, 24, 16, 8,
    alternated --rounds times; the mean event time per step fitted as a + b / K (least
    squares).  b is what one launch boundary costs; a window of `--steps` steps (484) over a
    32-slot ring pays it 16 times and needs it once, so the predicted gain of keeping the
    window in one launch is 15 · b over the window's time at depth 32.
 2. `DIR/step_ring_ab.json`: the parent library, this tree and this tree under
    QS_RING_LAUNCH=0 alternated --rounds times, judged by the gain rule of DESIGN.md §4
    (step_hot_ab.py), then with `--dump` the `--dump-outputs` arrays of each compared.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import step_hot_ab  # noqa: E402

DEPTHS = (32, 24, 16, 8)


def fit_depths(parent, rounds, bench_args, limit, out, window):
    runs = {k: [] for k in DEPTHS}
    for r in range(rounds):
        for k in DEPTHS:
            res = step_hot_ab.run_bench(parent, {"QS_MAX_FUSED_STEPS": str(k)}, bench_args, limit)
            us = 1e3 * res["timing"]["event_ms_per_step"]
            runs[k].append(us)
            print(f"round {r} depth {k}: {us:.4f} us/step", flush=True)
    mean = {k: sum(v) / len(v) for k, v in runs.items()}
    # least squares of y = a + b x over x = 1 / K
    xs, ys = [1.0 / k for k in DEPTHS], [mean[k] for k in DEPTHS]
    n = len(xs)
    mx, my = sum(xs) / n, sum(ys) / n
    b = sum((x - mx) * (y - my) for x, y in zip(xs, ys)) / sum((x - mx) ** 2 for x in xs)
    a = my - b * mx
    boundaries = -(-window // 32) - 1
    doc = {"what": "bench.py --gpus 1 " + " ".join(bench_args) + " on the parent library under QS_MAX_FUSED_STEPS = K, the "
                   "depths alternated --rounds times in one GPU job; event µs per step, fitted as a + b / K",
           "rounds": rounds, "us_per_step": {str(k): v for k, v in runs.items()}, "mean_us_per_step": {str(k): mean[k] for k in DEPTHS},
           "fit": {"a_us": a, "b_us": b, "residual_us": {str(k): mean[k] - (a + b / k) for k in DEPTHS}},
           "window_steps": window, "boundaries_saved": boundaries,
           "predicted_gain": boundaries * b / (window * mean[32])}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(json.dumps(doc, indent=1) + "\n")
    print(json.dumps({k: doc[k] for k in ("mean_us_per_step", "fit", "predicted_gain")}, indent=1), flush=True)


def main():
    argv = sys.argv[1:]
    bench_args = []
    if "--" in argv:
        k = argv.index("--")
        argv, bench_args = argv[:k], argv[k + 1:]
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent", required=True, help="the parent commit's libquadswarm.so")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out-dir", required=True)
    ap.add_argument("--dump", default=None)
    ap.add_argument("--limit", type=float, default=240.0, help="seconds per child")
    ap.add_argument("--window", type=int, default=484, help="the bench's timed steps (its --steps default)")
    ap.add_argument("--skip-fit", action="store_true")
    args = ap.parse_args(argv)
    if not args.skip_fit:
        fit_depths(args.parent, args.rounds, bench_args, args.limit, os.path.join(args.out_dir, "step_ring_depths.json"),
                   args.window)
    sys.argv = [sys.argv[0], "--variant", f"parent={args.parent}", "--variant", "this=", "--variant", "ring_off=,QS_RING_LAUNCH=0",
                "--rounds", str(args.rounds), "--limit", str(args.limit), "--out", os.path.join(args.out_dir, "step_ring_ab.json")]
    if args.dump:
        sys.argv += ["--dump", args.dump]
    sys.argv += ["--"] + bench_args
    step_hot_ab.main()


if __name__ == "__main__":
    main()
