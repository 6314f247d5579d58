#!/usr/bin/env python3
"""Alternate `bench.py` between builds of the library inside one GPU job.

  step_hot_ab.py --variant parent=/path/libquadswarm.so --variant this= \\
                 --variant general=,QS_HOT_SHAPE=0 --rounds 5 --out FILE [-- bench args]

A variant is `name=library[,VAR=value...]`: an empty library is this tree's own; the
settings go into the child's environment.  Each round runs every variant once, in the
order given, each in a fresh child process under its own time limit; a child that
fails, times out or prints no result line ends the whole run at once (nothing more is
started on the GPU).  With `--dump DIR` every variant then runs once more with
`--dump-outputs DIR/<name>` and the arrays are compared with the first variant's.

Gain rule: of the variant `--this` against the variant `--base`, the
slowest run of the first over the fastest run of the second must exceed one plus three
times the larger of the two spreads ((max − min) / min of `value`).
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(lib, env_extra, bench_args, limit):
    env = dict(os.environ)
    env.pop("QS_DEV_LIB", None)
    if lib:
        env["QS_DEV_LIB"] = os.path.abspath(lib)
    env.update(env_extra)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + bench_args
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=limit)
    if p.returncode != 0:
        sys.exit(f"step_hot_ab: bench.py ended with {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
    for line in reversed(p.stdout.splitlines()):
        if line.startswith("{"):
            return json.loads(line)
    sys.exit("step_hot_ab: no result line\n" + p.stdout[-2000:])


def main():
    argv = sys.argv[1:]
    bench_args = []
    if "--" in argv:
        k = argv.index("--")
        argv, bench_args = argv[:k], argv[k + 1:]
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--variant", action="append", required=True)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--base", default=None, help="variant the gain rule compares against (default: the first)")
    ap.add_argument("--this", default=None, help="variant the gain rule is about (default: the second)")
    ap.add_argument("--dump", default=None)
    ap.add_argument("--limit", type=float, default=240.0, help="seconds per child")
    ap.add_argument("--out", required=True)
    args = ap.parse_args(argv)
    variants = []
    for v in args.variant:
        name, _, rest = v.partition("=")
        parts = rest.split(",")
        variants.append((name, parts[0], dict(s.split("=", 1) for s in parts[1:] if s)))
    runs = {name: [] for name, _, _ in variants}
    doc = {"what": "bench.py --gpus 1 " + " ".join(bench_args) + ": the variants alternated --rounds times in one GPU "
                   "job, a fresh process each. value: agent-steps/s; event_ms_per_step: timing.event_ms_per_step.",
           "variants": {name: {"library": "this tree" if not lib else os.path.basename(os.path.dirname(lib)) or lib,
                               "env": env} for name, lib, env in variants},
           "rounds": args.rounds, "runs": runs}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")

    for r in range(args.rounds):
        for name, lib, env in variants:
            res = run_bench(lib, env, bench_args, args.limit)
            t = res.get("timing", {})
            runs[name].append({"value": res["value"], "event_ms_per_step": t.get("event_ms_per_step"),
                               "wall_ms_per_step": t.get("wall_ms_per_step")})
            print(f"round {r} {name}: {res['value'] / 1e9:.3f}e9 agent-steps/s, "
                  f"{1e3 * (t.get('event_ms_per_step') or 0):.4f} us/step", flush=True)
            save()
    spread = {n: (max(x["value"] for x in v) - min(x["value"] for x in v)) / min(x["value"] for x in v)
              for n, v in runs.items()}
    doc["spread"] = spread
    doc["mean_event_us_per_step"] = {n: 1e3 * sum(x["event_ms_per_step"] or 0 for x in v) / len(v) for n, v in runs.items()}
    base = args.base or variants[0][0]
    pairs = [(n, base) for n, _, _ in variants if n != base and (args.this is None or n == args.this)]
    doc["gain_rule"] = {}
    for this, b in pairs:
        ratio = min(x["value"] for x in runs[this]) / max(x["value"] for x in runs[b])
        need = 1 + 3 * max(spread[this], spread[b])
        doc["gain_rule"][f"{this}_over_{b}"] = {"slowest_over_fastest": ratio, "threshold": need,
                                                "counts_as_gain": bool(ratio > need)}
    save()
    if args.dump:
        import numpy as np
        same = {}
        for name, lib, env in variants:
            d = os.path.join(args.dump, name)
            os.makedirs(d, exist_ok=True)
            run_bench(lib, env, bench_args + ["--steps", "40", "--warmup", "5", "--dump-outputs", d], args.limit)
        first = os.path.join(args.dump, variants[0][0])
        for name, _, _ in variants[1:]:
            same[name] = {f: bool(np.array_equal(np.load(os.path.join(first, f)), np.load(os.path.join(args.dump, name, f))))
                          for f in sorted(os.listdir(first)) if f.endswith(".npy")}
        doc["dump_outputs_equal_to_" + variants[0][0]] = same
        save()
    print(json.dumps({k: doc[k] for k in doc if k != "runs"}, indent=1))


if __name__ == "__main__":
    main()
