#!/usr/bin/env python3
"""Time per MPPI and CEM tick with a sampling spec against the plain ticks of the parent commit.

MultiHover, one_d_pid, 8 drones, fp32, horizon n = --steps, at three shapes (E envs x C
candidates): 1 x 4096, 64 x 256, 4096 x 4; CEM with C / 8 elites (at least 2) and 3 iterations.

  parent   the plain ticks, `MPPIPlanner.plan()` and `CEMPlanner.plan()`, and `MPPIPlanner.sample()`
           alone, on the library given by --parent-lib (a build of the parent commit).
  this     the same on this tree's library after `set_sampling(rho=0.9)` (CEM: also
           keep = elites / 2): the serial-in-j sample kernel in the place of the (sample, n)
           launch, and for CEM the elite memory inside the refit, sample and finish launches.

The yardstick is the parent's plain tick: the feature should cost about nothing.

  sampling_ab.py --parent-lib /path/libquadswarm.so --rounds 5 --out FILE [-- bench.py arguments]

Each round runs the two ways once, `parent` first, each in a fresh child process (this script
with --child) under its own time limit; a child that fails, times out or prints no result ends
the whole run at once (nothing more is started on the GPU).  A child warms every case up, then
times one window of --ticks ticks per case with device events round synchronised work; nothing
inside a window reads back to the host.  After the ticks the plain `bench.py --gpus 1` (which
runs none of this code) is alternated between the two libraries the same number of times
(scripts/step_hot_ab.py's run_bench; the arguments after `--` go to it).  Last, one child runs the
closed loop on this tree (reported, not gated): 64 envs, C = 64, 200 ticks from one seed, the
16-step MPPI tick at rho 0, 0.5 and 0.9, the 16-step CEM tick with and without elite memory, and
the 64-step particle tick at rho 0 and 0.9; --closed-only runs just that and merges it into the
document --out already holds.  Rule: a difference counts where the slowest of one
side against the fastest of the other exceeds one plus three times the larger spread.

Writes one JSON document (--out) and prints it.  Needs a GPU: there is no fallback.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"E1_C4096": (1, 4096), "E64_C256": (64, 256), "E4096_C4": (4096, 4)}
SIGMA, SIGMA_MIN, LO, HI, LAM, PENALTY, RHO, ITERS = 0.3, 0.01, -1.0, 1.0, 1.0, 10.0, 0.9, 3


def elites_of(C):
    return max(2, C // 8)


def make_env(E, seed=0):
    sys.path.insert(0, os.path.join(ROOT, "marl-gym-pybullet-drones_amd"))
    from gym_pybullet_drones_amd.envs.swarm import grid_layout
    from gym_pybullet_drones_amd.vec_env.vec_env import SwarmVecEnv
    env = SwarmVecEnv(task="multihover", num_envs=E, num_drones=8, act="one_d_pid", initial_xyzs=grid_layout(8), seed=seed)
    env.reset_t()
    for _ in range(3):
        env.step_t(None)
    return env


def child(way, n, ticks, shapes):
    import torch
    if not torch.cuda.is_available():
        sys.exit("sampling_ab: no GPU (this script measures; it has no fallback)")

    def window(fn):
        for _ in range(10):
            fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(ticks):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3 / ticks   # µs

    out = {}
    for name in shapes:
        E, C = SHAPES[name]
        K = elites_of(C)
        env = make_env(E)
        mppi = env.mppi(n, C, SIGMA, lo=LO, hi=HI, lam=LAM, done_penalty=PENALTY, seed=1)
        cem = env.cem(n, C, K, SIGMA, iterations=ITERS, lo=LO, hi=HI, sigma_min=SIGMA_MIN, done_penalty=PENALTY, seed=1)
        if way == "this":
            mppi.set_sampling(RHO)
            cem.set_sampling(RHO, K // 2)
        out[f"{name}/mppi"] = window(mppi.plan)
        out[f"{name}/cem"] = window(cem.plan)
        out[f"{name}/mppi_sample"] = window(mppi.sample)
        env.close()
    print(json.dumps({"way": way, "device": torch.cuda.get_device_name(0), "us_per_tick": out}))


def child_closed(ticks=200, E=64, C=64):
    import torch
    lam = 0.5
    kw = dict(lo=LO, hi=HI, done_penalty=PENALTY, seed=1)
    cases = [("mppi_n16_rho0", "mppi", 0.0, 0), ("mppi_n16_rho0.5", "mppi", 0.5, 0), ("mppi_n16_rho0.9", "mppi", 0.9, 0),
             ("cem_n16", "cem", 0.0, 0), ("cem_n16_keep4", "cem", 0.0, 4), ("cem_n16_rho0.9", "cem", 0.9, 0),
             ("cem_n16_rho0.9_keep4", "cem", 0.9, 4), ("smc_n64_rho0", "smc", 0.0, 0), ("smc_n64_rho0.9", "smc", 0.9, 0)]
    out = {}
    for name, kind, rho, keep in cases:
        env = make_env(E, seed=5)
        if kind == "mppi":
            planner = env.mppi(16, C, SIGMA, lam=lam, **kw)
        elif kind == "cem":
            planner = env.cem(16, C, 8, SIGMA, iterations=ITERS, sigma_min=SIGMA_MIN, **kw)
        else:
            planner = env.smc(64, C, SIGMA, segment=16, lam=lam, ess_frac=0.5, **kw)
        if rho != 0.0 or keep != 0:
            planner.set_sampling(rho, keep)
        total = torch.zeros((), dtype=torch.float64, device=env.swarm.device)
        for _ in range(ticks):
            total += planner.step_t().reward.to(torch.float64).mean()
        torch.cuda.synchronize()
        out[name] = float(total.item()) / ticks
        env.close()
    print(json.dumps({"way": "closed", "device": torch.cuda.get_device_name(0), "mean_env_reward_per_step": out,
                      "ticks": ticks, "envs": E, "candidates": C, "cem_elites": 8, "cem_iterations": ITERS, "sigma": SIGMA,
                      "lambda": lam, "done_penalty": PENALTY, "smc_segment": 16, "smc_ess_frac": 0.5, "seeds": 1}))


def run_child(way, lib, args):
    env = dict(os.environ)
    env.pop("QS_DEV_LIB", None)
    if lib:
        env["QS_DEV_LIB"] = os.path.abspath(lib)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", way, "--steps", str(args.steps), "--ticks", str(args.ticks),
           "--shapes", args.shapes]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=args.limit)
    if p.returncode != 0:
        sys.exit(f"sampling_ab: the {way} child ended with {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
    for line in reversed(p.stdout.splitlines()):
        if line.startswith("{"):
            return json.loads(line)
    sys.exit("sampling_ab: no result line\n" + p.stdout[-2000:])


def by_the_rule(old, new, smaller_is_better):
    """(ratio, threshold): the slowest new against the fastest old, and one plus three times the larger spread."""
    spread = max((max(x) - min(x)) / min(x) for x in (old, new))
    ratio = min(old) / max(new) if smaller_is_better else min(new) / max(old)
    return ratio, 1 + 3 * spread


def main():
    argv, bench_args = sys.argv[1:], []
    if "--" in argv:
        k = argv.index("--")
        argv, bench_args = argv[:k], argv[k + 1:]
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-lib", default=None, help="libquadswarm.so built from the parent commit")
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--ticks", type=int, default=100, help="ticks per timed window")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--limit", type=float, default=240.0, help="seconds per child")
    ap.add_argument("--out", default=None)
    ap.add_argument("--closed-only", action="store_true",
                    help="run only the closed loop and merge it into the document --out already holds")
    ap.add_argument("--child", default=None, choices=("parent", "this", "closed"), help=argparse.SUPPRESS)
    args = ap.parse_args(argv)
    shapes = args.shapes.split(",")
    if args.child == "closed":
        return child_closed()
    if args.child:
        return child(args.child, args.steps, args.ticks, shapes)

    def save(doc):
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(json.dumps(doc, indent=1) + "\n")

    if args.closed_only:
        doc = json.load(open(args.out)) if args.out and os.path.exists(args.out) else {}
        res = run_child("closed", None, args)
        doc["closed_loop"] = {k: v for k, v in res.items() if k not in ("way", "device")}
        save(doc)
        print(json.dumps(doc["closed_loop"], indent=1))
        return None
    if not args.parent_lib or not os.path.exists(args.parent_lib):
        sys.exit("sampling_ab: --parent-lib must name a library built from the parent commit")
    if args.rounds < 3:
        sys.exit("sampling_ab: at least three rounds")
    cases = [f"{s}/{k}" for s in shapes for k in ("mppi", "cem", "mppi_sample")]
    us = {c: {"parent": [], "this": []} for c in cases}
    doc = {"what": "µs per tick (window time / --ticks), device events round synchronised windows; parent: the plain "
                   "MPPIPlanner.plan(), CEMPlanner.plan() and MPPIPlanner.sample() on the parent commit's library; this: the "
                   "same on this tree after set_sampling(rho = 0.9) (CEM: keep = elites / 2 too); the two alternated --rounds "
                   "times in one job, a fresh process each, after a warm-up of each case",
           "horizon": args.steps, "ticks_per_window": args.ticks, "rounds": args.rounds, "rho": RHO, "sigma": SIGMA,
           "lambda": LAM, "done_penalty": PENALTY, "cem_iterations": ITERS, "cases": {}, "plain_bench": None}
    for r in range(args.rounds):
        for way, lib in (("parent", args.parent_lib), ("this", None)):
            res = run_child(way, lib, args)
            doc["device"] = res["device"]
            for c in cases:
                us[c][way].append(res["us_per_tick"][c])
                E, C = SHAPES[c.split("/")[0]]
                doc["cases"][c] = {"envs": E, "candidates": C, "cem_elites": elites_of(C), "cem_keep": elites_of(C) // 2,
                                   "us_per_tick": us[c]}
            print(f"round {r} {way}: " + ", ".join(f"{k} {v:.1f}" for k, v in res["us_per_tick"].items()) + " us", flush=True)
            save(doc)
    for c in cases:
        old, new = us[c]["parent"], us[c]["this"]
        faster, need = by_the_rule(old, new, smaller_is_better=True)     # fastest parent over slowest this
        slower, _ = by_the_rule(new, old, smaller_is_better=True)        # fastest this over slowest parent
        doc["cases"][c].update(slowest_this_over_fastest_parent=max(new) / min(old), fastest_this_over_slowest_parent=slower,
                               threshold=need, this_is_slower_by_the_rule=bool(slower > need),
                               this_is_faster_by_the_rule=bool(faster > need))
    save(doc)
    import step_hot_ab
    runs = {"parent": [], "this": []}
    for r in range(args.rounds):
        for name, lib in (("parent", args.parent_lib), ("this", None)):
            res = step_hot_ab.run_bench(lib, {}, bench_args, args.limit)
            runs[name].append(res["value"])
            print(f"round {r} bench {name}: {res['value'] / 1e9:.4f}e9 agent-steps/s", flush=True)
            doc["plain_bench"] = {"arguments": bench_args, "unit": "agent-steps/s", "value": runs}
            save(doc)
    ratio, need = by_the_rule(runs["parent"], runs["this"], smaller_is_better=False)
    back, _ = by_the_rule(runs["this"], runs["parent"], smaller_is_better=False)
    doc["plain_bench"].update(slowest_this_over_fastest_parent=ratio, slowest_parent_over_fastest_this=back, threshold=need,
                              changed_by_the_rule=bool(ratio > need or back > need))
    save(doc)
    res = run_child("closed", None, args)
    doc["closed_loop"] = {k: v for k, v in res.items() if k not in ("way", "device")}
    save(doc)
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
