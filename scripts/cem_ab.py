#!/usr/bin/env python3
"""Time per CEM planner tick, two ways, alternated between two builds of the library.

MultiHover, one_d_pid, 8 drones, fp32, horizon n = --steps, I = --iterations, K = C / 8
elites (at least 1), at three shapes (E envs x C candidates): 1 x 4096, 64 x 256,
4096 x 4.  A tick is, I times: draw C candidate sequences round the mean with the
per-element spread, clip, score them from the envs' state (one qs_score launch either
way), pick the K best per env, refit mean and spread to them; then shift the mean by a
step and take the first action.

  torch    the tick in torch ops round `SwarmVecEnv.score_t`: randn, mul, add, clamp,
           score_t, topk, gather, mean / std, roll.  Needs nothing newer than qs_score, so
           it runs on the library given by --parent-lib (a build of the parent commit).
  native   `CEMPlanner.plan()` on this tree's library.

  cem_ab.py --parent-lib /path/libquadswarm.so --rounds 5 --out FILE

Each round runs the two ways once, `torch` first, each in a fresh child process (this
script with --child) under its own time limit; a child that fails, times out or prints
no result ends the whole run at once (nothing more is started on the GPU).  A child warms
every shape up, then times one window of --ticks ticks per shape with device events
around synchronised work; nothing inside a window reads back to the host.
Gain rule: the slowest `native` against the fastest `torch` must exceed one
plus three times the larger spread.

`--child trace` runs a few native ticks per shape and nothing else: the run to put under
a kernel trace for the split between sample, score, select and refit.

Writes one JSON document (--out) and prints it.  Needs a GPU: there is no fallback.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"E1_C4096": (1, 4096), "E64_C256": (64, 256), "E4096_C4": (4096, 4)}
SIGMA, SIGMA_MIN, LO, HI, PENALTY = 0.3, 0.01, -1.0, 1.0, 10.0


def child(way, n, iters, ticks, shapes):
    import torch
    sys.path.insert(0, os.path.join(ROOT, "marl-gym-pybullet-drones_amd"))
    from gym_pybullet_drones_amd.envs.swarm import grid_layout
    from gym_pybullet_drones_amd.vec_env.vec_env import SwarmVecEnv
    if not torch.cuda.is_available():
        sys.exit("cem_ab: no GPU (this script measures; it has no fallback)")
    out = {}
    for name in shapes:
        E, C = SHAPES[name]
        K = max(1, C // 8)
        env = SwarmVecEnv(task="multihover", num_envs=E, num_drones=8, act="one_d_pid", initial_xyzs=grid_layout(8), seed=0)
        env.reset_t()
        for _ in range(3):
            env.step_t(None)
        sw = env.swarm
        if way in ("native", "trace"):
            planner = env.cem(n, C, K, SIGMA, iterations=iters, lo=LO, hi=HI, sigma_min=SIGMA_MIN, done_penalty=PENALTY,
                              seed=1)
            tick = planner.plan
        else:
            gen = torch.Generator(device=sw.device).manual_seed(1)
            state = {"mean": torch.zeros((n, E, sw.num_drones, sw.act_dim), device=sw.device)}

            def tick():
                mean = state["mean"]
                std = torch.full_like(mean, SIGMA)
                for _ in range(iters):
                    noise = torch.randn((n, C, E, sw.num_drones, sw.act_dim), device=sw.device, generator=gen)
                    cand = (mean[:, None] + std[:, None] * noise).clamp_(LO, HI)
                    cand[:, 0] = mean
                    ret, first_done = env.score_t(cand)
                    s = ret - (first_done < n).to(torch.float64) * PENALTY
                    idx = torch.topk(s, K, dim=0).indices                                   # (K, E)
                    gidx = idx[None, :, :, None, None].expand(n, K, E, sw.num_drones, sw.act_dim)
                    el = torch.gather(cand, 1, gidx).to(torch.float64)
                    mean = el.mean(dim=1).to(torch.float32)
                    std = el.std(dim=1, unbiased=False).to(torch.float32).clamp_min_(SIGMA_MIN)
                state["action"] = mean[0]
                state["mean"] = torch.cat([mean[1:], mean[-1:]], dim=0)

        for _ in range(3 if way == "trace" else 10):
            tick()
        torch.cuda.synchronize()
        if way != "trace":
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(ticks):
                tick()
            b.record()
            torch.cuda.synchronize()
            out[name] = a.elapsed_time(b) * 1e3 / ticks   # µs per tick
        env.close()
    print(json.dumps({"way": way, "device": torch.cuda.get_device_name(0), "us_per_tick": out}))


def run_child(way, lib, args):
    env = dict(os.environ)
    env.pop("QS_DEV_LIB", None)
    if lib:
        env["QS_DEV_LIB"] = os.path.abspath(lib)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", way, "--steps", str(args.steps), "--ticks", str(args.ticks),
           "--iterations", str(args.iterations), "--shapes", args.shapes]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=args.limit)
    if p.returncode != 0:
        sys.exit(f"cem_ab: the {way} child ended with {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
    for line in reversed(p.stdout.splitlines()):
        if line.startswith("{"):
            return json.loads(line)
    sys.exit("cem_ab: no result line\n" + p.stdout[-2000:])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-lib", default=None, help="libquadswarm.so built from the parent commit (the torch way's)")
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--iterations", type=int, default=3)
    ap.add_argument("--ticks", type=int, default=200, help="ticks per timed window")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--limit", type=float, default=240.0, help="seconds per child")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, choices=("torch", "native", "trace"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    shapes = args.shapes.split(",")
    if args.child:
        return child(args.child, args.steps, args.iterations, args.ticks, shapes)
    if not args.parent_lib or not os.path.exists(args.parent_lib):
        sys.exit("cem_ab: --parent-lib must name a library built from the parent commit")
    if args.rounds < 3:
        sys.exit("cem_ab: at least three rounds")
    us = {name: {"torch": [], "native": []} for name in shapes}
    doc = {"what": "µs per CEM planner tick (window time / --ticks), device events around synchronised windows; torch: the "
                   "tick in torch ops round score_t on the parent commit's library; native: CEMPlanner.plan() on this "
                   "tree; the two alternated --rounds times in one job, a fresh process each, after a warm-up of each shape",
           "horizon": args.steps, "iterations": args.iterations, "elites": "C / 8, at least 1",
           "ticks_per_window": args.ticks, "rounds": args.rounds,
           "sigma": SIGMA, "sigma_min": SIGMA_MIN, "done_penalty": PENALTY, "shapes": {}}

    def save():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(json.dumps(doc, indent=1) + "\n")

    for r in range(args.rounds):
        for way, lib in (("torch", args.parent_lib), ("native", None)):
            res = run_child(way, lib, args)
            doc["device"] = res["device"]
            for name in shapes:
                us[name][way].append(res["us_per_tick"][name])
            print(f"round {r} {way}: " + ", ".join(f"{k} {v:.1f} us" for k, v in res["us_per_tick"].items()), flush=True)
            for name in shapes:
                doc["shapes"][name] = {"envs": SHAPES[name][0], "candidates": SHAPES[name][1],
                                       "elites": max(1, SHAPES[name][1] // 8), "us_per_tick": us[name]}
            save()
    for name in shapes:
        v = us[name]
        spread = {k: (max(x) - min(x)) / min(x) for k, x in v.items()}
        ratio = min(v["torch"]) / max(v["native"])
        need = 1 + 3 * max(spread.values())
        doc["shapes"][name].update(spread=spread, slowest_native_over_fastest_torch=ratio, gain_threshold=need,
                                   gain_by_the_rule=bool(ratio > need))
    save()
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
