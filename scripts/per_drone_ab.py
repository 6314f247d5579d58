#!/usr/bin/env python3
"""What per-drone returns and per-drone planner ticks cost, and what they change in closed loop.

MultiHover, one_d_pid, 8 drones, fp32, horizon n = --steps, at three shapes (E envs x C
candidates): 1 x 4096, 64 x 256, 4096 x 4, all on this tree's library.

  mppi_env / mppi_pd     `MPPIPlanner.plan()`, env-level and per_drone=True
  cem_env / cem_pd       `CEMPlanner.plan()` (K = C / 8, --iters iterations), likewise
  score / score_agents   the score launch alone over fixed candidates: `QuadSwarm.score` with
                         ret and first_done, without and with ret_agent

  per_drone_ab.py --parent-lib /path/libquadswarm.so --rounds 5 --out FILE [--part ticks,closed,bench]

Each round runs the six ways once, each in a fresh child process (this script with --child)
under its own time limit; a child that fails, times out or prints no result ends the whole
run at once (nothing more is started on the GPU).  A child warms every shape up, then times
one window of --ticks ticks per shape with device events around synchronised work; nothing
inside a window reads back to the host.  No number is promised: the file reports the costs.

Then, in the same job:
  bench    plain `bench.py --gpus 1` on the library given by --parent-lib (a build of the parent
           commit) and on this tree's, alternated --rounds times, and once each with
           --dump-outputs (scripts/step_hot_ab.py does both).  Unchanged by the rule of
           DESIGN.md §4: the slowest run of this tree is within the fastest of the parent
           times one plus three times the larger spread.
  closed   64 envs, C = 64, 200 receding-horizon ticks from one seed: the mean env reward per
           tick of env-level MPPI (lambda) against per-drone MPPI (lambda * D, the documented
           scale).  Recorded without a pass mark.

Writes one JSON document (--out) and prints it; --part runs some of the three parts and
keeps what --out already holds of the others, so that a job with a time limit can be cut in
two.  Needs a GPU: there is no fallback.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"E1_C4096": (1, 4096), "E64_C256": (64, 256), "E4096_C4": (4096, 4)}
WAYS = ("mppi_env", "mppi_pd", "cem_env", "cem_pd", "score", "score_agents")
SIGMA, SIGMA_MIN, LO, HI, LAM, PENALTY, D = 0.3, 0.01, -1.0, 1.0, 1.0, 10.0, 8
CLOSED = dict(envs=64, candidates=64, ticks=200, seed=5, sigma=0.3, lam=0.05)


def make_env(E, seed=0):
    sys.path.insert(0, os.path.join(ROOT, "marl-gym-pybullet-drones_amd"))
    from gym_pybullet_drones_amd.envs.swarm import grid_layout
    from gym_pybullet_drones_amd.vec_env.vec_env import SwarmVecEnv
    env = SwarmVecEnv(task="multihover", num_envs=E, num_drones=D, act="one_d_pid", initial_xyzs=grid_layout(D), seed=seed)
    env.reset_t()
    return env


def child(way, n, iters, ticks, shapes):
    import torch
    if not torch.cuda.is_available():
        sys.exit("per_drone_ab: no GPU (this script measures; it has no fallback)")
    if way == "closed":
        return closed(n)
    kind, _, mode = way.partition("_")
    out = {}
    for name in shapes:
        E, C = SHAPES[name]
        env = make_env(E)
        for _ in range(3):
            env.step_t(None)
        sw = env.swarm
        pd = mode == "pd"
        # a per-drone score is D times an env-level one: lambda and the penalty scale with it
        scale = D if pd else 1
        if kind == "mppi":
            tick = env.mppi(n, C, SIGMA, lo=LO, hi=HI, lam=LAM * scale, done_penalty=PENALTY * scale, seed=1, per_drone=pd).plan
        elif kind == "cem":
            tick = env.cem(n, C, max(1, C // 8), SIGMA, iterations=iters, lo=LO, hi=HI, sigma_min=SIGMA_MIN,
                           done_penalty=PENALTY * scale, seed=1, per_drone=pd).plan
        else:
            gen = torch.Generator(device=sw.device).manual_seed(1)
            cand = (SIGMA * torch.randn((n, C, E, D, sw.act_dim), device=sw.device, generator=gen)).clamp_(LO, HI)
            kw = dict(ret=torch.zeros((C, E), dtype=torch.float64, device=sw.device),
                      first_done=torch.zeros((C, E), dtype=torch.int32, device=sw.device))
            if mode == "agents":
                kw["ret_agent"] = torch.zeros((C, E, D), dtype=torch.float64, device=sw.device)

            def tick():
                sw.score(cand, **kw)

        for _ in range(10):
            tick()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(ticks):
            tick()
        b.record()
        torch.cuda.synchronize()
        out[name] = a.elapsed_time(b) * 1e3 / ticks   # µs per tick
        env.close()
    print(json.dumps({"way": way, "device": torch.cuda.get_device_name(0), "us_per_tick": out}))


def closed(n):
    """Both planners from the same reset, each driving its own envs; the reward stays on the device."""
    import torch
    c = CLOSED
    res = {}
    for mode, pd in (("env_level", False), ("per_drone", True)):
        env = make_env(c["envs"], seed=c["seed"])
        planner = env.mppi(n, c["candidates"], c["sigma"], lo=LO, hi=HI, lam=c["lam"] * (D if pd else 1), seed=c["seed"],
                           per_drone=pd)
        total = torch.zeros((), dtype=torch.float64, device=env.swarm.device)
        per_tick = []
        for _ in range(c["ticks"]):
            r = planner.step_t()
            m = r.reward.double().mean()
            total += m
            per_tick.append(m)
        torch.cuda.synchronize()
        curve = [float(x) for x in torch.stack(per_tick).cpu()]
        res[mode] = {"mean_env_reward_per_tick": float(total) / c["ticks"],
                     "first_50_ticks": sum(curve[:50]) / 50, "last_50_ticks": sum(curve[-50:]) / 50}
        env.close()
    print(json.dumps({"way": "closed", "device": torch.cuda.get_device_name(0), "closed_loop": res}))


def run_child(way, args):
    env = dict(os.environ)
    env.pop("QS_DEV_LIB", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", way, "--steps", str(args.steps), "--iters", str(args.iters),
           "--ticks", str(args.ticks), "--shapes", args.shapes]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=args.limit)
    if p.returncode != 0:
        sys.exit(f"per_drone_ab: the {way} child ended with {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
    for line in reversed(p.stdout.splitlines()):
        if line.startswith("{"):
            return json.loads(line)
    sys.exit("per_drone_ab: no result line\n" + p.stdout[-2000:])


def bench_ab(args):
    """scripts/step_hot_ab.py: bench.py on the two libraries, alternated, then --dump-outputs."""
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "bench.json")
        cmd = [sys.executable, os.path.join(ROOT, "scripts", "step_hot_ab.py"), "--variant", f"parent={args.parent_lib}",
               "--variant", "this=", "--rounds", str(args.rounds), "--limit", str(args.bench_limit), "--dump",
               os.path.join(tmp, "dump"), "--out", out]
        p = subprocess.run(cmd)   # (its progress lines pass through)
        if p.returncode != 0:
            sys.exit(f"per_drone_ab: the bench alternation ended with {p.returncode}")
        with open(out) as f:
            doc = json.load(f)
    v = {k: [x["value"] for x in runs] for k, runs in doc["runs"].items()}
    ratio = min(v["this"]) / max(v["parent"])
    floor = 1.0 / (1.0 + 3.0 * max(doc["spread"].values()))
    doc["unchanged_rule"] = {"slowest_this_over_fastest_parent": ratio, "floor": floor, "unchanged": bool(ratio >= floor)}
    doc.pop("gain_rule", None)
    return doc


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-lib", default=None, help="libquadswarm.so built from the parent commit (the bench alternation's)")
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--iters", type=int, default=3, help="CEM iterations a tick")
    ap.add_argument("--ticks", type=int, default=300, help="ticks per timed window")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--limit", type=float, default=240.0, help="seconds per child")
    ap.add_argument("--bench-limit", type=float, default=400.0, help="seconds per bench.py run")
    ap.add_argument("--part", default="ticks,closed,bench", help="which parts to run: ticks, closed, bench")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, choices=WAYS + ("closed",), help=argparse.SUPPRESS)
    args = ap.parse_args()
    shapes = args.shapes.split(",")
    if args.child:
        return child(args.child, args.steps, args.iters, args.ticks, shapes)
    parts = args.part.split(",")
    if "bench" in parts and (not args.parent_lib or not os.path.exists(args.parent_lib)):
        sys.exit("per_drone_ab: --parent-lib must name a library built from the parent commit")
    if args.rounds < 3:
        sys.exit("per_drone_ab: at least three rounds")
    us = {name: {w: [] for w in WAYS} for name in shapes}
    doc = {"what": "µs per tick (window time / --ticks), device events around synchronised windows, all on this tree's "
                   "library: plan() of the MPPI and CEM planners env-level (_env) and per-drone (_pd), and the score launch "
                   "alone without (score) and with ret_agent (score_agents); the six alternated --rounds times in one "
                   "job, a fresh process each, after a warm-up of each shape.  The per-drone planners run lambda and "
                   "done_penalty times D",
           "horizon": args.steps, "cem_iterations": args.iters, "cem_elites": "C / 8", "ticks_per_window": args.ticks,
           "rounds": args.rounds, "sigma": SIGMA, "lambda": LAM, "done_penalty": PENALTY, "drones": D, "shapes": {}}
    if args.out and os.path.exists(args.out) and "ticks" not in parts:
        with open(args.out) as f:
            doc = json.load(f)

    def save():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(json.dumps(doc, indent=1) + "\n")

    for r in range(args.rounds if "ticks" in parts else 0):
        for way in WAYS:
            res = run_child(way, args)
            doc["device"] = res["device"]
            for name in shapes:
                us[name][way].append(res["us_per_tick"][name])
            print(f"round {r} {way}: " + ", ".join(f"{k} {v:.1f} us" for k, v in res["us_per_tick"].items()), flush=True)
            for name in shapes:
                doc["shapes"][name] = {"envs": SHAPES[name][0], "candidates": SHAPES[name][1], "us_per_tick": us[name]}
            save()
    for name in shapes if "ticks" in parts else ():
        v = us[name]
        mean = {w: sum(x) / len(x) for w, x in v.items()}
        doc["shapes"][name].update(
            mean_us=mean, spread={w: (max(x) - min(x)) / min(x) for w, x in v.items()},
            per_drone_minus_env_level_us={"mppi": mean["mppi_pd"] - mean["mppi_env"], "cem": mean["cem_pd"] - mean["cem_env"],
                                          "score_launch": mean["score_agents"] - mean["score"]})
    save()
    if "closed" in parts:
        doc["closed_loop"] = {"what": "mean env reward per tick over 200 receding-horizon MPPI ticks from one seed, 64 envs, "
                                      "C = 64; env-level at lambda, per-drone at lambda * D; no pass mark",
                              **CLOSED, "horizon": args.steps, **run_child("closed", args)["closed_loop"]}
        save()
    if "bench" in parts:
        print("bench alternation ...", flush=True)
        doc["bench"] = bench_ab(args)
        save()
    print(json.dumps({k: v for k, v in doc.items()}, indent=1))


if __name__ == "__main__":
    main()
