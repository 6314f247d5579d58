#!/usr/bin/env python3
"""Time per MPPI tick with a policy prior, two ways, alternated between two builds of the library.

MultiHover, one_d_pid, 8 drones, fp32, horizon n = --steps, K = 4 prior candidates per env, at
three shapes (E envs x C candidates): 1 x 4096, 64 x 256, 4096 x 4 (there K = 3: candidate 0
stays the nominal, so a planner of 4 candidates takes at most 3), with an actor of hidden
size 64 and 256 behind the trainer's observation normaliser.  A tick is: roll the actor out
closed-loop K times per env from the envs' state, draw the other candidates, score them all,
softmax-weigh, fold into the nominal.

  torch    the tick in torch ops on the library given by --parent-lib (a build of the parent
           commit): `BranchSet.fork`, then per step the `MeanStdNormalizer`, three `F.linear`,
           two `tanh`, the scale, the noise, the clamp, the copy into the step's actions and a
           one-step `BranchSet.advance` that writes the next obs; then `MPPIPlanner.sample()`,
           the copy over the last K candidates, `score()` and `update()`.
  native   `MPPIPlanner.set_prior(...)` once, then `plan()`, on this tree's library.

  prior_ab.py --parent-lib /path/libquadswarm.so --rounds 5 --out FILE [-- bench.py arguments]

Each round runs the two ways once, `torch` first, each in a fresh child process (this script
with --child) under its own time limit; a child that fails, times out or prints no result
ends the whole run at once (nothing more is started on the GPU).  A child warms every case
up, then times one window of --ticks ticks per case with device events round synchronised
work; nothing inside a window reads back to the host.  After the ticks the plain
`bench.py --gpus 1` (which runs none of this code) is alternated between the two libraries
the same number of times (scripts/step_hot_ab.py's run_bench; the arguments after `--` go to
it).  Last, one child runs the closed loop (reported, not gated): an actor and a critic from
a short `MAPPO` run, then 64 envs, C = 64, 200 ticks from one seed with the deterministic
policy alone, the plain 16-step MPPI tick, the tick with the prior, and with the prior and
the value tail; --closed-only runs just that and merges it into the document --out already
holds.  Gain rule: the slowest of the new against the fastest of the old must
exceed one plus three times the larger spread.

Writes one JSON document (--out) and prints it.  Needs a GPU: there is no fallback.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"E1_C4096": (1, 4096, 4), "E64_C256": (64, 256, 4), "E4096_C4": (4096, 4, 3)}   # E, C, K
NETS = {"N64": 64, "N256": 256}
SIGMA, LO, HI, LAM, PENALTY, GAMMA, STD_SCALE = 0.3, -1.0, 1.0, 1.0, 10.0, 0.99, 1.0


def child(way, n, ticks, shapes):
    import torch
    import torch.nn.functional as F
    sys.path.insert(0, os.path.join(ROOT, "marl-gym-pybullet-drones_amd"))
    from gym_pybullet_drones_amd.envs.swarm import grid_layout
    from gym_pybullet_drones_amd.mappo.agent import MLPActor
    from gym_pybullet_drones_amd.mappo.normalization import MeanStdNormalizer
    from gym_pybullet_drones_amd.vec_env.vec_env import SwarmVecEnv
    if not torch.cuda.is_available():
        sys.exit("prior_ab: no GPU (this script measures; it has no fallback)")
    out = {}
    for name in shapes:
        E, C, K = SHAPES[name]
        for net, N in NETS.items():
            env = SwarmVecEnv(task="multihover", num_envs=E, num_drones=8, act="one_d_pid", initial_xyzs=grid_layout(8),
                              seed=0)
            env.reset_t()
            for _ in range(3):
                env.step_t(None)
            sw = env.swarm
            dev, D, O, A = sw.device, sw.num_drones, sw.obs_dim, sw.act_dim
            torch.manual_seed(N)
            actor = MLPActor(O, A, [N, N], "tanh", False, 0.5).to(dev)
            nz = MeanStdNormalizer(shape=(D, O), read_only=True, device=dev)
            nz.rms.mean.copy_(torch.randn((D, O), dtype=torch.float64) * 0.1)
            nz.rms.var.copy_(torch.rand((D, O), dtype=torch.float64) + 0.5)
            planner = env.mppi(n, C, SIGMA, lo=LO, hi=HI, lam=LAM, done_penalty=PENALTY, seed=1)
            if way == "native":
                planner.set_prior(actor, K, sw.obs, nz, std_scale=STD_SCALE)
                tick = planner.plan
            else:
                bs = env.branches(K)
                slots = torch.zeros((n, K, E, D, O), device=dev)
                acts = torch.zeros((n, K, E, D, A), device=dev)
                (w1, b1), (w2, b2), (w3, b3) = ((fc.weight, fc.bias) for fc in actor.pi_net.fcs)
                first = torch.ones((K, 1, 1, 1), device=dev)
                first[0] = 0.0                                      # trajectory 0 is the mode

                def tick():
                    with torch.no_grad():
                        bs.fork()
                        slots[0].copy_(sw.obs.expand(K, E, D, O))
                        std = STD_SCALE * torch.exp(actor.logstd)
                        for j in range(n):
                            x = nz(slots[j].view(K * E, D, O)).view(K * E * D, O)
                            mean = F.linear(torch.tanh(F.linear(torch.tanh(F.linear(x, w1, b1)), w2, b2)), w3, b3)
                            mean = (mean * actor.action_scale).view(K, E, D, A)
                            noise = torch.randn_like(mean) * std * first
                            torch.clamp(mean + noise, LO, HI, out=acts[j])
                            if j < n - 1:
                                bs.advance([acts[j]], [dict(obs=slots[j + 1])])
                        planner.sample()
                        planner.candidates[:, C - K:].copy_(acts)
                        planner.score()
                        planner.update()

            for _ in range(10):
                tick()
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(ticks):
                tick()
            b.record()
            torch.cuda.synchronize()
            out[f"{name}/{net}"] = a.elapsed_time(b) * 1e3 / ticks   # µs per tick
            env.close()
    print(json.dumps({"way": way, "device": torch.cuda.get_device_name(0), "us_per_tick": out}))


def child_closed(ticks=200, E=64, C=64, K=4, train_steps=30):
    """Closed loop (reported, not gated): an actor and a critic from a short MAPPO run (hidden 64, 64 envs,
    `train_steps` rollouts of 100 steps, gamma = 0.99, no normalisers), then 200 control steps from one seed with
    the deterministic policy alone and with the 16-step MPPI tick plain, with the prior, and with prior and value tail."""
    import tempfile
    import torch
    sys.path.insert(0, os.path.join(ROOT, "marl-gym-pybullet-drones_amd"))
    from gym_pybullet_drones_amd.envs import MultiHoverAviary
    from gym_pybullet_drones_amd.envs.swarm import grid_layout
    from gym_pybullet_drones_amd.mappo import MAPPO
    from gym_pybullet_drones_amd.utils.enums import ActionType, Physics
    from gym_pybullet_drones_amd.vec_env.vec_env import SwarmVecEnv
    env_func = lambda seed=0, **kw: MultiHoverAviary(num_drones=8, act=ActionType.ONE_D_PID, physics=Physics.DYN,   # noqa: E731
                                                     initial_xyzs=grid_layout(8))
    m = MAPPO(env_func, output_dir=tempfile.mkdtemp(), use_gpu=True, seed=0, hidden_dim=64, rollout_batch_size=E,
              rollout_steps=100)
    m.reset()
    for _ in range(train_steps):
        m.train_step()
    torch.cuda.synchronize()
    actor, critic = m.agent.ac.actor, m.agent.ac.critic
    lam, penalty = 0.5, PENALTY
    out = {}
    for name in ("policy", "mppi_n16", "mppi_n16_prior", "mppi_n16_prior_value"):
        env = SwarmVecEnv(task="multihover", num_envs=E, num_drones=8, act="one_d_pid", initial_xyzs=grid_layout(8), seed=5)
        env.reset_t()
        for _ in range(3):
            env.step_t(None)
        sw = env.swarm
        total = torch.zeros((), dtype=torch.float64, device=sw.device)
        if name == "policy":
            with torch.no_grad():
                for _ in range(ticks):
                    mode = actor.pi_net(sw.obs.view(-1, sw.obs_dim)) * actor.action_scale
                    act = torch.clamp(mode, LO, HI).view(E, sw.num_drones, sw.act_dim).contiguous()
                    total += env.step_t(act).reward.to(torch.float64).mean()
        else:
            planner = env.mppi(16, C, SIGMA, lo=LO, hi=HI, lam=lam, done_penalty=penalty, seed=1)
            if name != "mppi_n16":
                planner.set_prior(actor, K, sw.obs, std_scale=STD_SCALE)
            if name == "mppi_n16_prior_value":
                planner.set_value(critic, gamma=GAMMA)
            for _ in range(ticks):
                total += planner.step_t().reward.to(torch.float64).mean()
        torch.cuda.synchronize()
        out[name] = float(total.item()) / ticks
        env.close()
    print(json.dumps({"way": "closed", "device": torch.cuda.get_device_name(0), "mean_env_reward_per_step": out,
                      "ticks": ticks, "envs": E, "candidates": C, "prior_candidates": K, "std_scale": STD_SCALE,
                      "nets": {"hidden": 64, "train_steps": train_steps, "rollout_steps": 100, "gamma": GAMMA},
                      "lambda": lam, "done_penalty": penalty}))


def run_child(way, lib, args):
    env = dict(os.environ)
    env.pop("QS_DEV_LIB", None)
    if lib:
        env["QS_DEV_LIB"] = os.path.abspath(lib)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", way, "--steps", str(args.steps), "--ticks", str(args.ticks),
           "--shapes", args.shapes]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=args.limit)
    if p.returncode != 0:
        sys.exit(f"prior_ab: the {way} child ended with {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
    for line in reversed(p.stdout.splitlines()):
        if line.startswith("{"):
            return json.loads(line)
    sys.exit("prior_ab: no result line\n" + p.stdout[-2000:])


def by_the_rule(old, new, smaller_is_better):
    """(ratio, threshold, gain): the slowest new against the fastest old, and one plus three times the larger spread."""
    spread = max((max(x) - min(x)) / min(x) for x in (old, new))
    ratio = min(old) / max(new) if smaller_is_better else min(new) / max(old)
    return ratio, 1 + 3 * spread, bool(ratio > 1 + 3 * spread)


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
    ap.add_argument("--child", default=None, choices=("torch", "native", "closed"), help=argparse.SUPPRESS)
    args = ap.parse_args(argv)
    shapes = args.shapes.split(",")
    if args.child == "closed":
        return child_closed()
    if args.child:
        return child(args.child, args.steps, args.ticks, shapes)
    if args.closed_only:
        doc = json.load(open(args.out)) if args.out and os.path.exists(args.out) else {}
        res = run_child("closed", None, args)
        doc["closed_loop"] = {k: v for k, v in res.items() if k not in ("way", "device")}
        if args.out:
            with open(args.out, "w") as f:
                f.write(json.dumps(doc, indent=1) + "\n")
        print(json.dumps(doc["closed_loop"], indent=1))
        return None
    if not args.parent_lib or not os.path.exists(args.parent_lib):
        sys.exit("prior_ab: --parent-lib must name a library built from the parent commit")
    if args.rounds < 3:
        sys.exit("prior_ab: at least three rounds")
    cases = [f"{s}/{net}" for s in shapes for net in NETS]
    us = {c: {"torch": [], "native": []} for c in cases}
    doc = {"what": "µs per MPPI tick with a policy prior (window time / --ticks), device events round synchronised windows; "
                   "torch: BranchSet.fork, per step the normaliser, three linear, two tanh, scale, noise, clamp, copy and a "
                   "one-step BranchSet.advance, then sample(), the copy into candidates, score(), update() in torch ops on "
                   "the parent commit's library; native: set_prior() once, then plan() on this tree; the two alternated "
                   "--rounds times in one job, a fresh process each, after a warm-up of each case",
           "horizon": args.steps, "ticks_per_window": args.ticks, "rounds": args.rounds, "std_scale": STD_SCALE,
           "sigma": SIGMA, "lambda": LAM, "done_penalty": PENALTY, "cases": {}, "plain_bench": None}

    def save():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(json.dumps(doc, indent=1) + "\n")

    for r in range(args.rounds):
        for way, lib in (("torch", args.parent_lib), ("native", None)):
            res = run_child(way, lib, args)
            doc["device"] = res["device"]
            for c in cases:
                us[c][way].append(res["us_per_tick"][c])
                E, C, K = SHAPES[c.split("/")[0]]
                doc["cases"][c] = {"envs": E, "candidates": C, "prior_candidates": K, "hidden": NETS[c.split("/")[1]],
                                   "us_per_tick": us[c]}
            print(f"round {r} {way}: " + ", ".join(f"{k} {v:.1f}" for k, v in res["us_per_tick"].items()) + " us", flush=True)
            save()
    for c in cases:
        ratio, need, gain = by_the_rule(us[c]["torch"], us[c]["native"], smaller_is_better=True)
        doc["cases"][c].update(slowest_native_over_fastest_torch=ratio, gain_threshold=need, gain_by_the_rule=gain)
    save()
    import step_hot_ab
    runs = {"parent": [], "this": []}
    for r in range(args.rounds):
        for name, lib in (("parent", args.parent_lib), ("this", None)):
            res = step_hot_ab.run_bench(lib, {}, bench_args, args.limit)
            runs[name].append(res["value"])
            print(f"round {r} bench {name}: {res['value'] / 1e9:.4f}e9 agent-steps/s", flush=True)
            doc["plain_bench"] = {"arguments": bench_args, "unit": "agent-steps/s", "value": runs}
            save()
    ratio, need, gain = by_the_rule(runs["parent"], runs["this"], smaller_is_better=False)
    doc["plain_bench"].update(slowest_this_over_fastest_parent=ratio, gain_threshold=need, gain_by_the_rule=gain)
    save()
    res = run_child("closed", None, args)
    doc["closed_loop"] = {k: v for k, v in res.items() if k not in ("way", "device")}
    save()
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
