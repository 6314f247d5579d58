#!/usr/bin/env python3
"""Time per particle (SMC) planner tick, two ways, alternated between two builds of the
library; the native tick's split by stage; and a closed-loop comparison.

MultiHover, one_d_pid, 8 drones, fp32, horizon n = --steps in segments of L = --segment,
ess_frac = 0.5, at three shapes (E envs x C particles): 1 x 4096, 64 x 256, 4096 x 4.  A
tick forks C branches per env, and per segment draws actions round the nominal, advances
the branches, weighs them and resamples the envs whose effective sample size is low; then
it traces the surviving particles' actions back and folds them into the nominal.

  torch    the tick in torch ops round `BranchSet`: randn, mul, add, clamp, advance,
           softmax, cumsum, searchsorted, select, gather and a weighted mean.  Needs nothing
           newer than qs_branch_*, so it runs on the library given by --parent-lib (a build
           of the parent commit).
  native   `SMCPlanner.plan()` on this tree's library.

  smc_ab.py --parent-lib /path/libquadswarm.so --rounds 5 --out FILE

Each round runs the two ways once, `torch` first, each in a fresh child process (this
script with --child) under its own time limit; a child that fails, times out or prints
no result ends the whole run at once (nothing more is started on the GPU).  A child warms
every shape up, then times one window of --ticks ticks per shape with device events
around synchronised work; nothing inside a window reads back to the host.
Gain rule: the slowest `native` against the fastest `torch` must exceed one
plus three times the larger spread.

After the rounds two more children run on this tree's library, reported and not gated:
`split` times the native tick's stages inside real ticks with a device event after every
call (begin, sample, advance, resample, finish = weights + trace + sum; the select inside
resample also on its own; µs per tick), and `closed` runs 200 receding-horizon ticks from one
seed at 64 envs and C = 64 for SMC (n = 64), MPPI (n = 16) and SMC with ess_frac = 0, and
reports the mean env reward per step.

Writes one JSON document (--out) and prints it.  Needs a GPU: there is no fallback.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"E1_C4096": (1, 4096), "E64_C256": (64, 256), "E4096_C4": (4096, 4)}
SIGMA, LO, HI, LAM, PENALTY, FRAC = 0.3, -1.0, 1.0, 0.5, 10.0, 0.5


def make_env(E, seed=0):
    sys.path.insert(0, os.path.join(ROOT, "marl-gym-pybullet-drones_amd"))
    from gym_pybullet_drones_amd.envs.swarm import grid_layout
    from gym_pybullet_drones_amd.vec_env.vec_env import SwarmVecEnv
    env = SwarmVecEnv(task="multihover", num_envs=E, num_drones=8, act="one_d_pid", initial_xyzs=grid_layout(8), seed=seed)
    env.reset_t()
    for _ in range(3):
        env.step_t(None)
    return env


def torch_tick(env, n, seg, C):
    """The tick in torch ops round a `BranchSet`; returns the callable and its state."""
    import torch
    sw = env.swarm
    E, D, A, dev = sw.num_envs, sw.num_drones, sw.act_dim, sw.device
    gen = torch.Generator(device=dev).manual_seed(1)
    bs = env.branches(C)
    segs = [(j, min(seg, n - j)) for j in range(0, n, seg)]
    state = {"nominal": torch.zeros((n, E, D, A), device=dev)}
    ident = torch.arange(C, device=dev)[:, None].expand(C, E)
    rows = torch.arange(C, device=dev, dtype=torch.float64)[:, None]

    def weights(base, t):
        score = bs.ret - (bs.first_done < t).to(torch.float64) * PENALTY
        return score, torch.softmax((score - base) / LAM, dim=0)

    def tick():
        nom = state["nominal"]
        bs.fork()
        base = torch.zeros((C, E), dtype=torch.float64, device=dev)
        cands, parents = [], []
        for s, (a, b) in enumerate(segs):
            noise = torch.randn((b, C, E, D, A), device=dev, generator=gen)
            cand = (nom[a:a + b, None] + SIGMA * noise).clamp_(LO, HI)
            cand[:, 0] = nom[a:a + b]
            bs.advance(cand)
            cands.append(cand)
            if s == len(segs) - 1:
                break
            score, w = weights(base, a + b)
            go = (1.0 / (w * w).sum(dim=0) < FRAC * C)[None, :]
            cum = torch.cumsum(w, dim=0).t().contiguous()                                  # (E, C)
            u = torch.rand((E,), device=dev, generator=gen, dtype=torch.float64)
            pos = ((rows + u[None, :]) / C).t().contiguous()
            par = torch.searchsorted(cum, pos, right=True).clamp_(max=C - 1).t()             # the lowest c with cum > pos
            par = torch.where(go, par, ident)
            base = torch.where(go, torch.gather(score, 0, par), base)
            par32 = par.to(torch.int32).contiguous()
            bs.select(par32)
            parents.append(par)
        _, w = weights(base, n)
        anc, new = ident, [None] * len(segs)
        for s in range(len(segs) - 1, -1, -1):
            b = segs[s][1]
            path = torch.gather(cands[s], 1, anc[None, :, :, None, None].expand(b, C, E, D, A))
            new[s] = (w[None, :, :, None, None] * path.to(torch.float64)).sum(dim=1).to(torch.float32)
            if s > 0:
                anc = torch.gather(parents[s - 1], 0, anc)
        new = torch.cat(new, dim=0)
        state["action"] = new[0]
        state["nominal"] = torch.cat([new[1:], new[-1:]], dim=0)

    return tick, state


def window(fn, ticks):
    """µs per call of fn over one window of `ticks` calls, device events round synchronised work."""
    import torch
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(ticks):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / ticks


def child_ticks(way, n, seg, ticks, shapes):
    import torch
    out = {}
    for name in shapes:
        E, C = SHAPES[name]
        env = make_env(E)
        if way == "native":
            planner = env.smc(n, C, SIGMA, segment=seg, lo=LO, hi=HI, lam=LAM, done_penalty=PENALTY, ess_frac=FRAC, seed=1)
            tick = planner.plan
        else:
            tick, _ = torch_tick(env, n, seg, C)
        for _ in range(10):
            tick()
        out[name] = window(tick, ticks)
        env.close()
    print(json.dumps({"way": way, "device": torch.cuda.get_device_name(0), "us_per_tick": out}))


def child_split(n, seg, ticks, shapes):
    """The native tick's stages inside real ticks: a device event after every call of plan()'s own sequence, the
    time between two events charged to the call between them (so a stage carries the wait for its launch), summed
    by stage over a window of --ticks ticks; µs per tick.  The select inside resample is timed on its own, in a
    window of its own, and taken off to give the weigh + resample kernel."""
    import torch
    out = {}
    for name in shapes:
        E, C = SHAPES[name]
        env = make_env(E)
        pl = env.smc(n, C, SIGMA, segment=seg, lo=LO, hi=HI, lam=LAM, done_penalty=PENALTY, ess_frac=FRAC, seed=1)
        S = len(pl.segments)
        for _ in range(5):
            pl.plan()
        marks = []

        def mark(stage):
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            marks.append((stage, ev))

        resampled = torch.zeros((), dtype=torch.float64, device=env.swarm.device)
        torch.cuda.synchronize()
        for _ in range(ticks):
            mark(None)
            pl.begin()
            mark("begin_fork")
            for s in range(S):
                pl.sample(s)
                mark("sample")
                pl.advance(s)
                mark("advance")
                pl.resample(s)
                mark("resample_weigh_and_select")
            pl.finish()
            mark("finish_weights_trace_sum")
            resampled += pl.resampled[:max(S - 1, 1)].to(torch.float64).mean()
        torch.cuda.synchronize()
        res = {}
        for (_, a), (stage, b) in zip(marks[:-1], marks[1:]):
            if stage is not None:
                res[stage] = res.get(stage, 0.0) + a.elapsed_time(b) * 1e3 / ticks
        res["tick_by_stages"] = sum(res.values())
        res["select_alone"] = window(lambda: [pl.set.select(pl.parents[s]) for s in range(S - 1)], ticks)
        res["weigh_and_resample_kernel"] = res["resample_weigh_and_select"] - res["select_alone"]
        res["plan"] = window(pl.plan, ticks)
        res["envs_resampled_fraction"] = float(resampled.item()) / ticks
        out[name] = res
        env.close()
    print(json.dumps({"way": "split", "device": torch.cuda.get_device_name(0), "us_per_tick_by_stage": out}))


def child_closed(ticks=200, E=64, C=64):
    import torch
    out = {}
    for name in ("smc_n64", "mppi_n16", "smc_n64_ess0"):
        env = make_env(E, seed=5)
        kw = dict(lo=LO, hi=HI, lam=LAM, done_penalty=PENALTY, seed=1)
        if name == "mppi_n16":
            planner = env.mppi(16, C, SIGMA, **kw)
        else:
            planner = env.smc(64, C, SIGMA, segment=16, ess_frac=FRAC if name == "smc_n64" else 0.0, **kw)
        total = torch.zeros((), dtype=torch.float64, device=env.swarm.device)
        for _ in range(ticks):
            total += planner.step_t().reward.to(torch.float64).mean()
        torch.cuda.synchronize()
        out[name] = float(total.item()) / ticks
        env.close()
    print(json.dumps({"way": "closed", "device": torch.cuda.get_device_name(0), "mean_env_reward_per_step": out,
                      "ticks": ticks, "envs": E, "particles": C}))


def run_child(way, lib, args):
    env = dict(os.environ)
    env.pop("QS_DEV_LIB", None)
    if lib:
        env["QS_DEV_LIB"] = os.path.abspath(lib)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", way, "--steps", str(args.steps), "--segment", str(args.segment),
           "--ticks", str(args.ticks), "--shapes", args.shapes]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=args.limit)
    if p.returncode != 0:
        sys.exit(f"smc_ab: the {way} child ended with {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
    for line in reversed(p.stdout.splitlines()):
        if line.startswith("{"):
            return json.loads(line)
    sys.exit("smc_ab: no result line\n" + p.stdout[-2000:])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-lib", default=None, help="libquadswarm.so built from the parent commit (the torch way's)")
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--segment", type=int, default=16)
    ap.add_argument("--ticks", type=int, default=50, help="ticks per timed window")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--limit", type=float, default=240.0, help="seconds per child")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, choices=("torch", "native", "split", "closed"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    shapes = args.shapes.split(",")
    if args.child in ("torch", "native"):
        return child_ticks(args.child, args.steps, args.segment, args.ticks, shapes)
    if args.child == "split":
        return child_split(args.steps, args.segment, args.ticks, shapes)
    if args.child == "closed":
        return child_closed()
    if not args.parent_lib or not os.path.exists(args.parent_lib):
        sys.exit("smc_ab: --parent-lib must name a library built from the parent commit")
    if args.rounds < 3:
        sys.exit("smc_ab: at least three rounds")
    us = {name: {"torch": [], "native": []} for name in shapes}
    doc = {"what": "µs per SMC planner tick (window time / --ticks), device events around synchronised windows; torch: the "
                   "tick in torch ops round BranchSet on the parent commit's library; native: SMCPlanner.plan() on this "
                   "tree; the two alternated --rounds times in one job, a fresh process each, after a warm-up of each shape",
           "horizon": args.steps, "segment": args.segment, "ticks_per_window": args.ticks, "rounds": args.rounds,
           "sigma": SIGMA, "lambda": LAM, "done_penalty": PENALTY, "ess_frac": FRAC, "shapes": {}}

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
                doc["shapes"][name] = {"envs": SHAPES[name][0], "particles": SHAPES[name][1], "us_per_tick": us[name]}
            save()
    for name in shapes:
        v = us[name]
        spread = {k: (max(x) - min(x)) / min(x) for k, x in v.items()}
        ratio = min(v["torch"]) / max(v["native"])
        need = 1 + 3 * max(spread.values())
        doc["shapes"][name].update(spread=spread, slowest_native_over_fastest_torch=ratio, gain_threshold=need,
                                   gain_by_the_rule=bool(ratio > need))
    save()
    doc["split"] = run_child("split", None, args)["us_per_tick_by_stage"]
    save()
    closed = run_child("closed", None, args)
    doc["closed_loop"] = {k: closed[k] for k in ("mean_env_reward_per_step", "ticks", "envs", "particles")}
    save()
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
