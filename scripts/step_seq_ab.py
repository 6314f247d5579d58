#!/usr/bin/env python3
"""Time per control step of an action sequence known ahead of time, three ways.

At the bench's C3 shape (MultiHover, 16 384 envs x 8 drones, one_d_pid, fp32) and
its C4 shape (Spiral, 8 192 envs x 5 drones, vel), `--steps` steps whose actions
lie pre-generated on the device:

  eager        qs_step(h, actions[j]) per step (QuadSwarm.step)
  graph        those calls captured into one graph, replayed
  seq          qs_step_seq (QuadSwarm.step_many(outs, actions=...)), called eagerly
  seq_graph    that call captured into one graph, replayed
  random       random-policy step_many, the bound without an action read
  random_graph the same, captured

`eager` and `graph` run the single-step kernel; `seq` is the multi-step launch over
the caller's actions.  Every way is warmed up first; then the ways are alternated
`--rounds` times in this one process, each window timed with device events around
synchronised work.  Gain rule: the slowest `seq_graph` against the
fastest `graph` must exceed one plus three times the larger spread.

Writes one JSON document (--out) and prints it.  Needs a GPU: there is no fallback.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "marl-gym-pybullet-drones_amd"))

from gym_pybullet_drones_amd import _lib as L  # noqa: E402
from gym_pybullet_drones_amd.envs.swarm import QuadSwarm, grid_layout  # noqa: E402

SHAPES = {
    "C3": dict(task="multihover", num_envs=16384, num_drones=8, act="one_d_pid", initial_xyzs=grid_layout(8)),
    "C4": dict(task="spiral", num_envs=8192, num_drones=5, act="vel"),
}


def stagger(sw, gen):
    """Episode clocks spread over the episode length, so the truncations do not fall on one step."""
    env = sw.get_state(L.STATE_ENV).clone()
    steps = int(round(sw.episode_len_sec * sw.ctrl_freq))
    k = torch.randint(0, steps, (sw.num_envs,), generator=gen).to(device=env.device, dtype=torch.int32)
    env[L.E_STEP_COUNTER] = k * sw.substeps
    env[L.E_EP_LEN] = k
    sw.set_state(L.STATE_ENV, env)


def timed(fn, steps):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / steps   # µs per step


def graph_of(fn):
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    torch.cuda.synchronize()
    return g


def run_shape(name, cfg, steps, slots, rounds):
    sw = QuadSwarm(**cfg)
    sw.reset(0)
    gen = torch.Generator(device="cpu").manual_seed(1)
    stagger(sw, gen)
    E, D, O, A = sw.num_envs, sw.num_drones, sw.obs_dim, sw.act_dim
    kw = dict(device=sw.device)
    acts = (torch.rand((steps, E, D, A), generator=gen) * 2 - 1).to(sw.device)
    bufs = dict(obs=torch.empty((slots, E, D, O), **kw), reward=torch.empty((slots, E), dtype=sw.rdtype, **kw),
                terminated=torch.zeros((slots, E), dtype=torch.uint8, **kw),
                truncated=torch.zeros((slots, E), dtype=torch.uint8, **kw),
                actions_out=torch.empty((slots, E, D, A), **kw))
    kws = [{k: v[j % slots] for k, v in bufs.items()} for j in range(steps)]

    def eager():
        for j in range(steps):
            sw.step(acts[j], **kws[j])

    def seq():
        sw.step_many(kws, actions=acts)

    def rnd():
        sw.step_many(kws)

    g_single, g_seq, g_rnd = graph_of(eager), graph_of(seq), graph_of(rnd)
    ways = {"eager": eager, "graph": g_single.replay, "seq": seq, "seq_graph": g_seq.replay, "random": rnd,
            "random_graph": g_rnd.replay}
    for fn in ways.values():   # warm-up: every way once, untimed (a graph's first replay uploads it)
        fn()
    torch.cuda.synchronize()
    us = {k: [] for k in ways}
    for _ in range(rounds):
        for k, fn in ways.items():
            us[k].append(timed(fn, steps))
    out = {"config": {k: (v if isinstance(v, (int, str)) else "grid_layout") for k, v in cfg.items()},
           "agents": E * D, "act_dim": A, "steps": steps, "slots": slots, "us_per_step": us}
    spread = {k: (max(v) - min(v)) / min(v) for k, v in us.items()}
    out["spread"] = spread
    ratio = min(us["graph"]) / max(us["seq_graph"])   # slowest seq against fastest graph, as speeds
    need = 1 + 3 * max(spread["graph"], spread["seq_graph"])
    out["slowest_seq_graph_over_fastest_graph"] = ratio
    out["gain_threshold"] = need
    out["gain_by_the_rule"] = bool(ratio > need)
    assert sw.reset_error() == 0
    sw.close()
    return out


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--steps", type=int, default=484)
    p.add_argument("--slots", type=int, default=64, help="output buffer sets the steps cycle through")
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--shapes", default="C3,C4")
    p.add_argument("--out", default=None)
    args = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("step_seq_ab: no GPU (this script measures; it has no fallback)")
    if args.rounds < 3:
        sys.exit("step_seq_ab: at least three rounds")
    doc = {"what": "µs per control step, device events around synchronised windows of --steps steps; the ways "
                   "alternated --rounds times in one process after a warm-up of each",
           "device": torch.cuda.get_device_name(0), "QS_MAX_FUSED_STEPS": os.environ.get("QS_MAX_FUSED_STEPS"),
           "shapes": {}}
    for name in args.shapes.split(","):
        doc["shapes"][name] = run_shape(name, SHAPES[name], args.steps, args.slots, args.rounds)
    text = json.dumps(doc, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
