#!/usr/bin/env python3
"""Time per candidate-step of scoring C candidate action sequences from one state, two ways.

MultiHover, one_d_pid, 8 drones, fp32, n = --steps steps per candidate, at three shapes
(E envs x C candidates): 1 x 4096, 64 x 256, 4096 x 4.

  restore_seq     what a caller could do before qs_score, existing entry points only: per
                  candidate, qs_state_io(set) of the four state blocks from a snapshot, then
                  qs_step_seq over the candidate's actions (reward / terminated / truncated
                  per step).  The state copies go through the C entry directly, without the
                  host synchronisation of QuadSwarm.set_state.
  score_per_step  one qs_score launch writing the same three outputs per step for all
                  candidates, plus ret and first_done
  score           one qs_score launch writing ret and first_done only

Every way is warmed up first; then the ways are alternated `--rounds` times in this one
process, each window (all C candidates; --score-reps launches of them for the qs_score
ways, whose single launch is too short a window) timed with device events around
synchronised work.  `restore_seq` ends by restoring the snapshot once more, as its caller
must before the real step.
Gain rule: the slowest `score_per_step` against the fastest `restore_seq`
must exceed one plus three times the larger spread.

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

SHAPES = {"E1_C4096": (1, 4096), "E64_C256": (64, 256), "E4096_C4": (4096, 4)}
BLOCKS = (L.STATE_AGENT, L.STATE_ENV, L.STATE_HISTORY, L.STATE_EP_RETURN)


def timed(fn, work, reps):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / (work * reps)   # µs per candidate-step


def run_shape(E, C, n, rounds, score_reps):
    sw = QuadSwarm(task="multihover", num_envs=E, num_drones=8, act="one_d_pid", initial_xyzs=grid_layout(8))
    sw.reset(0)
    for _ in range(3):
        sw.step(None)
    gen = torch.Generator(device="cpu").manual_seed(1)
    kw = dict(device=sw.device)
    acts = (torch.rand((n, C, E, sw.num_drones, sw.act_dim), generator=gen) * 2 - 1).to(sw.device)
    snap = [sw.get_state(blk).clone() for blk in BLOCKS]
    one = dict(reward=torch.empty((n, E), dtype=sw.rdtype, **kw), terminated=torch.zeros((n, E), dtype=torch.uint8, **kw),
               truncated=torch.zeros((n, E), dtype=torch.uint8, **kw))
    one_kws = [{k: v[j] for k, v in one.items()} for j in range(n)]
    cand_acts = [[acts[j, c] for j in range(n)] for c in range(C)]
    many = dict(reward=torch.empty((n, C, E), dtype=sw.rdtype, **kw),
                terminated=torch.zeros((n, C, E), dtype=torch.uint8, **kw),
                truncated=torch.zeros((n, C, E), dtype=torch.uint8, **kw))
    many_kws = [{k: v[j] for k, v in many.items()} for j in range(n)]
    ret = torch.empty((C, E), dtype=torch.float64, **kw)
    fd = torch.empty((C, E), dtype=torch.int32, **kw)

    def restore():
        st = sw._stream()
        for blk, buf in zip(BLOCKS, snap):
            L.check(sw.lib.qs_state_io(sw._h, blk, L.ptr(buf), 1, st), "qs_state_io(set)")

    def restore_seq():
        for c in range(C):
            restore()
            sw.step_many(one_kws, actions=cand_acts[c])
        restore()   # the envs' own state again

    def score_per_step():
        sw.score(acts, many_kws, ret=ret, first_done=fd)

    def score():
        sw.score(acts, ret=ret, first_done=fd)

    ways = {"restore_seq": restore_seq, "score_per_step": score_per_step, "score": score}
    for fn in ways.values():
        fn()
    torch.cuda.synchronize()
    # the last candidate of restore_seq against the same candidate of the launch: the same bytes
    same = bool(torch.equal(one["reward"], many["reward"][:, C - 1]) and torch.equal(one["truncated"], many["truncated"][:, C - 1]))
    us = {k: [] for k in ways}
    reps = {"restore_seq": 1, "score_per_step": score_reps, "score": score_reps}
    for _ in range(rounds):
        for k, fn in ways.items():
            us[k].append(timed(fn, C * n, reps[k]))
    for blk, buf in zip(BLOCKS, snap):   # leave the swarm as it was
        sw.set_state(blk, buf)
    spread = {k: (max(v) - min(v)) / min(v) for k, v in us.items()}
    ratio = min(us["restore_seq"]) / max(us["score_per_step"])
    need = 1 + 3 * max(spread["restore_seq"], spread["score_per_step"])
    out = {"envs": E, "candidates": C, "steps": n, "score_depth": sw.score_depth(), "us_per_candidate_step": us,
           "launches_per_score_window": score_reps, "spread": spread, "last_candidate_rewards_equal": same,
           "slowest_score_per_step_over_fastest_restore_seq": ratio, "gain_threshold": need,
           "gain_by_the_rule": bool(ratio > need)}
    sw.close()
    return out


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--steps", type=int, default=16)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--score-reps", type=int, default=20, help="qs_score launches per timed window (one is ~0.1 ms)")
    p.add_argument("--shapes", default=",".join(SHAPES))
    p.add_argument("--out", default=None)
    args = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("step_score_ab: no GPU (this script measures; it has no fallback)")
    if args.rounds < 3:
        sys.exit("step_score_ab: at least three rounds")
    doc = {"what": "µs per candidate-step (window time / (C * n)), device events around synchronised windows of all C "
                   "candidates; the ways alternated --rounds times in one process after a warm-up of each",
           "device": torch.cuda.get_device_name(0), "shapes": {}}
    for name in args.shapes.split(","):
        E, C = SHAPES[name]
        doc["shapes"][name] = run_shape(E, C, args.steps, args.rounds, args.score_reps)
    text = json.dumps(doc, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
