#!/usr/bin/env python3
"""The ring launch's stores (QS_RING_ITEMS, csrc/step_kernel.h): the memory floor and the A/B.

  step_store_ab.py --parent /path/libquadswarm.so --dev-dir marl-gym-pybullet-drones_amd/build/dev \\
                   --rounds 7 --out-dir DIR [--tag _repeat] [--skip floor|ab] [--dump DIR] [-- bench args]

Two alternations in one GPU job, both on plain `bench.py --gpus 1` (scripts/step_hot_ab.py runs
the children: a fresh process each under its own time limit, the whole run ending at the first
child that fails):

 1. `DIR/step_store_floor<tag>.json`: the `-DQS_X_NOCOMPUTE` libraries (no PID, no substeps: what
    the launch's loads and stores alone take) of the parent, of this tree, and of this tree with
    each QS_RING_ITEMS bit left out.
 2. `DIR/step_store_ab<tag>.json`: the parent's library, this tree's, and this tree's with each
    bit left out, judged by the gain rule of DESIGN.md §4; with `--dump` the `--dump-outputs`
    arrays at `--steps 40` and at the default are then compared with the parent's.

The dev libraries come from scripts/build_dev_step.sh (only step_mh_ring differs between them):
  lib_floor_parent.so  the parent's sources, -DQS_X_NOCOMPUTE
  lib_floor.so         this tree, -DQS_X_NOCOMPUTE
  lib_floor_nohist.so  this tree, -DQS_X_NOCOMPUTE and QS_RING_ITEMS without bit 1
  lib_nohist.so        this tree, QS_RING_ITEMS without bit 1
A library that is not there is left out of the alternation.  (profiles/step_store_*.json were
taken on a tree that also carried bit 2, a placement of neighbouring env blocks on one XCD that
was not adopted, DESIGN.md §9l: there `this` has both bits, `no_place` (lib_noplace.so,
lib_floor_noplace.so: bit 1 alone) is what this tree builds, and `no_hist` is bit 2 alone.)
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import step_hot_ab  # noqa: E402


def alternate(variants, rounds, limit, out, bench_args, dump=None):
    sys.argv = [sys.argv[0]]
    for name, lib in variants:
        sys.argv += ["--variant", f"{name}={lib}"]
    sys.argv += ["--rounds", str(rounds), "--limit", str(limit), "--out", out]
    if dump:
        sys.argv += ["--dump", dump]
    sys.argv += ["--"] + bench_args
    step_hot_ab.main()


def dump_default(variants, limit, dump, out, bench_args):
    """--dump-outputs at the bench's default --steps, compared with the first variant's."""
    import numpy as np
    for name, lib in variants:
        d = os.path.join(dump, name + "_default")
        os.makedirs(d, exist_ok=True)
        step_hot_ab.run_bench(lib, {}, bench_args + ["--dump-outputs", d], limit)
    first = os.path.join(dump, variants[0][0] + "_default")
    same = {name: {f: bool(np.array_equal(np.load(os.path.join(first, f)), np.load(os.path.join(dump, name + "_default", f))))
                   for f in sorted(os.listdir(first)) if f.endswith(".npy")} for name, _ in variants[1:]}
    with open(out) as f:
        doc = json.load(f)
    doc["dump_outputs_default_steps_equal_to_" + variants[0][0]] = same
    with open(out, "w") as f:
        f.write(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(same, indent=1), flush=True)


def main():
    argv = sys.argv[1:]
    bench_args = []
    if "--" in argv:
        k = argv.index("--")
        argv, bench_args = argv[:k], argv[k + 1:]
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent", required=True, help="the parent commit's libquadswarm.so")
    ap.add_argument("--dev-dir", required=True, help="where build_dev_step.sh left the lib_*.so")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--floor-rounds", type=int, default=None, help="rounds of the floor alternation (default: --rounds)")
    ap.add_argument("--out-dir", required=True)
    ap.add_argument("--tag", default="")
    ap.add_argument("--skip", action="append", default=[], choices=["floor", "ab"])
    ap.add_argument("--dump", default=None)
    ap.add_argument("--limit", type=float, default=240.0, help="seconds per child")
    args = ap.parse_args(argv)

    def dev(name):
        p = os.path.join(args.dev_dir, f"lib_{name}.so")
        return os.path.abspath(p) if os.path.exists(p) else None

    if "floor" not in args.skip:
        v = [(n, dev(lib)) for n, lib in (("parent", "floor_parent"), ("this", "floor"), ("no_hist", "floor_nohist"),
                                          ("no_place", "floor_noplace"))]
        v = [(n, lib) for n, lib in v if lib]
        alternate(v, args.floor_rounds or args.rounds, args.limit,
                  os.path.join(args.out_dir, f"step_store_floor{args.tag}.json"), bench_args)
    if "ab" not in args.skip:
        v = [("parent", os.path.abspath(args.parent)), ("this", "")]
        v += [(n, dev(lib)) for n, lib in (("no_hist", "nohist"), ("no_place", "noplace")) if dev(lib)]
        out = os.path.join(args.out_dir, f"step_store_ab{args.tag}.json")
        alternate(v, args.rounds, args.limit, out, bench_args, args.dump)
        if args.dump:
            dump_default(v, args.limit, args.dump, out, bench_args)


if __name__ == "__main__":
    main()
