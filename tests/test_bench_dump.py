"""bench.py --dump-outputs: the arrays the last timed step of the headline rollout
returned, written as DIR/<name>.npy, and what a plain run (no --full) does."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("obs", "reward", "terminated", "truncated", "actions")


def test_dump_outputs_layout_and_seeded_sample(tmp_path, monkeypatch):
    """Under the size limit every row is written (uint8 flags as float32, float64
    kept); over it, the same seeded sample of env rows of every array, with the
    rows themselves in env_rows.npy, identical from call to call."""
    import bench
    E = 96
    g = torch.Generator().manual_seed(3)
    arrays = {"obs": torch.rand((E, 2, 5), generator=g), "reward": torch.rand(E, generator=g, dtype=torch.float64),
              "truncated": (torch.arange(E) % 3 == 0).to(torch.uint8)}
    bench.dump_outputs(str(tmp_path / "all"), 0, arrays)
    assert sorted(os.listdir(tmp_path / "all")) == ["obs.npy", "reward.npy", "truncated.npy"]
    for k, a in arrays.items():
        got = np.load(tmp_path / "all" / f"{k}.npy")
        assert got.dtype == (np.float64 if k == "reward" else np.float32)
        assert np.array_equal(got, a.numpy().astype(got.dtype))
    row_bytes = 2 * 5 * 4 + 8 + 4
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 40 * row_bytes + 7)
    for d in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / d), 1, arrays)
    rows = np.load(tmp_path / "s1" / "env_rows.rank1.npy").astype(np.int64)
    assert len(rows) == 40 and len(set(rows)) == 40 and (np.diff(rows) > 0).all() and rows.max() < E
    total = 0
    for k, a in arrays.items():
        got = np.load(tmp_path / "s1" / f"{k}.rank1.npy")
        total += got.nbytes
        assert np.array_equal(got, a.numpy()[rows].astype(got.dtype))
        assert np.array_equal(got, np.load(tmp_path / "s2" / f"{k}.rank1.npy"))
    assert total <= bench.DUMP_MAX_BYTES


@pytest.mark.gpu
def test_plain_run_dumps_the_last_timed_step(tmp_path):
    """A plain run times exactly --steps steps, runs no other leg, and writes what
    its last timed step returned: the same arrays as an eager rollout of the same
    seeded envs stepped as often as the bench steps them (warm-up, one untimed
    replay of the window's graph, the rehearsals, the window)."""
    import bench
    from gym_pybullet_drones_amd.envs import QuadSwarm
    from gym_pybullet_drones_amd.envs.swarm import grid_layout
    E, D, steps, warmup, rehearse = 96, 8, 5, 2, 1
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", str(warmup), "--envs", str(E), "--rehearse", str(rehearse),
                        "--dump-outputs", str(tmp_path / "dump")], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    line = json.loads(lines[0])
    assert line["steps"] == steps and line["warmup"] == warmup and line["full"] is False
    assert line["unit"] == "agent-steps/s" and line["dtype"] == "f32" and line["higher_is_better"] is True
    assert line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(E * D * steps / (line["ms_per_step"] * 1e-3 * steps), rel=1e-9)
    for k in ("cpu_baseline", "fp64", "pyb", "mappo", "mappo_t32", "mappo_configs", "mappo_rank_shapes", "configs"):
        assert line[k] is None, k
    assert sorted(os.listdir(tmp_path / "dump")) == sorted(f"{k}.npy" for k in NAMES)

    sw = QuadSwarm("multihover", num_envs=E, num_drones=D, act="one_d_pid", precision=4, initial_xyzs=grid_layout(D))
    sw.reset(0)
    bench.stagger_episodes(sw, "multihover")
    acts = torch.empty((E, D, sw.act_dim), dtype=torch.float32, device=sw.device)
    truncated = 0
    for _ in range(warmup + steps * (1 + rehearse + 1)):
        r = sw.step(None, actions_out=acts)
        truncated += int(r.truncated.sum())
    torch.cuda.synchronize()
    assert truncated > 0   # the staggered clocks: episodes ended (auto-reset) inside the rollout
    want = {"obs": r.obs, "reward": r.reward, "terminated": r.terminated, "truncated": r.truncated, "actions": acts}
    for k in NAMES:
        got = np.load(tmp_path / "dump" / f"{k}.npy")
        assert got.dtype == np.float32 and got.shape == tuple(want[k].shape)
        assert np.array_equal(got, want[k].cpu().numpy().astype(np.float32)), k
    sw.close()
