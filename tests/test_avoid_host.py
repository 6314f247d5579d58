"""csrc/avoid_sizes.h holds the plain arithmetic of the separation and obstacle terms
(qs_avoid_score / qs_avoid_mppi_set / qs_avoid_cem_set): every refusal at its boundary values
and in the order of the checks, the table's bytes, the two switches and the overlap test of
cost_agent.  tests/avoid_check.cpp exercises them as a stand-alone program built with the
address and undefined-behaviour sanitizers (no GPU, nothing loaded into Python)."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_avoid_arithmetic_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or "c++"
    exe = tmp_path / "avoid_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "marl-gym-pybullet-drones_amd", "csrc"),
                    os.path.join(ROOT, "tests", "avoid_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "avoid_sizes ok" in out.stdout


def test_reset_layouts_put_pairs_on_both_sides_of_the_radius():
    """The CPU check behind tests/avoid_case.py: with the grid layouts and their +-0.25 m reset
    noise, the share of ordered pairs inside the test spec's radius (heights scaled as the spec
    scales them) leaves each branch of the hinge at least a tenth, at the seeds the GPU tests use."""
    import numpy as np
    import qs_oracle
    from avoid_case import CONFIGS, DEFAULT_SEED, SEEDS, SEP_RADIUS, SEP_Z_SCALE
    shares = {}
    for name, cfg in CONFIGS.items():
        if cfg["task"] != "multihover":
            continue
        E, D = cfg["num_envs"], cfg["num_drones"]
        sim = qs_oracle.OracleSim(task="multihover", num_envs=E, num_drones=D, act=cfg["act"],
                                  initial_xyzs=cfg["initial_xyzs"])
        p = np.asarray(sim.reset(SEEDS.get(name, DEFAULT_SEED)))[..., :3].reshape(E, D, 3).astype(np.float64)
        inside = total = 0
        for d in range(D):
            for i in range(D):
                if i != d:
                    dx, dy = p[:, d, 0] - p[:, i, 0], p[:, d, 1] - p[:, i, 1]
                    dz = (p[:, d, 2] - p[:, i, 2]) * SEP_Z_SCALE
                    inside += int((SEP_RADIUS * SEP_RADIUS - ((dx * dx + dy * dy) + dz * dz) > 0).sum())
                    total += E
        shares[name] = inside / total
    print(shares)
    assert all(0.1 <= s <= 0.9 for s in shares.values()), shares
    assert round(shares["mh_d2_onedpid"], 2) == 0.81
