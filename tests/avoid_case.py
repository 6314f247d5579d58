"""The shared configurations, spec and float64 restatement of tests/test_gpu_avoid.py and
tests/test_gpu_avoid_planner.py (a plain module, not a conftest)."""
import numpy as np
import torch

from gym_pybullet_drones_amd.envs.swarm import avoid_spec, grid_layout
from track_case import CONFIGS as TRACK_CONFIGS
from track_case import cost_reference  # noqa: F401  (the tracking loop this one is held against with every switch off)

# The seven shapes of the tracking tests plus the smallest env that has a pair: D = 2 (wave
# reduction over two lanes, 32 envs a workgroup).
CONFIGS = dict(TRACK_CONFIGS)
CONFIGS["mh_d2_onedpid"] = dict(task="multihover", num_drones=2, num_envs=21, act="one_d_pid",
                                initial_xyzs=grid_layout(2))

# The reset seed of a configuration's swarms (tests/test_gpu_step_score.py `prepared`; its default
# elsewhere).  The D = 2 config has one pair an env and 21 envs, and one_d_pid never moves a drone
# sideways, so the seed's reset draw decides the split: with seed 3, 20 of the 21 pairs start inside
# 1.2 m; with seed 1, 17 (0.81), which leaves both branches of the hinge more than a tenth
# (tests/test_avoid_host.py holds that on the CPU oracle's reset).
SEEDS = {"mh_d2_onedpid": 1}
DEFAULT_SEED = 3

# The grid layouts put neighbours 1 m apart and a reset adds +-0.25 m an axis: a radius of
# 1.2 m has neighbours inside and diagonal or farther pairs outside.
SEP_RADIUS, SEP_WEIGHT, SEP_Z_SCALE = 1.2, 0.7, 0.5
# Spiral starts its D drones on a circle of radius 0.4 m at z = 0.3 (D = 5: neighbours
# 0.47 m apart, the others 0.76 m): a radius between the two.
SPIRAL_SEP_RADIUS = 0.6

# Rows: centre (3), axis weights (3), radius, weight.
OBSTACLES = (
    (0.0, 0.0, 0.5, 1.0, 1.0, 1.0, 0.9, 1.5),     # a sphere over the grid's centre
    (0.5, -0.5, 0.0, 1.0, 1.0, 0.0, 0.6, 0.8),    # a vertical cylinder
    (0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.45, 2.0),    # a floor slab: below z = 0.45
    (0.0, 0.0, 0.5, 1.0, 1.0, 1.0, 2.0, 0.0),     # weight 0: inside for most, contributes nothing
)
SPIRAL_OBSTACLES = (
    (0.0, 0.0, 0.3, 1.0, 1.0, 1.0, 0.5, 1.5),     # a sphere over the circle's centre: every drone starts inside
    (0.4, 0.0, 0.0, 1.0, 1.0, 0.0, 0.3, 0.8),     # a vertical cylinder round drone 0's start
    (0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.45, 2.0),    # the floor slab
    (0.0, 0.0, 0.3, 1.0, 1.0, 1.0, 2.0, 0.0),     # weight 0
)


def numbers_for(cfg):
    """(obstacle rows, sep_radius) of the test spec for a configuration."""
    if cfg["task"] == "spiral":
        return SPIRAL_OBSTACLES, SPIRAL_SEP_RADIUS
    return OBSTACLES, SEP_RADIUS


def many_rows(rows, M=16):
    """M rows: the given ones, then shifted and shrunk copies of them (all different)."""
    out = [tuple(r) for r in rows]
    k = 0
    while len(out) < M:
        r = rows[k % len(rows)]
        s = 1 + k // len(rows)
        out.append((r[0] + 0.3 * s, r[1] - 0.2 * s, r[2], r[3], r[4], r[5], r[6] * (1 + 0.1 * s), r[7] * 0.5))
        k += 1
    return tuple(out[:M])


def make_avoid(sw, rows=None, sep_radius=None, sep_weight=SEP_WEIGHT, sep_z_scale=SEP_Z_SCALE, off=False):
    """(spec, keep) of `avoid_spec` on `sw` (off: every switch off, no table)."""
    if off:
        return avoid_spec()
    cfg_rows, cfg_radius = numbers_for(dict(task=sw.task))
    rows = cfg_rows if rows is None else rows
    table = None
    if len(rows) > 0:
        table = torch.tensor(rows, dtype=torch.float32).reshape(-1, 8).to(sw.device).contiguous()
    return avoid_spec(table, cfg_radius if sep_radius is None else sep_radius, sep_weight, sep_z_scale)


def avoid_reference(obs, terminal_obs, terminated, truncated, actions_out, track=None, obstacles=(), sep_radius=0.0,
                    sep_weight=0.0, sep_z_scale=1.0):
    """(cost_agent (C, E, D) float64, stats) from one launch's outputs: the loop of
    include/quadswarm.h (qs_avoid_score) in NumPy float64, every subtraction, product and
    sum an operation of its own (NumPy does not fuse), i, m, k and a ascending.

    track: None or dict(ref, base, q, r, terminal) as `track_case.cost_reference` takes
    them.  obstacles: M rows of eight numbers (float32 in the table: widened, not the
    literals).  stats counts, over the steps that enter the sum: ordered pairs inside and
    outside the radius, and the drone-steps at which each obstacle row adds a term > 0."""
    n, C, E, D = obs.shape[:4]
    A = actions_out.shape[-1]
    f = lambda v: np.asarray(v, np.float32).astype(np.float64)   # noqa: E731
    tab = f(obstacles).reshape(-1, 8)
    M = tab.shape[0]
    sr, sw_, zs = f(sep_radius), f(sep_weight), f(sep_z_scale)
    sep_on = sr != 0 and sw_ != 0 and D > 1
    r2 = sr * sr
    if track is not None:
        rows = track["ref"].shape[0]
        base = np.zeros(E, np.int64) if track["base"] is None else track["base"].astype(np.int64)
        q, r, terminal = f(track["q"]), f(track["r"]), f(track["terminal"])
    cost = np.zeros((C, E, D), np.float64)
    live = np.ones((C, E), bool)
    env = np.arange(E)
    stats = dict(inside=0, outside=0, row_hits=np.zeros(M, np.int64), drone_steps=0)
    for j in range(n):
        done = (terminated[j] != 0) | (truncated[j] != 0)
        x = np.where(done[:, :, None, None], terminal_obs[j][..., :12], obs[j][..., :12])
        assert x.dtype == np.float32
        x = x.astype(np.float64)
        s = np.zeros((C, E, D), np.float64)
        if track is not None:
            row = np.clip(base + j, 0, rows - 1)
            target = track["ref"][row, env].astype(np.float64)[None]
            for k in range(12):
                dd = x[..., k] - target[..., k]
                s = s + q[k] * (dd * dd)
            if j == n - 1:
                s = terminal * s
            u = actions_out[j].astype(np.float64)
            for a in range(A):
                s = s + r[a] * (u[..., a] * u[..., a])
        p = x[..., :3]                                            # (C, E, D, 3)
        if sep_on:
            s_sep = np.zeros((C, E, D), np.float64)
            for d in range(D):
                acc = np.zeros((C, E), np.float64)
                for i in range(D):
                    if i == d:
                        continue
                    dx = p[:, :, d, 0] - p[:, :, i, 0]
                    dy = p[:, :, d, 1] - p[:, :, i, 1]
                    dz = (p[:, :, d, 2] - p[:, :, i, 2]) * zs
                    d2 = (dx * dx + dy * dy) + dz * dz
                    g = r2 - d2
                    hit = g > 0                                    # a NaN compares false
                    acc = np.where(hit, acc + g * g, acc)
                    stats["inside"] += int((hit & live).sum())
                    stats["outside"] += int((~hit & live).sum())
                s_sep[:, :, d] = acc
            s = s + sw_ * s_sep
        if M > 0:
            s_obs = np.zeros((C, E, D), np.float64)
            for m in range(M):
                c, ax, radius, weight = tab[m, 0:3], tab[m, 3:6], tab[m, 6], tab[m, 7]
                d2 = np.zeros((C, E, D), np.float64)
                for k in range(3):
                    dd = p[..., k] - c[k]
                    d2 = d2 + ax[k] * (dd * dd)
                g = radius * radius - d2
                hit = g > 0
                term = weight * (g * g)
                s_obs = np.where(hit, s_obs + term, s_obs)
                stats["row_hits"][m] += int((hit & (term > 0) & live[:, :, None]).sum())
            s = s + s_obs
        stats["drone_steps"] += int(live.sum()) * D
        cost = np.where(live[:, :, None], cost + s, cost)
        live = live & ~done
    return cost, stats
