"""The multi-step kernel's deferred obs copy against single steps, as raw bytes.

On the fast obs path (csrc/step_fuse.h `obs_pipe_ok`) a step of a multi-step launch
leaves its obs rows in LDS and the next step of the launch copies them to HBM under
its own PID; the last step's rows go out after the loop.  This may not change a bit:
the reference in every case is the single-step path (`QuadSwarm.step`) on the same
GPU, which test_gpu_parity.py and test_gpu_tolerance.py pin to the oracle; every
output, every state block and the episode log are compared as bytes.  Case 5 holds
the fast substep to the same standard where some lanes of a wave take the exp map's
sin/cos branch (a branch-free form of that substep differed from single steps by
1 ulp there and was dropped).

 1. C3's shape at depth 32, 70 steps (32 + 32 + 6): 16 envs (two full waves, both on
    the fast path) and 9 envs (a full wave on it and a one-env wave on the general
    path, in one launch), envs truncated on the first, a middle and the last step of
    a launch and on consecutive steps, terminal obs requested.
 2. Launches of 1, 2 and 3 steps over 7 steps (the copy after the loop right after
    the first step; a reset on every step of a launch).
 3. Obs buffers that start 4 bytes off 16-byte alignment, on every step and on one
    step of a launch only: the launch takes the general path; same bytes.
 4. A launch whose odd steps have no obs buffer (through the C ABI: `step_many`
    itself gives every step one): the even steps' obs equal the reference, the odd
    steps' canary rows stay untouched.
 5. Body rates of 150 rad/s on the drones of env 0 and env 8 of 9 (u >= 0.0625 on
    those lanes only: some lanes of a wave on the sin/cos path, the others on the
    series), 3 steps at depth 3, DYN and PYB.
 6. A VEL case (A = 4, D = 8, 72-float rows: wider than the fast path takes) at
    depth 32: the general path, unchanged.
"""
import ctypes

import numpy as np
import pytest
import torch

from gym_pybullet_drones_amd import _lib as L
from gym_pybullet_drones_amd.envs.swarm import QuadSwarm, grid_layout

from test_gpu_step_fusion import BLOCKS, Outs, set_clocks
from test_gpu_step_trim import RUNS, raw

pytestmark = pytest.mark.gpu


def c3(num_envs, **kw):
    return dict(task="multihover", num_drones=8, num_envs=num_envs, act="one_d_pid", initial_xyzs=grid_layout(8), **kw)


def pair(cfg, depth, monkeypatch, clocks, prepare=None):
    monkeypatch.setenv("QS_MAX_FUSED_STEPS", str(depth))
    one, many = QuadSwarm(**cfg), QuadSwarm(**cfg)
    for sw in (one, many):
        sw.reset(3)
        if clocks:
            set_clocks(sw, clocks)
        if prepare:
            prepare(sw)
    return one, many


def same_bytes(one, many, o1, o2, skip_obs=()):
    torch.cuda.synchronize()
    for k in o1.bufs:
        a, b = o1.bufs[k], o2.bufs[k]
        if k == "obs" and skip_obs:
            keep = [j for j in range(o1.n) if j not in skip_obs]
            a, b = a[keep], b[keep]
        assert np.array_equal(raw(a), raw(b)), k
    for blk in BLOCKS:
        assert np.array_equal(raw(one.get_state(blk)), raw(many.get_state(blk))), f"state block {blk}"
    (ra, ta), (rb, tb) = one.episode_log(), many.episode_log()
    assert ta == tb and np.array_equal(raw(ra), raw(rb))
    assert one.reset_error() == 0 and many.reset_error() == 0


def run(cfg, depth, steps, monkeypatch, clocks, prepare=None, obs_of=None, expect_trunc=True):
    """`steps` single steps against one step_many call; obs_of(j, default) may replace step j's obs buffer
    of the multi-step run (its content is copied back into the default buffer for the comparison)."""
    one, many = pair(cfg, depth, monkeypatch, clocks, prepare)
    o1, o2 = Outs(one, steps), Outs(many, steps)
    for j in range(steps):
        one.step(None, **o1.kw(j))
    kws = [o2.kw(j) for j in range(steps)]
    moved = {}
    if obs_of:
        for j in range(steps):
            alt = obs_of(j, kws[j]["obs"])
            if alt is not None:
                moved[j] = alt
                kws[j]["obs"] = alt
    many.step_many(kws)
    torch.cuda.synchronize()
    for j, alt in moved.items():
        o2.bufs["obs"][j].copy_(alt)
    if expect_trunc:
        assert o1.bufs["truncated"].sum().item() > 0
        assert o1.bufs["terminal_obs"].abs().sum().item() > 0
    same_bytes(one, many, o1, o2)
    one.close()
    many.close()


@pytest.mark.parametrize("num_envs", [16, 9], ids=["two_full_waves", "full_wave_and_one_env"])
def test_depth_32_full_and_partial_waves(num_envs, monkeypatch):
    steps, trunc_at = RUNS[32]
    run(c3(num_envs), 32, steps, monkeypatch, trunc_at)


@pytest.mark.parametrize("depth", [1, 2, 3])
def test_short_launches(depth, monkeypatch):
    run(c3(16), depth, 7, monkeypatch, (0, 1, 2, 3, 4, 5, 6))


def off_by_one_float(like, n):
    """n obs buffers whose rows start 4 bytes past a 16-byte boundary: views one float into larger rows."""
    E, D, O = like.shape
    assert (E * D * O) % 4 == 0
    big = torch.zeros((n, E * D * O + 4), device=like.device)
    views = [big[j, 1:1 + E * D * O].view(E, D, O) for j in range(n)]
    assert all(v.is_contiguous() and v.data_ptr() % 16 == 4 for v in views)
    return views


@pytest.mark.parametrize("which", ["every_step", "one_step"])
def test_misaligned_obs_takes_the_general_path(which, monkeypatch):
    steps, trunc_at = 37, RUNS[32][1]   # launches of 32 + 5 steps
    holder = {}

    def obs_of(j, default):
        assert default.data_ptr() % 16 == 0
        if "v" not in holder:
            holder["v"] = off_by_one_float(default, steps)
        return holder["v"][j] if which == "every_step" or j == 5 else None

    run(c3(16), 32, steps, monkeypatch, trunc_at, obs_of=obs_of)


def test_steps_without_obs_leave_nothing_pending(monkeypatch):
    steps, trunc_at = 12, (0, 3, 4, 5, 8, 11)
    one, many = pair(c3(16), 32, monkeypatch, trunc_at)
    o1, o2 = Outs(one, steps), Outs(many, steps)
    o2.bufs["obs"].fill_(-7.0)   # canary
    for j in range(steps):
        one.step(None, **o1.kw(j))
    recs = [many._step_out(**o2.kw(j))[0] for j in range(steps)]
    for j in range(1, steps, 2):
        recs[j].obs = None
    arr = (L.QsStepOut * steps)(*recs)
    L.check(many.lib.qs_step_many(many._h, steps, arr, many._stream()), "qs_step_many")
    torch.cuda.synchronize()
    assert o1.bufs["truncated"].sum().item() > 0
    obs = o2.bufs["obs"].cpu().numpy()
    for j in range(1, steps, 2):
        assert (obs[j] == -7.0).all(), j
    same_bytes(one, many, o1, o2, skip_obs=set(range(1, steps, 2)))
    one.close()
    many.close()


@pytest.mark.parametrize("physics", ["dyn", "pyb"])
def test_some_lanes_on_the_sincos_branch(physics, monkeypatch):
    def spin(sw):
        agent = sw.get_state(L.STATE_AGENT)
        D = sw.num_drones
        for e in (0, 8):
            agent[L.F_RPY_RATES, e * D:(e + 1) * D] = 150.0   # about x: u = (150 / 480)^2 = 0.098 >= 0.0625
        sw.set_state(L.STATE_AGENT, agent)

    run(c3(9, physics=physics), 3, 3, monkeypatch, None, prepare=spin, expect_trunc=False)


def test_vel_rows_keep_the_general_path(monkeypatch):
    steps, trunc_at = RUNS[32]
    cfg = dict(task="multihover", num_drones=8, num_envs=16, act="vel", initial_xyzs=grid_layout(8))
    run(cfg, 32, steps, monkeypatch, trunc_at)
