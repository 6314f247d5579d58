"""Multi-step launches over caller-supplied actions equal single steps, byte for byte.

`QuadSwarm.step_many(outs, actions=…)` (qs_step_seq) runs several control steps to
a launch and reads step j's actions from the buffer the caller names.  The
reference in every case is a twin handle stepped with eager
`QuadSwarm.step(actions[j], …)`: the single-step path, which
tests/test_gpu_parity.py pins to the oracle.  The multi-step launch does the single
step's operations on the same values and only takes the action row from LDS, so
outputs, the four state blocks and the episode log are compared as raw bytes.

 1. Shapes and instances: 37 steps at depth 16 (launches of 16 + 16 + 5), truncations
    and auto-resets on the first, a middle and the last step of a launch.
 2. Depths: the default 32 with 70 steps (32 + 32 + 6), 1 / 2 / 3 steps, depth 1.
 3. Pointer shapes: one (n, E, D, A) tensor or a list; action pointers that are
    only 4-byte aligned, all of them or one step of a launch.
 4. Aliasing between the actions and the outputs of other steps (the launch is cut).
 5. A layout that runs the deferred reset search after each step (single steps).
 6. `actions=None`: today's `step_many`.
 7. Refusals, none of which steps the envs.
 8. `SwarmVecEnv.rollout_t` against `step_t` in a loop.
"""
import ctypes

import numpy as np
import pytest
import torch

from gym_pybullet_drones_amd import _lib as L
from gym_pybullet_drones_amd.envs.swarm import QuadSwarm, grid_layout
from gym_pybullet_drones_amd.vec_env.vec_env import SwarmVecEnv

pytestmark = pytest.mark.gpu

STEPS = 37   # depth 16: launches of 16 + 16 + 5 steps
# the step (0-based) at which env e is truncated, e mod 9: first / middle / last step
# of each launch, and neighbours (15, 16, 17: consecutive steps, envs of one wave)
TRUNC_AT = (0, 7, 15, 16, 17, 24, 31, 32, 36)
# the same for 70 steps at depth 32 (launches of 32 + 32 + 6)
TRUNC_AT_70 = (0, 15, 31, 32, 33, 48, 63, 64, 69)

CONFIGS = {
    # A = 1, the fast obs path, a partial last wave
    "mh_d8_onedpid_dyn_f32": dict(task="multihover", num_drones=8, num_envs=21, act="one_d_pid",
                                  initial_xyzs=grid_layout(8)),
    "mh_d8_onedpid_dyn_f64": dict(task="multihover", num_drones=8, num_envs=5, act="one_d_pid",
                                  initial_xyzs=grid_layout(8), precision=8),
    # A = 4, an idle lane in every wave
    "mh_d3_vel_pyb": dict(task="multihover", num_drones=3, num_envs=22, act="vel", physics="pyb",
                          initial_xyzs=grid_layout(3)),
    "spiral_d5_vel": dict(task="spiral", num_drones=5, num_envs=13, act="vel"),
    # a run-time control frequency: the action history lives in LDS, not in registers
    "mh_d8_onedpid_60hz": dict(task="multihover", num_drones=8, num_envs=21, act="one_d_pid",
                               initial_xyzs=grid_layout(8), ctrl_freq=60),
    # A = 3
    "mh_d4_pid_grid": dict(task="multihover", num_drones=4, num_envs=17, act="pid", initial_xyzs=grid_layout(4)),
    "cf2p_d2_rpm": dict(task="multihover", num_drones=2, num_envs=40, act="rpm", drone_model="cf2p",
                        initial_xyzs=grid_layout(2)),
    # the MARL family: qs_step_seq takes single steps for it (its multi-step kernels round the
    # env reward 1 ulp apart from the single step's), through the same call
    "flock_d4_rpm": dict(task="flock", num_drones=4, num_envs=16, act="rpm"),
}
BLOCKS = (L.STATE_AGENT, L.STATE_ENV, L.STATE_HISTORY, L.STATE_EP_RETURN)
C3_SMALL = CONFIGS["mh_d8_onedpid_dyn_f32"]
QS_E_INVALID, QS_E_STATE = -1, -4


def set_clocks(sw, trunc_at):
    """Episode clocks such that env e is truncated (and auto-reset) in step
    trunc_at[e mod len]: the step that sees step_counter = limit + substeps."""
    E, S = sw.num_envs, sw.substeps
    limit = int(round(sw.episode_len_sec * sw.pyb_freq))
    env = sw.get_state(L.STATE_ENV).clone()
    at = torch.tensor([trunc_at[e % len(trunc_at)] for e in range(E)], dtype=torch.int32, device=env.device)
    env[L.E_STEP_COUNTER] = limit + S - S * at
    env[L.E_EP_LEN] = (limit + S - S * at) // S
    sw.set_state(L.STATE_ENV, env)


def ground(sw, env=3):
    """Drone 0 of `env` 1 cm above the ground: a MultiHover env crashes (z < 0.03) in the first step."""
    st = sw.get_state(L.STATE_AGENT).clone()
    st[L.F_POS + 2, env * sw.num_drones] = 0.01
    sw.set_state(L.STATE_AGENT, st)


def twins(cfg, seed=3, clocks=TRUNC_AT, n=2):
    out = [QuadSwarm(**cfg) for _ in range(n)]
    for sw in out:
        sw.reset(seed)
        if clocks:
            set_clocks(sw, clocks)
        if sw.task == "multihover":
            ground(sw)
    return out


def make_actions(sw, n, seed=5):
    """(n, E, D, A) actions, uniform in [-1.5, 1.5] (past every clip) from a seeded CPU
    generator, with an all-zero row, a row of -0.0 and rows of exactly +1 and -1 in known
    lanes of the first, a middle and the last step of the launches."""
    E, D, A = sw.num_envs, sw.num_drones, sw.act_dim
    gen = torch.Generator(device="cpu").manual_seed(seed)
    a = torch.rand((n, E, D, A), generator=gen) * 3 - 1.5
    for j in sorted({0, 1, 15, 16, n // 2, n - 1}):
        if j < n:
            a[j, 0, 0, :] = 0.0
            a[j, 1 % E, D - 1, :] = -0.0
            a[j, 2 % E, 0, :] = 1.0
            a[j, 2 % E, D - 1, :] = -1.0
    assert torch.signbit(a[0, 1 % E, D - 1]).all() and not torch.isnan(a).any()
    return a.to(sw.device)


class Outs:
    """`n` sets of step output buffers (zeroed: terminal_obs rows are written for done envs only)."""

    def __init__(self, sw, n):
        E, D, O, A = sw.num_envs, sw.num_drones, sw.obs_dim, sw.act_dim
        kw = dict(device=sw.device)
        self.n = n
        self.bufs = dict(obs=torch.zeros((n, E, D, O), **kw), reward=torch.zeros((n, E), dtype=sw.rdtype, **kw),
                         terminated=torch.zeros((n, E), dtype=torch.uint8, **kw),
                         truncated=torch.zeros((n, E), dtype=torch.uint8, **kw),
                         terminal_obs=torch.zeros((n, E, D, O), **kw),
                         reasons=torch.zeros((n, E, D), dtype=torch.uint8, **kw),
                         actions_out=torch.zeros((n, E, D, A), **kw))

    def kw(self, j):
        return {k: v[j % self.n] for k, v in self.bufs.items()}

    def kws(self, n=None):
        return [self.kw(j) for j in range(self.n if n is None else n)]


def same_bytes(a, b, what):
    a, b = a.cpu().numpy() if isinstance(a, torch.Tensor) else a, b.cpu().numpy() if isinstance(b, torch.Tensor) else b
    assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), what


def same_outputs(a, b):
    for k in a.bufs:
        same_bytes(a.bufs[k], b.bufs[k], k)


def same_state(a, b):
    torch.cuda.synchronize()
    for blk in BLOCKS:
        same_bytes(a.get_state(blk), b.get_state(blk), f"state block {blk}")
    (ra, ta), (rb, tb) = a.episode_log(), b.episode_log()
    assert ta == tb
    same_bytes(ra, rb, "episode log")


def eager(sw, acts, kws):
    for a, kw in zip(acts, kws):
        sw.step(a, **kw)


def close(*sws):
    for sw in sws:
        sw.close()


# ------------------------------------------------------------ 1. shapes and instances
@pytest.mark.parametrize("name", list(CONFIGS))
def test_sequence_equals_single_steps(name, monkeypatch):
    monkeypatch.setenv("QS_MAX_FUSED_STEPS", "16")
    one, many = twins(CONFIGS[name])
    acts = make_actions(one, STEPS)
    o1, o2 = Outs(one, STEPS), Outs(many, STEPS)
    eager(one, acts, o1.kws())
    res = many.step_many(o2.kws(), actions=acts)
    assert len(res) == STEPS and res[5].obs.data_ptr() == o2.bufs["obs"][5].data_ptr()
    torch.cuda.synchronize()
    assert o1.bufs["truncated"].sum().item() > 0
    if one.task == "multihover":
        assert o1.bufs["terminated"].sum().item() > 0
    same_bytes(o2.bufs["actions_out"], acts, "actions_out is the actions, -0.0 included")
    same_outputs(o1, o2)
    same_state(one, many)
    assert one.reset_error() == 0 and many.reset_error() == 0
    close(one, many)


# ------------------------------------------------------------------------ 2. depths
@pytest.mark.parametrize("depth,n", [(None, 70), (None, 1), (None, 2), (None, 3), ("1", 5)])
def test_depths(depth, n, monkeypatch):
    if depth is None:
        monkeypatch.delenv("QS_MAX_FUSED_STEPS", raising=False)
    else:
        monkeypatch.setenv("QS_MAX_FUSED_STEPS", depth)
    one, many = twins(C3_SMALL, clocks=TRUNC_AT_70 if n == 70 else (0, 1, 2, 4))
    acts = make_actions(one, n)
    o1, o2 = Outs(one, n), Outs(many, n)
    eager(one, acts, o1.kws())
    many.step_many(o2.kws(), actions=acts)
    torch.cuda.synchronize()
    assert o1.bufs["truncated"].sum().item() > 0 and o1.bufs["terminated"].sum().item() > 0
    same_outputs(o1, o2)
    same_state(one, many)
    close(one, many)


# ---------------------------------------------------------------- 3. pointer shapes
def offset_by_one_float(t):
    """A copy of `t` whose storage starts one float past an allocation: 4-byte aligned only."""
    buf = torch.zeros(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


@pytest.mark.parametrize("name", ["mh_d8_onedpid_dyn_f32", "mh_d3_vel_pyb"])   # A = 1, A = 4
def test_tensor_list_and_unaligned_actions(name, monkeypatch):
    monkeypatch.setenv("QS_MAX_FUSED_STEPS", "16")
    n = 20
    one, as_tensor, as_list, all_off, one_off = twins(CONFIGS[name], n=5)
    acts = make_actions(one, n)
    outs = [Outs(sw, n) for sw in (one, as_tensor, as_list, all_off, one_off)]
    eager(one, acts, outs[0].kws())
    as_tensor.step_many(outs[1].kws(), actions=acts)
    as_list.step_many(outs[2].kws(), actions=[acts[j].clone() for j in range(n)])
    all_off.step_many(outs[3].kws(), actions=[offset_by_one_float(acts[j]) for j in range(n)])
    one_off.step_many(outs[4].kws(), actions=[offset_by_one_float(acts[j]) if j == 5 else acts[j] for j in range(n)])
    torch.cuda.synchronize()
    assert outs[0].bufs["truncated"].sum().item() > 0
    for sw, o in zip((as_tensor, as_list, all_off, one_off), outs[1:]):
        same_outputs(outs[0], o)
        same_state(one, sw)
    close(one, as_tensor, as_list, all_off, one_off)


# ------------------------------------------------------------------------ 4. aliasing
def alias_same_buffer(sw, n, acts):
    o = Outs(sw, n)
    return [acts[0]] * n, o.kws(), o.bufs


def alias_actions_out_feeds_next(sw, n, acts):
    o = Outs(sw, n)
    return [acts[0]] + [o.bufs["actions_out"][j] for j in range(n - 1)], o.kws(), o.bufs


def alias_obs_feeds_next(sw, n, acts):
    o = Outs(sw, n)
    NA, shape = sw.num_agents * sw.act_dim, acts[0].shape
    return [acts[0]] + [o.bufs["obs"][j].view(-1)[:NA].view(shape) for j in range(n - 1)], o.kws(), o.bufs


def alias_reward_in_later_actions(sw, n, acts):
    """Step j's reward goes to the head of the actions of step j + 2."""
    o = Outs(sw, n)
    mine = acts.clone()
    kws = o.kws()
    for j in range(n - 2):
        kws[j]["reward"] = mine[j + 2].view(-1)[:sw.num_envs]
    return mine, kws, dict(o.bufs, actions=mine)


@pytest.mark.parametrize("build", [alias_same_buffer, alias_actions_out_feeds_next, alias_obs_feeds_next,
                                   alias_reward_in_later_actions])
def test_aliased_actions_equal_single_steps(build, monkeypatch):
    monkeypatch.setenv("QS_MAX_FUSED_STEPS", "16")
    n = 12
    one, many = twins(C3_SMALL, clocks=(0, 3, 6, 7, 11))
    assert one.rdtype == torch.float32
    acts = make_actions(one, n)
    a1, k1, t1 = build(one, n, acts)
    a2, k2, t2 = build(many, n, acts)
    eager(one, a1, k1)
    many.step_many(k2, actions=a2)
    torch.cuda.synchronize()
    assert t1["truncated"].sum().item() > 0
    for k in t1:
        same_bytes(t1[k], t2[k], k)
    same_state(one, many)
    close(one, many)


# ------------------------------------------------------- 5. deferred reset search layout
def test_deferred_reset_search_layout_takes_single_steps(monkeypatch):
    """The reference's diagonal layout (reset draws can be rejected: the search launch
    follows each step), C2's shape at 16 envs."""
    monkeypatch.delenv("QS_MAX_FUSED_STEPS", raising=False)
    n = 12
    one, many = twins(dict(task="multihover", num_drones=4, num_envs=16, act="rpm"), clocks=(0, 3, 6, 7, 11))
    acts = make_actions(one, n)
    o1, o2 = Outs(one, n), Outs(many, n)
    eager(one, acts, o1.kws())
    many.step_many(o2.kws(), actions=acts)
    torch.cuda.synchronize()
    assert o1.bufs["truncated"].sum().item() > 0
    same_outputs(o1, o2)
    same_state(one, many)
    assert one.reset_error() == 0 and many.reset_error() == 0
    close(one, many)


# ------------------------------------------------------------------ 6. actions=None
def test_no_actions_is_step_many(monkeypatch):
    monkeypatch.setenv("QS_MAX_FUSED_STEPS", "16")
    n = 20
    plain, kw_none, c_null = twins(C3_SMALL, n=3)
    o = [Outs(sw, n) for sw in (plain, kw_none, c_null)]
    plain.step_many(o[0].kws())
    kw_none.step_many(o[1].kws(), actions=None)
    recs = [c_null._step_out(**kw) for kw in o[2].kws()]
    arr = (L.QsStepOut * n)(*[so for so, _ in recs])
    L.check(c_null.lib.qs_step_seq(c_null._h, n, None, arr, c_null._stream()), "qs_step_seq")
    torch.cuda.synchronize()
    assert o[0].bufs["truncated"].sum().item() > 0
    for sw, oo in ((kw_none, o[1]), (c_null, o[2])):
        same_outputs(o[0], oo)
        same_state(plain, sw)
    close(plain, kw_none, c_null)


# ---------------------------------------------------------------------- 7. refusals
def test_refusals_step_nothing():
    sw = QuadSwarm(**C3_SMALL)
    n = 4
    o = Outs(sw, n)
    acts = make_actions(sw, n)
    with pytest.raises(L.QuadSwarmError, match="rc=-4"):   # QS_E_STATE: before reset
        sw.step_many(o.kws(), actions=acts)
    sw.reset(3)
    before = [sw.get_state(blk).cpu().numpy().tobytes() for blk in BLOCKS]
    with pytest.raises(ValueError):
        sw.step_many(o.kws(), actions=[acts[0], None, acts[2], acts[3]])
    with pytest.raises(ValueError):
        sw.step_many(o.kws(), actions=acts.double())
    with pytest.raises(ValueError):
        sw.step_many(o.kws(), actions=torch.cat([acts, acts], dim=3))
    with pytest.raises(ValueError):
        sw.step_many(o.kws(), actions=acts.cpu())
    with pytest.raises(ValueError):
        sw.step_many(o.kws(), actions=acts[:3])
    with pytest.raises(ValueError):
        sw.step_many(o.kws(), actions=[acts[0]] * 3)
    # the C entry itself: a NULL among the pointers, n < 0, outs missing
    recs = [sw._step_out(**kw) for kw in o.kws()]
    arr = (L.QsStepOut * n)(*[so for so, _ in recs])
    ptrs = (ctypes.c_void_p * n)(acts[0].data_ptr(), acts[1].data_ptr(), None, acts[3].data_ptr())
    assert sw.lib.qs_step_seq(sw._h, n, ptrs, arr, sw._stream()) == QS_E_INVALID
    assert b"actions[2]" in sw.lib.qs_last_error()
    ptrs = (ctypes.c_void_p * n)(*[acts[j].data_ptr() for j in range(n)])
    assert sw.lib.qs_step_seq(sw._h, -1, ptrs, arr, sw._stream()) == QS_E_INVALID
    assert sw.lib.qs_step_seq(sw._h, n, ptrs, None, sw._stream()) == QS_E_INVALID
    assert sw.lib.qs_step_seq(sw._h, 0, ptrs, arr, sw._stream()) == 0   # n == 0: nothing to do
    assert sw.step_many([], actions=[]) == []
    torch.cuda.synchronize()
    assert [sw.get_state(blk).cpu().numpy().tobytes() for blk in BLOCKS] == before
    assert o.bufs["obs"].abs().sum().item() == 0
    sw.close()


# --------------------------------------------------------------------- 8. rollout_t
def test_rollout_t_matches_step_t(monkeypatch):
    monkeypatch.setenv("QS_MAX_FUSED_STEPS", "16")
    n = 20
    a, b = (SwarmVecEnv(seed=3, **C3_SMALL) for _ in range(2))
    for v in (a, b):
        v.reset_t()
        set_clocks(v.swarm, (0, 7, 15, 16, 19, 20, 27, 35, 39))
        ground(v.swarm)
    ptrs = None
    for rnd in range(2):
        acts = make_actions(a.swarm, n, seed=5 + rnd)
        want = []
        for j in range(n):
            r = a.step_t(acts[j])
            want.append([t.clone() for t in (r.obs, r.reward, r.terminated, r.truncated)])
        got = b.rollout_t(acts)
        assert len(got) == 4 and got[0].shape == (n, a.num_envs, a.swarm.num_drones, a.swarm.obs_dim)
        for i, what in enumerate(("obs", "reward", "terminated", "truncated")):
            same_bytes(torch.stack([w[i] for w in want]), got[i], what)
        assert got[3].sum().item() > 0
        if ptrs is not None:
            assert [t.data_ptr() for t in got] == ptrs   # the same shape again: the same buffers
        ptrs = [t.data_ptr() for t in got]
    same_state(a.swarm, b.swarm)
    with pytest.raises(ValueError):
        b.rollout_t(acts[0])
    a.close()
    b.close()
