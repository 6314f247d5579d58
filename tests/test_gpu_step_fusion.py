"""Multi-step launches of the step kernel equal single steps, bit for bit.

The reference in every case is the single-step path (`QuadSwarm.step`, eager) on
the same GPU, which tests/test_gpu_parity.py and test_gpu_tolerance.py pin to the
oracle.  A multi-step launch does the same operations in the same order on the
same values and only keeps them on-chip between its steps, so every comparison
is `np.array_equal`: no tolerance.

 1. `step_many` (qs_step_many) against `step` × 37 at depth 16 (launches of
    16 + 16 + 5 steps), with truncations and auto-resets on the first, a middle
    and the last step of a launch and in consecutive steps of one wave.
 2. `step(None, …)` calls captured into a `torch.cuda.graph` (qs_step grows the
    capture's kernel node instead of launching) against eager steps.
 3. The captures that must not be joined: one output buffer for every step,
    policy actions, another call on the handle between two steps, a layout that
    runs the deferred reset search after each step.
"""
import numpy as np
import pytest
import torch

from gym_pybullet_drones_amd import _lib as L
from gym_pybullet_drones_amd.envs.swarm import QuadSwarm, grid_layout

pytestmark = pytest.mark.gpu

STEPS = 37   # depth 16: launches of 16 + 16 + 5 steps
# the step (0-based) at which env e is truncated, e mod 9: first / middle / last step
# of each launch, and neighbours (15, 16, 17: consecutive steps, envs of one wave)
TRUNC_AT = (0, 7, 15, 16, 17, 24, 31, 32, 36)

CONFIGS = {
    "mh_d8_onedpid_dyn_f32": dict(task="multihover", num_drones=8, num_envs=21, act="one_d_pid",
                                  initial_xyzs=grid_layout(8)),
    "mh_d8_onedpid_dyn_f64": dict(task="multihover", num_drones=8, num_envs=5, act="one_d_pid",
                                  initial_xyzs=grid_layout(8), precision=8),
    "mh_d3_vel_pyb": dict(task="multihover", num_drones=3, num_envs=22, act="vel", physics="pyb",
                          initial_xyzs=grid_layout(3)),
    "spiral_d5_vel": dict(task="spiral", num_drones=5, num_envs=13, act="vel"),
    # a run-time control frequency: the action history lives in LDS, not in registers
    "mh_d8_onedpid_60hz": dict(task="multihover", num_drones=8, num_envs=21, act="one_d_pid",
                               initial_xyzs=grid_layout(8), ctrl_freq=60),
    "cf2p_d2_rpm": dict(task="multihover", num_drones=2, num_envs=40, act="rpm", drone_model="cf2p",
                        initial_xyzs=grid_layout(2)),
}
BLOCKS = (L.STATE_AGENT, L.STATE_ENV, L.STATE_HISTORY, L.STATE_EP_RETURN)


def set_clocks(sw, trunc_at):
    """Episode clocks such that env e is truncated (and auto-reset) in step
    trunc_at[e mod len]: the step that sees step_counter = limit + substeps
    (truncation: step_counter / pyb_freq > episode_len_sec, on the counter before
    the step advances it)."""
    E, S = sw.num_envs, sw.substeps
    limit = int(round(sw.episode_len_sec * sw.pyb_freq))
    env = sw.get_state(L.STATE_ENV).clone()
    at = torch.tensor([trunc_at[e % len(trunc_at)] for e in range(E)], dtype=torch.int32, device=env.device)
    env[L.E_STEP_COUNTER] = limit + S - S * at
    env[L.E_EP_LEN] = (limit + S - S * at) // S
    sw.set_state(L.STATE_ENV, env)


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

    def numpy(self):
        return {k: v.cpu().numpy() for k, v in self.bufs.items()}


def same_outputs(a, b):
    a, b = a.numpy(), b.numpy()
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def same_state(a, b):
    torch.cuda.synchronize()
    for blk in BLOCKS:
        assert np.array_equal(a.get_state(blk).cpu().numpy(), b.get_state(blk).cpu().numpy()), f"state block {blk}"
    (ra, ta), (rb, tb) = a.episode_log(), b.episode_log()
    assert ta == tb and np.array_equal(ra, rb)


def twins(cfg, seed=3, clocks=TRUNC_AT):
    a, b = QuadSwarm(**cfg), QuadSwarm(**cfg)
    for sw in (a, b):
        sw.reset(seed)
        if clocks:
            set_clocks(sw, clocks)
    return a, b


@pytest.mark.parametrize("name", list(CONFIGS))
def test_step_many_equals_single_steps(name, monkeypatch):
    monkeypatch.setenv("QS_MAX_FUSED_STEPS", "16")
    one, many = twins(CONFIGS[name])
    o1, o2 = Outs(one, STEPS), Outs(many, STEPS)
    for j in range(STEPS):
        one.step(None, **o1.kw(j))
    res = many.step_many([o2.kw(j) for j in range(STEPS)])
    assert len(res) == STEPS and res[5].obs.data_ptr() == o2.bufs["obs"][5].data_ptr()
    torch.cuda.synchronize()
    assert o1.bufs["truncated"].sum().item() > 0
    same_outputs(o1, o2)
    same_state(one, many)
    assert one.reset_error() == 0 and many.reset_error() == 0
    one.close()
    many.close()


C3_SMALL = CONFIGS["mh_d8_onedpid_dyn_f32"]
# clocks for the captured rollouts (20 steps per replay, two replays): truncations in both
CAP_TRUNC_AT = (0, 3, 6, 7, 13, 19, 20, 27, 39)


def captured(sw, n, replays, step):
    """`n` calls of step(j) captured into one graph, replayed `replays` times."""
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for j in range(n):
            step(j)
    for _ in range(replays):
        g.replay()
    torch.cuda.synchronize()
    return g


@pytest.mark.parametrize("depth", [None, "1", "4"])
def test_captured_steps_equal_eager(depth, monkeypatch):
    """20 captured random-policy steps cycling through 7 buffer sets (so a kernel
    node can hold at most 7 steps), replayed twice, against 40 eager steps."""
    if depth is None:
        monkeypatch.delenv("QS_MAX_FUSED_STEPS", raising=False)
    else:
        monkeypatch.setenv("QS_MAX_FUSED_STEPS", depth)
    eager, cap = twins(C3_SMALL, clocks=CAP_TRUNC_AT)
    oe, oc = Outs(eager, 7), Outs(cap, 7)
    for t in range(40):
        eager.step(None, **oe.kw(t % 20))   # the graph's slot cycle restarts at each replay
    g = captured(cap, 20, 2, lambda j: cap.step(None, **oc.kw(j)))
    assert oe.bufs["truncated"].sum().item() > 0
    same_outputs(oe, oc)
    same_state(eager, cap)
    del g
    eager.close()
    cap.close()


def test_one_output_buffer_is_not_joined(monkeypatch):
    monkeypatch.delenv("QS_MAX_FUSED_STEPS", raising=False)
    eager, cap = twins(C3_SMALL, clocks=CAP_TRUNC_AT)
    for _ in range(12):
        eager.step(None, want_terminal=True, want_reasons=True, actions_out=None)
    g = captured(cap, 6, 2, lambda j: cap.step(None, want_terminal=True, want_reasons=True))
    for k in ("obs", "reward", "terminated", "truncated", "terminal_obs", "reasons"):
        assert np.array_equal(getattr(eager, k).cpu().numpy(), getattr(cap, k).cpu().numpy()), k
    same_state(eager, cap)
    del g
    eager.close()
    cap.close()


def test_policy_actions_are_not_joined(monkeypatch):
    monkeypatch.delenv("QS_MAX_FUSED_STEPS", raising=False)
    eager, cap = twins(C3_SMALL, clocks=CAP_TRUNC_AT)
    oe, oc = Outs(eager, 6), Outs(cap, 6)
    gen = torch.Generator(device="cpu").manual_seed(11)
    acts = (torch.rand((6, eager.num_envs, eager.num_drones, eager.act_dim), generator=gen) * 2 - 1).to(eager.device)
    for t in range(12):
        eager.step(acts[t % 6], **oe.kw(t % 6))
    g = captured(cap, 6, 2, lambda j: cap.step(acts[j], **oc.kw(j)))
    same_outputs(oe, oc)
    same_state(eager, cap)
    del g
    eager.close()
    cap.close()


def test_a_call_between_two_steps_is_not_joined_over(monkeypatch):
    """get_state between captured steps 2 and 3 reads the state after step 2 (of each replay)."""
    monkeypatch.delenv("QS_MAX_FUSED_STEPS", raising=False)
    eager, cap = twins(C3_SMALL, clocks=CAP_TRUNC_AT)
    oe, oc = Outs(eager, 6), Outs(cap, 6)
    mid_e = None
    for t in range(12):
        eager.step(None, **oe.kw(t % 6))
        if t == 6 + 2:
            mid_e = eager.get_state(L.STATE_AGENT).cpu().numpy()
    mid = {}

    def step(j):
        cap.step(None, **oc.kw(j))
        if j == 2:
            mid["agent"] = cap.get_state(L.STATE_AGENT)

    g = captured(cap, 6, 2, step)
    assert np.array_equal(mid["agent"].cpu().numpy(), mid_e)
    same_outputs(oe, oc)
    same_state(eager, cap)
    del g
    eager.close()
    cap.close()


def test_deferred_reset_search_layout_takes_single_steps(monkeypatch):
    """The reference's diagonal layout (reset draws can be rejected: the search
    launch follows each step), C2's shape at 16 envs, captured and through step_many."""
    monkeypatch.delenv("QS_MAX_FUSED_STEPS", raising=False)
    cfg = dict(task="multihover", num_drones=4, num_envs=16, act="rpm")
    eager, cap = twins(cfg, clocks=CAP_TRUNC_AT)
    many = QuadSwarm(**cfg)
    many.reset(3)
    set_clocks(many, CAP_TRUNC_AT)
    oe, oc, om = Outs(eager, 6), Outs(cap, 6), Outs(many, 6)
    for t in range(12):
        eager.step(None, **oe.kw(t % 6))
    g = captured(cap, 6, 2, lambda j: cap.step(None, **oc.kw(j)))
    many.step_many([om.kw(t % 6) for t in range(12)])
    assert oe.bufs["truncated"].sum().item() > 0
    same_outputs(oe, oc)
    same_outputs(oe, om)
    same_state(eager, cap)
    same_state(eager, many)
    del g
    for sw in (eager, cap, many):
        assert sw.reset_error() == 0
        sw.close()
