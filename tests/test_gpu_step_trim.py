"""The trimmed multi-step kernel against single steps, as bit patterns, and the
in-wave per-env reduction against the LDS one.

The multi-step instances carry each step's attitude readback into the next
step's PID, keep the action history in age order in registers, test truncation
as an integer compare and (for 2, 4, 8 or 16 drones) reduce the per-env reward
and flags inside the wave.  None of it may change a bit of any output or of the
state: the reference is the single-step path (`QuadSwarm.step`) on the same GPU,
which test_gpu_parity.py and test_gpu_tolerance.py pin to the oracle.

 1. `step_many` against `step` at depth 16 (37 steps: 16 + 16 + 5) and at depth 32
    (70 steps: 32 + 32 + 6, the 15-slot history ring wraps twice inside one
    launch), C3's shape on 9 envs (one full wave and a one-env wave), with envs
    truncated on the first, a middle and the last step of a launch and on
    consecutive steps.  Compared as raw bytes, so a −0 carried where the single
    step has +0 (the reset attitude that goes into the PID's last_rpy) shows.
 2. The same at depth 32 for the VEL action (A = 4, D = 3, PYB) and for a 60 Hz
    control frequency (history in LDS).
 3. Handles created under QS_WAVE_REDUCE=0 (LDS reduction) and under the default,
    D = 2, 4, 8, 16, single steps and one multi-step launch: reward, flags,
    reasons and the episode log bit-equal.  (The in-wave reduction is in the
    multi-step instances; single steps take the LDS path under either setting,
    and so does D = 5.)
"""
import numpy as np
import pytest
import torch

from gym_pybullet_drones_amd import _lib as L
from gym_pybullet_drones_amd.envs.swarm import QuadSwarm, grid_layout

from test_gpu_step_fusion import BLOCKS, Outs, set_clocks

pytestmark = pytest.mark.gpu

# (depth, steps, the step at which env e mod 9 is truncated): first / middle / last
# step of each launch, and consecutive steps across a launch boundary
RUNS = {
    16: (37, (0, 7, 15, 16, 17, 24, 31, 32, 36)),
    32: (70, (0, 15, 31, 32, 33, 48, 63, 64, 69)),
}
C3_9 = dict(task="multihover", num_drones=8, num_envs=9, act="one_d_pid", initial_xyzs=grid_layout(8))
VEL_PYB = dict(task="multihover", num_drones=3, num_envs=22, act="vel", physics="pyb", initial_xyzs=grid_layout(3))
HZ60 = dict(task="multihover", num_drones=8, num_envs=9, act="one_d_pid", initial_xyzs=grid_layout(8), ctrl_freq=60)


def raw(x):
    """The bytes of an array (int32 / uint8 views of the same memory): +0 and −0 differ."""
    x = np.ascontiguousarray(x.cpu().numpy() if isinstance(x, torch.Tensor) else x)
    return x.view(np.uint8) if x.dtype != np.bool_ else x.astype(np.uint8)


def run_pair(cfg, depth, monkeypatch, bits):
    steps, trunc_at = RUNS[depth]
    monkeypatch.setenv("QS_MAX_FUSED_STEPS", str(depth))
    one, many = QuadSwarm(**cfg), QuadSwarm(**cfg)
    for sw in (one, many):
        sw.reset(3)
        set_clocks(sw, trunc_at)
    o1, o2 = Outs(one, steps), Outs(many, steps)
    for j in range(steps):
        one.step(None, **o1.kw(j))
    many.step_many([o2.kw(j) for j in range(steps)])
    torch.cuda.synchronize()
    assert o1.bufs["truncated"].sum().item() > 0
    if bits:   # every env is truncated in the step its clock was set for
        tr = o1.bufs["truncated"].cpu().numpy()
        for e in range(one.num_envs):
            assert tr[trunc_at[e % len(trunc_at)], e] == 1, e
    view = raw if bits else (lambda x: x.cpu().numpy() if isinstance(x, torch.Tensor) else x)
    for k in o1.bufs:
        assert np.array_equal(view(o1.bufs[k]), view(o2.bufs[k])), k
    for blk in BLOCKS:
        assert np.array_equal(view(one.get_state(blk)), view(many.get_state(blk))), f"state block {blk}"
    (ra, ta), (rb, tb) = one.episode_log(), many.episode_log()
    assert ta == tb and np.array_equal(raw(ra) if bits else ra, raw(rb) if bits else rb)
    assert one.reset_error() == 0 and many.reset_error() == 0
    if bits and cfg.get("act") == "one_d_pid":
        # the case the byte compare is for: a reset env's next PID call stores the
        # pitch of the reset quaternion, asin(−0) = −0, as last_rpy
        agent = many.get_state(L.STATE_AGENT).cpu().numpy()
        assert np.signbit(agent[L.F_PID_LAST_RPY + 1]).any()
    one.close()
    many.close()


@pytest.mark.parametrize("depth", [16, 32])
def test_step_many_bit_patterns(depth, monkeypatch):
    run_pair(C3_9, depth, monkeypatch, bits=True)


@pytest.mark.parametrize("cfg", [VEL_PYB, HZ60], ids=["vel_d3_pyb", "60hz_lds_history"])
def test_step_many_depth_32_other_paths(cfg, monkeypatch):
    run_pair(cfg, 32, monkeypatch, bits=False)


WR_STEPS = 20
WR_TRUNC_AT = (0, 3, 7, 8, 13, 19)
WR_KEYS = ("reward", "terminated", "truncated", "reasons")


def reduction_run(D, wave, many, monkeypatch):
    """20 random-policy steps of MultiHover with D drones on ⌈70 / D⌉ envs (the last
    wave partly filled): outputs, episode log."""
    if wave:
        monkeypatch.delenv("QS_WAVE_REDUCE", raising=False)
    else:
        monkeypatch.setenv("QS_WAVE_REDUCE", "0")
    monkeypatch.delenv("QS_MAX_FUSED_STEPS", raising=False)
    sw = QuadSwarm(task="multihover", num_drones=D, num_envs=-(-70 // D), act="one_d_pid", initial_xyzs=grid_layout(D))
    sw.reset(5)
    set_clocks(sw, WR_TRUNC_AT)
    o = Outs(sw, WR_STEPS)
    if many:
        sw.step_many([o.kw(j) for j in range(WR_STEPS)])
    else:
        for j in range(WR_STEPS):
            sw.step(None, **o.kw(j))
    torch.cuda.synchronize()
    out = {k: raw(o.bufs[k]) for k in WR_KEYS}
    out["log"], out["log_total"] = sw.episode_log()
    out["env"] = raw(sw.get_state(L.STATE_ENV))
    out["ep_return"] = raw(sw.get_state(L.STATE_EP_RETURN))
    assert sw.reset_error() == 0
    sw.close()
    return out


def same_reduction(a, b):
    assert a["truncated"].sum() > 0
    for k in WR_KEYS + ("env", "ep_return"):
        assert np.array_equal(a[k], b[k]), k
    assert a["log_total"] == b["log_total"] and a["log_total"] > 0
    assert np.array_equal(raw(a["log"]), raw(b["log"]))


@pytest.mark.parametrize("D", [2, 4, 8, 16])
@pytest.mark.parametrize("many", [False, True], ids=["single", "many"])
def test_wave_reduction_equals_lds_reduction(D, many, monkeypatch):
    same_reduction(reduction_run(D, False, many, monkeypatch), reduction_run(D, True, many, monkeypatch))


def test_other_drone_counts_keep_the_lds_path(monkeypatch):
    same_reduction(reduction_run(5, False, True, monkeypatch), reduction_run(5, True, True, monkeypatch))
    same_reduction(reduction_run(5, True, False, monkeypatch), reduction_run(5, True, True, monkeypatch))
