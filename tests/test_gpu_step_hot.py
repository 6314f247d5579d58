"""The shape-specialised multi-step kernel instance ("hot shape", step_mh_hot.hip) against
the general instance and against single steps, as bit patterns.

A synthetic-policy launch of MultiHover / ONE_D_PID / 30 Hz with 8 drones, a multiple of 8
envs, a reject-free layout and the bench's output set (obs, reward, terminated, truncated,
actions_out; no terminal_obs, no reasons) runs a kernel with all of that folded in as
constants (qs::hot_shape_ok decides, per launch).  Nothing it computes may differ by a bit.
`QuadSwarm.launch_counts()` says which instance the launches ran on, so a predicate that
never fires (or always does) cannot pass.

 1. Full waves with resets: E = 8 (one wave) and E = 24 (three), depth 32, envs truncated on
    the first, second, 17th and last step of the launch, two envs of one wave on the same
    step, one wave with none.  Outputs per step, the four state blocks and the episode log
    against a QS_HOT_SHAPE=0 handle running the same step_many, and against 32 single steps.
 2. Depths 2 and 3 (7 steps: the launches end on different steps), and fp64 DYN / fp32 PYB at
    depth 4.
 3. Launches that do not qualify take the general instance and equal single steps: a partial
    workgroup (E = 12), D = 4, one step without a reward, one misaligned obs buffer, and
    terminal_obs / reasons requested.
 4. Captured graphs: five qualifying steps become one hot node; a fourth step that asks for
    terminal_obs turns the node general; a first step that does, with the rest qualifying,
    also ends general (the choice is made anew at every append).

The layout is grid_layout(8) at 1 m spacing: every pair of drones is at least 1 m apart in x
or y, so no reset draw (noise < 0.25 per axis) can be rejected, whatever the seed — checked
below on the host; the handles' reset_error() stays 0.
"""
import ctypes

import numpy as np
import pytest
import torch

from gym_pybullet_drones_amd import _lib as L
from gym_pybullet_drones_amd.envs.swarm import QuadSwarm, grid_layout

from test_gpu_step_fusion import BLOCKS, Outs, captured
from test_gpu_step_trim import raw

pytestmark = pytest.mark.gpu

NEVER = 200   # a step no run here reaches
HOT_KEYS = ("obs", "reward", "terminated", "truncated", "actions_out")


def cfg(E=8, D=8, **kw):
    return dict(task="multihover", num_drones=D, num_envs=E, act="one_d_pid", initial_xyzs=grid_layout(D), **kw)


def test_layout_is_reject_free():
    xyz = np.asarray(grid_layout(8), np.float64).reshape(8, 3)
    for i in range(8):
        for j in range(i + 1, 8):
            assert abs(xyz[i, 0] - xyz[j, 0]) >= 1.0 or abs(xyz[i, 1] - xyz[j, 1]) >= 1.0, (i, j)
    assert xyz[:, 2].min() - 0.25 >= 0.1   # the z clip never binds from below either


def end_steps(E, steps):
    """The step (0-based) at which each env is truncated: first, second, middle and last step;
    envs 2 and 4 of the first wave on the same step; the second wave of three has none."""
    at = np.full(E, NEVER, np.int64)
    at[:5] = (0, 1, steps // 2, steps - 1, steps // 2)
    if E >= 24:
        at[16], at[17], at[20] = steps - 1, 0, 0
    return at


def set_clocks_at(sw, at):
    S = sw.substeps
    limit = int(round(sw.episode_len_sec * sw.pyb_freq))
    env = sw.get_state(L.STATE_ENV).clone()
    t = torch.as_tensor(at, dtype=torch.int32, device=env.device)
    env[L.E_STEP_COUNTER] = limit + S - S * t
    env[L.E_EP_LEN] = (limit + S - S * t) // S
    sw.set_state(L.STATE_ENV, env)


class HotOuts:
    """`n` sets of the bench's step outputs (no terminal_obs, no reasons)."""

    def __init__(self, sw, n):
        E, D, O, A = sw.num_envs, sw.num_drones, sw.obs_dim, sw.act_dim
        kw = dict(device=sw.device)
        self.bufs = dict(obs=torch.zeros((n, E, D, O), **kw), reward=torch.zeros((n, E), dtype=sw.rdtype, **kw),
                         terminated=torch.zeros((n, E), dtype=torch.uint8, **kw),
                         truncated=torch.zeros((n, E), dtype=torch.uint8, **kw),
                         actions_out=torch.zeros((n, E, D, A), **kw))

    def kw(self, j):
        return {k: v[j] for k, v in self.bufs.items()}


def make(c, seed, at, hot, depth, monkeypatch):
    monkeypatch.setenv("QS_MAX_FUSED_STEPS", str(depth))
    if hot:
        monkeypatch.delenv("QS_HOT_SHAPE", raising=False)
    else:
        monkeypatch.setenv("QS_HOT_SHAPE", "0")
    sw = QuadSwarm(**c)
    sw.reset(seed)
    set_clocks_at(sw, at)
    return sw


def snapshot(sw, outs):
    torch.cuda.synchronize()
    snap = {k: raw(v) for k, v in outs.bufs.items()}
    for blk in BLOCKS:
        snap[f"state{blk}"] = raw(sw.get_state(blk))
    recs, total = sw.episode_log()
    snap["log"], snap["log_total"] = raw(recs), total
    assert sw.reset_error() == 0
    return snap


def same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        if k == "log_total":
            assert a[k] == b[k], (what, k)
        else:
            assert np.array_equal(a[k], b[k]), (what, k)


def run_many(c, steps, depth, hot, monkeypatch, seed=3, outs_cls=HotOuts):
    sw = make(c, seed, end_steps(c["num_envs"], steps), hot, depth, monkeypatch)
    o = outs_cls(sw, steps)
    sw.step_many([o.kw(j) for j in range(steps)])
    snap = snapshot(sw, o)
    counts = sw.launch_counts()
    sw.close()
    return snap, counts


def run_single(c, steps, monkeypatch, seed=3, outs_cls=HotOuts):
    sw = make(c, seed, end_steps(c["num_envs"], steps), True, 1, monkeypatch)
    o = outs_cls(sw, steps)
    for j in range(steps):
        sw.step(None, **o.kw(j))
    snap = snapshot(sw, o)
    assert sw.launch_counts() == (0, 0)
    sw.close()
    return snap


def n_launches(steps, depth):
    """Multi-step launches step_many makes of `steps` steps (a last run of one step is a single launch)."""
    return steps // depth + (1 if steps % depth > 1 else 0)


def check_hot(c, steps, depth, monkeypatch):
    hot, hc = run_many(c, steps, depth, True, monkeypatch)
    gen, gc = run_many(c, steps, depth, False, monkeypatch)
    one = run_single(c, steps, monkeypatch)
    at = end_steps(c["num_envs"], steps)
    tr = one["truncated"].reshape(steps, c["num_envs"])
    for e in np.nonzero(at < steps)[0]:
        assert tr[at[e], e] == 1, e
    assert one["log_total"] >= int((at < steps).sum())
    assert hc == (0, n_launches(steps, depth)) and gc == (n_launches(steps, depth), 0)
    same(hot, gen, "hot vs general")
    same(hot, one, "hot vs single steps")


@pytest.mark.parametrize("E", [8, 24])
def test_full_waves_with_resets(E, monkeypatch):
    check_hot(cfg(E), 32, 32, monkeypatch)
    if E == 8:   # the case the byte compare is for: a reset env's next PID call stores pitch asin(−0) = −0
        sw = make(cfg(E), 3, end_steps(E, 32), True, 32, monkeypatch)
        o = HotOuts(sw, 32)
        sw.step_many([o.kw(j) for j in range(32)])
        assert np.signbit(sw.get_state(L.STATE_AGENT).cpu().numpy()[L.F_PID_LAST_RPY + 1]).any()
        sw.close()


@pytest.mark.parametrize("depth", [2, 3])
def test_other_depths(depth, monkeypatch):
    check_hot(cfg(8), 7, depth, monkeypatch)


@pytest.mark.parametrize("extra", [dict(precision=8), dict(physics="pyb")], ids=["f64_dyn", "f32_pyb"])
def test_other_instances(extra, monkeypatch):
    check_hot(cfg(8, **extra), 8, 4, monkeypatch)


# ------------------------------------------------------------------ fallbacks
def check_general(c, steps, depth, monkeypatch, outs_cls=HotOuts):
    many, counts = run_many(c, steps, depth, True, monkeypatch, outs_cls=outs_cls)
    assert counts == (n_launches(steps, depth), 0)
    same(many, run_single(c, steps, monkeypatch, outs_cls=outs_cls), "general vs single steps")


def test_partial_workgroup_takes_the_general_instance(monkeypatch):
    check_general(cfg(12), 8, 8, monkeypatch)


def test_four_drones_take_the_general_instance(monkeypatch):
    check_general(cfg(16, D=4), 8, 8, monkeypatch)


def test_terminal_obs_and_reasons_take_the_general_instance(monkeypatch):
    check_general(cfg(8), 8, 8, monkeypatch, outs_cls=Outs)


class MisalignedObs(HotOuts):
    """Step 2's obs starts 4 bytes into a 16-byte unit."""

    def __init__(self, sw, n):
        super().__init__(sw, n)
        rows = sw.num_agents * sw.obs_dim
        self.flat = torch.zeros(rows + 4, device=sw.device)
        self.shape = (sw.num_envs, sw.num_drones, sw.obs_dim)
        assert self.flat.data_ptr() % 16 == 0

    def kw(self, j):
        d = super().kw(j)
        if j == 2:
            d["obs"] = self.flat[1:1 + self.flat.numel() - 4].view(self.shape)
            assert d["obs"].data_ptr() % 16 == 4
        return d


def test_misaligned_obs_takes_the_general_instance(monkeypatch):
    steps = 6
    res = []
    for single in (False, True):
        sw = make(cfg(8), 3, end_steps(8, steps), True, 1 if single else steps, monkeypatch)
        o = MisalignedObs(sw, steps)
        if single:
            for j in range(steps):
                sw.step(None, **o.kw(j))
        else:
            sw.step_many([o.kw(j) for j in range(steps)])
            assert sw.launch_counts() == (1, 0)
        snap = snapshot(sw, o)
        snap["obs2"] = raw(o.flat)
        res.append(snap)
        sw.close()
    assert res[0]["obs2"].any()
    same(res[0], res[1], "misaligned obs vs single steps")


def raw_steps(sw, kws, many):
    """Steps through the C entry points, so that an output may be absent (None)."""
    recs = [L.QsStepOut(L.ptr(k.get("obs")), L.ptr(k.get("reward")), L.ptr(k.get("terminated")), L.ptr(k.get("truncated")),
                        None, None, L.ptr(k.get("actions_out"))) for k in kws]
    if many:
        arr = (L.QsStepOut * len(recs))(*recs)
        L.check(sw.lib.qs_step_many(sw._h, len(recs), arr, sw._stream()), "qs_step_many")
    else:
        for r in recs:
            L.check(sw.lib.qs_step(sw._h, None, ctypes.byref(r), sw._stream()), "qs_step")


def test_a_step_without_reward_takes_the_general_instance(monkeypatch):
    steps = 6
    res = []
    for single in (False, True):
        sw = make(cfg(8), 3, end_steps(8, steps), True, 1 if single else steps, monkeypatch)
        o = HotOuts(sw, steps)
        kws = [o.kw(j) for j in range(steps)]
        kws[2] = {k: v for k, v in kws[2].items() if k != "reward"}
        raw_steps(sw, kws, many=not single)
        if not single:
            assert sw.launch_counts() == (1, 0)
        res.append(snapshot(sw, o))
        sw.close()
    rew = res[0]["reward"].reshape(steps, -1)
    assert not rew[2].any() and rew[1].any() and rew[3].any()
    same(res[0], res[1], "absent reward vs single steps")


# ------------------------------------------------------------- captured graphs
def captured_run(monkeypatch, terminal_at):
    """Five steps captured and replayed twice (the step `terminal_at`, if any, asks for
    terminal_obs), against ten eager single steps: (node counts, snapshots)."""
    steps = 5
    at = end_steps(8, 2 * steps)
    snaps = []
    counts = None
    for eager in (False, True):
        monkeypatch.delenv("QS_MAX_FUSED_STEPS", raising=False)
        sw = make(cfg(8), 3, at, True, 32, monkeypatch)
        o = HotOuts(sw, steps)
        tobs = torch.zeros((sw.num_envs, sw.num_drones, sw.obs_dim), device=sw.device)

        def step(j):
            kw = o.kw(j)
            if j == terminal_at:
                kw["terminal_obs"] = tobs
            sw.step(None, **kw)

        if eager:
            for t in range(2 * steps):
                step(t % steps)
        else:
            g = captured(sw, steps, 2, step)
            counts = sw.launch_counts()
        snap = snapshot(sw, o)
        snap["tobs"] = raw(tobs)
        snaps.append(snap)
        if not eager:
            del g
        sw.close()
    same(snaps[0], snaps[1], "captured vs eager single steps")
    return counts


def test_captured_steps_become_one_hot_node(monkeypatch):
    assert captured_run(monkeypatch, None) == (0, 1)


def test_capture_whose_fourth_step_disqualifies_ends_general(monkeypatch):
    assert captured_run(monkeypatch, 3) == (1, 0)


def test_capture_whose_first_step_disqualifies_stays_general(monkeypatch):
    assert captured_run(monkeypatch, 0) == (1, 0)
