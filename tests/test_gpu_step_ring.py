"""Ring launches (step_mh_ring.hip): a hot-shape launch that goes on past its distinct output
sets while the further steps write those sets again in the same order, against single steps,
as bit patterns.

A rollout that cycles through P buffer sets used to be cut every P steps (a launch's steps
must not share outputs).  qs::FuseGroup::can_wrap now keeps a step in the launch when it writes
exactly the set that is due in the cycle, and the ring instance of the kernel (step_kernel
HOT = 2) writes step k through set k mod P.  Afterwards every set must hold what the last
step that wrote it produced, which is what single steps leave; the totals below vary so that
every position of the cycle is the last one once.

The reference is always a twin handle with QS_MAX_FUSED_STEPS=1 that steps eagerly into its
own copy of the same slot cycle.  Compared as bytes: every output set, the four state blocks,
the episode log and its total; reset_error() stays 0.  Episode clocks are set so that envs are
truncated on step 0, step P − 1, step P (the first wrapped step) and the last step, two envs
of one wave on the same step, and (E = 24) one wave with no episode ending.

`QuadSwarm.ring_counts()` and `launch_counts()` say which path ran, so a rule that never
fires cannot pass the first group and one that fires too often cannot pass the second:
 1. ring launches: step_many with P = 3 and totals 4, 5, 6, 7, 11; P = 32 with total 70 (the
    bench's pattern); the fp64 and PYB instances (P = 4, total 9); 20 captured steps over 7
    sets, replayed twice, against 40 eager steps;
 2. launches that are cut as before: QS_RING_LAUNCH=0, depth 4 with 7 sets, a set out of turn,
    the same obs with another reward buffer, one set reused every step, D = 4, E = 12, a set
    with terminal_obs, and QS_RING_MAX_STEPS=10 (the ring launch is cut at the cap).

The layout is grid_layout(D) at 1 m spacing: no reset draw can be rejected.
"""
import numpy as np
import pytest
import torch

from gym_pybullet_drones_amd import _lib as L
from gym_pybullet_drones_amd.envs.swarm import QuadSwarm, grid_layout

pytestmark = pytest.mark.gpu

NEVER = 10000   # a step no run here reaches
BLOCKS = (L.STATE_AGENT, L.STATE_ENV, L.STATE_HISTORY, L.STATE_EP_RETURN)
KEYS = ("obs", "reward", "terminated", "truncated", "actions_out")
ENV_VARS = ("QS_MAX_FUSED_STEPS", "QS_RING_LAUNCH", "QS_RING_MAX_STEPS", "QS_HOT_SHAPE")


def cfg(E=8, D=8, **kw):
    return dict(task="multihover", num_drones=D, num_envs=E, act="one_d_pid", initial_xyzs=grid_layout(D), **kw)


def raw(x):
    """The bytes of an array: +0 and −0 differ."""
    x = np.ascontiguousarray(x.cpu().numpy() if isinstance(x, torch.Tensor) else x)
    return x.view(np.uint8)


def end_steps(E, P, total):
    """The step (0-based) at which each env is truncated: step 0, P − 1, P and the last one;
    envs 2 and 4 of the first wave on the same step; the second wave of three has none."""
    at = np.full(E, NEVER, np.int64)
    at[:5] = (0, P - 1, P, total - 1, P)
    if E >= 24:
        at[16], at[17], at[20] = total - 1, 0, P
    return at


def set_clocks_at(sw, at):
    S = sw.substeps
    limit = int(round(sw.episode_len_sec * sw.pyb_freq))
    env = sw.get_state(L.STATE_ENV).clone()
    t = torch.as_tensor(at, dtype=torch.int32, device=env.device)
    env[L.E_STEP_COUNTER] = limit + S - S * t
    env[L.E_EP_LEN] = (limit + S - S * t) // S
    sw.set_state(L.STATE_ENV, env)


class Slots:
    """`n` sets of the bench's step outputs (no terminal_obs, no reasons), a spare reward
    buffer and a spare terminal_obs buffer."""

    def __init__(self, sw, n):
        E, D, O, A = sw.num_envs, sw.num_drones, sw.obs_dim, sw.act_dim
        kw = dict(device=sw.device)
        self.bufs = dict(obs=torch.zeros((n, E, D, O), **kw), reward=torch.zeros((n, E), dtype=sw.rdtype, **kw),
                         terminated=torch.zeros((n, E), dtype=torch.uint8, **kw),
                         truncated=torch.zeros((n, E), dtype=torch.uint8, **kw),
                         actions_out=torch.zeros((n, E, D, A), **kw))
        self.spare = dict(reward=torch.zeros((E,), dtype=sw.rdtype, **kw), terminal_obs=torch.zeros((E, D, O), **kw))

    def kw(self, j):
        return {k: v[j] for k, v in self.bufs.items()}

    def step(self, spec):
        """spec: a set index, or (set index, "reward") / (set index, "terminal_obs"): that set
        with the spare reward buffer in place of its own / with the spare terminal_obs added."""
        if isinstance(spec, tuple):
            kw = self.kw(spec[0])
            kw[spec[1]] = self.spare[spec[1]]
            return kw
        return self.kw(spec)


def make(c, at, env, monkeypatch, seed=3):
    for v in ENV_VARS:
        monkeypatch.delenv(v, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    sw = QuadSwarm(**c)
    sw.reset(seed)
    set_clocks_at(sw, at)
    return sw


def snapshot(sw, slots):
    torch.cuda.synchronize()
    snap = {k: raw(v) for k, v in slots.bufs.items()}
    snap.update({"spare_" + k: raw(v) for k, v in slots.spare.items()})
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


_REFERENCE = {}


def reference(c, nsets, seq, at, monkeypatch):
    """Single eager steps of a QS_MAX_FUSED_STEPS=1 twin into the same slot cycle; computed
    once per case and shared."""
    key = (repr(sorted((k, repr(v)) for k, v in c.items())), nsets, tuple(seq), tuple(int(x) for x in at))
    if key not in _REFERENCE:
        sw = make(c, at, {"QS_MAX_FUSED_STEPS": 1}, monkeypatch)
        slots = Slots(sw, nsets)
        for spec in seq:
            sw.step(None, **slots.step(spec))
        snap = snapshot(sw, slots)
        assert sw.launch_counts() == (0, 0) and sw.ring_counts() == (0, 0)
        sw.close()
        assert snap["log_total"] >= int((np.asarray(at) < len(seq)).sum()) > 0
        _REFERENCE[key] = snap
    return _REFERENCE[key]


def run_many(c, nsets, seq, at, env, monkeypatch):
    sw = make(c, at, env, monkeypatch)
    slots = Slots(sw, nsets)
    sw.step_many([slots.step(spec) for spec in seq])
    snap = snapshot(sw, slots)
    counts = sw.launch_counts(), sw.ring_counts()
    sw.close()
    return snap, counts


def cycle(P, total):
    return [j % P for j in range(total)]


def check_ring(c, P, total, monkeypatch, env=None):
    at = end_steps(c["num_envs"], P, total)
    seq = cycle(P, total)
    snap, counts = run_many(c, P, seq, at, env or {}, monkeypatch)
    assert counts == ((0, 1), (1, total)), counts
    same(snap, reference(c, P, seq, at, monkeypatch), "ring launch vs single steps")


# ------------------------------------------------------------------ ring launches
@pytest.mark.parametrize("total", [4, 5, 6, 7, 11])
@pytest.mark.parametrize("E", [8, 24])
def test_three_sets(E, total, monkeypatch):
    check_ring(cfg(E), 3, total, monkeypatch)


@pytest.mark.parametrize("E", [8, 24])
def test_bench_pattern_32_sets_70_steps(E, monkeypatch):
    check_ring(cfg(E), 32, 70, monkeypatch)


@pytest.mark.parametrize("extra", [dict(precision=8), dict(physics="pyb")], ids=["f64_dyn", "f32_pyb"])
def test_other_instances(extra, monkeypatch):
    check_ring(cfg(8, **extra), 4, 9, monkeypatch)


def test_the_last_writer_of_every_set_is_seen(monkeypatch):
    """The check has teeth: with P = 3 the totals 4, 5 and 6 leave different bytes in the sets."""
    c = cfg(8)
    refs = [reference(c, 3, cycle(3, t), end_steps(8, 3, t), monkeypatch) for t in (4, 5, 6)]
    assert not np.array_equal(refs[0]["obs"], refs[1]["obs"]) and not np.array_equal(refs[1]["obs"], refs[2]["obs"])


@pytest.mark.parametrize("E", [8, 24])
def test_captured_steps_wrap_into_one_node(E, monkeypatch):
    """20 captured steps over 7 sets, replayed twice, against 40 eager steps: one node."""
    P, steps, replays = 7, 20, 2
    c = cfg(E)
    at = end_steps(E, P, steps * replays)
    sw = make(c, at, {}, monkeypatch)
    slots = Slots(sw, P)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for j in range(steps):
            sw.step(None, **slots.kw(j % P))
    assert sw.launch_counts() == (0, 1) and sw.ring_counts() == (1, steps)
    for _ in range(replays):
        g.replay()
    snap = snapshot(sw, slots)
    assert sw.launch_counts() == (0, 1) and sw.ring_counts() == (1, steps)
    del g
    sw.close()
    # (the eager twin's steps 20 .. 39 start again at set 0, as the replay does)
    seq = cycle(P, steps) * replays
    same(snap, reference(c, P, seq, at, monkeypatch), "captured ring node vs single steps")


# ------------------------------------------------------------------ launches that are cut
def parent_launches(seq, depth):
    """Multi-step launches of the rule without wrapping: the longest runs of steps that share
    no buffer, up to the depth (a run of one step is a single launch and does not count)."""
    def bufs(spec):
        if isinstance(spec, tuple):
            j, what = spec
            return {(j, k) for k in KEYS if k != what} | {("spare", what)}
        return {(spec, k) for k in KEYS}
    n, run, used = 0, 0, set()
    for spec in list(seq) + [None]:
        b = bufs(spec) if spec is not None else None
        if b is None or run == depth or (used & b):
            n += 1 if run > 1 else 0
            run, used = 0, set()
        if b is not None:
            run += 1
            used |= b
    return n


def check_cut(c, nsets, seq, env, monkeypatch, hot=True, depth=32, ring=(0, 0)):
    E = c["num_envs"]
    at = end_steps(E, min(nsets, 3), len(seq))
    snap, (launches, rc) = run_many(c, nsets, seq, at, env, monkeypatch)
    n = parent_launches(seq, depth)
    assert launches == ((0, n) if hot else (n, 0)), launches
    assert rc == ring, rc
    same(snap, reference(c, nsets, seq, at, monkeypatch), "cut launches vs single steps")


def test_parent_launches_rule():
    assert parent_launches(cycle(3, 11), 32) == 4 and parent_launches(cycle(7, 20), 4) == 5
    assert parent_launches([0] * 6, 32) == 0 and parent_launches([0, 1, 2, 1, 0, 2], 32) == 2
    assert parent_launches([0, 1, 2, (0, "reward"), 1, 2], 32) == 2


def test_switch_off(monkeypatch):
    check_cut(cfg(8), 3, cycle(3, 11), {"QS_RING_LAUNCH": 0}, monkeypatch)


def test_depth_4_with_7_sets(monkeypatch):
    check_cut(cfg(8), 7, cycle(7, 20), {"QS_MAX_FUSED_STEPS": 4}, monkeypatch, depth=4)


def test_a_set_out_of_turn(monkeypatch):
    check_cut(cfg(8), 3, [0, 1, 2, 1, 0, 2], {}, monkeypatch)


def test_same_obs_another_reward_buffer(monkeypatch):
    check_cut(cfg(8), 3, [0, 1, 2, (0, "reward"), 1, 2], {}, monkeypatch)


def test_one_set_reused_every_step(monkeypatch):
    check_cut(cfg(8), 1, [0] * 6, {}, monkeypatch)


def test_four_drones(monkeypatch):
    check_cut(cfg(16, D=4), 3, cycle(3, 7), {}, monkeypatch, hot=False)


def test_partial_workgroup(monkeypatch):
    check_cut(cfg(12), 3, cycle(3, 7), {}, monkeypatch, hot=False)


def test_a_step_with_terminal_obs(monkeypatch):
    check_cut(cfg(8), 3, [0, (1, "terminal_obs"), 2, 0, (1, "terminal_obs"), 2, 0], {}, monkeypatch, hot=False)


def test_step_cap(monkeypatch):
    """QS_RING_MAX_STEPS=10, P = 3, 25 steps: ring launches of 10, 10 and 5 steps."""
    c, P, total = cfg(8), 3, 25
    at = end_steps(8, P, total)
    seq = cycle(P, total)
    snap, counts = run_many(c, P, seq, at, {"QS_RING_MAX_STEPS": 10}, monkeypatch)
    assert counts == ((0, 3), (3, total)), counts
    same(snap, reference(c, P, seq, at, monkeypatch), "capped ring launches vs single steps")
