"""The ring instance's stores (step_mh_ring.hip, QS_RING_ITEMS): the action-history ring written
once after the loop from registers, against single steps, as bit patterns.

A ring launch no longer stores each step's action to history slot `total % 15`; after its last
step it writes all 15 slots from the registers that hold the history in age order.  Afterwards
every slot must hold what per-step stores would have left: the launch's last min(n, 15)
actions, each in the slot of its step, every other slot as it was.  The next launch reads the
ring from memory, so a misplaced slot shows in its obs.

Every case: a twin handle with QS_MAX_FUSED_STEPS=1 steps eagerly through the same slot cycle.
 1. 19 eager single steps on both handles: the ring is full of distinct non-zero actions and the
    next write slot is 19 % 15 = 4 (asserted), so a launch starts mid-ring;
 2. the ring launch (step_many, or a captured graph replayed twice) on one, single steps on the
    twin; compared as bytes: every output set, the four state blocks (STATE_HISTORY among them),
    the episode log and its total; reset_error() is 0; ring_counts() says the ring path ran;
 3. 16 more eager single steps on both, a buffer set each: every obs compared, then all of 2 again.
Episode clocks are set so that envs are truncated inside the ring launch (and one in the eager
steps before it): the auto-reset leaves the history alone.

Launch lengths 4, 13, 14, 15, 16 and 31 over P = 3 sets: fewer steps than slots (untouched slots
keep their bytes), one slot untouched, exactly the ring, one and many slots written twice.
E = 8 and E = 24 (one and three workgroups); the fp64 and PYB instances (P = 4, n = 16); 20
captured steps over 7 sets replayed twice against 40 eager steps (the second replay starts from
the slots the first one stored).

The layout is grid_layout(D) at 1 m spacing: no reset draw can be rejected.
"""
import numpy as np
import pytest
import torch

from gym_pybullet_drones_amd import _lib as L
from gym_pybullet_drones_amd.envs.swarm import QuadSwarm, grid_layout

pytestmark = pytest.mark.gpu

NEVER = 10000   # a step no run here reaches
H = 15          # history slots at the default control frequency
PRE, POST = 19, 16
BLOCKS = (L.STATE_AGENT, L.STATE_ENV, L.STATE_HISTORY, L.STATE_EP_RETURN)
ENV_VARS = ("QS_MAX_FUSED_STEPS", "QS_RING_LAUNCH", "QS_RING_MAX_STEPS", "QS_HOT_SHAPE")


def cfg(E=8, **kw):
    return dict(task="multihover", num_drones=8, num_envs=E, act="one_d_pid", initial_xyzs=grid_layout(8), **kw)


def raw(x):
    """The bytes of an array: +0 and −0 differ."""
    x = np.ascontiguousarray(x.cpu().numpy() if isinstance(x, torch.Tensor) else x)
    return x.view(np.uint8)


def set_clocks_at(sw, at):
    S = sw.substeps
    limit = int(round(sw.episode_len_sec * sw.pyb_freq))
    env = sw.get_state(L.STATE_ENV).clone()
    t = torch.as_tensor(at, dtype=torch.int32, device=env.device)
    env[L.E_STEP_COUNTER] = limit + S - S * t
    env[L.E_EP_LEN] = (limit + S - S * t) // S
    sw.set_state(L.STATE_ENV, env)


class Slots:
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


def snapshot(sw, slots, post):
    torch.cuda.synchronize()
    snap = {k: raw(v) for k, v in slots.bufs.items()}
    snap.update({"post_" + k: raw(v) for k, v in post.bufs.items()})
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


def run(c, at, P, n, how, monkeypatch):
    """The three phases on one handle.  how: "single" (the twin), "many" (one step_many call)
    or "graph" (n captured steps replayed twice; the twin then runs 2 n single steps).
    Returns the snapshots after phases 2 and 3."""
    for v in ENV_VARS:
        monkeypatch.delenv(v, raising=False)
    if how[0] == "single":
        monkeypatch.setenv("QS_MAX_FUSED_STEPS", "1")
    sw = QuadSwarm(**c)
    sw.reset(3)
    set_clocks_at(sw, at)
    slots, post = Slots(sw, P), Slots(sw, POST)
    for j in range(PRE):
        sw.step(None, **slots.kw(j % P))
    torch.cuda.synchronize()
    env = sw.get_state(L.STATE_ENV).cpu().numpy()
    assert (env[L.E_TOTAL_STEPS] == PRE).all() and PRE % H == 4
    hist = sw.get_state(L.STATE_HISTORY).cpu().numpy().reshape(H, -1)
    assert (hist != 0).all() and all(not np.array_equal(hist[i], hist[j]) for i in range(H) for j in range(i))
    graph = None
    if how == ("single", "many"):
        for j in range(n):
            sw.step(None, **slots.kw(j % P))
    elif how == ("single", "graph"):
        for j in range(2 * n):
            sw.step(None, **slots.kw(j % n % P))
    elif how == ("many",):
        sw.step_many([slots.kw(j % P) for j in range(n)])
        assert sw.launch_counts() == (0, 1) and sw.ring_counts() == (1, n)
    else:
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for j in range(n):
                sw.step(None, **slots.kw(j % P))
        assert sw.launch_counts() == (0, 1) and sw.ring_counts() == (1, n)
        graph.replay()
        graph.replay()   # starts mid-ring, from the slots the first replay stored
    mid = snapshot(sw, slots, post)
    for j in range(POST):   # these read the ring from memory
        sw.step(None, **post.kw(j))
    end = snapshot(sw, slots, post)
    if how[0] == "single":
        assert sw.launch_counts() == (0, 0) and sw.ring_counts() == (0, 0)
        assert mid["log_total"] > 0
    else:
        assert sw.launch_counts() == (0, 1) and sw.ring_counts() == (1, n)
    del graph
    sw.close()
    return mid, end


_REFERENCE = {}


def check(c, at, P, n, how, monkeypatch):
    key = (repr(sorted((k, repr(v)) for k, v in c.items())), tuple(int(x) for x in at), P, n, how)
    if key not in _REFERENCE:
        _REFERENCE[key] = run(c, at, P, n, ("single", how), monkeypatch)
    ref_mid, ref_end = _REFERENCE[key]
    mid, end = run(c, at, P, n, (how,), monkeypatch)
    same(mid, ref_mid, "after the ring launch")
    for j in range(POST):
        assert np.array_equal(end["post_obs"].reshape(POST, -1)[j], ref_end["post_obs"].reshape(POST, -1)[j]), ("obs of later step", j)
    same(end, ref_end, "after the later single steps")


def ends(E, n, envs):
    """Truncations: envs[0] in the eager steps before the launch, then the launch's first step,
    a step inside it and its last step, in turn."""
    at = np.full(E, NEVER, np.int64)
    when = (PRE, PRE + n // 2, PRE + n - 1)
    at[envs[0]] = PRE - 2
    for i, e in enumerate(envs[1:]):
        at[e] = when[i % 3]
    return at


# ------------------------------------------------------------------ the history ring
@pytest.mark.parametrize("n", [4, 13, 14, 15, 16, 31])
@pytest.mark.parametrize("E", [8, 24])
def test_history_slots_after_a_ring_launch(E, n, monkeypatch):
    check(cfg(E), ends(E, n, (0, 1, 2, 4) + ((17, 20) if E >= 24 else ())), 3, n, "many", monkeypatch)


@pytest.mark.parametrize("extra", [dict(precision=8), dict(physics="pyb")], ids=["f64_dyn", "f32_pyb"])
def test_other_instances(extra, monkeypatch):
    check(cfg(8, **extra), ends(8, 16, (0, 1, 2, 4)), 4, 16, "many", monkeypatch)


@pytest.mark.parametrize("E", [8, 24])
def test_captured_ring_node_replayed_twice(E, monkeypatch):
    """20 captured steps over 7 sets replayed twice against 40 eager steps."""
    n = 20
    at = ends(E, 2 * n, (0, 1, 2, 4) + ((17, 20) if E >= 24 else ()))
    at[3] = PRE + n   # the second replay's first step
    check(cfg(E), at, 7, n, "graph", monkeypatch)
