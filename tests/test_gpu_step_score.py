"""Branch rollouts: `QuadSwarm.score` (qs_score) runs C candidate action sequences from
the swarm's current state in one launch and leaves the swarm as it was.

The reference in every case is a twin handle: before each candidate its four state
blocks are restored from a snapshot of the scored swarm's, then it is stepped with
`step_many(outs, actions=a[:, c])` (qs_step_seq, which tests/test_gpu_step_sequence.py
pins to single steps and those to the oracle).  The branch-rollout kernel does the
same operations on the same values and only leaves the stores to the handle out, so
everything is compared as raw bytes.

 1. Equivalence over instances (A = 1 / 3 / 4, fp32 / fp64, history in registers and in
    LDS, CF2P, a shard offset, auto-reset off), n = 7 and n = score_depth().
 2. Wave and candidate boundaries.
 3. The scored swarm is unchanged, and steps on as a swarm that never scored.
 4. ret / first_done against a float64 running sum of the per-step rewards.
 5. Optional and misaligned buffers, shared action buffers.
 6. Depth and refusals, none of which changes the swarm.
 7. Graph capture.
 8. `SwarmVecEnv.score_t`.
"""
import ctypes

import numpy as np
import pytest
import torch

from gym_pybullet_drones_amd import _lib as L
from gym_pybullet_drones_amd.envs.swarm import QuadSwarm, grid_layout
from gym_pybullet_drones_amd.vec_env.vec_env import SwarmVecEnv

pytestmark = pytest.mark.gpu

CONFIGS = {
    "mh_d8_onedpid_f32": dict(task="multihover", num_drones=8, num_envs=21, act="one_d_pid", initial_xyzs=grid_layout(8)),
    "mh_d8_onedpid_f64": dict(task="multihover", num_drones=8, num_envs=5, act="one_d_pid", initial_xyzs=grid_layout(8),
                              precision=8),
    "mh_d3_vel_pyb": dict(task="multihover", num_drones=3, num_envs=22, act="vel", physics="pyb",
                          initial_xyzs=grid_layout(3)),
    "spiral_d5_vel": dict(task="spiral", num_drones=5, num_envs=13, act="vel"),
    # a run-time control frequency: the action history lives in LDS, not in registers
    "mh_d8_onedpid_60hz": dict(task="multihover", num_drones=8, num_envs=21, act="one_d_pid",
                               initial_xyzs=grid_layout(8), ctrl_freq=60),
    "mh_d4_pid_grid": dict(task="multihover", num_drones=4, num_envs=17, act="pid", initial_xyzs=grid_layout(4)),
    "cf2p_d2_rpm": dict(task="multihover", num_drones=2, num_envs=40, act="rpm", drone_model="cf2p",
                        initial_xyzs=grid_layout(2)),
    "mh_d8_offset7": dict(task="multihover", num_drones=8, num_envs=9, act="one_d_pid", initial_xyzs=grid_layout(8),
                          env_offset=7),
    # QS_FLAG_NO_AUTORESET: a done env stays done, so envs are done more than once in a candidate
    "mh_d8_noreset": dict(task="multihover", num_drones=8, num_envs=9, act="one_d_pid", initial_xyzs=grid_layout(8),
                          autoreset=False),
}
C3_SMALL = CONFIGS["mh_d8_onedpid_f32"]
BLOCKS = (L.STATE_AGENT, L.STATE_ENV, L.STATE_HISTORY, L.STATE_EP_RETURN)
OUT_KEYS = ("obs", "reward", "terminated", "truncated", "terminal_obs", "reasons", "actions_out")
QS_E_INVALID, QS_E_STATE = -1, -4


def set_clocks(sw, trunc_at):
    """Episode clocks such that env e is truncated in step trunc_at[e mod len] (None: never here)."""
    E, S = sw.num_envs, sw.substeps
    limit = int(round(sw.episode_len_sec * sw.pyb_freq))
    env = sw.get_state(L.STATE_ENV).clone()
    for e in range(E):
        at = trunc_at[e % len(trunc_at)]
        if at is not None:
            env[L.E_STEP_COUNTER, e] = limit + S - S * at
            env[L.E_EP_LEN, e] = (limit + S - S * at) // S
    sw.set_state(L.STATE_ENV, env)


def ground(sw, env=4):
    """Drone 0 of `env` 1 cm above the ground: a MultiHover env crashes (z < 0.03) in step 0."""
    st = sw.get_state(L.STATE_AGENT).clone()
    st[L.F_POS + 2, env * sw.num_drones] = 0.01
    sw.set_state(L.STATE_AGENT, st)


def clocks_for(n):
    """Truncations on the first, a middle and the last step of an n-step candidate; every fourth env none."""
    return (0, n // 2, n - 1, None, 1, min(5, n - 1))


def prepared(cfg, n, seed=3, warm=2, twins=1):
    """`twins` + 1 swarms in the same mid-episode state: reset, a few random-policy steps (a
    non-trivial history ring, PID state and episode return), clocks and a grounded drone."""
    out = [QuadSwarm(**cfg) for _ in range(twins + 1)]
    for sw in out:
        sw.reset(seed)
        for _ in range(warm):
            sw.step(None)
        set_clocks(sw, clocks_for(n))
        if sw.task == "multihover" and sw.num_envs > 4:
            ground(sw)
    return out


def make_actions(sw, n, C, seed=5):
    """(n, C, E, D, A) actions uniform in [-1.5, 1.5], every candidate different, with
    exact 0 / -0.0 / +-1 rows in known lanes of the first and last step."""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    a = torch.rand((n, C, sw.num_envs, sw.num_drones, sw.act_dim), generator=gen) * 3 - 1.5
    for j in {0, n - 1}:
        a[j, 0, 0, 0, :] = 0.0
        a[j, C - 1, 0, sw.num_drones - 1, :] = -0.0
        a[j, C // 2, sw.num_envs - 1, 0, :] = 1.0
    return a.to(sw.device)


class Outs:
    """n sets of the seven step outputs over `lead` + (E, ...) (zeroed: terminal_obs rows are
    written for done envs only)."""

    def __init__(self, sw, n, lead=()):
        E, D, O, A = sw.num_envs, sw.num_drones, sw.obs_dim, sw.act_dim
        kw = dict(device=sw.device)
        lead = (n,) + tuple(lead)
        self.n = n
        self.bufs = dict(obs=torch.zeros(lead + (E, D, O), **kw), reward=torch.zeros(lead + (E,), dtype=sw.rdtype, **kw),
                         terminated=torch.zeros(lead + (E,), dtype=torch.uint8, **kw),
                         truncated=torch.zeros(lead + (E,), dtype=torch.uint8, **kw),
                         terminal_obs=torch.zeros(lead + (E, D, O), **kw),
                         reasons=torch.zeros(lead + (E, D), dtype=torch.uint8, **kw),
                         actions_out=torch.zeros(lead + (E, D, A), **kw))

    def kws(self, keys=OUT_KEYS):
        return [{k: self.bufs[k][j] for k in keys} for j in range(self.n)]


def raw(t):
    return t.cpu().numpy().tobytes() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t).tobytes()


def same_bytes(a, b, what):
    assert tuple(a.shape) == tuple(b.shape) and raw(a) == raw(b), what


def snapshot(sw):
    torch.cuda.synchronize()
    return [sw.get_state(blk).clone() for blk in BLOCKS]


def fingerprint(sw):
    """Everything qs_score promises to leave alone, as bytes."""
    torch.cuda.synchronize()
    recs, total = sw.episode_log()
    return ([raw(sw.get_state(blk)) for blk in BLOCKS], raw(recs), total, sw.reset_error(), sw.launch_counts())


def reference(ref, snap, acts):
    """The twin's outputs for every candidate: (n, C, E, ...) like score's, from the snapshot each time."""
    n, C = acts.shape[0], acts.shape[1]
    want = Outs(ref, n, lead=(C,))
    for c in range(C):
        for blk, val in zip(BLOCKS, snap):
            ref.set_state(blk, val)
        one = Outs(ref, n)
        ref.step_many(one.kws(), actions=acts[:, c])
        torch.cuda.synchronize()
        for k in OUT_KEYS:
            want.bufs[k][:, c] = one.bufs[k]
    return want


def running_score(reward, terminated, truncated):
    """ret / first_done from (n, C, E) per-step arrays: a float64 running sum in step order up to the first done."""
    n, C, E = reward.shape
    ret, fd = np.zeros((C, E), np.float64), np.full((C, E), n, np.int32)
    for c in range(C):
        for e in range(E):
            acc = np.float64(0.0)
            for j in range(n):
                acc = acc + np.float64(reward[j, c, e])
                if terminated[j, c, e] or truncated[j, c, e]:
                    fd[c, e] = j
                    break
            ret[c, e] = acc
    return ret, fd


def close(*sws):
    for sw in sws:
        sw.close()


def check_equivalence(cfg, n, C):
    if n is None:
        probe = QuadSwarm(**cfg)
        n = probe.score_depth()
        probe.close()
    sw, ref = prepared(cfg, n)
    assert 1 <= n <= sw.score_depth() <= 32
    acts = make_actions(sw, n, C)
    snap = snapshot(sw)
    before = fingerprint(sw)
    got = Outs(sw, n, lead=(C,))
    ret = torch.full((C, sw.num_envs), -7.0, dtype=torch.float64, device=sw.device)
    fd = torch.full((C, sw.num_envs), -7, dtype=torch.int32, device=sw.device)
    sw.score(acts, got.kws(), ret=ret, first_done=fd)
    torch.cuda.synchronize()
    want = reference(ref, snap, acts)
    for k in OUT_KEYS:
        same_bytes(want.bufs[k], got.bufs[k], k)
    same_bytes(got.bufs["actions_out"], acts, "actions_out is the actions, -0.0 included")
    r, t, u = (want.bufs[k].cpu().numpy() for k in ("reward", "terminated", "truncated"))
    wret, wfd = running_score(r, t, u)
    assert np.array_equal(ret.cpu().numpy(), wret) and np.array_equal(fd.cpu().numpy(), wfd)
    assert fingerprint(sw) == before
    close(sw, ref)
    return r, t, u, wfd


# ------------------------------------------------------------------ 1. equivalence
@pytest.mark.parametrize("n", [7, None])   # None: score_depth()
@pytest.mark.parametrize("name", list(CONFIGS))
def test_score_equals_sequences_from_the_same_state(name, n):
    r, t, u, fd = check_equivalence(CONFIGS[name], n, C=3)
    steps = r.shape[0]
    assert u[0].any() and (fd == 0).any()
    if name != "mh_d4_pid_grid":   # (its random position targets end most episodes early)
        assert u[steps - 1].any() and (fd == steps).any()
    if name != "spiral_d5_vel":
        assert t[0, :, 4].all()   # the grounded drone's env, in every candidate
    if name == "mh_d8_noreset":
        assert ((t | u).sum(axis=0) > 1).any()   # done more than once: only the first counts


def test_reset_draw_is_the_source_envs_in_every_candidate():
    """An env truncated in step 0 auto-resets to the same drawn position in every candidate,
    the one the twin draws (keyed on the source env's global id and episode)."""
    sw, ref = prepared(C3_SMALL, 4)
    acts = make_actions(sw, 4, 5)
    got = Outs(sw, 4, lead=(5,))
    sw.score(acts, got.kws(["obs"]))
    torch.cuda.synchronize()
    pos = got.bufs["obs"][0, :, 0, :, :3].cpu().numpy()   # step 0, env 0 (truncated there), xyz of its drones
    assert all(np.array_equal(pos[0], pos[c]) for c in range(5))
    one = Outs(ref, 4)
    ref.step_many(one.kws(), actions=acts[:, 2])
    torch.cuda.synchronize()
    assert np.array_equal(pos[0], one.bufs["obs"][0, 0, :, :3].cpu().numpy())
    close(sw, ref)


# ------------------------------------------------------------ 2. wave / candidate boundaries
@pytest.mark.parametrize("E,C", [(1, 19), (5, 3), (21, 1)])
def test_wave_and_candidate_boundaries(E, C):
    """E = 1, C = 19: two full waves and one of three virtual envs; E = 5, C = 3: a candidate
    boundary inside a wave; C = 1: a plain sequence."""
    check_equivalence(dict(C3_SMALL, num_envs=E), 7, C)


# ------------------------------------------------------------------ 3. no mutation
def test_scored_swarm_steps_on_like_one_that_never_scored():
    n = 9
    sw, never = prepared(C3_SMALL, n)
    acts = make_actions(sw, n, 4)
    before = fingerprint(sw)
    assert before == fingerprint(never)
    got = Outs(sw, n, lead=(4,))
    fd = torch.zeros((4, sw.num_envs), dtype=torch.int32, device=sw.device)
    for _ in range(2):
        sw.score(acts, got.kws(), first_done=fd)
    torch.cuda.synchronize()
    assert (fd.cpu().numpy() < n).any() and got.bufs["terminated"].sum().item() > 0
    assert fingerprint(sw) == before
    o1, o2 = Outs(sw, n), Outs(never, n)
    sw.step_many(o1.kws(), actions=acts[:, 1])
    never.step_many(o2.kws(), actions=acts[:, 1])
    torch.cuda.synchronize()
    for k in OUT_KEYS:
        same_bytes(o1.bufs[k], o2.bufs[k], k)
    assert fingerprint(sw) == fingerprint(never) != before
    close(sw, never)


# ------------------------------------------------------------------ 4. ret / first_done
@pytest.mark.parametrize("name", ["mh_d8_onedpid_f32", "mh_d8_onedpid_f64", "mh_d8_noreset"])
def test_ret_alone_equals_the_running_sum(name):
    n, C = 11, 4
    (sw,) = prepared(CONFIGS[name], n, twins=0)
    acts = make_actions(sw, n, C)
    got = Outs(sw, n, lead=(C,))
    ret, fd = (torch.full((C, sw.num_envs), -7, dtype=dt, device=sw.device) for dt in (torch.float64, torch.int32))
    sw.score(acts, got.kws(["reward", "terminated", "truncated"]), ret=ret, first_done=fd)
    only = torch.full_like(ret, -7)
    sw.score(acts, None, ret=only)                     # nothing but ret
    only_fd = torch.full_like(fd, -7)
    sw.score(acts, first_done=only_fd)                 # nothing but first_done
    torch.cuda.synchronize()
    r, t, u = (got.bufs[k].cpu().numpy() for k in ("reward", "terminated", "truncated"))
    wret, wfd = running_score(r, t, u)
    assert (wfd == 0).any() and (wfd == n).any() and ((wfd > 0) & (wfd < n)).any()
    if name == "mh_d8_noreset":
        assert ((t | u).sum(axis=0) > 1).any()
    for x in (ret, only):
        assert np.array_equal(x.cpu().numpy(), wret)
    for x in (fd, only_fd):
        assert np.array_equal(x.cpu().numpy(), wfd)
    sw.close()


# ------------------------------------------------- 5. optional and misaligned buffers
def offset_by_one_float(t):
    """A copy of `t` whose storage starts one float past an allocation: 4-byte aligned only."""
    buf = torch.zeros(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


@pytest.mark.parametrize("name", ["mh_d8_onedpid_f32", "mh_d3_vel_pyb"])   # fast obs path and A = 1; general path, A = 4
def test_optional_and_misaligned_buffers(name):
    n, C = 6, 3
    (sw,) = prepared(CONFIGS[name], n, twins=0)
    acts = make_actions(sw, n, C)
    full = Outs(sw, n, lead=(C,))
    sw.score(acts, full.kws())
    # reward only
    o = Outs(sw, n, lead=(C,))
    sw.score(acts, o.kws(["reward"]))
    torch.cuda.synchronize()
    same_bytes(o.bufs["reward"], full.bufs["reward"], "reward only")
    assert all(o.bufs[k].abs().sum().item() == 0 for k in OUT_KEYS if k != "reward")
    # obs only, on the last step only
    o = Outs(sw, n, lead=(C,))
    sw.score(acts, [{}] * (n - 1) + [{"obs": o.bufs["obs"][n - 1]}])
    torch.cuda.synchronize()
    same_bytes(o.bufs["obs"][n - 1], full.bufs["obs"][n - 1], "obs of the last step only")
    assert o.bufs["obs"][: n - 1].abs().sum().item() == 0
    # obs offset by 4 bytes on one step, and on all of them (the general obs path)
    for off in ({2}, set(range(n))):
        o = Outs(sw, n, lead=(C,))
        obs = [offset_by_one_float(o.bufs["obs"][j]) if j in off else o.bufs["obs"][j] for j in range(n)]
        sw.score(acts, [dict(kw, obs=obs[j]) for j, kw in enumerate(o.kws())])
        torch.cuda.synchronize()
        same_bytes(torch.stack(obs), full.bufs["obs"], f"obs offset on steps {sorted(off)}")
        same_bytes(o.bufs["reward"], full.bufs["reward"], "reward beside offset obs")
    # action pointers that are only 4-byte aligned, as a list
    o = Outs(sw, n, lead=(C,))
    sw.score([offset_by_one_float(acts[j]) for j in range(n)], o.kws())
    torch.cuda.synchronize()
    for k in OUT_KEYS:
        same_bytes(o.bufs[k], full.bufs[k], k + " with offset actions")
    # every step reads the same action buffer
    o, want = Outs(sw, n, lead=(C,)), Outs(sw, n, lead=(C,))
    sw.score([acts[0]] * n, o.kws())
    sw.score(acts[:1].repeat(n, 1, 1, 1, 1), want.kws())
    torch.cuda.synchronize()
    for k in OUT_KEYS:
        same_bytes(o.bufs[k], want.bufs[k], k + " with one shared action buffer")
    sw.close()


# ------------------------------------------------------------------ 6. depth and refusals
def test_depth_and_refusals_leave_the_swarm_alone():
    sw = QuadSwarm(**C3_SMALL)
    depth = sw.score_depth()
    assert depth == 32
    C, E = 2, sw.num_envs
    acts = make_actions(sw, depth + 1, C)
    ret = torch.zeros((C, E), dtype=torch.float64, device=sw.device)
    with pytest.raises(L.QuadSwarmError, match="rc=-4"):   # QS_E_STATE: before reset
        sw.score(acts[:2], ret=ret)
    sw.reset(3)
    sw.step(None)
    before = fingerprint(sw)
    sw.score(acts[:1], ret=ret)                            # n = 1 works
    sw.score(acts[:depth], ret=ret)                        # and n = depth
    for bad in (lambda: sw.score(acts, ret=ret),                           # n = depth + 1
                lambda: sw.score(acts[:2]),                                # nothing to write
                lambda: sw.score(acts[:2], [{}, {}]),
                lambda: sw.score(acts[:2], ret=acts[0].view(-1).view(torch.float64)[: C * E].view(C, E)),   # ret over actions
                lambda: sw.score(acts[:2], [{"actions_out": acts[3]}, {"actions_out": acts[1]}]),           # an output over step 1's actions
                lambda: sw.score(acts[:2], [{"reward": ret.view(torch.float32).view(-1)[: C * E]}, {}], ret=ret)):   # two outputs overlap
        with pytest.raises(L.QuadSwarmError, match="rc=-1"):
            bad()
    # the C entry itself: C = 0, a NULL among the action pointers, n = 0
    so = L.QsScoreOut(L.ptr(ret), None)
    ptrs = (ctypes.c_void_p * 2)(acts[0].data_ptr(), acts[1].data_ptr())
    assert sw.lib.qs_score(sw._h, 2, 0, ptrs, None, ctypes.byref(so), sw._stream()) == QS_E_INVALID
    assert b"C must be" in sw.lib.qs_last_error()
    assert sw.lib.qs_score(sw._h, 0, C, ptrs, None, ctypes.byref(so), sw._stream()) == QS_E_INVALID
    ptrs = (ctypes.c_void_p * 2)(acts[0].data_ptr(), None)
    assert sw.lib.qs_score(sw._h, 2, C, ptrs, None, ctypes.byref(so), sw._stream()) == QS_E_INVALID
    assert b"actions[1]" in sw.lib.qs_last_error()
    assert sw.lib.qs_score(sw._h, 2, C, None, None, ctypes.byref(so), sw._stream()) == QS_E_INVALID
    # Python-side shape checks
    with pytest.raises(ValueError):
        sw.score(acts[:2, :, :, :, 0], ret=ret)
    with pytest.raises(ValueError):
        sw.score(acts[:2].double(), ret=ret)
    with pytest.raises(ValueError):
        sw.score(acts[:2], ret=ret[:1])
    with pytest.raises(ValueError):
        sw.score(acts[:2], [{"rewards": ret}, {}])
    assert fingerprint(sw) == before
    sw.close()


@pytest.mark.parametrize("cfg,why", [
    (dict(task="multihover", num_drones=4, num_envs=16, act="rpm"), "rejected"),   # the default diagonal layout
    (dict(task="flock", num_drones=4, num_envs=16, act="rpm"), "Flock"),
])
def test_handles_that_cannot_score(cfg, why):
    sw = QuadSwarm(**cfg)
    sw.reset(3)
    assert sw.score_depth() == 0
    before = fingerprint(sw)
    acts = torch.zeros((2, 2, sw.num_envs, sw.num_drones, sw.act_dim), device=sw.device)
    ret = torch.zeros((2, sw.num_envs), dtype=torch.float64, device=sw.device)
    with pytest.raises(L.QuadSwarmError, match="rc=-1.*cannot score.*" + why):
        sw.score(acts, ret=ret)
    assert fingerprint(sw) == before
    sw.close()


def test_depth_follows_the_lds_figures():
    """CF2P RPM (A = 4, history image of 15 slots, 72-float rows): 65 536 - 8 704 - 15 360 - 18 432
    bytes leave 22 steps of 1 024 bytes; QS_MAX_FUSED_STEPS plays no part."""
    sw = QuadSwarm(**CONFIGS["cf2p_d2_rpm"])
    assert sw.score_depth() == 22
    sw.close()


def test_depth_ignores_max_fused_steps(monkeypatch):
    monkeypatch.setenv("QS_MAX_FUSED_STEPS", "4")
    sw = QuadSwarm(**C3_SMALL)
    assert sw.score_depth() == 32
    sw.close()


# ------------------------------------------------------------------------ 7. graphs
def test_captured_score_replays_the_same_bytes():
    n, C = 7, 3
    (sw,) = prepared(C3_SMALL, n, twins=0)
    acts = make_actions(sw, n, C)
    eager, cap = Outs(sw, n, lead=(C,)), Outs(sw, n, lead=(C,))
    ret_e, ret_c = (torch.zeros((C, sw.num_envs), dtype=torch.float64, device=sw.device) for _ in range(2))
    sw.score(acts, eager.kws(), ret=ret_e)
    torch.cuda.synchronize()
    before = fingerprint(sw)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        sw.score(acts, cap.kws(), ret=ret_c)
    for replay in range(2):
        for t in list(cap.bufs.values()) + [ret_c]:
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        for k in OUT_KEYS:
            same_bytes(cap.bufs[k], eager.bufs[k], f"{k}, replay {replay}")
        same_bytes(ret_c, ret_e, "ret")
    assert fingerprint(sw) == before
    sw.close()


def test_score_between_captured_steps_ends_their_node():
    """step, score, step in one capture: the score forgets the kernel node the first step made,
    so the second step is a launch of its own, after the score, and both equal eager steps."""
    n, C = 4, 2
    cap, eager = prepared(C3_SMALL, n)
    acts = make_actions(cap, n, C)
    oc, oe = Outs(cap, 2), Outs(eager, 2)
    ret_c, ret_e = (torch.zeros((C, cap.num_envs), dtype=torch.float64, device=cap.device) for _ in range(2))
    eager.step(None, **oe.kws()[0])
    eager.score(acts, ret=ret_e)
    eager.step(None, **oe.kws()[1])
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap.step(None, **oc.kws()[0])
        cap.score(acts, ret=ret_c)
        cap.step(None, **oc.kws()[1])
    g.replay()
    torch.cuda.synchronize()
    for k in OUT_KEYS:
        same_bytes(oc.bufs[k], oe.bufs[k], k)
    same_bytes(ret_c, ret_e, "ret: scored from the state after the first captured step")
    assert fingerprint(cap) == fingerprint(eager)
    close(cap, eager)


# ----------------------------------------------------------------------- 8. score_t
def test_score_t():
    n, C = 5, 4
    v = SwarmVecEnv(seed=3, **C3_SMALL)
    v.reset_t()
    set_clocks(v.swarm, clocks_for(n))
    ground(v.swarm)
    acts = make_actions(v.swarm, n, C)
    before = fingerprint(v.swarm)
    ret, fd, rew, term, trunc = v.score_t(acts, per_step=True)
    assert rew.shape == (n, C, v.num_envs) and ret.dtype == torch.float64 and fd.dtype == torch.int32
    ret2, fd2 = v.score_t(acts)
    torch.cuda.synchronize()
    wret, wfd = running_score(rew.cpu().numpy(), term.cpu().numpy(), trunc.cpu().numpy())
    assert np.array_equal(ret.cpu().numpy(), wret) and np.array_equal(fd.cpu().numpy(), wfd) and (wfd < n).any()
    same_bytes(ret, ret2, "ret")
    same_bytes(fd, fd2, "first_done")
    assert v.score_t(acts)[0].data_ptr() == ret2.data_ptr()   # the same shape again: the same buffers
    assert fingerprint(v.swarm) == before
    with pytest.raises(ValueError):
        v.score_t(acts[0])
    v.close()
