"""Branch sets: `QuadSwarm.branches(C)` (qs_branch_*) keeps the state of C * E virtual
envs on the device, so branch rollouts can be chained past score_depth(), forked from
the swarm again and resampled, and never changes the swarm.

As in tests/test_gpu_step_score.py the reference is a twin handle: its four state
blocks are restored from a snapshot, then it is stepped with
`step_many(outs, actions=...)` (qs_step_seq).  Everything is compared as raw bytes.

 1. One advance is qs_score_agents.
 2. Chains: depth + 9 steps cut as (depth, 9) and as (7, 7, rest).
 3. Branch state after the chain.
 4. The handle is untouched.
 5. Fork is a snapshot.
 6. Select.
 7. Graph capture.
 8. Refusals.
 9. `BranchSet.rollout` and `SwarmVecEnv.branches`.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from gym_pybullet_drones_amd import _lib as L
from gym_pybullet_drones_amd.envs.swarm import QuadSwarm
from gym_pybullet_drones_amd.vec_env.vec_env import SwarmVecEnv
from test_gpu_step_score import CONFIGS, Outs, ground, make_actions, same_bytes, set_clocks, snapshot

pytestmark = pytest.mark.gpu

C3_SMALL = CONFIGS["mh_d8_onedpid_f32"]
BLOCKS = (L.STATE_AGENT, L.STATE_ENV, L.STATE_HISTORY, L.STATE_EP_RETURN)
SET_BLOCKS = (L.STATE_AGENT, L.STATE_ENV, L.STATE_HISTORY)
OUT_KEYS = ("obs", "reward", "terminated", "truncated", "terminal_obs", "reasons", "actions_out")
QS_E_INVALID, QS_E_STATE = -1, -4


def raw(t):
    return t.cpu().numpy().tobytes() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t).tobytes()


def prep(cfg, clocks, twins=1, seed=3, warm=2):
    """`twins` + 1 swarms in the same mid-episode state: reset, a few random-policy steps,
    env e truncated in step clocks[e mod len] (None: not), and, MultiHover with more than
    four envs, a drone of env 4 on the ground (its env crashes in step 0)."""
    out = [QuadSwarm(**cfg) for _ in range(twins + 1)]
    for sw in out:
        sw.reset(seed)
        for _ in range(warm):
            sw.step(None)
        set_clocks(sw, clocks)
        if sw.task == "multihover" and sw.num_envs > 4:
            ground(sw)
    return out


def fingerprint(sw):
    """Everything a branch call promises to leave alone, as bytes."""
    torch.cuda.synchronize()
    recs, total = sw.episode_log()
    return ([raw(sw.get_state(blk)) for blk in BLOCKS], raw(recs), total, sw.reset_error(), sw.launch_counts(),
            sw.ring_counts())


def set_print(bs):
    """A branch set's state and accumulators, as bytes."""
    torch.cuda.synchronize()
    return ([raw(bs.get_state(blk)) for blk in SET_BLOCKS], raw(bs.ret), raw(bs.first_done), raw(bs.ret_agent), bs.steps)


def restore(ref, snap):
    for blk, val in zip(BLOCKS, snap):
        ref.set_state(blk, val)


def reference(ref, snap, acts):
    """The twin's outputs for every candidate, (n, C, E, ...), from the snapshot each time, and
    its agent / env / history blocks after the n steps, stacked over the candidates like
    `BranchSet.get_state`."""
    n, C = acts.shape[0], acts.shape[1]
    want = Outs(ref, n, lead=(C,))
    blocks = [[] for _ in SET_BLOCKS]
    for c in range(C):
        restore(ref, snap)
        one = Outs(ref, n)
        ref.step_many(one.kws(), actions=acts[:, c])
        torch.cuda.synchronize()
        for k in OUT_KEYS:
            want.bufs[k][:, c] = one.bufs[k]
        for i, blk in enumerate(SET_BLOCKS):
            blocks[i].append(ref.get_state(blk))
    return want, [torch.stack(b, dim=1) for b in blocks]


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


def advance_cut(bs, acts, got, cut):
    j = 0
    for n in cut:
        bs.advance(acts[j:j + n], got.kws()[j:j + n])
        j += n
    assert j == acts.shape[0]


def close(*things):
    for t in things:
        t.close()


# ------------------------------------------------------------ 1. one advance is qs_score_agents
@pytest.mark.parametrize("n", [7, None])   # None: score_depth()
@pytest.mark.parametrize("name", list(CONFIGS))
def test_one_advance_is_score_agents(name, n):
    C = 3
    probe = QuadSwarm(**CONFIGS[name])
    depth = probe.score_depth()
    probe.close()
    n = depth if n is None else n
    (sw,) = prep(CONFIGS[name], (0, n // 2, n - 1, None, 1, min(5, n - 1)), twins=0)
    E, D = sw.num_envs, sw.num_drones
    acts = make_actions(sw, n, C)
    want, got = Outs(sw, n, lead=(C,)), Outs(sw, n, lead=(C,))
    ret = torch.full((C, E), -7.0, dtype=torch.float64, device=sw.device)
    fd = torch.full((C, E), -7, dtype=torch.int32, device=sw.device)
    ra = torch.full((C, E, D), -7.0, dtype=torch.float64, device=sw.device)
    sw.score(acts, want.kws(), ret=ret, first_done=fd, ret_agent=ra)
    bs = sw.branches(C)
    bs.fork()
    assert bs.steps == 0
    bs.advance(acts, got.kws())
    torch.cuda.synchronize()
    assert bs.steps == n
    for k in OUT_KEYS:
        same_bytes(want.bufs[k], got.bufs[k], k)
    same_bytes(ret, bs.ret, "ret")
    same_bytes(fd, bs.first_done, "first_done")
    same_bytes(ra, bs.ret_agent, "ret_agent")
    f = fd.cpu().numpy()
    assert (f == 0).any() and (f < n).any()
    close(bs, sw)


# ------------------------------------------------------------ 2. / 3. chains and the state after them
CUTS = ("depth_9", "7_7_rest")


@functools.lru_cache(maxsize=None)
def chain_case(name):
    """depth + 9 steps of C = 3 candidates on config `name`, cut both ways, and the twin's
    reference, all on the host: computed once, shared by the tests below, never changed."""
    cfg, C = CONFIGS[name], 3
    probe = QuadSwarm(**cfg)
    depth = probe.score_depth()
    probe.close()
    total = depth + 9
    # truncations inside the first chunk (3), on the last step of a chunk (depth - 1; 6 and 13 of
    # the other cut), on the first step of the next (depth; 7 and 14), in the last chunk
    # (total - 2), and none (env 4 is the grounded one where there is one: it crashes in step 0)
    clocks = (3, depth - 1, depth, total - 2, None, 6, 7, None, 13, 14)
    sw, ref = prep(cfg, clocks)
    acts = make_actions(sw, total, C)
    snap = snapshot(sw)
    before = fingerprint(sw)
    want, want_state = reference(ref, snap, acts)
    res = dict(depth=depth, total=total, E=sw.num_envs, autoreset=cfg.get("autoreset", True),
               want={k: want.bufs[k].cpu().numpy() for k in OUT_KEYS}, want_state=[b.cpu().numpy() for b in want_state])
    for label, cut in zip(CUTS, ((depth, 9), (7, 7, total - 14))):
        bs = sw.branches(C)
        bs.fork()
        got = Outs(sw, total, lead=(C,))
        advance_cut(bs, acts, got, cut)
        torch.cuda.synchronize()
        res[label] = dict(outs={k: got.bufs[k].cpu().numpy() for k in OUT_KEYS},
                          state=[bs.get_state(blk).cpu().numpy() for blk in SET_BLOCKS],
                          ret=bs.ret.cpu().numpy().copy(), fd=bs.first_done.cpu().numpy().copy(),
                          ra=bs.ret_agent.cpu().numpy().copy(), steps=bs.steps)
        bs.close()
    res["untouched"] = fingerprint(sw) == before
    close(sw, ref)
    return res


@pytest.mark.parametrize("name", list(CONFIGS))
def test_chains_equal_the_twins_sequence(name):
    r = chain_case(name)
    total, depth = r["total"], r["depth"]
    for label in CUTS:
        g = r[label]
        assert g["steps"] == total
        for k in OUT_KEYS:
            same_bytes(r["want"][k], g["outs"][k], f"{label}: {k}")
    a, b = (r[label] for label in CUTS)
    for k in OUT_KEYS:
        same_bytes(a["outs"][k], b["outs"][k], k + ": the two cuts")
    for k in ("ret", "fd", "ra"):
        same_bytes(a[k], b[k], k + ": the two cuts")
    rew, t, u = (r["want"][k] for k in ("reward", "terminated", "truncated"))
    wret, wfd = running_score(rew, t, u)
    assert raw(a["ret"]) == raw(wret) and np.array_equal(a["fd"], wfd)
    assert r["untouched"]
    # what the clocks were set for (the configs whose episodes do not end early for other reasons)
    if name.startswith("mh_d8"):
        for step in (3, depth - 1, depth, total - 2):
            assert u[step].any(), step
        assert t[0, :, 4].all() and (wfd[:, 4] == 0).all()          # the grounded drone's env
        period = 10                                                  # len(clocks) in chain_case
        for at, first in ((3, 0), (depth - 1, 1), (depth, 2), (total - 2, 3)):
            assert (wfd[:, first::period] == at).any(), at           # first done where the clock says
        if r["E"] > 7:
            assert (wfd[:, 7::period] == total).any()                # an env that is never done
            for at, first in ((6, 5), (7, 6)):
                assert (wfd[:, first::period] == at).any(), at
    if not r["autoreset"]:
        assert ((t | u).sum(axis=0) > 1).any()   # done more than once: only the first counts


@pytest.mark.parametrize("name", list(CONFIGS))
def test_branch_state_after_the_chain(name):
    r = chain_case(name)
    for label in CUTS:
        for blk, want, got in zip(("agent", "env", "history"), r["want_state"], r[label]["state"]):
            same_bytes(want, got, f"{label}: {blk} block")


# ------------------------------------------------------------------ 4. the handle is untouched
def test_handle_is_untouched_and_steps_on():
    n, C = 9, 4
    sw, never = prep(C3_SMALL, (0, 4, 8, None, 1, 5))
    acts = make_actions(sw, n, C)
    before = fingerprint(sw)
    assert before == fingerprint(never)
    bs = sw.branches(C)
    parent = torch.tensor([[1], [0], [3], [9]], dtype=torch.int32).repeat(1, sw.num_envs).to(sw.device)
    for _ in range(2):
        bs.fork()
        bs.advance(acts)
        bs.select(parent)
        bs.advance(acts[:3])
    torch.cuda.synchronize()
    assert (bs.first_done.cpu().numpy() < n + 3).any()
    assert fingerprint(sw) == before
    for blk in SET_BLOCKS:
        bs.get_state(blk)
    assert fingerprint(sw) == before
    o1, o2 = Outs(sw, n), Outs(never, n)
    sw.step_many(o1.kws(), actions=acts[:, 1])
    never.step_many(o2.kws(), actions=acts[:, 1])
    torch.cuda.synchronize()
    for k in OUT_KEYS:
        same_bytes(o1.bufs[k], o2.bufs[k], k)
    assert fingerprint(sw) == fingerprint(never) != before
    close(bs, sw, never)


# ------------------------------------------------------------------ 5. fork is a snapshot
def test_fork_is_a_snapshot():
    n, C = 7, 3
    sw, ref = prep(C3_SMALL, (0, 3, 6, None, 1, 5))
    acts = make_actions(sw, n, C)
    bs = sw.branches(C)
    snap = snapshot(sw)
    bs.fork()
    for _ in range(2):
        sw.step(None)
    got = Outs(sw, n, lead=(C,))
    bs.advance(acts, got.kws())
    torch.cuda.synchronize()
    want, want_state = reference(ref, snap, acts)
    for k in OUT_KEYS:
        same_bytes(want.bufs[k], got.bufs[k], k + ": from the fork-time state")
    for blk, w in zip(SET_BLOCKS, want_state):
        same_bytes(w, bs.get_state(blk), f"block {blk}")
    assert bs.steps == n and bs.ret.abs().sum().item() > 0
    # a second fork: steps and accumulators zeroed, the new state taken
    snap2 = snapshot(sw)
    assert raw(snap2[0]) != raw(snap[0])
    bs.fork()
    torch.cuda.synchronize()
    assert bs.steps == 0
    assert not bs.ret.any().item() and not bs.first_done.any().item() and not bs.ret_agent.any().item()
    assert raw(bs.ret) == bytes(bs.ret.numel() * 8)   # +0.0, not -0.0
    for blk, s in zip(SET_BLOCKS, snap2):
        same_bytes(torch.stack([s] * C, dim=1), bs.get_state(blk), f"block {blk} after the second fork")
    got2 = Outs(sw, n, lead=(C,))
    bs.advance(acts, got2.kws())
    torch.cuda.synchronize()
    want2, _ = reference(ref, snap2, acts)
    for k in OUT_KEYS:
        same_bytes(want2.bufs[k], got2.bufs[k], k + ": from the second fork's state")
    close(bs, sw, ref)


# ------------------------------------------------------------------------------ 6. select
def test_select_regroups_state_and_accumulators():
    n1, n2, C = 5, 6, 4
    sw, ref = prep(C3_SMALL, (0, 2, 4, None, 1, 7, 9, n1 + n2 - 1))
    E = sw.num_envs
    acts = make_actions(sw, n1, C)
    acts2 = make_actions(sw, n2, C, seed=11)
    rows = ([0, 1, 2, 3],      # identity
            [2, 2, 0, 2],      # a duplicated parent
            [1, 2, 3, 0],      # a permutation
            [0, 7, -1, 1])     # out of range twice: those candidates stay
    parent = torch.tensor([rows[e % 4] for e in range(E)], dtype=torch.int32).t().contiguous()   # (C, E)
    eff = parent.clone()
    for c in range(C):
        eff[c][(parent[c] < 0) | (parent[c] >= C)] = c
    snap = snapshot(sw)
    bs = sw.branches(C)
    bs.fork()
    bs.advance(acts)
    torch.cuda.synchronize()
    old_state = [bs.get_state(blk).cpu() for blk in SET_BLOCKS]
    old_acc = [bs.ret.cpu().clone(), bs.first_done.cpu().clone(), bs.ret_agent.cpu().clone()]
    ptrs = [t.data_ptr() for t in (bs.ret, bs.first_done, bs.ret_agent)]
    bs.select(parent.to(sw.device))
    torch.cuda.synchronize()
    assert bs.steps == n1
    assert ptrs == [t.data_ptr() for t in (bs.ret, bs.first_done, bs.ret_agent)]
    # state and accumulators are the parents'
    D = sw.num_drones
    idx_e = eff.long()                                        # (C, E)
    idx_a = idx_e.repeat_interleave(D, dim=1)                 # (C, E * D)
    agent, env, hist = old_state
    same_bytes(torch.gather(agent, 1, idx_a.unsqueeze(0).expand_as(agent)), bs.get_state(L.STATE_AGENT), "agent block")
    same_bytes(torch.gather(env, 1, idx_e.unsqueeze(0).expand_as(env)), bs.get_state(L.STATE_ENV), "env block")
    same_bytes(torch.gather(hist, 1, idx_a.unsqueeze(0).unsqueeze(-1).expand_as(hist)), bs.get_state(L.STATE_HISTORY),
               "history block")
    same_bytes(torch.gather(old_acc[0], 0, idx_e), bs.ret, "ret")
    same_bytes(torch.gather(old_acc[1], 0, idx_e), bs.first_done, "first_done")
    same_bytes(torch.gather(old_acc[2], 0, idx_e.unsqueeze(-1).expand_as(old_acc[2])), bs.ret_agent, "ret_agent")
    # a further advance equals twins that replay the parent's prefix and then the new actions
    got = Outs(sw, n2, lead=(C,))
    bs.advance(acts2, got.kws())
    torch.cuda.synchronize()
    assert bs.steps == n1 + n2
    ar = torch.arange(E)
    prefix = torch.stack([acts.cpu()[:, eff[c].long(), ar] for c in range(C)], dim=1)   # (n1, C, E, D, A)
    full = torch.cat([prefix.to(sw.device), acts2], dim=0).contiguous()
    want, want_state = reference(ref, snap, full)
    for k in OUT_KEYS:
        same_bytes(want.bufs[k][n1:], got.bufs[k], k + " after select")
    for blk, w in zip(SET_BLOCKS, want_state):
        same_bytes(w, bs.get_state(blk), f"block {blk} after select and advance")
    wret, wfd = running_score(*(want.bufs[k].cpu().numpy() for k in ("reward", "terminated", "truncated")))
    assert raw(bs.ret) == raw(wret) and np.array_equal(bs.first_done.cpu().numpy(), wfd)
    assert (wfd < n1).any() and ((wfd >= n1) & (wfd < n1 + n2)).any() and (wfd == n1 + n2).any()
    close(bs, sw, ref)


# ------------------------------------------------------------------------------ 7. capture
def test_captured_fork_advance_select_advance_replays():
    n1, n2, C = 5, 4, 3
    (sw,) = prep(C3_SMALL, (0, 2, 4, None, 1, 6, 8), twins=0)
    E = sw.num_envs
    acts = make_actions(sw, n1 + n2, C)
    parent = torch.tensor([[1, 2, 0][(c + e) % 3] if e % 2 else c for c in range(C) for e in range(E)],
                          dtype=torch.int32).view(C, E).to(sw.device)
    eager, cap = sw.branches(C), sw.branches(C)
    oe, oc = Outs(sw, n1 + n2, lead=(C,)), Outs(sw, n1 + n2, lead=(C,))

    def run(bs, o):
        bs.fork()
        bs.advance(acts[:n1], o.kws()[:n1])
        bs.select(parent)
        bs.advance(acts[n1:], o.kws()[n1:])

    run(eager, oe)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run(cap, oc)
    views = [cap.ret, cap.first_done, cap.ret_agent]
    ptrs = [t.data_ptr() for t in views]
    for replay in range(2):
        if replay:
            for _ in range(2):
                sw.step(None)                      # the handle moves on between the replays
            for t in oe.bufs.values():
                t.zero_()
            run(eager, oe)
        for t in oc.bufs.values():
            t.zero_()
        before = fingerprint(sw)
        g.replay()
        torch.cuda.synchronize()
        for k in OUT_KEYS:
            same_bytes(oe.bufs[k], oc.bufs[k], f"{k}, replay {replay}")
        for a, b, what in zip((eager.ret, eager.first_done, eager.ret_agent), views, ("ret", "first_done", "ret_agent")):
            same_bytes(a, b, f"{what}, replay {replay}")
        for blk in SET_BLOCKS:
            same_bytes(eager.get_state(blk), cap.get_state(blk), f"block {blk}, replay {replay}")
        assert fingerprint(sw) == before
    assert ptrs == [t.data_ptr() for t in (cap.ret, cap.first_done, cap.ret_agent)]
    first = raw(oc.bufs["obs"])
    assert first != bytes(len(first))
    close(eager, cap, sw)


# ------------------------------------------------------------------------------ 8. refusals
@pytest.mark.parametrize("cfg,why", [
    (dict(task="multihover", num_drones=4, num_envs=16, act="rpm"), "rejected"),   # the deferred reset search
    (dict(task="flock", num_drones=4, num_envs=16, act="rpm"), "Flock"),
])
def test_handles_that_cannot_score_get_no_branch_set(cfg, why):
    sw = QuadSwarm(**cfg)
    sw.reset(3)
    assert sw.score_depth() == 0
    before = fingerprint(sw)
    with pytest.raises(L.QuadSwarmError, match="rc=-1.*cannot score.*" + why):
        sw.branches(2)
    out = ctypes.c_void_p(4321)
    assert sw.lib.qs_branch_create(sw._h, 2, ctypes.byref(out)) == QS_E_INVALID and out.value == 4321
    assert fingerprint(sw) == before
    sw.close()


def test_refusals_leave_the_handle_and_the_set_alone():
    C = 2
    sw = QuadSwarm(**C3_SMALL)
    E, D = sw.num_envs, sw.num_drones
    depth = sw.score_depth()
    acts = make_actions(sw, depth + 1, C)
    out = ctypes.c_void_p(4321)
    for bad_c in (0, -3, (1 << 31) // (E * D) + 1, (1 << 31) - 1):   # C < 1; C * E * D at 2^31 and far past it
        with pytest.raises(L.QuadSwarmError, match="rc=-1"):
            sw.branches(bad_c)
        assert sw.lib.qs_branch_create(sw._h, bad_c, ctypes.byref(out)) == QS_E_INVALID and out.value == 4321
    assert b"32-bit" in sw.lib.qs_last_error()
    bs = sw.branches(C)
    with pytest.raises(L.QuadSwarmError, match="rc=-4"):   # QS_E_STATE: fork before qs_reset
        bs.fork()
    sw.reset(3)
    sw.step(None)
    with pytest.raises(L.QuadSwarmError, match="rc=-4"):   # advance and select before the first fork
        bs.advance(acts[:2])
    with pytest.raises(L.QuadSwarmError, match="rc=-4"):
        bs.select(torch.zeros((C, E), dtype=torch.int32, device=sw.device))
    bs.fork()
    bs.advance(acts[:3])
    before, before_set = fingerprint(sw), set_print(bs)
    rew = torch.zeros((C, E), dtype=sw.rdtype, device=sw.device)
    for bad in (lambda: bs.advance(acts),                                                        # n = depth + 1
                lambda: bs.advance(acts[:2], [{"actions_out": acts[3]}, {"actions_out": acts[1]}]),   # an output over step 1's actions
                lambda: bs.advance(acts[:2], [{"reward": rew}, {"reward": rew}]),                   # two outputs overlap
                lambda: bs.advance(acts[:2], [{"reward": bs.ret.view(sw.rdtype)}, {}])):            # an output inside the set
        with pytest.raises(L.QuadSwarmError, match="rc=-1"):
            bad()
    ptrs = (ctypes.c_void_p * 2)(acts[0].data_ptr(), None)
    assert sw.lib.qs_branch_advance(bs._p, 2, ptrs, None, sw._stream()) == QS_E_INVALID      # a NULL among actions[]
    assert b"actions[1]" in sw.lib.qs_last_error()
    assert sw.lib.qs_branch_advance(bs._p, 0, ptrs, None, sw._stream()) == QS_E_INVALID      # n = 0
    assert sw.lib.qs_branch_advance(bs._p, 2, None, None, sw._stream()) == QS_E_INVALID
    assert sw.lib.qs_branch_select(bs._p, None, sw._stream()) == QS_E_INVALID
    buf = torch.zeros(C * E, dtype=torch.float64, device=sw.device)
    assert sw.lib.qs_branch_state(bs._p, L.STATE_EP_RETURN, L.ptr(buf), sw._stream()) == QS_E_INVALID
    # Python-side shape checks
    with pytest.raises(ValueError):
        bs.advance(acts[:2, :1])
    with pytest.raises(ValueError):
        bs.advance(acts[:2].double())
    with pytest.raises(ValueError):
        bs.advance(acts[:2], [{"rewards": rew}, {}])
    with pytest.raises(ValueError):
        bs.select(torch.zeros((C, E), dtype=torch.int64, device=sw.device))
    with pytest.raises(ValueError):
        bs.get_state(L.STATE_EP_RETURN)
    assert fingerprint(sw) == before and set_print(bs) == before_set
    bs.advance(acts[:depth])            # n = depth works, and outs = None is valid
    assert bs.steps == 3 + depth
    close(bs, sw)


# ------------------------------------------------------- 9. rollout and SwarmVecEnv.branches
def test_rollout_and_vec_env_branches():
    C = 3
    v = SwarmVecEnv(seed=3, **C3_SMALL)
    v.reset_t()
    sw = v.swarm
    depth = sw.score_depth()
    n = 2 * depth + 3
    set_clocks(sw, (2, depth - 1, depth, 2 * depth, None, n - 1, depth + 5))
    ground(sw)
    ref = QuadSwarm(**C3_SMALL)
    ref.reset(3)
    acts = make_actions(sw, n, C)
    snap = snapshot(sw)
    before = fingerprint(sw)
    a, b = v.branches(C), v.branches(C)
    oa, ob = Outs(sw, n, lead=(C,)), Outs(sw, n, lead=(C,))
    a.fork()
    a.rollout(acts, oa.kws())
    b.fork()
    advance_cut(b, acts, ob, (depth, depth, 3))
    torch.cuda.synchronize()
    assert a.steps == b.steps == n
    want, want_state = reference(ref, snap, acts)
    for k in OUT_KEYS:
        same_bytes(want.bufs[k], oa.bufs[k], k + ": rollout against the twin")
        same_bytes(ob.bufs[k], oa.bufs[k], k + ": rollout against explicit advances")
    assert set_print(a) == set_print(b)
    for blk, w in zip(SET_BLOCKS, want_state):
        same_bytes(w, a.get_state(blk), f"block {blk}")
    wret, wfd = running_score(*(want.bufs[k].cpu().numpy() for k in ("reward", "terminated", "truncated")))
    assert raw(a.ret) == raw(wret) and np.array_equal(a.first_done.cpu().numpy(), wfd)
    assert (wfd == 0).any() and (wfd == depth - 1).any() and (wfd >= depth).any()
    c = v.branches(C)                   # without outputs, as a list of per-step tensors
    c.fork()
    c.rollout([acts[j] for j in range(n)])
    assert set_print(c) == set_print(a)
    assert fingerprint(sw) == before
    close(a, b, c, ref)
    v.close()
