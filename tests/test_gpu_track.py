"""Tracking cost: `QuadSwarm.score(..., track=, cost_agent=)` (qs_track_score) is the score launch
that also sums, per drone, a quadratic cost against a caller-supplied reference, and
qs_track_fold turns ret / ret_agent and that cost into the objective.

The state preparation, the actions and the twin are those of tests/test_gpu_step_score.py;
the spec and the float64 restatements are tests/track_case.py.  The spec under test has
L = 3 rows (below every n but 1: the clamp bites), a distinct row base per env from a
negative one to one past L, zeros and a -0.0 among q, a non-zero r and terminal = 2.5.

 1. cost_agent equals, as bytes, the NumPy float64 loop fed with the same launch's obs,
    terminal_obs, terminated, truncated and actions_out.
 2. Every other output equals qs_score_agents on a twin swarm, as bytes, and the swarm's
    fingerprint (state blocks, episode log, reset error, launch counts) is unchanged.
 3. Two calls give the same bytes; with q = r = 0 cost_agent is all +0.0.
 4. qs_track_fold against the NumPy formula as bytes, for both forms.
 5. Refusals, each with the entry point's name in the message and nothing written.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from gym_pybullet_drones_amd import _lib as L
from gym_pybullet_drones_amd.envs.swarm import QuadSwarm
from test_gpu_step_score import (OUT_KEYS, Outs, clocks_for, close, fingerprint, ground, make_actions, prepared, raw,
                                 set_clocks)
from track_case import CONFIGS, Q, R, ROWS, TERMINAL, cost_reference, fold_reference, make_spec

pytestmark = pytest.mark.gpu

C = 3
STEPS = (1, 5, None)   # None: score_depth()
QS_E_INVALID, QS_E_STATE = -1, -4


def steps_of(cfg, n):
    if n is not None:
        return n
    probe = QuadSwarm(**cfg)
    n = probe.score_depth()
    probe.close()
    return n


@functools.lru_cache(maxsize=None)
def launch(name, n):
    """One qs_track_score launch and its twin's qs_score_agents launch, everything on the host:
    (tracked outputs, twin outputs, spec tensors, fingerprints before and after)."""
    cfg = CONFIGS[name]
    n = steps_of(cfg, n)
    sw, twin = prepared(cfg, n)
    assert 1 <= n <= sw.score_depth() <= 32
    acts = make_actions(sw, n, C)
    track = make_spec(sw)
    assert track[0].L == ROWS and (n == 1 or ROWS < n)
    before = fingerprint(sw)

    def run(s, track=None):
        o = Outs(s, n, lead=(C,))
        own = dict(ret=torch.full((C, s.num_envs), -7.0, dtype=torch.float64, device=s.device),
                   first_done=torch.full((C, s.num_envs), -7, dtype=torch.int32, device=s.device),
                   ret_agent=torch.full((C, s.num_envs, s.num_drones), -7.0, dtype=torch.float64, device=s.device))
        if track is not None:
            own["cost_agent"] = torch.full((C, s.num_envs, s.num_drones), -7.0, dtype=torch.float64, device=s.device)
        s.score(acts, o.kws(), track=track, **own)
        torch.cuda.synchronize()
        res = {k: v.cpu().numpy() for k, v in o.bufs.items()}
        res.update({k: v.cpu().numpy() for k, v in own.items()})
        return res

    got = run(sw, track)
    again = run(sw, track)
    zero = run(sw, make_spec(sw, zero=True))
    after = fingerprint(sw)
    want = run(twin)
    ref, base = (t.cpu().numpy() for t in track[1])
    close(sw, twin)
    return dict(n=n, got=got, again=again, zero=zero, want=want, ref=ref, base=base, before=before, after=after)


def ends(r):
    """Some (c, e) ends inside the horizon and some does not."""
    fd = r["got"]["first_done"]
    assert (fd < r["n"]).any() and (fd == r["n"]).any()


# ------------------------------------------------------------------ 1. the cost
@pytest.mark.parametrize("n", STEPS)
@pytest.mark.parametrize("name", list(CONFIGS))
def test_cost_equals_the_float64_loop_as_bytes(name, n):
    r = launch(name, n)
    ends(r)
    g = r["got"]
    want = cost_reference(g["obs"], g["terminal_obs"], g["terminated"], g["truncated"], g["actions_out"], r["ref"],
                          r["base"], Q, R, TERMINAL)
    assert want.dtype == np.float64 and want.shape == g["cost_agent"].shape
    assert np.isfinite(want).all() and (want > 0).any()
    assert raw(want) == raw(g["cost_agent"])


# ------------------------------------------------------------------ 2. everything else
@pytest.mark.parametrize("n", STEPS)
@pytest.mark.parametrize("name", list(CONFIGS))
def test_other_outputs_are_score_agents_and_the_swarm_is_unchanged(name, n):
    r = launch(name, n)
    ends(r)
    for k in OUT_KEYS + ("ret", "first_done", "ret_agent"):
        assert r["got"][k].shape == r["want"][k].shape and raw(r["got"][k]) == raw(r["want"][k]), k
    assert r["before"] == r["after"]


# ------------------------------------------------------------------ 3. repeatable, and zero weights
@pytest.mark.parametrize("n", STEPS)
@pytest.mark.parametrize("name", list(CONFIGS))
def test_two_calls_agree_and_zero_weights_cost_nothing(name, n):
    r = launch(name, n)
    ends(r)
    for k in r["got"]:
        assert raw(r["got"][k]) == raw(r["again"][k]), k
    zero = r["zero"]["cost_agent"]
    assert raw(zero) == raw(np.zeros(zero.shape, np.float64))   # +0.0, every one
    for k in r["got"]:
        if k != "cost_agent":
            assert raw(r["got"][k]) == raw(r["zero"][k]), k


# ------------------------------------------------------------------ 4. the fold
@pytest.mark.parametrize("shape", [(3, 21, 8), (5, 13, 5), (2, 700, 3)])
@pytest.mark.parametrize("scale", [1.0, 0.0, -0.375])
def test_fold_equals_the_numpy_formula_as_bytes(shape, scale):
    lib = L.load()
    Cc, E, D = shape
    rng = np.random.default_rng(7)
    ret = rng.normal(size=(Cc, E)) * 10
    ret_agent = rng.normal(size=(Cc, E, D)) * 10
    cost = rng.random((Cc, E, D)) * 50
    cost[0, 0] = 0.0
    dev = torch.device("cuda", 0)
    d_cost = torch.from_numpy(cost).to(dev)
    want_ret, want_agent = fold_reference(scale, ret, ret_agent, cost)
    for with_ret, with_agent in ((True, True), (True, False), (False, True)):
        d_ret, d_agent = torch.from_numpy(ret).to(dev), torch.from_numpy(ret_agent).to(dev)
        rc = lib.qs_track_fold(Cc, E, D, scale, L.ptr(d_ret) if with_ret else None, L.ptr(d_agent) if with_agent else None,
                               L.ptr(d_cost), None)
        assert rc == 0, lib.qs_last_error()
        torch.cuda.synchronize()
        assert raw(d_ret) == raw(want_ret if with_ret else ret)
        assert raw(d_agent) == raw(want_agent if with_agent else ret_agent)
        assert raw(d_cost) == raw(cost)
    # refusals: nothing to fold, no cost, a non-finite scale, an empty shape
    d_ret = torch.from_numpy(ret).to(dev)
    for args in ((Cc, E, D, scale, None, None, L.ptr(d_cost)), (Cc, E, D, scale, L.ptr(d_ret), None, None),
                 (Cc, E, D, float("nan"), L.ptr(d_ret), None, L.ptr(d_cost)),
                 (Cc, E, D, float("inf"), L.ptr(d_ret), None, L.ptr(d_cost)),
                 (0, E, D, scale, L.ptr(d_ret), None, L.ptr(d_cost)), (Cc, E, 0, scale, L.ptr(d_ret), None, L.ptr(d_cost))):
        assert lib.qs_track_fold(*args, None) == QS_E_INVALID
        assert b"qs_track_fold" in lib.qs_last_error()
    torch.cuda.synchronize()
    assert raw(d_ret) == raw(ret)


# ------------------------------------------------------------------ 5. refusals
def test_refusals_name_the_entry_point_and_write_nothing():
    cfg = CONFIGS["mh_d3_vel_pyb"]   # A = 4: every r[a] is read
    n = 5
    sw, = prepared(cfg, n, twins=0)
    lib, E, D = sw.lib, sw.num_envs, sw.num_drones
    acts = make_actions(sw, n, C)
    before = fingerprint(sw)
    good, keep = make_spec(sw)
    cost = torch.full((C, E, D), -7.0, dtype=torch.float64, device=sw.device)
    ret_agent = torch.full((C, E, D), -7.0, dtype=torch.float64, device=sw.device)
    ret = torch.full((C, E), -7.0, dtype=torch.float64, device=sw.device)
    ptrs = (ctypes.c_void_p * n)(*[acts[j].data_ptr() for j in range(n)])
    so = L.QsScoreOut(L.ptr(ret), None)
    untouched = [raw(t) for t in (cost, ret_agent, ret, acts)]

    def call(spec, handle=None, cost_ptr=cost.data_ptr(), agent_ptr=ret_agent.data_ptr()):
        return lib.qs_track_score(sw._h if handle is None else handle, n, C, ptrs, None, ctypes.byref(so), agent_ptr,
                                  ctypes.byref(spec) if spec is not None else None, cost_ptr, sw._stream())

    def variant(**kw):
        s = L.QsTrackSpec.from_buffer_copy(good)
        for k, v in kw.items():
            if isinstance(v, tuple):   # (index, value) of an array member
                getattr(s, k)[v[0]] = v[1]
            else:
                setattr(s, k, v)
        return s

    def refused(rc, code=QS_E_INVALID):
        assert rc == code, (rc, lib.qs_last_error())
        assert b"qs_track_score" in lib.qs_last_error()
        torch.cuda.synchronize()
        assert [raw(t) for t in (cost, ret_agent, ret, acts)] == untouched

    assert call(good) == 0, lib.qs_last_error()   # the spec itself is fine
    torch.cuda.synchronize()
    assert not (cost == -7.0).any()
    cost.fill_(-7.0); ret_agent.fill_(-7.0); ret.fill_(-7.0)
    torch.cuda.synchronize()
    nan, inf = float("nan"), float("inf")
    bad = [variant(q=(0, -1e-30)), variant(q=(11, nan)), variant(q=(5, inf)), variant(r=(0, -0.5)), variant(r=(3, nan)),
           variant(r=(2, inf)), variant(terminal=-1.0), variant(terminal=inf), variant(terminal=nan),
           variant(reward_scale=nan), variant(reward_scale=inf), variant(reward_scale=-inf), variant(L=0), variant(L=-3),
           variant(ref=None), variant(ref=good.ref + 4), variant(ref=good.ref + 8),
           # the 32-bit bound: the first L whose L · E · D · 48 bytes reach 2^31 (refused before anything is read)
           variant(L=-(-(1 << 31) // (E * D * 48)))]
    for s in bad:
        refused(call(s))
    ok_rows = ((1 << 31) - 1) // (E * D * 48)
    assert ok_rows * E * D * 48 < (1 << 31) <= (ok_rows + 1) * E * D * 48 and bad[-1].L == ok_rows + 1
    refused(call(None))                                   # no spec
    refused(call(good, cost_ptr=None))                    # no cost_agent
    refused(call(good, cost_ptr=ret_agent.data_ptr()))    # cost_agent on an output
    refused(call(good, cost_ptr=ret.data_ptr()))          # ... on another, partly
    refused(call(good, cost_ptr=acts[n - 1].data_ptr()))  # ... on an action buffer
    refused(lib.qs_track_score(None, n, C, ptrs, None, ctypes.byref(so), None, ctypes.byref(good), cost.data_ptr(), None))
    assert fingerprint(sw) == before

    # a Flock handle cannot score; a MultiHover one not before its reset
    flock = QuadSwarm(task="flock", num_envs=E, num_drones=D, act="rpm")
    flock.reset(1)
    refused(call(good, handle=flock._h))
    fresh = QuadSwarm(**cfg)
    refused(call(good, handle=fresh._h), QS_E_STATE)
    close(sw, flock, fresh)


def test_vec_env_score_t_returns_the_cost():
    from gym_pybullet_drones_amd.vec_env.vec_env import SwarmVecEnv
    n = 5
    v = SwarmVecEnv(seed=3, **CONFIGS["mh_d8_onedpid_f32"])
    v.reset_t()
    set_clocks(v.swarm, clocks_for(n))
    ground(v.swarm)
    acts = make_actions(v.swarm, n, C)
    track = make_spec(v.swarm)
    before = fingerprint(v.swarm)
    ret, fd, ret_agent, cost = (t.clone() for t in v.score_t(acts, per_drone=True, track=track))
    plain = v.score_t(acts, per_drone=True)
    torch.cuda.synchronize()
    assert len(plain) == 3 and cost.shape == ret_agent.shape and cost.dtype == torch.float64
    for got, want, k in zip((ret, fd, ret_agent), plain, ("ret", "first_done", "ret_agent")):
        assert raw(got) == raw(want), k
    own = torch.zeros_like(cost)
    v.swarm.score(acts, track=track, cost_agent=own)
    torch.cuda.synchronize()
    assert raw(own) == raw(cost) and (cost > 0).any() and ((fd < n).any() and (fd == n).any())
    assert fingerprint(v.swarm) == before
    with pytest.raises(ValueError):
        v.swarm.score(acts, track=track)   # track without cost_agent
    v.close()
