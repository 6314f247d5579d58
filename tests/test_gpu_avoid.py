"""Separation and obstacle terms: `QuadSwarm.score(..., avoid=, cost_agent=)` (qs_avoid_score) is
the tracking score launch whose cost also holds a pairwise hinge among an env's drones and one
against every row of a caller-supplied obstacle table, with or without a tracking spec.

The state preparation, the actions and the twins are those of tests/test_gpu_step_score.py and
tests/test_gpu_track.py; the spec and the float64 restatement are tests/avoid_case.py.

 1. cost_agent equals, as bytes, the NumPy float64 loop fed with the same launch's obs,
    terminal_obs, terminated, truncated and actions_out: with a tracking spec, with track = NULL,
    and with the all-off avoidance spec against qs_track_score on a twin swarm.
 2. Every other output equals qs_track_score (without a tracking spec: qs_score_agents) on a
    twin, as bytes, and the swarm's fingerprint is unchanged.
 3. The reference itself takes both branches of both hinges (a kernel that skips one cannot pass).
 4. M = 16, M = 0 and each switch on its own.
 5. Refusals, each with the entry point's name in the message and nothing written.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from gym_pybullet_drones_amd import _lib as L
from gym_pybullet_drones_amd.envs.swarm import QuadSwarm, avoid_spec
from avoid_case import (CONFIGS, DEFAULT_SEED, SEEDS, SEP_WEIGHT, SEP_Z_SCALE, avoid_reference, cost_reference, make_avoid,
                        many_rows, numbers_for)
from test_gpu_step_score import (OUT_KEYS, Outs, clocks_for, close, fingerprint, ground, make_actions, prepared, raw,
                                 set_clocks)
from track_case import Q, R, TERMINAL, make_spec

pytestmark = pytest.mark.gpu

C = 3
STEPS = (1, 5, None)   # None: score_depth()
QS_E_INVALID, QS_E_STATE = -1, -4
OTHERS = OUT_KEYS + ("ret", "first_done", "ret_agent")


def steps_of(cfg, n):
    if n is not None:
        return n
    probe = QuadSwarm(**cfg)
    n = probe.score_depth()
    probe.close()
    return n


def run(s, n, acts, track=None, avoid=None):
    """One score launch with every output, on the host."""
    o = Outs(s, n, lead=(C,))
    own = dict(ret=torch.full((C, s.num_envs), -7.0, dtype=torch.float64, device=s.device),
               first_done=torch.full((C, s.num_envs), -7, dtype=torch.int32, device=s.device),
               ret_agent=torch.full((C, s.num_envs, s.num_drones), -7.0, dtype=torch.float64, device=s.device))
    if track is not None or avoid is not None:
        own["cost_agent"] = torch.full((C, s.num_envs, s.num_drones), -7.0, dtype=torch.float64, device=s.device)
    s.score(acts, o.kws(), track=track, avoid=avoid, **own)
    torch.cuda.synchronize()
    res = {k: v.cpu().numpy() for k, v in o.bufs.items()}
    res.update({k: v.cpu().numpy() for k, v in own.items()})
    return res


@functools.lru_cache(maxsize=None)
def launch(name, n):
    """The qs_avoid_score launches of one configuration and the twin's qs_track_score and
    qs_score_agents launches, everything on the host."""
    cfg = CONFIGS[name]
    n = steps_of(cfg, n)
    sw, twin = prepared(cfg, n, seed=SEEDS.get(name, DEFAULT_SEED))
    assert 1 <= n <= sw.score_depth() <= 32
    acts = make_actions(sw, n, C)
    track = make_spec(sw)
    avoid, off = make_avoid(sw), make_avoid(sw, off=True)
    before = fingerprint(sw)
    with_track = run(sw, n, acts, track, avoid)
    again = run(sw, n, acts, track, avoid)
    no_track = run(sw, n, acts, None, avoid)
    all_off = run(sw, n, acts, track, off)
    after = fingerprint(sw)
    want_track = run(twin, n, acts, track)
    want_plain = run(twin, n, acts)
    ref, base = (t.cpu().numpy() for t in track[1])
    close(sw, twin)
    rows, radius = numbers_for(cfg)
    return dict(n=n, with_track=with_track, again=again, no_track=no_track, all_off=all_off, want_track=want_track,
                want_plain=want_plain, track=dict(ref=ref, base=base, q=Q, r=R, terminal=TERMINAL), rows=rows,
                radius=radius, before=before, after=after)


def ends(r):
    """Some (c, e) ends inside the horizon and some does not."""
    fd = r["with_track"]["first_done"]
    assert (fd < r["n"]).any() and (fd == r["n"]).any()


def reference(r, g, track):
    return avoid_reference(g["obs"], g["terminal_obs"], g["terminated"], g["truncated"], g["actions_out"], track=track,
                           obstacles=r["rows"], sep_radius=r["radius"], sep_weight=SEP_WEIGHT, sep_z_scale=SEP_Z_SCALE)


def both_branches(stats):
    """Both branches of the pair hinge are taken in at least a tenth of the ordered pair-steps each;
    one obstacle row adds a term in at least a tenth of the drone-steps and one in none."""
    pairs = stats["inside"] + stats["outside"]
    assert pairs > 0 and stats["inside"] >= 0.1 * pairs and stats["outside"] >= 0.1 * pairs, stats
    assert stats["row_hits"].max() >= 0.1 * stats["drone_steps"] and stats["row_hits"].min() == 0, stats


# ------------------------------------------------------------------ 1. the cost
@pytest.mark.parametrize("n", STEPS)
@pytest.mark.parametrize("name", list(CONFIGS))
def test_cost_with_tracking_equals_the_float64_loop_as_bytes(name, n):
    r = launch(name, n)
    ends(r)
    g = r["with_track"]
    want, stats = reference(r, g, r["track"])
    print(name, r["n"], stats)
    both_branches(stats)
    assert want.dtype == np.float64 and want.shape == g["cost_agent"].shape and np.isfinite(want).all()
    assert raw(want) == raw(g["cost_agent"])
    assert raw(g["cost_agent"]) != raw(r["want_track"]["cost_agent"])   # the terms are there


@pytest.mark.parametrize("n", STEPS)
@pytest.mark.parametrize("name", list(CONFIGS))
def test_cost_without_tracking_equals_the_float64_loop_as_bytes(name, n):
    r = launch(name, n)
    g = r["no_track"]
    want, stats = reference(r, g, None)
    both_branches(stats)
    assert np.isfinite(want).all() and (want > 0).any()
    assert raw(want) == raw(g["cost_agent"])


@pytest.mark.parametrize("n", STEPS)
@pytest.mark.parametrize("name", list(CONFIGS))
def test_all_off_spec_gives_the_tracking_cost_as_bytes(name, n):
    r = launch(name, n)
    g, t = r["all_off"], r["track"]
    assert raw(g["cost_agent"]) == raw(r["want_track"]["cost_agent"])
    # and the restatement with every switch off is the tracking tests' loop
    mine, _ = avoid_reference(g["obs"], g["terminal_obs"], g["terminated"], g["truncated"], g["actions_out"], track=t)
    theirs = cost_reference(g["obs"], g["terminal_obs"], g["terminated"], g["truncated"], g["actions_out"], t["ref"],
                            t["base"], Q, R, TERMINAL)
    assert raw(mine) == raw(theirs) == raw(g["cost_agent"])


# ------------------------------------------------------------------ 2. everything else
@pytest.mark.parametrize("n", STEPS)
@pytest.mark.parametrize("name", list(CONFIGS))
def test_other_outputs_are_the_twins_and_the_swarm_is_unchanged(name, n):
    r = launch(name, n)
    ends(r)
    for k in OTHERS:
        for got, want in (("with_track", "want_track"), ("all_off", "want_track"), ("no_track", "want_plain")):
            assert r[got][k].shape == r[want][k].shape and raw(r[got][k]) == raw(r[want][k]), (k, got)
    for k in r["with_track"]:
        assert raw(r["with_track"][k]) == raw(r["again"][k]), k
    assert r["before"] == r["after"]


# ------------------------------------------------------------------ 4. table sizes and switches
@pytest.mark.parametrize("name", ["mh_d8_onedpid_f32", "mh_d3_vel_pyb", "mh_d8_onedpid_f64"])
def test_sixteen_rows_no_rows_and_each_switch_alone(name):
    cfg, n = CONFIGS[name], 5
    sw, = prepared(cfg, n, twins=0)
    acts = make_actions(sw, n, C)
    track = make_spec(sw)
    rows, radius = numbers_for(cfg)
    kw = dict(sep_weight=SEP_WEIGHT, sep_z_scale=SEP_Z_SCALE)
    cases = dict(sixteen=(many_rows(rows, 16), radius), none=((), radius), obstacles_only=(rows, 0.0),
                 one_row=(rows[2:3], radius))
    tr = dict(ref=track[1][0].cpu().numpy(), base=track[1][1].cpu().numpy(), q=Q, r=R, terminal=TERMINAL)
    for what, (tab, rad) in cases.items():
        assert len(tab) == dict(sixteen=16, none=0, obstacles_only=4, one_row=1)[what]
        g = run(sw, n, acts, track, make_avoid(sw, rows=tab, sep_radius=rad))
        want, stats = avoid_reference(g["obs"], g["terminal_obs"], g["terminated"], g["truncated"], g["actions_out"],
                                      track=tr, obstacles=tab, sep_radius=rad, **kw)
        assert raw(want) == raw(g["cost_agent"]), what
        if what == "sixteen":   # the rows past the fourth are read too
            assert stats["row_hits"][14] > 0, stats   # (row 15 is a copy of the one that weighs nothing)
    # a weight of zero switches the separation term off like a radius of zero
    g = run(sw, n, acts, None, make_avoid(sw, rows=(), sep_weight=0.0))
    assert raw(g["cost_agent"]) == raw(np.zeros(g["cost_agent"].shape, np.float64))   # +0.0, every one
    close(sw)


# ------------------------------------------------------------------ 5. refusals
def test_refusals_name_the_entry_point_and_write_nothing():
    cfg = CONFIGS["mh_d3_vel_pyb"]
    n = 5
    sw, = prepared(cfg, n, twins=0)
    lib, E, D = sw.lib, sw.num_envs, sw.num_drones
    acts = make_actions(sw, n, C)
    before = fingerprint(sw)
    track, track_keep = make_spec(sw)
    good, keep = make_avoid(sw)
    cost = torch.full((C, E, D), -7.0, dtype=torch.float64, device=sw.device)
    ret_agent = torch.full((C, E, D), -7.0, dtype=torch.float64, device=sw.device)
    ret = torch.full((C, E), -7.0, dtype=torch.float64, device=sw.device)
    ptrs = (ctypes.c_void_p * n)(*[acts[j].data_ptr() for j in range(n)])
    so = L.QsScoreOut(L.ptr(ret), None)
    untouched = [raw(t) for t in (cost, ret_agent, ret, acts)]

    def call(spec, tspec=None, handle=None, cost_ptr=cost.data_ptr()):
        return lib.qs_avoid_score(sw._h if handle is None else handle, n, C, ptrs, None, ctypes.byref(so),
                                  ret_agent.data_ptr(), ctypes.byref(tspec) if tspec is not None else None,
                                  ctypes.byref(spec) if spec is not None else None, cost_ptr, sw._stream())

    def variant(**kw):
        s = L.QsAvoidSpec.from_buffer_copy(good)
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    def refused(rc, code=QS_E_INVALID):
        assert rc == code, (rc, lib.qs_last_error())
        assert b"qs_avoid_score" in lib.qs_last_error()
        torch.cuda.synchronize()
        assert [raw(t) for t in (cost, ret_agent, ret, acts)] == untouched

    for tspec in (None, track):   # the specs themselves are fine
        assert call(good, tspec) == 0, lib.qs_last_error()
    assert call(variant(M=0, obstacles=None)) == 0 and call(variant(M=0, obstacles=good.obstacles + 4)) == 0
    assert call(variant(sep_radius=-0.0, sep_weight=-0.0, sep_z_scale=-0.0)) == 0, lib.qs_last_error()
    torch.cuda.synchronize()
    assert not (cost == -7.0).any()
    cost.fill_(-7.0); ret_agent.fill_(-7.0); ret.fill_(-7.0)
    torch.cuda.synchronize()
    nan, inf = float("nan"), float("inf")
    bad = [variant(M=-1), variant(M=17), variant(obstacles=None), variant(obstacles=good.obstacles + 4),
           variant(obstacles=good.obstacles + 8), variant(sep_radius=-1e-30), variant(sep_radius=nan),
           variant(sep_radius=inf), variant(sep_weight=-0.5), variant(sep_weight=nan), variant(sep_weight=inf),
           variant(sep_z_scale=-1.0), variant(sep_z_scale=nan), variant(sep_z_scale=inf)]
    for s in bad:
        refused(call(s))
        refused(call(s, track))
    bad_track = L.QsTrackSpec.from_buffer_copy(track)
    bad_track.L = 0
    refused(call(good, bad_track))                        # what qs_track_score refuses
    bad_track = L.QsTrackSpec.from_buffer_copy(track)
    bad_track.ref = None
    refused(call(good, bad_track))
    refused(call(None))                                   # no spec
    refused(call(good, cost_ptr=None))                    # no cost_agent
    refused(call(good, cost_ptr=ret_agent.data_ptr()))    # cost_agent on an output
    refused(call(good, cost_ptr=ret.data_ptr()))          # ... on another, partly
    refused(call(good, cost_ptr=acts[n - 1].data_ptr()))  # ... on an action buffer
    refused(lib.qs_avoid_score(None, n, C, ptrs, None, ctypes.byref(so), None, None, ctypes.byref(good), cost.data_ptr(),
                               None))
    assert fingerprint(sw) == before

    flock = QuadSwarm(task="flock", num_envs=E, num_drones=D, act="rpm")
    flock.reset(1)
    refused(call(good, handle=flock._h))
    fresh = QuadSwarm(**cfg)
    refused(call(good, handle=fresh._h), QS_E_STATE)
    close(sw, flock, fresh)
    del keep, track_keep


def test_python_arguments_and_vec_env_score_t():
    from gym_pybullet_drones_amd.vec_env.vec_env import SwarmVecEnv
    n = 5
    v = SwarmVecEnv(seed=3, **CONFIGS["mh_d2_onedpid"])
    v.reset_t()
    set_clocks(v.swarm, clocks_for(n))
    ground(v.swarm)
    acts = make_actions(v.swarm, n, C)
    track, avoid = make_spec(v.swarm), make_avoid(v.swarm)
    before = fingerprint(v.swarm)
    ret, fd, ret_agent, cost = (t.clone() for t in v.score_t(acts, per_drone=True, track=track, avoid=avoid))
    alone = v.score_t(acts, avoid=avoid)
    assert len(alone) == 3
    cost_alone = alone[2].clone()
    tracked = [t.clone() for t in v.score_t(acts, per_drone=True, track=track)]
    plain = v.score_t(acts, per_drone=True)
    torch.cuda.synchronize()
    assert len(plain) == 3 and cost.shape == ret_agent.shape and cost.dtype == torch.float64
    for got, want, k in zip((ret, fd, ret_agent), plain, ("ret", "first_done", "ret_agent")):
        assert raw(got) == raw(want), k
    assert (cost > tracked[3]).any() and not (cost < tracked[3]).any() and (cost_alone > 0).any()
    own = torch.zeros_like(cost)
    v.swarm.score(acts, track=track, avoid=avoid, cost_agent=own)
    torch.cuda.synchronize()
    assert raw(own) == raw(cost)
    assert fingerprint(v.swarm) == before
    with pytest.raises(ValueError):
        v.swarm.score(acts, avoid=avoid)   # avoid without cost_agent
    with pytest.raises(ValueError):
        avoid_spec(torch.zeros((2, 7), device=v.swarm.device))
    with pytest.raises(ValueError):
        avoid_spec(torch.zeros((2, 8)))    # not on the GPU
    spec, keep = avoid_spec()
    assert spec.M == 0 and not spec.obstacles and spec.sep_z_scale == 1.0 and keep == []
    v.close()
