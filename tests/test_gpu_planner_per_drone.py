"""The per-drone (factored) planner ticks: `QuadSwarm.mppi(..., per_drone=True)` and
`.cem(..., per_drone=True)` (qs_pd_mppi_create, qs_pd_cem_create).  Every drone weighs or
ranks the same C candidates by its own return `ret_agent` less the penalty of its env's
`first_done`; the semantics are the env-level ones with agent (e, d) in the place of env e.

 1. MPPI update against the float64 restatement of tests/test_gpu_mppi.py per (e, d), at
    that file's tolerances: both variants, A = 4, lambda > 0 and lambda = 0, a done penalty.
 2. Greedy choice per drone with hand-filled returns: different drones of an env copy
    different candidates bit for bit, ties go to the lower c, the penalty is the env's.
 3. CEM select + refit against the float64 restatement of tests/test_gpu_cem.py per (e, d),
    at that file's tolerances: both variants, the workgroup select, alpha, a zero sigma
    component, K = 1 and K = C, and NaN / infinite scores put in by hand.
 4. Sampling is the env-level planner's, byte for byte.
 5. plan(): no mutation, determinism, graph capture, `SwarmVecEnv`.
 6. Refusals.
"""
import ctypes

import numpy as np
import pytest
import torch

from gym_pybullet_drones_amd import _lib as L
from gym_pybullet_drones_amd.envs.swarm import QuadSwarm
from gym_pybullet_drones_amd.vec_env.vec_env import SwarmVecEnv
from planner_case import A4, F64, c3, fingerprint, planner_bytes, prepared, same_bytes
from planner_case import random_sequence

pytestmark = pytest.mark.gpu

MPPI_BUFS = ("nominal", "candidates", "ret", "first_done", "ret_agent", "weights", "best", "action", "tick")
CEM_BUFS = ("mean", "std", "candidates", "ret", "first_done", "ret_agent", "elites", "iter_best", "action", "tick")


def ids(v):
    return None if isinstance(v, dict) else str(v)


# ------------------------------------------------------------------- the restatements
def restate_mppi(pl, lam, penalty):
    """`restate` of tests/test_gpu_mppi.py with ret_agent: the update per (e, d) in float64 numpy."""
    torch.cuda.synchronize()
    cand = pl.candidates.cpu().numpy().astype(np.float64)      # (n, C, E, D, A)
    ra, fd = pl.ret_agent.cpu().numpy(), pl.first_done.cpu().numpy()
    n, C = cand.shape[0], cand.shape[1]
    with np.errstate(invalid="ignore"):
        s = ra - np.where(fd < n, np.float64(penalty), 0.0)[..., None]      # (C, E, D): the env's first_done
    best = np.argmax(s, axis=0)                                   # the first, i.e. lowest, c of the maximum
    if lam > 0:
        x = np.exp((s - s.max(axis=0)) / lam)
        w = x / x.sum(axis=0)
    else:
        w = (np.arange(C)[:, None, None] == best[None]).astype(np.float64)
    new = np.einsum("ced,jceda->jeda", w, cand)
    return dict(best=best.astype(np.int32), weights=w, new=new, action=new[0],
                nominal=np.concatenate([new[1:], new[-1:]], axis=0))


def check_update(pl, lam, penalty, bound, tick):
    want = restate_mppi(pl, lam, penalty)
    best, w = pl.best.cpu().numpy(), pl.weights.cpu().numpy()
    nominal, action = pl.nominal.cpu().numpy().astype(np.float64), pl.action.cpu().numpy().astype(np.float64)
    assert best.shape == want["best"].shape and w.shape == want["weights"].shape
    assert np.array_equal(best, want["best"])
    rel = np.abs(w - want["weights"]) / np.maximum(want["weights"], np.finfo(np.float64).tiny)
    print("weights: max relative difference", rel.max(), "sum - 1", np.abs(w.sum(axis=0) - 1).max())
    assert rel.max() <= 1e-12
    tol = 2.0 ** -23 * bound
    print("nominal: max abs difference", np.abs(nominal - want["nominal"]).max(), "allowed", tol)
    assert np.abs(nominal - want["nominal"]).max() <= tol and np.abs(action - want["action"]).max() <= tol
    n = nominal.shape[0]
    assert np.array_equal(nominal[-1], nominal[-2] if n > 1 else nominal[0])
    assert int(pl.tick.item()) == tick
    return want


def restate_cem(pl, mean0, std0):
    """`restate` of tests/test_gpu_cem.py with ret_agent: select + refit per (e, d) in float64 numpy."""
    torch.cuda.synchronize()
    cand = pl.candidates.cpu().numpy().astype(np.float64)      # (n, C, E, D, A)
    ra, fd = pl.ret_agent.cpu().numpy(), pl.first_done.cpu().numpy()
    n, C, E, D, A = cand.shape
    K, alpha = pl.num_elites, float(pl.spec.alpha)
    sigma = np.array(list(pl.spec.sigma)[:A], np.float32)
    smin = np.array(list(pl.spec.sigma_min)[:A], np.float32)
    with np.errstate(invalid="ignore"):
        s = ra - np.where(fd < n, np.float64(pl.spec.done_penalty), 0.0)[..., None]
    nan = np.isnan(s)
    neg = np.where(nan, 0.0, -s)
    elites = np.empty((K, E, D), np.int32)
    best = np.empty((E, D), np.float64)
    mean, std = np.empty((n, E, D, A)), np.empty((n, E, D, A))
    for e in range(E):
        for d in range(D):
            order = np.lexsort((np.arange(C), neg[:, e, d], nan[:, e, d]))   # numbers first, larger s first, lower c on ties
            elites[:, e, d] = order[:K]
            best[e, d] = s[order[0], e, d]
            x = cand[:, order[:K], e, d]                                          # (n, K, A)
            m = x.sum(axis=1) / K
            v = ((x - m[:, None]) ** 2).sum(axis=1) / K
            mean[:, e, d], std[:, e, d] = m, np.sqrt(v)
    if alpha != 0.0:
        mean = (1 - alpha) * mean + alpha * mean0.astype(np.float64)
        std = (1 - alpha) * std + alpha * std0.astype(np.float64)
    std = np.where(sigma == 0, std0.astype(np.float64), np.maximum(std, smin.astype(np.float64)))
    return dict(elites=elites, best=best, mean=mean, std=std)


def refit_and_check(pl, iteration=0):
    torch.cuda.synchronize()
    mean0, std0 = pl.mean.cpu().numpy().copy(), pl.std.cpu().numpy().copy()
    pl.refit(iteration)
    want = restate_cem(pl, mean0, std0)
    elites, best = pl.elites.cpu().numpy(), pl.iter_best.cpu().numpy()[iteration]
    mean, std = pl.mean.cpu().numpy().astype(np.float64), pl.std.cpu().numpy().astype(np.float64)
    assert elites.shape == want["elites"].shape and best.shape == want["best"].shape
    assert np.array_equal(elites, want["elites"])
    assert np.array_equal(best, want["best"], equal_nan=True)
    lo, hi = float(pl.spec.lo), float(pl.spec.hi)
    tol_m, tol_s = 2.0 ** -23 * max(abs(lo), abs(hi)), 2.0 ** -23 * (hi - lo)
    dm, ds = np.abs(mean - want["mean"]).max(), np.abs(std - want["std"]).max()
    print(f"mean: max abs difference {dm} (allowed {tol_m}); std: {ds} (allowed {tol_s})")
    assert dm <= tol_m and ds <= tol_s
    return want


def score(sw, pl):
    sw.score(pl.candidates, ret=pl.ret, first_done=pl.first_done, ret_agent=pl.ret_agent)


# ------------------------------------------------------------------- 1. MPPI update
@pytest.mark.parametrize("cfg,n,C,lam", [
    (c3(21), 7, 3, 1.0),          # one thread per agent / per (step, env, drone, component)
    (c3(21), 7, 3, 0.0),
    (c3(1), 7, 300, 1.0),         # a workgroup per agent / per (agent, step); C is no multiple of 64
    (c3(1), 7, 300, 0.0),
    (A4, 5, 130, 0.5),            # A = 4: a drone's row of 4, 15 agents
    (A4, 5, 130, 0.0),
    (F64, 7, 3, 0.5),             # ret_agent from double terms
], ids=ids)
def test_update_matches_the_float64_restatement_per_drone(cfg, n, C, lam):
    (sw,) = prepared(cfg, grounded=cfg["num_envs"] > 4)
    pen = 2.5 if cfg["num_envs"] > 4 else 0.0
    pl = sw.mppi(n, C, 0.3, lo=-1.0, hi=1.0, lam=lam, done_penalty=pen, seed=4, per_drone=True)
    E, D = sw.num_envs, sw.num_drones
    assert pl.per_drone and tuple(pl.ret_agent.shape) == (C, E, D) and pl.ret_agent.dtype == torch.float64
    assert tuple(pl.weights.shape) == (C, E, D) and tuple(pl.best.shape) == (E, D) and tuple(pl.ret.shape) == (C, E)
    pl.reset(random_sequence(pl, scale=0.9))
    pl.plan()
    want = check_update(pl, lam, pen, 1.0, tick=1)
    assert lam == 0 or (want["weights"] > 0).all()
    ra, ret = pl.ret_agent.cpu().numpy(), pl.ret.cpu().numpy()
    assert np.abs(ra.sum(axis=-1) / D - ret).max() < 1e-4 * max(1.0, np.abs(ret).max())      # ret is still filled
    if cfg["num_envs"] > 4:
        assert (pl.first_done.cpu().numpy()[:, 4] == 0).all()
    if C <= 3:
        assert (want["best"].max(axis=1) != want["best"].min(axis=1)).any()      # drones of one env disagree
    pl.plan()                                                   # a second tick, from the shifted nominal
    check_update(pl, lam, pen, 1.0, tick=2)
    # some candidates of an env done and others not (by hand: update reads the buffers as they are)
    pl.first_done[0::2, 0] = 3
    pl.update()
    check_update(pl, lam, pen, 1.0, tick=3)
    sw.close()


# ------------------------------------------------------- 2. per-drone greedy choice
@pytest.mark.parametrize("cfg,n,C", [(c3(5), 4, 9), (c3(1), 4, 70), (A4, 3, 130)], ids=ids)
def test_each_drone_copies_its_own_best_candidate(cfg, n, C):
    sw = QuadSwarm(**cfg)
    pen = 1.5
    pl = sw.mppi(n, C, 0.3, lam=0.0, done_penalty=pen, seed=4, per_drone=True)
    E, D = sw.num_envs, sw.num_drones
    pl.reset(random_sequence(pl, scale=0.9))
    pl.sample()
    c = torch.arange(C, dtype=torch.float64, device=sw.device)[:, None, None]
    tgt = (torch.arange(D, device=sw.device)[None, :] * 2 + torch.arange(E, device=sw.device)[:, None] + 1) % C   # (E, D)
    assert all(len(set(row.tolist())) == D for row in tgt)            # every drone of an env: another arg max
    pl.ret_agent.copy_(-(c - tgt[None].double()).abs())               # 0 at the target, -1 at both neighbours: a tie
    pl.first_done.fill_(n)
    pl.update()
    torch.cuda.synchronize()
    assert torch.equal(pl.best.long(), tgt)
    cand = pl.candidates.cpu().numpy()

    def check_slices(best):
        pick = np.stack([np.stack([cand[:, best[e, d], e, d] for d in range(D)], axis=1) for e in range(E)], axis=1)
        same_bytes(pl.action, pick[0], "action[e][d] = candidates[0][best[e][d]][e][d]")
        same_bytes(pl.nominal[-1], pick[-1], "held last step")
        same_bytes(pl.nominal[:-1], pick[1:], "nominal[j] = candidates[j + 1][best]")
        w = pl.weights.cpu().numpy()
        assert np.array_equal(w, (np.arange(C)[:, None, None] == best[None]).astype(np.float64))

    check_slices(tgt.cpu().numpy())
    # drone 0 of env 0 loses its best candidate to the env's penalty; its neighbours tie and the lower c wins
    t0 = int(tgt[0, 0])
    pl.first_done[t0, 0] = 1
    pl.update()
    torch.cuda.synchronize()
    want = tgt.clone()
    want[0, 0] = t0 - 1 if t0 >= 1 else t0 + 1
    assert torch.equal(pl.best.long(), want), (pl.best, want)
    assert np.array_equal(pl.best.cpu().numpy(), restate_mppi(pl, 0.0, pen)["best"])
    check_slices(want.cpu().numpy())
    assert int(pl.tick.item()) == 2
    sw.close()


# ------------------------------------------------------------------ 3. CEM refit
A4_SIGMA = (0.3, 0.2, 0.4, 0.0)      # a zero sigma component: its std stays as it is


@pytest.mark.parametrize("cfg,n,C,K,alpha", [
    (c3(21), 5, 9, 3, 0.0),            # one thread per agent
    (c3(21), 5, 9, 3, 0.5),
    (c3(2), 4, 130, 7, 0.5),           # a workgroup per agent / per (agent, step)
    (c3(1), 3, 600, 33, 0.0),          # from 512 candidates on the workgroup select runs whatever the shape
    (A4, 5, 9, 3, 0.5),                # A = 4 with a zero sigma component
    (A4, 5, 130, 7, 0.0),
    (F64, 5, 9, 3, 0.0),
    (c3(5), 4, 9, 1, 0.0), (c3(2), 4, 130, 1, 0.0),         # K = 1
    (c3(5), 4, 9, 9, 0.0), (c3(2), 4, 130, 130, 0.5),       # K = C
], ids=ids)
def test_refit_matches_the_float64_restatement_per_drone(cfg, n, C, K, alpha):
    (sw,) = prepared(cfg, grounded=cfg["num_envs"] > 4)
    sigma = A4_SIGMA if cfg is A4 else 0.3
    smin = tuple(min(0.01, s) for s in A4_SIGMA) if cfg is A4 else 0.01
    pl = sw.cem(n, C, K, sigma, iterations=2, lo=-1.0, hi=1.0, alpha=alpha, sigma_min=smin, done_penalty=0.75, seed=4,
                per_drone=True)
    E, D = sw.num_envs, sw.num_drones
    assert pl.per_drone and tuple(pl.ret_agent.shape) == (C, E, D)
    assert tuple(pl.elites.shape) == (K, E, D) and tuple(pl.iter_best.shape) == (2, E, D)
    pl.reset(random_sequence(pl, scale=0.9))
    pl.begin()
    for it in range(2):                # the second iteration samples from the refitted mean and std
        pl.sample(it)
        score(sw, pl)
        want = refit_and_check(pl, it)
        assert K == 1 or (want["std"][..., :3] > 0).all()
    el = pl.elites.cpu().numpy()
    assert K == C or (el > 0).any()
    if K < C:
        assert (el.max(axis=2) != el.min(axis=2)).any()                  # drones of one env keep different elites
    if cfg is A4:
        assert (pl.std[..., 3] == 0.0).all()
    sw.close()


@pytest.mark.parametrize("E,C,K", [(21, 9, 3), (21, 9, 9), (2, 130, 7), (2, 130, 130), (1, 600, 40)])
def test_the_total_order_per_drone(E, C, K):
    sw = QuadSwarm(**c3(E))
    D, n = 8, 4
    pl = sw.cem(n, C, K, 0.3, seed=4, done_penalty=2.5, per_drone=True)
    pl.reset(random_sequence(pl))
    pl.begin()
    pl.sample(0)
    pl.first_done.fill_(n)
    gen = torch.Generator(device="cpu").manual_seed(3)
    ra = torch.randn((C, E, D), generator=gen, dtype=torch.float64)      # another order for every drone
    ra[3, :, 0], ra[1, :, 1], ra[0, :, 2] = float("inf"), float("-inf"), float("nan")
    ra[C - 1, :, 2] = float("nan")
    ra[2, :, 3], ra[5, :, 3] = -0.0, 0.0                                  # equal: the index decides
    ra[4, :, 4] = ra[6, :, 4] = 9.0                                      # a tie at the top
    ra[:, :, 5] = float("nan")                                           # no number at all
    ra[:, :, 6] = 0.5                                                    # all equal
    pl.ret_agent.copy_(ra.to(sw.device))
    want = refit_and_check(pl)
    el, best = pl.elites.cpu().numpy(), pl.iter_best.cpu().numpy()[0]
    assert (el[0, :, 0] == 3).all() and np.isposinf(best[:, 0]).all()
    assert not (el[:, :, 1] == 1).any() or K == C
    assert (el[0, :, 4] == 4).all() and (K < 2 or (el[1, :, 4] == 6).all())
    ranks = np.arange(K, dtype=np.int32)[:, None].repeat(E, axis=1)
    assert np.array_equal(el[:, :, 5], ranks) and np.isnan(best[:, 5]).all()
    assert np.array_equal(el[:, :, 6], ranks)
    if K == C:                                                           # -inf the last of the numbers, then the NaNs by index
        assert (el[C - 1, :, 1] == 1).all()
        assert (el[C - 2, :, 2] == 0).all() and (el[C - 1, :, 2] == C - 1).all()
    # the env's penalty moves a candidate down for every drone of that env, and of no other
    pl.first_done[4, 0] = 1
    again = refit_and_check(pl)
    assert (pl.elites.cpu().numpy()[0, 0, 4] == 6) and np.array_equal(again["elites"][:, 1:], want["elites"][:, 1:])
    sw.close()


# ------------------------------------------------------------------- 4. same noise
def test_sampling_is_the_env_level_planners():
    (sw,) = prepared(c3(5))
    pd, ev = sw.mppi(6, 33, 0.4, seed=9, per_drone=True), sw.mppi(6, 33, 0.4, seed=9)
    assert ev.per_drone is False and ev.ret_agent is None and tuple(ev.weights.shape) == (33, 5)
    nom = random_sequence(pd)
    for tick in range(2):
        for p in (pd, ev):
            p.nominal.copy_(nom)
            p.sample()
        torch.cuda.synchronize()
        same_bytes(pd.candidates, ev.candidates, f"MPPI candidates, tick {tick}")
        same_bytes(pd.candidates[:, 0], nom, "candidate 0 is the nominal for every drone")
        for p in (pd, ev):
            p.update()                                                    # ret all zero: the tick moves on
    assert int(pd.tick.item()) == 2
    cd, ce = sw.cem(5, 17, 4, 0.3, iterations=3, seed=7, per_drone=True), sw.cem(5, 17, 4, 0.3, iterations=3, seed=7)
    m0 = random_sequence(cd)
    for p in (cd, ce):
        p.reset(m0)
        p.begin()
    for it in (0, 2):
        cd.sample(it)
        ce.sample(it)
        torch.cuda.synchronize()
        same_bytes(cd.candidates, ce.candidates, f"CEM candidates, iteration {it}")
    sw.close()


# ------------------------------------------------------------------------ 5. plan()
@pytest.mark.parametrize("kind,cfg,C", [("mppi", c3(21), 3), ("mppi", c3(1), 300), ("cem", c3(21), 9), ("cem", c3(1), 130)], ids=ids)
def test_plan_leaves_the_swarm_alone_and_repeats(kind, cfg, C):
    a, b = prepared(cfg, twins=1, grounded=cfg["num_envs"] > 4)

    def make(sw):
        if kind == "mppi":
            return sw.mppi(7, C, 0.3, lam=0.4, done_penalty=1.0, seed=4, per_drone=True)
        return sw.cem(7, C, 3, 0.3, iterations=2, done_penalty=1.0, seed=4, per_drone=True)

    pa, pb = make(a), make(b)
    before = fingerprint(a)
    for _ in range(2):
        pa.plan()
        pb.plan()
    assert fingerprint(a) == before
    assert int(pa.tick.item()) == 2
    bufs = MPPI_BUFS if kind == "mppi" else CEM_BUFS
    assert planner_bytes(pa, bufs) == planner_bytes(pb, bufs)             # the same inputs, the same bytes
    assert pa.ret_agent.abs().sum() > 0 and pa.action.abs().sum() > 0
    a.close()
    b.close()


@pytest.mark.parametrize("kind", ["mppi", "cem"])
def test_captured_tick_replays_what_eager_ticks_compute(kind):
    cap, eager = prepared(c3(5), twins=1)

    def make(sw):
        if kind == "mppi":
            return sw.mppi(7, 70, 0.3, lam=0.3, seed=8, per_drone=True)
        return sw.cem(7, 70, 5, 0.3, iterations=2, seed=8, per_drone=True)

    pc, pe = make(cap), make(eager)
    seq = random_sequence(pc, scale=0.9)
    pc.reset(seq)
    pe.reset(seq)
    want = []
    for _ in range(3):
        pe.plan()
        r = eager.step(pe.action)
        torch.cuda.synchronize()
        want.append((pe.action.clone(), r.obs.clone(), r.reward.clone(), pe.candidates.clone(), pe.ret_agent.clone()))
    assert not torch.equal(want[0][3][:, 1:], want[1][3][:, 1:])
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        pc.plan()
        r = cap.step(pc.action)
    for k in range(3):
        g.replay()
        torch.cuda.synchronize()
        assert int(pc.tick.item()) == k + 1
        same_bytes(pc.candidates, want[k][3], f"candidates, tick {k}")
        same_bytes(pc.ret_agent, want[k][4], f"ret_agent, tick {k}")
        same_bytes(pc.action, want[k][0], f"action, tick {k}")
        same_bytes(r.obs, want[k][1], f"obs, tick {k}")
        same_bytes(r.reward, want[k][2], f"reward, tick {k}")
    assert fingerprint(cap)[:4] == fingerprint(eager)[:4]     # (launch counts aside: a capture counts its node once)
    cap.close()
    eager.close()


def test_vec_env_per_drone():
    a, b = SwarmVecEnv(seed=3, **c3(5)), SwarmVecEnv(seed=3, **c3(5))
    pa, pb = a.mppi(6, 9, 0.3, lam=0.4, seed=2, per_drone=True), b.mppi(6, 9, 0.3, lam=0.4, seed=2, per_drone=True)
    assert pa.per_drone and tuple(pa.best.shape) == (5, 8)
    for v in (a, b):
        v.reset_t()
        v.step_t(None)
    for tick in range(2):
        ra = pa.step_t()
        rb = b.step_t(pb.plan())
        torch.cuda.synchronize()
        for k in ("obs", "reward", "terminated", "truncated"):
            same_bytes(getattr(ra, k), getattr(rb, k), f"{k}, tick {tick}")
        same_bytes(pa.action, pb.action, "action")
    pc = a.cem(6, 9, 3, 0.3, iterations=2, seed=2, per_drone=True)
    assert tuple(pc.elites.shape) == (3, 5, 8) and pc.step_t() is not None
    # score_t(per_drone=True) appends ret_agent, from cached buffers
    acts = pa.candidates.clone()
    ret, fd, ra1 = a.score_t(acts, per_drone=True)
    out = a.score_t(acts, per_step=True, per_drone=True)
    torch.cuda.synchronize()
    assert len(out) == 6 and tuple(ra1.shape) == (9, 5, 8) and ra1.dtype == torch.float64
    same_bytes(out[5], ra1, "ret_agent with and without the per-step outputs")
    assert a.score_t(acts, per_drone=True)[2].data_ptr() == ra1.data_ptr() and len(a.score_t(acts)) == 2
    ret0 = a.score_t(acts)[0]
    torch.cuda.synchronize()
    same_bytes(ret0, ret, "ret with and without ret_agent")
    a.close()
    b.close()


# --------------------------------------------------------------------- 6. refusals
def test_refusals():
    sw = QuadSwarm(**c3(21))
    sw.reset(3)
    before = fingerprint(sw)
    ev_m, ev_c = sw.mppi(4, 3, 0.3), sw.cem(4, 3, 2, 0.3)
    pd_m, pd_c = sw.mppi(4, 3, 0.3, per_drone=True), sw.cem(4, 3, 2, 0.3, per_drone=True)
    for fn, ev, pd in (("qs_pd_mppi_ret_agent", ev_m, pd_m), ("qs_pd_cem_ret_agent", ev_c, pd_c)):
        out = ctypes.c_void_p(0x55)
        assert getattr(sw.lib, fn)(ev._p, ctypes.byref(out)) == -1 and out.value == 0x55       # QS_E_INVALID
        assert fn.encode() in sw.lib.qs_last_error() and b"env-level" in sw.lib.qs_last_error()
        assert getattr(sw.lib, fn)(pd._p, ctypes.byref(out)) == 0 and out.value == pd.ret_agent.data_ptr()
    ok = dict(horizon=4, candidates=3, sigma=0.3, per_drone=True)
    for bad in (dict(horizon=0), dict(horizon=sw.score_depth() + 1), dict(candidates=1), dict(lam=-1.0),
                dict(candidates=(1 << 27) + 1),
                dict(candidates=1 << 21)):                   # C * E * D = 2^21 * 168 >= 2^28: ret_agent past the 32-bit offsets
        with pytest.raises(L.QuadSwarmError, match="rc=-1.*qs_pd_mppi_create"):
            sw.mppi(**{**ok, **bad})
    for bad in (dict(elites=0), dict(elites=4), dict(iterations=17), dict(alpha=1.0), dict(candidates=1 << 21, elites=2)):
        with pytest.raises(L.QuadSwarmError, match="rc=-1.*qs_pd_cem_create"):
            sw.cem(**{**ok, "elites": 2, **bad})
    assert fingerprint(sw) == before
    sw.close()
    for cfg in (dict(task="multihover", num_drones=4, num_envs=16, act="rpm"), dict(task="flock", num_drones=4, num_envs=16, act="rpm")):
        no = QuadSwarm(**cfg)
        no.reset(3)
        before = fingerprint(no)
        with pytest.raises(L.QuadSwarmError, match="rc=-1.*qs_pd_mppi_create.*cannot score"):
            no.mppi(4, 3, 0.3, per_drone=True)
        with pytest.raises(L.QuadSwarmError, match="rc=-1.*qs_pd_cem_create.*cannot score"):
            no.cem(4, 3, 2, 0.3, per_drone=True)
        assert fingerprint(no) == before
        no.close()
