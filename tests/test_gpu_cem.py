"""The native CEM planner tick (qs_cem_*, `QuadSwarm.cem`, `SwarmVecEnv.cem`).

 1. Sample: candidate 0 is the mean, every candidate is clipped, a zero spread copies its
    component, the noise over a hand-set std is N(0, 1) (one-sample KS at the 0.001 level,
    mean and variance within 4 standard errors), iterations and ticks draw new noise, a
    reset repeats the first draw, and the draw is not the MPPI planner's.
 2. Sharding: the noise is keyed on the global env id.
 3. Select + refit against a float64 numpy restatement that reads the planner's own
    candidates, ret and first_done: both variants, every thread striding, C past the LDS
    stage, A = 4, a row wider than a wave, fp64 rewards, K = 1 and K = C.  elites and
    iter_best must be equal; mean within 2^-23 max(|lo|, |hi|) and std within 2^-23 (hi - lo):
    with K <= 1 024 the double sums carry a relative error below 2^-33 and the two-pass
    variance is second-order in the mean's error, so what remains is one float32 rounding.
 4. The order's edges with hand-filled scores: ties, signed zeros, infinities, NaNs, the
    done penalty, identical elites.
 5. Smoothing (alpha > 0 reads the old values, alpha = 0 does not).
 6. Finish: the action, the shift at n = 1 and n = score_depth(), the tick.
 7. plan() equals its phases, byte for byte.
 8. plan() leaves the swarm as it was.
 9. plan() + step() captured into one graph replays what eager ticks compute.
10. Refusals leave the swarm and the planner as they were.
11. `SwarmVecEnv.cem(...).step_t()`.
"""
import numpy as np
import pytest
import torch

from gym_pybullet_drones_amd import _lib as L
from gym_pybullet_drones_amd.envs.swarm import CEMPlanner, QuadSwarm, grid_layout
from gym_pybullet_drones_amd.vec_env.vec_env import SwarmVecEnv
from planner_case import A4, F64, c3, fingerprint, ks_normal, planner_bytes, prepared, same_bytes
from planner_case import random_sequence as random_mean

pytestmark = pytest.mark.gpu

BUFS = ("mean", "std", "candidates", "ret", "first_done", "elites", "iter_best", "action", "tick")
STAGE = 4096   # cem_sizes.h kCemStage: the keys the per-workgroup select keeps in LDS
# (E, C, K) of the two variants (cem_variant: a workgroup per env from C = 64 on while E * D * A < 16 384)
THREAD, BLOCK = (21, 9, 3), (2, 130, 7)


def score(sw, pl):
    sw.score(pl.candidates, ret=pl.ret, first_done=pl.first_done)


def restate(pl, mean0, std0):
    """Select + refit in float64 numpy, from the planner's own candidates, ret and first_done
    and the mean / std from before the refit."""
    torch.cuda.synchronize()
    cand = pl.candidates.cpu().numpy().astype(np.float64)      # (n, C, E, D, A)
    ret, fd = pl.ret.cpu().numpy(), pl.first_done.cpu().numpy()
    n, C, E, _, A = cand.shape
    K, alpha = pl.num_elites, float(pl.spec.alpha)
    sigma = np.array(list(pl.spec.sigma)[:A], np.float32)
    smin = np.array(list(pl.spec.sigma_min)[:A], np.float32)
    with np.errstate(invalid="ignore"):
        s = ret - np.where(fd < n, np.float64(pl.spec.done_penalty), 0.0)
    nan = np.isnan(s)
    neg = np.where(nan, 0.0, -s)
    elites = np.empty((K, E), np.int32)
    best = np.empty(E, np.float64)
    mean, std = np.empty(cand.shape[:1] + cand.shape[2:]), np.empty(cand.shape[:1] + cand.shape[2:])
    for e in range(E):
        order = np.lexsort((np.arange(C), neg[:, e], nan[:, e]))   # numbers first, larger s first, lower c on ties
        elites[:, e] = order[:K]
        best[e] = s[order[0], e]
        x = cand[:, order[:K], e]                                     # (n, K, D, A)
        m = x.sum(axis=1) / K
        v = ((x - m[:, None]) ** 2).sum(axis=1) / K
        mean[:, e], std[:, e] = m, np.sqrt(v)
    if alpha != 0.0:
        mean = (1 - alpha) * mean + alpha * mean0.astype(np.float64)
        std = (1 - alpha) * std + alpha * std0.astype(np.float64)
    std = np.where(sigma == 0, std0.astype(np.float64), np.maximum(std, smin.astype(np.float64)))
    return dict(elites=elites, best=best, mean=mean, std=std)


def refit_and_check(pl, iteration=0):
    """refit(iteration) against the restatement made from the buffers as they are now."""
    torch.cuda.synchronize()
    mean0, std0 = pl.mean.cpu().numpy().copy(), pl.std.cpu().numpy().copy()
    pl.refit(iteration)
    want = restate(pl, mean0, std0)
    elites, best = pl.elites.cpu().numpy(), pl.iter_best.cpu().numpy()[iteration]
    mean, std = pl.mean.cpu().numpy().astype(np.float64), pl.std.cpu().numpy().astype(np.float64)
    assert np.array_equal(elites, want["elites"])
    assert np.array_equal(best, want["best"], equal_nan=True)
    lo, hi = float(pl.spec.lo), float(pl.spec.hi)
    tol_m, tol_s = 2.0 ** -23 * max(abs(lo), abs(hi)), 2.0 ** -23 * (hi - lo)
    dm, ds = np.abs(mean - want["mean"]).max(), np.abs(std - want["std"]).max()
    print(f"mean: max abs difference {dm} (allowed {tol_m}); std: {ds} (allowed {tol_s})")
    assert dm <= tol_m and ds <= tol_s
    return want


# ------------------------------------------------------------------------ 1. sample
def test_sample_copies_the_mean_clips_and_draws_anew():
    (sw,) = prepared(c3(5))
    pl = sw.cem(7, 33, 4, 0.8, iterations=3, lo=-1.0, hi=1.0, seed=5)
    assert isinstance(pl, CEMPlanner)
    m0 = random_mean(pl)
    pl.reset(m0)
    pl.begin()
    pl.sample(0)
    torch.cuda.synchronize()
    same_bytes(pl.mean, m0, "reset copies the mean")
    assert torch.equal(pl.std, torch.full_like(pl.std, 0.8))
    same_bytes(pl.candidates[:, 0], m0, "candidate 0")
    first = pl.candidates.clone()
    c = first.cpu().numpy()
    assert c.min() >= -1.0 and c.max() <= 1.0 and (c == 1.0).any() and (c == -1.0).any()
    assert not np.array_equal(c[:, 1], c[:, 2]) and not np.array_equal(c[:, 1, 0], c[:, 1, 1])
    assert int(pl.tick.item()) == 0          # sampling alone does not tick
    pl.sample(1)                             # another iteration of the same tick
    torch.cuda.synchronize()
    same_bytes(pl.candidates[:, 0], m0, "candidate 0, iteration 1")
    assert (first[:, 1:] != pl.candidates[:, 1:]).float().mean() > 0.9
    pl.finish()                              # tick 0 -> 1 (and the mean shifts: put it back)
    pl.mean.copy_(m0)
    pl.sample(0)
    torch.cuda.synchronize()
    assert int(pl.tick.item()) == 1
    assert (first[:, 1:] != pl.candidates[:, 1:]).float().mean() > 0.9
    pl.reset(m0)
    pl.begin()
    pl.sample(0)
    torch.cuda.synchronize()
    assert int(pl.tick.item()) == 0
    same_bytes(pl.candidates, first, "after reset the first sample repeats")
    pm = sw.mppi(7, 33, 0.8, lo=-1.0, hi=1.0, seed=5)     # the same seed, tick, envs, steps: domain tag 3, not 4
    pm.reset(m0)
    pm.sample()
    torch.cuda.synchronize()
    same_bytes(pm.candidates[:, 0], first[:, 0], "both copy the mean")
    assert (first[:, 1:] != pm.candidates[:, 1:]).float().mean() > 0.9
    sw.close()


def test_a_zero_spread_copies_its_component():
    sw = QuadSwarm(**A4)
    pl = sw.cem(6, 40, 5, (0.5, 1.0, 2.0, 0.0), lo=-100.0, hi=100.0, seed=2)
    m0 = random_mean(pl)
    pl.reset(m0)
    pl.begin()
    pl.sample(0)
    torch.cuda.synchronize()
    assert torch.equal(pl.candidates[..., 3], m0[:, None, ..., 3].expand(-1, 40, -1, -1))
    for a in range(3):
        assert not torch.equal(pl.candidates[:, 1, ..., a], m0[..., a])
    pl.std[..., 1] = 0.0                       # by hand: the sample reads the std, not sigma
    pl.sample(0)
    torch.cuda.synchronize()
    assert torch.equal(pl.candidates[..., 1], m0[:, None, ..., 1].expand(-1, 40, -1, -1))
    assert not torch.equal(pl.candidates[:, 1, ..., 0], m0[..., 0])
    sw.close()


def test_noise_over_a_hand_set_std_is_standard_normal():
    sw = QuadSwarm(**c3(4))
    pl = sw.cem(8, 257, 8, 0.5, iterations=2, lo=-1e6, hi=1e6, seed=1)
    m0 = random_mean(pl, scale=3.0)
    pl.reset(m0)
    pl.begin()
    gen = torch.Generator(device="cpu").manual_seed(5)
    std = (0.1 + 1.9 * torch.rand(tuple(pl.std.shape), generator=gen)).to(pl.std.device)
    pl.std.copy_(std)
    pl.sample(1)
    torch.cuda.synchronize()
    c = pl.candidates[:, 1:].cpu().numpy().astype(np.float64)        # 8 * 256 * 4 * 8 = 2^16 draws
    z = (c - m0.cpu().numpy().astype(np.float64)[:, None]) / std.cpu().numpy().astype(np.float64)[:, None]
    ks_normal(z)
    sw.close()


# ---------------------------------------------------------------------- 2. sharding
def test_noise_is_keyed_on_the_global_env():
    whole, lo_half, hi_half = QuadSwarm(**c3(6)), QuadSwarm(**c3(3, env_offset=0)), QuadSwarm(**c3(3, env_offset=3))
    pw, pa, pb = (sw.cem(5, 9, 3, 0.3, iterations=3, seed=7) for sw in (whole, lo_half, hi_half))
    m0 = random_mean(pw)
    pw.reset(m0)
    pa.reset(m0[:, 0:3].contiguous())
    pb.reset(m0[:, 3:6].contiguous())
    for p in (pw, pa, pb):
        p.begin()
    for it in (0, 2):
        for p in (pw, pa, pb):
            p.sample(it)
        torch.cuda.synchronize()
        same_bytes(pw.candidates[:, :, 0:3], pa.candidates, f"global envs 0 .. 2, iteration {it}")
        same_bytes(pw.candidates[:, :, 3:6], pb.candidates, f"global envs 3 .. 5, iteration {it}")
        assert not torch.equal(pa.candidates[:, 1:], pb.candidates[:, 1:])
    for sw in (whole, lo_half, hi_half):
        sw.close()


# ------------------------------------------------------------- 3. select + refit
W80 = dict(task="multihover", num_drones=20, num_envs=2, act="vel", physics="pyb", initial_xyzs=grid_layout(20))


@pytest.mark.parametrize("cfg,n,C,K", [
    (c3(5), 7, 130, 7),             # a workgroup per env / per (env, step); C is no multiple of 64
    (c3(2), 5, 2100, 33),           # every thread of the workgroup strides
    (c3(2), 3, STAGE + 37, 33),     # C past the keys kept in LDS
    (c3(300), 4, 9, 3),             # one thread per env: two 256-thread groups, the last one partial
    (A4, 5, 9, 3),                  # A = 4, a row of 12
    (A4, 5, 130, 7),                # ... in the workgroup variant: 12 of 16 lanes a group
    (W80, 3, 70, 5),                # a row of 80: wider than a wave
    (F64, 7, 9, 3),                 # ret from double rewards
    (c3(5), 4, 9, 1), (c3(2), 4, 130, 1),         # K = 1
    (c3(5), 4, 9, 9), (c3(2), 4, 130, 130),       # K = C
    (c3(2), 2, 1100, 1024),         # K at its bound
], ids=lambda v: None if isinstance(v, dict) else str(v))
def test_refit_matches_the_float64_restatement(cfg, n, C, K):
    (sw,) = prepared(cfg)
    assert n <= sw.score_depth()
    pl = sw.cem(n, C, K, 0.3, iterations=2, lo=-1.0, hi=1.0, sigma_min=0.01, seed=4)
    pl.reset(random_mean(pl, scale=0.9))
    pl.begin()
    for it in range(2):                # the second iteration samples from the refitted mean and std
        pl.sample(it)
        score(sw, pl)
        want = refit_and_check(pl, it)
        assert K == 1 or (want["std"] > 0).all()
    assert K == C or (pl.elites.cpu().numpy() > 0).any()
    sw.close()


# ------------------------------------------------------------------ 4. the order's edges
def edge_planner(E, C, K, **kw):
    sw = QuadSwarm(**c3(E))
    pl = sw.cem(4, C, K, 0.3, seed=4, **kw)
    pl.reset(random_mean(pl))
    pl.begin()
    pl.sample(0)
    pl.first_done.fill_(4)
    return sw, pl


def spread(C, E, device):
    """Distinct finite scores, falling with c."""
    return -1.0 - torch.arange(C, dtype=torch.float64, device=device)[:, None].expand(C, E).clone() / C


@pytest.mark.parametrize("E,C,K", [THREAD, (21, 9, 9), BLOCK, (2, 130, 130), (2, STAGE + 5, 40)])
def test_the_total_order(E, C, K):
    sw, pl = edge_planner(E, C, K)
    ranks = np.arange(K, dtype=np.int32)[:, None].repeat(E, axis=1)
    pl.ret.fill_(0.5)                                         # all equal: the index decides
    refit_and_check(pl)
    assert np.array_equal(pl.elites.cpu().numpy(), ranks)
    ret = spread(C, E, sw.device)                             # 0.0 against -0.0: equal, the index decides
    ret[2], ret[5] = -0.0, 0.0
    pl.ret.copy_(ret)
    refit_and_check(pl)
    el = pl.elites.cpu().numpy()
    assert (el[0] == 2).all() and (K < 2 or (el[1] == 5).all())
    assert np.signbit(pl.iter_best.cpu().numpy()[0]).all()   # s of rank 0 as it is: -0.0
    ret = spread(C, E, sw.device)                             # infinities are numbers
    ret[3], ret[1], ret[0] = float("inf"), float("-inf"), float("nan")
    ret[C - 1] = float("nan")
    pl.ret.copy_(ret)
    refit_and_check(pl)
    el = pl.elites.cpu().numpy()
    assert (el[0] == 3).all() and np.isposinf(pl.iter_best.cpu().numpy()[0]).all()
    if K == C:                                                # ... -inf the last of them, then the NaNs by index
        assert (el[C - 3] == 1).all() and (el[C - 2] == 0).all() and (el[C - 1] == C - 1).all()
    else:
        assert not np.isin(el, (0, 1, C - 1)).any()
    ret = torch.full((C, E), float("nan"), dtype=torch.float64, device=sw.device)
    ret[4], ret[7] = -3.0, 2.0                                # fewer numbers than K: the lowest-c NaNs fill the list
    pl.ret.copy_(ret)
    refit_and_check(pl)
    el = pl.elites.cpu().numpy()
    filled = [7, 4] + [c for c in range(C) if c not in (4, 7)]
    assert np.array_equal(el, np.array(filled[:K], np.int32)[:, None].repeat(E, axis=1))
    pl.ret.fill_(float("nan"))                                # no number at all
    refit_and_check(pl)
    assert np.array_equal(pl.elites.cpu().numpy(), ranks) and np.isnan(pl.iter_best.cpu().numpy()[0]).all()
    sw.close()


@pytest.mark.parametrize("E,C,K", [THREAD, BLOCK])
def test_done_penalty_moves_a_candidate_out(E, C, K):
    sw, pl = edge_planner(E, C, K, done_penalty=2.5)
    pl.ret.copy_(spread(C, E, sw.device))                     # candidate 0 is the best ...
    refit_and_check(pl)
    assert (pl.elites.cpu().numpy()[0] == 0).all()
    pl.first_done[0] = 1                                      # ... until it ends an episode
    pl.first_done[2, 1] = 0
    want = refit_and_check(pl)
    el = pl.elites.cpu().numpy()
    assert (el[0] == 1).all() and not (el == 0).any() and 2 in el[:, 0] and 2 not in el[:, 1]
    assert np.array_equal(want["best"], pl.ret.cpu().numpy()[1])
    sw.close()


@pytest.mark.parametrize("C,K", [(9, 3), (130, 7)])
def test_identical_elites_leave_the_floor(C, K):
    sw = QuadSwarm(**A4)
    sigma, smin = (0.5, 1.0, 2.0, 0.0), (0.125, 0.25, 0.0, 0.0)
    pl = sw.cem(4, C, K, sigma, sigma_min=smin, lo=-3.0, hi=3.0, seed=4)
    m0 = random_mean(pl)
    pl.reset(m0)
    pl.begin()
    pl.sample(0)
    row = pl.candidates[:, 5].clone()
    pl.candidates.copy_(row[:, None].expand_as(pl.candidates))
    pl.first_done.fill_(4)
    refit_and_check(pl)
    torch.cuda.synchronize()
    same_bytes(pl.mean, row, "the mean of identical rows is the row")
    for a in range(4):                                        # v is exactly 0: the floor, and 0 where sigma = 0
        assert (pl.std[..., a] == smin[a]).all()
    sw.close()


# --------------------------------------------------------------------- 5. smoothing
@pytest.mark.parametrize("E,C,K", [THREAD, BLOCK])
def test_smoothing(E, C, K):
    (sw,) = prepared(c3(E))
    pl = sw.cem(5, C, K, 0.4, iterations=2, alpha=0.25, sigma_min=0.05, seed=6)
    pl.reset(random_mean(pl, scale=0.9))
    pl.begin()
    for it in range(2):
        pl.sample(it)
        score(sw, pl)
        old = pl.mean.clone()
        want = refit_and_check(pl, it)                        # from the previous mean and std
        m = pl.mean.cpu().numpy().astype(np.float64)
        plain = (want["mean"] - 0.25 * old.cpu().numpy()) / 0.75
        assert np.abs(m - plain).max() > 1e-3                 # and the old mean does weigh in
    free = sw.cem(5, C, K, 0.4, iterations=2, alpha=0.0, seed=6)
    free.reset(random_mean(free, scale=0.9))
    free.begin()
    free.sample(0)
    score(sw, free)
    free.std.fill_(float("nan"))                              # alpha = 0 does not read the old values
    free.mean[1:] = float("nan")
    free.refit(0)
    torch.cuda.synchronize()
    assert torch.isfinite(free.std).all() and torch.isfinite(free.mean).all()
    sw.close()


# ------------------------------------------------------------------------ 6. finish
@pytest.mark.parametrize("E,C,K,n", [THREAD + (1,), THREAD + (32,), BLOCK + (1,), BLOCK + (32,), (300, 9, 3, 5)])
def test_finish_shifts_and_ticks(E, C, K, n):
    (sw,) = prepared(c3(E))
    assert n <= sw.score_depth() == 32
    pl = sw.cem(n, C, K, 0.3, iterations=3, seed=4)
    m0 = random_mean(pl)
    pl.reset(m0)
    pl.finish()
    torch.cuda.synchronize()
    same_bytes(pl.action, m0[0], "action = the old mean[0]")
    same_bytes(pl.mean[-1], m0[-1], "the last step holds")
    if n > 1:
        same_bytes(pl.mean[:-1], m0[1:], "mean[j] = mean[j + 1]")
    assert int(pl.tick.item()) == 1
    pl.plan()                                                 # three iterations, one tick
    pl.plan()
    torch.cuda.synchronize()
    assert int(pl.tick.item()) == 3
    assert np.isfinite(pl.iter_best.cpu().numpy()).all()
    sw.close()


# ---------------------------------------------------------- 7. plan() equals its phases
@pytest.mark.parametrize("E,C,K", [THREAD, BLOCK])
@pytest.mark.parametrize("I", [1, 3])
def test_plan_equals_its_phases(E, C, K, I):
    a, b = prepared(c3(E), twins=1)
    pa, pb = (sw.cem(6, C, K, 0.3, iterations=I, alpha=0.1, sigma_min=0.02, done_penalty=1.0, seed=8) for sw in (a, b))
    m0 = random_mean(pa, scale=0.9)
    pa.reset(m0)
    pb.reset(m0)
    for tick in range(2):
        act = pa.plan()
        assert act.data_ptr() == pa.action.data_ptr()
        pb.begin()
        for it in range(I):
            pb.sample(it)
            score(b, pb)
            pb.refit(it)
        pb.finish()
        for k, x, y in zip(BUFS, planner_bytes(pa, BUFS), planner_bytes(pb, BUFS)):
            assert x == y, f"{k}, tick {tick}"
    a.close()
    b.close()


# ------------------------------------------------------------------- 8. no mutation
@pytest.mark.parametrize("E,C,K", [THREAD, BLOCK])
def test_plan_leaves_the_swarm_alone(E, C, K):
    (sw,) = prepared(c3(E))
    pl = sw.cem(7, C, K, 0.3, seed=4)
    before = fingerprint(sw)
    pl.plan()
    pl.plan()
    assert fingerprint(sw) == before
    assert int(pl.tick.item()) == 2
    sw.close()


# ------------------------------------------------------- 9. determinism and capture
@pytest.mark.parametrize("E,C,K", [(5, 9, 3), BLOCK])
def test_captured_tick_replays_what_eager_ticks_compute(E, C, K):
    cap, eager = prepared(c3(E), twins=1)
    pc, pe = (sw.cem(7, C, K, 0.3, iterations=2, seed=8) for sw in (cap, eager))
    m0 = random_mean(pc, scale=0.9)
    pc.reset(m0)
    pe.reset(m0)
    want = []
    for _ in range(3):
        pe.plan()
        r = eager.step(pe.action)
        torch.cuda.synchronize()
        want.append((pe.action.clone(), r.obs.clone(), r.reward.clone(), [t.clone() for t in
                                                                          (getattr(pe, k) for k in BUFS)]))
    assert not torch.equal(want[0][3][2][:, 1:], want[1][3][2][:, 1:])      # the candidates of two ticks
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        pc.plan()
        r = cap.step(pc.action)
    for k in range(3):
        g.replay()
        torch.cuda.synchronize()
        assert int(pc.tick.item()) == k + 1
        for name, w in zip(BUFS, want[k][3]):
            same_bytes(getattr(pc, name), w, f"{name}, tick {k}")
        same_bytes(r.obs, want[k][1], f"obs, tick {k}")
        same_bytes(r.reward, want[k][2], f"reward, tick {k}")
    assert fingerprint(cap)[:4] == fingerprint(eager)[:4]     # (launch counts aside: a capture counts its node once)
    cap.close()
    eager.close()


# --------------------------------------------------------------------- 10. refusals
def test_refusals_leave_swarm_and_planner_alone():
    sw = QuadSwarm(**c3(21))
    depth = sw.score_depth()
    pl = sw.cem(depth, 9, 3, 0.3, iterations=2, seed=4)       # creating a planner needs no reset
    pl.reset(random_mean(pl))
    held = planner_bytes(pl, BUFS)
    with pytest.raises(L.QuadSwarmError, match="rc=-4.*qs_reset"):   # QS_E_STATE: plan before qs_reset
        pl.plan()
    assert planner_bytes(pl, BUFS) == held
    sw.reset(3)
    sw.step(None)
    before = fingerprint(sw)
    ok = dict(horizon=4, candidates=9, elites=3, sigma=0.3)
    inf, nan = float("inf"), float("nan")
    for bad in (dict(horizon=0), dict(horizon=depth + 1), dict(candidates=1, elites=1), dict(candidates=0, elites=1),
                dict(elites=0), dict(elites=10), dict(candidates=2000, elites=1025), dict(iterations=0),
                dict(iterations=17), dict(lo=1.0, hi=1.0), dict(lo=0.5, hi=-0.5), dict(lo=-inf), dict(hi=nan),
                dict(sigma=-0.1), dict(sigma=nan), dict(sigma=inf), dict(sigma_min=-0.1), dict(sigma_min=nan),
                dict(sigma_min=0.4), dict(alpha=-0.1), dict(alpha=1.0), dict(alpha=nan), dict(alpha=inf),
                dict(done_penalty=-0.5), dict(done_penalty=inf), dict(done_penalty=nan),
                dict(candidates=(1 << 27) + 1),                    # the counter word / 32-bit offsets
                dict(candidates=1 << 25)):                         # C * E * D = 2^25 * 168 > 2^31
        with pytest.raises(L.QuadSwarmError, match="rc=-1.*qs_cem_create"):
            sw.cem(**{**ok, **bad})
    sw.cem(4, 9, 9, 0.3, iterations=16, sigma_min=0.3, alpha=0.99).close()    # the last accepted values
    for call in (pl.sample, pl.refit):
        for it in (-1, 2, 16):
            with pytest.raises(L.QuadSwarmError, match="rc=-1.*iteration"):
                call(it)
    with pytest.raises(ValueError):
        sw.cem(4, 9, 3, (0.1, 0.2))                               # one sigma per component, A = 1
    with pytest.raises(ValueError):
        sw.cem(4, 9, 3, 0.3, sigma_min=(0.1, 0.2))
    with pytest.raises(ValueError):
        pl.reset(torch.zeros((depth, 21, 8), device=sw.device))
    assert fingerprint(sw) == before and planner_bytes(pl, BUFS) == held
    pl.plan()                                                      # and the planner still works
    torch.cuda.synchronize()
    assert int(pl.tick.item()) == 1
    sw.close()                                                     # closes its planners first
    assert not pl._p


@pytest.mark.parametrize("cfg,why", [
    (dict(task="multihover", num_drones=4, num_envs=16, act="rpm"), "cannot score"),   # the default diagonal layout
    (dict(task="flock", num_drones=4, num_envs=16, act="rpm"), "cannot score"),
])
def test_handles_that_cannot_score_cannot_plan(cfg, why):
    sw = QuadSwarm(**cfg)
    sw.reset(3)
    before = fingerprint(sw)
    with pytest.raises(L.QuadSwarmError, match="rc=-1.*" + why):
        sw.cem(4, 9, 3, 0.3)
    assert fingerprint(sw) == before
    sw.close()


# --------------------------------------------------------------------- 11. vec env
def test_vec_env_planner_step_t():
    a, b = SwarmVecEnv(seed=3, **c3(5)), SwarmVecEnv(seed=3, **c3(5))
    pa, pb = (v.cem(6, 9, 3, 0.3, iterations=2, seed=2) for v in (a, b))
    for v in (a, b):
        v.reset_t()
        v.step_t(None)
    for tick in range(2):
        before = fingerprint(a.swarm)[0]
        ra = pa.step_t()
        act = pb.plan()
        rb = b.step_t(act)
        torch.cuda.synchronize()
        assert act.data_ptr() == pb.action.data_ptr()
        for k in ("obs", "reward", "terminated", "truncated"):
            same_bytes(getattr(ra, k), getattr(rb, k), f"{k}, tick {tick}")
        same_bytes(pa.action, pb.action, "action")
        same_bytes(pa.mean, pb.mean, "mean")
        assert fingerprint(a.swarm)[0] != before                  # the env did advance
    obs = torch.zeros_like(a.swarm.obs)
    assert pa.step_t(obs=obs).obs.data_ptr() == obs.data_ptr()   # step_t's own buffers pass through
    a.close()
    b.close()
