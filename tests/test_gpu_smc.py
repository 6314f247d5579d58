"""The native particle (SMC) planner tick (qs_smc_*, `QuadSwarm.smc`, `SwarmVecEnv.smc`).

 1. Sample: particle 0 is the nominal in every segment, candidates are clipped, a zero sigma
    leaves its component alone, the noise is N(0, 1), segments and ticks draw different
    noise, a reset repeats the first draw, and the noise is keyed on the global env id.
 2. Weights, ESS and the resampling decision against a float64 numpy restatement made from
    the set's own ret / first_done and the planner's base.
 3. Systematic resampling as a property of the device's own weights, parents and offset.
 4. The chain end to end: every final particle's path, run on a twin swarm, gives the set's
    ret, first_done and state byte for byte.
 5. ess_frac = 0 is the long-horizon MPPI path: `BranchSet.rollout` of the candidates.
 6. Finish against the float64 restatement.
 7. plan() leaves the swarm as it was.
 8. plan() + step() captured into one graph replays what eager ticks compute.
 9. Refusals leave swarm, set and planner as they were.
10. `SwarmVecEnv.smc(...).step_t()`.

The default horizon is n = 40 in segments of L = 16: three segments, a ragged last one, and a
horizon past score_depth() = 32.
"""
import numpy as np
import pytest
import torch
from scipy import stats

from gym_pybullet_drones_amd import _lib as L
from gym_pybullet_drones_amd.envs.swarm import QuadSwarm, SMCPlanner
from gym_pybullet_drones_amd.vec_env.vec_env import SwarmVecEnv
from planner_case import A4, F64, c3, fingerprint, ks_normal, planner_bytes, prepared, random_sequence, same_bytes
from test_gpu_step_score import CONFIGS, Outs, running_score, set_clocks, snapshot

pytestmark = pytest.mark.gpu

BUFS = ("nominal", "candidates", "base", "weights", "parents", "ancestors", "ess", "offset", "resampled", "best", "action",
        "tick")
BLOCKS = (L.STATE_AGENT, L.STATE_ENV, L.STATE_HISTORY, L.STATE_EP_RETURN)
SET_BLOCKS = (L.STATE_AGENT, L.STATE_ENV, L.STATE_HISTORY)
N, SEG = 40, 16
# (config, particles): the per-thread variant; the per-workgroup one with C no multiple of 64; the same with
# env rows E apart; A = 4 on PYB in both; fp64 rewards
SHAPES = [(c3(3), 5), (c3(1), 300), (c3(5), 70), (A4, 4), (A4, 130), (F64, 3)]
SHAPE_IDS = ["c3x3_C5", "c3x1_C300", "c3x5_C70", "A4_C4", "A4_C130", "F64_C3"]


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy().copy()


def restate_weights(ret, fd, base, t, lam, pen):
    """Scores, weights and ESS in float64 numpy from (C, E) ret / first_done / base, t steps after the fork."""
    score = ret - np.where(fd < t, np.float64(pen), 0.0)
    logw = (score - base) / np.float64(lam)
    nan = np.isnan(logw)
    none = nan.all(axis=0)
    m = np.where(none, 0.0, np.max(np.where(nan, -np.inf, logw), axis=0))
    with np.errstate(invalid="ignore"):
        x = np.where(nan, 0.0, np.exp(logw - m))
    x[:, none] = 1.0
    w = x / x.sum(axis=0)
    return dict(score=score, w=w, ess=1.0 / (w * w).sum(axis=0), none=none)


def check_weights(got_w, got_ess, want):
    rel = np.abs(got_w - want["w"]) / np.maximum(want["w"], np.finfo(np.float64).tiny)
    ess_rel = np.abs(got_ess - want["ess"]) / want["ess"]
    print("weights: max relative difference", rel.max(), "ess:", ess_rel.max(), "sum - 1", np.abs(got_w.sum(axis=0) - 1).max())
    assert rel.max() <= 1e-12 and ess_rel.max() <= 1e-12


def resample_checked(pl, s, lam, pen, frac):
    """`pl.resample(s)` between a snapshot of what it reads and the checks of what it writes: weights, ESS
    and the decision against the restatement (2.), the parents as a property of the device's own weights and
    offset (3.), and the set gathered by them.  Returns the restatement and the mask of the resampled envs."""
    C = pl.num_particles
    ret, fd, base = host(pl.set.ret), host(pl.set.first_done), host(pl.base)
    t = (s + 1) * pl.segment
    pl.resample(s)
    want = restate_weights(ret, fd, base, t, lam, pen)
    w, ess = host(pl.weights), host(pl.ess)[s]
    check_weights(w, ess, want)
    # the inputs keep the comparison away from the threshold, so it cannot flip
    assert (np.abs(want["ess"] - frac * C) >= 1e-6 * C).all(), want["ess"]
    go = (want["ess"] < frac * C) & ~want["none"]
    assert np.array_equal(host(pl.resampled)[s], go.astype(np.int32))
    parents, u, new_base = host(pl.parents)[s], host(pl.offset)[s], host(pl.base)
    ident = np.arange(C, dtype=np.int32)[:, None]
    assert np.array_equal(parents[:, ~go], np.broadcast_to(ident, parents.shape)[:, ~go])
    assert not u[~go].any() and raw_eq(new_base[:, ~go], base[:, ~go])
    assert ((u >= 0) & (u < 1)).all() and np.array_equal(u * 2.0 ** 24, np.floor(u * 2.0 ** 24))
    # 3. systematic resampling, from the device's own weights: cum by numpy, delta = C * 2^-52
    cum = np.cumsum(w, axis=0)
    delta = C * 2.0 ** -52
    i = np.arange(C, dtype=np.float64)[:, None]
    pos = (i + u[None, :]) / np.float64(C)
    e_ix = np.broadcast_to(np.arange(w.shape[1])[None, :], parents.shape)
    assert ((parents >= 0) & (parents < C)).all()
    hi = cum[parents, e_ix]
    lo = np.where(parents > 0, cum[np.maximum(parents - 1, 0), e_ix], 0.0)
    ok = (lo - delta <= pos) & (pos < hi + delta)
    assert ok[:, go].all()
    assert (np.diff(parents, axis=0) >= 0)[:, go].all()                         # non-decreasing in i
    for e in np.flatnonzero(go):
        counts = np.bincount(parents[:, e], minlength=C)
        # within 1 of C * w_c; the interval a particle owns is its weight give or take the two roundings of cum
        assert (np.abs(counts - C * w[:, e]) <= 1 + 2 * C * delta).all(), (e, counts, C * w[:, e])
        assert raw_eq(new_base[:, e], want["score"][parents[:, e], e])           # byte for byte
    # qs_branch_select ran on parents[s]
    assert raw_eq(host(pl.set.ret), ret[parents, e_ix]) and np.array_equal(host(pl.set.first_done), fd[parents, e_ix])
    return want, go


def raw_eq(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def compose(parents):
    """ancestors from parents, on the host."""
    S, C, E = parents.shape
    anc = np.empty_like(parents)
    anc[S - 1] = np.arange(C, dtype=parents.dtype)[:, None]
    e_ix = np.broadcast_to(np.arange(E)[None, :], (C, E))
    for s in range(S - 2, -1, -1):
        anc[s] = parents[s][anc[s + 1], e_ix]
    return anc


def paths(cand, anc, Lseg):
    """(n, C, E, D, A): the action sequence of every final particle."""
    n, C, E = cand.shape[:3]
    e_ix = np.broadcast_to(np.arange(E)[None, :], (C, E))
    return np.stack([cand[j][anc[j // Lseg], e_ix] for j in range(n)], axis=0)


def smc(sw, C, n=N, seg=SEG, sigma=0.3, **kw):
    pl = sw.smc(n, C, sigma, segment=seg, **kw)
    assert isinstance(pl, SMCPlanner) and pl.segments == [(j, min(seg, n - j)) for j in range(0, n, seg)]
    return pl


# ------------------------------------------------------------------------ 1. sample
def test_sample_copies_the_nominal_and_clips():
    (sw,) = prepared(c3(5))
    pl = smc(sw, 33, sigma=0.8, seed=5)
    assert pl.segments == [(0, 16), (16, 16), (32, 8)] and sw.score_depth() == 32 < pl.horizon
    nom = random_sequence(pl)
    pl.reset(nom)
    for s in range(3):
        pl.sample(s)
    torch.cuda.synchronize()
    same_bytes(pl.nominal, nom, "reset copies the nominal")
    same_bytes(pl.candidates[:, 0], nom, "particle 0, every segment")
    c = pl.candidates.cpu().numpy()
    for a, b in pl.segments:
        seg = c[a:a + b]
        assert seg.min() >= -1.0 and seg.max() <= 1.0 and (seg == 1.0).any() and (seg == -1.0).any()
    assert not np.array_equal(c[:, 1], c[:, 2]) and not np.array_equal(c[:, 1, 0], c[:, 1, 1])
    assert int(pl.tick.item()) == 0          # sampling alone does not tick
    # a segment writes its own steps only
    pl.candidates.zero_()
    pl.sample(1)
    torch.cuda.synchronize()
    assert not pl.candidates[:16].any() and not pl.candidates[32:].any() and pl.candidates[16:32, 1:].any()
    sw.close()


def test_noise_is_standard_normal_and_segments_differ():
    sw = QuadSwarm(**c3(1))
    pl = smc(sw, 172, n=48, sigma=0.5, lo=-100.0, hi=100.0, seed=1)
    for s in range(3):
        pl.sample(s)
    z = pl.candidates[:, 1:].cpu().numpy() / 0.5          # zero nominal: 48 * 171 * 8 = 65 664 draws
    ks_normal(z)
    for a in range(3):
        for b in range(a + 1, 3):                          # the same local steps, another segment: other noise
            assert (z[16 * a:16 * a + 16] != z[16 * b:16 * b + 16]).mean() > 0.99
    sw.close()


def test_zero_sigma_leaves_its_component_alone_a4():
    sw = QuadSwarm(**A4)
    sigma = (0.5, 1.0, 2.0, 0.0)
    pl = smc(sw, 9, sigma=sigma, lo=-100.0, hi=100.0, seed=2)
    nom = random_sequence(pl)
    pl.reset(nom)
    for s in range(3):
        pl.sample(s)
    torch.cuda.synchronize()
    assert torch.equal(pl.candidates[..., 3], nom[:, None, ..., 3].expand(-1, 9, -1, -1))
    for a in range(3):
        assert not torch.equal(pl.candidates[:, 1, ..., a], nom[..., a])
    sw.close()


def test_ticks_differ_and_a_reset_repeats():
    (sw,) = prepared(c3(5))
    pl = smc(sw, 12, sigma=0.4, seed=9)
    nom = random_sequence(pl)
    pl.reset(nom)

    def draw():
        for s in range(3):
            pl.sample(s)
        return pl.candidates.clone()

    first = draw()
    pl.begin()
    pl.finish()                      # ret all zero: uniform weights; tick 0 -> 1
    pl.nominal.copy_(nom)            # the same nominal again, the tick is what differs
    second = draw()
    torch.cuda.synchronize()
    assert int(pl.tick.item()) == 1
    same_bytes(first[:, 0], second[:, 0], "particle 0 is the nominal at every tick")
    assert (first[:, 1:] != second[:, 1:]).float().mean() > 0.9
    pl.reset(nom)
    third = draw()
    torch.cuda.synchronize()
    assert int(pl.tick.item()) == 0
    same_bytes(third, first, "after reset the first sample repeats")
    sw.close()


def test_noise_is_keyed_on_the_global_env():
    whole, part = QuadSwarm(**c3(4)), QuadSwarm(**c3(2, env_offset=2))
    pw, pp = smc(whole, 9, seed=7), smc(part, 9, seed=7)
    nom = random_sequence(pw)
    pw.reset(nom)
    pp.reset(nom[:, 2:4].contiguous())
    for p in (pw, pp):
        for s in range(3):
            p.sample(s)
    torch.cuda.synchronize()
    same_bytes(pw.candidates[:, :, 2:4], pp.candidates, "global envs 2 and 3")
    assert not torch.equal(pw.candidates[:, 1:, 0:2], pw.candidates[:, 1:, 2:4])
    whole.close()
    part.close()


# ------------------------------------------------- 2. / 3. weights, ESS, systematic resampling
@pytest.mark.parametrize("cfg,C", SHAPES, ids=SHAPE_IDS)
def test_resample_on_real_rollouts(cfg, C):
    lam, frac = 0.05, 0.6
    (sw,) = prepared(cfg)
    pl = smc(sw, C, lam=lam, ess_frac=frac, seed=4)
    pl.reset(random_sequence(pl, scale=0.9))
    pl.begin()
    seen = []
    for s in range(2):
        pl.sample(s)
        pl.advance(s)
        assert pl.set.steps == (s + 1) * SEG
        want, go = resample_checked(pl, s, lam, 0.0, frac)
        seen.append(go)
        base = host(pl.base)          # after a resampling the next segment starts at log weight 0
        assert raw_eq(base[:, go], (host(pl.set.ret))[:, go])
    assert np.concatenate(seen).any()
    pl.resample(2)                    # the last segment: nothing is launched
    torch.cuda.synchronize()
    assert not host(pl.resampled)[2].any() and np.array_equal(host(pl.parents)[2], np.broadcast_to(
        np.arange(C, dtype=np.int32)[:, None], (C, sw.num_envs)))
    sw.close()


@pytest.mark.parametrize("C", [5, 70])
def test_resample_with_a_grounded_env_and_a_done_penalty(C):
    lam, pen, frac = 0.5, 2.5, 0.6
    (sw,) = prepared(c3(5), grounded=True)
    pl = smc(sw, C, lam=lam, done_penalty=pen, ess_frac=frac, seed=4)
    pl.reset(random_sequence(pl, scale=0.9))
    pl.begin()
    pl.sample(0)
    pl.advance(0)
    torch.cuda.synchronize()
    assert (pl.set.first_done[:, 4] == 0).all()                 # the grounded env is done at once, in every particle
    # some particles of an env done and others not (by hand: resample reads the set as it is)
    pl.set.first_done[0::2, 1] = 3
    pl.set.first_done[1, 2] = 0
    ret, fd, base = host(pl.set.ret), host(pl.set.first_done), host(pl.base)
    want, go = resample_checked(pl, 0, lam, pen, frac)
    free = restate_weights(ret, fd, base, SEG, lam, 0.0)
    assert not np.allclose(want["w"][:, 1], free["w"][:, 1]) and np.allclose(want["w"][:, 4], free["w"][:, 4])
    sw.close()


def synthetic_ret(C, E, device):
    """Env 0: all equal; env 1: one dominant particle; env 2: a NaN among finite values; env 3: all NaN;
    env 4: spread out."""
    assert E == 5
    gen = torch.Generator(device="cpu").manual_seed(21)
    ret = torch.zeros((C, E), dtype=torch.float64)
    ret[:, 0] = -3.25
    ret[:, 1] = -torch.rand(C, generator=gen, dtype=torch.float64)
    ret[C // 2, 1] = 40.0
    ret[:, 2] = torch.rand(C, generator=gen, dtype=torch.float64) * 4
    ret[C // 3, 2] = float("nan")
    ret[:, 3] = float("nan")
    ret[:, 4] = torch.rand(C, generator=gen, dtype=torch.float64) * 6
    return ret.to(device)


@pytest.mark.parametrize("C", [5, 70, 300])
def test_resample_on_synthetic_returns(C):
    lam, frac = 1.0, 0.5
    (sw,) = prepared(c3(5))
    pl = smc(sw, C, lam=lam, ess_frac=frac, seed=6)
    pl.begin()
    pl.sample(0)
    pl.advance(0)
    pl.set.ret.copy_(synthetic_ret(C, 5, sw.device))
    want, go = resample_checked(pl, 0, lam, 0.0, frac)
    w, ess = host(pl.weights), host(pl.ess)[0]
    assert np.array_equal(w[:, 0], np.full(C, 1.0 / C)) and abs(ess[0] - C) <= 1e-12 * C and not go[0]     # all equal
    assert go[1] and ess[1] < 1.0 + 1e-9 and (host(pl.parents)[0][:, 1] == C // 2).all()                    # one dominant
    assert w[C // 3, 2] == 0.0 and np.isfinite(w[:, 2]).all() and abs(w[:, 2].sum() - 1) < 1e-14            # a NaN
    assert np.array_equal(w[:, 3], np.full(C, 1.0 / C)) and not go[3] and want["none"][3]                   # all NaN
    assert not (host(pl.parents)[0][:, 2] == C // 3).any() or not go[2]      # a weightless particle has no offspring
    sw.close()


def test_offset_is_uniform():
    """E = 4 096, C = 2, four resampling segments a tick, four ticks: 2^16 offsets."""
    E, C, ticks = 4096, 2, 4
    (sw,) = prepared(c3(E), warm=0)
    pl = smc(sw, C, n=5, seg=1, lam=1.0, ess_frac=1.0, seed=12)
    force = torch.zeros((C, E), dtype=torch.float64, device=sw.device)
    got = []
    for tick in range(ticks):
        pl.begin()
        for s in range(4):
            force[1] = 50.0 * (s + 1)          # particle 1 dominates again, whatever base has become
            pl.set.ret.copy_(force)
            pl.resample(s)
        torch.cuda.synchronize()
        assert pl.resampled[:4].all() and not pl.resampled[4].any()
        got.append(host(pl.offset)[:4])
        pl.finish()
    u = np.concatenate(got).ravel()
    assert u.size == 1 << 16 and ((u >= 0) & (u < 1)).all()
    d = stats.kstest(u, "uniform").statistic
    print(f"N = {u.size}: KS {d:.5f} (critical {1.95 / np.sqrt(u.size):.5f}), mean {u.mean():.5f}")
    assert d < 1.95 / np.sqrt(u.size)
    assert len(np.unique(u)) > 0.99 * u.size                   # ticks, segments and envs never share a draw
    for a in range(ticks):
        for b in range(a + 1, ticks):
            assert (got[a] != got[b]).mean() > 0.99            # keyed on the tick
    sw.close()


def test_offset_is_keyed_on_the_global_env():
    whole, part = prepared(c3(4), warm=0)[0], prepared(c3(2, env_offset=2), warm=0)[0]
    pw, pp = (smc(sw, 3, n=3, seg=1, ess_frac=1.0, seed=7) for sw in (whole, part))
    for p in (pw, pp):
        p.begin()
        for s in range(2):
            p.set.ret[2] = 60.0 * (s + 1)      # particle 2 dominates again, whatever base has become
            p.resample(s)
    torch.cuda.synchronize()
    assert pw.resampled[:2].all() and pp.resampled[:2].all()
    same_bytes(pw.offset[:, 2:4], pp.offset, "global envs 2 and 3")
    assert not torch.equal(pw.offset[:2, 0:2], pw.offset[:2, 2:4])
    whole.close()
    part.close()


# --------------------------------------------------------------------- 4. the chain
CHAIN = {
    "c3x3_C5": (c3(3), 5, None),
    "c3x3_C5_truncations": (c3(3), 5, (3, 20, None)),        # env 0 ends in segment 0, env 1 in segment 1
    "spiral": (CONFIGS["spiral_d5_vel"], 3, None),
    "f64": (CONFIGS["mh_d8_onedpid_f64"], 3, None),
}


@pytest.mark.parametrize("name", list(CHAIN))
def test_every_final_particle_ran_its_path(name):
    cfg, C, clocks = CHAIN[name]
    sw, ref = prepared(cfg, twins=1)
    if clocks:
        for s in (sw, ref):
            set_clocks(s, clocks)
    pl = smc(sw, C, lam=0.05, ess_frac=1.0, seed=4)
    pl.reset(random_sequence(pl, scale=0.9))
    snap = snapshot(sw)
    pl.plan()
    torch.cuda.synchronize()
    assert pl.set.steps == N and int(pl.tick.item()) == 1
    resampled = host(pl.resampled)
    print("resampled", resampled.tolist(), "ess", host(pl.ess).tolist())
    assert not resampled[2].any() and (resampled[:2].all() if name == "c3x3_C5" else resampled[:2].any())
    parents, anc = host(pl.parents), host(pl.ancestors)
    assert np.array_equal(anc, compose(parents))
    assert (anc[0] != np.arange(C)[:, None]).any()
    path = torch.from_numpy(paths(host(pl.candidates), anc, SEG)).to(sw.device)       # (n, C, E, D, A)
    E = sw.num_envs
    rew = np.zeros((N, C, E), np.float64)
    term, trunc = np.zeros((N, C, E), np.uint8), np.zeros((N, C, E), np.uint8)
    got_state = [pl.set.get_state(blk) for blk in SET_BLOCKS]
    for c in range(C):
        for blk, val in zip(BLOCKS, snap):
            ref.set_state(blk, val)
        one = Outs(ref, N)
        ref.step_many(one.kws(), actions=path[:, c].contiguous())
        torch.cuda.synchronize()
        rew[:, c], term[:, c], trunc[:, c] = (one.bufs[k].cpu().numpy() for k in ("reward", "terminated", "truncated"))
        for blk, got in zip(SET_BLOCKS, got_state):
            same_bytes(got[:, c], ref.get_state(blk), f"state block {blk} of particle {c}")
    ret, fd = running_score(rew, term, trunc)
    same_bytes(pl.set.ret, ret, "ret")
    same_bytes(pl.set.first_done, fd, "first_done")
    if clocks:
        assert (fd[:, 0] == 3).all() and (fd[:, 1] == 20).all() and (fd[:, 2] == N).all()
    sw.close()
    ref.close()


# ------------------------------------------------------------------ 5. ess_frac = 0
@pytest.mark.parametrize("cfg,C", [(c3(3), 5), (c3(1), 300)], ids=["c3x3_C5", "c3x1_C300"])
def test_without_resampling_the_tick_is_a_long_rollout(cfg, C):
    sw, twin = prepared(cfg, twins=1)
    pl = smc(sw, C, lam=0.3, ess_frac=0.0, seed=4)
    pl.reset(random_sequence(pl, scale=0.9))
    pl.plan()
    torch.cuda.synchronize()
    bs = twin.branches(C)
    bs.fork()
    bs.rollout(pl.candidates)
    torch.cuda.synchronize()
    same_bytes(pl.set.ret, bs.ret, "ret")
    same_bytes(pl.set.first_done, bs.first_done, "first_done")
    ident = np.broadcast_to(np.arange(C, dtype=np.int32)[None, :, None], (3, C, sw.num_envs))
    assert np.array_equal(host(pl.parents), ident) and np.array_equal(host(pl.ancestors), ident)   # no select ran
    assert not pl.resampled.any() and not pl.offset.any() and not pl.base.any()
    check_finish(pl, 0.3, 0.0, 1.0, tick=1)
    bs.close()
    sw.close()
    twin.close()


# ------------------------------------------------------------------------ 6. finish
def check_finish(pl, lam, pen, bound, tick):
    """The planner's buffers after a finish against the float64 restatement, made from the set's ret and
    first_done, the planner's base, parents and candidates (none of which finish writes)."""
    n, Lseg = pl.horizon, pl.segment
    want = restate_weights(host(pl.set.ret), host(pl.set.first_done), host(pl.base), n, lam, pen)
    w, S = host(pl.weights), len(pl.segments)
    check_weights(w, host(pl.ess)[S - 1], want)
    assert np.array_equal(host(pl.best), np.argmax(want["w"], axis=0).astype(np.int32))   # the lowest c of the maximum
    anc = compose(host(pl.parents))
    assert np.array_equal(host(pl.ancestors), anc)
    new = np.einsum("ce,jceda->jeda", want["w"], paths(host(pl.candidates).astype(np.float64), anc, Lseg))
    nominal, action = host(pl.nominal).astype(np.float64), host(pl.action).astype(np.float64)
    tol = 2.0 ** -23 * bound
    want_nominal = np.concatenate([new[1:], new[-1:]], axis=0)
    print("nominal: max abs difference", np.abs(nominal - want_nominal).max(), "allowed", tol)
    assert np.abs(nominal - want_nominal).max() <= tol and np.abs(action - new[0]).max() <= tol
    assert np.array_equal(nominal[-1], nominal[-2] if n > 1 else nominal[0])    # the hold
    assert int(pl.tick.item()) == tick
    return want


@pytest.mark.parametrize("cfg,C", SHAPES, ids=SHAPE_IDS)
def test_finish_matches_the_float64_restatement(cfg, C):
    lam = 0.1
    (sw,) = prepared(cfg)
    pl = smc(sw, C, lam=lam, ess_frac=0.7, seed=4)
    pl.reset(random_sequence(pl, scale=0.9))
    pl.plan()
    want = check_finish(pl, lam, 0.0, 1.0, tick=1)
    assert host(pl.resampled)[:2].any() and (want["w"] > 0).any()
    pl.plan()                                                   # a second tick, from the shifted nominal
    check_finish(pl, lam, 0.0, 1.0, tick=2)
    sw.close()


@pytest.mark.parametrize("n,seg", [(1, 16), (16, 16), (256, 1)], ids=["n1", "nL", "n256_L1"])
def test_finish_at_the_ends_of_the_range(n, seg):
    (sw,) = prepared(c3(1))
    pl = smc(sw, 2, n=n, seg=seg, lam=0.05, ess_frac=1.0, seed=4)
    assert len(pl.segments) == -(-n // seg) and pl.parents.shape == (len(pl.segments), 2, 1)
    pl.reset(random_sequence(pl, scale=0.9))
    pl.plan()
    check_finish(pl, 0.05, 0.0, 1.0, tick=1)
    assert pl.set.steps == n
    if n == 256:
        assert host(pl.resampled)[:255].any() and (host(pl.ancestors)[0] != np.arange(2)[:, None]).any()
    sw.close()


# ------------------------------------------------------------------- 7. no mutation
@pytest.mark.parametrize("cfg,C", [(c3(21), 3), (c3(1), 300)], ids=["c3x21_C3", "c3x1_C300"])
def test_plan_leaves_the_swarm_alone(cfg, C):
    (sw,) = prepared(cfg, grounded=cfg["num_envs"] > 4)
    pl = smc(sw, C, lam=0.1, ess_frac=0.8, seed=4)
    before = fingerprint(sw)
    pl.plan()
    pl.plan()
    assert fingerprint(sw) == before
    assert int(pl.tick.item()) == 2 and pl.resampled.any()
    sw.close()


# ------------------------------------------------------- 8. determinism and capture
@pytest.mark.parametrize("cfg,C", [(c3(5), 3), (c3(1), 300)], ids=["c3x5_C3", "c3x1_C300"])
def test_captured_tick_replays_what_eager_ticks_compute(cfg, C):
    cap, eager = prepared(cfg, twins=1)
    pc, pe = (smc(sw, C, lam=0.1, ess_frac=0.8, seed=8) for sw in (cap, eager))
    nom = random_sequence(pc, scale=0.9)
    pc.reset(nom)
    pe.reset(nom)
    keys = ("parents", "offset", "nominal", "action", "candidates", "weights", "ancestors", "ess", "resampled", "best", "base")
    want = []
    for _ in range(3):
        pe.plan()
        r = eager.step(pe.action)
        torch.cuda.synchronize()
        want.append(({k: getattr(pe, k).clone() for k in keys}, r.obs.clone(), r.reward.clone(), pe.set.ret.clone()))
    assert not torch.equal(want[0][0]["candidates"][:, 1:], want[1][0]["candidates"][:, 1:])
    assert any(w[0]["resampled"].any() for w in want)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        pc.plan()
        r = cap.step(pc.action)
    for k in range(3):
        g.replay()
        torch.cuda.synchronize()
        assert int(pc.tick.item()) == k + 1
        for key in keys:
            same_bytes(getattr(pc, key), want[k][0][key], f"{key}, tick {k}")
        same_bytes(r.obs, want[k][1], f"obs, tick {k}")
        same_bytes(r.reward, want[k][2], f"reward, tick {k}")
        same_bytes(pc.set.ret, want[k][3], f"the set's ret, tick {k}")
    assert fingerprint(cap)[:4] == fingerprint(eager)[:4]     # (launch counts aside: a capture counts its node once)
    cap.close()
    eager.close()


# --------------------------------------------------------------------- 9. refusals
def set_bytes(pl):
    torch.cuda.synchronize()
    return [t.cpu().numpy().tobytes() for t in (pl.set.ret, pl.set.first_done, pl.set.ret_agent)]


def test_refusals_leave_swarm_set_and_planner_alone():
    sw = QuadSwarm(**c3(21))
    depth = sw.score_depth()
    pl = smc(sw, 3, seed=4)                              # creating a planner needs no reset
    pl.reset(random_sequence(pl))
    held, held_set = planner_bytes(pl, BUFS), set_bytes(pl)
    for call in (pl.plan, pl.begin):
        with pytest.raises(L.QuadSwarmError, match="rc=-4.*qs_reset"):   # QS_E_STATE: before qs_reset
            call()
    for call in (pl.advance, pl.resample):
        with pytest.raises(L.QuadSwarmError, match="rc=-4.*qs_smc_begin"):   # ... and before the first begin
            call(0)
    assert planner_bytes(pl, BUFS) == held and set_bytes(pl) == held_set
    sw.reset(3)
    sw.step(None)
    before = fingerprint(sw)
    ok = dict(horizon=40, particles=3, sigma=0.3, segment=16)
    for bad in (dict(horizon=0), dict(horizon=-1), dict(horizon=257, segment=1), dict(horizon=256 * 16 + 1),
                dict(segment=0), dict(segment=depth + 1), dict(particles=1), dict(particles=0), dict(particles=4097),
                dict(lo=1.0, hi=1.0), dict(lo=0.5, hi=-0.5), dict(sigma=-0.1), dict(sigma=float("nan")),
                dict(done_penalty=-0.5), dict(done_penalty=float("inf")), dict(lam=0.0), dict(lam=-1.0),
                dict(lam=float("inf")), dict(lam=float("nan")), dict(ess_frac=-0.01), dict(ess_frac=1.01),
                dict(ess_frac=float("nan"))):
        with pytest.raises(L.QuadSwarmError, match="rc=-1.*qs_smc_create"):
            sw.smc(**{**ok, **bad})
    for good in (dict(horizon=256, segment=1, particles=2), dict(segment=depth, horizon=depth + 1), dict(ess_frac=1.0),
                 dict(ess_frac=0.0), dict(lam=1e-300), dict(done_penalty=0.0, sigma=0.0)):
        sw.smc(**{**ok, **good}).close()                  # the last accepted values
    with pytest.raises(ValueError):
        sw.smc(40, 3, (0.1, 0.2))                          # one sigma per component, A = 1
    with pytest.raises(ValueError):
        pl.reset(torch.zeros((N, 21, 8), device=sw.device))
    for call in (pl.sample, pl.advance, pl.resample):
        for s in (-1, 3):
            with pytest.raises(L.QuadSwarmError, match="rc=-1.*segment"):
                call(s)
    assert fingerprint(sw) == before and planner_bytes(pl, BUFS) == held and set_bytes(pl) == held_set
    pl.plan()                                              # and the planner still works
    torch.cuda.synchronize()
    assert int(pl.tick.item()) == 1
    sw.close()                                             # closes its planners first
    assert not pl._p and not pl.set._p


@pytest.mark.parametrize("cfg,why", [
    (dict(task="multihover", num_drones=4, num_envs=16, act="rpm"), "cannot score"),   # the default diagonal layout
    (dict(task="flock", num_drones=4, num_envs=16, act="rpm"), "cannot score"),
])
def test_handles_that_cannot_score_cannot_plan(cfg, why):
    sw = QuadSwarm(**cfg)
    sw.reset(3)
    before = fingerprint(sw)
    with pytest.raises(L.QuadSwarmError, match="rc=-1.*" + why):
        sw.smc(40, 3, 0.3, segment=16)
    assert fingerprint(sw) == before
    sw.close()


# --------------------------------------------------------------------- 10. vec env
def test_vec_env_planner_step_t():
    a, b = SwarmVecEnv(seed=3, **c3(5)), SwarmVecEnv(seed=3, **c3(5))
    pa, pb = (v.smc(N, 9, 0.3, segment=SEG, lam=0.1, ess_frac=0.8, seed=2) for v in (a, b))
    assert isinstance(pa, SMCPlanner)
    for v in (a, b):
        v.reset_t()
        v.step_t(None)
    for tick in range(2):
        ra = pa.step_t()
        act = pb.plan()
        rb = b.step_t(act)
        torch.cuda.synchronize()
        assert act.data_ptr() == pb.action.data_ptr()
        for k in ("obs", "reward", "terminated", "truncated"):
            same_bytes(getattr(ra, k), getattr(rb, k), f"{k}, tick {tick}")
        same_bytes(pa.action, pb.action, "action")
        same_bytes(pa.nominal, pb.nominal, "nominal")
    obs = torch.zeros_like(a.swarm.obs)
    assert pa.step_t(obs=obs).obs.data_ptr() == obs.data_ptr()   # step_t's own buffers pass through
    a.close()
    b.close()
