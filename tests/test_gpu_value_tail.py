"""The value tail of the MPPI and CEM ticks (qs_value_tail, qs_value_mppi_* / qs_value_cem_*;
`MPPIPlanner.set_value`, `.score`, `.clear_value`): discounted, critic-bootstrapped returns.

  1. qs_value_tail alone on synthetic inputs: `value` against torch's float32 forward
     (rtol = atol = 1e-5, with and without the float64 normaliser), every hidden size, input
     widths that are no multiple of the MFMA's k or of the K-chunk, row counts that are no
     multiple of the row tile, and both row tiles;
  2. the fold, bit for bit against its float64 NumPy restatement, and the launch's determinism;
  3. a constant critic moves MPPI's best / CEM's first elite to the surviving candidate
     exactly when the bootstrap term outweighs the difference of the returns;
  4. discount only (no net), and gamma = 1 with no net, which launches nothing;
  5. the MPPI and CEM ticks stage by stage with a random critic;
  6. plan() with a value attached leaves the swarm alone;
  7. a captured tick replays the eager ticks and reads the critic's weights live;
  8. refusals leave planner and swarm as they were;
  9. clear_value() returns the planner to the plain tick."""
import numpy as np
import pytest
import torch

from gym_pybullet_drones_amd import _lib as L
from gym_pybullet_drones_amd.envs.swarm import QuadSwarm, grid_layout, value_spec
from planner_case import c3, fingerprint, planner_bytes, prepared, random_sequence, same_bytes
from value_case import (CEM_BUFS, MPPI_BUFS, SPIRAL64, assert_close, cem_refit_and_check, critic_of, fold64, forward32,
                        mppi_check_update, normalizer_of, raw_set, tail, weights_of)

pytestmark = pytest.mark.gpu
DEV = "cuda"


def synthetic(C, E, D, O, seed):
    """Rows of N(0, 2) inputs; column 3 holds values far past the normaliser's clip."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn((C, E, D, O), generator=gen) * 2.0
    x.view(C * E, D * O)[:, 3] *= 100.0
    return x.to(DEV)


# ------------------------------------------------------------------ 1. the launch alone
def check_value(N, D, O, C, E):
    I, n = D * O, 5
    critic = critic_of(I, N, seed=N + I, device=DEV)
    x = synthetic(C, E, D, O, seed=C + I)
    fd = torch.full((C, E), n, dtype=torch.int32, device=DEV)
    for nz in (None, normalizer_of(I, seed=I, device=DEV, zero_var_col=min(5, I - 1))):
        spec, keep = value_spec(critic, 1.0, 1.0, nz)
        ret = torch.zeros((C, E), dtype=torch.float64, device=DEV)
        value = torch.full((C, E), float("nan"), device=DEV)
        assert tail(spec, n, C, E, D, O, x, None, ret, fd, value) == 0, L.load().qs_last_error()
        torch.cuda.synchronize()
        want = forward32(x.view(C * E, I), critic, nz)
        assert_close(value, want, f"value, N = {N}, I = {I}, V = {C * E}, normaliser {nz is not None}")
        assert_close(value.view(-1)[-1:], want[-1:], "the last row of the last tile")
        assert torch.equal(ret, value.double())     # gamma = 1, never done: 0 + (1 * 1) * V
        if nz is not None:                          # the extremes reach the net as the clip, not as an inf or a NaN
            y = (x.view(C * E, I).double() - nz.rms.mean) / torch.sqrt(nz.rms.var + nz.epsilon)
            assert (y[:, 3].abs() > nz.clip).any() and (y[:, min(5, I - 1)].abs() > nz.clip).any()


@pytest.mark.parametrize("C,E", [(1, 1), (33, 5), (257, 1)])
@pytest.mark.parametrize("D,O", [(2, 27), (8, 27), (5, 38), (1, 13)])
@pytest.mark.parametrize("N", [64, 128, 256])
def test_value_matches_the_float32_forward(N, D, O, C, E):
    check_value(N, D, O, C, E)


# 8 225 rows are more than 16 rows x 256 compute units: N = 64 and 128 take the 32-row tile (value_sizes.h), with
# a partial last tile, at the narrowest and the widest of the inputs above
@pytest.mark.parametrize("D,O", [(8, 27), (1, 13)])
@pytest.mark.parametrize("N", [64, 128])
def test_value_on_the_wide_row_tile(N, D, O):
    check_value(N, D, O, 8225, 1)


# ------------------------------------------------------------------------- 2. the fold
@pytest.mark.parametrize("scale", [1.0, -2.5])
@pytest.mark.parametrize("gamma", [1.0, 0.99, 0.5])
@pytest.mark.parametrize("rdtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
def test_the_fold_is_exact(rdtype, gamma, scale):
    n, C, E, D, O, N = 7, 33, 5, 2, 27, 64
    critic = critic_of(D * O, N, seed=2, device=DEV)
    x = synthetic(C, E, D, O, seed=9)
    gen = torch.Generator().manual_seed(31)
    fd = torch.randint(0, n + 1, (C, E), generator=gen, dtype=torch.int32)
    fd[0, 0], fd[-1, -1], fd[1, 0], fd[1, 1] = 0, n, n - 1, n
    assert fd.min() == 0 and fd.max() == n
    rewards = [(torch.randn((C, E), generator=gen, dtype=torch.float64) - 0.5).to(rdtype).to(DEV) for _ in range(n)]
    ret0 = torch.randn((C, E), generator=gen, dtype=torch.float64).to(DEV)
    fd = fd.to(DEV)
    spec, keep = value_spec(critic, gamma, scale)
    got = []
    for _ in range(2):
        ret, value = ret0.clone(), torch.zeros((C, E), device=DEV)
        assert tail(spec, n, C, E, D, O, x, rewards if gamma != 1.0 else None, ret, fd, value) == 0
        torch.cuda.synchronize()
        got.append((ret.cpu().numpy(), value.cpu().numpy()))
    assert got[0][0].tobytes() == got[1][0].tobytes() and got[0][1].tobytes() == got[1][1].tobytes()   # determinism
    ret, value = got[0]
    rw = np.stack([r.cpu().numpy() for r in rewards])
    want = fold64(n, gamma, scale, fd.cpu().numpy(), value, rw, ret0.cpu().numpy())
    assert ret.tobytes() == want.tobytes()
    # rows that ended inside the horizon carry no value term
    plain = fold64(n, gamma, scale, fd.cpu().numpy(), None, rw, ret0.cpu().numpy())
    ended = fd.cpu().numpy() < n
    assert np.array_equal(ret[ended], plain[ended]) and not np.array_equal(ret[~ended], plain[~ended])
    assert_close(torch.from_numpy(value), forward32(x.view(C * E, D * O), critic), "value")
    # and without a net: the discounted sum alone (gamma = 1: nothing to do, ret stays)
    spec0, _ = value_spec(None, gamma, scale)
    ret = ret0.clone()
    assert tail(spec0, n, C, E, D, O, None, rewards if gamma != 1.0 else None, ret, fd, None) == 0
    torch.cuda.synchronize()
    assert ret.cpu().numpy().tobytes() == plain.tobytes()


# ------------------------------------------------------------------ 3. a constant critic
def constant_critic(I, v0):
    critic = critic_of(I, 64, seed=1, device=DEV)
    with torch.no_grad():
        for p in critic.parameters():
            p.zero_()
        critic.v_net.fcs[2].bias.fill_(v0)
    return critic


def split_swarm():
    """A MultiHover swarm whose env 4 has drone 0 just above the crash height and sinking: the
    candidate that pushes every drone down ends the episode inside the horizon, the one that
    pushes up does not."""
    (sw,) = prepared(c3(5))
    st = sw.get_state(L.STATE_AGENT).clone()
    st[L.F_POS + 2, 4 * sw.num_drones] = 0.045
    st[L.F_VEL + 2, 4 * sw.num_drones] = -0.05
    sw.set_state(L.STATE_AGENT, st)
    return sw


def down_and_up(pl):
    pl.candidates[:, 0] = -1.0
    pl.candidates[:, 1] = 1.0


@pytest.mark.parametrize("kind", ["mppi", "cem"])
def test_constant_critic_moves_the_choice_to_the_survivor(kind):
    n, gamma, e = 7, 0.99, 4
    sw = split_swarm()
    pl = sw.mppi(n, 2, 0.3, lam=0.0, seed=4) if kind == "mppi" else sw.cem(n, 2, 1, 0.3, iterations=1, seed=4)

    def tick(first):
        if kind == "mppi":
            pl.sample()
        else:
            pl.begin()
            pl.sample(0)
        down_and_up(pl)
        pl.score()
        pl.update() if kind == "mppi" else pl.refit(0)
        torch.cuda.synchronize()
        return int((pl.best if kind == "mppi" else pl.elites[0])[e].item())

    pl.set_value(None, gamma=gamma)                       # the discounted returns of the two candidates
    first = tick(True)
    fd, g = pl.first_done.cpu().numpy()[:, e], pl.ret.cpu().numpy()[:, e]
    assert fd[0] < n and fd[1] == n, f"the scenario: first_done of (down, up) in env {e} is {fd}"
    disc_n = fold64(n, gamma, 1.0, np.full((1,), n, np.int32), np.ones((1,), np.float32), np.zeros((n, 1)))[0]
    need = (g[0] - g[1]) / disc_n                          # the value at which the two returns meet
    print(f"returns (ended, survived) = {g}, disc[n] = {disc_n}, v0 at the tie = {need}")
    assert first == (1 if g[1] > g[0] else 0)
    for v0, survivor in ((need + 1e-3 * (1 + abs(need)), True), (need - 1e-3 * (1 + abs(need)), False)):
        critic = constant_critic(sw.num_drones * sw.obs_dim, v0)
        pl.set_value(critic, gamma=gamma)
        choice = tick(False)
        assert torch.equal(pl.value, torch.full_like(pl.value, v0))          # tanh(0) = 0: exactly b3
        ret = pl.ret.cpu().numpy()[:, e]
        assert ret[0] == g[0] and ret[1] == g[1] + np.float64(disc_n) * np.float64(np.float32(v0))
        assert (ret[1] > ret[0]) == survivor and choice == (1 if survivor else 0), (v0, ret, choice)
    sw.close()


# ------------------------------------------------------------------- 4. discount only
def test_discount_only_and_the_plain_tick():
    n, C, gamma = 7, 33, 0.9
    a, b = prepared(c3(5), twins=1, grounded=True)
    pa, pb = (sw.mppi(n, C, 0.3, lam=0.5, done_penalty=1.5, seed=6) for sw in (a, b))
    nom = random_sequence(pa, scale=0.9)
    pa.reset(nom)
    pb.reset(nom)
    pa.set_value(None, gamma=gamma)
    assert pa.last_obs is None and pa.value is None and tuple(pa.rewards.shape) == (n, C, 5)
    pa.sample()
    pa.score()
    torch.cuda.synchronize()
    rew = [torch.empty((C, 5), device=DEV) for _ in range(n)]
    ret, fd = torch.empty((C, 5), dtype=torch.float64, device=DEV), torch.empty((C, 5), dtype=torch.int32, device=DEV)
    a.score(pa.candidates, [dict(reward=r) for r in rew], ret=ret, first_done=fd)
    torch.cuda.synchronize()
    same_bytes(pa.rewards, torch.stack(rew), "rewards")
    same_bytes(pa.first_done, fd, "first_done")
    assert (fd[:, 4] == 0).all() and (fd[:, 0] == n).all()
    want = fold64(n, gamma, 1.0, fd.cpu().numpy(), None, pa.rewards.cpu().numpy())
    assert pa.ret.cpu().numpy().tobytes() == want.tobytes()
    assert not np.array_equal(want, ret.cpu().numpy())
    pa.update()
    mppi_check_update(pa, 0.5, 1.5, 1.0, tick=1)
    # gamma = 1 and no net: three ticks are those of a planner that never had a value, in bytes and in launches
    pa.reset(nom)
    pa.set_value(None, gamma=1.0)
    assert pa.last_obs is None and pa.value is None and pa.rewards is None
    for k in range(3):
        pa.plan()
        pb.plan()
        assert planner_bytes(pa, MPPI_BUFS) == planner_bytes(pb, MPPI_BUFS), f"tick {k}"
        a.step(pa.action)
        b.step(pb.action)
    assert fingerprint(a) == fingerprint(b)
    a.close()
    b.close()


# ------------------------------------------------------------- 5. the ticks, stage by stage
def reference_score(sw, pl, n, C):
    """What QuadSwarm.score writes itself for the planner's candidates: last obs, rewards, ret, first_done."""
    E = sw.num_envs
    obs = torch.empty((C, E, sw.num_drones, sw.obs_dim), device=DEV)
    rew = [torch.empty((C, E), dtype=sw.rdtype, device=DEV) for _ in range(n)]
    ret, fd = torch.empty((C, E), dtype=torch.float64, device=DEV), torch.empty((C, E), dtype=torch.int32, device=DEV)
    outs = [dict(reward=r) for r in rew]
    outs[-1]["obs"] = obs
    sw.score(pl.candidates, outs, ret=ret, first_done=fd)
    torch.cuda.synchronize()
    return obs, torch.stack(rew), ret, fd


def check_score(sw, pl, n, C, critic, nz, gamma, scale):
    obs, rew, ret, fd = reference_score(sw, pl, n, C)
    same_bytes(pl.last_obs, obs, "last_obs")
    same_bytes(pl.first_done, fd, "first_done")
    if gamma != 1.0:
        same_bytes(pl.rewards, rew, "rewards")
    else:
        assert pl.rewards is None
    assert_close(pl.value, forward32(obs.view(C * sw.num_envs, -1), critic, nz), "value")
    want = fold64(n, gamma, scale, fd.cpu().numpy(), pl.value.cpu().numpy(), rew.cpu().numpy(), ret.cpu().numpy())
    assert pl.ret.cpu().numpy().tobytes() == want.tobytes()
    return fd.cpu().numpy()


TICK_CASES = [(cfg, N, norm) for cfg in ("mh32", "spiral64") for N in (64, 256) for norm in (False, True)]


def tick_setup(cfg, N, norm):
    (sw,) = prepared(c3(5), grounded=True) if cfg == "mh32" else prepared(SPIRAL64)
    I = sw.num_drones * sw.obs_dim
    critic = critic_of(I, N, seed=N, device=DEV)
    nz = normalizer_of(I, seed=3, device=DEV) if norm else None
    gamma = 0.99 if (N == 64) == norm else 1.0
    return sw, critic, nz, gamma, -1.5


@pytest.mark.parametrize("cfg,N,norm", TICK_CASES)
def test_mppi_tick_with_a_critic(cfg, N, norm):
    n, C, lam, pen = 7, 33, 0.5, 1.5
    sw, critic, nz, gamma, scale = tick_setup(cfg, N, norm)
    pl = sw.mppi(n, C, 0.3, lam=lam, done_penalty=pen, seed=5)
    pl.reset(random_sequence(pl, scale=0.9))
    pl.set_value(critic, gamma=gamma, scale=scale, obs_normalizer=nz)
    for k in range(2):
        pl.sample()
        pl.score()
        fd = check_score(sw, pl, n, C, critic, nz, gamma, scale)
        if cfg == "mh32":
            assert (fd[:, 4] == 0).all() and (fd[:, :4] == n).all()
        pl.update()
        mppi_check_update(pl, lam, pen, 1.0, tick=k + 1)
    sw.close()


@pytest.mark.parametrize("cfg,N,norm", TICK_CASES)
def test_cem_tick_with_a_critic(cfg, N, norm):
    n, C, K, iters = 7, 33, 5, 2
    sw, critic, nz, gamma, scale = tick_setup(cfg, N, norm)
    pl = sw.cem(n, C, K, 0.3, iterations=iters, done_penalty=1.5, seed=5)
    pl.reset(random_sequence(pl, scale=0.9))
    pl.set_value(critic, gamma=gamma, scale=scale, obs_normalizer=nz)
    pl.begin()
    for i in range(iters):
        pl.sample(i)
        pl.score()
        check_score(sw, pl, n, C, critic, nz, gamma, scale)
        cem_refit_and_check(pl, i)
    pl.finish()
    torch.cuda.synchronize()
    assert int(pl.tick.item()) == 1
    sw.close()


# ------------------------------------------------------------------------ 6. no mutation
@pytest.mark.parametrize("kind", ["mppi", "cem"])
def test_plan_with_a_value_leaves_the_swarm_alone(kind):
    (sw,) = prepared(c3(5), grounded=True)
    pl = sw.mppi(7, 33, 0.3, seed=5) if kind == "mppi" else sw.cem(7, 33, 5, 0.3, iterations=2, seed=5)
    pl.set_value(critic_of(216, 64, seed=4, device=DEV), gamma=0.99, obs_normalizer=normalizer_of(216, 3, DEV))
    before = fingerprint(sw)
    pl.plan()
    pl.plan()
    assert fingerprint(sw) == before
    assert torch.isfinite(pl.value).all() and pl.value.abs().max() > 0
    sw.close()


# ---------------------------------------------------------------------------- 7. capture
def test_captured_tick_replays_eager_ticks_and_reads_live_weights():
    n, C = 7, 33
    cap, eager = prepared(c3(5), twins=1)
    critic = critic_of(216, 64, seed=4, device=DEV)
    nz = normalizer_of(216, 3, DEV)
    pc, pe = (sw.mppi(n, C, 0.3, lam=0.3, seed=8) for sw in (cap, eager))
    nom = random_sequence(pc, scale=0.9)
    for pl in (pc, pe):
        pl.reset(nom)
        pl.set_value(critic, gamma=0.99, scale=0.5, obs_normalizer=nz)
    want = []
    for _ in range(3):
        pe.plan()
        r = eager.step(pe.action)
        torch.cuda.synchronize()
        want.append((pe.action.clone(), r.obs.clone(), pe.ret.clone(), pe.value.clone()))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        pc.plan()
        r = cap.step(pc.action)
    for k in range(3):
        g.replay()
        torch.cuda.synchronize()
        same_bytes(pc.action, want[k][0], f"action, tick {k}")
        same_bytes(r.obs, want[k][1], f"obs, tick {k}")
        same_bytes(pc.ret, want[k][2], f"ret, tick {k}")
        same_bytes(pc.value, want[k][3], f"value, tick {k}")
    assert fingerprint(cap)[:4] == fingerprint(eager)[:4]
    # the weights are read where they live: an in-place update shows in the next replay
    with torch.no_grad():
        critic.v_net.fcs[2].bias.add_(1.0)
    g.replay()
    pe.plan()                                                            # (the eager planner reads them live too)
    torch.cuda.synchronize()
    same_bytes(pc.value, pe.value, "value, captured against eager, after the update")
    rows = pc.last_obs.view(C * 5, -1)
    assert_close(pc.value, forward32(rows, critic, nz), "value after the in-place update")
    with torch.no_grad():
        critic.v_net.fcs[2].bias.sub_(1.0)
    assert_close(pc.value, forward32(rows, critic, nz) + 1.0, "value against the old critic's, moved by 1")
    cap.close()
    eager.close()


# --------------------------------------------------------------------------- 8. refusals
@pytest.mark.parametrize("kind", ["mppi", "cem"])
def test_refusals_leave_planner_and_swarm_alone(kind):
    bufs = MPPI_BUFS if kind == "mppi" else CEM_BUFS

    def make(sw, per_drone=False, C=33, n=7):
        return (sw.mppi(n, C, 0.3, seed=5, per_drone=per_drone) if kind == "mppi"
                else sw.cem(n, C, 5, 0.3, iterations=2, seed=5, per_drone=per_drone))

    a, b = prepared(c3(5), twins=1, grounded=True)
    pa, pb = make(a), make(b)
    nom = random_sequence(pa, scale=0.9)
    pa.reset(nom)
    pb.reset(nom)
    held, before = planner_bytes(pa, bufs), fingerprint(a)
    I = 216
    critic, nz = critic_of(I, 64, seed=4, device=DEV), normalizer_of(I, 3, DEV)
    msg = f"rc=-1.*qs_value_{kind}_set"
    # a per-drone planner
    pd = make(a, per_drone=True)
    with pytest.raises(L.QuadSwarmError, match=msg + ".*one value per env"):
        pd.set_value(critic)
    assert pd.value is None
    pd.close()
    # in_dim != D * O; hidden outside {64, 128, 256}
    with pytest.raises(L.QuadSwarmError, match=msg + ".*in_dim"):
        pa.set_value(critic_of(I + 1, 64, seed=4, device=DEV))
    for N in (32, 96, 512):
        with pytest.raises(L.QuadSwarmError, match=msg + ".*hidden"):
            pa.set_value(critic_of(I, N, seed=4, device=DEV))
    # a net that is partly NULL; one of obs_mean / obs_var without the other
    for name in ("w1", "b1", "w2", "b2", "w3", "b3"):
        spec, keep = value_spec(critic, 0.99, 1.0, nz)
        setattr(spec, name, None)
        rc, text = raw_set(pa, spec)
        assert rc == -1 and "all NULL" in text, (name, rc, text)
    for name in ("obs_mean", "obs_var"):
        spec, keep = value_spec(critic, 0.99, 1.0, nz)
        setattr(spec, name, None)
        rc, text = raw_set(pa, spec)
        assert rc == -1 and "obs_mean and obs_var" in text, (name, rc, text)
    # gamma outside (0, 1]; a scale that is not finite
    for gamma in (0.0, -0.5, 1.5, float("nan"), float("inf")):
        with pytest.raises(L.QuadSwarmError, match=msg + ".*gamma"):
            pa.set_value(critic, gamma=gamma)
    for scale in (float("inf"), float("-inf"), float("nan")):
        with pytest.raises(L.QuadSwarmError, match=msg + ".*scale"):
            pa.set_value(critic, scale=scale)
    # what the Python layer turns down before the library sees it
    with pytest.raises(ValueError):
        pa.set_value(critic_of(I, 64, seed=4, device="cpu"))
    with pytest.raises(ValueError):
        pa.set_value(tuple(t.double() for t in weights_of(critic)))
    with pytest.raises(ValueError):
        pa.set_value(tuple(weights_of(critic))[:5])
    assert pa.last_obs is None and pa.value is None and pa.rewards is None
    assert planner_bytes(pa, bufs) == held and fingerprint(a) == before
    # a refusal with a value attached keeps that value
    pa.set_value(critic, gamma=0.99)
    keep_ptr = pa.value.data_ptr()
    with pytest.raises(L.QuadSwarmError, match=msg):
        pa.set_value(critic, gamma=2.0)
    assert pa.value.data_ptr() == keep_ptr
    pa.clear_value()
    # last_obs past the 32-bit offsets: 500 000 candidates x 5 envs x 216 floats
    big = make(a, C=500000, n=1)
    with pytest.raises(L.QuadSwarmError, match=msg + ".*32-bit"):
        big.set_value(critic)
    big.set_value(None, gamma=0.5)          # (no net: no last_obs)
    big.close()
    # in_dim = D * O, but above 1024: 40 drones x 27
    wide = QuadSwarm(task="multihover", num_drones=40, num_envs=1, act="one_d_pid", initial_xyzs=grid_layout(40))
    pw = make(wide)
    with pytest.raises(L.QuadSwarmError, match=msg + ".*in_dim"):
        pw.set_value(critic_of(40 * 27, 64, seed=4, device=DEV))
    wide.close()
    # and the planner still plans what a fresh one plans
    assert planner_bytes(pa, bufs) == held and fingerprint(a) == before
    pa.plan()
    pb.plan()
    assert planner_bytes(pa, bufs) == planner_bytes(pb, bufs)
    # qs_value_tail's own argument checks
    x, ret = torch.zeros((2, 1, 8, 27), device=DEV), torch.zeros((2, 1), dtype=torch.float64, device=DEV)
    fd, value = torch.zeros((2, 1), dtype=torch.int32, device=DEV), torch.zeros((2, 1), device=DEV)
    spec, keep = value_spec(critic, 0.99, 1.0)
    assert tail(spec, 4, 2, 1, 8, 27, x, None, ret, fd, value) == -1            # gamma != 1 without rewards
    assert tail(spec, 33, 2, 1, 8, 27, x, None, ret, fd, value) == -1           # n > 32
    assert tail(spec, 4, 2, 1, 8, 26, x, None, ret, fd, value) == -1            # in_dim != D * O
    spec, keep = value_spec(critic, 1.0, 1.0)
    assert tail(spec, 4, 2, 1, 8, 27, None, None, ret, fd, value) == -1         # a net without last_obs
    assert tail(spec, 4, 2, 1, 8, 27, x, None, ret, fd, value) == 0
    a.close()
    b.close()


# ------------------------------------------------------------------------ 9. clear_value
@pytest.mark.parametrize("kind", ["mppi", "cem"])
def test_clear_value_returns_the_plain_tick(kind):
    bufs = MPPI_BUFS if kind == "mppi" else CEM_BUFS
    a, b = prepared(c3(5), twins=1, grounded=True)
    pa, pb = ((sw.mppi(7, 33, 0.3, lam=0.5, seed=6) if kind == "mppi" else sw.cem(7, 33, 5, 0.3, iterations=2, seed=6))
              for sw in (a, b))
    nom = random_sequence(pa, scale=0.9)
    pa.reset(nom)
    pb.reset(nom)
    pa.set_value(critic_of(216, 128, seed=4, device=DEV), gamma=0.9, scale=2.0, obs_normalizer=normalizer_of(216, 3, DEV))
    if kind == "mppi":
        pa.sample()
    else:
        pa.begin()
        pa.sample(0)
    pa.score()
    torch.cuda.synchronize()
    assert pa.value.abs().max() > 0
    pa.clear_value()
    assert pa.last_obs is None and pa.value is None and pa.rewards is None
    for k in range(3):
        pa.plan()
        pb.plan()
        assert planner_bytes(pa, bufs) == planner_bytes(pb, bufs), f"tick {k}"
        a.step(pa.action)
        b.step(pb.action)
    assert fingerprint(a) == fingerprint(b)
    a.close()
    b.close()
