"""The policy prior of the MPPI and CEM ticks (qs_prior_act, qs_prior_mppi_* / qs_prior_cem_*;
`MPPIPlanner.set_prior`, `.prior`, `.clear_prior`): closed-loop actor rollouts as candidates.

  1. qs_prior_act alone on synthetic obs: the noise-free actions against torch's float32 forward
     times action_scale (rtol = atol = 1e-5, with and without the float64 normaliser), every
     hidden size, input widths that are no multiple of the MFMA's k or of the K-chunk, 1 to 4
     outputs, row counts that are no multiple of the row tile, both row tiles, the broadcast
     read and the copy of the obs;
  2. the noise: trajectory 0 has none, the others' is standard normal, keyed on tick and global
     env id, and clipped;
  3. the prior stage's closed loop is the open loop's bytes: its candidates, scored by
     QuadSwarm.score, see the obs the actor saw, and each step's actions are the actor's on them;
  4. a prior that knows the best constant action wins the tick, per env and per drone;
  5. the MPPI and CEM ticks stage by stage;
  6. plan() with a prior leaves the swarm alone;
  7. a captured tick replays the eager ticks and reads the actor's weights live;
  8. refusals leave planner and swarm as they were;
  9. clear_prior() returns the planner to the plain tick."""
import numpy as np
import pytest
import torch

from gym_pybullet_drones_amd import _lib as L
from gym_pybullet_drones_amd.envs.swarm import grid_layout, prior_spec
from gym_pybullet_drones_amd.vec_env.vec_env import SwarmVecEnv
from planner_case import c3, fingerprint, ks_normal, planner_bytes, prepared, random_sequence, same_bytes
from prior_case import WIDE, act, actor_of, constant_actor, forward32, normalizer_of, raw_set, weights_of
from value_case import CEM_BUFS, MPPI_BUFS, assert_close, critic_of

pytestmark = pytest.mark.gpu
DEV = "cuda"


def synthetic(K, E, D, O, seed):
    """Rows of N(0, 2) obs; column 3 holds values far past the normaliser's clip."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn((K, E, D, O), generator=gen) * 2.0
    x[..., 3] *= 100.0
    return x.to(DEV)


def zero_tick():
    return torch.zeros(1, dtype=torch.int64, device=DEV)


# ------------------------------------------------------------------ 1. the launch alone
def check_act(N, O, A, K, E, D):
    x = synthetic(K, E, D, O, seed=K * E * D + O)
    x0 = x[0].contiguous()                                  # the caller's (E, D, O) obs of the broadcast read
    tick = zero_tick()
    for scale in (1.0, 0.5):
        actor = actor_of(O, A, N, seed=N + O + A, device=DEV, action_scale=scale)
        for nz in (None, normalizer_of(D, O, seed=O, device=DEV, zero_var_col=min(5, O - 1))):
            what = f"N = {N}, O = {O}, A = {A}, R = {K * E * D}, action_scale {scale}, normaliser {nz is not None}"
            spec, keep = prior_spec(actor, K, x0, nz, std_scale=0.0)            # no noise: every row is its mean
            rc, got, seen = act(spec, 0, K, E, D, x, False, tick)
            assert rc == 0, L.load().qs_last_error()
            want = forward32(x, actor, nz)
            assert_close(got, want, "actions, " + what)
            assert_close(got[0], want[0], "trajectory 0")
            assert_close(got.view(-1, A)[-1:], want.view(-1, A)[-1:], "the last row of the last tile")
            same_bytes(seen, x, "obs_seen")
            if nz is not None:                              # the extremes reach the net as the clip, not as an inf or a NaN
                y = (x.double() - nz.rms.mean) / torch.sqrt(nz.rms.var + nz.epsilon)
                assert (y[..., 3].abs() > nz.clip).any() and (y[..., min(5, O - 1)].abs() > nz.clip).any()
            # the broadcast read of (E, D, O) equals the plain read of its expansion, byte for byte
            wide = x0.expand(K, E, D, O).contiguous()
            spec1, keep1 = prior_spec(actor, K, x0, nz, std_scale=1.0)
            rc, plain, seen_plain = act(spec1, 2, K, E, D, wide, False, tick, seed=5)
            rc2, bc, seen_bc = act(spec1, 2, K, E, D, x0, True, tick, seed=5)
            assert rc == 0 and rc2 == 0
            same_bytes(bc, plain, "broadcast against expanded, " + what)
            same_bytes(seen_bc, wide, "obs_seen of the broadcast read")
            same_bytes(seen_plain, wide, "obs_seen of the plain read")
            assert_close(bc[0], forward32(x0, actor, nz), "trajectory 0 of the broadcast read")


@pytest.mark.parametrize("K,E,D", [(1, 1, 1), (3, 5, 2), (2, 1, 8), (257, 1, 1)])
@pytest.mark.parametrize("O,A", [(13, 1), (27, 1), (27, 4), (38, 3)])
@pytest.mark.parametrize("N", [64, 128, 256])
def test_actions_match_the_float32_forward(N, O, A, K, E, D):
    check_act(N, O, A, K, E, D)


# 8 232 rows are more than 16 rows x 256 compute units: N = 64 and 128 take the 32-row tile (value_sizes.h), with
# a partial last tile, at the narrowest input with one output and at a wider one with four
@pytest.mark.parametrize("O,A", [(13, 1), (27, 4)])
@pytest.mark.parametrize("N", [64, 128])
def test_actions_on_the_wide_row_tile(N, O, A):
    check_act(N, O, A, 3, 343, 8)


# ---------------------------------------------------------------------------- 2. noise
@pytest.mark.parametrize("O,A,K", [(27, 1, 9), (38, 3, 5), (27, 4, 3)])
def test_the_noise_is_the_policys(O, A, K):
    E, D, j = 1024, 8, 3
    actor = actor_of(O, A, 64, seed=7, device=DEV, action_scale=0.5)
    x = synthetic(K, E, D, O, seed=21)
    x0 = x[0].contiguous()
    tick = zero_tick()
    std = torch.exp(actor.logstd.detach())
    quiet, _ = prior_spec(actor, K, x0, std_scale=0.0)
    for std_scale in (1.0, 0.25):
        spec, keep = prior_spec(actor, K, x0, std_scale=std_scale)
        rc0, a0, _ = act(quiet, j, K, E, D, x, False, tick, seed=9, genv0=100)
        rc1, a1, _ = act(spec, j, K, E, D, x, False, tick, seed=9, genv0=100)
        assert rc0 == 0 and rc1 == 0
        same_bytes(a1[0], a0[0], "trajectory 0 is the mode")                 # std_scale 0 and std_scale > 0
        z = (a1[1:] - a0[1:]) / (std_scale * std)
        assert z.numel() >= 1 << 16 and torch.isfinite(z).all()
        assert (a1.abs() < WIDE).all()                                       # no element was clipped, none is left out
        ks_normal(z.cpu().numpy())
        for a in range(A):                                                   # and each component on its own scale
            assert abs(float(z[..., a].std()) - 1.0) < 0.02, a
    # the same tick gives the same bytes, the next tick and another step different ones
    rc, again, _ = act(spec, j, K, E, D, x, False, tick, seed=9, genv0=100)
    same_bytes(again, a1, "the same tick")
    tick += 1
    rc, later, _ = act(spec, j, K, E, D, x, False, tick, seed=9, genv0=100)
    same_bytes(later[0], a1[0], "trajectory 0, the next tick")
    assert not torch.equal(later[1:], a1[1:]) and (later[1:] != a1[1:]).float().mean() > 0.99
    rc, other, _ = act(spec, j + 1, K, E, D, x, False, tick, seed=9, genv0=100)
    assert (other[1:] != later[1:]).float().mean() > 0.99
    # two shards with env_offset reproduce the unsharded rows
    cut = 400
    rc, lo_part, _ = act(spec, j, K, cut, D, x[:, :cut].contiguous(), False, tick, seed=9, genv0=100)
    rc2, hi_part, _ = act(spec, j, K, E - cut, D, x[:, cut:].contiguous(), False, tick, seed=9, genv0=100 + cut)
    assert rc == 0 and rc2 == 0
    same_bytes(lo_part, later[:, :cut], "shard 0")
    same_bytes(hi_part, later[:, cut:], "shard 1")
    # with tight bounds every element lies in [lo, hi], and the bounds are reached
    rc, tight, _ = act(spec, j, K, E, D, x, False, tick, lo=-0.05, hi=0.1, seed=9, genv0=100)
    assert rc == 0 and torch.isfinite(tight).all()
    assert float(tight.min()) == float(np.float32(-0.05)) and float(tight.max()) == float(np.float32(0.1))


# ------------------------------------------------ 3. the closed loop is the open loop's bytes
def mh2(**kw):
    return dict(task="multihover", num_drones=2, num_envs=5, act="one_d_pid", initial_xyzs=grid_layout(2), env_offset=37, **kw)


def spiral(**kw):
    return dict(task="spiral", num_drones=5, num_envs=64, act="vel", **kw)


CLOSED = {"mh-fp32": mh2(), "mh-fp64": mh2(precision=8), "spiral-fp32": spiral(), "spiral-fp64": spiral(precision=8)}


@pytest.mark.parametrize("cfg", list(CLOSED))
def test_closed_loop_is_the_open_loops_bytes(cfg):
    n, K, C = 7, 3, 8
    (sw,) = prepared(CLOSED[cfg])
    E, D, O, A = sw.num_envs, sw.num_drones, sw.obs_dim, sw.act_dim
    obs = sw.obs                                             # what reset and every step wrote: the current state's obs
    actor = actor_of(O, A, 64, seed=3, device=DEV, action_scale=0.5)
    nz = normalizer_of(D, O, seed=4, device=DEV)
    pl = sw.mppi(n, C, 0.3, seed=5)
    pl.reset(random_sequence(pl, scale=0.9))
    pl.set_prior(actor, K, obs, nz, std_scale=0.7)
    assert tuple(pl.prior_actions.shape) == (n, K, E, D, A) and tuple(pl.prior_obs.shape) == (n, K, E, D, O)
    before = fingerprint(sw)
    pl.prior()
    pl.sample()
    torch.cuda.synchronize()
    same_bytes(pl.candidates[:, C - K:], pl.prior_actions, "the last K candidates are the prior's")
    same_bytes(pl.candidates[:, 0], pl.nominal, "candidate 0 is the nominal")
    assert (pl.prior_actions[:, 1:] != pl.prior_actions[:, :1]).float().mean() > 0.9       # the noise is there
    # the open loop: QuadSwarm.score of the candidates, with every step's obs
    seen = torch.empty((n, C, E, D, O), device=DEV)
    sw.score(pl.candidates, [dict(obs=seen[j]) for j in range(n)])
    torch.cuda.synchronize()
    same_bytes(pl.prior_obs[0], obs.expand(K, E, D, O), "slot 0 is the caller's obs")
    for j in range(n - 1):
        same_bytes(pl.prior_obs[j + 1], seen[j, C - K:], f"the obs after step {j}")
    # every step's actions are the actor's on the obs of that slot
    spec, keep = prior_spec(actor, K, obs, nz, std_scale=0.7)
    for j in range(n):
        rc, alone, _ = act(spec, j, K, E, D, pl.prior_obs[j], False, pl.tick, lo=-1.0, hi=1.0, seed=5,
                           genv0=sw.env_offset, seen=False)
        assert rc == 0, L.load().qs_last_error()
        same_bytes(alone, pl.prior_actions[j], f"qs_prior_act alone, step {j}")
        assert_close(alone[0], forward32(pl.prior_obs[j][0], actor, nz).clamp(-1.0, 1.0), f"trajectory 0, step {j}")
    assert fingerprint(sw) == before
    sw.close()


# ------------------------------------------------------------- 4. the prior wins when it should
@pytest.mark.parametrize("per_drone", [False, True], ids=["env", "per-drone"])
@pytest.mark.parametrize("kind", ["mppi", "cem"])
def test_a_prior_that_knows_the_best_constant_wins(kind, per_drone):
    n, C, K = 7, 8, 3
    env = SwarmVecEnv(seed=3, **c3(5))                          # (its planners are the swarm's, with step_t bound)
    env.reset_t()
    for _ in range(2):
        env.step_t(None)
    sw = env.swarm
    E, D, A = sw.num_envs, sw.num_drones, sw.act_dim
    scan = torch.linspace(-1.0, 1.0, 9, device=DEV)
    G = scan.numel()
    acts = scan.view(1, G, 1, 1, 1).expand(n, G, E, D, A).contiguous()
    ret, _, ret_agent = env.score_t(acts, per_drone=True)
    torch.cuda.synchronize()
    score = ret_agent if per_drone else ret
    g = int(ret.sum(1).argmax())
    u = float(scan[g])
    worst = score.argmin(0)                                     # per env, or per (env, drone)
    print(f"best constant {u}, returns {ret.sum(1).cpu().numpy()}, worst per unit {worst.flatten().cpu().numpy()}")
    assert (score[g] > score.gather(0, worst[None])[0]).all(), "the scenario: u* beats every unit's worst constant"
    nominal = scan[worst].view(1, E, D if per_drone else 1, 1).expand(n, E, D, A).contiguous()
    pl = (env.mppi(n, C, 0.0, lam=0.0, seed=2, per_drone=per_drone) if kind == "mppi"
          else env.cem(n, C, 1, 0.0, iterations=1, seed=2, per_drone=per_drone))
    pl.reset(nominal)
    pl.set_prior(constant_actor(sw.obs_dim, A, u, DEV), K, sw.obs, std_scale=0.0)
    action = pl.plan()
    torch.cuda.synchronize()
    same_bytes(pl.prior_actions, torch.full_like(pl.prior_actions, u), "the prior's actions are u* exactly")
    chosen = pl.best if kind == "mppi" else pl.elites[0]
    assert tuple(chosen.shape) == ((E, D) if per_drone else (E,))
    assert (chosen >= C - K).all(), chosen
    assert torch.equal(action, torch.full_like(action, u))
    env.close()


# ------------------------------------------------------------------------ 5. stage by stage
PRIOR_BUFS = ("prior_actions", "prior_obs")
VALUE_BUFS = ("last_obs", "value", "rewards")


def make(sw, kind, per_drone=False, C=33, n=7, seed=5):
    return (sw.mppi(n, C, 0.3, lam=0.5, done_penalty=1.5, seed=seed, per_drone=per_drone) if kind == "mppi"
            else sw.cem(n, C, 5, 0.3, iterations=2, done_penalty=1.5, seed=seed, per_drone=per_drone))


def staged_tick(pl, kind):
    if kind == "mppi":
        pl.prior()
        pl.sample()
        pl.score()
        pl.update()
        return
    pl.begin()
    pl.prior()
    for i in range(pl.iterations):
        pl.sample(i)
        pl.score()
        pl.refit(i)
    pl.finish()


@pytest.mark.parametrize("with_value", [False, True], ids=["plain", "value-tail"])
@pytest.mark.parametrize("kind", ["mppi", "cem"])
def test_the_stages_give_plans_bytes(kind, with_value):
    K = 4
    a, b = prepared(c3(5), twins=1, grounded=True)
    actor = actor_of(27, 1, 128, seed=6, device=DEV)
    nz = normalizer_of(8, 27, seed=4, device=DEV)
    pa, pb = make(a, kind), make(b, kind)
    nom = random_sequence(pa, scale=0.9)
    bufs = (MPPI_BUFS if kind == "mppi" else CEM_BUFS) + PRIOR_BUFS + (VALUE_BUFS if with_value else ())
    for sw, pl in ((a, pa), (b, pb)):
        pl.reset(nom)
        pl.set_prior(actor, K, sw.obs, nz, std_scale=0.5)
        if with_value:
            pl.set_value(critic_of(216, 64, seed=4, device=DEV), gamma=0.99, scale=0.5)
    for k in range(2):
        pa.plan()
        staged_tick(pb, kind)
        assert planner_bytes(pa, bufs) == planner_bytes(pb, bufs), f"tick {k}"
        same_bytes(pa.candidates[:, 33 - K:], pa.prior_actions, "the last K candidates")
        a.step(pa.action)                                       # (writes a.obs, which the next tick's prior reads)
        b.step(pb.action)
    assert int(pa.tick.item()) == 2 and fingerprint(a) == fingerprint(b)
    a.close()
    b.close()


# ------------------------------------------------------------------------ 6. no mutation
@pytest.mark.parametrize("per_drone", [False, True], ids=["env", "per-drone"])
@pytest.mark.parametrize("kind", ["mppi", "cem"])
def test_plan_with_a_prior_leaves_the_swarm_alone(kind, per_drone):
    (sw,) = prepared(c3(5), grounded=True)
    pl = make(sw, kind, per_drone)
    pl.set_prior(actor_of(27, 1, 64, seed=6, device=DEV), 4, sw.obs, normalizer_of(8, 27, 4, DEV))
    before = fingerprint(sw)
    pl.plan()
    pl.plan()
    assert fingerprint(sw) == before
    assert torch.isfinite(pl.prior_actions).all() and pl.prior_actions.abs().max() > 0
    sw.close()


# ---------------------------------------------------------------------------- 7. capture
def test_captured_tick_replays_eager_ticks_and_reads_live_weights():
    n, C, K = 7, 33, 4
    cap, eager = prepared(c3(5), twins=1)
    actor = actor_of(27, 1, 64, seed=6, device=DEV)
    nz = normalizer_of(8, 27, 4, DEV)
    pc, pe = (sw.mppi(n, C, 0.3, lam=0.3, seed=8) for sw in (cap, eager))
    nom = random_sequence(pc, scale=0.9)
    for sw, pl in ((cap, pc), (eager, pe)):
        pl.reset(nom)
        pl.set_prior(actor, K, sw.obs, nz, std_scale=0.5)
    want = []
    for _ in range(3):
        pe.plan()
        r = eager.step(pe.action, obs=eager.obs)
        torch.cuda.synchronize()
        want.append((pe.action.clone(), r.obs.clone(), pe.prior_actions.clone(), pe.prior_obs.clone(), pe.ret.clone()))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        pc.plan()
        r = cap.step(pc.action, obs=cap.obs)
    for k in range(3):
        g.replay()
        torch.cuda.synchronize()
        same_bytes(pc.action, want[k][0], f"action, tick {k}")
        same_bytes(r.obs, want[k][1], f"obs, tick {k}")
        same_bytes(pc.prior_actions, want[k][2], f"prior_actions, tick {k}")
        same_bytes(pc.prior_obs, want[k][3], f"prior_obs, tick {k}")
        same_bytes(pc.ret, want[k][4], f"ret, tick {k}")
    assert fingerprint(cap)[:4] == fingerprint(eager)[:4]
    # the weights are read where they live: an in-place update shows in the next replay
    with torch.no_grad():
        actor.pi_net.fcs[2].bias.add_(0.25)
    g.replay()
    pe.plan()                                                            # (the eager planner reads them live too)
    torch.cuda.synchronize()
    same_bytes(pc.prior_actions, pe.prior_actions, "prior_actions, captured against eager, after the update")
    mode = forward32(pc.prior_obs[0][0], actor, nz)
    assert_close(pc.prior_actions[0][0], mode.clamp(-1.0, 1.0), "trajectory 0 after the in-place update")
    with torch.no_grad():
        actor.pi_net.fcs[2].bias.sub_(0.25)
    old = forward32(pc.prior_obs[0][0], actor, nz)
    assert_close(pc.prior_actions[0][0], (old + 0.25).clamp(-1.0, 1.0), "against the old actor's, moved by 0.25")
    assert (old.abs() < 0.7).all()                                       # (the move was not lost in the clip)
    cap.close()
    eager.close()


# --------------------------------------------------------------------------- 8. refusals
@pytest.mark.parametrize("kind", ["mppi", "cem"])
def test_refusals_leave_planner_and_swarm_alone(kind):
    bufs = MPPI_BUFS if kind == "mppi" else CEM_BUFS
    a, b = prepared(c3(5), twins=1, grounded=True)
    pa, pb = make(a, kind), make(b, kind)
    nom = random_sequence(pa, scale=0.9)
    pa.reset(nom)
    pb.reset(nom)
    held, before = planner_bytes(pa, bufs), fingerprint(a)
    O, A, D, C = 27, 1, 8, 33
    actor, nz = actor_of(O, A, 64, seed=6, device=DEV), normalizer_of(D, O, 4, DEV)
    msg = f"rc=-1.*qs_prior_{kind}_set"
    # count outside 1 .. C - 1
    for K in (0, -1, C, C + 1):
        with pytest.raises(L.QuadSwarmError, match=msg + ".*count"):
            pa.set_prior(actor, K, a.obs)
    # hidden outside {64, 128, 256}; act_dim != the swarm's
    for N in (32, 96, 512):
        with pytest.raises(L.QuadSwarmError, match=msg + ".*hidden"):
            pa.set_prior(actor_of(O, A, N, seed=6, device=DEV), 4, a.obs)
    with pytest.raises(L.QuadSwarmError, match=msg + ".*act_dim"):
        pa.set_prior(actor_of(O, 2, 64, seed=6, device=DEV), 4, a.obs)
    # in_dim != obs_dim (the critic's width among them)
    for I in (O + 1, D * O):
        spec, keep = prior_spec(actor, 4, a.obs, nz)
        spec.in_dim = I
        rc, text = raw_set(pa, spec)
        assert rc == -1 and "in_dim" in text, (I, rc, text)
    # a net that is partly NULL; one of obs_mean / obs_var without the other; a NULL obs
    for name in ("w1", "b1", "w2", "b2", "w3", "b3", "logstd"):
        spec, keep = prior_spec(actor, 4, a.obs, nz)
        setattr(spec, name, None)
        rc, text = raw_set(pa, spec)
        assert rc == -1 and "must all be set" in text, (name, rc, text)
    for name in ("obs_mean", "obs_var"):
        spec, keep = prior_spec(actor, 4, a.obs, nz)
        setattr(spec, name, None)
        rc, text = raw_set(pa, spec)
        assert rc == -1 and "obs_mean and obs_var" in text, (name, rc, text)
    spec, keep = prior_spec(actor, 4, a.obs, nz)
    spec.obs = None
    rc, text = raw_set(pa, spec)
    assert rc == -1 and "obs is NULL" in text, (rc, text)
    # std_scale not finite or negative
    for s in (float("inf"), float("nan"), -1.0, -1e-30):
        with pytest.raises(L.QuadSwarmError, match=msg + ".*std_scale"):
            pa.set_prior(actor, 4, a.obs, std_scale=s)
    # what the Python layer turns down before the library sees it
    with pytest.raises(ValueError):
        pa.set_prior(actor_of(O, A, 64, seed=6, device="cpu"), 4, a.obs)
    with pytest.raises(ValueError):
        pa.set_prior(tuple(weights_of(actor)), 4, a.obs)                       # six tensors: no logstd
    with pytest.raises(ValueError):
        pa.set_prior(actor, 4, a.obs[:, :4].contiguous())                      # not the swarm's (E, D, O)
    with pytest.raises(ValueError):
        pa.set_prior(actor, 4, a.obs, normalizer_of(1, O, 4, DEV))             # a normaliser of one drone's obs
    assert pa.prior_actions is None and pa.prior_obs is None
    assert planner_bytes(pa, bufs) == held and fingerprint(a) == before
    # a refusal with a prior attached keeps that prior
    pa.set_prior(tuple(weights_of(actor)) + (actor.logstd.detach(),), 4, a.obs, action_scale=0.5)
    keep_ptr = pa.prior_actions.data_ptr()
    with pytest.raises(L.QuadSwarmError, match=msg):
        pa.set_prior(actor, C, a.obs)
    assert pa.prior_actions.data_ptr() == keep_ptr
    pa.clear_prior()
    assert pa.prior_actions is None and pa.prior_obs is None
    with pytest.raises(L.QuadSwarmError, match="no prior is attached"):
        pa.prior()
    # a step's obs past the 32-bit offsets: 499 999 trajectories x 5 envs x 8 drones x 27 floats
    big = make(a, kind, C=500000, n=1)
    with pytest.raises(L.QuadSwarmError, match=msg + ".*32-bit"):
        big.set_prior(actor, 499999, a.obs)
    big.close()
    # and the planner still plans what a fresh one plans
    assert planner_bytes(pa, bufs) == held and fingerprint(a) == before
    pa.plan()
    pb.plan()
    assert planner_bytes(pa, bufs) == planner_bytes(pb, bufs)
    # qs_prior_act's own argument checks
    x, tick = torch.zeros((2, 1, 8, 27), device=DEV), zero_tick()
    spec, keep = prior_spec(actor, 2, x[0].contiguous())
    assert act(spec, 32, 2, 1, 8, x, False, tick)[0] == -1                     # j outside 0 .. 31
    assert act(spec, 0, 2, 1, 257, x, False, tick)[0] == -1                    # D above 256
    assert act(spec, 0, 2, 1, 8, x, False, tick, lo=1.0, hi=1.0)[0] == -1      # lo not below hi
    assert act(spec, 0, 2, 1, 8, x, False, None)[0] == -1                      # no tick
    assert act(spec, 0, 2, 1, 8, x, False, tick)[0] == 0
    a.close()
    b.close()


# ------------------------------------------------------------------------ 9. clear_prior
@pytest.mark.parametrize("per_drone", [False, True], ids=["env", "per-drone"])
@pytest.mark.parametrize("kind", ["mppi", "cem"])
def test_clear_prior_returns_the_plain_tick(kind, per_drone):
    bufs = MPPI_BUFS if kind == "mppi" else CEM_BUFS
    a, b = prepared(c3(5), twins=1, grounded=True)
    pa, pb = make(a, kind, per_drone, seed=6), make(b, kind, per_drone, seed=6)
    nom = random_sequence(pa, scale=0.9)
    pa.reset(nom)
    pb.reset(nom)
    pa.set_prior(actor_of(27, 1, 128, seed=6, device=DEV), 4, a.obs, normalizer_of(8, 27, 4, DEV))
    pa.prior()
    if kind == "cem":
        pa.begin()
    pa.sample()
    torch.cuda.synchronize()
    assert pa.prior_actions.abs().max() > 0
    same_bytes(pa.candidates[:, -4:], pa.prior_actions, "the prior was injected")
    pa.clear_prior()
    assert pa.prior_actions is None and pa.prior_obs is None
    for k in range(3):
        pa.plan()
        pb.plan()
        assert planner_bytes(pa, bufs) == planner_bytes(pb, bufs), f"tick {k}"
        a.step(pa.action)
        b.step(pb.action)
    assert fingerprint(a) == fingerprint(b)
    a.close()
    b.close()
