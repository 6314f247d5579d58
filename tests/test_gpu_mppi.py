"""The native MPPI planner tick (qs_mppi_*, `QuadSwarm.mppi`, `SwarmVecEnv.mppi`).

 1. Sample: candidate 0 is the nominal, every candidate is clipped, the noise is N(0, 1)
    (one-sample KS at the 0.001 level, mean and variance within 4 standard errors), and a
    zero sigma leaves its component alone.
 2. Sharding: the noise is keyed on the global env id.
 3. Ticks draw new noise; a reset repeats the first draw.
 4. Update against a float64 numpy restatement that reads the planner's own candidates,
    ret and first_done: both reduction variants, A = 4, fp64 rewards, done penalties, ties.
 5. Greedy (lambda = 0) copies the best candidate bit for bit.
 6. The shift at n = 1 (hold only) and n = score_depth().
 7. plan() leaves the swarm as it was.
 8. plan() + step() captured into one graph replays what eager ticks compute.
 9. Refusals leave the swarm and the planner as they were.
10. `SwarmVecEnv.mppi(...).step_t()`.
"""
import numpy as np
import pytest
import torch

from gym_pybullet_drones_amd import _lib as L
from gym_pybullet_drones_amd.envs.swarm import MPPIPlanner, QuadSwarm
from gym_pybullet_drones_amd.vec_env.vec_env import SwarmVecEnv
from planner_case import A4, F64, c3, fingerprint, ks_normal, planner_bytes, prepared, same_bytes
from planner_case import random_sequence as random_nominal

pytestmark = pytest.mark.gpu

BUFS = ("nominal", "candidates", "ret", "first_done", "weights", "best", "action", "tick")


def restate(pl, lam, penalty):
    """The update in float64 numpy, from the planner's own candidates, ret and first_done."""
    torch.cuda.synchronize()
    cand = pl.candidates.cpu().numpy().astype(np.float64)      # (n, C, E, D, A)
    ret, fd = pl.ret.cpu().numpy(), pl.first_done.cpu().numpy()
    n, C = cand.shape[0], cand.shape[1]
    s = ret - np.where(fd < n, np.float64(penalty), 0.0)
    best = np.argmax(s, axis=0)                                   # the first, i.e. lowest, c of the maximum
    if lam > 0:
        x = np.exp((s - s.max(axis=0)) / lam)
        w = x / x.sum(axis=0)
    else:
        w = (np.arange(C)[:, None] == best[None, :]).astype(np.float64)
    new = np.einsum("ce,jceda->jeda", w, cand)
    return dict(best=best.astype(np.int32), weights=w, new=new, action=new[0],
                nominal=np.concatenate([new[1:], new[-1:]], axis=0))


def check_update(pl, lam, penalty, bound, tick):
    """The planner's buffers after an update against the restatement (made from the same buffers)."""
    want = restate(pl, lam, penalty)
    best, w = pl.best.cpu().numpy(), pl.weights.cpu().numpy()
    nominal, action = pl.nominal.cpu().numpy().astype(np.float64), pl.action.cpu().numpy().astype(np.float64)
    assert np.array_equal(best, want["best"])
    rel = np.abs(w - want["weights"]) / np.maximum(want["weights"], np.finfo(np.float64).tiny)
    print("weights: max relative difference", rel.max(), "sum - 1", np.abs(w.sum(axis=0) - 1).max())
    assert rel.max() <= 1e-12
    tol = 2.0 ** -23 * bound
    print("nominal: max abs difference", np.abs(nominal - want["nominal"]).max(), "allowed", tol)
    assert np.abs(nominal - want["nominal"]).max() <= tol and np.abs(action - want["action"]).max() <= tol
    # the shift: steps 1 .. n-1 moved up, the last one held; the action is the step that left
    n = nominal.shape[0]
    assert np.array_equal(nominal[-1], nominal[-2] if n > 1 else nominal[0])
    assert int(pl.tick.item()) == tick
    return want


# ------------------------------------------------------------------------ 1. sample
def test_sample_copies_the_nominal_and_clips():
    (sw,) = prepared(c3(5))
    pl = sw.mppi(7, 33, 0.8, lo=-1.0, hi=1.0, seed=5)
    nom = random_nominal(pl)
    pl.reset(nom)
    pl.sample()
    torch.cuda.synchronize()
    same_bytes(pl.nominal, nom, "reset copies the nominal")
    same_bytes(pl.candidates[:, 0], nom, "candidate 0")
    c = pl.candidates.cpu().numpy()
    assert c.min() >= -1.0 and c.max() <= 1.0 and (c == 1.0).any() and (c == -1.0).any()
    assert not np.array_equal(c[:, 1], c[:, 2]) and not np.array_equal(c[:, 1, 0], c[:, 1, 1])
    assert int(pl.tick.item()) == 0          # sampling alone does not tick
    assert isinstance(pl, MPPIPlanner)
    sw.close()


def test_noise_is_standard_normal_a1():
    sw = QuadSwarm(**c3(1))
    pl = sw.mppi(16, 513, 0.5, lo=-100.0, hi=100.0, seed=1)
    pl.sample()
    ks_normal(pl.candidates[:, 1:].cpu().numpy() / 0.5)      # 16 * 512 * 8 = 2^16 draws
    sw.close()


def test_noise_is_standard_normal_in_every_component_a4():
    sw = QuadSwarm(**A4)
    sigma = (0.5, 1.0, 2.0, 0.0)
    pl = sw.mppi(16, 400, sigma, lo=-100.0, hi=100.0, seed=2)
    pl.sample()
    c = pl.candidates[:, 1:].cpu().numpy()                    # 16 * 399 * 5 * 3 = 95 760 draws a component
    for a in range(3):
        ks_normal(c[..., a] / sigma[a])
    z = np.stack([c[..., a].ravel() / sigma[a] for a in range(3)])
    assert np.abs(np.corrcoef(z) - np.eye(3)).max() < 4 / np.sqrt(z.shape[1])   # z0..z2: uncorrelated
    assert not c[..., 3].any()                                # sigma = 0 on a zero nominal
    nom = random_nominal(pl)
    pl.reset(nom)
    pl.sample()
    torch.cuda.synchronize()
    assert torch.equal(pl.candidates[..., 3], nom[:, None, ..., 3].expand(-1, 400, -1, -1))
    assert not torch.equal(pl.candidates[:, 1, ..., 0], nom[..., 0])
    sw.close()


# ---------------------------------------------------------------------- 2. sharding
def test_noise_is_keyed_on_the_global_env():
    whole, part = QuadSwarm(**c3(4)), QuadSwarm(**c3(2, env_offset=2))
    pw, pp = whole.mppi(5, 9, 0.3, seed=7), part.mppi(5, 9, 0.3, seed=7)
    nom = random_nominal(pw)
    pw.reset(nom)
    pp.reset(nom[:, 2:4].contiguous())
    for tick in range(2):
        pw.sample()
        pp.sample()
        torch.cuda.synchronize()
        same_bytes(pw.candidates[:, :, 2:4], pp.candidates, f"global envs 2 and 3, tick {tick}")
        assert not torch.equal(pw.candidates[:, 1:, 0:2], pw.candidates[:, 1:, 2:4])
        for p in (pw, pp):      # the same tick and nominal on both: tick on, nominal back
            p.update()
            p.nominal.copy_(nom if p is pw else nom[:, 2:4])
    whole.close()
    part.close()


# ------------------------------------------------------------------------- 3. ticks
def test_ticks_differ_and_a_reset_repeats():
    (sw,) = prepared(c3(5))
    pl = sw.mppi(6, 12, 0.4, seed=9)
    nom = random_nominal(pl)
    pl.reset(nom)
    pl.sample()
    first = pl.candidates.clone()
    pl.update()                      # ret all zero: uniform weights; tick 0 -> 1
    pl.nominal.copy_(nom)            # the same nominal again, the tick is what differs
    pl.sample()
    second = pl.candidates.clone()
    torch.cuda.synchronize()
    assert int(pl.tick.item()) == 1
    same_bytes(first[:, 0], second[:, 0], "candidate 0 is the nominal at every tick")
    assert not torch.equal(first[:, 1:], second[:, 1:])
    assert (first[:, 1:] != second[:, 1:]).float().mean() > 0.9
    pl.reset(nom)
    pl.sample()
    torch.cuda.synchronize()
    assert int(pl.tick.item()) == 0
    same_bytes(pl.candidates, first, "after reset the first sample repeats")
    sw.close()


# ------------------------------------------------------------------------ 4. update
@pytest.mark.parametrize("cfg,n,C,lam", [
    (c3(21), 7, 3, 1.0),          # one thread per env / per (step, env, drone, component)
    (c3(21), 7, 3, 0.02),
    (c3(1), 7, 300, 1.0),         # a workgroup per env / per (env, step); C is no multiple of 64
    (c3(1), 7, 300, 0.02),
    (c3(5), 3, 70, 0.3),          # the same at E > 1: rows of one env are E rows apart
    (A4, 5, 4, 0.5),              # A = 4, a row of 12
    (A4, 5, 130, 0.5),            # ... in the workgroup variant: 12 of 16 lanes a group
    (F64, 7, 3, 0.5),             # ret from double rewards
    (c3(1), 1, 300, 0.3),         # n = 1: the hold is the whole shift
    (c3(21), 32, 3, 0.3),         # n = score_depth()
    (c3(1), 32, 70, 0.3),
], ids=lambda v: None if isinstance(v, dict) else str(v))
def test_update_matches_the_float64_restatement(cfg, n, C, lam):
    (sw,) = prepared(cfg)
    assert n <= sw.score_depth() == 32
    pl = sw.mppi(n, C, 0.3, lo=-1.0, hi=1.0, lam=lam, seed=4)
    pl.reset(random_nominal(pl, scale=0.9))
    pl.plan()
    want = check_update(pl, lam, 0.0, 1.0, tick=1)
    assert lam < 0.1 or (want["weights"] > 0).all()
    pl.plan()                                                   # a second tick, from the shifted nominal
    check_update(pl, lam, 0.0, 1.0, tick=2)
    sw.close()


@pytest.mark.parametrize("E,C", [(21, 3), (5, 70)])
def test_done_penalty(E, C):
    n, lam, pen = 7, 0.5, 2.5
    (sw,) = prepared(c3(E), grounded=True)
    pl = sw.mppi(n, C, 0.3, lam=lam, done_penalty=pen, seed=4)
    pl.reset(random_nominal(pl, scale=0.9))
    pl.plan()
    fd = pl.first_done.cpu().numpy()
    assert (fd[:, 4] == 0).all()                                # the grounded env is done at once, in every candidate
    check_update(pl, lam, pen, 1.0, tick=1)
    # some candidates of an env done and others not (by hand: update reads the buffers as they are)
    pl.first_done[0::2, 1] = 3
    pl.first_done[1, 2] = 0
    pl.update()
    want = check_update(pl, lam, pen, 1.0, tick=2)
    free = restate(pl, lam, 0.0)
    assert not np.allclose(want["weights"][:, 1], free["weights"][:, 1])
    sw.close()


@pytest.mark.parametrize("E,C,tied", [(21, 3, (1, 2)), (1, 300, (70, 200)), (1, 300, (5, 261)), (1, 300, (64, 65))])
@pytest.mark.parametrize("lam", [0.0, 0.7])
def test_ties_go_to_the_lower_candidate(E, C, tied, lam):
    sw = QuadSwarm(**c3(E))
    pl = sw.mppi(4, C, 0.3, lam=lam, seed=4)
    pl.reset(random_nominal(pl))
    pl.sample()
    ret = -1.0 - torch.arange(C, dtype=torch.float64, device=sw.device)[:, None].expand(C, E).clone() / C
    ret[tied[0]] = ret[tied[1]] = 0.25
    pl.ret.copy_(ret)
    pl.first_done.fill_(4)
    pl.update()
    torch.cuda.synchronize()
    assert (pl.best.cpu().numpy() == tied[0]).all()
    want = check_update(pl, lam, 0.0, 1.0, tick=1)
    if lam > 0:
        assert np.array_equal(want["weights"][tied[0]], want["weights"][tied[1]])
        same_bytes(pl.weights[tied[0]], pl.weights[tied[1]], "equal scores, equal weights")
    sw.close()


# ------------------------------------------------------------------------ 5. greedy
@pytest.mark.parametrize("cfg,n,C", [(c3(21), 7, 3), (c3(1), 7, 300), (A4, 5, 130), (c3(5), 1, 3)],
                         ids=lambda v: None if isinstance(v, dict) else str(v))
def test_greedy_copies_the_best_candidate(cfg, n, C):
    (sw,) = prepared(cfg)
    pl = sw.mppi(n, C, 0.3, lam=0.0, seed=4)
    pl.reset(random_nominal(pl, scale=0.9))
    pl.plan()
    torch.cuda.synchronize()
    want = restate(pl, 0.0, 0.0)
    best = pl.best.cpu().numpy()
    assert np.array_equal(best, want["best"]) and (n == 1 or (best > 0).any())
    w = pl.weights.cpu().numpy()
    assert np.array_equal(w, want["weights"]) and set(np.unique(w)) == {0.0, 1.0}
    cand = pl.candidates.cpu().numpy()
    pick = np.stack([cand[:, best[e], e] for e in range(sw.num_envs)], axis=1)     # (n, E, D, A)
    same_bytes(pl.action, pick[0], "action = candidates[0][best]")
    same_bytes(pl.nominal[-1], pick[-1], "held last step")
    if n > 1:
        same_bytes(pl.nominal[:-1], pick[1:], "nominal[j] = candidates[j + 1][best]")
    sw.close()


# ------------------------------------------------------------------- 7. no mutation
@pytest.mark.parametrize("cfg,C", [(c3(21), 3), (c3(1), 300)], ids=lambda v: None if isinstance(v, dict) else str(v))
def test_plan_leaves_the_swarm_alone(cfg, C):
    (sw,) = prepared(cfg, grounded=cfg["num_envs"] > 4)
    pl = sw.mppi(7, C, 0.3, seed=4)
    before = fingerprint(sw)
    pl.plan()
    pl.plan()
    assert fingerprint(sw) == before
    assert int(pl.tick.item()) == 2
    sw.close()


# ------------------------------------------------------- 8. determinism and capture
@pytest.mark.parametrize("cfg,C", [(c3(5), 3), (c3(1), 300)], ids=lambda v: None if isinstance(v, dict) else str(v))
def test_captured_tick_replays_what_eager_ticks_compute(cfg, C):
    cap, eager = prepared(cfg, twins=1)
    pc, pe = (sw.mppi(7, C, 0.3, lam=0.3, seed=8) for sw in (cap, eager))
    nom = random_nominal(pc, scale=0.9)
    pc.reset(nom)
    pe.reset(nom)
    want = []
    for _ in range(3):
        pe.plan()
        r = eager.step(pe.action)
        torch.cuda.synchronize()
        want.append((pe.action.clone(), r.obs.clone(), r.reward.clone(), pe.candidates.clone()))
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
        same_bytes(pc.action, want[k][0], f"action, tick {k}")
        same_bytes(r.obs, want[k][1], f"obs, tick {k}")
        same_bytes(r.reward, want[k][2], f"reward, tick {k}")
    assert fingerprint(cap)[:4] == fingerprint(eager)[:4]     # (launch counts aside: a capture counts its node once)
    cap.close()
    eager.close()


# --------------------------------------------------------------------- 9. refusals
def test_refusals_leave_swarm_and_planner_alone():
    sw = QuadSwarm(**c3(21))
    depth = sw.score_depth()
    pl = sw.mppi(depth, 3, 0.3, seed=4)               # creating a planner needs no reset
    pl.reset(random_nominal(pl))
    held = planner_bytes(pl, BUFS)
    with pytest.raises(L.QuadSwarmError, match="rc=-4.*qs_reset"):   # QS_E_STATE: plan before qs_reset
        pl.plan()
    assert planner_bytes(pl, BUFS) == held
    sw.reset(3)
    sw.step(None)
    before = fingerprint(sw)
    ok = dict(horizon=4, candidates=3, sigma=0.3)
    for bad in (dict(horizon=0), dict(horizon=depth + 1), dict(candidates=1), dict(candidates=0), dict(lo=1.0, hi=1.0),
                dict(lo=0.5, hi=-0.5), dict(sigma=-0.1), dict(lam=-1.0), dict(done_penalty=-0.5),
                dict(sigma=float("nan")), dict(lam=float("inf")),
                dict(candidates=(1 << 27) + 1),                   # the counter word / 32-bit offsets
                dict(candidates=1 << 25)):                         # C * E * D = 2^25 * 168 > 2^31
        with pytest.raises(L.QuadSwarmError, match="rc=-1.*qs_mppi_create"):
            sw.mppi(**{**ok, **bad})
    with pytest.raises(ValueError):
        sw.mppi(4, 3, (0.1, 0.2))                                 # one sigma per component, A = 1
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
        sw.mppi(4, 3, 0.3)
    assert fingerprint(sw) == before
    sw.close()


# --------------------------------------------------------------------- 10. vec env
def test_vec_env_planner_step_t():
    a, b = SwarmVecEnv(seed=3, **c3(5)), SwarmVecEnv(seed=3, **c3(5))
    pa, pb = a.mppi(6, 9, 0.3, lam=0.4, seed=2), b.mppi(6, 9, 0.3, lam=0.4, seed=2)
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
