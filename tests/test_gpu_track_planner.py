"""Planner ticks on a tracking objective: `set_tracking` on `MPPIPlanner` / `CEMPlanner`
(qs_track_mppi_* / qs_track_cem_*) makes the score stage qs_track_score and the fold, and
update, select and refit consume the folded objective unchanged.

Setup: MultiHover one_d_pid, D = 4, E = 6, C = 16, n = 8.  Tests 1 to 4 run for MPPI and CEM,
env-level and per-drone.

 1. After sample() and track(), cost_agent and the folded ret / ret_agent equal, as bytes,
    the float64 restatement (tests/track_case.py) run over planner.candidates.
 2. q = r = 0 and reward_scale = 1: every buffer after plan() equals a twin planner's without
    tracking, as bytes.
 3. reward_scale = 0, MPPI lam = 0: best (CEM: the rank-0 elite) is the arg-min of the folded
    cost per unit from planner.cost_agent, the lower index on ties.
 4. After clear_tracking(), plan() equals the twin's plain tick as bytes; tracking next to a
    value tail is refused, in either order.
 5. step_t() (plan() and the control step) and base.add_(1), captured into one graph and
    replayed three times, equal the same three eager rounds as bytes; an in-place update of
    ref between replays is seen by the next replay.
 6. Direction only: with q on z alone and reward_scale = 0, 40 closed-loop ticks towards a
    reference height of 0.9 end higher than towards 0.3.
"""
import numpy as np
import pytest
import torch

from gym_pybullet_drones_amd import _lib as L
from gym_pybullet_drones_amd.envs.swarm import QuadSwarm, grid_layout
from planner_case import fingerprint, prepared, random_sequence, raw, same_bytes
from track_case import Q, R, TERMINAL, cost_reference, fold_reference, make_reference

pytestmark = pytest.mark.gpu

CFG = dict(task="multihover", num_drones=4, num_envs=6, act="one_d_pid", initial_xyzs=grid_layout(4))
N, C, K = 8, 16, 4
KINDS = [("mppi", False), ("mppi", True), ("cem", False), ("cem", True)]
IDS = ["mppi", "mppi_pd", "cem", "cem_pd"]
BUFS = {"mppi": ("nominal", "candidates", "ret", "first_done", "weights", "best", "action", "tick"),
        "cem": ("mean", "std", "candidates", "ret", "first_done", "elites", "iter_best", "action", "tick")}


def planner(sw, kind, per_drone, lam=0.5, seed=8):
    if kind == "mppi":
        pl = sw.mppi(N, C, 0.3, lam=lam, seed=seed, per_drone=per_drone)
        pl.reset(random_sequence(pl, scale=0.9))
    else:
        pl = sw.cem(N, C, K, 0.3, iterations=2, seed=seed, per_drone=per_drone)
        pl.reset(random_sequence(pl, scale=0.9))
    return pl


def sample(pl, kind):
    if kind == "cem":
        pl.begin()
        pl.sample(0)
    else:
        pl.sample()


def buffers(pl, kind):
    torch.cuda.synchronize()
    names = BUFS[kind] + (("ret_agent",) if pl.per_drone else ())
    return {k: raw(getattr(pl, k)) for k in names}


def attach(pl, sw, zero=False, reward_scale=1.0):
    ref, base = make_reference(sw)
    q, r = ((0.0,) * 12, (0.0,) * 4) if zero else (Q, R)
    pl.set_tracking(ref, q, r, terminal=TERMINAL, reward_scale=reward_scale, base=base)
    return ref, base


# ------------------------------------------------------------------ 1. the stage on its own
@pytest.mark.parametrize("kind,per_drone", KINDS, ids=IDS)
def test_track_stage_equals_the_restatement(kind, per_drone):
    sw, = prepared(CFG, grounded=True)
    pl = planner(sw, kind, per_drone)
    scale = -0.75
    ref, base = attach(pl, sw, reward_scale=scale)
    assert pl.cost_agent.shape == (C, 6, 4) and pl.ret_agent.shape == (C, 6, 4)
    before = fingerprint(sw)
    sample(pl, kind)
    pl.track()
    torch.cuda.synchronize()
    assert fingerprint(sw) == before
    # the plain launch over the same candidates, with everything the restatement reads
    E, D, O, A = sw.num_envs, sw.num_drones, sw.obs_dim, sw.act_dim
    kw = dict(device=sw.device)
    outs = dict(obs=torch.zeros((N, C, E, D, O), **kw), terminal_obs=torch.zeros((N, C, E, D, O), **kw),
                terminated=torch.zeros((N, C, E), dtype=torch.uint8, **kw),
                truncated=torch.zeros((N, C, E), dtype=torch.uint8, **kw), actions_out=torch.zeros((N, C, E, D, A), **kw))
    ret = torch.zeros((C, E), dtype=torch.float64, **kw)
    fd = torch.zeros((C, E), dtype=torch.int32, **kw)
    ret_agent = torch.zeros((C, E, D), dtype=torch.float64, **kw)
    sw.score(pl.candidates, [{k: v[j] for k, v in outs.items()} for j in range(N)], ret=ret, first_done=fd,
             ret_agent=ret_agent)
    torch.cuda.synchronize()
    o = {k: v.cpu().numpy() for k, v in outs.items()}
    cost = cost_reference(o["obs"], o["terminal_obs"], o["terminated"], o["truncated"], o["actions_out"],
                          ref.cpu().numpy(), base.cpu().numpy(), Q, R, TERMINAL)
    want_ret, want_agent = fold_reference(np.float32(scale), ret.cpu().numpy(), ret_agent.cpu().numpy(), cost)   # (the spec's is a float32)
    assert (fd.cpu().numpy() < N).any() and (fd.cpu().numpy() == N).any() and (cost > 0).all()
    assert raw(pl.cost_agent) == raw(cost)
    assert raw(pl.ret) == raw(want_ret)
    assert raw(pl.ret_agent) == raw(want_agent)
    same_bytes(pl.first_done, fd, "first_done")
    sw.close()


# ------------------------------------------------------------------ 2. zero weights: the return exactly
@pytest.mark.parametrize("kind,per_drone", KINDS, ids=IDS)
def test_zero_weights_plan_like_a_planner_without_tracking(kind, per_drone):
    sw, twin = prepared(CFG, twins=1, grounded=True)
    pl, plain = planner(sw, kind, per_drone), planner(twin, kind, per_drone)
    attach(pl, sw, zero=True, reward_scale=1.0)
    for tick in range(2):
        pl.plan()
        plain.plan()
        assert buffers(pl, kind) == buffers(plain, kind), tick
    assert raw(pl.cost_agent) == raw(np.zeros((C, 6, 4)))
    assert fingerprint(sw) == fingerprint(twin)
    sw.close()
    twin.close()


# ------------------------------------------------------------------ 3. the cost alone decides
@pytest.mark.parametrize("kind,per_drone", KINDS, ids=IDS)
def test_cost_alone_picks_the_cheapest_candidate(kind, per_drone):
    sw, = prepared(CFG)
    pl = planner(sw, kind, per_drone, lam=0.0)
    attach(pl, sw, reward_scale=0.0)
    pl.plan()
    torch.cuda.synchronize()
    cost = pl.cost_agent.cpu().numpy()
    if per_drone:
        folded = cost                               # (C, E, D): a drone's own cost
    else:
        folded = np.zeros(cost.shape[:2])
        for d in range(cost.shape[2]):
            folded = folded + cost[..., d]
        folded = folded / np.float64(cost.shape[2])   # (C, E)
    want = np.argmin(folded, axis=0)                # the lower index on ties
    got = (pl.best if kind == "mppi" else pl.elites[0]).cpu().numpy()
    assert np.array_equal(got, want)
    assert len(set(want.ravel().tolist())) > 1      # not the same candidate everywhere
    sw.close()


# ------------------------------------------------------------------ 4. detach, and the value tail
@pytest.mark.parametrize("kind,per_drone", KINDS, ids=IDS)
def test_clear_tracking_restores_the_plain_tick_and_value_is_refused(kind, per_drone):
    sw, twin = prepared(CFG, twins=1, grounded=True)
    pl, plain = planner(sw, kind, per_drone), planner(twin, kind, per_drone)
    attach(pl, sw)
    pl.track()
    if not per_drone:   # (a value tail is env-level only)
        with pytest.raises(L.QuadSwarmError, match="qs_value_" + kind + "_set"):
            pl.set_value(gamma=0.9)
        assert pl.cost_agent is not None
    pl.clear_tracking()
    assert pl.cost_agent is None and (pl.ret_agent is None) == (not per_drone)
    for tick in range(2):   # (track() moved neither the tick nor the sequence)
        pl.plan()
        plain.plan()
        assert buffers(pl, kind) == buffers(plain, kind), tick
    if not per_drone:
        pl.set_value(gamma=0.9)
        ref, base = make_reference(sw)
        with pytest.raises(L.QuadSwarmError, match="qs_track_" + kind + "_set"):
            pl.set_tracking(ref, Q, R, base=base)
        assert pl.cost_agent is None
        pl.clear_value()
        pl.set_tracking(ref, Q, R, base=base)
        assert pl.cost_agent is not None
    sw.close()
    twin.close()


# ------------------------------------------------------------------ 5. capture
def test_captured_rounds_replay_eager_rounds_and_read_ref_live():
    cap, eager = prepared(CFG, twins=1)
    pc, pe = (sw.mppi(N, C, 0.3, lam=0.3, seed=8) for sw in (cap, eager))
    nom = random_sequence(pc, scale=0.9)
    refs = []
    for sw, pl in ((cap, pc), (eager, pe)):
        pl.reset(nom)
        ref, base = make_reference(sw, rows=N + 2)
        base.zero_()
        pl.set_tracking(ref, Q, R, terminal=TERMINAL, reward_scale=0.25, base=base)
        refs.append((ref, base))
    want = []
    for _ in range(3):
        r = pe.step_t()
        refs[1][1].add_(1)
        torch.cuda.synchronize()
        want.append((pe.action.clone(), r.obs.clone(), pe.ret.clone(), pe.cost_agent.clone()))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        r = pc.step_t()
        refs[0][1].add_(1)
    for k in range(3):
        g.replay()
        torch.cuda.synchronize()
        same_bytes(pc.action, want[k][0], f"action, round {k}")
        same_bytes(r.obs, want[k][1], f"obs, round {k}")
        same_bytes(pc.ret, want[k][2], f"ret, round {k}")
        same_bytes(pc.cost_agent, want[k][3], f"cost_agent, round {k}")
    same_bytes(refs[0][1], refs[1][1], "base")
    assert int(refs[0][1][0]) == 3
    assert fingerprint(cap)[:4] == fingerprint(eager)[:4]
    # the reference is read where it lives: an in-place update shows in the next replay
    for ref, _ in refs:
        ref.add_(0.5)
    g.replay()
    pe.step_t()
    refs[1][1].add_(1)
    torch.cuda.synchronize()
    same_bytes(pc.cost_agent, pe.cost_agent, "cost_agent, captured against eager, after the update")
    same_bytes(pc.action, pe.action, "action after the update")
    for ref, _ in refs:
        ref.sub_(0.5)
    g.replay()
    torch.cuda.synchronize()
    moved = pc.cost_agent.clone()
    pe.step_t()
    torch.cuda.synchronize()
    same_bytes(moved, pe.cost_agent, "cost_agent once more, the update undone")
    cap.close()
    eager.close()


# ------------------------------------------------------------------ 6. direction
def test_a_higher_reference_ends_higher():
    heights = []
    for z in (0.3, 0.9):
        sw = QuadSwarm(**CFG)
        sw.reset(5)
        pl = sw.mppi(N, C, 0.5, lam=0.05, seed=2)
        ref = torch.zeros((1, sw.num_envs, sw.num_drones, 12), device=sw.device)
        ref[..., 2] = z
        q = [0.0] * 12
        q[2] = 1.0
        pl.set_tracking(ref, q, reward_scale=0.0)
        for _ in range(40):
            pl.step_t()
        torch.cuda.synchronize()
        heights.append(float(sw.get_state(L.STATE_AGENT)[L.F_POS + 2].double().mean()))
        sw.close()
    print(f"mean final height: reference 0.3 -> {heights[0]:.4f}, reference 0.9 -> {heights[1]:.4f}")
    assert heights[1] > heights[0]
