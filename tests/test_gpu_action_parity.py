"""Given-action steps of the HIP kernel against the CPU oracle where the random
policy never goes ("given-action matrix").

Planner ticks, branch sets and `score` are byte-identical to `step_many` over
caller-supplied actions, and that to `step(actions)`; this file pins that last
link to the oracle on inputs that reach the clamp chain of the DSL PID, every
termination reason and its auto-reset, the terminal obs of a crash, the
reward's threshold branches and the VEL zero-direction guard.

 1. test_given_action_parity: teacher-forced one-step parity (test_gpu_parity's
    loop and tolerances, unchanged) against the oracle at the SAME precision,
    16 envs, 300 steps, reset seed 3, over the (config, program) pairs of
    action_programs.MATRIX x precision {8, 4}.  Exact: actions, truncated,
    terminated, reasons, env block, history.  Within OBS_TOL / REW_TOL /
    STATE_TOL: obs, reward, terminal obs of done envs, agent state.  Each run
    also asserts, from the oracle side, that it reached the branches it is
    there for (action_programs.Coverage, floor 16), so it cannot pass by not
    going there.  tests/test_action_programs_cases.py shows on the CPU that
    the exact-fp32 restatement holds a quarter of the fp32 bounds on these
    inputs with no flag difference, so a miss here is a kernel finding.
    No flag or reason tie is excused: the file skips no env-step.
 2. test_program_sequences_equal_single_steps: the first 32 steps of `extreme`
    and of `hold` from reset through `step_many(outs, actions=...)` against 32
    single `step(actions[j])` calls, byte for byte (outputs, the four state
    blocks, the episode log); both end episodes inside the window.
 3. test_score_of_programs_equals_sequences: `score` with the candidates
    `zero`, `hold`, `extreme` against `step_many` per candidate, bytes, and
    ret / first_done against the float64 running sum up to the first done.

Downwash configs stay out: the two oracles themselves part there.

Largest error / tolerance per config and precision over its programs (state,
obs incl. terminal obs, reward), MI355X, as printed by test 1:
    config                   fp64: state  obs    reward   fp32: state  obs    reward
    C3_mh_onedpid_d8               0.000  0.000  0.000          0.006  0.006  0.015
    C3v_mh_vel_d8                  0.027  0.000  0.000          0.242  0.230  0.099
    C4_spiral_vel_d5               0.036  0.000  0.001          0.426  0.439  0.049
    mh_pid_d3                      0.015  0.000  0.001          0.209  0.202  0.158
    C2_mh_rpm_d4                   0.001  0.000  0.000          0.012  0.040  0.012
    mh_onedrpm_d2                  0.000  0.000  0.000          0.001  0.001  0.011
    cf2p_mh_vel_d4_pyb             0.011  0.000  0.000          0.087  0.090  0.074
    meetup_vel_d4                  0.009  0.000  0.000          0.092  0.090  0.021
    leader_onedpid_d3_pyb          0.000  0.000  0.000          0.003  0.003  0.011
(0.000: below 0.0005.)  The largest, 0.44, is Spiral VEL `extreme` at fp32; the
CPU file's exact-fp32 restatement reaches 0.21 against the fp64 oracle there.
Every flag, reason, env counter and history byte was equal; nothing needed fixing.

Sensitivity, observed once on an MI355X with deliberately wrong kernels (scratch
builds, not committed), each run through test 1 of this file (54 cases) and
through tests/test_gpu_parity.py (108 tests):
  a. MAX_PWM clip of the DSL PID's mixer raised from 65535 to 70000.  Here: 34
     cases fail at "obs" -- every `hold`, `wide` and `extreme` case of the seven
     PID-type configs and all of mh_pid_d3's.  Also caught by the old file (25
     tests): teacher-forced mh_pid_d3 and the D = 4 and downwash one_d_pid
     configs, and test_given_actions_parity.
  b. Hover bonus dropped from the MultiHover reward.  Here: 14 cases fail at
     "reward" -- `seek` on C3, C3-VEL, mh_pid_d3 and CF2P VEL, C3 `hold`, C3-VEL
     `wide`, mh_onedrpm_d2 `hold`.  Also caught by the old file (28 tests, all
     one_d_pid / one_d_rpm configs, C3 among them; no VEL config).
  c. one_d_pid: the reasons of an env that auto-resets taken after the reset.
     Here: C3 `hold` and `extreme` fail at "reasons", fp64 and fp32.  Also caught
     by the old file (15 tests) on the one_d_pid configs whose random-policy
     episodes crash (D = 4 default layout, downwash), not on C3.
So the old file, through its smaller configs, already catches all three.  Two
further wrong kernels that it does NOT catch (all 108 of its tests pass) and
this file does, and a third that it catches on one config only:
  d. The VEL zero-direction guard (`n != 0`) lost.  Old file: passes.  Here:
     `zero` on C3-VEL and C4 and `hold` on C3-VEL fail, three cases at "obs" and
     three at the finiteness assertion of this file's loop (assert_close's
     `err > lim` lets a NaN through).
  e. The QS_REASON_OOB test dropped.  Old file: only teacher-forced
     C2p_mh_rpm_d4_pyb fails ("reasons").  Here: `extreme` on C3-VEL and on
     mh_pid_d3 fail at "terminated", fp64 and fp32.
  f. Hover bonus dropped for VEL actions only.  Old file: passes.  Here: C3-VEL
     `wide` and `seek` and CF2P VEL `seek` fail at "reward", fp64 and fp32.
"""
import numpy as np
import pytest
import torch

import action_programs as ap
import test_gpu_parity as gp
import test_gpu_step_score as ss
import test_gpu_step_sequence as sq

pytestmark = pytest.mark.gpu

CASES = [(name, prog, precision) for name, prog in ap.PAIRS for precision in (8, 4)]
CASE_IDS = [f"{name}-{prog}-fp{8 * precision}" for name, prog, precision in CASES]


def ratio(got, want, tol):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if got.size == 0:
        return 0.0
    return float((np.abs(got - want) / (tol[0] + tol[1] * np.abs(want))).max())


def teacher_forced(name, prog, precision):
    """test_gpu_parity.teacher_forced with the program's actions formed from the oracle's
    state, the run's coverage counted from the oracle side and the worst error / tolerance
    kept; every assertion of that loop is here."""
    cfg = gp.CONFIGS[name]
    E = ap.E
    sw, orc = gp.make_pair(cfg, E, precision)
    o_g = sw.reset(ap.RESET_SEED).cpu().numpy()
    o_c = orc.reset(ap.RESET_SEED)
    np.testing.assert_array_equal(o_g[..., :3], o_c[..., :3])   # reset draws bit-identical
    gp.assert_close("reset obs", o_g, o_c, gp.OBS_TOL[precision])
    fn = ap.Program(prog, cfg["act"], E, orc.D, orc.A)
    cov = ap.Coverage(cfg["task"], cfg["act"], E, orc.D)
    obs_tol, st_tol, rew_tol = gp.OBS_TOL[precision], gp.STATE_TOL[precision], (gp.REW_TOL[precision],) * 2
    worst = dict(state=0.0, obs=0.0, reward=0.0)
    actions_out = torch.zeros((E, sw.num_drones, sw.act_dim), device=sw.device)
    for t in range(ap.STEPS):
        gp.inject(sw, orc)
        before = orc.get_state(0)
        acts = fn(t, before)
        r = sw.step(torch.as_tensor(acts, device=sw.device), want_terminal=True, want_reasons=True,
                    actions_out=actions_out)
        c = orc.step(acts)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(c["actions"], acts, err_msg=f"oracle actions t={t}")
        np.testing.assert_array_equal(r.actions.cpu().numpy(), c["actions"], err_msg=f"actions t={t}")
        np.testing.assert_array_equal(r.truncated.cpu().numpy(), c["truncated"], err_msg=f"truncated t={t}")
        np.testing.assert_array_equal(r.terminated.cpu().numpy(), c["terminated"], err_msg=f"terminated t={t}")
        np.testing.assert_array_equal(r.reasons.cpu().numpy(), c["reasons"], err_msg=f"reasons t={t}")
        done = (c["terminated"] | c["truncated"]).astype(bool)
        obs, rew, tob = r.obs.cpu().numpy(), r.reward.cpu().numpy(), r.terminal_obs.cpu().numpy()
        st, after = sw.get_state(0).cpu().numpy(), orc.get_state(0)
        # assert_close's `err > lim` lets a NaN through (a lost zero-direction guard gives 0 / 0)
        assert np.isfinite(obs).all() and np.isfinite(rew).all() and np.isfinite(st).all(), f"not finite t={t}"
        assert np.isfinite(tob[done]).all(), f"terminal obs not finite t={t}"
        worst["obs"] = max(worst["obs"], ratio(obs, c["obs"], obs_tol), ratio(tob[done], c["terminal_obs"][done], obs_tol))
        worst["reward"] = max(worst["reward"], ratio(rew, c["reward"], rew_tol))
        worst["state"] = max(worst["state"], ratio(st, after, st_tol))
        gp.assert_close(f"obs t={t}", obs, c["obs"], obs_tol)
        gp.assert_close(f"reward t={t}", rew, c["reward"], rew_tol)
        if done.any():
            gp.assert_close(f"terminal obs t={t}", tob[done], c["terminal_obs"][done], obs_tol)
        gp.assert_close(f"agent state t={t}", st, after, st_tol)
        np.testing.assert_array_equal(sw.get_state(1).cpu().numpy(), orc.get_state(1), err_msg=f"env t={t}")
        np.testing.assert_array_equal(sw.get_state(2).cpu().numpy(), orc.get_state(2), err_msg=f"hist t={t}")
        cov.update(before, c, after)
    assert sw.reset_error() == 0
    sw.close()
    orc.close()
    return worst, cov


@pytest.mark.parametrize("name,prog,precision", CASES, ids=CASE_IDS)
def test_given_action_parity(name, prog, precision):
    worst, cov = teacher_forced(name, prog, precision)
    print(f"\nRATIO {name} {prog} fp{8 * precision}: state {worst['state']:.3f} obs {worst['obs']:.3f} "
          f"reward {worst['reward']:.3f} | " + " ".join(f"{k}={v}" for k, v in cov.n.items() if v))
    cov.check(name, prog)


# ------------------------------------------------------- multi-step launches on the same inputs
SEQ_STEPS = ap.SEQ_STEPS


def program_actions(prog, name, sw):
    """The first SEQ_STEPS steps of an open-loop program as an (n, E, D, A) tensor on the swarm's device."""
    a = ap.sequence(prog, gp.CONFIGS[name]["act"], sw.num_envs, sw.num_drones, sw.act_dim, SEQ_STEPS)
    return torch.as_tensor(a, device=sw.device)


def swarms(name, n):
    out = []
    for _ in range(n):
        sw, orc = gp.make_pair(gp.CONFIGS[name], ap.E, 4)
        orc.close()
        sw.reset(ap.RESET_SEED)
        out.append(sw)
    return out


@pytest.mark.parametrize("prog", ap.SEQ_PROGRAMS)
@pytest.mark.parametrize("name", ap.SEQ_CONFIGS)
def test_program_sequences_equal_single_steps(name, prog, monkeypatch):
    monkeypatch.delenv("QS_MAX_FUSED_STEPS", raising=False)
    one, many = swarms(name, 2)
    acts = program_actions(prog, name, one)
    o1, o2 = sq.Outs(one, SEQ_STEPS), sq.Outs(many, SEQ_STEPS)
    sq.eager(one, acts, o1.kws())
    many.step_many(o2.kws(), actions=acts)
    torch.cuda.synchronize()
    assert o1.bufs["terminated"].sum().item() > 0   # episodes end inside the window
    sq.same_bytes(o2.bufs["actions_out"], acts, "actions_out is the actions")
    sq.same_outputs(o1, o2)
    sq.same_state(one, many)
    assert one.reset_error() == 0 and many.reset_error() == 0
    sq.close(one, many)


def test_score_of_programs_equals_sequences(monkeypatch):
    monkeypatch.delenv("QS_MAX_FUSED_STEPS", raising=False)
    n, progs, name = SEQ_STEPS, ap.SCORE_PROGRAMS, ap.SEQ_CONFIGS[0]
    sw, ref = swarms(name, 2)
    assert sw.score_depth() >= n
    acts = torch.stack([program_actions(p, name, sw) for p in progs], dim=1).contiguous()   # (n, C, E, D, A)
    C = len(progs)
    snap, before = ss.snapshot(sw), ss.fingerprint(sw)
    got = ss.Outs(sw, n, lead=(C,))
    ret = torch.full((C, sw.num_envs), -7.0, dtype=torch.float64, device=sw.device)
    fd = torch.full((C, sw.num_envs), -7, dtype=torch.int32, device=sw.device)
    sw.score(acts, got.kws(), ret=ret, first_done=fd)
    torch.cuda.synchronize()
    want = ss.reference(ref, snap, acts)
    for k in ss.OUT_KEYS:
        ss.same_bytes(want.bufs[k], got.bufs[k], k)
    r, t, u = (want.bufs[k].cpu().numpy() for k in ("reward", "terminated", "truncated"))
    wret, wfd = ss.running_score(r, t, u)
    assert np.array_equal(ret.cpu().numpy(), wret) and np.array_equal(fd.cpu().numpy(), wfd)
    assert (wfd[0] == n).all()                            # `zero` holds every env for the window
    assert (wfd[1] < n).any()                             # `hold` crashes some envs,
    assert (wfd[2, 1::2] < n).all() and (wfd[2, 0::2] == n).all()   # `extreme` the odd ones (-20), no even one (+20)
    assert ss.fingerprint(sw) == before
    ss.close(sw, ref)
