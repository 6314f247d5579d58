"""The inputs of tests/test_gpu_action_parity.py, checked without a GPU: every
(config, program) pair of action_programs.MATRIX, 16 envs, 300 steps, reset
seed 3, on the CPU oracle alone.

The fp64 oracle runs free under the program.  Before each step its four state
blocks are injected into the oracle's fp32 instantiation (the exact fp32
restatement: IEEE division / sqrt, libm transcendentals) and both step the
same actions.  Three properties make the pair a valid GPU case:

 1. Conditioning.  The fp32 oracle's state, obs and reward stay within HALF of
    the project's fp32 teacher-forced tolerances (test_gpu_parity's STATE_TOL,
    OBS_TOL, REW_TOL at precision 4, the same atol + rtol * |x| form) of the
    fp64 oracle, at every step.  So where an exact fp32 evaluation lands is not
    in question on these inputs, and a kernel that misses the full tolerance
    there is wrong rather than unlucky.  Measured largest error / tolerance
    per config over its programs, as (state, obs, reward), printed by this
    file under `pytest -s`:
        C3_mh_onedpid_d8       0.045  0.006  0.038
        C3v_mh_vel_d8          0.168  0.172  0.056
        C4_spiral_vel_d5       0.213  0.173  0.031   (state: `wide`)
        mh_pid_d3              0.211  0.169  0.081   (state: `hold`)
        C2_mh_rpm_d4           0.030  0.047  0.049
        mh_onedrpm_d2          0.004  0.004  0.099
        cf2p_mh_vel_d4_pyb     0.082  0.082  0.030
        meetup_vel_d4          0.067  0.066  0.025
        leader_onedpid_d3_pyb  0.005  0.002  0.059
    The terminal obs of done envs
    counts as obs here, since the GPU test asserts it: that is what found the
    roll = +-pi sign flip behind action_programs.RPM_HOLD_SKEW.
 2. No flag difference: terminated, truncated and reasons never differ.
 3. Coverage: each counter action_programs.MATRIX names for the pair reaches
    the floor of 16 (one per env on average), on the fp64 run and on a free run
    of the fp32 oracle (the run the GPU test's precision-4 case steps beside).

Downwash stays out: with `dw` in aux the reference's downwash
term is singular as a drone passes another's height, the two oracles part by up
to 2e8 times the tolerance in one control step under these programs, and no
kernel parity can be asserted there; the matrix test below keeps such configs out.
"""
import numpy as np
import pytest

import action_programs as ap
import qs_oracle
import test_gpu_parity as gp

CONDITION = 0.5


def ratio(got, want, tol):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float((np.abs(got - want) / (tol[0] + tol[1] * np.abs(want))).max())


def oracle(cfg, precision):
    return qs_oracle.OracleSim(num_envs=ap.E, precision=precision, **cfg)


def run_pair(name, prog):
    """(worst ratios, flag differences, Coverage) of the injected fp32 oracle beside the free fp64 one."""
    cfg = gp.CONFIGS[name]
    hi, lo = oracle(cfg, 8), oracle(cfg, 4)
    hi.reset(ap.RESET_SEED)
    lo.reset(ap.RESET_SEED)
    fn = ap.Program(prog, cfg["act"], hi.E, hi.D, hi.A)
    cov = ap.Coverage(cfg["task"], cfg["act"], hi.E, hi.D)
    worst = dict(state=0.0, obs=0.0, reward=0.0)
    flags = 0
    for t in range(ap.STEPS):
        for block in range(4):
            lo.set_state(block, hi.get_state(block))
        before = hi.get_state(0)
        a = fn(t, before)
        assert a.shape == (hi.E, hi.D, hi.A) and a.dtype == np.float32 and np.isfinite(a).all()
        c, g = hi.step(a), lo.step(a)
        np.testing.assert_array_equal(c["actions"], a)
        flags += sum(int((c[k] != g[k]).sum()) for k in ("terminated", "truncated", "reasons"))
        after = hi.get_state(0)
        assert np.isfinite(after).all() and np.isfinite(c["obs"]).all(), f"t={t}"
        worst["state"] = max(worst["state"], ratio(lo.get_state(0), after, gp.STATE_TOL[4]))
        worst["obs"] = max(worst["obs"], ratio(g["obs"], c["obs"], gp.OBS_TOL[4]))
        worst["reward"] = max(worst["reward"], ratio(g["reward"], c["reward"], (gp.REW_TOL[4],) * 2))
        done = (c["terminated"] | c["truncated"]).astype(bool)
        if done.any():
            worst["obs"] = max(worst["obs"], ratio(g["terminal_obs"][done], c["terminal_obs"][done], gp.OBS_TOL[4]))
        cov.update(before, c, after)
    hi.close()
    lo.close()
    return worst, flags, cov


def free_coverage(name, prog, precision):
    """Coverage of the oracle at `precision` running free under the program (the GPU test's oracle side)."""
    cfg = gp.CONFIGS[name]
    o = oracle(cfg, precision)
    o.reset(ap.RESET_SEED)
    fn = ap.Program(prog, cfg["act"], o.E, o.D, o.A)

    def steps():
        for t in range(ap.STEPS):
            before = o.get_state(0)
            c = o.step(fn(t, before))
            yield before, c, o.get_state(0)

    cov = ap.coverage(cfg["task"], cfg["act"], o.E, o.D, steps())
    o.close()
    return cov


@pytest.mark.parametrize("name,prog", ap.PAIRS, ids=ap.PAIR_IDS)
def test_pair_is_conditioned_flag_exact_and_reaches_its_branches(name, prog):
    worst, flags, cov = run_pair(name, prog)
    print(f"\n{name} {prog}: ratio state {worst['state']:.3f} obs {worst['obs']:.3f} reward {worst['reward']:.3f} "
          f"flag differences {flags} | " + " ".join(f"{k}={v}" for k, v in cov.n.items() if v))
    for k, v in worst.items():
        assert v <= CONDITION, f"{name} {prog}: fp32 oracle {k} at {v:.3f} of the fp32 tolerance (> {CONDITION})"
    assert flags == 0
    cov.check(name, prog)
    free = free_coverage(name, prog, 4)
    print(f"{name} {prog}: free fp32 oracle | " + " ".join(f"{k}={v}" for k, v in free.n.items() if v))
    free.check(name, prog)


@pytest.mark.parametrize("prog", ap.SEQ_PROGRAMS)
@pytest.mark.parametrize("name", ap.SEQ_CONFIGS)
def test_sequence_windows_end_episodes(name, prog):
    """The multi-step launches' inputs: the first 32 steps of the program from reset end
    episodes (terminations, hence auto-resets inside one launch) on the fp32 oracle."""
    cfg = gp.CONFIGS[name]
    o = oracle(cfg, 4)
    o.reset(ap.RESET_SEED)
    acts = ap.sequence(prog, cfg["act"], o.E, o.D, o.A, ap.SEQ_STEPS)
    assert acts.shape == (ap.SEQ_STEPS, o.E, o.D, o.A) and acts.dtype == np.float32
    ended = sum(int(o.step(a)["terminated"].sum()) for a in acts)
    o.close()
    assert ended >= 4, ended


def test_matrix_names_known_configs_programs_and_counters():
    assert len(ap.PAIRS) == 27
    for name, progs in ap.MATRIX.items():
        cfg = gp.CONFIGS[name]
        assert "dw" not in cfg.get("aux", ())   # downwash stays out: the oracles themselves part there
        for prog, counters in progs.items():
            assert set(counters) <= set(ap.Coverage.KEYS) and counters
            if prog == "seek":
                assert cfg["task"] == "multihover" and cfg["act"] != "rpm"
            if "n0" in counters:
                assert cfg["act"] == "vel"
            if {"far", "near", "int_xy"} & set(counters):
                assert cfg["act"] == "pid"


def test_programs_are_deterministic_and_shaped():
    st = np.zeros((29, 6))
    st[ap.F_TARGET + 2] = 1.0
    for name in ("zero", "hold", "wide", "extreme", "seek"):
        a, b = (ap.Program(name, "vel", 2, 3, 4) for _ in range(2))
        for t in (0, 1, 24, 25, 26):
            x, y = a(t, st), b(t, st)
            assert x.shape == (2, 3, 4) and x.dtype == np.float32 and np.array_equal(x, y)
    hold = ap.Program("hold", "pid", 2, 3, 3)
    h0, h24, h25 = hold(0, st), hold(24, st), hold(25, st)
    assert np.array_equal(h0, h24) and not np.array_equal(h0, h25) and set(np.unique(h0)) <= set(ap.HOLD_VALUES)
    skew = ap.Program("hold", "rpm", 2, 3, 4)(0, st) - ap.Program("hold", "vel", 2, 3, 4)(0, st)
    np.testing.assert_allclose(skew, np.broadcast_to(0.01 * np.arange(4), (2, 3, 4)), atol=1e-6)
    ex = ap.Program("extreme", "rpm", 4, 2, 4)(0, st)
    assert (ex[0::2] == 20).all() and (ex[1::2] == -20).all()
    seek = ap.Program("seek", "vel", 2, 3, 4)(0, st)   # 1 m below the target: straight up at full speed
    assert np.array_equal(seek[..., :3], np.broadcast_to(np.float32([0, 0, 1]), (2, 3, 3))) and (seek[..., 3] == 1).all()
    assert (ap.Program("seek", "one_d_pid", 2, 3, 1)(0, st) == 1).all()
    with pytest.raises(ValueError):
        ap.Program("seek", "rpm", 2, 3, 4)
