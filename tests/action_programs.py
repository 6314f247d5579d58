"""Deterministic action programs that take given-action steps where the random
policy never goes, and the counters that prove they got there (test
infrastructure: no GPU import; used by tests/test_action_programs_cases.py on
the CPU and tests/test_gpu_action_parity.py on the GPU).

The in-kernel random policy (uniform in [-1, 1), zero mean) ends no episode but
by truncation on the flagship configs, never saturates the PID integrators or
the motor command, never gives a VEL action of zero direction and hardly ever
earns the hover bonus.  The programs here do, by construction:

  zero     all zeros (VEL: the `n != 0` guard of the direction normalisation)
  hold     every component redrawn from {-3, -1, -0.5, 0, 0.5, 1, 3} every 25
           steps and held in between (integrator wind-up, saturated motors,
           crashes, flips).  25, not 50: at 50 the one_d_pid D = 8 run earns
           the hover bonus 16 times, exactly the floor; at 25, 168 times.
           On rpm actions motor k gets + 0.01 k (RPM_HOLD_SKEW below).
  wide     3 * N(0, 1), independent every step, drawn as float32 (flips,
           Spiral z range: 21 ends; drawn as float64 and rounded, 15, one
           short of the floor)
  extreme  +20 in even envs, -20 in odd envs, every component, every step
           (every clamp of the chain at once; crashes and out-of-bounds)
  seek     closed loop on the state about to be stepped, MultiHover only and
           not for `rpm`: flies every drone to its target (the hover bonus and
           the reward's threshold branches)

A program is `Program(name, act, E, D, A)`; calling it with `(t, state0)`, the
agent state-of-arrays block of the oracle that is about to step, returns the
(E, D, A) float32 actions of step t.  Its generator is
`np.random.default_rng(7)`, created per program object, i.e. per run.

`Coverage` counts, from the oracle's step outputs and its state block 0 alone,
what a run reached.  MATRIX lists, per config of test_gpu_parity.CONFIGS and
program, the counters that must reach FLOOR.
"""
import numpy as np

# rows of the agent state-of-arrays block (include/quadswarm.h, QS_F_*)
F_POS, F_VEL, F_LAST_RPM, F_PID_INT_POS, F_TARGET = 0, 7, 13, 17, 26
# QS_REASON_* bits
REASON_BITS = dict(crash=1, flip=2, oob=4, zrange=8)

E, STEPS, RESET_SEED, RNG_SEED = 16, 300, 3, 7
FLOOR = 16   # one event per env on average

HOLD_EVERY = 25
HOLD_VALUES = (-1.0, 1.0, -0.5, 0.5, 0.0, 3.0, -3.0)
# `hold` on rpm actions adds k * this to motor k.  Equal values on a motor pair give a torque about
# exactly one body axis; a pure pitch tumble that passes 90 degrees inside the step that ends the
# episode leaves roll = atan2(+-rounding noise, negative) = +-pi in the terminal obs, whose sign no
# two evaluations agree on (fp64 oracle +pi, fp32 oracle -pi: 15 000 times the obs tolerance)
RPM_HOLD_SKEW = 0.01
WIDE_SIGMA = 3.0
EXTREME = 20.0

# the DSL PID's integrator clamps and the motor command's PWM clip, as rpm (PWM2RPM_SCALE * pwm + PWM2RPM_CONST)
INT_Z_CLAMP, INT_XY_CLAMP = 0.15, 2.0
RPM_AT_MAX_PWM = 0.2685 * 65535 + 4070.3
RPM_AT_MIN_PWM = 0.2685 * 20000 + 4070.3
HOVER_BAND = 0.03   # MultiHover bonus: err_xy, |err_z| and |v_z| all below it

# config -> program -> the counters that must reach FLOOR ("n0" under `zero`: every row of every step)
MATRIX = {
    "C3_mh_onedpid_d8": dict(hold=("crash", "hover", "int_z", "pwm_hi"), extreme=("crash", "int_z", "pwm_hi"),
                             seek=("hover",)),
    "C3v_mh_vel_d8": dict(zero=("n0",), hold=("crash", "pwm_hi"), wide=("flip",),
                          extreme=("crash", "flip", "oob", "pwm_hi"), seek=("hover",)),
    "C4_spiral_vel_d5": dict(zero=("n0",), hold=("zrange", "pwm_hi"), wide=("zrange",), extreme=("zrange", "pwm_hi")),
    "mh_pid_d3": dict(hold=("far", "near", "crash", "int_xy"), extreme=("oob", "int_xy"), seek=("hover",)),
    "C2_mh_rpm_d4": dict(hold=("flip",), wide=("flip",), extreme=("crash",)),
    "mh_onedrpm_d2": dict(hold=("crash",), extreme=("crash",)),
    "cf2p_mh_vel_d4_pyb": dict(hold=("crash",), extreme=("crash", "flip"), seek=("hover",)),
    "meetup_vel_d4": dict(hold=("trunc",), extreme=("trunc",)),
    "leader_onedpid_d3_pyb": dict(hold=("int_z",), extreme=("int_z", "trunc")),
}
PAIRS = [(name, prog) for name, progs in MATRIX.items() for prog in progs]
PAIR_IDS = [f"{name}-{prog}" for name, prog in PAIRS]

# the multi-step launches' inputs: the first SEQ_STEPS steps of SEQ_PROGRAMS from reset, fp32
SEQ_CONFIGS = ("C3_mh_onedpid_d8", "C3v_mh_vel_d8", "mh_pid_d3", "C2_mh_rpm_d4", "C4_spiral_vel_d5")
SEQ_PROGRAMS = ("extreme", "hold")
SEQ_STEPS = 32
SCORE_PROGRAMS = ("zero", "hold", "extreme")   # the candidates of the `score` case, on SEQ_CONFIGS[0]


def agents(state0, row, n, E, D):
    """Rows row .. row + n of a (fields, E * D) state block as (E, D, n)."""
    return np.asarray(state0[row:row + n], np.float64).T.reshape(E, D, n)


class Program:
    def __init__(self, name, act, E, D, A):
        if name not in ("zero", "hold", "wide", "extreme", "seek"):
            raise ValueError(name)
        if name == "seek" and act == "rpm":
            raise ValueError("seek is not defined for rpm actions")
        self.name, self.act, self.shape = name, act, (E, D, A)
        self.rng = np.random.default_rng(RNG_SEED)
        self.held = None

    def __call__(self, t, state0):
        E, D, A = self.shape
        if self.name == "zero":
            return np.zeros(self.shape, np.float32)
        if self.name == "hold":
            if t % HOLD_EVERY == 0:
                self.held = self.rng.choice(HOLD_VALUES, size=self.shape).astype(np.float32)
                if self.act == "rpm":
                    self.held += np.float32(RPM_HOLD_SKEW) * np.arange(A, dtype=np.float32)
            return self.held.copy()
        if self.name == "wide":
            return self.rng.standard_normal(self.shape, dtype=np.float32) * np.float32(WIDE_SIGMA)
        if self.name == "extreme":
            sign = np.where(np.arange(E) % 2 == 0, EXTREME, -EXTREME).astype(np.float32)
            return np.broadcast_to(sign[:, None, None], self.shape).copy()
        pos, tgt = agents(state0, F_POS, 3, E, D), agents(state0, F_TARGET, 3, E, D)
        a = np.zeros(self.shape, np.float32)
        if self.act == "pid":
            a[:] = tgt
        elif self.act in ("one_d_pid", "one_d_rpm"):
            a[..., 0] = np.clip((tgt[..., 2] - pos[..., 2]) / 0.1, -1.0, 1.0)
        elif self.act == "vel":
            d = tgt - pos
            a[..., :3] = d
            a[..., 3] = np.minimum(2.0 * np.linalg.norm(d, axis=-1), 1.0)
        else:
            raise ValueError(self.act)
        return a


def sequence(name, act, E, D, A, n):
    """The first n steps of an open-loop program (every one but `seek`) as an (n, E, D, A) float32 array."""
    if name == "seek":
        raise ValueError("seek is closed loop: it has no sequence without the states")
    prog = Program(name, act, E, D, A)
    return np.stack([prog(t, None) for t in range(n)])


class Coverage:
    """Event counts of one run.  update() takes what one oracle step gives: its
    state block 0 before the step, its output dict, its state block 0 after.
    `done` and `pwm_lo` (motor command at the MIN_PWM rpm) are informational:
    they are printed with the others but no pair has a floor for them."""
    KEYS = ("done", "trunc", "crash", "flip", "oob", "zrange", "hover", "int_z", "int_xy", "pwm_hi", "pwm_lo", "n0",
            "far", "near")

    def __init__(self, task, act, E, D):
        self.task, self.act, self.E, self.D = task, act, E, D
        self.rows = 0
        self.n = dict.fromkeys(self.KEYS, 0)

    def update(self, before, out, after):
        E, D, n = self.E, self.D, self.n
        self.rows += E * D
        term, trunc = out["terminated"].astype(bool), out["truncated"].astype(bool)
        n["done"] += int((term | trunc).sum())
        n["trunc"] += int(trunc.sum())
        for k, bit in REASON_BITS.items():
            n[k] += int(((out["reasons"] & bit) != 0).sum())
        after = np.asarray(after, np.float64)
        if self.task == "multihover":
            p, tg = after[F_POS:F_POS + 3], after[F_TARGET:F_TARGET + 3]
            exy, ez, vz = np.hypot(p[0] - tg[0], p[1] - tg[1]), np.abs(p[2] - tg[2]), np.abs(after[F_VEL + 2])
            n["hover"] += int(((exy < HOVER_BAND) & (ez < HOVER_BAND) & (vz < HOVER_BAND)).sum())
        n["int_z"] += int((np.abs(after[F_PID_INT_POS + 2]) >= INT_Z_CLAMP).sum())
        n["int_xy"] += int((np.abs(after[F_PID_INT_POS:F_PID_INT_POS + 2]) >= INT_XY_CLAMP).sum())
        rpm = after[F_LAST_RPM:F_LAST_RPM + 4]
        n["pwm_hi"] += int(np.isclose(rpm, RPM_AT_MAX_PWM, rtol=1e-6, atol=0.0).sum())
        n["pwm_lo"] += int(np.isclose(rpm, RPM_AT_MIN_PWM, rtol=1e-6, atol=0.0).sum())
        a = np.asarray(out["actions"], np.float64)
        if self.act == "vel":
            n["n0"] += int((np.linalg.norm(a[..., :3], axis=-1) == 0).sum())
        if self.act == "pid":
            dist = np.linalg.norm(a - agents(before, F_POS, 3, E, D), axis=-1)
            n["far"] += int((dist > 1.0).sum())
            n["near"] += int((dist <= 1.0).sum())

    def check(self, config, program):
        """The floors of MATRIX[config][program]; returns the counts."""
        for k in MATRIX[config][program]:
            if program == "zero" and k == "n0":
                assert self.n[k] == self.rows, f"{config} {program}: n0 {self.n[k]} of {self.rows} rows"
            else:
                assert self.n[k] >= FLOOR, f"{config} {program}: {k} = {self.n[k]} < {FLOOR} ({self.n})"
        return dict(self.n)


def coverage(task, act, E, D, steps):
    """The Coverage of a run given as an iterable of (before, out, after)
    triples: the oracle's state block 0 before a step, the step's output dict,
    its state block 0 after."""
    cov = Coverage(task, act, E, D)
    for before, out, after in steps:
        cov.update(before, out, after)
    return cov
