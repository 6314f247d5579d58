"""QuadSwarm: the device-resident batch of (env × drone) quadrotors.

Thin host object over the C-ABI handle (include/quadswarm.h).  It owns no
physics: every call is one launch of the HIP step kernel on the caller's
current stream, with inputs and outputs as torch tensors resident in HBM
(zero-copy — their data pointers are passed straight through).

Reference semantics it implements (paths relative to gym_pybullet_drones/):
  BaseAviary.step/reset                envs/BaseAviary.py:220-383
  BaseRLAviary action/obs types        envs/BaseRLAviary.py:132-319
  MultiHoverAviary task                envs/MultiHoverAviary.py:12-285
  SpiralFormationAviary task           envs/SpiralAviary.py:20-205
  SubprocVecEnv worker auto-reset      safe_control_gym/envs/env_wrappers/
                                       vectorized_env/subproc_vec_env.py:188-206
"""
import ctypes
import weakref
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from .. import _lib as L
from ..utils.enums import ActionType, DroneModel, Physics

_ACT = {ActionType.RPM: L.ACT_RPM, ActionType.PID: L.ACT_PID, ActionType.VEL: L.ACT_VEL,
        ActionType.ONE_D_RPM: L.ACT_ONE_D_RPM, ActionType.ONE_D_PID: L.ACT_ONE_D_PID}
# Physics → (integrator, aux force bits) (enums.py:13-21, BA:352-367).
_PHYS = {Physics.DYN: (L.PHYS_DYN, 0), Physics.PYB: (L.PHYS_PYB, 0),
         Physics.PYB_GND: (L.PHYS_PYB, L.AUX_GND), Physics.PYB_DRAG: (L.PHYS_PYB, L.AUX_DRAG),
         Physics.PYB_DW: (L.PHYS_PYB, L.AUX_DW),
         Physics.PYB_GND_DRAG_DW: (L.PHYS_PYB, L.AUX_GND | L.AUX_DRAG | L.AUX_DW)}
_AUX_NAMES = {"gnd": L.AUX_GND, "drag": L.AUX_DRAG, "dw": L.AUX_DW}
TASKS = {"multihover": L.TASK_MULTIHOVER, "spiral": L.TASK_SPIRAL, "flock": L.TASK_FLOCK, "meetup": L.TASK_MEETUP,
         "leaderfollower": L.TASK_LEADERFOLLOWER}


@dataclass
class StepResult:
    obs: torch.Tensor          # (E, D, O) float32, post auto-reset
    reward: torch.Tensor       # (E,) float32/float64
    terminated: torch.Tensor   # (E,) uint8
    truncated: torch.Tensor    # (E,) uint8
    terminal_obs: Optional[torch.Tensor] = None
    reasons: Optional[torch.Tensor] = None
    actions: Optional[torch.Tensor] = None


def grid_layout(num_drones, spacing=1.0, z=0.5):
    """Centred square-ish grid (SURVEY §7 hard-2 deviation for D >= 6): the
    reference's diagonal 4L layout (BaseAviary.py:194-197) cannot pass its own
    0.5 m rejection test for D >= 6, so the large-D configs use explicit
    initial_xyzs with `spacing` >= 1 m (acceptance 1 with the ±0.25 m noise)."""
    cols = int(np.ceil(np.sqrt(num_drones)))
    rows = int(np.ceil(num_drones / cols))
    out = []
    for i in range(num_drones):
        r, c = divmod(i, cols)
        out.append([(c - (cols - 1) / 2) * spacing, (r - (rows - 1) / 2) * spacing, z])
    return np.asarray(out, np.float64)


def _as_enum(x, enum):
    return x if isinstance(x, enum) else enum(x)


class QuadSwarm:
    """Batch of `num_envs` envs of `num_drones` drones (DroneModel.CF2X, the
    MAPPO tasks' model, or CF2P) on one GPU."""

    def __init__(self, task="multihover", num_envs=1, num_drones=2, act=ActionType.RPM, physics=Physics.DYN,
                 pyb_freq=240, ctrl_freq=None, precision=4, device=None, env_offset=0, initial_xyzs=None,
                 episode_len_sec=None, autoreset=True, drone_model=DroneModel.CF2X,
                 spiral_radius=0.4, spiral_period=10.0, height_rate=0.05, target_center=(0.0, 0.0, 0.0),
                 aux=(), inkernel_reset_search=False):
        """inkernel_reset_search: run MultiHover's whole reset rejection loop inside
        the step kernel instead of the deferred search launch (validation form).
        aux: extra force models ("gnd", "drag", "dw") added on top of `physics`;
        with Physics.DYN this is the build-defined DYN + aux combination (SURVEY §8
        physics-mode note), e.g. C5's DYN + downwash."""
        if task not in TASKS:
            raise ValueError(f"unknown task {task!r}")
        act = _as_enum(act, ActionType)
        physics = _as_enum(physics, Physics)
        drone_model = _as_enum(drone_model, DroneModel)
        # CF2X and CF2P: the models DSLPIDControl accepts (DSLPIDControl.py:34-36);
        # CF2P's inertia, props, torques and mixer ride on QS_FLAG_CF2P
        if drone_model not in (DroneModel.CF2X, DroneModel.CF2P):
            raise NotImplementedError("DroneModel.CF2X and CF2P are implemented (RACE has no DSL PID, "
                                      "DSLPIDControl.py:34-36)")
        if any(a not in _AUX_NAMES for a in aux):
            raise ValueError(f"unknown aux force model in {aux!r} (gnd, drag, dw)")
        if not torch.cuda.is_available():
            raise L.QuadSwarmError("QuadSwarm needs a ROCm GPU: the step runs only as a HIP kernel (no CPU path)")
        self.lib = L.load()
        self.task = task
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        if ctrl_freq is None:
            ctrl_freq = 48 if task == "spiral" else 30           # SP:28; MH:20 and the other MARL tasks
        if episode_len_sec is None:
            episode_len_sec = 12.0 if task == "spiral" else 8.0       # SP:39; MH:58 and the other MARL tasks
        spec = L.QsSpec()
        spec.task = TASKS[task]
        spec.num_envs = int(num_envs)
        spec.num_drones = int(num_drones)
        spec.act_type = _ACT[act]
        phys_id, aux_bits = _PHYS[physics]
        spec.physics = phys_id
        spec.aux_forces = aux_bits | sum(_AUX_NAMES[a] for a in set(aux))
        spec.pyb_freq = int(pyb_freq)
        spec.ctrl_freq = int(ctrl_freq)
        spec.precision = int(precision)
        spec.flags = ((0 if autoreset else L.FLAG_NO_AUTORESET) | (L.FLAG_INKERNEL_RESET_SEARCH if inkernel_reset_search else 0)
                      | (L.FLAG_CF2P if drone_model == DroneModel.CF2P else 0))
        spec.env_offset = int(env_offset)
        spec.episode_len_sec = float(episode_len_sec)
        self._xyz_keep = None
        if initial_xyzs is not None:
            xyz = np.ascontiguousarray(np.asarray(initial_xyzs, np.float64))
            if xyz.shape != (num_drones, 3):
                raise ValueError("invalid initial_xyzs, try initial_xyzs.reshape(NUM_DRONES,3)")  # BA:198-201
            self._xyz_keep = xyz
            spec.initial_xyzs = xyz.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        spec.spiral_radius, spec.spiral_period, spec.height_rate = spiral_radius, spiral_period, height_rate
        for i in range(3):
            spec.target_center[i] = float(target_center[i])
        self.spec = spec
        self.act_type, self.physics, self.drone_model = act, physics, drone_model
        self._h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            L.check(self.lib.qs_create(ctypes.byref(spec), self.device.index, ctypes.byref(self._h)), "qs_create")
        dims = L.QsDims()
        L.check(self.lib.qs_get_dims(self._h, ctypes.byref(dims)), "qs_get_dims")
        self.dims = dims
        self.num_envs, self.num_drones, self.num_agents = dims.num_envs, dims.num_drones, dims.num_agents
        self.act_dim, self.obs_dim, self.hist_len = dims.act_dim, dims.obs_dim, dims.hist_len
        self.substeps = dims.substeps
        self.precision = dims.precision
        self.rdtype = torch.float64 if self.precision == 8 else torch.float32
        self.pyb_freq, self.ctrl_freq = int(pyb_freq), int(ctrl_freq)
        self.episode_len_sec = float(episode_len_sec)
        self.env_offset = int(env_offset)
        E, D, O = self.num_envs, self.num_drones, self.obs_dim
        kw = dict(device=self.device)
        self.obs = torch.zeros((E, D, O), dtype=torch.float32, **kw)
        self.reward = torch.zeros(E, dtype=self.rdtype, **kw)
        self.terminated = torch.zeros(E, dtype=torch.uint8, **kw)
        self.truncated = torch.zeros(E, dtype=torch.uint8, **kw)
        self.terminal_obs = torch.zeros((E, D, O), dtype=torch.float32, **kw)
        self.reasons = torch.zeros((E, D), dtype=torch.uint8, **kw)
        self.seed = 0
        self.reset_generation = 0   # qs_reset count: the device episode counters restart at each

    # ------------------------------------------------------------------ utils
    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def close(self):
        if getattr(self, "_h", None):
            for planner in list(getattr(self, "_planners", ())):
                planner.close()
            torch.cuda.synchronize(self.device)
            self.lib.qs_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -------------------------------------------------------------- stepping
    def reset(self, seed=0, obs: Optional[torch.Tensor] = None):
        """Construct-time reset of every env (episode 0 draws); returns obs."""
        self.seed = int(seed)
        out = self.obs if obs is None else obs
        L.check(self.lib.qs_reset(self._h, ctypes.c_uint64(self.seed), L.ptr(out), self._stream()), "qs_reset")
        self.reset_generation += 1
        return out

    def reset_envs(self, mask: Optional[torch.Tensor] = None, obs: Optional[torch.Tensor] = None):
        """env.reset() (MultiHoverAviary.reset semantics) for envs with mask != 0."""
        if mask is not None:
            assert mask.dtype == torch.uint8 and mask.numel() == self.num_envs and mask.is_contiguous()
        out = self.obs if obs is None else obs
        L.check(self.lib.qs_reset_envs(self._h, L.ptr(mask), L.ptr(out), self._stream()), "qs_reset_envs")
        return out

    def step(self, actions: Optional[torch.Tensor] = None, *, obs=None, reward=None, terminated=None,
             truncated=None, terminal_obs=None, reasons=None, actions_out=None, want_terminal=False,
             want_reasons=False) -> StepResult:
        """One control step of every env.  actions: (E, D, A) float32 on device, or None
        for the synthetic random policy (Philox U(-1,1))."""
        if actions is not None:
            self._check_actions(actions)
        so, res = self._step_out(obs, reward, terminated, truncated, terminal_obs, reasons, actions_out,
                                 want_terminal, want_reasons)
        L.check(self.lib.qs_step(self._h, L.ptr(actions), ctypes.byref(so), self._stream()), "qs_step")
        return res

    def _step_out(self, obs=None, reward=None, terminated=None, truncated=None, terminal_obs=None, reasons=None,
                  actions_out=None, want_terminal=False, want_reasons=False):
        """The qs_step_out record and the StepResult of one step's output keywords."""
        obs = self.obs if obs is None else obs
        reward = self.reward if reward is None else reward
        terminated = self.terminated if terminated is None else terminated
        truncated = self.truncated if truncated is None else truncated
        # the kernel writes whole rows through these pointers: refuse a buffer it would overrun
        for t, dt, n, what in ((obs, torch.float32, self.num_agents * self.obs_dim, "obs"),
                               (reward, self.rdtype, self.num_envs, "reward"),
                               (terminated, torch.uint8, self.num_envs, "terminated"),
                               (truncated, torch.uint8, self.num_envs, "truncated")):
            if t.dtype != dt or not t.is_contiguous() or t.numel() < n or t.device != self.device:
                raise ValueError(f"{what} must be a contiguous {dt} tensor of >= {n} elements on {self.device}")
        if want_terminal and terminal_obs is None:
            terminal_obs = self.terminal_obs
        if want_reasons and reasons is None:
            reasons = self.reasons
        so = L.QsStepOut(L.ptr(obs), L.ptr(reward), L.ptr(terminated), L.ptr(truncated), L.ptr(terminal_obs),
                         L.ptr(reasons), L.ptr(actions_out))
        return so, StepResult(obs, reward, terminated, truncated, terminal_obs, reasons, actions_out)

    def _check_actions(self, actions):
        if (actions.dtype != torch.float32 or not actions.is_contiguous() or actions.device != self.device
                or actions.numel() != self.num_agents * self.act_dim):
            raise ValueError(f"actions must be a contiguous float32 ({self.num_envs},{self.num_drones},"
                             f"{self.act_dim}) tensor on {self.device}")

    def step_many(self, outs, actions=None):
        """len(outs) consecutive control steps, as `step(actions[j], **outs[j])` for
        each j, but several steps to a launch with the envs' state kept on-chip in
        between (the depth is QS_MAX_FUSED_STEPS at construction).  outs: one dict
        of step()'s output keywords per step.  actions: None for the synthetic
        random policy (qs_step_many), or the steps' actions (qs_step_seq) as a list
        of len(outs) (E, D, A) tensors or one (len(outs), E, D, A) tensor, whose
        slices are passed as they are (no copy).  Steps share a launch only while
        their output buffers are distinct and none of them reads as actions what
        another one writes; otherwise the launch is cut, so the result always
        equals the single steps'.  (A launch of the shape-specialised kernel also
        keeps the steps that write its buffer sets again in the same order: see
        `ring_counts`.)  Returns the steps' StepResults."""
        n = len(outs)
        acts = None
        if actions is not None:
            if isinstance(actions, torch.Tensor):
                if actions.dim() < 1 or actions.shape[0] != n:
                    raise ValueError(f"actions must hold {n} steps: ({n},{self.num_envs},{self.num_drones},{self.act_dim})")
                acts = [actions[j] for j in range(n)]
            else:
                acts = list(actions)
                if len(acts) != n:
                    raise ValueError(f"actions must hold {n} steps, one tensor each")
            for a in acts:
                if not isinstance(a, torch.Tensor):
                    raise ValueError("actions: every step needs its tensor (None for all of them draws the random policy)")
                self._check_actions(a)
        recs = [self._step_out(**kw) for kw in outs]
        arr = (L.QsStepOut * max(1, n))(*[so for so, _ in recs])
        if acts is None:
            L.check(self.lib.qs_step_many(self._h, n, arr, self._stream()), "qs_step_many")
        else:
            ptrs = (ctypes.c_void_p * max(1, n))(*[a.data_ptr() for a in acts])
            L.check(self.lib.qs_step_seq(self._h, n, ptrs, arr, self._stream()), "qs_step_seq")
        return [res for _, res in recs]

    # ------------------------------------------------------- branch rollouts
    def score_depth(self):
        """The longest candidate (in steps) one `score` call takes on this swarm
        (qs_score_depth); 0: this swarm cannot score (a layout whose reset draws
        can be rejected, or the Flock / Meetup / LeaderFollower tasks)."""
        return int(self.lib.qs_score_depth(self._h))

    _SCORE_OUTS = ("obs", "reward", "terminated", "truncated", "terminal_obs", "reasons", "actions_out")

    def score(self, actions, outs=None, *, ret=None, first_done=None, ret_agent=None, track=None, cost_agent=None,
              avoid=None):
        """Run C candidate action sequences of n steps each from the swarm's current
        state in one launch, and leave the swarm exactly as it was (qs_score): no
        state, history, episode log or counter changes.  Virtual env (c, e) starts
        from env e and follows candidate c; its per-step outputs are, bit for bit,
        what `step_many(outs, actions=actions[:, c])` would write from this state.

        actions: one (n, C, E, D, A) float32 tensor, whose slices are passed as they
        are (no copy), or a list of n (C, E, D, A) tensors (4-byte alignment will do;
        steps may share a tensor).  outs: None, or one dict of step()'s output
        keywords per step, each buffer stacked over the candidates (obs (C, E, D, O),
        reward (C, E), ...); an output that is not named is not written.  ret:
        (C, E) float64, the rewards of steps 0 .. the candidate's first done step
        (all n if none), summed in step order; first_done: (C, E) int32, that step,
        or n.  ret_agent: (C, E, D) float64, each drone's own terms of those rewards
        before the division by D, summed over the same steps (qs_score_agents): ret
        is about ret_agent.sum(-1) / D.  At least one output must be named, none may
        overlap another or an action tensor, and 1 <= n <= score_depth().

        track, cost_agent: a `track_spec(...)` result and a (C, E, D) float64 tensor
        (both or neither): the same launch also sums each drone's tracking cost
        against the spec's reference over the same steps (qs_track_score); every
        other output is the bytes it is without.

        avoid: an `avoid_spec(...)` result, with cost_agent and with or without
        track: cost_agent also holds the pairwise separation term among an env's
        drones and the terms of the spec's obstacle table (qs_avoid_score)."""
        E, D, A, O = self.num_envs, self.num_drones, self.act_dim, self.obs_dim
        if isinstance(actions, torch.Tensor):
            if actions.dim() != 5:
                raise ValueError(f"actions must be (n, C, {E}, {D}, {A}) or a list of (C, {E}, {D}, {A}) tensors")
            acts = [actions[j] for j in range(actions.shape[0])]
        else:
            acts = list(actions)
        n = len(acts)
        if n < 1 or not isinstance(acts[0], torch.Tensor) or acts[0].dim() != 4:
            raise ValueError(f"actions must hold at least one step of shape (C, {E}, {D}, {A})")
        C = acts[0].shape[0]
        for a in acts:
            if (not isinstance(a, torch.Tensor) or a.dtype != torch.float32 or not a.is_contiguous()
                    or a.device != self.device or tuple(a.shape) != (C, E, D, A)):
                raise ValueError(f"actions: every step must be a contiguous float32 ({C},{E},{D},{A}) tensor on {self.device}")
        want = dict(obs=(torch.float32, C * E * D * O), reward=(self.rdtype, C * E), terminated=(torch.uint8, C * E),
                    truncated=(torch.uint8, C * E), terminal_obs=(torch.float32, C * E * D * O),
                    reasons=(torch.uint8, C * E * D), actions_out=(torch.float32, C * E * D * A),
                    ret=(torch.float64, C * E), first_done=(torch.int32, C * E), ret_agent=(torch.float64, C * E * D),
                    cost_agent=(torch.float64, C * E * D))

        def buf(t, what):
            if t is None:
                return None
            dt, numel = want[what]
            if (not isinstance(t, torch.Tensor) or t.dtype != dt or not t.is_contiguous() or t.numel() < numel
                    or t.device != self.device):
                raise ValueError(f"{what} must be a contiguous {dt} tensor of >= {numel} elements on {self.device}")
            return L.ptr(t)

        arr = None
        if outs is not None:
            if len(outs) != n:
                raise ValueError(f"outs must hold {n} steps, one dict each")
            recs = []
            for kw in outs:
                unknown = set(kw) - set(self._SCORE_OUTS)
                if unknown:
                    raise ValueError(f"outs: unknown output {sorted(unknown)}")
                recs.append(L.QsStepOut(*[buf(kw.get(k), k) for k in self._SCORE_OUTS]))
            arr = (L.QsStepOut * n)(*recs)
        so = None
        if ret is not None or first_done is not None:
            so = ctypes.byref(L.QsScoreOut(buf(ret, "ret"), buf(first_done, "first_done")))
        ptrs = (ctypes.c_void_p * n)(*[a.data_ptr() for a in acts])
        if avoid is not None:
            if cost_agent is None:
                raise ValueError("avoid and cost_agent go together")
            if not hasattr(self.lib, "qs_avoid_score"):
                raise L.QuadSwarmError(f"{L.LIB_PATH} has no qs_avoid_score: rebuild the HIP extension")
            tspec = ctypes.byref(_check_track(self, track)) if track is not None else None
            aspec = _check_avoid(self, avoid)
            L.check(self.lib.qs_avoid_score(self._h, n, C, ptrs, arr, so, buf(ret_agent, "ret_agent"), tspec,
                                            ctypes.byref(aspec), buf(cost_agent, "cost_agent"), self._stream()),
                    "qs_avoid_score")
            return
        if (track is None) != (cost_agent is None):
            raise ValueError("track and cost_agent go together")
        if track is not None:
            if not hasattr(self.lib, "qs_track_score"):
                raise L.QuadSwarmError(f"{L.LIB_PATH} has no qs_track_score: rebuild the HIP extension")
            spec = _check_track(self, track)
            L.check(self.lib.qs_track_score(self._h, n, C, ptrs, arr, so, buf(ret_agent, "ret_agent"), ctypes.byref(spec),
                                            buf(cost_agent, "cost_agent"), self._stream()), "qs_track_score")
            return
        if ret_agent is None:
            L.check(self.lib.qs_score(self._h, n, C, ptrs, arr, so, self._stream()), "qs_score")
            return
        if not hasattr(self.lib, "qs_score_agents"):
            raise L.QuadSwarmError(f"{L.LIB_PATH} has no qs_score_agents: rebuild the HIP extension")
        L.check(self.lib.qs_score_agents(self._h, n, C, ptrs, arr, so, buf(ret_agent, "ret_agent"), self._stream()),
                "qs_score_agents")

    def branches(self, C):
        """A `BranchSet` of C candidates on this swarm (qs_branch_create): the state
        of C · E virtual envs kept on the device, so that branch rollouts can be
        chained past score_depth(), forked from the swarm again and resampled."""
        if not hasattr(self.lib, "qs_branch_create"):
            raise L.QuadSwarmError(f"{L.LIB_PATH} has no qs_branch_create: rebuild the HIP extension")
        bs = BranchSet(self, C)
        self.__dict__.setdefault("_planners", weakref.WeakSet()).add(bs)   # close() ends them first
        return bs

    def mppi(self, horizon, candidates, sigma, lo=-1.0, hi=1.0, lam=1.0, done_penalty=0.0, seed=0, per_drone=False):
        """An `MPPIPlanner` on this swarm (qs_mppi_create): `candidates` action
        sequences of `horizon` steps (1 .. score_depth()) are drawn round a nominal
        one with per-component noise `sigma` (a number or one per action component),
        clipped to [lo, hi], scored from the swarm's current state and folded back
        by their softmax weights at temperature `lam` (0: the best one wins);
        `done_penalty` is taken off a candidate that ends an episode.  per_drone=True
        (qs_pd_mppi_create): every drone weighs the candidates by its own return
        (`MPPIPlanner`)."""
        planner = MPPIPlanner(self, horizon, candidates, sigma, lo, hi, lam, done_penalty, seed, per_drone)
        self.__dict__.setdefault("_planners", weakref.WeakSet()).add(planner)   # close() ends them first
        return planner

    def cem(self, horizon, candidates, elites, sigma, iterations=3, lo=-1.0, hi=1.0, alpha=0.0, sigma_min=0.0,
            done_penalty=0.0, seed=0, per_drone=False):
        """A `CEMPlanner` on this swarm (qs_cem_create): per tick and env,
        `iterations` rounds of drawing `candidates` action sequences of `horizon`
        steps (1 .. score_depth()) round a mean with a per-element spread (started
        from `sigma` at every tick: a number or one per action component), clipped
        to [lo, hi], scoring them from the swarm's current state and refitting mean
        and spread to the `elites` best, smoothed by `alpha` and floored at
        `sigma_min`; `done_penalty` is taken off a candidate that ends an episode.
        per_drone=True (qs_pd_cem_create): every drone ranks the candidates by its own
        return (`CEMPlanner`)."""
        planner = CEMPlanner(self, horizon, candidates, elites, sigma, iterations, lo, hi, alpha, sigma_min,
                             done_penalty, seed, per_drone)
        self.__dict__.setdefault("_planners", weakref.WeakSet()).add(planner)   # close() ends them first
        return planner

    def smc(self, horizon, particles, sigma, segment=None, lo=-1.0, hi=1.0, lam=1.0, done_penalty=0.0, ess_frac=0.5,
            seed=0):
        """An `SMCPlanner` on this swarm (qs_smc_create): `particles` branch rollouts
        of `horizon` steps (any length: it is run in segments of `segment` steps,
        1 .. score_depth(), by default min(horizon, score_depth())) forked from the
        swarm's current state.  Each segment draws actions round the nominal with
        per-component noise `sigma`, clipped to [lo, hi], advances the particles and
        weighs them at temperature `lam`; an env whose effective sample size falls
        below `ess_frac` * particles is resampled systematically (0: never, which
        makes the tick a long-horizon MPPI tick).  The surviving particles' action
        sequences are folded back into the nominal by their weights; `done_penalty`
        is taken off a particle that ends an episode."""
        if not hasattr(self.lib, "qs_smc_create"):
            raise L.QuadSwarmError(f"{L.LIB_PATH} has no qs_smc_create: rebuild the HIP extension")
        planner = SMCPlanner(self, horizon, particles, sigma, segment, lo, hi, lam, done_penalty, ess_frac, seed)
        self.__dict__.setdefault("_planners", weakref.WeakSet()).add(planner)   # close() ends them first
        return planner

    def launch_counts(self):
        """(general, hot): the multi-step launches made so far on the general kernel
        instances and on the shape-specialised one (qs_launch_counts; QS_HOT_SHAPE=0
        at construction keeps every launch on the general ones)."""
        out = (ctypes.c_int64 * 2)()
        L.check(self.lib.qs_launch_counts(self._h, out), "qs_launch_counts")
        return int(out[0]), int(out[1])

    def ring_counts(self):
        """(launches, steps): the ring launches made so far and the control steps they
        held (qs_ring_counts): hot-shape launches that went on past their distinct
        output sets because the further steps wrote those sets again in order
        (QS_RING_LAUNCH=0 at construction cuts them as before)."""
        n, k = ctypes.c_int64(0), ctypes.c_int64(0)
        L.check(self.lib.qs_ring_counts(self._h, ctypes.byref(n), ctypes.byref(k)), "qs_ring_counts")
        return int(n.value), int(k.value)

    # ------------------------------------------------------------ state I/O
    def _state_buf(self, block):
        kw = dict(device=self.device)
        if block == L.STATE_AGENT:
            return torch.zeros((L.AGENT_FIELDS, self.num_agents), dtype=self.rdtype, **kw)
        if block == L.STATE_ENV:
            return torch.zeros((L.ENV_FIELDS, self.num_envs), dtype=torch.int32, **kw)
        if block == L.STATE_HISTORY:
            return torch.zeros((self.hist_len, self.num_agents, self.act_dim), dtype=torch.float32, **kw)
        if block == L.STATE_EP_RETURN:
            return torch.zeros(self.num_envs, dtype=torch.float64, **kw)
        raise ValueError(block)

    def get_state(self, block=L.STATE_AGENT) -> torch.Tensor:
        buf = self._state_buf(block)
        L.check(self.lib.qs_state_io(self._h, block, L.ptr(buf), 0, self._stream()), "qs_state_io(get)")
        return buf

    def set_state(self, block, value):
        buf = self._state_buf(block)
        buf.copy_(torch.as_tensor(value).reshape(buf.shape).to(buf.dtype))
        L.check(self.lib.qs_state_io(self._h, block, L.ptr(buf), 1, self._stream()), "qs_state_io(set)")
        torch.cuda.current_stream(self.device).synchronize()

    def episode_log(self, cap=1 << 16):
        """(records ndarray[EPISODE_DTYPE] of the most recent ≤cap completed episodes, total ever)."""
        dst = torch.empty(max(cap, 1) * L.EPISODE_DTYPE.itemsize, dtype=torch.uint8, device=self.device)
        total, written = ctypes.c_int64(0), ctypes.c_int64(0)
        L.check(self.lib.qs_episode_log(self._h, L.ptr(dst) if cap > 0 else None, cap, ctypes.byref(total),
                                        ctypes.byref(written), self._stream()), "qs_episode_log")
        n = written.value   # fewer than min(total, cap) when rings dropped episodes
        recs = dst[: n * L.EPISODE_DTYPE.itemsize].cpu().numpy().view(L.EPISODE_DTYPE)
        order = np.lexsort((recs["env"], recs["seq"]))   # the reference's env-loop order per step
        return recs[order], total.value

    def reset_error(self):
        v = ctypes.c_int(0)
        L.check(self.lib.qs_reset_error(self._h, ctypes.byref(v)), "qs_reset_error")
        return v.value


class _DeviceSpan:
    """A span of the planner's device memory, as `torch.as_tensor` reads it
    (__cuda_array_interface__ version 2): the tensor views the memory, no copy."""

    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False),
                                         "version": 2, "strides": None}


class BranchSet:
    """Persistent branch rollouts on a swarm (qs_branch_*, include/quadswarm.h).

    The set owns the state of C · E virtual envs (candidate c of env e).  `fork()`
    makes every candidate of env e a copy of the swarm's env e as it is at that
    point of the stream; `advance(actions, outs)` runs 1 .. score_depth() steps of
    every candidate in one launch, from the set's state and back into it;
    `rollout(actions, outs)` takes any number of steps and chains `advance` in
    chunks of at most score_depth(); `select(parent)` makes candidate c of env e a
    copy of the old candidate parent[c, e] of that env (a value outside 0 .. C-1
    keeps it).  The swarm itself is never changed.  Every call is stream-ordered
    with no host sync and may be captured into a graph (with the fork its advances
    follow: a captured advance carries the step index of its capture).

    `ret` (C, E) float64, `first_done` (C, E) int32 and `ret_agent` (C, E, D)
    float64 are torch tensors over the set's own device memory (no copies; they
    dangle after `close()`), accumulated since the last fork as `QuadSwarm.score`
    forms them: an env's rewards count up to its first done step, whose index
    since the fork `first_done` holds (`steps` while there is none).  `steps`: the
    steps advanced since the last fork.  The swarm must outlive the set."""

    def __init__(self, swarm, C):
        self.swarm, self.lib, self.num_candidates = swarm, swarm.lib, int(C)
        self._p = ctypes.c_void_p()
        with torch.cuda.device(swarm.device):
            L.check(self.lib.qs_branch_create(swarm._h, self.num_candidates, ctypes.byref(self._p)), "qs_branch_create")
        bufs = L.QsBranchBufs()
        L.check(self.lib.qs_branch_buffers(self._p, ctypes.byref(bufs)), "qs_branch_buffers")
        C, E, D = self.num_candidates, swarm.num_envs, swarm.num_drones
        for name, shape, typestr in (("ret", (C, E), "<f8"), ("first_done", (C, E), "<i4"), ("ret_agent", (C, E, D), "<f8")):
            setattr(self, name, torch.as_tensor(_DeviceSpan(getattr(bufs, name), shape, typestr), device=swarm.device))

    def _stream(self):
        return self.swarm._stream()

    @property
    def steps(self):
        v = ctypes.c_int64(0)
        L.check(self.lib.qs_branch_steps(self._p, ctypes.byref(v)), "qs_branch_steps")
        return int(v.value)

    def fork(self):
        L.check(self.lib.qs_branch_fork(self._p, self._stream()), "qs_branch_fork")

    def _steps_of(self, actions):
        sw, C = self.swarm, self.num_candidates
        shape = (C, sw.num_envs, sw.num_drones, sw.act_dim)
        if isinstance(actions, torch.Tensor):
            if actions.dim() != 5:
                raise ValueError(f"actions must be (n,) + {shape} or a list of {shape} tensors")
            acts = [actions[j] for j in range(actions.shape[0])]
        else:
            acts = list(actions)
        if len(acts) < 1:
            raise ValueError(f"actions must hold at least one step of shape {shape}")
        for a in acts:
            if (not isinstance(a, torch.Tensor) or a.dtype != torch.float32 or not a.is_contiguous()
                    or a.device != sw.device or tuple(a.shape) != shape):
                raise ValueError(f"actions: every step must be a contiguous float32 {shape} tensor on {sw.device}")
        return acts

    def _outs_of(self, outs, n):
        if outs is None:
            return None
        sw, C = self.swarm, self.num_candidates
        E, D, A, O = sw.num_envs, sw.num_drones, sw.act_dim, sw.obs_dim
        want = dict(obs=(torch.float32, C * E * D * O), reward=(sw.rdtype, C * E), terminated=(torch.uint8, C * E),
                    truncated=(torch.uint8, C * E), terminal_obs=(torch.float32, C * E * D * O),
                    reasons=(torch.uint8, C * E * D), actions_out=(torch.float32, C * E * D * A))
        if len(outs) != n:
            raise ValueError(f"outs must hold {n} steps, one dict each")
        recs = []
        for kw in outs:
            unknown = set(kw) - set(want)
            if unknown:
                raise ValueError(f"outs: unknown output {sorted(unknown)}")
            ptrs = []
            for k in QuadSwarm._SCORE_OUTS:
                t = kw.get(k)
                if t is not None:
                    dt, numel = want[k]
                    if (not isinstance(t, torch.Tensor) or t.dtype != dt or not t.is_contiguous() or t.numel() < numel
                            or t.device != sw.device):
                        raise ValueError(f"{k} must be a contiguous {dt} tensor of >= {numel} elements on {sw.device}")
                ptrs.append(L.ptr(t))
            recs.append(L.QsStepOut(*ptrs))
        return recs

    def _advance(self, acts, recs):
        n = len(acts)
        ptrs = (ctypes.c_void_p * n)(*[a.data_ptr() for a in acts])
        arr = None if recs is None else (L.QsStepOut * n)(*recs)
        L.check(self.lib.qs_branch_advance(self._p, n, ptrs, arr, self._stream()), "qs_branch_advance")

    def advance(self, actions, outs=None):
        """n = len(actions) steps, 1 <= n <= score_depth(), in one launch.  actions: one
        (n, C, E, D, A) float32 tensor, whose slices are passed as they are (no copy),
        or a list of n (C, E, D, A) tensors; outs: None, or one dict of step()'s
        output keywords per step, each buffer stacked over the candidates as in
        `QuadSwarm.score`."""
        acts = self._steps_of(actions)
        self._advance(acts, self._outs_of(outs, len(acts)))

    def rollout(self, actions, outs=None):
        """`advance` for any n >= 1: the steps are cut into launches of at most
        score_depth() steps, in order."""
        acts = self._steps_of(actions)
        recs = self._outs_of(outs, len(acts))
        depth = self.swarm.score_depth()
        for j in range(0, len(acts), depth):
            self._advance(acts[j:j + depth], None if recs is None else recs[j:j + depth])

    def select(self, parent):
        """parent: (C, E) int32 on the device."""
        sw = self.swarm
        if (not isinstance(parent, torch.Tensor) or parent.dtype != torch.int32 or not parent.is_contiguous()
                or parent.device != sw.device or tuple(parent.shape) != (self.num_candidates, sw.num_envs)):
            raise ValueError(f"parent must be a contiguous int32 ({self.num_candidates},{sw.num_envs}) tensor on {sw.device}")
        L.check(self.lib.qs_branch_select(self._p, L.ptr(parent), self._stream()), "qs_branch_select")

    def get_state(self, block=L.STATE_AGENT) -> torch.Tensor:
        """The set's copy of a state block, stacked over the candidates: STATE_AGENT
        (fields, C, E · D), STATE_ENV (4, C, E) or STATE_HISTORY (H, C, E · D, A)."""
        sw, C = self.swarm, self.num_candidates
        kw = dict(device=sw.device)
        if block == L.STATE_AGENT:
            buf = torch.zeros((L.AGENT_FIELDS, C, sw.num_agents), dtype=sw.rdtype, **kw)
        elif block == L.STATE_ENV:
            buf = torch.zeros((L.ENV_FIELDS, C, sw.num_envs), dtype=torch.int32, **kw)
        elif block == L.STATE_HISTORY:
            buf = torch.zeros((sw.hist_len, C, sw.num_agents, sw.act_dim), dtype=torch.float32, **kw)
        else:
            raise ValueError(block)
        L.check(self.lib.qs_branch_state(self._p, block, L.ptr(buf), self._stream()), "qs_branch_state")
        return buf

    def close(self):
        if getattr(self, "_p", None):
            torch.cuda.synchronize(self.swarm.device)
            self.lib.qs_branch_destroy(self._p)
            self._p = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _BranchView(BranchSet):
    """A branch set that another object owns (`SMCPlanner.set`): the accumulators,
    `steps` and `get_state` for reading; `close()` only lets go of it."""

    def __init__(self, swarm, C, p):
        self.swarm, self.lib, self.num_candidates = swarm, swarm.lib, int(C)
        self._p = p
        bufs = L.QsBranchBufs()
        L.check(self.lib.qs_branch_buffers(self._p, ctypes.byref(bufs)), "qs_branch_buffers")
        E, D = swarm.num_envs, swarm.num_drones
        for name, shape, typestr in (("ret", (C, E), "<f8"), ("first_done", (C, E), "<i4"), ("ret_agent", (C, E, D), "<f8")):
            setattr(self, name, torch.as_tensor(_DeviceSpan(getattr(bufs, name), shape, typestr), device=swarm.device))

    def close(self):
        self._p = ctypes.c_void_p()


class _Planner:
    """What `MPPIPlanner`, `CEMPlanner` and `SMCPlanner` share: creation through the entry
    points `<_PREFIX>_*`, the device views, `plan`, `step_t` and `close`."""

    _PREFIX = None   # "qs_mppi" / "qs_cem"
    per_drone = False
    ret_agent = None   # per-drone mode: the (C, E, D) float64 view of the planner's ret_agent

    def _bind(self, swarm, per_drone=False):
        self.swarm, self.lib, self.per_drone = swarm, swarm.lib, bool(per_drone)
        self._create_fn = f"{self._PREFIX.replace('qs_', 'qs_pd_') if self.per_drone else self._PREFIX}_create"
        if not hasattr(self.lib, self._create_fn):
            raise L.QuadSwarmError(f"{L.LIB_PATH} has no {self._create_fn}: rebuild the HIP extension")

    def _units(self):
        """The leading shape of what is weighed on its own: (E,), or (E, D) in per-drone mode."""
        sw = self.swarm
        return (sw.num_envs, sw.num_drones) if self.per_drone else (sw.num_envs,)

    def _per_component(self, v, what):
        A = self.swarm.act_dim
        out = [float(v)] * A if np.isscalar(v) else [float(s) for s in v]
        if len(out) != A:
            raise ValueError(f"{what} must be a number or one per action component ({A})")
        return out

    def _call(self, name, *args):
        fn = f"{self._PREFIX}_{name}"
        L.check(getattr(self.lib, fn)(self._p, *args, self._stream()), fn)

    def _create(self, spec, bufs, views):
        """`<_PREFIX>_create(spec)`, then one attribute per (name, shape, typestr)
        of `views`: a tensor over that member of `bufs`."""
        swarm = self.swarm
        self.spec = spec
        self._p = ctypes.c_void_p()
        self._stepper = swarm.step   # what step_t runs the action with (SwarmVecEnv.mppi / .cem: its step_t)
        with torch.cuda.device(swarm.device):
            L.check(getattr(self.lib, self._create_fn)(swarm._h, ctypes.byref(spec), ctypes.byref(self._p)), self._create_fn)
        L.check(getattr(self.lib, f"{self._PREFIX}_buffers")(self._p, ctypes.byref(bufs)), f"{self._PREFIX}_buffers")
        for name, shape, typestr in views:
            setattr(self, name, torch.as_tensor(_DeviceSpan(getattr(bufs, name), shape, typestr), device=swarm.device))
        if self.per_drone:
            fn, ra = self._create_fn.replace("_create", "_ret_agent"), ctypes.c_void_p()
            L.check(getattr(self.lib, fn)(self._p, ctypes.byref(ra)), fn)
            shape = (spec.candidates, swarm.num_envs, swarm.num_drones)
            self.ret_agent = torch.as_tensor(_DeviceSpan(ra.value, shape, "<f8"), device=swarm.device)

    def _stream(self):
        return self.swarm._stream()

    def _reset(self, seq, name):
        """`<_PREFIX>_reset` with `seq` (None: zeros) for the buffer `name`."""
        if seq is not None:
            shape = tuple(getattr(self, name).shape)
            if (not isinstance(seq, torch.Tensor) or seq.dtype != torch.float32 or not seq.is_contiguous()
                    or seq.device != self.swarm.device or tuple(seq.shape) != shape):
                raise ValueError(f"{name} must be a contiguous float32 {shape} tensor on {self.swarm.device}")
        self._call("reset", L.ptr(seq))

    def plan(self):
        """One planner tick from the swarm's current state; returns `action`."""
        self._call("plan")
        return self.action

    def step_t(self, **bufs):
        """One receding-horizon tick: `plan()`, then the control step that runs
        `action` (the swarm's `step`, or `SwarmVecEnv.step_t`), with its return."""
        self.plan()
        return self._stepper(self.action, **bufs)

    def close(self):
        if getattr(self, "_p", None):
            torch.cuda.synchronize(self.swarm.device)
            getattr(self.lib, f"{self._PREFIX}_destroy")(self._p)
            self._p = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def value_spec(critic=None, gamma=1.0, scale=1.0, obs_normalizer=None, device=None):
    """The `QsValueSpec` of a value tail (include/quadswarm.h qs_value_spec) and the
    tensors it points into, which the caller keeps alive as long as the spec is used.

    critic: None (discount only), a `CentralizedCritic`, an `MLP` with two hidden
    layers, tanh and one output, or the six tensors (w1, b1, w2, b2, w3, b3) in
    nn.Linear's layout.  obs_normalizer: a `MeanStdNormalizer`, whose `rms.mean` /
    `rms.var` (float64), `clip` and `epsilon` are used.  Every tensor must be
    contiguous, of the right dtype and on `device`; nothing is copied, so a critic
    that training updates in place is read as it is at every launch."""
    spec, keep = L.QsValueSpec(), []
    spec.gamma, spec.scale = float(gamma), float(scale)

    def dev_ptr(t, dtype, what):
        if (not isinstance(t, torch.Tensor) or t.dtype != dtype or not t.is_contiguous() or not t.is_cuda
                or (device is not None and t.device != device)):
            raise ValueError(f"{what} must be a contiguous {dtype} tensor on {device if device is not None else 'the GPU'}")
        keep.append(t)
        return t.data_ptr()

    if critic is not None:
        net = getattr(critic, "v_net", critic)
        if isinstance(net, (tuple, list)):
            if len(net) != 6:
                raise ValueError("critic: a tuple must hold the six tensors (w1, b1, w2, b2, w3, b3)")
            w1, b1, w2, b2, w3, b3 = net
        else:
            fcs = getattr(net, "fcs", None)
            if fcs is None or len(fcs) != 3 or not getattr(net, "_tanh3", False) or fcs[2].out_features != 1:
                raise ValueError("critic must be a CentralizedCritic, an MLP with two hidden layers, tanh and one "
                                 "output, or a tuple of six tensors")
            if getattr(critic, "include_actions", False):
                raise ValueError("critic: a critic that takes actions (include_actions) has no value of an obs alone")
            w1, b1, w2, b2, w3, b3 = (t.detach() for fc in fcs for t in (fc.weight, fc.bias))
        for t in (w1, b1, w2, b2, w3, b3):
            if not isinstance(t, torch.Tensor):
                raise ValueError("critic: the weights must be torch tensors")
        N, I = tuple(w1.shape) if w1.dim() == 2 else (0, 0)
        if (w1.dim() != 2 or tuple(b1.shape) != (N,) or tuple(w2.shape) != (N, N) or tuple(b2.shape) != (N,)
                or w3.numel() != N or w3.dim() not in (1, 2) or b3.numel() != 1):
            raise ValueError("critic: shapes must be w1 (N, I), b1 (N,), w2 (N, N), b2 (N,), w3 (1, N), b3 (1,)")
        spec.in_dim, spec.hidden = int(I), int(N)
        for name, t in zip(("w1", "b1", "w2", "b2", "w3", "b3"), (w1, b1, w2, b2, w3, b3)):
            setattr(spec, name, dev_ptr(t, torch.float32, f"critic {name}"))
    if obs_normalizer is not None:
        rms = obs_normalizer.rms
        mean, var = rms.mean.reshape(-1), rms.var.reshape(-1)   # (views: contiguous statistics stay shared)
        if critic is not None and mean.numel() != spec.in_dim:
            raise ValueError(f"obs_normalizer has {mean.numel()} columns, the critic takes {spec.in_dim}")
        spec.obs_mean, spec.obs_var = dev_ptr(mean, torch.float64, "obs_normalizer.rms.mean"), dev_ptr(
            var, torch.float64, "obs_normalizer.rms.var")
        spec.obs_eps, spec.obs_clip = float(obs_normalizer.epsilon), float(obs_normalizer.clip)
        keep.append(obs_normalizer)
    keep.append(critic)
    return spec, keep


class _ValueTail:
    """What `MPPIPlanner` and `CEMPlanner` add for discounted, critic-bootstrapped
    returns (qs_value_mppi_* / qs_value_cem_*: set, buffers, score; include/quadswarm.h)."""

    last_obs = value = rewards = None   # the views, while a value is attached and the buffer exists
    _value_keep = None

    def _need(self, name):
        fn = f"qs_value_{self._PREFIX[3:]}_{name}"
        if not hasattr(self.lib, fn):
            raise L.QuadSwarmError(f"{L.LIB_PATH} has no {fn}: rebuild the HIP extension")
        return fn

    def set_value(self, critic=None, gamma=1.0, scale=1.0, obs_normalizer=None):
        """Attach a value to the score stage: `ret` becomes the discounted rewards
        up to the candidate's first done step plus, where it was never done,
        gamma^n · scale · critic(last obs).  See `value_spec` for the arguments; the
        planner keeps the tensors alive.  Afterwards `last_obs` (C, E, D, O) float32
        and `value` (C, E) float32 (with a critic) and `rewards` (n, C, E) in the
        swarm's precision (with gamma != 1) view the planner's buffers; each is None
        where its buffer does not exist.  A host call: not to be captured.  A
        refusal (ValueError / QuadSwarmError) leaves the planner as it was."""
        sw = self.swarm
        spec, keep = value_spec(critic, gamma, scale, obs_normalizer, device=sw.device)
        fn = self._need("set")
        with torch.cuda.device(sw.device):
            L.check(getattr(self.lib, fn)(self._p, ctypes.byref(spec)), fn)
        self._value_keep = keep
        self._value_views()

    def clear_value(self):
        """Detach the value: the planner scores by the plain sum of rewards again."""
        fn = self._need("set")
        with torch.cuda.device(self.swarm.device):
            L.check(getattr(self.lib, fn)(self._p, None), fn)
        self._value_keep = None
        self._value_views()

    def _value_views(self):
        sw, fn = self.swarm, self._need("buffers")
        ptrs = [ctypes.c_void_p() for _ in range(3)]
        L.check(getattr(self.lib, fn)(self._p, *[ctypes.byref(p) for p in ptrs]), fn)
        n, C, E, D, O = self.horizon, self.num_candidates, sw.num_envs, sw.num_drones, sw.obs_dim
        shapes = (("last_obs", (C, E, D, O), "<f4"), ("value", (C, E), "<f4"),
                  ("rewards", (n, C, E), "<f8" if sw.rdtype == torch.float64 else "<f4"))
        for p, (name, shape, typestr) in zip(ptrs, shapes):
            setattr(self, name, torch.as_tensor(_DeviceSpan(p.value, shape, typestr), device=sw.device) if p.value else None)

    def score(self):
        """The scoring stage of `plan()` on its own: the candidates are run from the
        swarm's current state into `ret` / `first_done` (and, with a value attached,
        `last_obs`, `rewards`, `value` and the folded `ret`)."""
        fn = self._need("score")
        L.check(getattr(self.lib, fn)(self._p, self._stream()), fn)


def track_spec(ref, q, r=0.0, terminal=1.0, reward_scale=1.0, base=None):
    """The `QsTrackSpec` of a tracking cost (include/quadswarm.h qs_track_spec) and the
    tensors it points into, which the caller keeps alive as long as the spec is used.

    ref: (L, E, D, 12) float32 on the GPU, contiguous and 16-byte aligned: the reference
    of every drone's pos, rpy, vel and angular velocity, row by row.  base: None (every
    env reads row j at step j) or an (E,) int32 tensor on the same device, the row of
    step 0 for each env; step j reads row clamp(base + j, 0, L - 1).  Nothing is copied:
    `ref.copy_(...)`, `base.add_(1)` and `base[done] = 0` are seen by the next launch,
    also by the next replay of a captured one.  q: twelve state weights (or one number
    for all), r: the action weights (a number or up to four), terminal: the factor on
    the state part of the last step, reward_scale: the task reward's weight in the
    folded objective.  All finite; q, r and terminal >= 0 (the library refuses others)."""
    if (not isinstance(ref, torch.Tensor) or ref.dtype != torch.float32 or ref.dim() != 4 or ref.shape[-1] != 12
            or not ref.is_contiguous() or not ref.is_cuda or ref.shape[0] < 1):
        raise ValueError("ref must be a contiguous float32 (L, E, D, 12) tensor on the GPU")
    if ref.data_ptr() % 16 != 0:
        raise ValueError("ref must be 16-byte aligned")
    spec, keep = L.QsTrackSpec(), [ref]
    spec.ref, spec.L = ref.data_ptr(), int(ref.shape[0])
    if base is not None:
        if (not isinstance(base, torch.Tensor) or base.dtype != torch.int32 or not base.is_contiguous()
                or base.device != ref.device or tuple(base.shape) != (ref.shape[1],)):
            raise ValueError(f"base must be a contiguous int32 ({ref.shape[1]},) tensor on {ref.device}")
        spec.base = base.data_ptr()
        keep.append(base)
    qs = [float(q)] * 12 if np.isscalar(q) else [float(v) for v in q]
    if len(qs) != 12:
        raise ValueError("q must be a number or twelve (pos, rpy, vel, angular velocity)")
    rs = [float(r)] * 4 if np.isscalar(r) else [float(v) for v in r]
    if len(rs) > 4:
        raise ValueError("r must be a number or at most four (one per action component)")
    rs += [0.0] * (4 - len(rs))
    spec.q, spec.r = (ctypes.c_float * 12)(*qs), (ctypes.c_float * 4)(*rs)
    spec.terminal, spec.reward_scale = float(terminal), float(reward_scale)
    return spec, keep


def _check_track(swarm, track):
    """`track` as (spec, keep) from `track_spec`, held against the swarm's shape."""
    spec, keep = track
    ref = keep[0]
    if ref.device != swarm.device or tuple(ref.shape[1:3]) != (swarm.num_envs, swarm.num_drones):
        raise ValueError(f"track: ref must be (L, {swarm.num_envs}, {swarm.num_drones}, 12) on {swarm.device}")
    return spec


class _Tracking:
    """What `MPPIPlanner` and `CEMPlanner` add for a tracking cost (qs_track_mppi_* /
    qs_track_cem_*: set, buffers, score; include/quadswarm.h)."""

    cost_agent = None   # (C, E, D) float64, while a tracking spec is attached
    _track_keep = None

    def _track_fn(self, name):
        fn = f"qs_track_{self._PREFIX[3:]}_{name}"
        if not hasattr(self.lib, fn):
            raise L.QuadSwarmError(f"{L.LIB_PATH} has no {fn}: rebuild the HIP extension")
        return fn

    def set_tracking(self, ref, q, r=0.0, terminal=1.0, reward_scale=1.0, base=None):
        """Plan on a tracking objective: the score stage sums, per drone, the cost of
        `track_spec` inside the score launch and folds it, so `ret` becomes
        reward_scale · ret − mean_d cost and `ret_agent` reward_scale · ret_agent − cost;
        update, select and refit consume that unchanged.  Afterwards `cost_agent` and
        `ret_agent` (C, E, D) float64 view the planner's buffers.  The planner keeps
        the tensors alive and reads them at every launch.  A host call: not to be
        captured.  Refused next to a value tail; a refusal leaves the planner as it was."""
        sw = self.swarm
        track = track_spec(ref, q, r, terminal, reward_scale, base)
        spec, fn = _check_track(sw, track), self._track_fn("set")
        with torch.cuda.device(sw.device):
            L.check(getattr(self.lib, fn)(self._p, ctypes.byref(spec)), fn)
        self._track_keep = track
        self._track_views()

    def clear_tracking(self):
        """Detach the tracking spec: the planner scores by the task's reward again."""
        fn = self._track_fn("set")
        with torch.cuda.device(self.swarm.device):
            L.check(getattr(self.lib, fn)(self._p, None), fn)
        self._track_keep = None
        self._track_views()

    def _track_views(self):
        sw, fn = self.swarm, self._track_fn("buffers")
        cost, ra = ctypes.c_void_p(), ctypes.c_void_p()
        L.check(getattr(self.lib, fn)(self._p, ctypes.byref(cost), ctypes.byref(ra)), fn)
        shape = (self.num_candidates, sw.num_envs, sw.num_drones)
        self.cost_agent = torch.as_tensor(_DeviceSpan(cost.value, shape, "<f8"), device=sw.device) if cost.value else None
        if not self.per_drone:   # (a per-drone planner's ret_agent is its own, with or without tracking)
            self.ret_agent = torch.as_tensor(_DeviceSpan(ra.value, shape, "<f8"), device=sw.device) if ra.value else None

    def track(self):
        """The scoring stage of `plan()` on its own, as it runs with the attached
        tracking spec: `cost_agent` and the folded `ret` / `ret_agent` of the
        candidates from the swarm's current state (without a spec: the plain score)."""
        fn = self._track_fn("score")
        L.check(getattr(self.lib, fn)(self._p, self._stream()), fn)


def avoid_spec(obstacles=None, sep_radius=0.0, sep_weight=0.0, sep_z_scale=1.0):
    """The `QsAvoidSpec` of the separation and obstacle terms (include/quadswarm.h
    qs_avoid_spec) and the tensors it points into, which the caller keeps alive as long
    as the spec is used.

    obstacles: None (no obstacle term) or an (M, 8) float32 tensor on the GPU, M up to
    16, contiguous and 16-byte aligned, a row being centre (3), axis weights (3), radius,
    weight: the drone pays weight · max(0, radius² − Σ_k a_k (p_k − c_k)²)² a step.  Axis
    weights (1, 1, 1) make a sphere, (1, 1, 0) a vertical cylinder, (0, 0, 1) a slab such
    as a floor or a ceiling.  The table is shared by all envs and candidates; nothing is
    copied: `obstacles.copy_(...)` is seen by the next launch, also by the next replay of
    a captured one.  sep_radius, sep_weight, sep_z_scale: every other drone of the env
    closer than sep_radius (height differences times sep_z_scale) costs
    sep_weight · (sep_radius² − d²)² a step; a radius or weight of 0 switches the term
    off.  All finite and >= 0 (the library refuses others)."""
    spec, keep = L.QsAvoidSpec(), []
    if obstacles is not None:
        if (not isinstance(obstacles, torch.Tensor) or obstacles.dtype != torch.float32 or obstacles.dim() != 2
                or obstacles.shape[-1] != 8 or not obstacles.is_contiguous() or not obstacles.is_cuda):
            raise ValueError("obstacles must be a contiguous float32 (M, 8) tensor on the GPU")
        if obstacles.shape[0] > 0:
            if obstacles.data_ptr() % 16 != 0:
                raise ValueError("obstacles must be 16-byte aligned")
            spec.obstacles = obstacles.data_ptr()
        spec.M = int(obstacles.shape[0])
        keep.append(obstacles)
    spec.sep_radius, spec.sep_weight, spec.sep_z_scale = float(sep_radius), float(sep_weight), float(sep_z_scale)
    return spec, keep


def _check_avoid(swarm, avoid):
    """`avoid` as (spec, keep) from `avoid_spec`, held against the swarm's device."""
    spec, keep = avoid
    for t in keep:
        if t.device != swarm.device:
            raise ValueError(f"avoid: obstacles must be on {swarm.device}")
    return spec


class _Avoidance:
    """What `MPPIPlanner` and `CEMPlanner` add for the separation and obstacle terms
    (qs_avoid_mppi_* / qs_avoid_cem_*: set, buffers, score; include/quadswarm.h).  The
    spec attaches and detaches independently of a tracking spec (`_Tracking`), and the
    two share `cost_agent`, `ret_agent` and the score stage."""

    _avoid_keep = None

    def _avoid_fn(self, name):
        fn = f"qs_avoid_{self._PREFIX[3:]}_{name}"
        if not hasattr(self.lib, fn):
            raise L.QuadSwarmError(f"{L.LIB_PATH} has no {fn}: rebuild the HIP extension")
        return fn

    def set_avoidance(self, obstacles=None, sep_radius=0.0, sep_weight=0.0, sep_z_scale=1.0):
        """Plan with the terms of `avoid_spec` in the cost: the score stage sums them per
        drone inside the score launch, after the tracking cost where a tracking spec is
        attached too, and folds the cost as `set_tracking` describes (with reward_scale 1
        without a tracking spec).  A pair of drones counts for both, so an env-level
        planner sees a pair twice over D; a per-drone planner with a separation term
        optimises every drone against the others' candidate of the same index, the same
        kind of approximation as for downwash.  Afterwards `cost_agent` and `ret_agent`
        (C, E, D) float64 view the planner's buffers.  The planner keeps `obstacles`
        alive and reads it at every launch.  A host call: not to be captured.  Refused
        next to a value tail; a refusal leaves the planner as it was."""
        sw = self.swarm
        avoid = avoid_spec(obstacles, sep_radius, sep_weight, sep_z_scale)
        spec, fn = _check_avoid(sw, avoid), self._avoid_fn("set")
        with torch.cuda.device(sw.device):
            L.check(getattr(self.lib, fn)(self._p, ctypes.byref(spec)), fn)
        self._avoid_keep = avoid
        self._track_views()

    def clear_avoidance(self):
        """Detach the avoidance spec: the planner scores as it did without it (by the
        tracking objective, where a tracking spec is attached)."""
        fn = self._avoid_fn("set")
        with torch.cuda.device(self.swarm.device):
            L.check(getattr(self.lib, fn)(self._p, None), fn)
        self._avoid_keep = None
        self._track_views()

    def avoid(self):
        """The scoring stage of `plan()` on its own, as it runs with the attached specs:
        `cost_agent` and the folded `ret` / `ret_agent` of the candidates from the
        swarm's current state (with neither spec: the plain score)."""
        fn = self._avoid_fn("score")
        L.check(getattr(self.lib, fn)(self._p, self._stream()), fn)


def prior_spec(actor, count, obs, obs_normalizer=None, std_scale=1.0, device=None, action_scale=None):
    """The `QsPriorSpec` of a policy prior (include/quadswarm.h qs_prior_spec) and the
    tensors it points into, which the caller keeps alive as long as the spec is used.

    actor: an `MLPActor` (its `pi_net`, two hidden tanh layers, its `logstd` and
    `action_scale`), a `MAPPOActorCritic` (its `.actor`), or the seven tensors (w1, b1,
    w2, b2, w3, b3, logstd) in nn.Linear's layout with `action_scale` (default 1).
    count: the prior candidates per env.  obs: the contiguous (E, D, O) float32 obs of
    the swarm's current state.  obs_normalizer: the trainer's `MeanStdNormalizer` over
    an env's (D, O) obs, whose `rms.mean` / `rms.var` (float64), `clip` and `epsilon`
    are used.  std_scale multiplies exp(logstd) (0: every prior candidate is the
    mode).  Every tensor must be contiguous, of the right dtype and on `device`;
    nothing is copied, so an actor that training updates in place is read as it is
    at every launch."""
    spec, keep = L.QsPriorSpec(), []

    def dev_ptr(t, dtype, what):
        if (not isinstance(t, torch.Tensor) or t.dtype != dtype or not t.is_contiguous() or not t.is_cuda
                or (device is not None and t.device != device)):
            raise ValueError(f"{what} must be a contiguous {dtype} tensor on {device if device is not None else 'the GPU'}")
        keep.append(t)
        return t.data_ptr()

    net = getattr(actor, "actor", actor)
    if isinstance(net, (tuple, list)):
        if len(net) != 7:
            raise ValueError("actor: a tuple must hold the seven tensors (w1, b1, w2, b2, w3, b3, logstd)")
        w1, b1, w2, b2, w3, b3, logstd = net
        scale = 1.0 if action_scale is None else action_scale
    else:
        pi = getattr(net, "pi_net", None)
        fcs = getattr(pi, "fcs", None)
        if fcs is None or len(fcs) != 3 or not getattr(pi, "_tanh3", False) or not hasattr(net, "logstd"):
            raise ValueError("actor must be an MLPActor with two hidden tanh layers, a MAPPOActorCritic or a tuple of "
                             "seven tensors")
        w1, b1, w2, b2, w3, b3 = (t.detach() for fc in fcs for t in (fc.weight, fc.bias))
        logstd = net.logstd.detach()
        scale = net.action_scale if action_scale is None else action_scale
    for t in (w1, b1, w2, b2, w3, b3, logstd):
        if not isinstance(t, torch.Tensor):
            raise ValueError("actor: the weights must be torch tensors")
    N, I = tuple(w1.shape) if w1.dim() == 2 else (0, 0)
    A = w3.shape[0] if w3.dim() == 2 else 0
    if (w1.dim() != 2 or tuple(b1.shape) != (N,) or tuple(w2.shape) != (N, N) or tuple(b2.shape) != (N,)
            or tuple(w3.shape) != (A, N) or tuple(b3.shape) != (A,) or tuple(logstd.shape) != (A,)):
        raise ValueError("actor: shapes must be w1 (N, I), b1 (N,), w2 (N, N), b2 (N,), w3 (A, N), b3 (A,), logstd (A,)")
    spec.in_dim, spec.hidden, spec.act_dim, spec.count = int(I), int(N), int(A), int(count)
    for name, t in zip(("w1", "b1", "w2", "b2", "w3", "b3", "logstd"), (w1, b1, w2, b2, w3, b3, logstd)):
        setattr(spec, name, dev_ptr(t, torch.float32, f"actor {name}"))
    spec.action_scale, spec.std_scale = float(scale), float(std_scale)
    if not isinstance(obs, torch.Tensor) or obs.dim() != 3 or obs.shape[2] != I:
        raise ValueError(f"obs must be the (num_envs, num_drones, {I}) obs of the swarm's current state")
    spec.obs = dev_ptr(obs, torch.float32, "obs")
    if obs_normalizer is not None:
        rms = obs_normalizer.rms
        mean, var = rms.mean.reshape(-1), rms.var.reshape(-1)   # (views: contiguous statistics stay shared)
        if mean.numel() != obs.shape[1] * I or var.numel() != mean.numel():
            raise ValueError(f"obs_normalizer has {mean.numel()} entries, an env's obs {obs.shape[1]} x {I}")
        spec.obs_mean, spec.obs_var = dev_ptr(mean, torch.float64, "obs_normalizer.rms.mean"), dev_ptr(
            var, torch.float64, "obs_normalizer.rms.var")
        spec.obs_eps, spec.obs_clip = float(obs_normalizer.epsilon), float(obs_normalizer.clip)
        keep.append(obs_normalizer)
    keep.append(actor)
    return spec, keep


class _PolicyPrior:
    """What `MPPIPlanner` and `CEMPlanner`, env-level and per-drone alike, add for a
    policy prior (qs_prior_mppi_* / qs_prior_cem_*: set, buffers, rollout;
    include/quadswarm.h)."""

    prior_actions = prior_obs = None   # the views, while a prior is attached
    _prior_keep = None

    def _prior_fn(self, name):
        fn = f"qs_prior_{self._PREFIX[3:]}_{name}"
        if not hasattr(self.lib, fn):
            raise L.QuadSwarmError(f"{L.LIB_PATH} has no {fn}: rebuild the HIP extension")
        return fn

    def set_prior(self, actor, count, obs, obs_normalizer=None, std_scale=1.0, action_scale=None):
        """Make the last `count` candidates of every env closed-loop rollouts of
        `actor` from the swarm's current state: the first is the policy's mode,
        the others add std_scale · exp(logstd) noise, all clipped to [lo, hi].
        `obs` is the contiguous (E, D, O) float32 tensor that always holds the obs
        of the swarm's current state (the one passed as obs= to `step` / `step_t`);
        it is read at every tick and not copied.  See `prior_spec` for the other
        arguments; the planner keeps the tensors alive.  Afterwards `prior_actions`
        (n, count, E, D, A) and `prior_obs` (n, count, E, D, O) view the planner's
        buffers: slot j of `prior_obs` is the obs the actor saw at step j.  A host
        call: not to be captured.  A refusal (ValueError / QuadSwarmError) leaves
        the planner as it was."""
        sw = self.swarm
        spec, keep = prior_spec(actor, count, obs, obs_normalizer, std_scale, device=sw.device, action_scale=action_scale)
        if tuple(obs.shape) != (sw.num_envs, sw.num_drones, sw.obs_dim):
            raise ValueError(f"obs must be ({sw.num_envs}, {sw.num_drones}, {sw.obs_dim}), the swarm's obs")
        fn = self._prior_fn("set")
        with torch.cuda.device(sw.device):
            L.check(getattr(self.lib, fn)(self._p, ctypes.byref(spec)), fn)
        self._prior_keep = keep
        self._prior_views(int(count))

    def clear_prior(self):
        """Detach the prior: every candidate but the first is sampled again."""
        fn = self._prior_fn("set")
        with torch.cuda.device(self.swarm.device):
            L.check(getattr(self.lib, fn)(self._p, None), fn)
        self._prior_keep = None
        self._prior_views(0)

    def _prior_views(self, K):
        sw, fn = self.swarm, self._prior_fn("buffers")
        ptrs = [ctypes.c_void_p() for _ in range(2)]
        L.check(getattr(self.lib, fn)(self._p, *[ctypes.byref(p) for p in ptrs]), fn)
        n, E, D = self.horizon, sw.num_envs, sw.num_drones
        for p, name, last in zip(ptrs, ("prior_actions", "prior_obs"), (sw.act_dim, sw.obs_dim)):
            setattr(self, name,
                    torch.as_tensor(_DeviceSpan(p.value, (n, K, E, D, last), "<f4"), device=sw.device) if p.value else None)

    def prior(self):
        """The prior stage of `plan()` on its own: the actor's `count` closed-loop
        rollouts from the swarm's current state into `prior_actions` / `prior_obs`
        (2 · horizon launches, no host sync).  The next `sample()` copies them over
        the last `count` candidates."""
        fn = self._prior_fn("rollout")
        L.check(getattr(self.lib, fn)(self._p, self._stream()), fn)


class _Sampling:
    """What `MPPIPlanner`, `CEMPlanner` and `SMCPlanner` add for time-correlated noise and,
    on a CEM planner, an elite memory (qs_sampling_mppi_set / qs_sampling_cem_set /
    qs_sampling_smc_set, qs_sampling_cem_buffers; include/quadswarm.h)."""

    kept = kept_n = None   # CEM: the views, while a spec with keep > 0 is attached

    def _sampling_fn(self, name):
        fn = f"qs_sampling_{self._PREFIX[3:]}_{name}"
        if not hasattr(self.lib, fn):
            raise L.QuadSwarmError(f"{L.LIB_PATH} has no {fn}: rebuild the HIP extension")
        return fn

    def _sampling_set(self, spec):
        fn = self._sampling_fn("set")
        with torch.cuda.device(self.swarm.device):
            L.check(getattr(self.lib, fn)(self._p, None if spec is None else ctypes.byref(spec)), fn)
        self.kept = self.kept_n = None
        if self._PREFIX == "qs_cem":
            sw, fn = self.swarm, self._sampling_fn("buffers")
            kept, kept_n = ctypes.c_void_p(), ctypes.c_void_p()
            L.check(getattr(self.lib, fn)(self._p, ctypes.byref(kept), ctypes.byref(kept_n)), fn)
            if kept.value and kept_n.value:
                shape = (self.horizon, int(spec.keep), sw.num_envs, sw.num_drones, sw.act_dim)
                self.kept = torch.as_tensor(_DeviceSpan(kept.value, shape, "<f4"), device=sw.device)
                self.kept_n = torch.as_tensor(_DeviceSpan(kept_n.value, (1,), "<i4"), device=sw.device)

    def set_sampling(self, rho=0.0, keep=0):
        """Draw the candidates' noise as an AR(1) sequence along the steps: per action
        component eps_0 = xi_0, eps_j = rho · eps_{j-1} + sqrt(1 - rho²) · xi_j, xi the
        normals the planner draws anyway, so eps keeps unit variance and a candidate
        is a smooth deviation from the nominal / mean.  rho: a number or one per
        action component, each in [0, 1); a component with rho = 0 is drawn as before,
        byte for byte.  On an `SMCPlanner` the recurrence restarts at every segment
        (no noise state follows a particle through resampling), so segment = 1 makes
        rho a no-op.  keep (CEM only, 0 .. elites): the `keep` best candidates of
        every refit re-enter the next sample as candidates 1 .. keep, across
        iterations and, shifted by one step, across ticks; `kept` (n, keep, E, D, A)
        float32 and `kept_n` (1,) int32 then view the planner's buffers and are None
        otherwise.  A host call: not to be captured.  A refusal (ValueError /
        QuadSwarmError) leaves the planner, and an earlier spec, as they were."""
        spec = L.QsSamplingSpec()
        for a, r in enumerate(self._per_component(rho, "rho")):
            spec.rho[a] = r
        spec.keep = int(keep)
        self._sampling_set(spec)

    def clear_sampling(self):
        """Detach the sampling spec: independent noise at every step and no elite memory."""
        self._sampling_set(None)


class MPPIPlanner(_Avoidance, _Tracking, _Sampling, _PolicyPrior, _ValueTail, _Planner):
    """The native MPPI tick round `QuadSwarm.score` (qs_mppi_*, include/quadswarm.h).

    `sample()` draws `candidates` sequences round `nominal` (candidate 0 is the
    nominal itself), `update()` weighs them by the scores in `ret` / `first_done`,
    writes the weighted mean, shifted by one step, back to `nominal` and its first
    step to `action`; `plan()` is sample, score from the swarm's current state,
    update.  Every call is a few launches on the current stream with no host
    sync, and may be captured into a graph together with the `step` that runs
    `action`: the tick counter that keys the noise lives on the device.

    The buffers are torch tensors that view the planner's device memory (no
    copies; they dangle after `close()`): nominal (n, E, D, A), candidates
    (n, C, E, D, A), ret (C, E) float64, first_done (C, E) int32, weights (C, E)
    float64, best (E,) int32, action (E, D, A), tick (1,) (the uint64 counter,
    viewed as int64).  The swarm must outlive the planner.

    per_drone=True (qs_pd_mppi_create): every drone weighs the candidates by its
    own return, `ret_agent` (C, E, D) float64, less `done_penalty` where its env
    ends; weights is then (C, E, D) and best (E, D), and with lam = 0 each drone
    copies its own best candidate's slice.  ret is about ret_agent.sum(-1) / D, so
    a per-drone `lam` or `done_penalty` is on a scale D times the env-level one;
    with downwash or contacts a drone's return also depends on the others'
    actions and the factored weighting is an approximation.

    `set_value(critic, gamma, scale, obs_normalizer)` (env-level planners only)
    makes `ret` the discounted return bootstrapped with the trainer's critic
    behind the horizon, in one more launch after the score launch; `score()` is
    that stage on its own and `clear_value()` undoes it (`_ValueTail`).

    `set_prior(actor, count, obs, obs_normalizer, std_scale)` makes the last
    `count` candidates closed-loop rollouts of the trainer's actor, which
    `plan()` forms before it samples (2 · horizon launches more); `prior()` is
    that stage on its own, `prior_actions` / `prior_obs` its results and
    `clear_prior()` undoes it (`_PolicyPrior`).

    `set_sampling(rho)` makes the noise of every candidate an AR(1) sequence along
    the steps, in the same number of launches; `clear_sampling()` undoes it
    (`_Sampling`).

    `set_tracking(ref, q, r, terminal, reward_scale, base)` makes the objective a
    quadratic tracking cost against a reference, summed inside the score launch
    and folded into `ret` / `ret_agent` by one more launch; `track()` is that stage
    on its own, `cost_agent` its result and `clear_tracking()` undoes it
    (`_Tracking`; not together with `set_value`).

    `set_avoidance(obstacles, sep_radius, sep_weight, sep_z_scale)` adds a pairwise
    separation term among an env's drones and the terms of an obstacle table to that
    cost, with or without tracking; `avoid()` is the stage on its own and
    `clear_avoidance()` undoes it (`_Avoidance`; not together with `set_value`)."""

    _PREFIX = "qs_mppi"

    def __init__(self, swarm, horizon, candidates, sigma, lo=-1.0, hi=1.0, lam=1.0, done_penalty=0.0, seed=0,
                 per_drone=False):
        self._bind(swarm, per_drone)
        sig = self._per_component(sigma, "sigma")
        spec = L.QsMppiSpec()
        spec.horizon, spec.candidates = int(horizon), int(candidates)
        for a, s in enumerate(sig):
            spec.sigma[a] = s
        spec.lo, spec.hi, spec.lambda_, spec.done_penalty = float(lo), float(hi), float(lam), float(done_penalty)
        spec.seed = int(seed)
        self.horizon, self.num_candidates = int(horizon), int(candidates)
        n, C, E, D, A = self.horizon, self.num_candidates, swarm.num_envs, swarm.num_drones, swarm.act_dim
        self._create(spec, L.QsMppiBufs(), (
            ("nominal", (n, E, D, A), "<f4"), ("candidates", (n, C, E, D, A), "<f4"), ("ret", (C, E), "<f8"),
            ("first_done", (C, E), "<i4"), ("weights", (C,) + self._units(), "<f8"), ("best", self._units(), "<i4"),
            ("action", (E, D, A), "<f4"), ("tick", (1,), "<i8")))

    def reset(self, nominal=None):
        """Set the nominal sequence ((n, E, D, A) float32 on the device; None: zeros) and tick = 0."""
        self._reset(nominal, "nominal")

    def sample(self):
        self._call("sample")

    def update(self):
        self._call("update")


class CEMPlanner(_Avoidance, _Tracking, _Sampling, _PolicyPrior, _ValueTail, _Planner):
    """The native CEM tick round `QuadSwarm.score` (qs_cem_*, include/quadswarm.h).

    `begin()` restarts the spread `std` at sigma; `sample(i)` draws `candidates`
    sequences round `mean` with spread `std` (candidate 0 is the mean itself);
    `refit(i)` ranks them by the scores in `ret` / `first_done`, writes the
    `elites` best in rank order and refits `mean` and `std` to them; `finish()`
    takes `mean[0]` as `action` and shifts the mean by one step.  `plan()` is
    begin, `iterations` times (sample, score from the swarm's current state,
    refit), finish.  Every call is a few launches on the current stream with no
    host sync, and may be captured into a graph together with the `step` that
    runs `action`: the tick counter that keys the noise lives on the device.

    The buffers are torch tensors that view the planner's device memory (no
    copies; they dangle after `close()`): mean and std (n, E, D, A), candidates
    (n, C, E, D, A), ret (C, E) float64, first_done (C, E) int32, elites (K, E)
    int32, iter_best (I, E) float64, action (E, D, A), tick (1,) (the uint64
    counter, viewed as int64).  The swarm must outlive the planner.

    per_drone=True (qs_pd_cem_create): every drone ranks the candidates by its own
    return, `ret_agent` (C, E, D) float64, less `done_penalty` where its env ends,
    and refits its own A components; elites is then (K, E, D) and iter_best
    (I, E, D).  The scale and the caveat are `MPPIPlanner`'s.

    `set_value`, `score()` and `clear_value()` are `MPPIPlanner`'s: with a value
    attached every iteration's scoring is followed by the value tail.
    `set_prior`, `prior()` and `clear_prior()` are `MPPIPlanner`'s too: the prior
    stage runs once per tick, after `begin()`, and every iteration's `sample(i)`
    ends with the actor's rollouts as its last `count` candidates.

    `set_sampling(rho, keep)` makes the noise an AR(1) sequence along the steps
    and, with keep > 0, keeps the `keep` best candidates of every refit in `kept`
    (n, keep, E, D, A): they re-enter the next sample as candidates 1 .. keep
    (`kept_n` (1,) int32 says how many: 0 until the first refit after a reset), and
    `finish()` shifts them by one step with the mean, so a good sequence found once
    is not lost to resampling.  `clear_sampling()` undoes it (`_Sampling`).

    `set_tracking(...)` and `set_avoidance(...)` set the objective as they do for
    `MPPIPlanner` (`_Tracking`, `_Avoidance`)."""

    _PREFIX = "qs_cem"

    def __init__(self, swarm, horizon, candidates, elites, sigma, iterations=3, lo=-1.0, hi=1.0, alpha=0.0,
                 sigma_min=0.0, done_penalty=0.0, seed=0, per_drone=False):
        self._bind(swarm, per_drone)
        sig, smin = self._per_component(sigma, "sigma"), self._per_component(sigma_min, "sigma_min")
        spec = L.QsCemSpec()
        spec.horizon, spec.candidates, spec.elites, spec.iterations = int(horizon), int(candidates), int(elites), int(iterations)
        for a in range(len(sig)):
            spec.sigma[a], spec.sigma_min[a] = sig[a], smin[a]
        spec.lo, spec.hi, spec.alpha, spec.done_penalty = float(lo), float(hi), float(alpha), float(done_penalty)
        spec.seed = int(seed)
        self.horizon, self.num_candidates, self.num_elites, self.iterations = (int(horizon), int(candidates), int(elites),
                                                                               int(iterations))
        n, C, K, I = self.horizon, self.num_candidates, self.num_elites, self.iterations
        E, D, A = swarm.num_envs, swarm.num_drones, swarm.act_dim
        self._create(spec, L.QsCemBufs(), (
            ("mean", (n, E, D, A), "<f4"), ("std", (n, E, D, A), "<f4"), ("candidates", (n, C, E, D, A), "<f4"),
            ("ret", (C, E), "<f8"), ("first_done", (C, E), "<i4"), ("elites", (K,) + self._units(), "<i4"),
            ("iter_best", (I,) + self._units(), "<f8"), ("action", (E, D, A), "<f4"), ("tick", (1,), "<i8")))

    def reset(self, mean=None):
        """Set the mean sequence ((n, E, D, A) float32 on the device; None: zeros) and tick = 0."""
        self._reset(mean, "mean")

    def begin(self):
        self._call("begin")

    def sample(self, iteration=0):
        self._call("sample", int(iteration))

    def refit(self, iteration=0):
        self._call("refit", int(iteration))

    def finish(self):
        self._call("finish")


class SMCPlanner(_Sampling, _Planner):
    """The native particle (sequential Monte Carlo) tick on a branch set (qs_smc_*,
    include/quadswarm.h).

    `begin()` forks the planner's own branch set from the swarm; for each segment
    s of `segments` (a list of (start, length)), `sample(s)` draws the particles'
    actions round `nominal` (particle 0 follows the nominal), `advance(s)` runs
    them and `resample(s)` weighs the particles and, in every env whose effective
    sample size is below ess_frac * particles, resamples them systematically into
    `parents[s]` and gathers the branch set by it; `finish()` weighs the final
    particles, traces their `ancestors` back through `parents`, writes the
    weighted mean of their paths, shifted by one step, back to `nominal` and its
    first step to `action`.  `plan()` is all of that.  Every call is a few
    launches on the current stream with no host sync, and may be captured into a
    graph together with the `step` that runs `action`.  With ess_frac = 0 nothing
    is resampled: an MPPI tick whose horizon is not held to score_depth().

    The buffers are torch tensors that view the planner's device memory (no
    copies; they dangle after `close()`): nominal (n, E, D, A), candidates
    (n, C, E, D, A), base and weights (C, E) float64, parents and ancestors
    (S, C, E) int32, ess and offset (S, E) float64, resampled (S, E) int32, best
    (E,) int32, action (E, D, A), tick (1,) (the uint64 counter, viewed as int64).
    `set` is the planner's branch set for reading (`ret`, `first_done`,
    `ret_agent`, `steps`, `get_state`); the planner owns it.  There is no
    per-drone mode: the drones of an env share a branch's state, and no policy
    prior (`MPPIPlanner.set_prior`): the particles are resampled mid-horizon, which
    a closed-loop trajectory fixed before the tick cannot follow.  `set_sampling(rho)`
    correlates the noise along the steps of each segment (`_Sampling`; the sequence
    restarts at a segment's first step).  The swarm must outlive the planner."""

    _PREFIX = "qs_smc"

    def __init__(self, swarm, horizon, particles, sigma, segment=None, lo=-1.0, hi=1.0, lam=1.0, done_penalty=0.0,
                 ess_frac=0.5, seed=0):
        self._bind(swarm)
        sig = self._per_component(sigma, "sigma")
        if segment is None:
            segment = min(int(horizon), swarm.score_depth())
        spec = L.QsSmcSpec()
        spec.horizon, spec.segment, spec.particles = int(horizon), int(segment), int(particles)
        for a, s in enumerate(sig):
            spec.sigma[a] = s
        spec.lo, spec.hi, spec.lambda_, spec.done_penalty = float(lo), float(hi), float(lam), float(done_penalty)
        spec.ess_frac, spec.seed = float(ess_frac), int(seed)
        self.horizon, self.segment, self.num_particles = int(horizon), int(segment), int(particles)
        n, Lseg, C, E, D, A = self.horizon, self.segment, self.num_particles, swarm.num_envs, swarm.num_drones, swarm.act_dim
        self.segments = [(j, min(Lseg, n - j)) for j in range(0, n, Lseg)] if Lseg >= 1 else []
        S = max(len(self.segments), 1)
        self._create(spec, L.QsSmcBufs(), (
            ("nominal", (n, E, D, A), "<f4"), ("candidates", (n, C, E, D, A), "<f4"), ("base", (C, E), "<f8"),
            ("weights", (C, E), "<f8"), ("parents", (S, C, E), "<i4"), ("ancestors", (S, C, E), "<i4"),
            ("ess", (S, E), "<f8"), ("offset", (S, E), "<f8"), ("resampled", (S, E), "<i4"), ("best", (E,), "<i4"),
            ("action", (E, D, A), "<f4"), ("tick", (1,), "<i8")))
        b = ctypes.c_void_p()
        L.check(self.lib.qs_smc_branch(self._p, ctypes.byref(b)), "qs_smc_branch")
        self.set = _BranchView(swarm, C, b)

    def reset(self, nominal=None):
        """Set the nominal sequence ((n, E, D, A) float32 on the device; None: zeros) and tick = 0."""
        self._reset(nominal, "nominal")

    def begin(self):
        self._call("begin")

    def sample(self, segment=0):
        self._call("sample", int(segment))

    def advance(self, segment=0):
        self._call("advance", int(segment))

    def resample(self, segment=0):
        self._call("resample", int(segment))

    def finish(self):
        self._call("finish")

    def close(self):
        if getattr(self, "set", None) is not None:
            self.set.close()
        super().close()
