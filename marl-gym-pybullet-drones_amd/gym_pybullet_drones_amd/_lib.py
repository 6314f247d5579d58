"""ctypes binding of libquadswarm.so — the C-ABI declared in include/quadswarm.h.

This is exactly the binding a maintainer would add on the reference side
(INTEGRATION.md): plain pointers, sizes and a hipStream_t, no torch types.
The library must be built in-tree (``__graft_entry__.build()``); importing the
product path without it raises — there is no CPU fallback.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("QS_DEV_LIB") or os.path.join(_HERE, "lib", "libquadswarm.so")   # QS_DEV_LIB: dev variant builds

QS_OK = 0
TASK_MULTIHOVER, TASK_SPIRAL, TASK_FLOCK, TASK_MEETUP, TASK_LEADERFOLLOWER = 0, 1, 2, 3, 4
ACT_RPM, ACT_PID, ACT_VEL, ACT_ONE_D_RPM, ACT_ONE_D_PID = 0, 1, 2, 3, 4
PHYS_PYB, PHYS_DYN = 0, 1
AUX_GND, AUX_DRAG, AUX_DW = 1, 2, 4
AGENT_FIELDS, ENV_FIELDS = 29, 4
STATE_AGENT, STATE_ENV, STATE_HISTORY, STATE_EP_RETURN = 0, 1, 2, 3
FLAG_NO_AUTORESET = 1
FLAG_INKERNEL_RESET_SEARCH = 2
FLAG_CF2P = 4   # DroneModel.CF2P (include/quadswarm.h QS_FLAG_CF2P)
REASON_CRASH, REASON_FLIP, REASON_OOB, REASON_ZRANGE = 1, 2, 4, 8

# agent field offsets (include/quadswarm.h)
F_POS, F_QUAT, F_VEL, F_RPY_RATES, F_LAST_RPM = 0, 3, 7, 10, 13
F_PID_INT_POS, F_PID_INT_RPY, F_PID_LAST_RPY, F_TARGET = 17, 20, 23, 26
E_STEP_COUNTER, E_EPISODE, E_TOTAL_STEPS, E_EP_LEN = 0, 1, 2, 3


class QsSpec(ctypes.Structure):
    _fields_ = [
        ("task", ctypes.c_int32), ("num_envs", ctypes.c_int32), ("num_drones", ctypes.c_int32),
        ("act_type", ctypes.c_int32), ("physics", ctypes.c_int32), ("aux_forces", ctypes.c_uint32),
        ("pyb_freq", ctypes.c_int32), ("ctrl_freq", ctypes.c_int32), ("precision", ctypes.c_int32),
        ("flags", ctypes.c_uint32), ("env_offset", ctypes.c_int64), ("episode_len_sec", ctypes.c_double),
        ("initial_xyzs", ctypes.POINTER(ctypes.c_double)), ("spiral_radius", ctypes.c_double),
        ("spiral_period", ctypes.c_double), ("height_rate", ctypes.c_double),
        ("target_center", ctypes.c_double * 3),
    ]


class QsDims(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in (
        "num_envs", "num_drones", "num_agents", "act_dim", "obs_dim", "hist_len", "substeps",
        "precision", "agent_fields", "env_fields")]


class QsStepOut(ctypes.Structure):
    _fields_ = [("obs", ctypes.c_void_p), ("reward", ctypes.c_void_p), ("terminated", ctypes.c_void_p),
                ("truncated", ctypes.c_void_p), ("terminal_obs", ctypes.c_void_p), ("reasons", ctypes.c_void_p),
                ("actions_out", ctypes.c_void_p)]


class QsScoreOut(ctypes.Structure):
    """include/quadswarm.h qs_score_out: the per-candidate summary of qs_score."""
    _fields_ = [("ret", ctypes.c_void_p), ("first_done", ctypes.c_void_p)]


class QsBranchBufs(ctypes.Structure):
    """include/quadswarm.h qs_branch_bufs: a branch set's accumulators (device pointers)."""
    _fields_ = [("ret", ctypes.c_void_p), ("first_done", ctypes.c_void_p), ("ret_agent", ctypes.c_void_p)]


class QsMppiSpec(ctypes.Structure):
    """include/quadswarm.h qs_mppi_spec: what a planner is created from."""
    _fields_ = [("horizon", ctypes.c_int32), ("candidates", ctypes.c_int32), ("sigma", ctypes.c_float * 4),
                ("lo", ctypes.c_float), ("hi", ctypes.c_float), ("lambda_", ctypes.c_double),
                ("done_penalty", ctypes.c_double), ("seed", ctypes.c_uint64)]


class QsMppiBufs(ctypes.Structure):
    """include/quadswarm.h qs_mppi_bufs: the planner's device buffers."""
    _fields_ = [("nominal", ctypes.c_void_p), ("candidates", ctypes.c_void_p), ("ret", ctypes.c_void_p),
                ("first_done", ctypes.c_void_p), ("weights", ctypes.c_void_p), ("best", ctypes.c_void_p),
                ("action", ctypes.c_void_p), ("tick", ctypes.c_void_p)]


class QsCemSpec(ctypes.Structure):
    """include/quadswarm.h qs_cem_spec: what a CEM planner is created from."""
    _fields_ = [("horizon", ctypes.c_int32), ("candidates", ctypes.c_int32), ("elites", ctypes.c_int32),
                ("iterations", ctypes.c_int32), ("sigma", ctypes.c_float * 4), ("sigma_min", ctypes.c_float * 4),
                ("lo", ctypes.c_float), ("hi", ctypes.c_float), ("alpha", ctypes.c_double),
                ("done_penalty", ctypes.c_double), ("seed", ctypes.c_uint64)]


class QsCemBufs(ctypes.Structure):
    """include/quadswarm.h qs_cem_bufs: the CEM planner's device buffers."""
    _fields_ = [("mean", ctypes.c_void_p), ("std", ctypes.c_void_p), ("candidates", ctypes.c_void_p),
                ("ret", ctypes.c_void_p), ("first_done", ctypes.c_void_p), ("elites", ctypes.c_void_p),
                ("iter_best", ctypes.c_void_p), ("action", ctypes.c_void_p), ("tick", ctypes.c_void_p)]


class QsValueSpec(ctypes.Structure):
    """include/quadswarm.h qs_value_spec: the critic, normaliser and discount of a value tail."""
    _fields_ = [("in_dim", ctypes.c_int32), ("hidden", ctypes.c_int32),
                ("w1", ctypes.c_void_p), ("b1", ctypes.c_void_p), ("w2", ctypes.c_void_p), ("b2", ctypes.c_void_p),
                ("w3", ctypes.c_void_p), ("b3", ctypes.c_void_p), ("obs_mean", ctypes.c_void_p),
                ("obs_var", ctypes.c_void_p), ("obs_eps", ctypes.c_double), ("obs_clip", ctypes.c_double),
                ("gamma", ctypes.c_double), ("scale", ctypes.c_double)]


class QsPriorSpec(ctypes.Structure):
    """include/quadswarm.h qs_prior_spec: the actor, normaliser, count and obs of a policy prior."""
    _fields_ = [("in_dim", ctypes.c_int32), ("hidden", ctypes.c_int32), ("act_dim", ctypes.c_int32),
                ("w1", ctypes.c_void_p), ("b1", ctypes.c_void_p), ("w2", ctypes.c_void_p), ("b2", ctypes.c_void_p),
                ("w3", ctypes.c_void_p), ("b3", ctypes.c_void_p), ("logstd", ctypes.c_void_p),
                ("action_scale", ctypes.c_float), ("std_scale", ctypes.c_float), ("obs_mean", ctypes.c_void_p),
                ("obs_var", ctypes.c_void_p), ("obs_eps", ctypes.c_double), ("obs_clip", ctypes.c_double),
                ("count", ctypes.c_int32), ("obs", ctypes.c_void_p)]


class QsSamplingSpec(ctypes.Structure):
    """include/quadswarm.h qs_sampling_spec: the AR(1) coefficients and the CEM elite memory of a sampling spec."""
    _fields_ = [("rho", ctypes.c_float * 4), ("keep", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class QsTrackSpec(ctypes.Structure):
    """include/quadswarm.h qs_track_spec: the reference, row base and weights of a tracking cost."""
    _fields_ = [("ref", ctypes.c_void_p), ("base", ctypes.c_void_p), ("L", ctypes.c_int32), ("q", ctypes.c_float * 12),
                ("r", ctypes.c_float * 4), ("terminal", ctypes.c_float), ("reward_scale", ctypes.c_float)]


class QsAvoidSpec(ctypes.Structure):
    """include/quadswarm.h qs_avoid_spec: the obstacle table and the separation term's numbers."""
    _fields_ = [("obstacles", ctypes.c_void_p), ("M", ctypes.c_int32), ("sep_radius", ctypes.c_float),
                ("sep_weight", ctypes.c_float), ("sep_z_scale", ctypes.c_float)]


class QsSmcSpec(ctypes.Structure):
    """include/quadswarm.h qs_smc_spec: what a particle (SMC) planner is created from."""
    _fields_ = [("horizon", ctypes.c_int32), ("segment", ctypes.c_int32), ("particles", ctypes.c_int32),
                ("sigma", ctypes.c_float * 4), ("lo", ctypes.c_float), ("hi", ctypes.c_float),
                ("lambda_", ctypes.c_double), ("done_penalty", ctypes.c_double), ("ess_frac", ctypes.c_double),
                ("seed", ctypes.c_uint64)]


class QsSmcBufs(ctypes.Structure):
    """include/quadswarm.h qs_smc_bufs: the particle planner's device buffers."""
    _fields_ = [(n, ctypes.c_void_p) for n in (
        "nominal", "candidates", "base", "weights", "parents", "ancestors", "ess", "offset", "resampled", "best",
        "action", "tick")]


EPISODE_DTYPE = np.dtype([("ret", "<f8"), ("len", "<i4"), ("env", "<i4"), ("seq", "<i8")])

# Every symbol include/quadswarm.h declares (tests check the .so exports them).
ABI_VERSION = 4   # include/quadswarm.h QS_ABI_VERSION
EXPORTS = ("qs_create", "qs_destroy", "qs_last_error", "qs_abi_version", "qs_get_dims", "qs_reset",
           "qs_reset_envs", "qs_step", "qs_step_many", "qs_step_seq", "qs_score_depth", "qs_score",
           "qs_mppi_create", "qs_mppi_destroy", "qs_mppi_buffers", "qs_mppi_reset", "qs_mppi_sample", "qs_mppi_update",
           "qs_mppi_plan", "qs_cem_create", "qs_cem_destroy", "qs_cem_buffers", "qs_cem_reset", "qs_cem_begin", "qs_cem_sample",
           "qs_cem_refit", "qs_cem_finish", "qs_cem_plan", "qs_score_agents", "qs_pd_mppi_create", "qs_pd_mppi_ret_agent",
           "qs_pd_cem_create", "qs_pd_cem_ret_agent",
           "qs_value_tail", "qs_value_mppi_set", "qs_value_mppi_buffers", "qs_value_mppi_score", "qs_value_cem_set",
           "qs_value_cem_buffers", "qs_value_cem_score",
           "qs_prior_act", "qs_prior_mppi_set", "qs_prior_mppi_buffers", "qs_prior_mppi_rollout", "qs_prior_cem_set",
           "qs_prior_cem_buffers", "qs_prior_cem_rollout",
           "qs_sampling_mppi_set", "qs_sampling_cem_set", "qs_sampling_cem_buffers", "qs_sampling_smc_set",
           "qs_track_score", "qs_track_fold", "qs_track_mppi_set", "qs_track_mppi_buffers", "qs_track_mppi_score",
           "qs_track_cem_set", "qs_track_cem_buffers", "qs_track_cem_score",
           "qs_avoid_score", "qs_avoid_mppi_set", "qs_avoid_mppi_buffers", "qs_avoid_mppi_score",
           "qs_avoid_cem_set", "qs_avoid_cem_buffers", "qs_avoid_cem_score",
           "qs_branch_create", "qs_branch_destroy", "qs_branch_buffers", "qs_branch_steps", "qs_branch_fork",
           "qs_branch_advance", "qs_branch_select", "qs_branch_state",
           "qs_smc_create", "qs_smc_destroy", "qs_smc_buffers", "qs_smc_branch", "qs_smc_reset", "qs_smc_begin",
           "qs_smc_sample", "qs_smc_advance", "qs_smc_resample", "qs_smc_finish", "qs_smc_plan", "qs_launch_counts", "qs_ring_counts", "qs_state_io", "qs_episode_log", "qs_reset_error", "qs_calib_copy",
           # include/qs_learner.h
           "qs_gae", "qs_adam_gated", "qs_adam_commit", "qs_ppo_heads", "qs_ppo_heads_work_bytes",
           "qs_mlp_bias_tanh", "qs_mlp_bwd_blocks", "qs_mlp_tanh_bwd", "qs_mlp_sum_partials",
           "qs_mlp_sum_partials_multi", "qs_adam_step", "qs_mlp3_tiles", "qs_mlp3_pack_floats",
           "qs_mlp3_pack", "qs_mlp3_fwd", "qs_mlp3_fwd_rows", "qs_mlp3_fwd_group_rows", "qs_mlp3_bwd", "qs_mlp_wgrad", "qs_mlp_wgrad_chunks", "qs_adam_multi",
           "qs_adam_multi_pack", "qs_mlp_sum_adam", "qs_mlp_sum_adam_work_bytes", "qs_mlp3f_tiles", "qs_mlp3f_pack_floats", "qs_mlp3f_work_bytes",
           "qs_mlp3f_pack", "qs_mlp3f_actor", "qs_mlp3f_actor_w1", "qs_value_head", "qs_mlp_wgrad_x_chunks", "qs_mlp_wgrad_x",
           "qs_wgrad_rm", "qs_learner_last_error", "qs_rms_work_bytes", "qs_rms_update", "qs_rms_normalize",
           "qs_rms_last_error", "qs_mlp3_value_work_bytes", "qs_mlp3_fwd_rows_value", "qs_policy_sample", "qs_rollout_record", "qs_rollout_last_error", "qs_ppo_small_work_bytes", "qs_ppo_small_step", "qs_ppo_small_last_error",
           "qs_ppo_small_layout", "qs_ppo_critic_tiles", "qs_wgrad_t", "qs_ppo_small_grads", "qs_ppo_small_adam")
QS_PACK_F16 = 1 << 16   # pack_I flag: a qs_mlp3f_pack image (include/qs_learner.h)
QS_PACK_W2T = 1 << 17   # pack_I flag: a [256][256] W2ᵀ copy (include/qs_learner.h)
QS_PPO_SMALL_LAYOUT_N = 29   # include/qs_learner.h: entries qs_ppo_small_layout writes
QS_PPO_SMALL_MAX_ROWS = 16384   # include/qs_learner.h: mb·D at most on qs_ppo_small_step / _grads

_lib = None


class QsMlp256(ctypes.Structure):
    """include/qs_learner.h qs_mlp256: one 256-wide tanh MLP inside its flat Adam buffers."""
    _fields_ = [("params", ctypes.c_void_p), ("exp_avg", ctypes.c_void_p), ("exp_avg_sq", ctypes.c_void_p),
                ("step", ctypes.c_void_p), ("w2t", ctypes.c_void_p),
                ("w1", ctypes.c_int64), ("b1", ctypes.c_int64), ("w2", ctypes.c_int64), ("b2", ctypes.c_int64),
                ("w3", ctypes.c_int64), ("b3", ctypes.c_int64), ("logstd", ctypes.c_int64),
                ("in_", ctypes.c_int32), ("out", ctypes.c_int32),
                ("lr", ctypes.c_float), ("beta1", ctypes.c_float), ("beta2", ctypes.c_float), ("eps", ctypes.c_float),
                ("w1p", ctypes.c_void_p)]


class QuadSwarmError(RuntimeError):
    pass


def load():
    """Load libquadswarm.so (after torch, so both share one HIP runtime)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise QuadSwarmError(
            f"{LIB_PATH} is missing: build the HIP extension first "
            "(python -c 'import __graft_entry__ as g; g.build()'). There is no CPU fallback.")
    try:
        import torch  # noqa: F401  (registers libamdhip64.so.7 first)
    except ImportError:
        pass
    L = ctypes.CDLL(LIB_PATH)
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    L.qs_last_error.restype = ctypes.c_char_p
    L.qs_abi_version.restype = i32
    if L.qs_abi_version() != ABI_VERSION:   # a stale build: its signatures differ from the argtypes below
        raise QuadSwarmError(f"{LIB_PATH} has ABI version {L.qs_abi_version()}, this package binds "
                             f"{ABI_VERSION}: rebuild the HIP extension")
    L.qs_create.argtypes = [ctypes.POINTER(QsSpec), i32, ctypes.POINTER(vp)]
    L.qs_destroy.argtypes = [vp]
    L.qs_get_dims.argtypes = [vp, ctypes.POINTER(QsDims)]
    L.qs_reset.argtypes = [vp, ctypes.c_uint64, vp, vp]
    L.qs_reset_envs.argtypes = [vp, vp, vp, vp]
    L.qs_step.argtypes = [vp, vp, ctypes.POINTER(QsStepOut), vp]
    L.qs_step_many.argtypes = [vp, i32, ctypes.POINTER(QsStepOut), vp]
    L.qs_step_seq.argtypes = [vp, i32, ctypes.POINTER(vp), ctypes.POINTER(QsStepOut), vp]
    if hasattr(L, "qs_score"):   # (a QS_DEV_LIB build from before the entry points: A/B runs)
        L.qs_score_depth.argtypes = [vp]
        L.qs_score.argtypes = [vp, i32, i32, ctypes.POINTER(vp), ctypes.POINTER(QsStepOut), ctypes.POINTER(QsScoreOut), vp]
    if hasattr(L, "qs_mppi_create"):   # (a QS_DEV_LIB build from before the entry points: A/B runs)
        L.qs_mppi_create.argtypes = [vp, ctypes.POINTER(QsMppiSpec), ctypes.POINTER(vp)]
        L.qs_mppi_destroy.argtypes = [vp]
        L.qs_mppi_buffers.argtypes = [vp, ctypes.POINTER(QsMppiBufs)]
        L.qs_mppi_reset.argtypes = [vp, vp, vp]
        L.qs_mppi_sample.argtypes = [vp, vp]
        L.qs_mppi_update.argtypes = [vp, vp]
        L.qs_mppi_plan.argtypes = [vp, vp]
    if hasattr(L, "qs_cem_create"):   # (a QS_DEV_LIB build from before the entry points: A/B runs)
        L.qs_cem_create.argtypes = [vp, ctypes.POINTER(QsCemSpec), ctypes.POINTER(vp)]
        L.qs_cem_destroy.argtypes = [vp]
        L.qs_cem_buffers.argtypes = [vp, ctypes.POINTER(QsCemBufs)]
        L.qs_cem_reset.argtypes = [vp, vp, vp]
        L.qs_cem_begin.argtypes = [vp, vp]
        L.qs_cem_sample.argtypes = [vp, i32, vp]
        L.qs_cem_refit.argtypes = [vp, i32, vp]
        L.qs_cem_finish.argtypes = [vp, vp]
        L.qs_cem_plan.argtypes = [vp, vp]
    if hasattr(L, "qs_score_agents"):   # (a QS_DEV_LIB build from before the entry points: A/B runs)
        L.qs_score_agents.argtypes = [vp, i32, i32, ctypes.POINTER(vp), ctypes.POINTER(QsStepOut), ctypes.POINTER(QsScoreOut),
                                      vp, vp]
        L.qs_pd_mppi_create.argtypes = [vp, ctypes.POINTER(QsMppiSpec), ctypes.POINTER(vp)]
        L.qs_pd_mppi_ret_agent.argtypes = [vp, ctypes.POINTER(vp)]
        L.qs_pd_cem_create.argtypes = [vp, ctypes.POINTER(QsCemSpec), ctypes.POINTER(vp)]
        L.qs_pd_cem_ret_agent.argtypes = [vp, ctypes.POINTER(vp)]
    if hasattr(L, "qs_value_tail"):   # (a QS_DEV_LIB build from before the entry points: A/B runs)
        L.qs_value_tail.argtypes = [ctypes.POINTER(QsValueSpec), i32, i32, i32, i32, i32, i32, vp, ctypes.POINTER(vp), vp,
                                    vp, vp, vp]
        for who in ("mppi", "cem"):
            getattr(L, f"qs_value_{who}_set").argtypes = [vp, ctypes.POINTER(QsValueSpec)]
            getattr(L, f"qs_value_{who}_buffers").argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(vp)]
            getattr(L, f"qs_value_{who}_score").argtypes = [vp, vp]
    if hasattr(L, "qs_prior_act"):   # (a QS_DEV_LIB build from before the entry points: A/B runs)
        L.qs_prior_act.argtypes = [ctypes.POINTER(QsPriorSpec), i32, i32, i32, i32, ctypes.c_float, ctypes.c_float,
                                   ctypes.c_uint64, i64, vp, vp, i32, vp, vp, vp]
        for who in ("mppi", "cem"):
            getattr(L, f"qs_prior_{who}_set").argtypes = [vp, ctypes.POINTER(QsPriorSpec)]
            getattr(L, f"qs_prior_{who}_buffers").argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(vp)]
            getattr(L, f"qs_prior_{who}_rollout").argtypes = [vp, vp]
    if hasattr(L, "qs_sampling_cem_set"):   # (a QS_DEV_LIB build from before the entry points: A/B runs)
        for who in ("mppi", "cem", "smc"):
            getattr(L, f"qs_sampling_{who}_set").argtypes = [vp, ctypes.POINTER(QsSamplingSpec)]
        L.qs_sampling_cem_buffers.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(vp)]
    if hasattr(L, "qs_track_score"):   # (a QS_DEV_LIB build from before the entry points: A/B runs)
        L.qs_track_score.argtypes = [vp, i32, i32, ctypes.POINTER(vp), ctypes.POINTER(QsStepOut), ctypes.POINTER(QsScoreOut),
                                     vp, ctypes.POINTER(QsTrackSpec), vp, vp]
        L.qs_track_fold.argtypes = [i32, i32, i32, ctypes.c_double, vp, vp, vp, vp]
        for who in ("mppi", "cem"):
            getattr(L, f"qs_track_{who}_set").argtypes = [vp, ctypes.POINTER(QsTrackSpec)]
            getattr(L, f"qs_track_{who}_buffers").argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(vp)]
            getattr(L, f"qs_track_{who}_score").argtypes = [vp, vp]
    if hasattr(L, "qs_avoid_score"):   # (a QS_DEV_LIB build from before the entry points: A/B runs)
        L.qs_avoid_score.argtypes = [vp, i32, i32, ctypes.POINTER(vp), ctypes.POINTER(QsStepOut), ctypes.POINTER(QsScoreOut),
                                     vp, ctypes.POINTER(QsTrackSpec), ctypes.POINTER(QsAvoidSpec), vp, vp]
        for who in ("mppi", "cem"):
            getattr(L, f"qs_avoid_{who}_set").argtypes = [vp, ctypes.POINTER(QsAvoidSpec)]
            getattr(L, f"qs_avoid_{who}_buffers").argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(vp)]
            getattr(L, f"qs_avoid_{who}_score").argtypes = [vp, vp]
    if hasattr(L, "qs_branch_create"):   # (a QS_DEV_LIB build from before the entry points: A/B runs)
        L.qs_branch_create.argtypes = [vp, i32, ctypes.POINTER(vp)]
        L.qs_branch_destroy.argtypes = [vp]
        L.qs_branch_buffers.argtypes = [vp, ctypes.POINTER(QsBranchBufs)]
        L.qs_branch_steps.argtypes = [vp, ctypes.POINTER(i64)]
        L.qs_branch_fork.argtypes = [vp, vp]
        L.qs_branch_advance.argtypes = [vp, i32, ctypes.POINTER(vp), ctypes.POINTER(QsStepOut), vp]
        L.qs_branch_select.argtypes = [vp, vp, vp]
        L.qs_branch_state.argtypes = [vp, i32, vp, vp]
    if hasattr(L, "qs_smc_create"):   # (a QS_DEV_LIB build from before the entry points: A/B runs)
        L.qs_smc_create.argtypes = [vp, ctypes.POINTER(QsSmcSpec), ctypes.POINTER(vp)]
        L.qs_smc_destroy.argtypes = [vp]
        L.qs_smc_buffers.argtypes = [vp, ctypes.POINTER(QsSmcBufs)]
        L.qs_smc_branch.argtypes = [vp, ctypes.POINTER(vp)]
        L.qs_smc_reset.argtypes = [vp, vp, vp]
        L.qs_smc_begin.argtypes = [vp, vp]
        L.qs_smc_sample.argtypes = [vp, i32, vp]
        L.qs_smc_advance.argtypes = [vp, i32, vp]
        L.qs_smc_resample.argtypes = [vp, i32, vp]
        L.qs_smc_finish.argtypes = [vp, vp]
        L.qs_smc_plan.argtypes = [vp, vp]
    if hasattr(L, "qs_launch_counts"):   # (a QS_DEV_LIB build from before the entry point: A/B runs)
        L.qs_launch_counts.argtypes = [vp, ctypes.POINTER(i64)]
    if hasattr(L, "qs_ring_counts"):
        L.qs_ring_counts.argtypes = [vp, ctypes.POINTER(i64), ctypes.POINTER(i64)]
    L.qs_state_io.argtypes = [vp, i32, vp, i32, vp]
    L.qs_episode_log.argtypes = [vp, vp, i64, ctypes.POINTER(i64), ctypes.POINTER(i64), vp]
    L.qs_reset_error.argtypes = [vp, ctypes.POINTER(i32)]
    L.qs_calib_copy.argtypes = [vp, vp, i64, vp]
    L.qs_gae.argtypes = [ctypes.c_int32, i64, vp, vp, vp, vp, vp, ctypes.c_double, ctypes.c_double, ctypes.c_int32,
                         vp, vp, vp]
    f32 = ctypes.c_float
    L.qs_adam_gated.argtypes = [i64, vp, vp, vp, vp, vp, f32, f32, f32, f32, vp, f32, vp]
    L.qs_adam_commit.argtypes = [vp, vp, f32, vp]
    L.qs_ppo_heads.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, vp, vp, vp, f32, vp, vp, vp, vp, vp,
                               f32, f32, vp, vp, vp, vp, vp, vp, vp]
    L.qs_ppo_heads_work_bytes.argtypes = [ctypes.c_int32, ctypes.c_int32]
    L.qs_mlp_bias_tanh.argtypes = [i64, ctypes.c_int32, vp, vp, vp, ctypes.c_int32, vp, vp, vp, vp]
    L.qs_mlp_bwd_blocks.argtypes = [i64]
    L.qs_mlp_tanh_bwd.argtypes = [i64, ctypes.c_int32, vp, vp, ctypes.c_int32, vp, vp, vp, vp, vp]
    L.qs_mlp_sum_partials.argtypes = [ctypes.c_int32, i64, vp, vp, i64, vp, i64, vp, vp]
    L.qs_mlp_sum_partials_multi.argtypes = [ctypes.c_int32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.qs_adam_step.argtypes = [i64, vp, vp, vp, vp, vp, f32, f32, f32, f32, vp, f32, vp, vp]
    L.qs_adam_multi.argtypes = [ctypes.c_int32] + [vp] * 14
    L.qs_mlp3_tiles.argtypes = [i64, i32]
    L.qs_mlp3_pack_floats.argtypes = [ctypes.c_int32]
    L.qs_mlp3_pack.argtypes = [ctypes.c_int32, ctypes.c_int32, vp, vp, vp, vp]
    L.qs_mlp3_fwd.argtypes = [i64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32] + [vp] * 10
    L.qs_mlp3_bwd.argtypes = [i64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32] + [vp] * 10
    L.qs_mlp3_fwd_rows.argtypes = [i64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32] + [vp] * 12
    L.qs_mlp_wgrad_chunks.argtypes = [i64, ctypes.c_int32, ctypes.c_int32]
    L.qs_mlp_wgrad_chunks.restype = ctypes.c_int32
    L.qs_mlp_wgrad.argtypes = [i64, ctypes.c_int32, ctypes.c_int32, vp, vp, ctypes.c_int32, ctypes.c_int32, vp, vp]
    L.qs_mlp3_fwd_group_rows.argtypes = [i64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, vp, vp,
                                         ctypes.c_int32] + [vp] * 9
    L.qs_adam_multi_pack.argtypes = [ctypes.c_int32] + [vp] * 16 + [ctypes.c_int32, vp, vp]
    L.qs_mlp_sum_adam.argtypes = [ctypes.c_int32] + [vp] * 9 + [ctypes.c_int32] + [vp] * 18
    L.qs_mlp3f_tiles.argtypes = [i64]
    L.qs_mlp3f_pack_floats.argtypes = [ctypes.c_int32]
    L.qs_mlp3f_work_bytes.argtypes = [i64]
    L.qs_mlp3f_pack.argtypes = [ctypes.c_int32, vp, vp, vp, vp]
    L.qs_mlp3f_actor.argtypes = ([i64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32] + [vp] * 8 + [f32] + [vp] * 3
                                 + [f32, f32] + [vp] * 12)
    L.qs_mlp3f_actor_w1.argtypes = ([i64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32] + [vp] * 8 + [f32] + [vp] * 3
                                    + [f32, f32] + [vp] * 13)
    L.qs_value_head.argtypes = [ctypes.c_int32, ctypes.c_int32] + [vp] * 7
    L.qs_mlp_wgrad_x_chunks.argtypes = [i64, ctypes.c_int32]
    L.qs_mlp_wgrad_x.argtypes = [i64, ctypes.c_int32, ctypes.c_int32, vp, ctypes.c_int32, vp, vp, vp]
    L.qs_wgrad_rm.argtypes = [i64, ctypes.c_int32, ctypes.c_int32, vp, vp, ctypes.c_int32, vp, vp]
    L.qs_learner_last_error.restype = ctypes.c_char_p
    L.qs_rms_last_error.restype = ctypes.c_char_p
    L.qs_rollout_last_error.restype = ctypes.c_char_p
    L.qs_mlp3_value_work_bytes.argtypes = [i64]
    L.qs_mlp3_fwd_rows_value.argtypes = [i64, ctypes.c_int32, ctypes.c_int32] + [vp] * 16
    L.qs_policy_sample.argtypes = [i64, ctypes.c_int32, vp, vp, f32, f32, ctypes.c_int32, vp, vp, vp, vp]
    L.qs_rollout_record.argtypes = [i64] + [vp] * 7
    L.qs_ppo_small_last_error.restype = ctypes.c_char_p
    L.qs_ppo_small_work_bytes.argtypes = [ctypes.c_int32] * 5
    L.qs_ppo_small_layout.argtypes = [ctypes.c_int32] * 5 + [vp, ctypes.c_int32]
    L.qs_ppo_critic_tiles.argtypes = [ctypes.c_int32, ctypes.c_int32, vp, vp, vp, ctypes.POINTER(QsMlp256), vp, vp, vp]
    L.qs_wgrad_t.argtypes = [i64, i64, ctypes.c_int32, ctypes.c_int32, vp, vp, ctypes.c_int32, vp, vp]
    L.qs_ppo_small_step.argtypes = ([ctypes.c_int32, ctypes.c_int32] + [vp] * 6 + [f32, f32, f32, ctypes.c_int32, f32]
                                    + [ctypes.POINTER(QsMlp256)] * 2 + [vp] * 4)
    L.qs_ppo_small_grads.argtypes = ([ctypes.c_int32, ctypes.c_int32] + [vp] * 6 + [f32, f32, f32]
                                     + [ctypes.POINTER(QsMlp256)] * 2 + [vp] * 6)
    L.qs_ppo_small_adam.argtypes = ([ctypes.c_int32, ctypes.c_int32] + [ctypes.POINTER(QsMlp256)] * 2 + [vp] * 2
                                    + [f32, ctypes.c_int32, f32] + [vp] * 3)
    L.qs_rms_work_bytes.argtypes = [i64, ctypes.c_int32]
    L.qs_rms_update.argtypes = [i64, ctypes.c_int32] + [vp] * 7
    L.qs_rms_normalize.argtypes = [i64, ctypes.c_int32, vp, vp, vp, ctypes.c_double, ctypes.c_double, vp, vp]
    for name in EXPORTS:
        if (name in ("qs_launch_counts", "qs_ring_counts", "qs_score_depth", "qs_score") or name.startswith(("qs_mppi_", "qs_cem_", "qs_pd_", "qs_branch_", "qs_smc_"))
                or name == "qs_score_agents" or name.startswith(("qs_value_", "qs_prior_", "qs_sampling_", "qs_track_", "qs_avoid_"))) and not hasattr(L, name):
            continue   # (a QS_DEV_LIB build from before the entry point)
        if name not in ("qs_last_error", "qs_learner_last_error", "qs_rms_last_error", "qs_ppo_small_last_error",
                        "qs_rollout_last_error"):
            getattr(L, name).restype = i32
    L.qs_ppo_heads_work_bytes.restype = i64
    L.qs_mlp3_pack_floats.restype = i64
    L.qs_mlp3f_pack_floats.restype = i64
    L.qs_mlp3f_work_bytes.restype = i64
    L.qs_mlp_sum_adam_work_bytes.restype = i64
    L.qs_rms_work_bytes.restype = i64
    L.qs_mlp3_value_work_bytes.restype = i64
    L.qs_ppo_small_work_bytes.restype = i64
    L.qs_mlp_sum_adam_work_bytes.argtypes = []
    _lib = L
    return L


def check(rc, what=""):
    if rc != QS_OK:
        lib = load()
        if what.startswith("qs_rms"):
            msg = lib.qs_rms_last_error()
        elif what.startswith(("qs_policy_sample", "qs_rollout")):
            msg = lib.qs_rollout_last_error()
        elif what.startswith(("qs_ppo_small", "qs_ppo_critic", "qs_wgrad_t")):
            msg = lib.qs_ppo_small_last_error()
        elif what.startswith(("qs_gae", "qs_adam", "qs_ppo", "qs_mlp", "qs_wgrad", "qs_value_head")):
            msg = lib.qs_learner_last_error()
        else:
            msg = lib.qs_last_error()
        raise QuadSwarmError(f"{what} failed (rc={rc}): {msg.decode() if msg else ''}")


def ptr(t):
    """Device pointer of a torch tensor (or None)."""
    return None if t is None else ctypes.c_void_p(t.data_ptr())
