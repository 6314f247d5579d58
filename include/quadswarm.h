/*
 * quadswarm.h — C-ABI of the MI355X-native batched quadrotor-swarm step.
 *
 * This is the drop-in boundary for the reference's per-control-step drone
 * update.  In the reference that boundary is the pybullet
 * CPython extension plus the Python env classes that drive it:
 *
 *   reference interface replaced                        entry point here
 *   --------------------------------------------------  ------------------
 *   BaseAviary.__init__ (+ _parseURDFParameters)         qs_create
 *     gym_pybullet_drones/envs/BaseAviary.py:25-216, 985-1017
 *   BaseAviary.reset / MultiHoverAviary.reset            qs_reset
 *     BaseAviary.py:220-255, MultiHoverAviary.py:75-110
 *   BaseAviary.step (preprocess → PYB_STEPS_PER_CTRL     qs_step
 *     substeps → readback → obs/reward/term/trunc)
 *     BaseAviary.py:259-383, BaseRLAviary.py:160-239, 284-319,
 *     DSLPIDControl.py:82-259, MultiHoverAviary.py:128-268,
 *     SpiralAviary.py:82-196
 *   worker.step_env auto-reset                           qs_step (in-kernel)
 *     safe_control_gym/.../subproc_vec_env.py:188-206
 *   p.resetBasePositionAndOrientation / getBase*         qs_state_io
 *     BaseAviary.py:509-519, 865-875 (state injection / readback)
 *   VecRecordEpisodeStatistics.step_wait                 qs_episode_log
 *     safe_control_gym/.../record_episode_statistics.py:144-172
 *   BaseAviary.close (p.disconnect)                      qs_destroy
 *
 * Conventions
 *  - All array arguments of qs_reset/qs_step/qs_state_io/qs_episode_log are
 *    DEVICE pointers (HBM, from hipMalloc or a torch tensor's data_ptr()).
 *    `stream` is a hipStream_t passed as void*; every call is stream-ordered
 *    and asynchronous unless documented otherwise.
 *  - Agent index a = env * num_drones + drone.  Observation layout is
 *    [env][drone][obs_dim] float32 (the reference's per-env (D, O) float32
 *    obs stacked over envs, BaseRLAviary.py:315-319, SpiralAviary.py:146).
 *  - Actions are float32 [env][drone][act_dim] (the trainer's dtype).
 *  - Rewards are `real` = float (precision 4) or double (precision 8).
 *  - Errors: every function returns 0 on success or a negative QS_E_* code;
 *    qs_last_error() returns a thread-local message.  Nothing calls exit().
 *  - Threading: a handle is bound to one device, is not re-entrant, and must
 *    be used from one host thread at a time (one handle per rank).
 */
#ifndef QUADSWARM_H
#define QUADSWARM_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QS_ABI_VERSION 4   /* 2: qs_episode_log reports the records it wrote; 3: qs_ppo_small_layout takes
                              the caller's entry count; 4: QS_FLAG_CF2P (qs_step_seq came later as a new
                              symbol: nothing that existed changed, so the number stayed) */

/* ---- status codes ------------------------------------------------------ */
#define QS_OK 0
#define QS_E_INVALID (-1)   /* bad argument / unsupported configuration     */
#define QS_E_HIP (-2)       /* HIP runtime error (message has the HIP text)  */
#define QS_E_NOMEM (-3)     /* device allocation failed                      */
#define QS_E_STATE (-4)     /* handle in wrong state (e.g. step before reset) */

/* ---- enums mirroring gym_pybullet_drones/utils/enums.py:3-48 ------------ */
typedef enum {
  QS_TASK_MULTIHOVER = 0, /* MultiHoverAviary.py                          */
  QS_TASK_SPIRAL = 1,     /* SpiralAviary.py (SpiralFormationAviary)      */
  QS_TASK_FLOCK = 2,      /* FlockAviary.py                               */
  QS_TASK_MEETUP = 3,     /* MeetupAviary.py                              */
  QS_TASK_LEADERFOLLOWER = 4 /* LeaderFollowerAviary.py                   */
} qs_task;

typedef enum {            /* ActionType (enums.py:35-41)                   */
  QS_ACT_RPM = 0,
  QS_ACT_PID = 1,         /* waypoint via _calculateNextStep (BA:1108-1150) */
  QS_ACT_VEL = 2,
  QS_ACT_ONE_D_RPM = 3,
  QS_ACT_ONE_D_PID = 4
} qs_action_type;

typedef enum {            /* Physics (enums.py:13-21)                      */
  QS_PHYS_PYB = 0,        /* Bullet's step of BaseAviary._physics forces
                             (BA:679-711, 369-370), restated */
  QS_PHYS_DYN = 1         /* BaseAviary._dynamics (BA:815-892)            */
} qs_physics;

/* Extra force models: BaseAviary._groundEffect (BA:715-750), _drag
 * (BA:754-781), _downwash (BA:785-811).  With QS_PHYS_PYB they give the
 * reference's PYB_GND / PYB_DRAG / PYB_DW / PYB_GND_DRAG_DW; with
 * QS_PHYS_DYN they are added to the DYN force/torque sum (build-defined
 * combination, SURVEY §8 "Physics-mode note").                           */
#define QS_AUX_GND 1u
#define QS_AUX_DRAG 2u
#define QS_AUX_DW 4u

/* qs_spec.flags */
#define QS_FLAG_NO_AUTORESET 1u  /* single-env facade: BaseAviary.step never
                                    resets by itself (BaseAviary.py:259-383) */
#define QS_FLAG_INKERNEL_RESET_SEARCH 2u  /* MultiHover layouts that can reject:
                                    run the whole reset rejection loop
                                    (MultiHoverAviary.py:83-102) inside the
                                    step kernel, no deferred search launch
                                    (the validation form of the deferred one) */
#define QS_FLAG_CF2P 4u  /* DroneModel.CF2P, the + configuration (cf2p.urdf:
                                    inertia and prop links on the axes;
                                    BaseAviary.py:852-853 torques,
                                    DSLPIDControl.py:54-60 mixer); default
                                    DroneModel.CF2X */

typedef struct qs_spec {
  int32_t task;          /* qs_task                                        */
  int32_t num_envs;      /* E on this device (the rank's shard)            */
  int32_t num_drones;    /* D                                              */
  int32_t act_type;      /* qs_action_type                                 */
  int32_t physics;       /* qs_physics                                     */
  uint32_t aux_forces;   /* OR of QS_AUX_*                                 */
  int32_t pyb_freq;      /* 240 (BA:32)                                    */
  int32_t ctrl_freq;     /* MultiHover 30 (MH:20), Spiral 48 (SP:28)       */
  int32_t precision;     /* 4 = fp32 state/math, 8 = fp64 state/math       */
  uint32_t flags;        /* OR of QS_FLAG_*                                 */
  int64_t env_offset;    /* global id of env 0 (multi-GPU shard offset)    */
  double episode_len_sec;/* MH 8 (MH:58), SP 12 (SP:39)                    */
  /* [D][3] initial positions, or NULL for the reference default:
   *   MultiHover: diagonal grid x=y=i*4L, z=0.1125 (BA:194-197)
   *   Spiral: circle radius R at z=0.3 (SP:47-53)                         */
  const double* initial_xyzs;
  /* Spiral parameters (SP:33-45); ignored for MultiHover. */
  double spiral_radius;  /* 0.4  */
  double spiral_period;  /* 10.0 */
  double height_rate;    /* 0.05 */
  double target_center[3];
} qs_spec;

/* Derived sizes (BRL:66, 141-147, 262-277; SP:105-113). */
typedef struct qs_dims {
  int32_t num_envs, num_drones, num_agents;  /* N = E*D                   */
  int32_t act_dim;        /* A                                            */
  int32_t obs_dim;        /* O = 12 + H*A (+11 Spiral)                    */
  int32_t hist_len;       /* H = ctrl_freq // 2                           */
  int32_t substeps;       /* PYB_STEPS_PER_CTRL                           */
  int32_t precision;      /* 4 or 8                                       */
  int32_t agent_fields;   /* QS_AGENT_FIELDS                              */
  int32_t env_fields;     /* QS_ENV_FIELDS                                */
} qs_dims;

/* Per-agent state, structure-of-arrays [field][N] in `real` precision.
 * This is what BaseAviary keeps in pybullet + its numpy arrays
 * (BA:471-477, 509-519), plus DSLPIDControl's integrators
 * (DSLPIDControl.py:73-78) and MultiHover's TARGET_POS (MH:106).        */
enum {
  QS_F_POS = 0,        /* 3: x y z (world)                                */
  QS_F_QUAT = 3,       /* 4: x y z w (pybullet order, NOT renormalised)   */
  QS_F_VEL = 7,        /* 3: world linear velocity                        */
  QS_F_RPY_RATES = 10, /* 3: body angular rates, DYN (BA:477, 877)        */
  QS_F_LAST_RPM = 13,  /* 4: last_clipped_action (BA:372, 468)            */
  QS_F_PID_INT_POS = 17, /* 3: integral_pos_e (PID:190-192)               */
  QS_F_PID_INT_RPY = 20, /* 3: integral_rpy_e (PID:249-251)               */
  QS_F_PID_LAST_RPY = 23,/* 3: last_rpy (PID:247-248)                     */
  QS_F_TARGET = 26,    /* 3: MultiHover TARGET_POS (MH:72, 106)           */
  QS_AGENT_FIELDS = 29
};

/* Per-env int32 state [field][E]. */
enum {
  QS_E_STEP_COUNTER = 0, /* BaseAviary.step_counter (PYB steps, BA:382)   */
  QS_E_EPISODE = 1,      /* episodes started by this env (RNG counter)    */
  QS_E_TOTAL_STEPS = 2,  /* control steps ever taken (history ring head)  */
  QS_E_EP_LEN = 3,       /* VecRecordEpisodeStatistics.episode_length     */
  QS_ENV_FIELDS = 4
};

typedef enum {
  QS_STATE_AGENT = 0,    /* real  [QS_AGENT_FIELDS][N]                     */
  QS_STATE_ENV = 1,      /* int32 [QS_ENV_FIELDS][E]                       */
  QS_STATE_HISTORY = 2,  /* float [H][N][A] action ring (BRL:66-67, 187)   */
  QS_STATE_EP_RETURN = 3 /* double [E] episode_return accumulator          */
} qs_state_block;

/* Termination reason bits (MultiHoverAviary._computeTerminated MH:216-241). */
#define QS_REASON_CRASH 1u   /* z < 0.03                                  */
#define QS_REASON_FLIP 2u    /* |roll| > 1.2 or |pitch| > 1.2             */
#define QS_REASON_OOB 4u     /* |x| > 3 or |y| > 3                         */
#define QS_REASON_ZRANGE 8u  /* Spiral: z < 0.05 or z > 3 (SP:185-191)    */

typedef struct qs_handle qs_handle;

/* Optional outputs of one control step. Every pointer may be NULL. */
typedef struct qs_step_out {
  float* obs;            /* [E][D][O] float32 (post auto-reset obs)        */
  void* reward;          /* [E] real                                      */
  uint8_t* terminated;   /* [E]                                           */
  uint8_t* truncated;    /* [E]                                           */
  float* terminal_obs;   /* [E][D][O]: obs before auto-reset; only rows of
                            envs with terminated|truncated are written     */
  uint8_t* reasons;      /* [E][D] QS_REASON_* bits at the terminal state  */
  float* actions_out;    /* [E][D][A]: copy of the actions consumed
                            (useful with the random policy)                */
} qs_step_out;

/* Random policy: when `actions` is NULL, qs_step draws i.i.d. U(-1,1)
 * actions from Philox4x32-10(key=seed, counter=(env_total_steps,
 * global_env, 0, (1<<24)|drone)) — the synthetic workload of SURVEY §8(d). */

int qs_create(const qs_spec* spec, int device, qs_handle** out);
int qs_destroy(qs_handle* h);
const char* qs_last_error(void);
int qs_abi_version(void);
int qs_get_dims(const qs_handle* h, qs_dims* out);

/* Reset every env (episode 0 draws), as MAPPO.reset → VecEnv.reset does
 * (mappo.py:147-167).  Writes the initial obs if obs != NULL.  PID state,
 * action history and episode counters are zeroed only here (the reference
 * never resets them inside an episode boundary). */
int qs_reset(qs_handle* h, uint64_t seed, float* obs, void* stream);

/* env.reset() for the envs with mask[e] != 0 (mask: device uint8 [E], NULL =
 * all): MultiHoverAviary.reset semantics (MH:75-110) — new episode draw,
 * step_counter = 0; PID integrators and the action history persist, as in
 * the reference.  Writes obs rows of the reset envs if obs != NULL. */
int qs_reset_envs(qs_handle* h, const uint8_t* mask, float* obs, void* stream);

/* One control step of every env: the reference's BaseAviary.step for all
 * envs + the worker's auto-reset.  actions: [E][D][A] float32 or NULL.
 *
 * Environment QS_WAVE_REDUCE (read once, at qs_create; default 1): in the
 * multi-step launches (qs_step_many, captured qs_step) with 2, 4, 8 or 16
 * drones per env the per-env reward sum, done flag and reset flag are formed
 * inside the wavefront (DPP reads, ballots); 0 keeps them on the LDS path that
 * every other drone count, the MARL tasks and the single-step launches take.
 * Results are bit-identical either way; the switch is there for A/B runs and
 * tests. */
int qs_step(qs_handle* h, const float* actions, const qs_step_out* out,
            void* stream);

/* n consecutive control steps under the random policy (qs_step with actions
 * = NULL, n times); step j writes outs[j].  The steps run K to a launch, K =
 * the handle's fusion depth (environment QS_MAX_FUSED_STEPS at qs_create,
 * 1..32: the depth cap, one set of output pointers per step in the kernel's
 * arguments), with the envs' state kept on-chip between the steps of a launch;
 * every output is bit-identical to n qs_step calls.  Steps share a launch only
 * while no output range of one overlaps an output range of another, and
 * handles that run the deferred reset search after each step (MultiHover
 * layouts whose reset draws can be rejected) take one step per launch.
 *
 * qs_step itself joins consecutive random-policy steps in the same way while
 * its stream is being captured into a graph: a call whose stream's capture
 * still ends in the kernel node of the previous call, and whose outputs are
 * disjoint from that node's, extends the node instead of launching.  An event
 * recorded on the capturing stream between two such steps and waited for by
 * another stream therefore marks the whole node, later steps included. */
int qs_step_many(qs_handle* h, int n, const qs_step_out* outs, void* stream);

/* n consecutive control steps; step j consumes actions[j] ([E][D][A] float32,
 * device) and writes outs[j].  Equal, bit for bit, to n qs_step(h, actions[j],
 * &outs[j], stream) calls.  actions == NULL: exactly qs_step_many.
 *
 * `actions` is a host array of n device pointers, read during the call; the
 * buffers need 4-byte alignment only.  Either every step reads its actions or
 * none does: an array with a NULL among its entries is QS_E_INVALID.  n < 0, or
 * n > 0 without outs, is QS_E_INVALID; a call before qs_reset is QS_E_STATE;
 * n == 0 does nothing.
 *
 * Like qs_step_many it runs up to QS_MAX_FUSED_STEPS steps to a launch with the
 * state on-chip in between.  A launch reads the action rows of all its steps
 * into LDS before its first step runs, 256 · A bytes per step and workgroup, so
 * its depth is capped further where that would keep the launch's workgroups
 * from being resident at once (MultiHover, 16 384 envs × 8 drones, A = 1: 19).
 * Steps share a launch while
 *  - their outputs are disjoint across steps (as in qs_step_many),
 *  - a step's actions overlap no output of an earlier step of the launch, and
 *  - a step's outputs overlap no actions of an earlier step of the launch;
 * the launch is cut before a step that breaks one of these, which restores the
 * order of single steps: feeding step j's actions_out (or obs) to step j + 1
 * works, one step per launch.  Steps may read the same actions.  Handles that
 * run the deferred reset search after each step take one step per launch, and
 * so do the Flock / Meetup / LeaderFollower tasks (their multi-step kernels
 * round the env reward 1 ulp apart from the single step's). */
int qs_step_seq(qs_handle* h, int n, const float* const* actions,
                const qs_step_out* outs, void* stream);

/* Branch rollouts: C candidate action sequences of n steps each, all from the
 * handle's current state, in one launch that leaves the handle as it was (what a
 * sampling planner does once per control tick).  The launch runs C · E virtual
 * envs, virtual env c · E + e starting from the state of env e, so it fills
 * wavefronts whatever E is.  (New entry points of ABI 4, like qs_step_seq.)
 *
 * actions: a host array of n device pointers, read during the call, each
 * [C][E][D][A] float32.  outs: n sets of step outputs or NULL, every buffer
 * sized for C · E envs (obs [C][E][D][O], reward [C][E], ...).  score: the
 * per-candidate summary below, or NULL.
 *
 *  - Equivalence.  For every candidate c the per-step outputs equal, bit for
 *    bit, what qs_step_seq(h', n, actions[.][c], outs', stream) writes on a
 *    handle h' whose four state blocks equal h's at the time of the call,
 *    auto-resets inside the candidate included: the reset draw is keyed on the
 *    source env's global id and episode counter, so it is the same in every
 *    candidate.  QS_FLAG_NO_AUTORESET handles are included.
 *  - No mutation.  h is not advanced: agent state, env record, history ring,
 *    episode return, episode log (records and total), reset-error flag and
 *    qs_launch_counts are unchanged byte for byte after the call.
 *  - Optional outputs.  Every pointer in outs[j] may be NULL, outs may be NULL,
 *    and score or either of its members may be NULL; a call with nothing to
 *    write is QS_E_INVALID.
 *  - Alignment.  Actions need 4-byte alignment only, and steps may share action
 *    buffers.  No output may overlap another output or any action buffer
 *    (QS_E_INVALID).  Nothing is cut into several launches: qs_score keeps no
 *    branch state between launches (a branch set does: qs_branch_advance).
 *  - Depth.  1 <= n <= qs_score_depth(h): 32, lowered only where the steps'
 *    action rows (256 · A bytes per step and workgroup) plus the kernel's other
 *    LDS would pass the 64 KB a workgroup of the action-sequence launches may
 *    take.  It depends neither on C nor on QS_MAX_FUSED_STEPS.  Longer horizons
 *    are refused here, not approximated: chain qs_branch_advance calls on a
 *    branch set (qs_branch_create) for them.
 *  - Handles that cannot score: qs_score_depth returns 0 and qs_score
 *    QS_E_INVALID with a message for handles that run the deferred reset search
 *    after each step (MultiHover layouts whose reset draws can be rejected) and
 *    for the Flock / Meetup / LeaderFollower tasks (their multi-step kernels
 *    round the env reward 1 ulp apart from the single step's).
 *  - Other refusals.  C < 1, n out of range or a NULL among actions[]:
 *    QS_E_INVALID; C · E · D too large for the 32-bit offsets of a requested
 *    output: QS_E_INVALID; a call before qs_reset: QS_E_STATE.
 *  - Capture.  Like every other call on the handle it ends the kernel node a
 *    captured qs_step was growing; the call itself may be captured. */
typedef struct qs_score_out {
  void* ret;           /* [C][E] double: sum, in step order and in double, of
                          the (real) rewards of steps 0..jd, jd = the candidate's
                          first step with terminated|truncated for that env, or
                          n-1 if none                                          */
  int32_t* first_done; /* [C][E]: jd, or n if the env was never done in the
                          candidate                                            */
} qs_score_out;

/* Largest n one qs_score call takes on this handle (0: the handle cannot
 * score).  Host only. */
int qs_score_depth(const qs_handle* h);

int qs_score(qs_handle* h, int n, int C, const float* const* actions,
             const qs_step_out* outs, const qs_score_out* score, void* stream);

/* qs_score plus each drone's own share of the return.  (A new entry point of
 * ABI 4, like qs_step_seq.)  ret_agent: device, [C][E][D] double, or NULL.
 *
 * MultiHover and Spiral form a step's env reward as the mean of D per-drone
 * terms.  ret_agent[c][e][d] is the sum, in step order and in double, of drone
 * d's term (in the handle's precision, widened) BEFORE the division by D, over
 * steps 0..jd with jd as in qs_score_out.ret: the launch's own numbers, kept per
 * lane and written once.
 *
 *  - ret_agent == NULL: the call is qs_score, in results and refusals.
 *  - Every other output is, byte for byte, what qs_score writes; ret_agent is the
 *    same bytes whatever else is requested.
 *  - ret_agent counts as an output: it alone is something to write, and it may
 *    not overlap an action buffer or another output (QS_E_INVALID).  C · E · D · 8
 *    bytes past the 32-bit offsets: QS_E_INVALID.
 *  - No mutation, depth, capture and the handles that cannot score: as qs_score.
 *  - Scale.  ret[c][e] is about sum_d ret_agent[c][e][d] / D (the env reward
 *    rounds the mean at every step), so a temperature or a penalty meant per
 *    drone is on a scale D times the env-level one.
 *  - Meaning.  A drone's term depends on its own actions alone only where drones
 *    do not act on each other: with QS_AUX_DW (downwash) or PYB contacts another
 *    drone's actions move it too, and weighting by ret_agent is an approximation. */
int qs_score_agents(qs_handle* h, int n, int C, const float* const* actions,
                    const qs_step_out* outs, const qs_score_out* score,
                    double* ret_agent, void* stream);

/* Branch sets: branch rollouts that persist.  A branch set owns the state of
 * C · E virtual envs (virtual env v = c · E + e, as in qs_score), so a rollout can
 * go on from one launch to the next, be forked from the handle again, or be
 * resampled: horizons past qs_score_depth, beam search, particle planners.  (New
 * entry points of ABI 4, like qs_step_seq.)
 *
 * A branch set is bound to one handle, which must outlive it, and owns its device
 * memory: the agent block [QS_AGENT_FIELDS][C · E · D] in the handle's precision,
 * the four env fields of QS_STATE_ENV per virtual env, the action-history ring
 * [H][C · E · D][A] and the three accumulators below (and as much again, which
 * qs_branch_select gathers into).  It keeps no episode log, no reset-error flag
 * and no episode returns: nothing in a branch reads them.  Every call but create /
 * destroy / buffers / steps is stream-ordered and asynchronous, reads nothing
 * back to the host and may be captured into a graph.  Like a handle, a branch set
 * is used from one host thread at a time.
 *
 *  - qs_branch_fork.  Every candidate of env e becomes a copy of the handle's env
 *    e (agent state, env counters, history ring) as the handle is at that point
 *    of the stream: a snapshot, which later steps of the handle do not change.
 *    ret and ret_agent become 0, first_done 0 and steps 0.  QS_E_STATE before
 *    qs_reset.
 *  - qs_branch_advance.  n steps, 1 <= n <= qs_score_depth(h), in one launch:
 *    the qs_score launch with the state loaded from the set and stored back to
 *    it.  actions[j]: [C][E][D][A] float32; outs: NULL, or n sets of step outputs
 *    over C · E envs, laid out exactly as for qs_score (every pointer optional;
 *    outs == NULL is valid here, since the state and the accumulators are
 *    written).  For every candidate the per-step outputs of a chain of advances
 *    equal, bit for bit, what qs_step_seq writes on a handle that started from
 *    the forked state and ran the candidate's actions; the reset draws inside a
 *    branch are keyed on the source env's global id (env_offset + e) and the
 *    branch's own episode counter.  qs_score's alignment, overlap and 32-bit
 *    size rules hold, and no named buffer may lie in the set's own memory.  Call
 *    it any number of times: that is how the horizon grows.  QS_E_STATE before
 *    the first fork.
 *  - Accumulators.  With t = steps before the call, an env of a candidate is
 *    live iff first_done == t.  While live, ret += (double)reward in step order
 *    and each drone's ret_agent grows by its own term, exactly as in
 *    qs_score_agents; first_done becomes the index since the fork of the first
 *    done step, or t + n if there is still none.  After its first done step the
 *    env keeps stepping (and resets, with auto-reset on, as in qs_score) and
 *    its accumulators are frozen.  A chain of total length <= qs_score_depth
 *    therefore writes the same bytes as one qs_score_agents call.
 *  - qs_branch_select.  parent: device int32 [C][E].  The new candidate c of env
 *    e takes the state and the three accumulators of the old candidate
 *    parent[c][e] of the same env; a value outside 0 .. C-1 keeps candidate c.
 *    All candidates read the old set, so duplicates and permutations are both
 *    well defined.  steps is unchanged, and the pointers of qs_branch_buffers
 *    stay valid and current (the gather goes into the set's second allocation
 *    and is copied back on the device, on every replay of a captured call).
 *    QS_E_STATE before the first fork.
 *  - qs_branch_state.  Copies QS_STATE_AGENT ([fields][C · E · D]), QS_STATE_ENV
 *    ([4][C · E] int32) or QS_STATE_HISTORY ([H][C · E · D][A]) into buf (device);
 *    QS_STATE_EP_RETURN: QS_E_INVALID.
 *  - qs_branch_steps.  Host only: the steps advanced since the last fork, as
 *    counted when the calls were made.  A captured advance carries the step index
 *    of its capture, so a graph should hold the fork that its advances follow.
 *  - No mutation.  No call changes the handle: its four state blocks, episode
 *    log (records and total), reset-error flag, qs_launch_counts and
 *    qs_ring_counts are byte for byte as before, as qs_score guarantees.  Like
 *    any call on the handle, a branch call ends a growing captured qs_step node.
 *  - Refusals (QS_E_INVALID with a message, nothing launched, *out untouched on
 *    create): a handle with qs_score_depth(h) == 0; C < 1; a block of C · E · D
 *    agents past the 32-bit offsets; n out of range; a NULL among actions[]; an
 *    output that overlaps another output or an action buffer.                  */
typedef struct qs_branch_bufs { /* device pointers owned by the set, stable until
                                   qs_branch_destroy                             */
  double* ret;          /* [C][E]    rewards up to the first done step, in double */
  int32_t* first_done;  /* [C][E]    that step's index since the fork, or steps   */
  double* ret_agent;    /* [C][E][D] each drone's own terms, as qs_score_agents   */
} qs_branch_bufs;

typedef struct qs_branch qs_branch;

int qs_branch_create(qs_handle* h, int C, qs_branch** out);
int qs_branch_destroy(qs_branch* b);
int qs_branch_buffers(const qs_branch* b, qs_branch_bufs* out);
int qs_branch_steps(const qs_branch* b, int64_t* out);
int qs_branch_fork(qs_branch* b, void* stream);
int qs_branch_advance(qs_branch* b, int n, const float* const* actions,
                      const qs_step_out* outs, void* stream);
int qs_branch_select(qs_branch* b, const int32_t* parent, void* stream);
int qs_branch_state(qs_branch* b, int block, void* buf, void* stream);

/* MPPI planner tick on top of qs_score: sample C candidate sequences round a
 * nominal one, score them from the handle's current state, and fold them back
 * into the nominal by their softmax weights, all on the device.  (New entry
 * points of ABI 4, like qs_step_seq.)
 *
 * A planner is bound to one handle, which must outlive it, and owns its device
 * buffers (qs_mppi_buffers; stable until qs_mppi_destroy).  Every call but
 * create / destroy / buffers is stream-ordered and asynchronous, reads nothing
 * back to the host and may be captured into a graph; the tick counter lives on
 * the device, so a replayed graph draws new noise each time.  No float atomics:
 * the same inputs give the same bytes.  Like a handle, a planner is used from
 * one host thread at a time.
 *
 *  - qs_mppi_sample.  One Philox4x32-10 call per (step j, candidate c, env e,
 *    drone d): key = seed, counter = (low word of *tick, env_offset + e,
 *    c · 32 + j, (3 << 24) | d).  Word i gives u_i = ((x_i >> 8) + 1) · 2^-24 in
 *    (0, 1]; z0, z1 = sqrt(-2 ln u0) · (cos, sin)(2π u1) and z2, z3 likewise from
 *    u2, u3 (float32).  candidates[j][0][e][d][a] = nominal[j][e][d][a] as it is;
 *    for c > 0, clamp(nominal + sigma[a] · z_a, lo, hi), the sum left out where
 *    sigma[a] = 0.  The counter holds the global env id, so the noise does not
 *    depend on how envs are sharded.
 *  - qs_mppi_update.  Per env e, in double: s_c = ret[c][e] - (first_done[c][e]
 *    < n ? done_penalty : 0); best[e] = the lowest c with the largest s;
 *    lambda > 0: weights[c][e] = exp((s_c - s_best) / lambda) / sum over c;
 *    lambda = 0: 1 at best, 0 elsewhere.  new[j] = (float) sum over c of
 *    weights[c] · candidates[j][c] (lambda = 0: the best candidate's row, bit for
 *    bit); action = new[0]; nominal[j] = new[j + 1] for j < n - 1 and
 *    nominal[n - 1] = new[n - 1] (hold); *tick += 1.  Two launches.  It reads
 *    candidates, ret and first_done as they are: a caller may fill them itself.
 *  - qs_mppi_plan = sample, qs_score(h, n, C, candidates, NULL, {ret,
 *    first_done}), update.  QS_E_STATE before qs_reset, with nothing launched.
 *    (With a value attached the middle stage is qs_value_mppi_score, below.)
 *  - qs_mppi_reset copies `nominal` (device, [n][E][D][A]; NULL: zeros) into the
 *    planner and sets *tick = 0.  A new planner is in that state with zeros.
 *  - qs_mppi_create refusals (QS_E_INVALID, *out untouched): a handle with
 *    qs_score_depth(h) = 0, horizon outside 1 .. qs_score_depth(h), candidates
 *    < 2 or > 2^27, lo >= hi, a negative or non-finite sigma, lambda or
 *    done_penalty, and sizes beyond the 32-bit offsets qs_score refuses.       */
typedef struct qs_mppi_spec {
  int32_t horizon;      /* n: 1 .. qs_score_depth(h)                              */
  int32_t candidates;   /* C >= 2; candidate 0 is the nominal itself, unperturbed */
  float sigma[4];       /* noise std per action component (first A used), >= 0    */
  float lo, hi;         /* candidates are clipped to [lo, hi]; lo < hi            */
  double lambda;        /* temperature; 0 = greedy (arg max, lowest c on ties)    */
  double done_penalty;  /* subtracted from a candidate's score for env e when its
                           first_done[c][e] < n                                   */
  uint64_t seed;
} qs_mppi_spec;

typedef struct qs_mppi_bufs { /* device pointers owned by the planner; per-drone
                                 mode (qs_pd_mppi_create): weights [C][E][D],
                                 best [E][D]                                   */
  float* nominal;       /* [n][E][D][A]                                          */
  float* candidates;    /* [n][C][E][D][A]  (what qs_score reads)                */
  double* ret;          /* [C][E]  qs_score's ret                                */
  int32_t* first_done;  /* [C][E]                                                */
  double* weights;      /* [C][E]  normalised; greedy: 1 at best, 0 elsewhere    */
  int32_t* best;        /* [E]     arg max of the penalised score, lowest c      */
  float* action;        /* [E][D][A] the first step of the updated nominal       */
  uint64_t* tick;       /* [1]     device counter, +1 per update                 */
} qs_mppi_bufs;

typedef struct qs_mppi qs_mppi;

int qs_mppi_create(qs_handle* h, const qs_mppi_spec* spec, qs_mppi** out);
int qs_mppi_destroy(qs_mppi* p);
int qs_mppi_buffers(const qs_mppi* p, qs_mppi_bufs* out);
int qs_mppi_reset(qs_mppi* p, const float* nominal, void* stream);
int qs_mppi_sample(qs_mppi* p, void* stream);
int qs_mppi_update(qs_mppi* p, void* stream);
int qs_mppi_plan(qs_mppi* p, void* stream);

/* CEM (cross-entropy method) planner tick on top of qs_score: per env, I
 * iterations of "sample C candidate sequences round a mean with a per-element
 * spread, score them from the handle's current state, refit mean and spread to
 * the K best", all on the device.  (New entry points of ABI 4, like qs_mppi_*.)
 *
 * A planner is bound to one handle, which must outlive it, and owns its device
 * buffers (qs_cem_buffers; stable until qs_cem_destroy).  Every call but
 * create / destroy / buffers is stream-ordered and asynchronous, reads nothing
 * back to the host and may be captured into a graph; the tick counter lives on
 * the device, so a replayed graph draws new noise each time.  No float atomics
 * and every sum in a fixed order: the same inputs give the same bytes.  Like a
 * handle, a planner is used from one host thread at a time.  Every env plans
 * independently of the others.
 *
 *  - qs_cem_begin.  std[j][e][d][a] = sigma[a] everywhere: the spread restarts
 *    at every tick, only the mean carries over.
 *  - qs_cem_sample(p, i).  One Philox4x32-10 call per (step j, candidate c, env
 *    e, drone d): key = seed, counter = (low word of *tick, env_offset + e,
 *    c · 32 + j, (4 << 24) | (i << 8) | d).  Word k gives u_k = ((x_k >> 8) + 1) ·
 *    2^-24 in (0, 1]; z0, z1 = sqrt(-2 ln u0) · (cos, sin)(2π u1) and z2, z3
 *    likewise from u2, u3 (float32): qs_mppi_sample's construction under domain
 *    tag 4, with the iteration above the drone index.  candidates[j][0][e][d][a]
 *    = mean[j][e][d][a] as it is; for c > 0, clamp(mean + std · z_a, lo, hi),
 *    mean and std at [j][e][d][a], the sum left out (the mean copied) where that
 *    std is 0.  The counter holds the global env id, so the noise does not depend
 *    on how envs are sharded; iterations, ticks, envs, candidates, steps and
 *    drones never share a counter.
 *  - qs_cem_refit(p, i).  Per env e, in double: s_c = ret[c][e] -
 *    (first_done[c][e] < n ? done_penalty : 0).  Candidates are ranked by the
 *    total order "larger s first, lower c on equal s": -0.0 and 0.0 are equal,
 *    -inf is a number, and a NaN ranks after every number, lower c first among
 *    NaNs.  elites[r][e] = the candidate of rank r for r < K; iter_best[i][e] =
 *    s of rank 0.  For every (j, d, a), with x_r = candidates[j][elites[r][e]][e]
 *    [d][a]: m = (1/K) sum_r x_r and v = (1/K) sum_r (x_r - m)^2 (two passes,
 *    population variance), in double and in a fixed order; mean = (float)((1 -
 *    alpha) · m + alpha · (double)mean) and std = max((float)((1 - alpha) · sqrt(v) +
 *    alpha · (double)std), sigma_min[a]); with alpha = 0 the old values are not
 *    read.  Where sigma[a] = 0 the std is left as it is (0 after begin).  Two
 *    launches.  It reads candidates, ret and first_done as they are: a caller
 *    may fill them itself.
 *  - qs_cem_finish.  action = mean[0]; mean[j] = mean[j + 1] for j < n - 1 and
 *    mean[n - 1] holds; *tick += 1 (once a tick, not once an iteration).
 *  - qs_cem_plan = begin, I × (sample(i), qs_score(h, n, C, candidates, NULL,
 *    {ret, first_done}), refit(i)), finish.  QS_E_STATE before qs_reset, with
 *    nothing launched.  (With a value attached the scoring of every iteration is
 *    qs_value_cem_score, below.)
 *  - qs_cem_reset copies `mean` (device, [n][E][D][A]; NULL: zeros) into the
 *    planner and sets *tick = 0.  A new planner is in that state with zeros.
 *  - qs_cem_sample / qs_cem_refit with an iteration outside 0 .. I - 1:
 *    QS_E_INVALID, nothing launched.
 *  - qs_cem_create refusals (QS_E_INVALID, *out untouched): a handle with
 *    qs_score_depth(h) = 0, horizon outside 1 .. qs_score_depth(h), candidates
 *    < 2 or > 2^27, elites < 1, > candidates or > 1024, iterations outside
 *    1 .. 16, lo >= hi or non-finite, a negative or non-finite sigma, sigma_min,
 *    alpha or done_penalty, alpha >= 1, sigma_min[a] > sigma[a], and sizes beyond
 *    the 32-bit offsets qs_score refuses.                                       */
typedef struct qs_cem_spec {
  int32_t horizon;      /* n: 1 .. qs_score_depth(h)                              */
  int32_t candidates;   /* C >= 2; candidate 0 is the mean itself, unperturbed    */
  int32_t elites;       /* K: 1 .. min(C, 1024)                                   */
  int32_t iterations;   /* I: 1 .. 16                                             */
  float sigma[4];       /* the spread every tick starts from, per action
                           component (first A used), >= 0; 0: never perturbed     */
  float sigma_min[4];   /* floor of the refitted spread, 0 <= sigma_min <= sigma  */
  float lo, hi;         /* candidates are clipped to [lo, hi]; lo < hi            */
  double alpha;         /* smoothing in [0, 1): the share of the old mean / std   */
  double done_penalty;  /* subtracted from a candidate's score for env e when its
                           first_done[c][e] < n                                   */
  uint64_t seed;
} qs_cem_spec;

typedef struct qs_cem_bufs {  /* device pointers owned by the planner; per-drone
                                 mode (qs_pd_cem_create): elites [K][E][D],
                                 iter_best [I][E][D]                           */
  float* mean;          /* [n][E][D][A]                                          */
  float* std;           /* [n][E][D][A]                                          */
  float* candidates;    /* [n][C][E][D][A]  (what qs_score reads)                */
  double* ret;          /* [C][E]  qs_score's ret                                */
  int32_t* first_done;  /* [C][E]                                                */
  int32_t* elites;      /* [K][E]  the K best candidates of the last refit, in
                           rank order                                            */
  double* iter_best;    /* [I][E]  the best penalised score of each iteration    */
  float* action;        /* [E][D][A] mean[0] as finish found it                  */
  uint64_t* tick;       /* [1]     device counter, +1 per finish                 */
} qs_cem_bufs;

typedef struct qs_cem qs_cem;

int qs_cem_create(qs_handle* h, const qs_cem_spec* spec, qs_cem** out);
int qs_cem_destroy(qs_cem* p);
int qs_cem_buffers(const qs_cem* p, qs_cem_bufs* out);
int qs_cem_reset(qs_cem* p, const float* mean, void* stream);
int qs_cem_begin(qs_cem* p, void* stream);
int qs_cem_sample(qs_cem* p, int iteration, void* stream);
int qs_cem_refit(qs_cem* p, int iteration, void* stream);
int qs_cem_finish(qs_cem* p, void* stream);
int qs_cem_plan(qs_cem* p, void* stream);

/* Per-drone (factored) planner ticks.  qs_pd_mppi_create / qs_pd_cem_create take
 * the same spec records and return the same planner types, driven by the same
 * qs_mppi_* / qs_cem_* calls, in per-drone mode: every drone weighs (MPPI) or
 * ranks (CEM) the same C candidates by its own return, so C candidates serve D
 * searches at once.  (New entry points of ABI 4.)
 *
 * The semantics are the env-level ones above with agent (e, d) in the place of
 * env e and the drone's A components in the place of the env's D · A:
 *  - Score.  s[c][e][d] = ret_agent[c][e][d] - (first_done[c][e] < n ?
 *    done_penalty : 0): the penalty comes from the env's first_done.
 *  - Buffers.  The planner owns ret_agent [C][E][D] (qs_pd_*_ret_agent); weights
 *    is [C][E][D], best [E][D], elites [K][E][D], iter_best [I][E][D].  ret and
 *    first_done keep their shape and are still filled.
 *  - MPPI.  best[e][d] = the lowest c of the largest s; w = softmax over c at
 *    temperature lambda; new[j][e][d][a] = (float) sum_c w[c][e][d] ·
 *    candidates[j][c][e][d][a], summed in double in the env-level order.  With
 *    lambda = 0 the best candidate's [d][.] slice is copied bit for bit, so the
 *    drones of one env may copy different candidates.  Shift, action and tick as
 *    before.
 *  - CEM.  Ranking (the same total order), the K elites, the two-pass refit,
 *    alpha, sigma_min and iter_best per (e, d) over that drone's A components.
 *  - Sampling is unchanged: the same Philox counters and the same bytes as the
 *    env-level planner of the same spec, seed and tick; candidate 0 is the
 *    nominal / mean for every drone.
 *  - plan() scores with qs_score_agents(h, n, C, candidates, NULL, {ret,
 *    first_done}, ret_agent, stream).  update / refit read candidates, ret_agent
 *    and first_done as they are, so a caller may fill them itself.
 *  - Scale.  ret is about sum_d ret_agent / D: a per-drone lambda or
 *    done_penalty is on a scale D times the env-level one.
 *  - Meaning.  Per-drone weighting is exact only where a drone's term depends on
 *    its own actions; with QS_AUX_DW or contacts it is an approximation.
 *  - Refusals (QS_E_INVALID, *out untouched): whatever qs_mppi_create /
 *    qs_cem_create refuse, and C · E · D · 8 bytes of ret_agent or E · D · n
 *    workgroups at 2^31 or more.  qs_pd_*_ret_agent on an env-level planner:
 *    QS_E_INVALID.                                                              */
int qs_pd_mppi_create(qs_handle* h, const qs_mppi_spec* spec, qs_mppi** out);
int qs_pd_mppi_ret_agent(const qs_mppi* p, double** out);
int qs_pd_cem_create(qs_handle* h, const qs_cem_spec* spec, qs_cem** out);
int qs_pd_cem_ret_agent(const qs_cem* p, double** out);

/* Value tail: discounted, critic-bootstrapped returns for the MPPI and CEM ticks.
 * (New entry points of ABI 4.)  With a value attached, a planner's score stage
 * turns qs_score's undiscounted sum into the n-step bootstrapped return
 *
 *   G(c, e) = sum_{j <= jd} gamma^j · r_j  +  [first_done == n] · gamma^n · scale · V(s_n)
 *
 * where V is a tanh MLP with two hidden layers of `hidden` units and one output
 * (the trainer's centralized critic) over the D · O concatenated obs of the env.
 *
 *  - The tail is ONE launch after the score launch, over the V = C · E virtual
 *    envs: row v = c · E + e is last_obs[c][e][.][.], the obs the score launch wrote
 *    for step n - 1 (post auto-reset; for a candidate that was never done it is
 *    the true s_n).  With obs_mean / obs_var every input column i becomes
 *    clamp((x - mean[i]) / sqrt(var[i] + eps), -clip, clip), evaluated in double
 *    and rounded to float (qs_rms_normalize's expression).  H1 = tanh(X · W1^T +
 *    b1), H2 = tanh(H1 · W2^T + b2), V = H2 · w3^T + b3 on the f32-input MFMA, the
 *    activations kept on-chip.  The weights are torch nn.Linear tensors (w1
 *    [hidden][in_dim], w2 [hidden][hidden], w3 [1][hidden], float32, contiguous),
 *    read from the caller's pointers AT EVERY LAUNCH: there is no pack step, so a
 *    critic updated in place is seen by the next tick and by a replayed graph.  The
 *    caller keeps them alive while the value is attached.
 *  - value[c][e] (float) is written for every row, whatever first_done says.
 *  - The fold, in double, in place, with disc[0] = 1, disc[j] = disc[j - 1] · gamma
 *    formed on the host and jd = first_done[c][e]: acc = 0; for j = 0 .. min(jd,
 *    n - 1) in order acc = acc + disc[j] · (double) r_j[c][e]; if jd == n, acc = acc
 *    + (disc[n] · scale) · (double) V; ret[c][e] = acc.  No multiply-add is
 *    contracted.  With gamma = 1 no per-step rewards are requested and the sum is
 *    the score launch's own ret: only the bootstrap term is added.  With gamma = 1
 *    and no net there is nothing to do and nothing is launched.  No atomics and a
 *    fixed summation order: the same inputs give the same bytes.
 *  - A truncated candidate counts as ended, like a terminated one: its return
 *    stops at the done step and it gets no bootstrap from terminal_obs.
 *  - The critic must have been trained at the same norm_obs setting as the spec
 *    (with the normaliser if obs_mean / obs_var are given, without it if not), and
 *    `scale` undoes a reward normalisation the critic was trained under.
 *  - Everything downstream reads ret as before: done_penalty still applies where
 *    first_done < n.
 *
 * qs_value_tail is that launch on caller-owned buffers, bound to no handle (for
 * callers who compose qs_score themselves).  last_obs [C][E][D][O] float and
 * value_out [C][E] float are needed with a net; rewards is a host array of n
 * device pointers, each [C][E] reals of real_bytes (4 or 8), needed with gamma !=
 * 1 and not read otherwise; ret [C][E] double and first_done [C][E] int32 always.
 * It runs on the current device.  1 <= n <= 32.
 *
 * qs_value_mppi_set / qs_value_cem_set copy the spec (NULL detaches the value)
 * and allocate the planner's last_obs and value (with a net) and rewards
 * [n][C][E] in the handle's precision (with gamma != 1); qs_value_*_buffers
 * returns the three pointers, NULL where a buffer does not exist.  Both are host
 * calls that may synchronise the device: do not capture them.  qs_value_mppi_score /
 * qs_value_cem_score is the scoring stage of plan() as its own call, next to sample /
 * update / refit: qs_score into the planner's ret / first_done, which with a value
 * attached also names outs[n - 1].obs = last_obs and, for gamma != 1, outs[j].reward
 * = rewards[j], followed by the tail.  Without a value it is exactly the qs_score
 * call plan() made before.  QS_E_STATE before qs_reset.
 *
 * Refusals (QS_E_INVALID with a message; nothing is allocated and the planner is
 * as it was): a per-drone planner (a centralized critic has one value per env);
 * in_dim != D · O or > 1024; hidden outside {64, 128, 256}; a net that is partly
 * NULL; one of obs_mean / obs_var without the other, or either without a net;
 * gamma outside (0, 1]; a non-finite scale; last_obs (C · E · D · O · 4 bytes) past
 * the 32-bit offsets.  The particle tick (qs_smc_*) takes no value: its weights
 * are increments since the last resampling step.                                */
typedef struct qs_value_spec {
  int32_t in_dim;            /* I, must equal D · O of the handle, <= 1024            */
  int32_t hidden;            /* N: 64, 128 or 256                                   */
  const float *w1, *b1, *w2, *b2, *w3, *b3;   /* device; all NULL: no net (discount only) */
  const double *obs_mean, *obs_var;           /* device [I], both or neither         */
  double obs_eps, obs_clip;
  double gamma;              /* 0 < gamma <= 1                                       */
  double scale;              /* finite; multiplies V (reward-normalised critics)     */
} qs_value_spec;

int qs_value_tail(const qs_value_spec* spec, int n, int C, int E, int D, int O, int real_bytes, const float* last_obs,
                  const void* const* rewards, double* ret, const int32_t* first_done, float* value_out, void* stream);
int qs_value_mppi_set(qs_mppi* p, const qs_value_spec* spec);
int qs_value_mppi_buffers(const qs_mppi* p, float** last_obs, float** value, void** rewards);
int qs_value_mppi_score(qs_mppi* p, void* stream);
int qs_value_cem_set(qs_cem* p, const qs_value_spec* spec);
int qs_value_cem_buffers(const qs_cem* p, float** last_obs, float** value, void** rewards);
int qs_value_cem_score(qs_cem* p, void* stream);

/* Policy prior of the MPPI and CEM ticks: `count` = K of a planner's C candidates
 * per env are closed-loop rollouts of the trainer's actor from the handle's
 * current state, so that the ordinary weighting / ranking decides among them and
 * the sampled candidates and the plan is never worse, on the model, than the
 * policy.  (New entry points of ABI 4, like qs_value_*.)
 *
 *  - The actor launch is ONE launch over the R = K · E · D rows of a step: row
 *    r = (k · E + e) · D + d reads its O = in_dim floats of obs (with bcast != 0
 *    from row r mod (E · D): the caller's [E][D][O] obs for every trajectory).
 *    With obs_mean / obs_var (the trainer's normaliser over an env's [D][O] obs:
 *    D · O entries) column i of drone d becomes clamp((x - mean[d · O + i]) /
 *    sqrt(var[d · O + i] + eps), -clip, clip), evaluated in double and rounded to
 *    float (qs_rms_normalize's expression).  H1 = tanh(X · W1^T + b1), H2 = tanh(H1 ·
 *    W2^T + b2) on the f32-input MFMA, the activations kept on-chip, out = H2 ·
 *    W3^T in float in a fixed order, mean = action_scale · (out + b3).  Trajectory
 *    k >= 1 adds std_scale · exp(logstd[a]) · z_a, z the Box-Muller normals of
 *    qs_mppi_sample drawn from Philox4x32-10(key = seed, counter = (tick, genv0 +
 *    e, k · 32 + j, (7 << 24) | d)); trajectory 0 is the mode.  The result is
 *    clipped to [lo, hi] and stored to actions_out[k][e][d][.]; the raw obs row is
 *    copied to obs_seen[k][e][d][.] (NULL: no copy; it must not be obs_in).
 *  - The weights are torch nn.Linear tensors (w1 [hidden][in_dim], w2
 *    [hidden][hidden], w3 [act_dim][hidden], logstd [act_dim], float32,
 *    contiguous).  They, logstd and the statistics are read from the caller's
 *    pointers AT EVERY LAUNCH: there is no pack step, so an actor updated in place
 *    is seen by the next tick and by a replayed graph.  The caller keeps them, and
 *    `obs`, alive while the prior is attached.  No atomics: the same inputs give
 *    the same bytes.
 *  - qs_prior_act is that launch for step j on caller-owned buffers, bound to no
 *    handle (spec->obs and spec->count are not read: obs_in and K are).  tick:
 *    device uint64, read as qs_mppi_sample reads the planner's.  It runs on the
 *    current device.  0 <= j < 32, D <= 256.
 *  - qs_prior_mppi_set / qs_prior_cem_set copy the spec (NULL detaches the prior),
 *    create a branch set of K candidates that the planner owns and allocate
 *    prior_actions [n][K][E][D][A] and prior_obs [n][K][E][D][O] (float32);
 *    qs_prior_*_buffers returns the two pointers, NULL without a prior.  Both are
 *    host calls that may synchronise the device: do not capture them.
 *  - qs_prior_mppi_rollout / qs_prior_cem_rollout is the prior stage on its own:
 *    qs_branch_fork of the planner's set, then for j = 0 .. n - 1 the actor launch
 *    reading obs slot j (step 0: spec->obs, broadcast, and copied to slot 0) and
 *    writing prior_actions[j], and for j < n - 1 a one-step qs_branch_advance with
 *    prior_actions[j] whose obs output is slot j + 1: 2 n launches, stream-ordered,
 *    no host sync, capturable, keyed on the planner's seed, the global env id and
 *    the device tick counter, clipped to the planner's [lo, hi].  spec->obs is the
 *    caller's [E][D][O] obs of the handle's current state (the buffer it passes as
 *    qs_step_out.obs, and qs_reset's obs at first), read at every tick and never
 *    copied.  The handle is not changed.  QS_E_STATE before qs_reset or without a
 *    prior.
 *  - With a prior attached qs_mppi_plan runs the stage first and qs_cem_plan runs
 *    it once per tick after begin, and every qs_mppi_sample / qs_cem_sample is
 *    followed by one inject launch that copies prior_actions[j] over candidates
 *    C - K .. C - 1 of step j.  Candidate 0 stays the nominal / mean; score, value
 *    tail, update / refit and the per-drone variants are unchanged.  Without a
 *    prior a planner launches and writes exactly what it did before.
 *
 * Refusals (QS_E_INVALID with a message; nothing is allocated and the planner is
 * as it was): count outside 1 .. C - 1; a net (w1 .. b3, logstd) that is partly
 * NULL; hidden outside {64, 128, 256}; in_dim != obs_dim or > 1024; act_dim != the
 * handle's; one of obs_mean / obs_var without the other; a NULL obs; std_scale not
 * finite or negative, action_scale not finite; a step's obs (K · E · D · O · 4 bytes)
 * past the 32-bit offsets; what qs_branch_create refuses.  The particle tick
 * (qs_smc_*) takes no prior: its particles are resampled mid-horizon, which a
 * closed-loop trajectory fixed before the tick cannot follow.                    */
typedef struct qs_prior_spec {
  int32_t in_dim;            /* O, must equal obs_dim of the handle, <= 1024         */
  int32_t hidden;            /* N: 64, 128 or 256                                   */
  int32_t act_dim;           /* A, must equal act_dim of the handle, <= 4            */
  const float *w1, *b1, *w2, *b2, *w3, *b3;   /* device; the actor's pi_net          */
  const float* logstd;       /* device [A]                                          */
  float action_scale;        /* finite; multiplies the net's output                 */
  float std_scale;           /* finite, >= 0; multiplies exp(logstd) (0: no noise)   */
  const double *obs_mean, *obs_var;           /* device [D · O], both or neither     */
  double obs_eps, obs_clip;
  int32_t count;             /* K: 1 .. candidates - 1 prior candidates per env      */
  const float* obs;          /* device [E][D][O]: the obs of the handle's state      */
} qs_prior_spec;

int qs_prior_act(const qs_prior_spec* spec, int j, int K, int E, int D, float lo, float hi, uint64_t seed, int64_t genv0,
                 const uint64_t* tick, const float* obs_in, int bcast, float* actions_out, float* obs_seen, void* stream);
int qs_prior_mppi_set(qs_mppi* p, const qs_prior_spec* spec);
int qs_prior_mppi_buffers(const qs_mppi* p, float** prior_actions, float** prior_obs);
int qs_prior_mppi_rollout(qs_mppi* p, void* stream);
int qs_prior_cem_set(qs_cem* p, const qs_prior_spec* spec);
int qs_prior_cem_buffers(const qs_cem* p, float** prior_actions, float** prior_obs);
int qs_prior_cem_rollout(qs_cem* p, void* stream);

/* Sampling spec of the MPPI, CEM and particle ticks: time-correlated noise for all
 * three, and for the CEM tick an elite memory (iCEM, Pinneri et al. 2020).  An
 * attachable spec like the value tail and the prior; a planner that never had one
 * launches and writes exactly what it did before, and so does one with the all-zero
 * spec.  (New entry points of ABI 4, like qs_prior_*.)
 *
 *  - Correlated noise.  Let xi_j be the float32 normal that qs_mppi_sample /
 *    qs_cem_sample / qs_smc_sample form for step j of candidate c > 0, env e, drone
 *    d, component a (the same Philox key and counter, the same u_k and Box-Muller
 *    pairs).  With a spec attached the noise of component a is
 *      eps_0 = xi_0,   eps_j = rho[a] · eps_{j-1} + s_a · xi_j   (j >= 1),
 *    s_a = (float)sqrt(1 - (double)rho[a]^2) formed once on the host, the two
 *    products and the sum each rounded to float32 (no multiply-add is contracted).
 *    A component with rho[a] = 0 takes eps_j = xi_j with no arithmetic: today's
 *    bytes.  The candidate is formed as before with eps for z: clamp(mean + std ·
 *    eps_j, lo, hi), the mean copied where the spread is 0, candidate 0 the mean
 *    itself.  eps has unit variance at every step and corr(eps_j, eps_k) =
 *    rho^|j - k|.  Where some rho[a], a < A, is not 0 the sample launch is another
 *    kernel over the same workgroups in x and no y: one thread per (c, e, d) walks
 *    the steps with eps in registers, one Philox call per step.  The launch count
 *    of a tick does not change; the prior's inject launch follows it unchanged.
 *    Per-drone planners take the env-level planner's noise byte for byte, as before.
 *  - Particle tick.  qs_smc_sample(p, s) runs the recurrence over the steps of
 *    segment s only: eps = xi at a segment's first step.  Resampling reassigns
 *    the particles between segments and no noise state follows them through
 *    parents, so segment = 1 makes rho a no-op.
 *  - Elite memory (keep > 0, CEM only).  The planner owns kept [n][keep][E][D][A]
 *    (float32) and kept_n, one int32 device word, both zeroed when the spec is
 *    attached; qs_cem_reset zeroes kept_n again (stream-ordered).
 *    qs_cem_refit(p, i) also writes kept[j][r][e][d][a] =
 *    candidates[j][elites[r][e]][e][d][a] for r < keep (per-drone mode:
 *    elites[r][e][d], so a kept row is the composite of every drone's own r-th
 *    elite slice) and *kept_n = keep, in the refit launch itself, which reads
 *    those values anyway.  qs_cem_sample(p, i) makes candidates 1 .. *kept_n bit
 *    copies of kept rows 0 .. *kept_n - 1 in the place of drawing them, not
 *    clipped again, in the sample launch itself (the count is read on the device,
 *    so the first iteration after create or reset injects nothing, iteration 0 of
 *    a later tick sees the previous tick's elites, and a captured plan replays
 *    correctly; the other candidates are the bytes they would be without keep).
 *    qs_cem_finish shifts kept as it shifts mean: kept[j] = kept[j + 1], the last
 *    step holds, by more workgroups of the finish launch.  A tick of I iterations
 *    is begin, I × (sample, score, select, refit), finish as before: keep adds no
 *    launch.  Slot 0 is the mean, slots 1 .. keep the elite memory, the last `count` slots a policy prior's; they never overlap
 *    (refusals).  The value tail is independent of all this.  The score launch is
 *    deterministic and a candidate's outputs do not depend on its slot, so a kept
 *    elite scores the same bits again: without a value tail iter_best[i + 1][e] >=
 *    iter_best[i][e] within a tick, for every env.
 *  - qs_sampling_*_set copy the spec (NULL detaches) and, with keep > 0, allocate
 *    kept and kept_n; qs_sampling_cem_buffers returns the two pointers, NULL
 *    without a spec or with keep = 0.  They are host calls that may synchronise
 *    the device, not stream-ordered: do not capture them.
 *
 * Refusals (QS_E_INVALID with a message that names the entry point and the field;
 * the planner, and a spec attached earlier, are as they were): a null planner;
 * rho[a] outside [0, 1) or not finite for some a < A; reserved != 0; keep < 0;
 * keep != 0 on an MPPI or particle planner; keep > elites; 1 + keep + the prior's
 * count > candidates (also refused by qs_prior_cem_set where the sampling spec is
 * attached first); a step of kept (keep · E · D · A · 4 bytes) past the 32-bit
 * offsets.                                                                       */
typedef struct qs_sampling_spec {
  float rho[4];              /* per action component (first A used): AR(1)
                                coefficient in [0, 1)                               */
  int32_t keep;              /* CEM only: elites carried over, 0 .. min(elites,
                                candidates - 1 - prior count); 0 for MPPI / SMC     */
  int32_t reserved;          /* must be 0                                           */
} qs_sampling_spec;

int qs_sampling_mppi_set(qs_mppi* p, const qs_sampling_spec* spec);
int qs_sampling_cem_set(qs_cem* p, const qs_sampling_spec* spec);
int qs_sampling_cem_buffers(const qs_cem* p, float** kept, int32_t** kept_n);

/* Tracking cost: a quadratic cost against a caller-supplied reference, summed inside
 * the score launch next to ret_agent, and the MPPI / CEM ticks that plan on it.  (New
 * entry points of ABI 4, like qs_step_seq; every name starts with qs_track_.)
 *
 * The cost.  For candidate c, env e, drone d, over steps j = 0 .. jd (jd as in
 * qs_score_out.ret: the env's first done step in that candidate, or n - 1):
 *   x[0:12]  the drone's pos, rpy, vel, angular velocity after step j and before any
 *            auto-reset, each cast to float: the values the step writes to
 *            obs[..., 0:12] (terminal_obs[..., 0:12] on a done step), on fp64 handles too
 *   row      clamp(base[e] + j, 0, L - 1); base == NULL means 0
 *   u        the float32 action the step consumed (actions_out)
 *   s = 0;  for k in 0..11: dd = (double)x[k] - (double)ref[row][e][d][k];
 *                           s = s + (double)q[k] * (dd * dd)
 *   if j == n - 1: s = (double)terminal * s
 *   for a in 0..A-1: s = s + (double)r[a] * ((double)u[a] * (double)u[a])
 *   cost_agent[c][e][d] += s
 * in double, k and a ascending, every product and sum rounded on its own (no fused
 * multiply-add): a plain float64 loop over the launch's outputs gives the same bytes.
 *
 *  - ref and base are the caller's device memory, read at every launch and never
 *    copied: update them in place (base += 1 to step along the reference, base[done]
 *    = 0 to restart an env's phase) and the next launch, or the next replay of a
 *    captured one, sees it.  E is the handle's local env count.
 *  - qs_track_score is qs_score_agents plus cost_agent ([C][E][D] double): every
 *    other output is, byte for byte, what qs_score_agents writes; depth, refusals,
 *    no mutation and capture as there.  cost_agent counts as an output in the overlap
 *    check.  It refuses a NULL spec or cost_agent.
 *  - qs_track_fold forms the objective in place on caller-owned buffers, in float64,
 *    every operation rounded on its own, d ascending, one thread per (c, e):
 *      ret[c][e]          = scale * ret[c][e] - (sum_d cost_agent[c][e][d]) / D
 *      ret_agent[c][e][d] = scale * ret_agent[c][e][d] - cost_agent[c][e][d]
 *    each where the pointer is not NULL (ret first: it reads cost_agent only).
 *  - qs_track_mppi_set / qs_track_cem_set copy the spec's numbers and pointers (NULL
 *    detaches) and allocate cost_agent, and ret_agent on an env-level planner.  The
 *    score stage of plan() is then qs_track_score and the fold with the spec's
 *    reward_scale, so ret (per-drone mode: ret_agent) holds the objective; update,
 *    select and refit consume it unchanged, done_penalty still applies through
 *    first_done.  *_score is that stage on its own; *_buffers returns cost_agent and
 *    the ret_agent in use (NULL without a spec).  The set calls are host calls that
 *    may synchronise the device: do not capture them.  A planner without a spec
 *    launches and writes exactly what it did before.
 *  - Tracking and the value tail do not compose (a discounted tail, an undiscounted
 *    cost): the second to be attached is refused.  Branch sets and the particle tick
 *    have no tracking.
 *
 * Refusals (QS_E_INVALID with a message that names the entry point; nothing is
 * written): a null argument; q[k], r[a] (a < A) or terminal negative or not finite;
 * reward_scale not finite; L < 1; ref NULL or not 16-byte aligned; L * E * D * 48
 * bytes at or past 2^31.                                                         */
typedef struct qs_track_spec {
  const float* ref;      /* device [L][E][D][12] float32, the caller's; read at every launch, never copied; 16-byte aligned */
  const int32_t* base;   /* device [E] int32 or NULL: row of step 0 for each env; the caller's, read at every launch */
  int32_t L;             /* >= 1; L * E * D * 48 must stay below 2^31 (32-bit offsets), refused otherwise */
  float q[12];           /* finite, >= 0 */
  float r[4];            /* finite, >= 0 (first A used) */
  float terminal;        /* finite, >= 0: multiplies the state part of the launch's last step */
  float reward_scale;    /* finite: the task reward's weight in the folded objective (planners, qs_track_fold) */
} qs_track_spec;

int qs_track_score(qs_handle* h, int n, int C, const float* const* actions,
                   const qs_step_out* outs, const qs_score_out* score, double* ret_agent,
                   const qs_track_spec* spec, double* cost_agent, void* stream);
int qs_track_fold(int C, int E, int D, double reward_scale, double* ret, double* ret_agent,
                  const double* cost_agent, void* stream);
int qs_track_mppi_set(qs_mppi* p, const qs_track_spec* spec);
int qs_track_mppi_buffers(const qs_mppi* p, double** cost_agent, double** ret_agent);
int qs_track_mppi_score(qs_mppi* p, void* stream);
int qs_track_cem_set(qs_cem* p, const qs_track_spec* spec);
int qs_track_cem_buffers(const qs_cem* p, double** cost_agent, double** ret_agent);
int qs_track_cem_score(qs_cem* p, void* stream);

/* Separation and obstacle terms: two more parts of the cost that qs_track_score sums,
 * for collision-free formation changes and obstacle avoidance.  (New entry points of
 * ABI 4; every name starts with qs_avoid_.  The qs_track_ names and records stand.)
 *
 * The terms.  For candidate c, env e, drone d, at every step j = 0 .. jd (jd as for
 * ret_agent), with p_i the three floats the obs row of drone i of the same virtual
 * env starts with after step j and before any auto-reset (obs[..., 0:3], or
 * terminal_obs[..., 0:3] on a done step; on fp64 handles too), all in double, every
 * subtraction, product and sum rounded on its own (no fused multiply-add):
 *   separation (skipped where sep_weight == 0, sep_radius == 0 or D == 1):
 *     r2 = sep_radius * sep_radius;  s_sep = 0
 *     for i in 0..D-1, i != d:
 *       dx = p_d[0] - p_i[0];  dy = p_d[1] - p_i[1];  dz = (p_d[2] - p_i[2]) * sep_z_scale
 *       d2 = (dx * dx + dy * dy) + dz * dz;  g = r2 - d2
 *       if g > 0: s_sep = s_sep + g * g          (a NaN compares false: no term)
 *   obstacles (skipped where M == 0); row m of the table is c[3], a[3], radius, weight:
 *     s_obs = 0
 *     for m in 0..M-1:
 *       d2 = 0;  for k in 0..2: dd = p_d[k] - c[k];  d2 = d2 + a[k] * (dd * dd)
 *       g = radius * radius - d2
 *       if g > 0: s_obs = s_obs + weight * (g * g)
 *   the step's cost: s as in qs_track_score (terminal and the action terms included;
 *   +0.0 without a tracking spec), then s = s + sep_weight * s_sep, then s = s + s_obs;
 *   cost_agent[c][e][d] += s.
 * The avoidance terms are not scaled by `terminal`.  An axis weight of 0 drops an axis:
 * a = (1, 1, 1) is a sphere, (1, 1, 0) a vertical cylinder, (0, 0, 1) a slab such as a
 * floor or a ceiling.  A pair contributes to both of its drones, so the fold's mean over
 * D counts a pair twice over D.
 *
 *  - obstacles is the caller's device memory, shared by all envs and candidates, read at
 *    every launch and never copied: an update in place is seen by the next launch, or the
 *    next replay of a captured one.  Its contents are not validated.
 *  - qs_avoid_score is qs_track_score with the two terms; track may be NULL (no tracking
 *    part: nothing of a reference is read).  With every switch off and a tracking spec,
 *    cost_agent is qs_track_score's, byte for byte; every other output is what
 *    qs_track_score (track == NULL: qs_score_agents) writes.
 *  - qs_avoid_mppi_set / qs_avoid_cem_set copy the spec (NULL detaches), independently of
 *    a tracking spec.  The score stage of plan() is then qs_avoid_score with the planner's
 *    tracking spec or NULL, and qs_track_fold with that spec's reward_scale, or 1.
 *    *_score is that stage on its own; *_buffers returns cost_agent and the ret_agent in
 *    use (NULL with neither spec).  The set calls are host calls that may synchronise.
 *    Avoidance and the value tail do not compose: the second to be attached is refused.
 *    Branch sets and the particle tick have none of this.
 *
 * Refusals (QS_E_INVALID, the entry point's name first; nothing is written): a null
 * handle, avoid or cost_agent; M outside 0 .. 16; obstacles NULL or not 16-byte aligned
 * where M > 0; sep_radius, sep_weight or sep_z_scale negative or not finite; whatever
 * qs_track_score refuses, where track is given; cost_agent overlapping an output or an
 * action buffer.                                                                   */
typedef struct qs_avoid_spec {
  const float* obstacles;   /* device [M][8] float32: c[3], a[3], radius, weight; the caller's, read at every launch; 16-byte aligned */
  int32_t M;                /* 0 .. 16 rows */
  float sep_radius;         /* finite, >= 0; 0 switches the separation term off */
  float sep_weight;         /* finite, >= 0; 0 switches the separation term off */
  float sep_z_scale;        /* finite, >= 0: the factor on the height difference of a pair */
} qs_avoid_spec;

int qs_avoid_score(qs_handle* h, int n, int C, const float* const* actions,
                   const qs_step_out* outs, const qs_score_out* score, double* ret_agent,
                   const qs_track_spec* track /* may be NULL */, const qs_avoid_spec* avoid,
                   double* cost_agent, void* stream);
int qs_avoid_mppi_set(qs_mppi* p, const qs_avoid_spec* spec);
int qs_avoid_mppi_buffers(const qs_mppi* p, double** cost_agent, double** ret_agent);
int qs_avoid_mppi_score(qs_mppi* p, void* stream);
int qs_avoid_cem_set(qs_cem* p, const qs_avoid_spec* spec);
int qs_avoid_cem_buffers(const qs_cem* p, double** cost_agent, double** ret_agent);
int qs_avoid_cem_score(qs_cem* p, void* stream);

/* Particle (sequential Monte Carlo) planner tick on top of a branch set: fork C
 * particles from the handle's current state, run the horizon in S = ceil(n / L)
 * segments of at most L steps, each "sample actions, advance the particles, weigh
 * them and systematically resample per env", trace every surviving particle's
 * action sequence back through the resampling steps and fold the sequences into
 * the nominal by their weights, as MPPI does, all on the device.  The horizon is
 * not held to qs_score_depth: only a segment is.  With ess_frac = 0 nothing is
 * ever resampled and the tick is an MPPI tick of any length.  (New entry points of
 * ABI 4, like qs_branch_*.)
 *
 * A planner is bound to one handle, which must outlive it, and owns its device
 * buffers (qs_smc_buffers; stable until qs_smc_destroy) and one branch set of C
 * candidates (qs_branch_create), which qs_smc_branch hands out for reading only
 * (qs_branch_buffers, qs_branch_state, qs_branch_steps): the caller neither
 * destroys nor forks it.  ret, first_done and ret_agent are that set's.  Every call
 * but create / destroy / buffers / branch is stream-ordered and asynchronous,
 * reads nothing back to the host and may be captured into a graph; the tick
 * counter lives on the device, so a replayed graph draws new noise each time.  No
 * float atomics and every sum in a fixed order: the same inputs give the same
 * bytes.  Like a handle, a planner is used from one host thread at a time.  Every
 * env plans independently of the others.
 *
 * Segment s holds the steps s · L .. min(n, (s + 1) · L) - 1 of the tick.
 *
 *  - qs_smc_begin.  qs_branch_fork of the set; base = 0; parents[s][c][e] = c for
 *    every s; resampled, offset and ess = 0.  QS_E_STATE before qs_reset, with
 *    nothing launched.
 *  - qs_smc_sample(p, s).  qs_mppi_sample's kernel over the steps of segment s: one
 *    Philox4x32-10 call per (step j, particle c, env e, drone d): key = seed,
 *    counter = (low word of *tick, env_offset + e, c · 32 + (j - s · L),
 *    (5 << 24) | (s << 8) | d), the normals formed as in qs_mppi_sample.
 *    candidates[j][0][e][d][a] = nominal[j][e][d][a] as it is (particle 0 draws no
 *    noise); for c > 0, clamp(nominal + sigma[a] · z_a, lo, hi), the sum left out
 *    where sigma[a] = 0.  The counter holds the global env id, so the noise does
 *    not depend on how envs are sharded; segments, ticks, envs, particles, steps
 *    and drones never share a counter.
 *  - qs_smc_advance(p, s).  qs_branch_advance of the segment's steps from
 *    candidates, with outs = NULL.  QS_E_STATE before the first begin.
 *  - qs_smc_resample(p, s), 0 <= s < S - 1.  Per env e, in double, with t =
 *    (s + 1) · L the steps since the fork: score_c = ret[c][e] - (first_done[c][e]
 *    < t ? done_penalty : 0); logw_c = (score_c - base[c][e]) / lambda; x_c =
 *    exp(logw_c - max logw) and weights[c][e] = x_c / sum over c.  A NaN logw
 *    gives weight 0 (and is passed over by the max); where no logw is a number
 *    the weights are uniform and the env does not resample.  ess[s][e] = 1 / sum
 *    over c of weights^2.  The env resamples iff ess < ess_frac · C, which
 *    resampled[s][e] records.  If it does: one Philox call per env, key = seed,
 *    counter = (low word of *tick, env_offset + e, s, 6 << 24), u = (x0 >> 8) ·
 *    2^-24 in [0, 1) into offset[s][e]; with pos_i = (i + u) / C,
 *    parents[s][i][e] = the lowest c whose inclusive cumulative weight (in index
 *    order) exceeds pos_i, C - 1 if none does; base[i][e] = score of that
 *    parent, so every new particle starts the next segment at log weight 0.  If
 *    it does not: parents[s][.][e] is the identity, base is untouched and
 *    offset[s][e] = 0.  Then qs_branch_select(set, parents[s]).  The cumulative
 *    sum's rounding is the variant's own: one thread per env adds the weights up
 *    in index order; the workgroup per env (C >= 64 and few envs, the criterion
 *    of the MPPI update's variants) scans them in blocks and takes the running
 *    maximum of the scan, so that it never falls; either is within C · 2^-53 of
 *    the exact sum.  It reads ret and first_done as they are: a caller may
 *    overwrite them through the set's pointers first.  With ess_frac = 0, and for
 *    s = S - 1 (finish weighs the last segment), nothing is launched and the call
 *    returns QS_OK.  QS_E_STATE before the first begin.
 *  - qs_smc_finish.  weights from the final logw as above, with t = n, and
 *    ess[S - 1][e] from them; best[e] = the lowest c with the largest weight;
 *    ancestors[S - 1][c][e] = c and ancestors[s][c][e] = parents[s][ancestors[s +
 *    1][c][e]][e] for s = S - 2 .. 0; new[j] = (float) sum over c of
 *    weights[c][e] · candidates[j][ancestors[s(j)][c][e]][e], s(j) = j / L, summed
 *    in double; action = new[0]; nominal[j] = new[j + 1] for j < n - 1 and
 *    nominal[n - 1] = new[n - 1] (hold); *tick += 1.  Three launches.
 *  - qs_smc_plan = begin, then for s = 0 .. S - 1: sample(s), advance(s),
 *    resample(s), then finish.  QS_E_STATE before qs_reset, with nothing launched.
 *  - qs_smc_reset copies `nominal` (device, [n][E][D][A]; NULL: zeros) into the
 *    planner and sets *tick = 0.  A new planner is in that state with zeros.
 *  - Per-drone mode: none.  A branch's state is shared by the env's drones, so the
 *    drones of an env cannot be resampled apart.
 *  - qs_smc_create refusals (QS_E_INVALID with a message, nothing launched, *out
 *    untouched): horizon < 1 or more than 256 segments, segment outside 1 ..
 *    qs_score_depth(h), particles < 2 or > 4096 (the workgroup variant keeps one
 *    env's cumulative weights in LDS, four particles to each of its 1024
 *    threads), lo >= hi or non-finite, a negative or non-finite sigma or
 *    done_penalty, lambda <= 0 or non-finite, ess_frac outside [0, 1], whatever
 *    qs_branch_create refuses (a handle with qs_score_depth(h) = 0 among it), and
 *    sizes beyond the 32-bit offsets of a branch advance or S · C · E >= 2^31.
 *    qs_smc_sample / advance / resample with s outside 0 .. S - 1: QS_E_INVALID,
 *    nothing launched.
 *  - No policy prior (qs_prior_*): the particles are resampled mid-horizon, which
 *    a closed-loop trajectory fixed before the tick cannot follow.              */
typedef struct qs_smc_spec {
  int32_t horizon;      /* n >= 1 steps per tick; S = ceil(n / segment) <= 256     */
  int32_t segment;      /* L: 1 .. qs_score_depth(h) steps per advance; the last
                           segment may be shorter                                 */
  int32_t particles;    /* C: 2 .. 4096; particle 0 draws no noise (it follows the
                           nominal's actions)                                     */
  float sigma[4];       /* noise std per action component (first A used), >= 0    */
  float lo, hi;         /* candidates are clipped to [lo, hi]; lo < hi            */
  double lambda;        /* temperature, > 0 and finite                            */
  double done_penalty;  /* >= 0; subtracted from a particle's score once its env
                           has ended an episode                                   */
  double ess_frac;      /* 0 .. 1; after a segment but the last, env e resamples
                           iff ESS_e < ess_frac * C.  0 = never: no resample or
                           select launch is issued at all                         */
  uint64_t seed;
} qs_smc_spec;

typedef struct qs_smc_bufs {  /* device pointers owned by the planner             */
  float* nominal;       /* [n][E][D][A]                                          */
  float* candidates;    /* [n][C][E][D][A]  (what the advances read)             */
  double* base;         /* [C][E]  the score a particle had when last resampled  */
  double* weights;      /* [C][E]  normalised, of the last resample or finish    */
  int32_t* parents;     /* [S][C][E] who particle c of env e was copied from
                           after segment s (identity where nothing resampled)    */
  int32_t* ancestors;   /* [S][C][E] whose actions the final particle c ran in
                           segment s                                             */
  double* ess;          /* [S][E]  effective sample size after segment s         */
  double* offset;       /* [S][E]  the resampling offset u, 0 where not drawn    */
  int32_t* resampled;   /* [S][E]  1 where env e resampled after segment s       */
  int32_t* best;        /* [E]     the lowest c with the largest final weight    */
  float* action;        /* [E][D][A] the first step of the updated nominal       */
  uint64_t* tick;       /* [1]     device counter, +1 per finish                 */
} qs_smc_bufs;

typedef struct qs_smc qs_smc;

int qs_smc_create(qs_handle* h, const qs_smc_spec* spec, qs_smc** out);
int qs_smc_destroy(qs_smc* p);
int qs_smc_buffers(const qs_smc* p, qs_smc_bufs* out);
int qs_smc_branch(const qs_smc* p, qs_branch** out);
int qs_smc_reset(qs_smc* p, const float* nominal, void* stream);
int qs_smc_begin(qs_smc* p, void* stream);
int qs_smc_sample(qs_smc* p, int segment, void* stream);
int qs_smc_advance(qs_smc* p, int segment, void* stream);
int qs_smc_resample(qs_smc* p, int segment, void* stream);
int qs_smc_finish(qs_smc* p, void* stream);
int qs_smc_plan(qs_smc* p, void* stream);
int qs_sampling_smc_set(qs_smc* p, const qs_sampling_spec* spec);   /* the sampling spec above, on a particle planner */

/* Multi-step launches this handle has made so far (host, no device work):
 * out[0] on the general multi-step kernel instances, out[1] on the
 * shape-specialised one.  The specialised instance serves synthetic-policy
 * launches of two or more steps of MultiHover, ONE_D_PID at 30 / 240 Hz with no
 * extra forces and CF2X, 8 drones, a multiple of 8 envs, a reject-free layout,
 * auto-reset on, and at every step of the launch 16-byte aligned obs, reward,
 * terminated, truncated and actions_out and neither terminal_obs nor reasons;
 * every other launch, and every launch of a process with QS_HOT_SHAPE=0 in its
 * environment at qs_create, runs the general instances.  Results do not
 * depend on which one runs.  The kernel node that qs_step calls build on a
 * capturing stream counts once, under the instance it names when the capture
 * ends.  (A new entry point of ABI 4, like qs_step_seq.) */
int qs_launch_counts(const qs_handle* h, int64_t out[2]);

/* Ring launches this handle has made so far (host, no device work).  A launch
 * of the shape-specialised instance goes on past its distinct output sets, up
 * to QS_MAX_FUSED_STEPS of them, while the further steps write exactly those
 * sets again in the same order (a rollout into a ring of buffers): step k of
 * the launch writes set k mod P, and every set ends up holding what the last
 * step that wrote it produced, as after single steps.  *launches: such
 * launches (they also count under qs_launch_counts' out[1]); *steps: the
 * control steps they held.  At most 1024 steps to a launch (QS_RING_MAX_STEPS
 * at qs_create lowers it); QS_RING_LAUNCH=0 at qs_create cuts every launch at
 * the first repeated set, as all other shapes are cut.  A capture's kernel node
 * counts once, with the steps it holds when the capture ends.  (An additive
 * entry point of ABI 4.) */
int qs_ring_counts(const qs_handle* h, int64_t* launches, int64_t* steps);

/* Copy a state block between the handle and `buf` (device pointer).
 * dir = 0: handle → buf (get), dir = 1: buf → handle (set). */
int qs_state_io(qs_handle* h, int block, void* buf, int dir, void* stream);

/* Completed-episode log: a ring per env (max(8, 65536 / num_envs) slots,
 * appended in-kernel on done, no atomics).  Each record: {double return;
 * int32 length; int32 env; int64 seq}: seq = the step index at which it
 * completed.  qs_episode_log merges the rings in (seq, env) order — the
 * order the reference's env loop logs them — copies up to `cap` most-recent
 * records to `dst` (device) and writes the total number of episodes ever
 * logged to *total and the number of records written to dst to *written
 * (host, synchronous; written may be NULL): fewer than min(total, cap) when
 * rings dropped episodes.  The selection runs on the device
 * (a seq-distance histogram, then a compaction): O(cap) records cross to the
 * host, and cap = 0 reads back the total alone.  An env that completes more episodes
 * than its ring holds between two reads keeps only its latest ones. */
typedef struct qs_episode_rec {
  double ret;
  int32_t len;
  int32_t env;
  int64_t seq;
} qs_episode_rec;
int qs_episode_log(qs_handle* h, qs_episode_rec* dst, int64_t cap,
                   int64_t* total, int64_t* written, void* stream);

/* 1 if an in-kernel reset rejection search hit its try cap (2^24) since the
 * last qs_reset (synchronous). */
int qs_reset_error(qs_handle* h, int* out);

/* Diagnostics: a dword-per-lane copy with the same access pattern as the
 * step kernel's SoA loads/stores; used to calibrate rocprofv3 FETCH_SIZE /
 * WRITE_SIZE on gfx950 (MI355X_MICROARCH.md §HBM). */
int qs_calib_copy(float* dst, const float* src, int64_t n, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* QUADSWARM_H */
