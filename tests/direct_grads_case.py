"""The shared cases of tests/test_direct_grads_cases.py (CPU) and
tests/test_gpu_direct_grads.py: MAPPOAgent._iteration_direct — the 256-wide
split-K update every minibatch above _SMALL_MAX_ROWS actor rows takes, and what
every rank of a multi-GPU run executes — on the data construction and the
float64 restatement of tests/small_grads_case.py (30-50 % of the rows outside
the clip bounds, none within 5e-3 of one).

A case is a shape and a seed; its tables are drawn once per process (`base`),
with an agent that is never stepped: the float64 reference and torch's float32
autograd are formed from that agent's weights.  Every test steps agents of its
own (`fresh`): the same seed gives the same weights, and a MAPPOBuffer of
T = 2, E = mb holds the case's tables in the same row order.

The seeds follow small_grads_case's rule: the first from 11 upwards whose draw,
judged on the references alone, keeps float32 autograd within 1.5e-6 on both
idx draws and meets the data and detection conditions of
tests/test_direct_grads_cases.py (the latter decided one seed: at 3 000
env-timesteps and hidden width 128, seed 13's draw moves a tensor by only
1.4e-4 when one env-timestep is dropped; 14 and 15 fail the float32 condition).
"""
import types

import torch

import small_grads_case as sg
from small_grads_case import (CLIP, ENT_COEF, NAMES, actor_rows, fp32_autograd_errors, losses, param_tensors,  # noqa: F401
                              reference, rel_err, row_groups)

GRAD_BOUND = 2e-5   # tests/test_gpu_small_grads.py's: 16 x float32 autograd under the same metric

# keyword arguments of the agent per variant (fold_w1: _F16Work.fold_w1 = True
# on the class while the agent's workspace is built, see `folded`)
VARIANTS = {
    "fused": {},                                   # _F16Work: qs_mlp3f_actor_w1 + split-K GEMMs | _M3Work + qs_value_head
    "fused_vh": dict(fused_value_head=True),       # ... | qs_mlp3_fwd_rows_value
    "fused_tiles": dict(critic_tiles=True),        # ... | _CriticTiles: qs_ppo_critic_tiles + qs_wgrad_t
    "two_kernel": dict(fused_actor=False),         # qs_mlp3_fwd_group_rows + qs_ppo_heads + qs_mlp3_bwd | _M3Work
    "fold_w1": {},                                 # dW1 folded into the fused launch | _M3Work
}

# id, mb, D, O, A, action_scale, seed, then what the host code does with the
# shape (tests/test_direct_grads_cases.py proves each from the workspace
# objects): the chunk counts (S1, S2) of dW1 / dW2 for the fused actor, the
# two-kernel actor and the _M3Work critic (1 = one GEMM straight into .grad, a
# `whole` task); the partial rows of qs_mlp3f_actor, of the two-kernel actor's
# qs_mlp3_bwd and of the critic's.
_C = lambda id, mb, D, O, A, scale, seed, f16, m3, cr, Gf, Ga, Gc: dict(
    id=id, mb=mb, D=D, O=O, A=A, scale=scale, seed=seed, f16_chunks=f16, m3_chunks=m3, critic_chunks=cr,
    f16_tiles=Gf, m3_tiles=Ga, critic_tiles=Gc)
CASES = [
    # 1 024 actor rows: every weight gradient is one GEMM straight into .grad
    _C("c3_slice", 128, 8, 27, 1, 1.0, 12, (1, 1), (1, 1), (1, 1), 8, 32, 4),
    # 185 rows: a partial 16-row tile and a partial 128-row workgroup; 37 critic rows of 360 inputs
    _C("ragged_185", 37, 5, 72, 2, 0.7, 11, (1, 1), (1, 1), (1, 1), 2, 6, 2),
    # 3 actor rows, 1 critic row (seed 11 leaves no zero-gradient clipped row, 12 fails the float32 condition)
    _C("three_rows", 1, 3, 27, 1, 1.0, 13, (1, 1), (1, 1), (1, 1), 1, 1, 1),
    _C("A3_critic_432", 96, 16, 27, 3, 0.7, 12, (1, 1), (1, 1), (1, 1), 12, 48, 3),
    # input widths 119 and 595; the fused actor's dW1 in 2 chunks beside a one-GEMM dW2
    _C("spiral_A4", 512, 5, 119, 4, 0.4, 12, (2, 1), (2, 2), (1, 1), 20, 80, 16),
    # the fused actor's dW1 in 4 chunks, dW2 in 2
    _C("rows_4096", 512, 8, 27, 1, 1.0, 11, (4, 2), (4, 4), (1, 1), 32, 128, 16),
    # D = 1: 3 000 rows in 2 chunks of 1 500; actor and critic both 27 wide
    _C("one_agent_3000", 3000, 1, 27, 1, 1.0, 12, (2, 1), (2, 2), (2, 2), 24, 94, 94),
    # qs_mlp3_bwd's 128-row blocks (K >= 16 384, I <= 64); the critic's gradients in chunks
    _C("rows_16384", 2048, 8, 27, 1, 1.0, 13, (16, 8), (16, 16), (2, 2), 128, 128, 64),
    # 32-row blocks at 16 384 rows: 512 partial rows, the sum launch's tall-task instance
    _C("rows_16384_in72", 2048, 8, 72, 2, 0.7, 11, (16, 8), (16, 16), (2, 2), 128, 512, 64),
]
CASE_IDS = [c["id"] for c in CASES]

# every case runs fused and two_kernel; the opt-in variants where they differ most
RUNS = [(c["id"], v) for c in CASES for v in ("fused", "two_kernel")] + \
       [(cid, "fused_vh") for cid in ("c3_slice", "ragged_185", "rows_16384")] + \
       [(cid, "fused_tiles") for cid in ("c3_slice", "one_agent_3000", "rows_4096")] + \
       [(cid, "fold_w1") for cid in ("ragged_185", "spiral_A4")]
RUN_IDS = [f"{cid}-{v}" for cid, v in RUNS]

# the autograd-driven fused iteration (_iteration_fused: qs_ppo_heads around
# the MLPs under autograd, then qs_adam_multi) at hidden widths 64 and 128:
# (case, width) -> seed, by the same rule for those nets.  MLP.forward takes
# _TanhMLP3 (qs_mlp_bias_tanh / qs_mlp_tanh_bwd) from 2 048 rows: the first two
# cases' nets run as plain torch layers around the HIP loss heads; both nets of
# one_agent_3000 (3 000 rows each: 47 blocks, the last one partial) and the
# four-output actor of spiral_A4 (2 560 rows) run on the kernels.
HIDDEN_SEEDS = {("ragged_185", 64): 11, ("ragged_185", 128): 16, ("A3_critic_432", 64): 13, ("A3_critic_432", 128): 12,
                ("one_agent_3000", 64): 11, ("one_agent_3000", 128): 16, ("spiral_A4", 128): 11}
HIDDEN_RUNS = list(HIDDEN_SEEDS)


def case_of(cid):
    return CASES[CASE_IDS.index(cid)]


def build(c, device, seed=None, hidden_dim=256):
    """The case's agent (never stepped: small=False, the default variant) and
    tables, as small_grads_case.draw lays them out."""
    seed = c["seed"] if seed is None else seed
    agent = sg.make_agent(c["D"], c["O"], c["A"], c["scale"], seed, device, hidden_dim=hidden_dim, small=False)
    return sg.draw(agent, c["mb"], c["D"], c["O"], c["A"], c["scale"], seed, 2 * c["mb"], device)


_built = {}


def base(cid, device, hidden_dim=256):
    """The case `cid` on `device`, built once per process; its float64
    references are cached on it (no test changes it).  hidden_dim: the nets'
    hidden width (HIDDEN_RUNS; the old log-probabilities follow that actor)."""
    key = (cid, str(device), hidden_dim)
    if key not in _built:
        seed = case_of(cid)["seed"] if hidden_dim == 256 else HIDDEN_SEEDS[(cid, hidden_dim)]
        _built[key] = build(case_of(cid), device, seed=seed, hidden_dim=hidden_dim)
    return _built[key]


class folded:
    """_F16Work.fold_w1 = True while an agent's workspace is built (the flag is
    read in _F16Work.__init__ only); restored on exit."""

    def __init__(self, on=True):
        self.on = on

    def __enter__(self):
        from gym_pybullet_drones_amd.mappo.agent import _F16Work
        self.cls, self.prev = _F16Work, _F16Work.fold_w1
        if self.on:
            _F16Work.fold_w1 = True

    def __exit__(self, *exc):
        self.cls.fold_w1 = self.prev
        return False


def fill_buffer(b, agent, logp_shift=0.0):
    """A MAPPOBuffer of T = 2, E = mb with the case's tables (obs, act, logp,
    adv_env, ret_env): env-timestep t·mb + e is table row t·mb + e."""
    from gym_pybullet_drones_amd.mappo.buffer import MAPPOBuffer
    buf = MAPPOBuffer(agent.obs_space, agent.act_space, 2, b.mb, include_global_state=True, device=b.device)
    buf.obs.copy_(b.obs.reshape(2, b.mb, b.D, b.O))
    buf.act.copy_(b.act.reshape(2, b.mb, b.D, b.A))
    buf.logp.copy_((b.logp_old + logp_shift).reshape(2, b.mb, b.D, 1))
    buf.adv_env.copy_(b.adv_env.reshape(2, b.mb))
    buf.ret_env.copy_(b.ret_env.reshape(2, b.mb))
    buf.t, buf.full = 0, True
    return buf


def fresh(cid, device, variant="fused", hidden_dim=256, logp_shift=0.0, setup=True, **agent_kw):
    """A freshly built agent of `variant` with the case's weights, a buffer with
    its tables, and (setup, hidden 256) the direct iteration's workspace, built
    the way the first minibatch would."""
    c, b = case_of(cid), base(cid, device, hidden_dim)
    kw = dict(VARIANTS[variant], small=False)
    kw.update(agent_kw)
    agent = sg.make_agent(c["D"], c["O"], c["A"], c["scale"], b.seed, device, hidden_dim=hidden_dim, **kw)
    run = types.SimpleNamespace(cid=cid, variant=variant, base=b, agent=agent, mb=b.mb, D=b.D, O=b.O, A=b.A)
    run.buf = fill_buffer(b, agent, logp_shift)
    if setup and hidden_dim == 256:
        with folded(variant == "fold_w1"):
            agent._direct_setup(b.mb, b.D, b.O, b.A)
    return run


def run_params(run):
    """The 13 parameters of the run's own agent by name."""
    return param_tensors(types.SimpleNamespace(agent=run.agent))


def flat_view(fb, p, buf):
    """The slice of FlatBuffers fb's flat buffer `buf` (exp_avg, ...) that belongs to its parameter p."""
    off, cnt = fb.offsets[[id(q) for q in fb.params].index(id(p))]
    return buf[off:off + cnt].view_as(p)
