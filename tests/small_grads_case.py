"""The shared cases of tests/test_small_grads_cases.py (CPU) and
tests/test_gpu_small_grads.py: the tile learner's two 256-wide tanh MLPs with
every input of one qs_ppo_small_grads call, and a float64 autograd restatement
of the losses (compute_policy_loss / compute_value_loss, AG:602-683) through
the whole nets.  Plain torch with a `device` argument: the reference half runs
on the CPU, and the data (drawn from seeded CPU generators) is the same on
every device.  tests/direct_grads_case.py builds the direct iteration's cases
from the same pieces (make_agent, draw, losses, check_against_float64).

Old log-probabilities lie 0.25·noise from the current ones, so 30-50 % of the
rows are outside the clip bounds (both branches of the tile kernel's PPO head,
with and without gradient).  A row whose ratio sits on a bound takes different
branches in float32 and float64 — plain draws put one within 1.4e-5 of a bound
at 4 096 rows — so rows within GUARD of a bound are moved GUARD_SHIFT away
from it, on the side they were on, before logp_old is rounded to float32.

The seeds.  The tests' metric divides a tensor's largest error by its largest
float64 element.  For the few-element tensors that are sums over every row
(the actor's b3 and logstd: A elements) the rows' terms can cancel, and then
any float32 evaluation is far off in that metric: over seeds, torch's own
float32 autograd gave 1e-6 .. 3e-6 for most draws and up to 1e-4 (2e-3 once at
120 rows) where such a sum cancelled.  Each entry's seed is the first from 11
upwards whose draw — judged on the references alone, on the CPU — keeps
float32 autograd within 1.5e-6 on both idx draws and meets the data conditions
of tests/test_small_grads_cases.py."""
import math
import types

import numpy as np
import torch

CLIP, ENT_COEF = 0.2, 0.01
NOISE, GUARD, GUARD_SHIFT = 0.25, 0.01, 0.02

# mb, D, O, A, action_scale, then the layout the entry is meant to hit
# (tests/test_small_grads_cases.py proves it with qs_ppo_small_layout): the
# actor's / critic's 16-row blocks per tile, whether the actor's / critic's
# weight gradients are split in K-chunks (launch 3), whether the wide (> 256
# inputs) forward/backward instance runs; w1p False: no padded W1 copies
# (layer 1 by clamped scalar loads).
_C = lambda id, mb, D, O, A, scale, rb, rbc, sa, sc, wide, seed, w1p=True: dict(
    id=id, mb=mb, D=D, O=O, A=A, scale=scale, rb=rb, rbc=rbc, sa_chunks=sa, sc_chunks=sc, wide=wide, seed=seed, w1p=w1p)
CASES = [
    _C("ref_shape", 32, 8, 27, 1, 1.0, 1, 1, False, False, False, 12),            # the reference's learner shape
    _C("ragged_120_rows", 15, 8, 27, 1, 1.0, 1, 1, False, False, False, 12),      # a partial last tile in both nets
    _C("three_rows", 1, 3, 27, 1, 1.0, 1, 1, False, False, False, 26),            # 3 actor rows, 1 critic row
    _C("A3_critic_432", 9, 16, 27, 3, 0.7, 1, 1, False, False, True, 11),
    _C("A2_critic_576", 16, 8, 72, 2, 0.7, 1, 1, False, False, True, 11),
    _C("A4_in_119_critic_595", 8, 5, 119, 4, 0.4, 1, 1, False, False, True, 14),  # input width not a multiple of 4
    _C("rows_4096", 512, 8, 27, 1, 1.0, 2, 1, True, False, False, 11),            # actor gradients in K-chunks
    _C("rows_4096_critic_432", 256, 16, 27, 1, 1.0, 2, 1, True, False, True, 13),
    _C("rows_3072_one_agent", 3072, 1, 27, 1, 1.0, 2, 2, True, True, False, 11),
    _C("rows_8192", 1024, 8, 27, 1, 1.0, 3, 1, True, True, False, 22),
    _C("rows_8192_critic_432", 512, 16, 27, 1, 1.0, 3, 1, True, False, True, 11),
    _C("rows_16384", 2048, 8, 27, 1, 1.0, 3, 3, True, True, False, 13),
    _C("A4_rows_5120_critic_595", 1024, 5, 119, 4, 0.4, 2, 1, True, True, True, 12),   # the 32-row four-output instance
    _C("ref_shape_no_w1p", 32, 8, 27, 1, 1.0, 1, 1, False, False, False, 12, w1p=False),
    # beyond the instances above: two-block tiles without the padded copies, and beside a wide two-block critic
    _C("rows_4096_no_w1p", 512, 8, 27, 1, 1.0, 2, 1, True, False, False, 11, w1p=False),
    _C("rows_3072_one_agent_no_w1p", 3072, 1, 27, 1, 1.0, 2, 2, True, True, False, 11, w1p=False),
    _C("rows_7000_critic_270", 700, 10, 27, 1, 1.0, 2, 2, True, False, True, 14),
]
CASE_IDS = [c["id"] for c in CASES]

NAMES = ["actor.W1", "actor.b1", "actor.W2", "actor.b2", "actor.W3", "actor.b3", "actor.logstd",
         "critic.W1", "critic.b1", "critic.W2", "critic.b2", "critic.W3", "critic.b3"]


def param_tensors(case):
    """The 13 parameters of the case's nets by name (views into the FlatBuffers;
    each one's .grad is its view of the flat gradient buffer)."""
    pa, pc = case.agent.ac.actor.pi_net.fcs, case.agent.ac.critic.v_net.fcs
    t = [pa[0].weight, pa[0].bias, pa[1].weight, pa[1].bias, pa[2].weight, pa[2].bias, case.agent.ac.actor.logstd,
         pc[0].weight, pc[0].bias, pc[1].weight, pc[1].bias, pc[2].weight, pc[2].bias]
    return dict(zip(NAMES, t))


def _mlp(p, net, x):
    h1 = torch.tanh(x @ p[net + ".W1"].T + p[net + ".b1"])
    h2 = torch.tanh(h1 @ p[net + ".W2"].T + p[net + ".b2"])
    return h2 @ p[net + ".W3"].T + p[net + ".b3"]


def _logp(p, scale, obs_rows, act_rows):
    """Σ_a Normal(mean·scale, exp(logstd)).log_prob(act) per row (distributions.py:9-33)."""
    mean = _mlp(p, "actor", obs_rows) * scale
    logstd = p["actor.logstd"]
    lp = -((act_rows - mean) ** 2) / (2 * torch.exp(logstd) ** 2) - logstd - math.log(math.sqrt(2 * math.pi))
    return lp.sum(-1)


def actor_rows(case, idx):
    """The minibatch's actor rows of the [T_E·D] tables: row i·D + d = agent d of env-timestep idx[i]."""
    return (idx[:, None] * case.D + torch.arange(case.D, device=idx.device)[None, :]).reshape(-1)


def make_agent(D, O, A, action_scale, seed, device, hidden_dim=256, **agent_kw):
    """MAPPOAgent with the cases' loss settings, its weights drawn from `seed`
    (the same on every device and for every keyword) and logstd spread over
    -0.7 .. -0.3; the spaces it was built for as .obs_space / .act_space."""
    from gym_pybullet_drones_amd.mappo.agent import MAPPOAgent
    from gym_pybullet_drones_amd.utils.spaces import Box
    obs_space = Box(-np.inf * np.ones((D, O)), np.inf * np.ones((D, O)))
    act_space = Box(-np.ones((D, A)), np.ones((D, A)))
    agent_kw.setdefault("use_graphs", False)
    torch.manual_seed(seed)
    agent = MAPPOAgent(obs_space, act_space, hidden_dim=hidden_dim, entropy_coef=ENT_COEF, clip_param=CLIP,
                       action_scale=action_scale, device=device, **agent_kw)
    with torch.no_grad():
        agent.ac.actor.logstd.copy_(torch.linspace(-0.7, -0.3, A))
    return agent


def draw(agent, mb, D, O, A, action_scale, seed, T_E, device):
    """The inputs of one minibatch of mb env-timesteps out of a table of
    T_E > mb, from a CPU generator seeded with `seed`; the old
    log-probabilities from the float64 copy of `agent`'s actor."""
    assert T_E > mb
    g = torch.Generator().manual_seed(seed)
    dev = torch.device(device)
    case = types.SimpleNamespace(mb=mb, D=D, O=O, A=A, scale=float(action_scale), seed=seed, T_E=T_E, device=dev,
                                 agent=agent)
    case.obs = torch.randn((T_E, D, O), generator=g).to(dev)
    case.act = torch.randn((T_E, D, A), generator=g).to(dev)
    case.adv_env = torch.randn(T_E, generator=g, dtype=torch.float64).to(dev)
    case.ret_env = torch.randn(T_E, generator=g, dtype=torch.float64).to(dev)
    noise = torch.randn(T_E * D, generator=g, dtype=torch.float64).to(dev)
    perm = torch.randperm(T_E, generator=g).to(dev)
    case.idx = perm[:mb].contiguous()
    case.idx2 = perm[T_E - mb:].contiguous()   # another draw (disjoint from the first when T_E >= 2·mb)
    # old log-probabilities of every table row, from the float64 copy of the actor
    with torch.no_grad():
        p64 = {k: v.detach().double() for k, v in param_tensors(case).items()}
        logp64 = _logp(p64, case.scale, case.obs.reshape(-1, O).double(), case.act.reshape(-1, A).double())
    logp_old = logp64 + NOISE * noise
    case.logp_old_unguarded = logp_old.float()
    ratio = torch.exp(logp64 - logp_old)
    for bound in (1.0 - CLIP, 1.0 + CLIP):
        near = (ratio - bound).abs() < GUARD
        moved = torch.where(ratio < bound, torch.full_like(ratio, bound - GUARD_SHIFT),
                            torch.full_like(ratio, bound + GUARD_SHIFT))
        logp_old = torch.where(near, logp64 - torch.log(moved), logp_old)
    case.logp_old = logp_old.float()
    case._ref, case._e32 = {}, {}
    return case


def build(mb, D, O, A, action_scale, seed, T_E, device, w1p=True):
    """The nets as MAPPOAgent(hidden_dim=256, small=True) builds them (inside
    FlatBuffers), their qs_mlp256 structs, and the inputs of one minibatch of
    mb env-timesteps out of a table of T_E > mb."""
    from gym_pybullet_drones_amd import _lib as L
    from gym_pybullet_drones_amd.mappo.agent import _mlp256
    agent = make_agent(D, O, A, action_scale, seed, device, small=True)
    case = draw(agent, mb, D, O, A, action_scale, seed, T_E, device)
    dev = case.device
    # the path's own copies: W2ᵀ of both nets and (w1p) W1 padded to whole 16-column quads
    mlps = (agent.ac.actor.pi_net, agent.ac.critic.v_net)
    case.w2t = [m.fcs[1].weight.detach().t().contiguous() for m in mlps]
    case.w1p = None
    if w1p:
        case.w1p = [torch.zeros((256, (m.fcs[0].in_features + 15) // 16 * 16), device=dev) for m in mlps]
        for wp, m in zip(case.w1p, mlps):
            wp[:, :m.fcs[0].in_features].copy_(m.fcs[0].weight.detach())
    case.nets = (_mlp256(agent.actor_opt, mlps[0], agent.ac.actor.logstd, case.w2t[0], L.QsMlp256,
                         case.w1p[0] if w1p else None),
                 _mlp256(agent.critic_opt, mlps[1], None, case.w2t[1], L.QsMlp256, case.w1p[1] if w1p else None))
    return case


_built = {}


def get_case(i, device):
    """Case CASES[i] on `device`, built once per process (its float64 reference
    is cached on it: no test changes either)."""
    key = (i, str(device))
    if key not in _built:
        c = CASES[i]
        _built[key] = build(c["mb"], c["D"], c["O"], c["A"], c["scale"], c["seed"], 2 * c["mb"], device, c["w1p"])
    return _built[key]


def losses(case, idx, dtype, logp_old=None, clamp=True):
    """compute_policy_loss / compute_value_loss (AG:602-683) restated over the
    whole nets in `dtype` with autograd: the gradients of policy + ent_coef ·
    entropy + value by every parameter, the losses and the per-row terms.
    clamp=False: the policy loss without its clipped term (a fault the tests'
    metric must see, never the reference)."""
    p = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in param_tensors(case).items()}
    rows = actor_rows(case, idx)
    lpo = (case.logp_old if logp_old is None else logp_old)[rows].to(dtype)
    logp = _logp(p, case.scale, case.obs.reshape(-1, case.O)[rows].to(dtype),
                 case.act.reshape(-1, case.A)[rows].to(dtype))
    adv = case.adv_env[idx].to(dtype).repeat_interleave(case.D)
    ratio = torch.exp(logp - lpo)
    min_term = torch.min(ratio * adv, torch.clamp(ratio, 1.0 - CLIP, 1.0 + CLIP) * adv) if clamp else ratio * adv
    policy = -min_term.mean()
    ent = (0.5 + 0.5 * math.log(2 * math.pi) + p["actor.logstd"]).sum()   # Normal.entropy summed over A (any row)
    entropy = -ent
    approx_kl = (lpo - logp).mean()
    v = _mlp(p, "critic", case.obs.reshape(case.T_E, case.D * case.O)[idx].to(dtype))[:, 0]
    value = 0.5 * ((v - case.ret_env[idx].to(dtype)) ** 2).mean()
    (policy + ENT_COEF * entropy + value).backward()
    return dict(grads={k: t.grad.detach() for k, t in p.items()}, policy=policy.item(), value=value.item(),
                entropy=entropy.item(), approx_kl=approx_kl.item(), ratio=ratio.detach(), adv=adv.detach(),
                mean_abs_min_term=min_term.detach().abs().mean().item(),
                mean_abs_dlogp=(lpo - logp).detach().abs().mean().item())


def reference(case, which="idx"):
    """The float64 reference of the case's minibatch `which` ("idx" or "idx2"), computed once."""
    if which not in case._ref:
        case._ref[which] = losses(case, getattr(case, which), torch.float64)
    return case._ref[which]


def rel_err(g, g64):
    """max|g − g64| / max|g64| of one tensor."""
    g64 = g64.double()
    return ((g.double() - g64).abs().max() / g64.abs().max()).item()


def fp32_autograd_errors(case, which="idx"):
    """rel_err of torch's own float32 autograd against the float64 reference, per tensor."""
    ref = reference(case, which)["grads"]
    got = losses(case, getattr(case, which), torch.float32)["grads"]
    return {k: rel_err(got[k], ref[k]) for k in NAMES}


def row_groups(ref):
    """The minibatch's rows by clip branch: inside the bounds; outside with zero
    gradient (the min picks the clamped term); outside on the side that still
    carries gradient."""
    r, a = ref["ratio"], ref["adv"]
    lo, hi = 1.0 - CLIP, 1.0 + CLIP
    inside = (r >= lo) & (r <= hi)
    zero = ((r > hi) & (a > 0)) | ((r < lo) & (a < 0))
    live = ((r > hi) & (a < 0)) | ((r < lo) & (a > 0))
    return inside, zero, live


def check_against_float64(cid, case, which, grads, acc, kl, bound, names=NAMES, losses_too=True):
    """The GPU suites' conditions on one minibatch: every tensor of `names`
    within `bound` of the float64 reference under rel_err (printed beside
    float32 autograd's figure); the policy loss within 1e-6 of mean|min-term|,
    approx_kl (acc[3] and the kl slot) within 1e-5 of mean|dlogp|, the value
    and entropy losses within 1e-6 relative.  Returns the errors by name."""
    ref = reference(case, which)
    if which not in case._e32:
        case._e32[which] = fp32_autograd_errors(case, which)
    e32 = case._e32[which]
    errs = {}
    for k in names:
        assert grads[k].shape == ref["grads"][k].shape and bool(torch.isfinite(grads[k]).all()), (cid, which, k)
        errs[k] = rel_err(grads[k], ref["grads"][k])
        print(f"{cid} {which} {k}: e = {errs[k]:.2e} (float32 autograd {e32[k]:.2e})")
    bad = {k: (v, e32[k]) for k, v in errs.items() if not v <= bound}
    assert not bad, (cid, which, bad)
    if not losses_too:
        return errs
    pol, val, ent, akl = (float(x) for x in acc)
    d_pol, d_kl = abs(pol - ref["policy"]), max(abs(float(kl) - ref["approx_kl"]), abs(akl - ref["approx_kl"]))
    print(f"{cid} {which} losses: policy {d_pol / ref['mean_abs_min_term']:.1e} of mean|min-term|, approx_kl "
          f"{d_kl / ref['mean_abs_dlogp']:.1e} of mean|dlogp|, value {abs(val / ref['value'] - 1):.1e}, "
          f"entropy {abs(ent / ref['entropy'] - 1):.1e} relative")
    assert d_pol <= 1e-6 * ref["mean_abs_min_term"], (pol, ref["policy"])
    assert d_kl <= 1e-5 * ref["mean_abs_dlogp"], (float(kl), akl, ref["approx_kl"])
    assert abs(val - ref["value"]) <= 1e-6 * abs(ref["value"]), (val, ref["value"])
    assert abs(ent - ref["entropy"]) <= 1e-6 * abs(ref["entropy"]), (ent, ref["entropy"])
    return errs
