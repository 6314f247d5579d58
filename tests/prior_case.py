"""The shared helpers of tests/test_gpu_prior.py (a plain module, not a conftest): actors and
normalisers drawn from a seed, the actor launch on caller-owned buffers (qs_prior_act) and its
reference, torch's float32 forward behind the float64 normaliser."""
import ctypes

import torch
import torch.nn.functional as F

from gym_pybullet_drones_amd import _lib as L
from gym_pybullet_drones_amd.mappo.agent import MLPActor
from gym_pybullet_drones_amd.mappo.normalization import MeanStdNormalizer

WIDE = 1e6   # bounds that clip nothing


def actor_of(O, A, N, seed, device, action_scale=1.0):
    """An MLPActor with nn.Linear's default initialisation drawn on the CPU from `seed`, and a
    different logstd per component."""
    torch.manual_seed(seed)
    actor = MLPActor(O, A, [N, N], "tanh", False, action_scale)
    with torch.no_grad():
        actor.logstd.copy_(torch.linspace(-0.9, -0.3, A))
    return actor.to(device)


def constant_actor(O, A, u, device):
    """Zero weights and b3 = u: the net's output is exactly u whatever it sees."""
    actor = actor_of(O, A, 64, 1, device)
    with torch.no_grad():
        for p in actor.pi_net.parameters():
            p.zero_()
        actor.pi_net.fcs[2].bias.fill_(u)
    return actor


def weights_of(actor):
    return [t.detach() for fc in actor.pi_net.fcs for t in (fc.weight, fc.bias)]


def normalizer_of(D, O, seed, device, zero_var_col=None):
    """A read-only MeanStdNormalizer over an env's (D, O) obs with random statistics, different
    for every drone; column `zero_var_col` of every drone has var = 0."""
    gen = torch.Generator().manual_seed(seed)
    nz = MeanStdNormalizer(shape=(D, O), read_only=True, clip=10.0, epsilon=1e-8, device=device)
    nz.rms.mean.copy_(torch.randn((D, O), generator=gen, dtype=torch.float64) * 0.5)
    var = torch.rand((D, O), generator=gen, dtype=torch.float64) * 2 + 0.25
    if zero_var_col is not None:
        var[:, zero_var_col] = 0.0
    nz.rms.var.copy_(var)
    return nz


def forward32(x, actor, nz=None):
    """torch's float32 forward times action_scale over x (..., D, O): (..., D, A).  The normaliser
    is clamp((x - mean) / sqrt(var + eps), +-clip) in float64, rounded to float32."""
    w1, b1, w2, b2, w3, b3 = weights_of(actor)
    if nz is not None:
        y = (x.to(torch.float64) - nz.rms.mean) / torch.sqrt(nz.rms.var + nz.epsilon)
        x = torch.clamp(y, -nz.clip, nz.clip).to(torch.float32)
    return F.linear(torch.tanh(F.linear(torch.tanh(F.linear(x, w1, b1)), w2, b2)), w3, b3) * actor.action_scale


def act(spec, j, K, E, D, obs_in, bcast, tick, lo=-WIDE, hi=WIDE, seed=0, genv0=0, seen=True):
    """qs_prior_act on fresh output tensors: (rc, actions (K, E, D, A), obs_seen (K, E, D, O) or None)."""
    dev = obs_in.device
    actions = torch.full((K, E, D, spec.act_dim), float("nan"), device=dev)
    obs_seen = torch.full((K, E, D, spec.in_dim), float("nan"), device=dev) if seen else None
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = L.load().qs_prior_act(ctypes.byref(spec), j, K, E, D, lo, hi, seed, genv0, L.ptr(tick), L.ptr(obs_in), int(bcast),
                               L.ptr(actions), L.ptr(obs_seen), st)
    torch.cuda.synchronize()
    return rc, actions, obs_seen


def raw_set(pl, spec):
    """qs_prior_mppi_set / qs_prior_cem_set with a hand-built spec (None: NULL); returns (rc, message)."""
    fn = getattr(pl.lib, f"qs_prior_{pl._PREFIX[3:]}_set")
    with torch.cuda.device(pl.swarm.device):
        rc = fn(pl._p, None if spec is None else ctypes.byref(spec))
    return rc, (pl.lib.qs_last_error() or b"").decode()
