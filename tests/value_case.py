"""The shared helpers of tests/test_gpu_value_tail.py (a plain module, not a conftest): the
value tail's launch on caller-owned buffers, its references (torch's float32 forward, the
float64 normaliser, the NumPy restatement of the fold) and the float64 restatements of the MPPI
update and the CEM refit, copied from tests/test_gpu_mppi.py and tests/test_gpu_cem.py."""
import ctypes

import numpy as np
import torch
import torch.nn.functional as F

from gym_pybullet_drones_amd import _lib as L
from gym_pybullet_drones_amd.envs.swarm import value_spec
from gym_pybullet_drones_amd.mappo.agent import CentralizedCritic
from gym_pybullet_drones_amd.mappo.normalization import MeanStdNormalizer

RTOL = ATOL = 1e-5   # tests/test_learner_splitk.py::test_fused_inference_forward holds qs_mlp3_fwd to these
SPIRAL64 = dict(task="spiral", num_drones=5, num_envs=3, act="vel", precision=8)
MPPI_BUFS = ("nominal", "candidates", "ret", "first_done", "weights", "best", "action", "tick")
CEM_BUFS = ("mean", "std", "candidates", "ret", "first_done", "elites", "iter_best", "action", "tick")


def critic_of(I, N, seed, device, gain=1.0):
    """A CentralizedCritic with nn.Linear's default initialisation, drawn on the CPU from `seed`."""
    torch.manual_seed(seed)
    critic = CentralizedCritic(I, (N, N), "tanh")
    with torch.no_grad():
        for p in critic.parameters():
            p.mul_(gain)
    return critic.to(device)


def weights_of(critic):
    return [t.detach() for fc in critic.v_net.fcs for t in (fc.weight, fc.bias)]


def normalizer_of(I, seed, device, zero_var_col=None):
    """A read-only MeanStdNormalizer over I columns with random statistics; `zero_var_col` has var = 0."""
    gen = torch.Generator().manual_seed(seed)
    nz = MeanStdNormalizer(shape=(I,), read_only=True, clip=10.0, epsilon=1e-8, device=device)
    nz.rms.mean.copy_(torch.randn(I, generator=gen, dtype=torch.float64) * 0.5)
    var = torch.rand(I, generator=gen, dtype=torch.float64) * 2 + 0.25
    if zero_var_col is not None:
        var[zero_var_col] = 0.0
    nz.rms.var.copy_(var)
    return nz


def normalise64(x, nz):
    """clamp((x - mean) / sqrt(var + eps), +-clip) in float64, rounded to float32."""
    y = (x.to(torch.float64) - nz.rms.mean) / torch.sqrt(nz.rms.var + nz.epsilon)
    return torch.clamp(y, -nz.clip, nz.clip).to(torch.float32)


def forward32(x, critic, nz=None):
    """torch's float32 nn.Linear / tanh forward over the rows of x (V, I)."""
    w1, b1, w2, b2, w3, b3 = weights_of(critic)
    if nz is not None:
        x = normalise64(x, nz)
    return F.linear(torch.tanh(F.linear(torch.tanh(F.linear(x, w1, b1)), w2, b2)), w3, b3).reshape(-1)


def assert_close(got, want, what):
    got, want = got.reshape(-1).double().cpu(), want.reshape(-1).double().cpu()
    err = (got - want).abs()
    allowed = ATOL + RTOL * want.abs()
    print(f"{what}: max abs difference {err.max().item():.3e} (allowed at that element "
          f"{allowed[err.argmax()].item():.3e}), largest |value| {want.abs().max().item():.3f}")
    assert torch.isfinite(got).all() and (err <= allowed).all(), what


def tail(spec, n, C, E, D, O, last_obs, rewards, ret, first_done, value):
    """qs_value_tail on caller-owned tensors; rewards: None or a list of n (C, E) tensors."""
    real = 4
    arr = None
    if rewards is not None:
        real = rewards[0].element_size()
        arr = (ctypes.c_void_p * n)(*[r.data_ptr() for r in rewards])
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    return L.load().qs_value_tail(ctypes.byref(spec), n, C, E, D, O, real, L.ptr(last_obs), arr, L.ptr(ret),
                                  L.ptr(first_done), L.ptr(value), st)


def fold64(n, gamma, scale, first_done, value=None, rewards=None, ret=None):
    """The fold in NumPy float64, in the kernel's order of operations.  first_done (C, E) int32;
    value (C, E) float32 or None (no net); rewards (n, C, E) for gamma != 1, else `ret` (C, E)
    float64, the score launch's own sum."""
    disc = [1.0]
    for _ in range(n):
        disc.append(disc[-1] * float(gamma))
    fd = np.asarray(first_done)
    if gamma != 1.0:
        acc = np.zeros(fd.shape, np.float64)
        last = np.minimum(fd, n - 1)
        for j in range(n):
            term = np.float64(disc[j]) * np.asarray(rewards[j]).astype(np.float64)
            acc = np.where(j <= last, acc + term, acc)
    else:
        acc = np.asarray(ret, np.float64).copy()
    if value is not None:
        boot = np.float64(disc[n] * float(scale))
        acc = np.where(fd == n, acc + boot * np.asarray(value).astype(np.float64), acc)
    return acc


def raw_set(pl, spec):
    """qs_value_mppi_set / qs_value_cem_set with a hand-built spec (None: NULL); returns (rc, message)."""
    fn = getattr(pl.lib, f"qs_value_{pl._PREFIX[3:]}_set")
    with torch.cuda.device(pl.swarm.device):
        rc = fn(pl._p, None if spec is None else ctypes.byref(spec))
    return rc, (pl.lib.qs_last_error() or b"").decode()


def full_spec(critic, nz=None, gamma=1.0, scale=1.0):
    return value_spec(critic, gamma, scale, nz)


# ---- the float64 restatements of the stages that read ret (tests/test_gpu_mppi.py, tests/test_gpu_cem.py)
def mppi_restate(pl, lam, penalty):
    """The update in float64 numpy, from the planner's own candidates, ret and first_done."""
    torch.cuda.synchronize()
    cand = pl.candidates.cpu().numpy().astype(np.float64)      # (n, C, E, D, A)
    ret, fd = pl.ret.cpu().numpy(), pl.first_done.cpu().numpy()
    n, C = cand.shape[0], cand.shape[1]
    s = ret - np.where(fd < n, np.float64(penalty), 0.0)
    best = np.argmax(s, axis=0)                                   # the first, i.e. lowest, c of the maximum
    if lam > 0:
        x = np.exp((s - s.max(axis=0)) / lam)
        w = x / x.sum(axis=0)
    else:
        w = (np.arange(C)[:, None] == best[None, :]).astype(np.float64)
    new = np.einsum("ce,jceda->jeda", w, cand)
    return dict(best=best.astype(np.int32), weights=w, new=new, action=new[0],
                nominal=np.concatenate([new[1:], new[-1:]], axis=0))


def mppi_check_update(pl, lam, penalty, bound, tick):
    """The planner's buffers after an update against the restatement (made from the same buffers)."""
    want = mppi_restate(pl, lam, penalty)
    best, w = pl.best.cpu().numpy(), pl.weights.cpu().numpy()
    nominal, action = pl.nominal.cpu().numpy().astype(np.float64), pl.action.cpu().numpy().astype(np.float64)
    assert np.array_equal(best, want["best"])
    rel = np.abs(w - want["weights"]) / np.maximum(want["weights"], np.finfo(np.float64).tiny)
    print("weights: max relative difference", rel.max(), "sum - 1", np.abs(w.sum(axis=0) - 1).max())
    assert rel.max() <= 1e-12
    tol = 2.0 ** -23 * bound
    print("nominal: max abs difference", np.abs(nominal - want["nominal"]).max(), "allowed", tol)
    assert np.abs(nominal - want["nominal"]).max() <= tol and np.abs(action - want["action"]).max() <= tol
    n = nominal.shape[0]
    assert np.array_equal(nominal[-1], nominal[-2] if n > 1 else nominal[0])
    assert int(pl.tick.item()) == tick
    return want


def cem_restate(pl, mean0, std0):
    """Select + refit in float64 numpy, from the planner's own candidates, ret and first_done
    and the mean / std from before the refit."""
    torch.cuda.synchronize()
    cand = pl.candidates.cpu().numpy().astype(np.float64)      # (n, C, E, D, A)
    ret, fd = pl.ret.cpu().numpy(), pl.first_done.cpu().numpy()
    n, C, E, _, A = cand.shape
    K, alpha = pl.num_elites, float(pl.spec.alpha)
    sigma = np.array(list(pl.spec.sigma)[:A], np.float32)
    smin = np.array(list(pl.spec.sigma_min)[:A], np.float32)
    with np.errstate(invalid="ignore"):
        s = ret - np.where(fd < n, np.float64(pl.spec.done_penalty), 0.0)
    nan = np.isnan(s)
    neg = np.where(nan, 0.0, -s)
    elites = np.empty((K, E), np.int32)
    best = np.empty(E, np.float64)
    mean, std = np.empty(cand.shape[:1] + cand.shape[2:]), np.empty(cand.shape[:1] + cand.shape[2:])
    for e in range(E):
        order = np.lexsort((np.arange(C), neg[:, e], nan[:, e]))   # numbers first, larger s first, lower c on ties
        elites[:, e] = order[:K]
        best[e] = s[order[0], e]
        x = cand[:, order[:K], e]                                     # (n, K, D, A)
        m = x.sum(axis=1) / K
        v = ((x - m[:, None]) ** 2).sum(axis=1) / K
        mean[:, e], std[:, e] = m, np.sqrt(v)
    if alpha != 0.0:
        mean = (1 - alpha) * mean + alpha * mean0.astype(np.float64)
        std = (1 - alpha) * std + alpha * std0.astype(np.float64)
    std = np.where(sigma == 0, std0.astype(np.float64), np.maximum(std, smin.astype(np.float64)))
    return dict(elites=elites, best=best, mean=mean, std=std)


def cem_refit_and_check(pl, iteration=0):
    """refit(iteration) against the restatement made from the buffers as they are now."""
    torch.cuda.synchronize()
    mean0, std0 = pl.mean.cpu().numpy().copy(), pl.std.cpu().numpy().copy()
    pl.refit(iteration)
    want = cem_restate(pl, mean0, std0)
    elites, best = pl.elites.cpu().numpy(), pl.iter_best.cpu().numpy()[iteration]
    mean, std = pl.mean.cpu().numpy().astype(np.float64), pl.std.cpu().numpy().astype(np.float64)
    assert np.array_equal(elites, want["elites"])
    assert np.array_equal(best, want["best"], equal_nan=True)
    lo, hi = float(pl.spec.lo), float(pl.spec.hi)
    tol_m, tol_s = 2.0 ** -23 * max(abs(lo), abs(hi)), 2.0 ** -23 * (hi - lo)
    dm, ds = np.abs(mean - want["mean"]).max(), np.abs(std - want["std"]).max()
    print(f"mean: max abs difference {dm} (allowed {tol_m}); std: {ds} (allowed {tol_s})")
    assert dm <= tol_m and ds <= tol_s
    return want
