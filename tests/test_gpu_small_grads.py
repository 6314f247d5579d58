"""The tile learner (csrc/ppo_small.hip) against float64, before Adam.

* qs_ppo_small_grads: the raw gradients of all 13 tensors, the losses and
  approx_kl against a float64 autograd restatement through the whole nets
  (tests/small_grads_case.py), on data with 30-50 % of the rows outside the
  clip bounds: every forward/backward instance of s_launch_fb (16 / 32 / 48-row
  tiles, narrow and wide, 1-4 outputs, layer 1 with and without the padded W1
  copies), the weight gradients in one chunk and in K-chunks.
* qs_ppo_small_adam from given gradients against torch.optim.Adam, gate open
  and closed.
* qs_wgrad_t against a float64 matmul per chunk.
* qs_ppo_critic_tiles: the transposed activations and per-tile partial rows it
  leaves in the workspace against the float64 forward / backward.

The gradient bound, e = max|g − g64| / max|g64| <= 2e-5 per tensor, is 16 times
what torch's own float32 autograd gives under the same metric on the same data
(<= 1.2e-6 measured, <= 2.5e-6 asserted in tests/test_small_grads_cases.py);
one row dropped or doubled at 120 rows moves a tensor by ~8e-3, a wrong tile or
chunk at the large shapes by >= 1e-3, a wrong normaliser by >= 0.5.
"""
import ctypes
import math

import pytest
import torch

import small_grads_case as sg

pytestmark = pytest.mark.gpu

GRAD_BOUND = 2e-5


def _L():
    from gym_pybullet_drones_amd import _lib as L
    return L


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _work(case):
    L = _L()
    n = int(L.load().qs_ppo_small_work_bytes(case.mb, case.D, case.O, case.D * case.O, case.A))
    assert n > 0
    return torch.zeros(n, dtype=torch.uint8, device="cuda")   # zeroed once


def _grads_call(case, idx, work, acc):
    """One qs_ppo_small_grads call, the arguments as MAPPOAgent._iteration_small passes them."""
    L, a = _L(), case.agent
    na, nc = case.nets
    L.check(L.load().qs_ppo_small_grads(case.mb, case.D, L.ptr(case.obs), L.ptr(idx), L.ptr(case.act),
                                        L.ptr(case.logp_old), L.ptr(case.adv_env), L.ptr(case.ret_env), case.scale,
                                        sg.CLIP, sg.ENT_COEF, ctypes.byref(na), ctypes.byref(nc),
                                        L.ptr(a.actor_opt.grad), L.ptr(a.critic_opt.grad), L.ptr(a._kl), L.ptr(acc),
                                        L.ptr(work), _stream()), "qs_ppo_small_grads")


def _state(case):
    a = case.agent
    s = {}
    for k, fb in (("actor", a.actor_opt), ("critic", a.critic_opt)):
        s.update({k + ".flat": fb.flat.clone(), k + ".m": fb.exp_avg.clone(), k + ".v": fb.exp_avg_sq.clone(),
                  k + ".step": fb.step.clone()})
    for k in range(2):
        s[f"w2t{k}"] = case.w2t[k].clone()
        if case.w1p is not None:
            s[f"w1p{k}"] = case.w1p[k].clone()
    return s


def _run(case, idx, work):
    """NaN-filled gradient buffers (every parameter element must be written),
    zeroed statistics, one call: the 13 gradients, acc[4] and kl_out."""
    a = case.agent
    a._reduce_buf.fill_(float("nan"))
    acc = torch.zeros(4, dtype=torch.float64, device="cuda")
    _grads_call(case, idx, work, acc)
    torch.cuda.synchronize()
    grads = {k: p.grad.clone() for k, p in sg.param_tensors(case).items()}
    return grads, acc.clone(), a._kl.clone()


def _check_against_float64(cid, case, which, grads, acc, kl):
    return sg.check_against_float64(cid, case, which, grads, acc, kl, GRAD_BOUND)


@pytest.mark.parametrize("i", range(len(sg.CASES)), ids=sg.CASE_IDS)
def test_small_grads_match_float64(i):
    """qs_ppo_small_grads' raw gradients, losses and approx_kl against float64
    autograd; a second call on the same workspace with another idx draw meets
    the same bounds, and repeating the first draw gives the first call's bits
    (the counters, the padding columns and the bias-correction slot are left
    ready); the parameters, moments and step counts are not touched."""
    cid, case = sg.CASE_IDS[i], sg.get_case(i, "cuda")
    before = _state(case)
    work = _work(case)
    g1, acc1, kl1 = _run(case, case.idx, work)
    _check_against_float64(cid, case, "idx", g1, acc1, kl1)
    g2, acc2, kl2 = _run(case, case.idx2, work)
    _check_against_float64(cid, case, "idx2", g2, acc2, kl2)
    g3, acc3, kl3 = _run(case, case.idx, work)
    for k in sg.NAMES:
        assert torch.equal(g3[k], g1[k]), (cid, k)
    assert torch.equal(acc3, acc1) and torch.equal(kl3, kl1)
    after = _state(case)
    for k in before:
        assert torch.equal(before[k], after[k]), (cid, k)


def _copies_current(case, nets=(0, 1)):
    """_assert_small_copies_current's conditions (tests/test_gpu_learner.py) on the case's copies."""
    mlps = (case.agent.ac.actor.pi_net, case.agent.ac.critic.v_net)
    for k in nets:
        I = mlps[k].fcs[0].in_features
        assert torch.equal(case.w2t[k], mlps[k].fcs[1].weight.t())
        assert torch.equal(case.w1p[k][:, :I], mlps[k].fcs[0].weight)
        assert not case.w1p[k][:, I:].any()


@pytest.mark.parametrize("gate_open", [True, False], ids=["gate_open", "gate_closed"])
@pytest.mark.parametrize("i", [0, 5, 6], ids=[sg.CASE_IDS[i] for i in (0, 5, 6)])
def test_small_adam_from_given_gradients(i, gate_open):
    """qs_ppo_small_adam (the Adam launch after the rank all-reduce) from
    gradient buffers and an approx_kl that stand in for two ranks' sums
    (doubled, grad_div = 2), three steps with fresh gradients, against
    torch.optim.Adam fed the same float32 gradients — test_gated_adam_matches_
    torch_adam's tolerances.  Gate open: both nets step and the W2ᵀ / padded
    W1 copies follow; gate closed: no actor element, moment or step count
    moves, the critic steps."""
    L = _L()
    c = sg.CASES[i]
    case = sg.build(c["mb"], c["D"], c["O"], c["A"], c["scale"], c["seed"], 2 * c["mb"], "cuda")   # (stepped: its own)
    a = case.agent
    params = sg.param_tensors(case)
    twins = {k: p.detach().clone().requires_grad_(True) for k, p in params.items()}
    fbs = {"actor": a.actor_opt, "critic": a.critic_opt}
    opts = {n: torch.optim.Adam([twins[k] for k in sg.NAMES if k.startswith(n)], lr=fb.lr, betas=fb.betas, eps=fb.eps)
            for n, fb in fbs.items()}
    before = _state(case)
    work = _work(case)
    acc = torch.zeros(4, dtype=torch.float64, device="cuda")
    na, nc = case.nets
    for it in range(3):
        a._reduce_buf.zero_()
        _grads_call(case, case.idx if it != 1 else case.idx2, work, acc)
        a._reduce_buf.mul_(2.0)   # [critic grads | actor grads | approx_kl]: two equal ranks' sum
        kl = float(a._kl) / 2.0
        for k, p in params.items():
            twins[k].grad = (p.grad / 2.0).clone()
        thr = kl + 0.5 if gate_open else kl - 0.5
        L.check(L.load().qs_ppo_small_adam(case.mb, case.D, ctypes.byref(na), ctypes.byref(nc),
                                           L.ptr(a.actor_opt.grad), L.ptr(a.critic_opt.grad), 2.0, 1, thr,
                                           L.ptr(a._kl), L.ptr(work), _stream()), "qs_ppo_small_adam")
        opts["critic"].step()
        if gate_open:
            opts["actor"].step()
    torch.cuda.synchronize()
    assert float(a.critic_opt.step) == 3.0 and float(a.actor_opt.step) == (3.0 if gate_open else 0.0)
    stepped = ["actor", "critic"] if gate_open else ["critic"]
    for k in sg.NAMES:
        n = k.split(".")[0]
        if n not in stepped:
            continue
        torch.testing.assert_close(params[k], twins[k], rtol=2e-6, atol=2e-7, msg=lambda m, k=k: f"{k}: {m}")
        fb = fbs[n]
        off, cnt = fb.offsets[[id(p) for p in fb.params].index(id(params[k]))]
        torch.testing.assert_close(fb.exp_avg[off:off + cnt].view_as(params[k]), opts[n].state[twins[k]]["exp_avg"],
                                   rtol=1e-5, atol=1e-9, msg=lambda m, k=k: f"exp_avg of {k}: {m}")
    if gate_open:
        assert not torch.equal(before["actor.flat"], a.actor_opt.flat)
        _copies_current(case)
    else:
        after = _state(case)
        for k in ("actor.flat", "actor.m", "actor.v", "actor.step", "w2t0", "w1p0"):
            assert torch.equal(before[k], after[k]), k
        _copies_current(case, nets=(1,))
    assert not torch.equal(before["critic.flat"], a.critic_opt.flat)


@pytest.mark.parametrize("N,M,KP,S,ld", [(16, 1, 16, 1, 16), (256, 27, 64, 1, 80), (256, 216, 128, 4, 144),
                                        (32, 595, 192, 3, 208)])
def test_wgrad_t_matches_float64(N, M, KP, S, ld):
    """qs_wgrad_t's chunk partials against a float64 matmul per chunk.  The
    columns KP..ld of both operands hold 1e30 (never read), the partials start
    as NaN (every element written).  Bound: 2e-6·max|p64| — 16 · 2⁻²⁴ · the
    √K-scale rounding of a sum over K <= 64 rows per chunk."""
    L = _L()
    g = torch.Generator().manual_seed(7 + N + M)
    at = torch.randn((N, ld), generator=g).cuda()
    xt = torch.randn((M, ld), generator=g).cuda()
    at[:, KP:] = 1e30
    xt[:, KP:] = 1e30
    part = torch.full((S, N, M), float("nan"), device="cuda")
    L.check(L.load().qs_wgrad_t(KP, ld, N, M, L.ptr(at), L.ptr(xt), S, L.ptr(part), _stream()), "qs_wgrad_t")
    torch.cuda.synchronize()
    rows = KP // S
    assert rows <= 64
    for s in range(S):
        sl = slice(s * rows, (s + 1) * rows)
        p64 = at[:, sl].double() @ xt[:, sl].double().T
        err = ((part[s].double() - p64).abs().max() / p64.abs().max()).item()
        print(f"qs_wgrad_t N={N} M={M} KP={KP} S={S} chunk {s}: max|p - p64| / max|p64| = {err:.2e}")
        assert bool(torch.isfinite(part[s]).all())
        assert err <= 2e-6, (s, err)


@pytest.mark.parametrize("mb,D,O,seed", [(15, 8, 27, 32), (64, 8, 27, 31), (9, 5, 119, 31)])
def test_critic_tiles_intermediates_match_float64(mb, D, O, seed):
    """qs_ppo_critic_tiles' workspace (the Ia = 0 layout) against the float64
    forward / backward of the critic: Xᵀ exact, H1ᵀ within 1e-6, dZ2ᵀ and dZ1ᵀ
    under the gradient metric; past the minibatch's mb columns Xᵀ, dZ2ᵀ and
    dZ1ᵀ are exactly zero up to the row stride, and so is H1ᵀ past the tiles'
    rows — inside the last tile its padding rows hold H1 of an all-zero input
    (tanh(b1)), which the weight gradients multiply by dZ2 = 0.  The per-tile
    partial rows sum to db2, dW3, db3 and db1; acc[1] is the value loss."""
    L = _L()
    I = D * O
    case = sg.build(mb, D, O, 1, 1.0, seed, 2 * mb, "cuda", w1p=I > 256)   # (<= 256 inputs: layer 1 from the parameters)
    off = (ctypes.c_int64 * L.QS_PPO_SMALL_LAYOUT_N)()
    L.check(L.load().qs_ppo_small_layout(mb, D, 0, I, 1, off, len(off)), "qs_ppo_small_layout")
    nC, KcP, ld = int(off[17]), int(off[19]), int(off[22])
    assert mb <= KcP <= ld and nC == (mb + 15) // 16
    work = torch.zeros(int(off[20]), dtype=torch.uint8, device="cuda")
    view = lambda i, *shape: work[off[i]:off[i] + 4 * math.prod(shape)].view(torch.float32).view(*shape)
    xT, h1T, dz2T, dz1T = view(4, I, ld), view(5, 256, ld), view(6, 256, ld), view(7, 256, ld)
    part_a, part_b = view(10, nC, 513), view(11, nC, 256)
    acc = torch.zeros(4, dtype=torch.float64, device="cuda")
    L.check(L.load().qs_ppo_critic_tiles(mb, D, L.ptr(case.obs), L.ptr(case.idx), L.ptr(case.ret_env),
                                         ctypes.byref(case.nets[1]), L.ptr(acc), L.ptr(work), _stream()),
            "qs_ppo_critic_tiles")
    torch.cuda.synchronize()
    p = {k: v.detach().double() for k, v in sg.param_tensors(case).items()}
    X32 = case.obs.reshape(case.T_E, I)[case.idx]
    X = X32.double()
    H1 = torch.tanh(X @ p["critic.W1"].T + p["critic.b1"])
    H2 = torch.tanh(H1 @ p["critic.W2"].T + p["critic.b2"])
    v = (H2 @ p["critic.W3"].T + p["critic.b3"])[:, 0]
    dv = (v - case.ret_env[case.idx]) / mb
    dZ2 = dv[:, None] * p["critic.W3"] * (1 - H2 ** 2)
    dZ1 = (dZ2 @ p["critic.W2"]) * (1 - H1 ** 2)
    assert torch.equal(xT[:, :mb], X32.T)
    e_h1 = (h1T[:, :mb].double() - H1.T).abs().max().item()
    e_z2, e_z1 = sg.rel_err(dz2T[:, :mb], dZ2.T), sg.rel_err(dz1T[:, :mb], dZ1.T)
    print(f"critic tiles mb={mb} I={I}: |H1 - H1_64| {e_h1:.2e}, dZ2 e = {e_z2:.2e}, dZ1 e = {e_z1:.2e}")
    assert e_h1 <= 1e-6 and e_z2 <= GRAD_BOUND and e_z1 <= GRAD_BOUND
    for name, t in (("xT", xT), ("dz2T", dz2T), ("dz1T", dz1T)):
        assert not t[:, mb:].any(), name
    assert not h1T[:, KcP:].any()
    if KcP > mb:
        pad = torch.tanh(p["critic.b1"])[:, None].expand(256, KcP - mb)
        assert (h1T[:, mb:KcP].double() - pad).abs().max().item() <= 1e-6
    ref = sg.reference(case)
    sums = {"critic.b2": part_a[:, :256].double().sum(0), "critic.W3": part_a[:, 256:512].double().sum(0)[None, :],
            "critic.b3": part_a[:, 512].double().sum(0).reshape(1), "critic.b1": part_b.double().sum(0)}
    for k, got in sums.items():
        e = sg.rel_err(got, ref["grads"][k])
        print(f"critic tiles mb={mb} I={I} {k} from the partial rows: e = {e:.2e}")
        assert e <= GRAD_BOUND, (k, e)
    assert float(acc[1]) == pytest.approx(ref["value"], rel=1e-6)
    assert float(acc[0]) == 0.0 and float(acc[2]) == 0.0 and float(acc[3]) == 0.0
