"""MAPPOAgent._iteration_direct (the 256-wide split-K update of every minibatch
above _SMALL_MAX_ROWS actor rows, and of every rank of a multi-GPU run) against
float64, before Adam, on the cases of tests/direct_grads_case.py: data with
30-50 % of the rows outside the clip bounds, action_scale != 1, 1-4 actor
outputs, ragged and tiny row counts, every split of the weight gradients.

One eager minibatch on a freshly built agent, as update() drives it
(agent._step_minibatch), target_kl = 0.  The one-rank launch qs_mlp_sum_adam
never writes gradients; from zero moments the first step leaves exp_avg =
(1 − β1)·g, so g = exp_avg / (float32(1) − float32(β1)) per tensor, exact to
one rounding (exp_avg_sq / (1 − β2) = g² is the cross-check).

The bound.  e = max|g − g64| / max|g64| <= 2e-5 per tensor, the tile suite's
GRAD_BOUND (tests/test_gpu_small_grads.py): 16 times what torch's own float32
autograd gives under the same metric on the same data (<= 1.5e-6 by the seed
rule, <= 2.5e-6 asserted in tests/test_direct_grads_cases.py).  On the float64
reference a dropped env-timestep moves every tensor by >= 4.9e-4, a missing
clamp every actor tensor by >= 6.5e-2, a dropped action_scale factor the
actor's MLP tensors by 0.43 (same file).

Largest e measured per variant over its cases and both idx draws (MI355X;
for the direct variants it is the actor's logstd, an A-element sum over all
rows, on ragged_185's second draw unless named):
  fused 3.4e-6, fused_vh 3.4e-6, fold_w1 3.4e-6, two_kernel 4.0e-6,
  fused_tiles 2.0e-6 (rows_4096); the critic's tensors <= 1.5e-6 everywhere;
  the fused iteration at hidden 64 / 128: 1.4e-6 (one_agent_3000) / 1.7e-6
  (A3_critic_432), both the actor's W1; on the kernel-run nets of
  one_agent_3000 and spiral_A4 at hidden 128: 1.1e-6 / 1.4e-6.
Torch's float32 autograd on the GPU, printed beside each figure, reaches
5.0e-6 on the same data (the weight matrices at 16 384 rows).  Losses, worst
case: policy 1.1e-7 of mean|min-term|, approx_kl 5.3e-7 of mean|dlogp|, value
1.1e-7 and entropy 2.2e-8 relative.  The side-stream and the graph-replay
bit-identities hold on this data (ragged_185 and rows_4096, fused and
two_kernel), as do the repeat-draw bits and the pack images after three steps,
in all 58 tests of the first run; nothing was found to fix.  With the pack
segments withheld from qs_mlp_sum_adam all 11 pack tests fail, and with one
env-timestep of idx replaced by another all 26 gradient tests fail.
"""
import ctypes

import pytest
import torch

import direct_grads_case as dg
import small_grads_case as sg

pytestmark = pytest.mark.gpu

DEV = "cuda"
ACTOR = [k for k in dg.NAMES if k.startswith("actor.")]
CRITIC = [k for k in dg.NAMES if k.startswith("critic.")]


def _L():
    from gym_pybullet_drones_amd import _lib as L
    return L


def _fbs(run):
    return {"actor": run.agent.actor_opt, "critic": run.agent.critic_opt}


def _step(run, idx):
    """One minibatch the way update() runs it, eager; the loss statistics."""
    acc = torch.zeros(4, dtype=torch.float64, device=DEV)
    run.agent._step_minibatch(run.buf, idx, acc)
    torch.cuda.synchronize()
    return acc


def _one_minus(beta):
    return (torch.tensor(1.0, dtype=torch.float32) - torch.tensor(beta, dtype=torch.float32)).double().item()


def _recover(run, names=dg.NAMES):
    """The raw float32 gradients of the first step from its moments (float64
    holds them exactly but for exp_avg's one rounding); exp_avg_sq must agree:
    g² to the three float32 roundings of (1 − β2)·g·g and of g itself."""
    fbs, out = _fbs(run), {}
    for k, p in dg.run_params(run).items():
        if k not in names:
            continue
        fb = fbs[k.split(".")[0]]
        assert float(fb.step) == 1.0, k
        g = dg.flat_view(fb, p, fb.exp_avg).double() / _one_minus(fb.betas[0])
        g2 = dg.flat_view(fb, p, fb.exp_avg_sq).double() / _one_minus(fb.betas[1])
        torch.testing.assert_close(g2, g * g, rtol=1e-6, atol=1e-30, msg=lambda m, k=k: f"exp_avg_sq of {k}: {m}")
        out[k] = g
    return out


def _state(run):
    """Every bit the step may change: parameters, moments, step counts, pack images."""
    s = {}
    for n, fb in _fbs(run).items():
        s.update({n + ".flat": fb.flat.clone(), n + ".m": fb.exp_avg.clone(), n + ".v": fb.exp_avg_sq.clone(),
                  n + ".step": fb.step.clone()})
    a = run.agent
    s["actor.pack"] = a._ws_actor.pack.clone()
    s["critic.pack"] = (a._ws_critic.w2t if _is(a._ws_critic, "_CriticTiles") else a._ws_critic.pack).clone()
    return s


def _same_bits(x, y):
    return x.shape == y.shape and torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))


def _is(ws, name):
    return type(ws).__name__ == name


def _assert_variant(run):
    """The workspaces the variant names, on the direct path."""
    a, v = run.agent, run.variant
    assert a._direct_ok() and not a._small_ok(run.buf, run.mb) and a._fused_heads_ok(run.buf)
    assert _is(a._ws_actor, "_M3Work" if v == "two_kernel" else "_F16Work")
    assert _is(a._ws_critic, "_CriticTiles" if v == "fused_tiles" else "_M3Work")
    if v != "two_kernel":
        assert (a._ws_actor.pw1f is not None) == (v == "fold_w1")
    assert a.fused_value_head == (v == "fused_vh")


def _check(run, which, grads, acc, kl, names=dg.NAMES, losses_too=True):
    tag = f"{run.cid}-{run.variant}"
    errs = sg.check_against_float64(tag, run.base, which, grads, acc, kl, dg.GRAD_BOUND, names=names,
                                    losses_too=losses_too)
    print(f"{tag} {which}: largest e = {max(errs.values()):.2e}")
    return errs


@pytest.mark.parametrize("cid,variant", dg.RUNS, ids=dg.RUN_IDS)
def test_direct_grads_match_float64(cid, variant):
    """The raw gradients of all 13 tensors, the losses and approx_kl of one
    direct minibatch against float64 autograd; for the fused actor the actor
    output it hands out against the float64 forward (test_fused_inference_
    forward's tolerance); the parameters after the step against a
    torch.optim.Adam twin fed the recovered float32 gradients
    (test_gated_adam_matches_torch_adam's tolerances); a second idx draw
    through a fresh agent meets the same bounds, and repeating the first draw
    on another fresh agent gives the first run's bits."""
    run = dg.fresh(cid, DEV, variant, target_kl=0.0)
    _assert_variant(run)
    b = run.base
    mean = None
    if variant == "fused":
        mean = run.agent._ws_actor.mean = torch.full((run.mb * run.D, run.A), float("nan"), device=DEV)
    start = {k: p.detach().clone() for k, p in dg.run_params(run).items()}
    for k, p in sg.param_tensors(b).items():
        assert torch.equal(start[k], p), k   # the weights the reference was formed from
    acc = _step(run, b.idx)
    grads = _recover(run)
    _check(run, "idx", grads, acc, run.agent._kl)
    if mean is not None:
        p64 = {k: v.double() for k, v in start.items()}
        want = sg._mlp(p64, "actor", b.obs.reshape(-1, b.O)[sg.actor_rows(b, b.idx)].double())
        torch.testing.assert_close(mean.double(), want, rtol=1e-5, atol=1e-5)
    # the step itself
    twins = {k: v.clone().requires_grad_(True) for k, v in start.items()}
    for n, fb in _fbs(run).items():
        mine = [k for k in dg.NAMES if k.startswith(n)]
        for k in mine:
            twins[k].grad = grads[k].float()
        torch.optim.Adam([twins[k] for k in mine], lr=fb.lr, betas=fb.betas, eps=fb.eps).step()
    for k, p in dg.run_params(run).items():
        torch.testing.assert_close(p, twins[k], rtol=2e-6, atol=2e-7, msg=lambda m, k=k: f"{k} after Adam: {m}")
        assert not torch.equal(p, start[k]), k
    # another draw, then the first one again, each through a fresh agent
    run2 = dg.fresh(cid, DEV, variant, target_kl=0.0)
    acc2 = _step(run2, b.idx2)
    _check(run2, "idx2", _recover(run2), acc2, run2.agent._kl)
    run3 = dg.fresh(cid, DEV, variant, target_kl=0.0)
    acc3 = _step(run3, b.idx)
    s1, s3 = _state(run), _state(run3)
    for k in s1:
        assert _same_bits(s1[k], s3[k]), (cid, variant, k)
    assert torch.equal(acc, acc3) and torch.equal(run.agent._kl, run3.agent._kl)


def _fresh_images(run):
    """(name, live image, an image packed from the current weights into a
    NaN-filled buffer of its own) of both workspaces."""
    L, lib = _L(), _L().load()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = []
    for name, ws in (("actor", run.agent._ws_actor), ("critic", run.agent._ws_critic)):
        f0, f1, _ = ws.mlp.fcs
        if _is(ws, "_CriticTiles"):
            out.append((name + " W2ᵀ copy", ws.w2t, f1.weight.detach().t().contiguous()))
            continue
        img = torch.full_like(ws.pack, float("nan"))
        if _is(ws, "_F16Work"):
            L.check(lib.qs_mlp3f_pack(ws.I, L.ptr(f0.weight), L.ptr(f1.weight), L.ptr(img), st), "qs_mlp3f_pack")
        else:
            L.check(lib.qs_mlp3_pack(ws.I, 256, L.ptr(f0.weight), L.ptr(f1.weight), L.ptr(img), st), "qs_mlp3_pack")
        out.append((name + " pack", ws.pack, img))
    torch.cuda.synchronize()
    return out


_PACK_RUNS = [(cid, v) for cid, v in dg.RUNS if cid in ("c3_slice", "spiral_A4", "ragged_185")]


@pytest.mark.parametrize("cid,variant", _PACK_RUNS, ids=[f"{c}-{v}" for c, v in _PACK_RUNS])
def test_pack_images_current_after_three_steps(cid, variant):
    """After three steps (idx, idx2, idx) every pack image the Adam launch keeps
    — the qs_mlp3_pack image of an _M3Work, the qs_mlp3f_pack image of the
    _F16Work, the W2ᵀ copy of the _CriticTiles — equals, byte for byte, a fresh
    image of the current weights."""
    run = dg.fresh(cid, DEV, variant, target_kl=0.0)
    _assert_variant(run)
    before = _state(run)
    for name, live, img in _fresh_images(run):   # as built
        assert _same_bits(live, img), (name, "before the first step")
    for idx in (run.base.idx, run.base.idx2, run.base.idx):
        _step(run, idx)
    assert float(run.agent.actor_opt.step) == 3.0 and float(run.agent.critic_opt.step) == 3.0
    after = _state(run)
    for k in ("actor.flat", "critic.flat", "actor.pack", "critic.pack"):
        assert not torch.equal(before[k], after[k]), k
    for name, live, img in _fresh_images(run):
        assert bool(torch.isfinite(img).all()), name
        assert _same_bits(live, img), name


_GATE_RUNS = [("c3_slice", "fused"), ("c3_slice", "fused_vh"), ("c3_slice", "fused_tiles"), ("c3_slice", "two_kernel"),
              ("spiral_A4", "fold_w1")]


@pytest.mark.parametrize("cid,variant", _GATE_RUNS, ids=[f"{c}-{v}" for c, v in _GATE_RUNS])
def test_gate_closed(cid, variant):
    """Default target_kl and old log-probabilities 0.1 higher (approx_kl about
    0.1 > 1.5·target_kl): no byte of the actor's parameters, moments, step count
    or pack image changes; the critic steps, and its recovered gradients meet
    the bound."""
    run = dg.fresh(cid, DEV, variant, logp_shift=0.1)
    _assert_variant(run)
    assert run.agent.target_kl == 0.01
    before = _state(run)
    acc = _step(run, run.base.idx)
    after = _state(run)
    assert float(run.agent._kl) > 1.5 * run.agent.target_kl and not run.agent._actor_gate_open()
    assert float(run.agent._kl) == pytest.approx(0.1 + dg.reference(run.base)["approx_kl"], abs=1e-5)
    for k in before:
        if k.startswith("actor."):
            assert _same_bits(before[k], after[k]), k
    assert float(run.agent.actor_opt.step) == 0.0 and float(run.agent.critic_opt.step) == 1.0
    assert not torch.equal(before["critic.flat"], after["critic.flat"])
    _check(run, "idx", _recover(run, CRITIC), acc, run.agent._kl, names=CRITIC, losses_too=False)
    ref = dg.reference(run.base)
    assert float(acc[1]) == pytest.approx(ref["value"], rel=1e-6)
    for name, live, img in _fresh_images(run):
        assert _same_bits(live, img), name


_BIT_RUNS = [(cid, v) for cid in ("ragged_185", "rows_4096") for v in ("fused", "two_kernel")]
_BIT_IDS = [f"{c}-{v}" for c, v in _BIT_RUNS]


@pytest.mark.parametrize("cid,variant", _BIT_RUNS, ids=_BIT_IDS)
def test_side_stream_bit_identical_on_clipped_data(cid, variant):
    """side_stream=False equals the default bit for bit on data with clipped
    rows and (ragged_185) action_scale != 1: two eager steps (idx, idx2)."""
    runs = [dg.fresh(cid, DEV, variant, target_kl=0.0, **kw) for kw in ({}, dict(side_stream=False))]
    accs = []
    for run in runs:
        _assert_variant(run)
        accs.append(torch.stack([_step(run, run.base.idx), _step(run, run.base.idx2)]))
    assert runs[0].agent.side_stream and not runs[1].agent.side_stream
    s0, s1 = _state(runs[0]), _state(runs[1])
    for k in s0:
        assert _same_bits(s0[k], s1[k]), k
    assert torch.equal(accs[0], accs[1])
    assert float(runs[0].agent.actor_opt.step) == 2.0


@pytest.mark.parametrize("cid,variant", _BIT_RUNS, ids=_BIT_IDS)
def test_graph_replay_equals_eager_on_clipped_data(cid, variant):
    """A two-epoch agent.update (two minibatches an epoch, captured as one
    graph) with use_graphs=True equals the same call with use_graphs=False bit
    for bit in the parameters, both moments, the pack images and the returned
    statistics."""
    runs, res = [], []
    try:
        for graphs in (False, True):
            run = dg.fresh(cid, DEV, variant, target_kl=0.0, use_graphs=graphs, opt_epochs=2,
                           mini_batch_size=dg.case_of(cid)["mb"])
            runs.append(run)
            gen = torch.Generator(device=DEV)
            gen.manual_seed(5)
            res.append(run.agent.update(run.buf, generator=gen))
            torch.cuda.synchronize()
            _assert_variant(run)
        assert runs[0].agent._graph is None and runs[1].agent._graph is not None
        s0, s1 = _state(runs[0]), _state(runs[1])
        for k in s0:
            assert _same_bits(s0[k], s1[k]), k
        assert float(runs[0].agent.actor_opt.step) == 4.0 and float(runs[0].agent.critic_opt.step) == 4.0
        assert res[0] == res[1]
    finally:
        for run in runs:
            run.agent.release_graphs()


def test_allreduce_form_gradients_match_float64(monkeypatch):
    """The multi-rank form (one rank, nccl, _force_allreduce) on rows_4096:
    what _flush_sums and the two-bucket exchange leave in .grad — read by a
    wrapper around FlatBuffers.adam_multi before the zeroing Adam — meets the
    bound, and is the gradient the moments then hold."""
    import socket
    import torch.distributed as dist
    from gym_pybullet_drones_amd.mappo.agent import FlatBuffers
    own = not dist.is_initialized()
    if own:
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1,
                                device_id=torch.device("cuda", torch.cuda.current_device()))
    run = None
    try:
        run = dg.fresh("rows_4096", DEV, "fused", target_kl=0.0)
        run.agent._force_allreduce = True
        _assert_variant(run)
        snaps = []
        inner = FlatBuffers.adam_multi

        def spy(segs, work, packs=None, zero_grads=False):
            snaps.append(run.agent._reduce_buf.clone())
            assert zero_grads and packs is not None
            return inner(segs, work, packs=packs, zero_grads=zero_grads)

        monkeypatch.setattr(FlatBuffers, "adam_multi", staticmethod(spy))
        acc = _step(run, run.base.idx)
        assert len(snaps) == 1
        snap, a = snaps[0], run.agent
        nc, na = a.critic_opt.n, a.actor_opt.n
        assert snap.numel() == nc + na + 1
        views = {"critic": snap[:nc], "actor": snap[nc:nc + na]}
        grads = {k: dg.flat_view(_fbs(run)[k.split(".")[0]], p, views[k.split(".")[0]]).clone()
                 for k, p in dg.run_params(run).items()}
        _check(run, "idx", grads, acc, snap[nc + na:])
        assert not a._reduce_buf[:nc + na].any()   # zeroed by the Adam launch
        for k, g in _recover(run).items():
            torch.testing.assert_close(g, grads[k].double(), rtol=2e-7, atol=1e-30,
                                       msg=lambda m, k=k: f"{k} from the moments: {m}")
    finally:
        if run is not None:
            run.agent.release_graphs()
        torch.cuda.synchronize()
        if own:
            dist.destroy_process_group()


@pytest.mark.parametrize("cid,hidden", dg.HIDDEN_RUNS, ids=[f"{c}-hidden{h}" for c, h in dg.HIDDEN_RUNS])
def test_fused_iteration_grads_match_float64(cid, hidden):
    """The autograd-driven fused iteration (_iteration_fused: qs_ppo_heads, the
    MLPs under autograd, qs_adam_multi) at hidden widths 64 and 128: the
    gradients read straight from .grad, the losses and approx_kl under the same
    metric and bound.  From 2 048 rows a net runs as _TanhMLP3 on
    qs_mlp_bias_tanh / qs_mlp_tanh_bwd (one_agent_3000: both nets; spiral_A4:
    the actor); below that its layers are plain torch."""
    run = dg.fresh(cid, DEV, "fused", hidden_dim=hidden, setup=False, target_kl=0.0)
    a, b = run.agent, run.base
    assert not a._direct_ok() and not a._small_ok(run.buf, run.mb) and a._fused_heads_ok(run.buf)
    x = torch.empty((2, b.O), device=DEV)
    for net, rows in ((a.ac.actor.pi_net, b.mb * b.D), (a.ac.critic.v_net, b.mb)):
        kernels = net._fused_ok(x.new_empty((rows, net.fcs[0].in_features)))
        assert kernels == (rows >= 2048)
        assert net.fcs[0].out_features == net.fcs[1].out_features == hidden
    start = {k: p.detach().clone() for k, p in dg.run_params(run).items()}
    acc = _step(run, b.idx)
    grads = {k: p.grad.detach().clone() for k, p in dg.run_params(run).items()}
    errs = sg.check_against_float64(f"{cid}-hidden{hidden}", b, "idx", grads, acc, a._kl, dg.GRAD_BOUND)
    print(f"{cid}-hidden{hidden} idx: largest e = {max(errs.values()):.2e}")
    assert float(a.actor_opt.step) == 1.0 and float(a.critic_opt.step) == 1.0
    for k, p in dg.run_params(run).items():
        assert not torch.equal(p, start[k]), k
