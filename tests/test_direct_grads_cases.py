"""The cases of tests/direct_grads_case.py, checked without a GPU: each entry
reaches the host-side choices it claims (the workspace objects' chunk counts
and partial rows are host code), its data exercises both clip branches of the
loss heads away from the bounds, the error metric of
tests/test_gpu_direct_grads.py applied to torch's own float32 autograd stays
where that test's bound was derived from, and the metric sees the faults the
GPU test exists for at ten times its bound or more."""
import os
import re

import pytest
import torch

import direct_grads_case as dg

ALL = range(len(dg.CASES))
# (case, hidden width) of every reference the GPU file uses: the direct cases and the hidden-64 / -128 runs
REFS = [(cid, 256) for cid in dg.CASE_IDS] + dg.HIDDEN_RUNS
REF_IDS = [cid if h == 256 else f"{cid}-hidden{h}" for cid, h in REFS]


def _workspaces(c, fold=False):
    """The direct iteration's workspaces for the case on the CPU (allocation and
    host calls only; _direct_setup itself packs on the GPU): the fused actor's,
    the two-kernel actor's, the _M3Work critic's."""
    from gym_pybullet_drones_amd.mappo import agent as ag
    agent = dg.base(c["id"], "cpu").agent
    pa, pc = agent.ac.actor.pi_net, agent.ac.critic.v_net
    K = c["mb"] * c["D"]
    assert agent._direct_ok() and ag._f16_ok(pa) and ag._m3_shape_ok(K, c["O"])
    assert not ag._SPLITK_MIN_ROWS   # the chunk sizes below are the defaults'
    assert (pa.fcs[0].in_features, pc.fcs[0].in_features, pa.fcs[2].out_features) == (c["O"], c["D"] * c["O"], c["A"])
    with dg.folded(fold):
        f16 = ag._F16Work(pa, K, "cpu")
    return f16, ag._M3Work(pa, K, "cpu"), ag._M3Work(pc, c["mb"], "cpu")


def _tall_threshold():
    """QS_SUM_TALL_G of csrc/learner.hip: partial rows from which a sum task
    takes mlp_sum_cols = 1 (the tall instance of the sum launch)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "marl-gym-pybullet-drones_amd", "csrc", "learner.hip")).read()
    return int(re.search(r"#define QS_SUM_TALL_G (\d+)", src).group(1))


@pytest.mark.parametrize("i", ALL, ids=dg.CASE_IDS)
def test_case_reaches_what_it_claims(i):
    from gym_pybullet_drones_amd import _lib as L
    from gym_pybullet_drones_amd.mappo.agent import _SMALL_MAX_IN, _splitk_chunks
    c = dg.CASES[i]
    K, mb, lib = c["mb"] * c["D"], c["mb"], L.load()
    f16, m3, cr = _workspaces(c)
    assert (f16.S1, f16.S2) == c["f16_chunks"] and (m3.S1, m3.S2) == c["m3_chunks"]
    assert (cr.S1, cr.S2) == c["critic_chunks"]
    assert (f16.C1, f16.C2, m3.C1, m3.C2, cr.C1, cr.C2) == (0,) * 6   # split-K GEMMs, not qs_mlp_wgrad
    assert (f16.S1, f16.S2) == (_splitk_chunks(K, 1024), _splitk_chunks(K, 2048))
    for ws in (f16, m3, cr):   # a `whole` task exactly where there are no chunk partials
        assert (ws.pw1 is None) == (ws.S1 == 1) and (ws.pw2 is None) == (ws.S2 == 1)
        assert ws.K % ws.S1 == 0 and ws.K % ws.S2 == 0
    assert f16.G == lib.qs_mlp3f_tiles(K) == c["f16_tiles"] == (K + 127) // 128
    assert m3.G == lib.qs_mlp3_tiles(K, c["O"]) == c["m3_tiles"]
    assert cr.G == lib.qs_mlp3_tiles(mb, c["D"] * c["O"]) == c["critic_tiles"] == (mb + 31) // 32
    assert m3.G == ((K + 127) // 128 if c["id"] == "rows_16384" else (K + 31) // 32)
    assert c["D"] * c["O"] <= _SMALL_MAX_IN


def test_cases_cover_the_direct_path():
    C = {c["id"]: c for c in dg.CASES}
    K = lambda c: c["mb"] * c["D"]
    assert {c["A"] for c in dg.CASES} == {1, 2, 3, 4}
    assert any(c["scale"] != 1.0 for c in dg.CASES) and any(c["O"] % 4 and (c["D"] * c["O"]) % 4 for c in dg.CASES)
    assert any(c["D"] == 1 for c in dg.CASES)
    # a partial 16-row tile, a partial 128-row workgroup, a partial 32-row block, an odd row count
    r = C["ragged_185"]
    assert K(r) % 16 and K(r) % 128 and r["mb"] % 32 and r["mb"] % 2 and K(r) > 128 and r["mb"] > 32
    assert (K(C["three_rows"]), C["three_rows"]["mb"]) == (3, 1)
    # every weight gradient whole; chunked beside whole; both chunked with different counts; the critic's chunked
    assert C["c3_slice"]["f16_chunks"] == C["c3_slice"]["m3_chunks"] == C["c3_slice"]["critic_chunks"] == (1, 1)
    assert C["spiral_A4"]["f16_chunks"][0] > 1 and C["spiral_A4"]["f16_chunks"][1] == 1
    s1, s2 = C["rows_4096"]["f16_chunks"]
    assert s1 > 1 and s2 > 1 and s1 != s2
    assert C["one_agent_3000"]["m3_chunks"] == C["one_agent_3000"]["critic_chunks"] == (2, 2)
    assert min(C["rows_16384"]["critic_chunks"]) > 1
    # qs_mlp3_tiles' 128-row blocks against 32-row blocks at the same row count; the tall sum task
    assert C["rows_16384"]["m3_tiles"] * 128 == K(C["rows_16384"]) == C["rows_16384_in72"]["m3_tiles"] * 32
    tall = _tall_threshold()
    assert C["rows_16384_in72"]["m3_tiles"] >= tall
    assert all(max(c["f16_tiles"], c["m3_tiles"], c["critic_tiles"]) < tall for c in dg.CASES
               if c["id"] != "rows_16384_in72")
    # the critic tiles only where D·O <= 256 (_direct_setup's condition)
    assert all(C[cid]["D"] * C[cid]["O"] <= 256 for cid, v in dg.RUNS if v == "fused_tiles")
    runs = set(dg.RUNS)
    assert all((c["id"], v) in runs for c in dg.CASES for v in ("fused", "two_kernel"))
    assert {v for _, v in runs} == set(dg.VARIANTS)


@pytest.mark.parametrize("cid", [cid for cid, v in dg.RUNS if v == "fused_tiles"])
def test_critic_tiles_layout(cid):
    """_CriticTiles' chunking of the case's critic: S whole chunks of whole
    16-row tiles, the row stride no shorter than the padded rows."""
    from gym_pybullet_drones_amd.mappo.agent import _CriticTiles
    c = dg.case_of(cid)
    ct = _CriticTiles(dg.base(cid, "cpu").agent, c["mb"], c["D"])
    assert ct.nC == (c["mb"] + 15) // 16 and ct.nC % ct.S == 0 and ct.KcP % (16 * ct.S) == 0
    assert c["mb"] <= ct.KcP <= ct.ld and ct.ld % 4 == 0
    assert torch.equal(ct.w2t, ct.mlp.fcs[1].weight.t())


def test_fold_w1_workspace():
    """fold_w1 (patched on the class) gives the folded partials in place of dW1's chunks."""
    for cid, v in dg.RUNS:
        if v == "fold_w1":
            c = dg.case_of(cid)
            f16, _, _ = _workspaces(c, fold=True)
            assert f16.pw1f is not None and f16.pw1 is None and tuple(f16.pw1f.shape) == (c["f16_tiles"], 256, c["O"])
    from gym_pybullet_drones_amd.mappo.agent import _F16Work
    assert _F16Work.fold_w1 is False   # restored


def _gap(r):
    return torch.minimum((r - (1 - dg.CLIP)).abs(), (r - (1 + dg.CLIP)).abs()).min().item()


@pytest.mark.parametrize("cid,hidden", REFS, ids=REF_IDS)
def test_case_data_exercises_both_clip_branches(cid, hidden):
    """Every ratio at least 5e-3 from both bounds on both draws, rows in every
    branch of the heads, idx no contiguous range."""
    case = dg.base(cid, "cpu", hidden)
    for which in ("idx", "idx2"):
        r = dg.reference(case, which)["ratio"]
        assert r.numel() == case.mb * case.D
        assert _gap(r) >= 5e-3, (which, _gap(r))
    assert not torch.equal(case.idx, case.idx2)
    assert int((case.idx[1:] - case.idx[:-1] != 1).sum()) > 0 or case.mb == 1
    ref = dg.reference(case)
    inside, zero, live = (g.double().mean().item() for g in dg.row_groups(ref))
    n = ref["ratio"].numel()
    if n >= 64:
        assert inside >= 0.10 and zero >= 0.10 and live >= 0.05, (inside, zero, live)
    else:
        assert inside * n >= 1 and zero * n >= 1, (inside, zero, live)   # one inside, one outside


@pytest.mark.parametrize("cid,hidden", REFS, ids=REF_IDS)
def test_metric_on_float32_autograd(cid, hidden):
    """The GPU test's metric on torch's float32 autograd: at most 2.5e-6 on
    both draws, as in the tile suite (the seed rule keeps it within 1.5e-6)."""
    case = dg.base(cid, "cpu", hidden)
    for which in ("idx", "idx2"):
        e = dg.fp32_autograd_errors(case, which)
        print(cid, hidden, which, {k: f"{v:.2e}" for k, v in e.items()})
        assert max(e.values()) <= 2.5e-6, e


@pytest.mark.parametrize("cid,hidden", REFS, ids=REF_IDS)
def test_metric_sees_the_faults(cid, hidden):
    """On the float64 reference, each of these faults moves the tensors it
    touches by at least 10 x the GPU bound under the GPU test's metric:
    * the minibatch's last env-timestep dropped (its rows' terms missing from
      sums still divided by the full row counts): all 13 tensors;
    * the policy loss without the clamp: the 7 actor tensors;
    * the backward's action_scale factor dropped (the actor's MLP gradients
      divided by it): the actor's 6 MLP tensors, where scale != 1."""
    c = dg.case_of(cid)
    case = dg.base(cid, "cpu", hidden)
    ref = dg.reference(case)["grads"]
    need = 10 * dg.GRAD_BOUND
    mb = case.mb
    if mb > 1:   # the gradients of the mb − 1 others, rescaled to the full minibatch's normaliser
        short = dg.losses(case, case.idx[:-1], torch.float64)["grads"]
        dropped = {k: short[k] * ((mb - 1) / mb) for k in dg.NAMES}
    else:
        dropped = {k: torch.zeros_like(ref[k]) for k in dg.NAMES}
    e_drop = {k: dg.rel_err(dropped[k], ref[k]) for k in dg.NAMES}
    noclamp = dg.losses(case, case.idx, torch.float64, clamp=False)["grads"]
    e_clamp = {k: dg.rel_err(noclamp[k], ref[k]) for k in dg.NAMES if k.startswith("actor.")}
    print(cid, hidden, "dropped env-timestep: min e", f"{min(e_drop.values()):.2e}", "no clamp: min e",
          f"{min(e_clamp.values()):.2e}")
    assert min(e_drop.values()) >= need, e_drop
    assert min(e_clamp.values()) >= need, e_clamp
    if c["scale"] != 1.0:
        e_scale = {k: dg.rel_err(ref[k] / c["scale"], ref[k]) for k in dg.NAMES
                   if k.startswith("actor.") and k != "actor.logstd"}
        assert min(e_scale.values()) >= need, e_scale
