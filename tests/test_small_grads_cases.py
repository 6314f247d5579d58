"""The cases of tests/small_grads_case.py, checked without a GPU: each entry
hits the tile layout it claims (qs_ppo_small_layout is host code), its data
exercises both clip branches of the PPO head away from the bounds, and the
error metric of tests/test_gpu_small_grads.py, applied to torch's own float32
autograd, stays where that test's bound was derived from."""
import ctypes

import pytest
import torch

import small_grads_case as sg

MAX_CPU_ROWS = 4096   # actor rows up to which the float64 reference is formed here


def _layout(c):
    from gym_pybullet_drones_amd import _lib as L
    off = (ctypes.c_int64 * L.QS_PPO_SMALL_LAYOUT_N)()
    assert L.load().qs_ppo_small_layout(c["mb"], c["D"], c["O"], c["D"] * c["O"], c["A"], off, len(off)) == 0
    nA, nC, KaP, KcP = off[16], off[17], off[18], off[19]
    assert KaP % (16 * nA) == 0 and KcP % (16 * nC) == 0
    return dict(rb=KaP // (16 * nA), rbc=KcP // (16 * nC), Sa=off[27], Sc=off[28])


@pytest.mark.parametrize("i", range(len(sg.CASES)), ids=sg.CASE_IDS)
def test_case_hits_its_claimed_layout(i):
    c = sg.CASES[i]
    lay = _layout(c)
    assert (lay["rb"], lay["rbc"]) == (c["rb"], c["rbc"]), lay
    assert (lay["Sa"] > 1, lay["Sc"] > 1) == (c["sa_chunks"], c["sc_chunks"]), lay
    assert (c["D"] * c["O"] > 256 or c["O"] > 256) == c["wide"]
    assert c["mb"] * c["D"] <= 16384   # QS_PPO_SMALL_MAX_ROWS


def test_cases_cover_every_instance_family():
    """s_launch_fb's instances: the actor's row blocks 1 / 2 / 3 with the
    critic's 1 / 2 / 3, the narrow and the wide tile, 1-4 actor outputs (the
    wider heads at 16 and at 32 rows), layer 1 with and without the padded W1
    copies; the weight gradients in one chunk (two launches) and in K-chunks."""
    C = sg.CASES
    fam = {(c["rb"], c["rbc"], c["wide"]) for c in C}
    assert {(1, 1, False), (1, 1, True), (2, 1, False), (2, 1, True), (2, 2, False), (2, 2, True), (3, 1, False),
            (3, 1, True), (3, 3, False)} <= fam
    assert {c["A"] for c in C} == {1, 2, 3, 4}
    assert {c["A"] for c in C if c["rb"] == 1 and c["A"] > 1} == {2, 3, 4}
    assert any(c["A"] > 1 and c["rb"] == 2 for c in C)
    assert {(c["rb"], c["rbc"]) for c in C if not c["w1p"]} == {(1, 1), (2, 1), (2, 2)}
    assert any(c["scale"] != 1.0 for c in C) and any(c["O"] % 4 for c in C)
    assert {(c["sa_chunks"], c["sc_chunks"]) for c in C} == {(False, False), (True, False), (True, True)}


_small = [i for i, c in enumerate(sg.CASES) if c["mb"] * c["D"] <= MAX_CPU_ROWS and c["w1p"]]


@pytest.mark.parametrize("i", _small, ids=[sg.CASE_IDS[i] for i in _small])
def test_case_data_exercises_both_clip_branches(i):
    """Every ratio at least 5e-3 from both bounds (the guard yields >= 1e-2
    before logp_old is rounded; float32 log-probabilities move a ratio by about
    1e-5), and rows in every branch of the head."""
    case = sg.get_case(i, "cpu")
    for which in ("idx", "idx2"):
        ref = sg.reference(case, which)
        r = ref["ratio"]
        assert r.numel() == case.mb * case.D
        gap = torch.minimum((r - (1 - sg.CLIP)).abs(), (r - (1 + sg.CLIP)).abs()).min().item()
        assert gap >= 5e-3, gap
    assert not torch.equal(case.idx, case.idx2)
    assert int((case.idx[1:] - case.idx[:-1] != 1).sum()) > 0 or case.mb == 1   # not a contiguous range
    ref = sg.reference(case)
    inside, zero, live = (g.double().mean().item() for g in sg.row_groups(ref))
    n = ref["ratio"].numel()
    if n >= 64:
        assert inside >= 0.10 and zero >= 0.10 and live >= 0.05, (inside, zero, live)
    else:
        assert inside * n >= 1 and zero * n >= 1, (inside, zero, live)


def test_guard_moves_rows_off_the_clip_bounds():
    """Why the guard exists: the 4 096-row case's plain draw (logp_old before
    the guard) has 192 rows within 1e-2 of a bound and one 6.4e-5 from it —
    float32 and float64 may put such a row on different branches; with the
    guard the nearest row is 1e-2 away."""
    i = sg.CASE_IDS.index("rows_4096")
    case = sg.get_case(i, "cpu")
    gap = lambda r: torch.minimum((r - (1 - sg.CLIP)).abs(), (r - (1 + sg.CLIP)).abs()).min().item()
    plain = sg.losses(case, case.idx, torch.float64, logp_old=case.logp_old_unguarded)["ratio"]
    assert gap(plain) < 1e-4 < 5e-3 <= gap(sg.reference(case)["ratio"])


@pytest.mark.parametrize("i", _small, ids=[sg.CASE_IDS[i] for i in _small])
def test_metric_on_float32_autograd(i):
    """The GPU test's metric (max|g − g64| / max|g64| per tensor) on torch's
    float32 autograd: at most 2.5e-6 on the six smallest cases and the others
    up to 4 096 rows, on both idx draws (measured: at most 1.5e-6).  The GPU
    test's bound, 2e-5, is 16 times the figure these shapes were first
    measured at (1.2e-6)."""
    case = sg.get_case(i, "cpu")
    for which in ("idx", "idx2"):
        e = sg.fp32_autograd_errors(case, which)
        print(sg.CASE_IDS[i], which, {k: f"{v:.2e}" for k, v in e.items()})
        assert max(e.values()) <= 2.5e-6, e
