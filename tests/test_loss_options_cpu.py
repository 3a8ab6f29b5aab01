"""tests/loss_options_ref.py pinned on the CPU, and the option checks of the C ABI, which need no GPU:

  * the fp64 reference reproduces what the reference project's own SoftDiceLoss(smooth=...) produced (tests/golden/loss_smooth.npz),
    and at the default options it is headloss_ref.ce_dice;
  * hrseg_loss_partials_opt / _finalize_opt / _bwd_opt refuse a negative or non-finite option under their own name before
    anything is launched;
  * at the exact inputs of tests/test_loss_options_gpu.py the float32 evaluation of the reference stays within a quarter of the
    bar the GPU test applies (the rule of tests/test_headloss_cpu.py), on every pattern but `saturated`, whose yardstick is
    that fp32 evaluation itself; the saturated inputs do pass the two logit gaps they are there for.

Run with -s to see the measured fp32 distances per group."""
import ctypes
import math

import pytest
import torch

from tests import headloss_ref as R
from tests import loss_options_ref as LR
from tests.helpers import load_golden
from tests.test_headloss_cpu import _headroom


# ------------------------------------------------------------------------------------------------ the reference is right
def test_reference_reproduces_the_smooth_dice_golden():
    g = load_golden("loss_smooth")
    w = [float(v) for v in g["w"]]
    t = torch.from_numpy(g["t"]).double()
    for i, smooth in enumerate(float(v) for v in g["smooth"]):
        z = torch.from_numpy(g["z"]).double().requires_grad_(True)
        _, dice, nvalid = LR.ce_dice(z, t, w, (0.0, smooth, 0.5, 0.5))
        assert nvalid == 3, "with smooth > 0 the fully ignored item counts"
        assert abs(float(dice.detach()) - float(g[f"dice{i}"])) < 1e-6
        dice.backward()
        assert R.rel(z.grad, torch.from_numpy(g[f"dz{i}"])) < 1e-5
    # the same inputs without smoothing: that item is 0/0 and dropped
    assert LR.ce_dice(torch.from_numpy(g["z"]).double(), t, w)[2] == 2


@pytest.mark.parametrize("C", LR.LOSS_C)
def test_reference_at_default_options_is_headloss_ref(C):
    for hw in (1, 257):
        for B in LR.LOSS_B:
            for pattern in LR.LOSS_PATTERNS:
                a, b = LR.run(C, hw, B, pattern, LR.DEFAULTS, torch.float64), R.loss_run(C, hw, B, pattern, torch.float64)
                assert a["nvalid"] == b["nvalid"]
                assert R.absdiff(a["ce"], b["ce"]) < 1e-13 and R.absdiff(a["dice"], b["dice"]) < 1e-13
                assert R.absdiff(a["dz"], b["dz"]) <= 1e-13 * max(1.0, float(b["dz"].abs().max()))


def test_one_minus_p_is_stable_where_the_subtraction_is_not():
    z = torch.tensor([[30.0, 0.0, -5.0], [120.0, 0.0, 1.0], [0.0, 0.0, 0.0]]).t().reshape(1, 3, 3)     # pixels along the last axis
    om32, om64 = LR.one_minus_p(z), LR.one_minus_p(z.double())
    assert float((1.0 - torch.softmax(z, 1))[0, 0, 0]) == 0.0          # the naive form at a gap of 30
    assert float(om32[0, 0, 0]) > 0 and R.rel(om32, om64) < 1e-6
    assert torch.equal(LR.one_minus_p(torch.zeros(2, 1, 5)), torch.zeros(2, 1, 5))       # C = 1: no other channel


# ------------------------------------------------------------------------------------------------ ABI refusals
def _lib():
    from hrseg_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    lib.hrseg_last_error_string.restype = ctypes.c_char_p
    for name in ("hrseg_loss_partials_opt", "hrseg_loss_finalize_opt", "hrseg_loss_bwd_opt"):
        getattr(lib, name).argtypes = _lib.PROTOTYPES[name]
    return lib


def test_bad_loss_options_are_refused_without_a_gpu():
    """placeholder pointers, never dereferenced: each refusal comes before a launch and names the entry point that was called"""
    lib = _lib()
    P = ctypes.c_void_p(4096)

    def partials(gamma):
        return lib.hrseg_loss_partials_opt(P, P, P, 2, 4, 100, gamma, None)

    def finalize(smooth=0.0, alpha=0.5, beta=0.5):
        return lib.hrseg_loss_finalize_opt(P, P, 2, 4, smooth, alpha, beta, P, P, None)

    def bwd(gamma):
        return lib.hrseg_loss_bwd_opt(P, P, P, P, P, 0, 2, 4, 100, gamma, None)

    def refused(rc, name):
        msg = lib.hrseg_last_error_string().decode()
        return rc == -1 and msg.startswith(name + ": ")

    for bad in (-0.5, math.nan, math.inf):
        assert refused(partials(bad), "hrseg_loss_partials_opt"), bad
        assert refused(bwd(bad), "hrseg_loss_bwd_opt"), bad
        assert refused(finalize(smooth=bad), "hrseg_loss_finalize_opt"), bad
        assert refused(finalize(alpha=bad), "hrseg_loss_finalize_opt"), bad
        assert refused(finalize(beta=bad), "hrseg_loss_finalize_opt"), bad
    assert b"gamma" in lib.hrseg_last_error_string() or b"smooth" in lib.hrseg_last_error_string()
    # sizes are still checked, under the name that was called
    assert lib.hrseg_loss_partials_opt(P, P, P, 2, 17, 100, 0.0, None) == -1
    assert lib.hrseg_last_error_string().decode().startswith("hrseg_loss_partials_opt: bad arguments")
    assert lib.hrseg_loss_bwd_opt(P, P, P, P, None, 0, 2, 4, 100, 0.0, None) == -1
    assert lib.hrseg_last_error_string().decode().startswith("hrseg_loss_bwd_opt: bad arguments")
    assert lib.hrseg_loss_finalize_opt(P, None, 2, 4, 0.0, 0.5, 0.5, P, P, None) == -1
    assert lib.hrseg_last_error_string().decode().startswith("hrseg_loss_finalize_opt: bad arguments")


def test_loss_objects_validate_their_options():
    from hrseg_amd.Metrics import losses as PL
    for bad in (-1.0, math.nan, math.inf):
        with pytest.raises(ValueError):
            PL.CrossEntropyLoss(focal_gamma=bad)
        for key in ("smooth", "alpha", "beta"):
            with pytest.raises(ValueError):
                PL.SoftDiceLoss(**{key: bad})
    ce, dice = PL.CrossEntropyLoss(smooth=0.3, focal_gamma=2.0), PL.SoftDiceLoss(smooth=1, alpha=0.3, beta=0.7)
    assert PL.LossOptions.from_pair(ce, dice) == (2.0, 1.0, 0.3, 0.7)
    assert PL.LossOptions.from_pair(ce, None) == (2.0, 0.0, 0.5, 0.5), "CrossEntropyLoss.smooth is not an option of the kernels"
    assert PL.LossOptions.from_pair(None, dice) == (0.0, 1.0, 0.3, 0.7)
    assert PL.LossOptions.from_pair(PL.CrossEntropyLoss(), PL.SoftDiceLoss()).or_none() is None
    assert PL.LossOptions.from_pair(ce, dice).or_none() == (2.0, 1.0, 0.3, 0.7)


# ------------------------------------------------------------------------------------------------ fp32 headroom of the bars
@pytest.mark.parametrize("C", LR.LOSS_C)
def test_headroom_loss_options(C):
    cases = [(C, hw, B, pat, opt) for hw in LR.LOSS_HW for B in LR.LOSS_B for pat in LR.LOSS_PATTERNS for opt in LR.OPTION_SETS]
    _headroom(f"loss C={C}", cases, LR.run, LR.LOSS_BARS, absolute=("ce", "dice"))
    for case in cases:
        assert LR.run(*case, torch.float32)["nvalid"] == LR.run(*case, torch.float64)["nvalid"]


def test_saturated_inputs_pass_both_gaps_and_stay_finite_in_fp32():
    worst = 0.0
    for C in LR.LOSS_C:
        for hw in LR.LOSS_HW:
            for B in LR.LOSS_B:
                x = LR.inputs(C, hw, B, LR.SATURATED)
                assert torch.equal(x["t"], R.loss_inputs(C, hw, B, "random_ignore")["t"])
                if C >= 4 and hw >= 255:
                    gaps = LR.max_gaps(x["z"])
                    mid = ((gaps > LR.GAP_EPS) & (gaps < LR.GAP_UNDERFLOW)).float().mean()
                    assert float(mid) > 0.05 and float((gaps > LR.GAP_UNDERFLOW).float().mean()) > 0.05, (C, hw, B)
                    assert 0.2 < float((gaps > LR.GAP_EPS).float().mean()) < 0.4
                for opt in LR.OPTION_SETS:
                    a, b = LR.run(C, hw, B, LR.SATURATED, opt, torch.float32), LR.run(C, hw, B, LR.SATURATED, opt, torch.float64)
                    for k in ("ce", "dice", "dz"):
                        assert bool(torch.isfinite(a[k]).all()) and bool(torch.isfinite(b[k]).all()), (C, hw, B, opt, k)
                    assert a["nvalid"] == b["nvalid"]
                    worst = max(worst, R.rel(a["dz"], b["dz"]))
    print(f"\nsaturated: worst fp32-CPU dz distance from fp64 {worst:.2e} (BAR_REDUCED {LR.BAR_REDUCED:.0e})")
