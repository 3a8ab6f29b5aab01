"""tests/ohem_ref.py pinned on the CPU, and everything about online hard example mining that needs no GPU:

  * the rule itself on small hand-made inputs: ties at lam_k are all kept, min_kept >= N keeps every candidate (the CE is then the
    plain CE, value and gradient), thresh = 0 with min_kept = 0 keeps nothing (CE = the constant 1.0, no CE gradient), a NaN
    score is kept and stays loud;
  * the yardstick of tests/test_ohem_gpu.py: on the shared case list the fp32 evaluation of the reference against its fp64
    evaluation -- the keep masks (band and cap of ohem_ref.flips) and, with the fp64 mask handed to both, the values: within a
    quarter of the bars on the six patterns of tests/headloss_ref.py (the rule of tests/test_headloss_cpu.py); on `saturated`
    the fp32 evaluation is the yardstick itself, as in tests/test_loss_options_cpu.py (its CE reaches 60: fp32 cannot hold
    an absolute 2e-6 there, measured 6.8e-6 = 1.1e-7 of the value);
  * option validation in Python, LossOptions unchanged, and the argument refusals of the four entry points through ctypes
    (placeholder pointers, no launch).

Run with -s for the measured distances."""
import ctypes
import math

import pytest
import torch

from tests import headloss_ref as R
from tests import loss_options_ref as LR
from tests import ohem_ref as OR
from tests.test_headloss_cpu import HEADROOM


# ------------------------------------------------------------------------------------------------ the rule
def test_select_keeps_ties_and_counts():
    q = torch.tensor([0.5, 0.2, -1.0, 0.2, 0.9, 0.2, 0.7, -1.0])
    lam, n, keep = OR.select(q, 0.0, 2)
    assert n == 6 and float(lam) == float(torch.tensor(0.2)) and keep.tolist() == [False, True, False, True, False, True, False, False]
    assert int(keep.sum()) >= 2, "ties at lam_k are all kept: n_kept >= min(min_kept, N)"
    lam, n, keep = OR.select(q, 0.6, 0)
    assert float(lam) == -1.0 and keep.tolist() == [True, True, False, True, False, True, False, False]
    lam, n, keep = OR.select(q, 0.0, 10 ** 9)
    assert float(lam) == float(torch.tensor(0.9)) and int(keep.sum()) == 6, "the largest score is kept too"
    lam, n, keep = OR.select(torch.full((5,), -1.0), 1.0, 3)
    assert n == 0 and float(lam) == -1.0 and not bool(keep.any())
    qn = torch.tensor([0.5, float("nan"), 0.1, -1.0])
    lam, n, keep = OR.select(qn, 0.0, 1)
    assert n == 3 and float(lam) == float(torch.tensor(0.1)) and keep.tolist() == [False, True, True, False], "NaN sorts last, is kept"
    assert math.isnan(float(OR.select(qn, 0.0, 3)[0]))


def test_scores_are_the_true_class_probability_among_valid_channels():
    z = torch.tensor([[1.0, 2.0, 0.5], [0.0, 0.0, 0.0]]).t().reshape(1, 3, 1, 2).double()
    t = torch.tensor([[0.0, 1.0, -1.0], [-1.0, -1.0, -1.0]]).t().reshape(1, 3, 1, 2).double()
    q = OR.scores(z, t)
    assert abs(float(q[0, 0]) - float(torch.softmax(z[0, :, 0, 0], 0)[1])) < 1e-15 and float(q[0, 1]) == -1.0


@pytest.mark.parametrize("gamma", OR.OHEM_GAMMAS)
def test_min_kept_beyond_the_candidates_is_the_plain_ce(gamma):
    for C, hw, B, pattern in ((5, 257, 3, "random_ignore"), (4, 255, 1, "no_ignore"), (9, 256, 3, "plane_ignored"), (8, 5000, 3, LR.SATURATED)):
        a = OR.run(C, hw, B, pattern, (0.0, 10 ** 9), gamma, torch.float64)
        b = LR.run(C, hw, B, pattern, OR.options(gamma), torch.float64)
        assert bool(a["keep"].reshape(-1).eq((a["q"] != -1).reshape(-1)).all())
        assert R.absdiff(a["ce"], b["ce"]) == 0.0 and R.absdiff(a["dice"], b["dice"]) == 0.0
        assert R.absdiff(a["dz"], b["dz"]) <= 1e-13 * max(1.0, float(b["dz"].abs().max())), "(two graphs: the sums of the terms round apart)"


@pytest.mark.parametrize("gamma", OR.OHEM_GAMMAS)
def test_nothing_kept_is_the_constant_one_without_ce_gradient(gamma):
    for C, hw, B, pattern in ((5, 257, 3, "random_ignore"), (4, 255, 1, "no_ignore"), (16, 256, 3, "item_ignored")):
        a = OR.run(C, hw, B, pattern, (0.0, 0), gamma, torch.float64)
        assert not bool(a["keep"].any()) and float(a["ce"]) == 1.0
        parts = OR.run_parts(C, hw, B, pattern, (0.0, 0), gamma, torch.float64)
        assert float(parts["ce"].abs().max()) == 0.0
        plain = LR.run(C, hw, B, pattern, OR.options(gamma), torch.float64)
        assert R.absdiff(a["dice"], plain["dice"]) == 0.0 and a["nvalid"] == plain["nvalid"]
        assert R.absdiff(a["dz"], parts["dice"]) <= 1e-13 * max(1.0, float(a["dz"].abs().max())), "what is left of dz is the Dice term's"


def test_a_nan_score_is_kept_and_stays_loud():
    x = LR.inputs(5, 257, 3, "random_ignore")
    t = x["t"].clone()
    t[1, :, 0, 100] = torch.tensor([1.0, 0.0, 0.0, -1.0, 0.0])
    for ch in (0, 1, 3):                # a target-1 channel, a target-0 channel, an ignored channel of that pixel
        z = x["z"].double().clone()
        z[1, ch, 0, 100] = float("nan")
        z.requires_grad_(True)
        ce, dice, _, keep, q, lam = OR.ce_dice(z, t, x["w"], OR.options(0.0), 0.0, 1)
        assert math.isnan(float(q[1, 100])) and bool(keep[1, 100])
        assert int(keep.sum()) == int((q == lam).sum()) + 1, "the smallest score with its ties, and the NaN"
        assert math.isnan(float(ce.detach()))
        ce.backward()
        assert bool(torch.isnan(z.grad[1, :, 0, 100]).all())


def test_dice_term_ignores_the_selection():
    for pair in OR.ohem_pairs(257):
        a = OR.run(5, 257, 3, "random_ignore", pair, 2.0, torch.float64)
        b = LR.run(5, 257, 3, "random_ignore", OR.options(2.0), torch.float64)
        assert R.absdiff(a["dice"], b["dice"]) == 0.0 and a["nvalid"] == b["nvalid"]


# ------------------------------------------------------------------------------------------------ fp32 against fp64 on the case list
@pytest.mark.parametrize("C", OR.LOSS_C)
def test_fp32_evaluation_against_fp64_on_the_case_list(C):
    worst, ties = {}, 0
    for case in OR.cases(C):
        ref, own = OR.run(*case, torch.float64), OR.run(*case, torch.float32)
        thresh = case[4][0]
        outside, plain, tie = OR.flips(own["keep"], own["q"], own["lam"], ref["keep"], ref["q"], ref["lam"], thresh)
        assert OR.flips_ok(outside, plain, tie), (case, outside, plain, tie)
        ties = max(ties, tie)
        if case[3] != LR.SATURATED:
            assert outside + plain + tie == 0, (case, "measured: the two evaluations agree at every pixel of these patterns")
        f32 = OR.run(*case, torch.float32, keep=ref["keep"])
        assert f32["nvalid"] == ref["nvalid"], case
        group = worst.setdefault("saturated" if case[3] == LR.SATURATED else "patterns", {})
        for name, bar in OR.LOSS_BARS.items():
            d = R.rel(f32[name], ref[name]) if name == "dz" else R.absdiff(f32[name], ref[name])
            if case[3] == LR.SATURATED:
                assert bool(torch.isfinite(f32[name]).all()), (case, name)
                if name == "ce":
                    d /= max(1.0, abs(float(ref["ce"])))
            assert d <= HEADROOM * bar, (case, name, d, bar)
            group[name] = max(group.get(name, 0.0), d)
    for g, w in worst.items():
        print(f"\nfp32-CPU distance from fp64, OHEM C={C}, {g}: " + ", ".join(f"{k} {v:.2e} (bar {OR.LOSS_BARS[k]:.0e})" for k, v in w.items()))
    print(f"most exact-tie pixels kept by fp32 alone in one case: {ties}")


# ------------------------------------------------------------------------------------------------ Python options
def test_loss_objects_validate_their_ohem_options():
    from hrseg_amd.Metrics import losses as PL
    for bad in (-0.1, 1.5, math.nan, math.inf, -math.inf):
        with pytest.raises(ValueError):
            PL.CrossEntropyLoss(ohem_thresh=bad)
    for bad in (-1, 1.5, math.nan, math.inf, "3", True):
        with pytest.raises(ValueError):
            PL.CrossEntropyLoss(ohem_thresh=0.7, ohem_min_kept=bad)
    assert PL.OhemOptions.from_ce(None) is None and PL.OhemOptions.from_ce(PL.CrossEntropyLoss()) is None
    assert PL.OhemOptions.from_ce(PL.CrossEntropyLoss(ohem_min_kept=5)) is None, "ohem_thresh=None is off whatever min_kept says"
    ce = PL.CrossEntropyLoss(focal_gamma=2.0, ohem_thresh=0.9, ohem_min_kept=100000)
    assert PL.OhemOptions.from_ce(ce) == (0.9, 100000) and ce.last_ohem is None and ce.kept_fraction() is None
    assert PL.OhemOptions.from_ce(PL.CrossEntropyLoss(ohem_thresh=0, ohem_min_kept=3.0)) == (0.0, 3)
    ce.ohem_thresh = 2.0                    # set behind the constructor's back: caught where the options are read
    with pytest.raises(ValueError):
        PL.OhemOptions.from_ce(ce)


def test_loss_options_stays_the_four_field_tuple():
    from hrseg_amd.Metrics import losses as PL
    assert PL.LossOptions._fields == ("gamma", "smooth", "alpha", "beta") and PL.LossOptions() == (0.0, 0.0, 0.5, 0.5)
    ce, dice = PL.CrossEntropyLoss(focal_gamma=2.0, ohem_thresh=0.7, ohem_min_kept=10), PL.SoftDiceLoss(smooth=1, alpha=0.3, beta=0.7)
    assert PL.LossOptions.from_pair(ce, dice) == (2.0, 1.0, 0.3, 0.7)
    assert PL.LossOptions.from_pair(PL.CrossEntropyLoss(ohem_thresh=0.7), PL.SoftDiceLoss()).or_none() is None, \
        "OHEM alone leaves the loss options at their defaults"


# ------------------------------------------------------------------------------------------------ ABI refusals
OHEM_ENTRY_POINTS = ("hrseg_ohem_scores", "hrseg_ohem_select", "hrseg_loss_partials_ohem", "hrseg_loss_bwd_ohem")


def test_ohem_entry_points_refuse_bad_arguments_without_a_gpu():
    """placeholder pointers, never dereferenced: each refusal comes before a launch and names the entry point that was called"""
    from hrseg_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    lib.hrseg_last_error_string.restype = ctypes.c_char_p
    lib.hrseg_ohem_workspace_bytes.restype = ctypes.c_size_t
    for name in OHEM_ENTRY_POINTS:
        getattr(lib, name).argtypes = _lib.PROTOTYPES[name]
    assert lib.hrseg_ohem_workspace_bytes() == _lib.ohem_workspace_bytes() >= (2048 + 2048 + 1024) * 4
    _lib.launch_count("ohem", reset=True)
    P = ctypes.c_void_p(4096)

    def scores(z=P, t=P, q=P, B=2, C=4, hw=100):
        return lib.hrseg_ohem_scores(z, t, q, B, C, hw, None), "hrseg_ohem_scores"

    def select(q=P, n=200, thresh=0.7, min_kept=10, ws=P, rec=P):
        return lib.hrseg_ohem_select(q, n, thresh, min_kept, ws, rec, None), "hrseg_ohem_select"

    def partials(z=P, t=P, q=P, rec=P, thresh=0.7, part=P, B=2, C=4, hw=100, gamma=0.0):
        return lib.hrseg_loss_partials_ohem(z, t, q, rec, thresh, part, B, C, hw, gamma, None), "hrseg_loss_partials_ohem"

    def bwd(z=P, t=P, q=P, rec=P, thresh=0.7, coef=P, g=P, dz=P, B=2, C=4, hw=100, gamma=0.0):
        return lib.hrseg_loss_bwd_ohem(z, t, q, rec, thresh, coef, g, dz, 0, B, C, hw, gamma, None), "hrseg_loss_bwd_ohem"

    def refused(result, text=None):
        rc, name = result
        msg = lib.hrseg_last_error_string().decode()
        return rc == -1 and msg.startswith(name + ": ") and (text is None or text in msg)

    for bad in (-0.01, 1.01, math.nan, math.inf, -math.inf):
        for fn in (select, partials, bwd):
            assert refused(fn(thresh=bad), "thresh"), (fn.__name__, bad)
    assert refused(select(min_kept=-1), "min_kept")
    for bad in (0, -5, 2 ** 31):
        assert refused(select(n=bad), "n="), bad
    for fn in (scores, partials, bwd):
        for bad in (0, 17):
            assert refused(fn(C=bad)), (fn.__name__, bad)
        assert refused(fn(hw=0)) and refused(fn(B=0)), fn.__name__
    for fn, names in ((scores, ("z", "t", "q")), (select, ("q", "ws", "rec")), (partials, ("z", "t", "q", "rec", "part")),
                      (bwd, ("z", "t", "q", "rec", "coef", "g", "dz"))):
        for k in names:
            assert refused(fn(**{k: None})), (fn.__name__, k)
    for fn in (partials, bwd):
        for bad in (-0.5, math.nan):
            assert refused(fn(gamma=bad), "gamma"), (fn.__name__, bad)
    assert refused(select(ws=ctypes.c_void_p(4097)), "aligned")
    assert _lib.launch_count("ohem") == 0, "nothing was launched"
