"""The loss kernels of csrc/loss.hip with their options -- focal exponent on the CE, smoothing and Tversky weights in the Dice
term (hrseg_loss_partials_opt / _finalize_opt / _bwd_opt) -- against the fp64 reference of tests/loss_options_ref.py on the case
grid of tests/headloss_ref.py (every CT instance edge, every block edge, every ignore pattern) times five option sets, at the
bars of tests/test_headloss_gpu.py; the defaults through the _opt entry points against the entry points without options, bit
for bit; the reference project's own SoftDiceLoss(smooth=...) values; saturated logits, where 1 - p is 0 as a subtraction;
and a NaN logit, which stays loud.  tests/test_loss_options_cpu.py pins the reference and the room fp32 has at these inputs.
Run with -s for the worst distances and the saturated-case ratios."""
import pytest
import torch

from tests import headloss_ref as R
from tests import loss_options_ref as LR
from tests.helpers import load_golden

pytestmark = pytest.mark.gpu

WORST = {}
RATIOS = {}


@pytest.fixture(scope="module")
def ops():
    from hrseg_amd import ops as o
    assert torch.cuda.is_available()
    yield o
    for group, d in WORST.items():
        print(f"\nworst vs fp64, {group}: " + ", ".join(f"{k} {v[0]:.2e} (bar {v[1]:.0e})" for k, v in d.items()))
    for opt, (kernel, cpu32) in RATIOS.items():
        print(f"saturated dz, options {opt}: kernel {kernel:.2e}, fp32 CPU reference {cpu32:.2e} of max |dz| from fp64: "
              f"ratio {kernel / max(cpu32, 1e-30):.2f} (allowed {LR.SATURATED_SLACK:.0f}, never under the bar {LR.BAR_REDUCED:.0e})")


@pytest.fixture
def deterministic():
    from hrseg_amd import _lib
    _lib.set_deterministic(True)
    yield
    _lib.set_deterministic(False)


def reference(C, hw, B, pattern, options, dtype=torch.float64):
    """(every case is needed by one test only: nothing to share or cache)"""
    return LR.run(C, hw, B, pattern, options, dtype)


def check(group, name, got, ref, bar, absolute=False):
    d = R.absdiff(got, ref) if absolute else R.rel(got, ref)
    w = WORST.setdefault(group, {})
    w[name] = (max(w.get(name, (0.0, bar))[0], d), bar)
    assert d < bar, (group, name, d, bar)


def device_case(C, hw, B, pattern):
    x = LR.inputs(C, hw, B, pattern)
    return x["z"].cuda(), x["t"].cuda(), torch.tensor(x["w"]).cuda(), torch.tensor(LR.LOSS_UPSTREAM).cuda()


@pytest.mark.parametrize("C", LR.LOSS_C)
def test_loss_options_fwd_bwd(ops, C):
    for hw in LR.LOSS_HW:
        for B in LR.LOSS_B:
            for pattern in LR.LOSS_PATTERNS:
                z, t, w, up = device_case(C, hw, B, pattern)
                for opt in LR.OPTION_SETS:
                    ref = reference(C, hw, B, pattern, opt)
                    out, coef = ops.loss_fwd(z, t, w, opt)
                    out = out.cpu()
                    check("loss options", "ce", out[0], ref["ce"], LR.LOSS_BARS["ce"], absolute=True)
                    check("loss options", "dice", out[1], ref["dice"], LR.LOSS_BARS["dice"], absolute=True)
                    assert float(out[2]) == ref["nvalid"], (C, hw, B, pattern, opt)
                    dz = ops.loss_bwd(z, t, coef, up, options=opt)
                    check("loss options", "dz", dz, ref["dz"], LR.LOSS_BARS["dz"])
                    # accumulated onto a buffer of the gradient's own magnitude, as tests/test_headloss_gpu.py does (on an O(1)
                    # buffer the fp32 rounding of the sum alone would hide the kernel's error)
                    scale = float(ref["dz"].abs().max()) or 1.0
                    base = scale * torch.randn(z.shape, generator=torch.Generator().manual_seed(3))
                    acc = ops.loss_bwd(z, t, coef, up, dz=base.cuda(), accumulate=True, options=opt)
                    check("loss options", "dz", acc.cpu().double() - base.double(), ref["dz"], LR.LOSS_BARS["dz"])


@pytest.mark.parametrize("C", LR.LOSS_C)
def test_defaults_through_the_opt_entry_points_keep_the_bits(ops, deterministic, C):
    """(deterministic mode: one adder per image, so that two runs of ONE entry point agree bit for bit to begin with)"""
    for hw in (257, 5000):
        for pattern in LR.LOSS_PATTERNS:
            z, t, w, up = device_case(C, hw, 3, pattern)
            out0, coef0 = ops.loss_fwd(z, t, w)
            out1, coef1 = ops.loss_fwd(z, t, w, LR.DEFAULTS)
            assert torch.equal(out0, out1) and torch.equal(coef0, coef1), (C, hw, pattern)
            assert torch.equal(ops.loss_bwd(z, t, coef0, up), ops.loss_bwd(z, t, coef1, up, options=LR.DEFAULTS))


def test_soft_dice_smooth_reproduces_the_reference_project(ops):
    """SoftDiceLoss(smooth=s) against the values the reference project's own class produced on the same inputs, one item of which
    is fully ignored: with smooth > 0 it counts (tests/golden/loss_smooth.npz)"""
    from hrseg_amd.Metrics import losses as PL
    g = load_golden("loss_smooth")
    w = [float(v) for v in g["w"]]
    t = torch.from_numpy(g["t"]).cuda()
    for i, smooth in enumerate(float(v) for v in g["smooth"]):
        z = torch.from_numpy(g["z"]).cuda().requires_grad_(True)
        dice = PL.SoftDiceLoss(smooth=smooth)(z, t, logits_input=True, class_weight=w)
        dice.backward()
        assert abs(float(dice.detach()) - float(g[f"dice{i}"])) < R.BAR_LOSS
        assert R.rel(z.grad, torch.from_numpy(g[f"dz{i}"])) < R.BAR_REDUCED
        assert float(ops.loss_fwd(z.detach(), t, torch.tensor(w).cuda(), (0.0, smooth, 0.5, 0.5))[0][2]) == 3.0
    assert float(ops.loss_fwd(torch.from_numpy(g["z"]).cuda(), t, torch.tensor(w).cuda())[0][2]) == 2.0


@pytest.mark.parametrize("C", LR.LOSS_C)
def test_saturated_logits(ops, C):
    """logit gaps beyond 17 (1 - p below fp32 epsilon) and beyond 104 (the other exponentials underflow): everything finite, CE
    relative to max(1, |ref|), dz at most SATURATED_SLACK times as far from fp64 as the fp32 CPU evaluation of the stable
    formula on the same case (a different summation order, other expf / logf), never asked to be closer than BAR_REDUCED"""
    for hw in LR.LOSS_HW:
        for B in LR.LOSS_B:
            z, t, w, up = device_case(C, hw, B, LR.SATURATED)
            for opt in LR.OPTION_SETS:
                ref, cpu32 = reference(C, hw, B, LR.SATURATED, opt), reference(C, hw, B, LR.SATURATED, opt, torch.float32)
                out, coef = ops.loss_fwd(z, t, w, opt)
                dz = ops.loss_bwd(z, t, coef, up, options=opt)
                out = out.cpu()
                assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(dz).all()), (C, hw, B, opt)
                d = R.absdiff(out[0], ref["ce"]) / max(1.0, abs(float(ref["ce"])))
                assert d < LR.BAR_LOSS, (C, hw, B, opt, "ce", d)
                check("saturated", "dice", out[1], ref["dice"], LR.LOSS_BARS["dice"], absolute=True)
                assert float(out[2]) == ref["nvalid"], (C, hw, B, opt)
                yard = R.rel(cpu32["dz"], ref["dz"])
                got = R.rel(dz, ref["dz"])
                bar = max(LR.SATURATED_SLACK * yard, LR.BAR_REDUCED)
                worst = RATIOS.get(opt)
                if worst is None or got / max(yard, 1e-30) > worst[0] / max(worst[1], 1e-30):
                    RATIOS[opt] = (got, yard)
                assert got <= bar, (C, hw, B, opt, "dz", got, yard, bar)


@pytest.mark.parametrize("opt", [(2.0, 0.0, 0.5, 0.5), (2.0, 1.0, 0.3, 0.7)])
def test_a_nan_logit_stays_loud_under_the_focal_ce(ops, opt):
    z, t, w, up = device_case(5, 257, 3, "random_ignore")
    t[1, :, 0, 100] = torch.tensor([1.0, 0.0, 0.0, -1.0, 0.0]).cuda()
    for ch in (0, 1, 3):                # a target-1 channel, a target-0 channel, an ignored channel of that pixel
        zn = z.clone()
        zn[1, ch, 0, 100] = float("nan")
        out, coef = ops.loss_fwd(zn, t, w, opt)
        assert bool(torch.isnan(out[0])), (ch, out)
        dz = ops.loss_bwd(zn, t, coef, up, options=opt)
        assert bool(torch.isnan(dz[1, :, 0, 100]).all()), ch
