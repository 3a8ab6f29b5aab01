"""The per-pixel-weight instances of the loss kernels (hrseg_loss_partials_pw / hrseg_loss_bwd_pw, csrc/loss.hip) against the
fp64 reference of tests/border_ref.py on the grid of tests/test_border_cpu.py's room check, at the bars of
tests/test_loss_options_gpu.py; maps of ones and of twos against the entry points without weights, bit for bit; a class mask of
weighted mass 0; a NaN logit, which stays loud whatever its weight; and the plumbing up to CrossEntropyLoss(border=) through
get_loss.  Run with -s for the worst distances."""
import pytest
import torch

from tests import border_ref as BR
from tests import headloss_ref as R
from tests import loss_options_ref as LR

pytestmark = pytest.mark.gpu

WORST = {}


@pytest.fixture(scope="module")
def ops():
    from hrseg_amd import ops as o
    assert torch.cuda.is_available()
    yield o
    for group, d in WORST.items():
        print(f"\nworst vs fp64, {group}: " + ", ".join(f"{k} {v[0]:.2e} (bar {v[1]:.0e})" for k, v in d.items()))


@pytest.fixture
def deterministic():
    from hrseg_amd import _lib
    _lib.set_deterministic(True)
    yield
    _lib.set_deterministic(False)


def check(group, name, got, ref, bar, absolute=False):
    d = R.absdiff(got, ref) if absolute else R.rel(got, ref)
    w = WORST.setdefault(group, {})
    w[name] = (max(w.get(name, (0.0, bar))[0], d), bar)
    assert d < bar, (group, name, d, bar)


def device_case(C, hw, B, pattern, kind):
    x = LR.inputs(C, hw, B, pattern)
    pw = BR.pixel_weights(kind, C, hw, B, pattern).reshape(B, 1, hw)
    return x["z"].cuda(), x["t"].cuda(), torch.tensor(x["w"]).cuda(), torch.tensor(LR.LOSS_UPSTREAM).cuda(), pw.cuda()


@pytest.mark.parametrize("kind", BR.WEIGHT_KINDS)
@pytest.mark.parametrize("C", LR.LOSS_C)
def test_loss_pw_fwd_bwd(ops, C, kind):
    for hw in LR.LOSS_HW:
        for B in LR.LOSS_B:
            for pattern in LR.LOSS_PATTERNS:
                z, t, w, up, pw = device_case(C, hw, B, pattern, kind)
                for opt in BR.PW_OPTION_SETS:
                    ref = BR.run(C, hw, B, pattern, kind, opt, torch.float64)
                    o = None if opt == LR.DEFAULTS else opt
                    out, coef = ops.loss_fwd(z, t, w, o, pixel_weight=pw)
                    out = out.cpu()
                    check(kind, "ce", out[0], ref["ce"], LR.LOSS_BARS["ce"], absolute=True)
                    check(kind, "dice", out[1], ref["dice"], LR.LOSS_BARS["dice"], absolute=True)
                    assert float(out[2]) == ref["nvalid"], (C, hw, B, pattern, opt)
                    dz = ops.loss_bwd(z, t, coef, up, options=o, pixel_weight=pw)
                    check(kind, "dz", dz, ref["dz"], LR.LOSS_BARS["dz"])
                    # accumulated onto a buffer of the gradient's own magnitude, as tests/test_loss_options_gpu.py does
                    scale = float(ref["dz"].abs().max()) or 1.0
                    base = scale * torch.randn(z.shape, generator=torch.Generator().manual_seed(3))
                    acc = ops.loss_bwd(z, t, coef, up, dz=base.cuda(), accumulate=True, options=o, pixel_weight=pw)
                    check(kind, "dz", acc.cpu().double() - base.double(), ref["dz"], LR.LOSS_BARS["dz"])


@pytest.mark.parametrize("C", LR.LOSS_C)
def test_maps_of_ones_and_twos_keep_the_bits(ops, deterministic, C):
    """scaling by a power of two commutes with every rounding on the path (deterministic mode: one adder per image)"""
    for hw in (257, 5000):
        for pattern in LR.LOSS_PATTERNS:
            for opt in (None, (2.0, 0.0, 0.5, 0.5)):
                z, t, w, up, _ = device_case(C, hw, 3, pattern, "ones")
                out0, coef0 = ops.loss_fwd(z, t, w, opt)
                dz0 = ops.loss_bwd(z, t, coef0, up, options=opt)
                for kind in ("ones", "twos"):
                    pw = BR.pixel_weights(kind, C, hw, 3, pattern).cuda()
                    out1, coef1 = ops.loss_fwd(z, t, w, opt, pixel_weight=pw)
                    assert torch.equal(out0.view(torch.int32), out1.view(torch.int32)), (C, hw, pattern, opt, kind)
                    dz1 = ops.loss_bwd(z, t, coef1, up, options=opt, pixel_weight=pw)
                    assert torch.equal(dz0.view(torch.int32), dz1.view(torch.int32)), (C, hw, pattern, opt, kind)
                    if kind == "ones":
                        assert torch.equal(coef0.view(torch.int32), coef1.view(torch.int32)), (C, hw, pattern, opt)


@pytest.mark.parametrize("opt", [None, (2.0, 0.0, 0.5, 0.5)])
def test_a_mask_of_weighted_mass_zero_is_an_empty_mask(ops, opt):
    C, hw, B = 5, 257, 3
    z, t, w, up, pw = device_case(C, hw, B, "random_ignore", "plane_zero")
    b, c = BR.plane_zero_at(B, C)
    out, coef = ops.loss_fwd(z, t, w, opt, pixel_weight=pw)
    coef = coef.reshape(B, C, 4)
    assert bool((coef[b, :, 0] == 0).all()) and bool((coef[:b, :, 0] != 0).all())
    # CE alone (the Dice seed 0): the item's gradient is exactly 0, the others' is not
    ce_only = torch.tensor([1.0, 0.0]).cuda()
    dz = ops.loss_bwd(z, t, coef.reshape(-1), ce_only, options=opt, pixel_weight=pw)
    assert float(dz[b].abs().max()) == 0.0 and float(dz[:b].abs().max()) > 0.0
    # the item is the constant 1.0: the CE of the batch is that of the other items and one 1.0
    others, _ = ops.loss_fwd(z[:b].contiguous(), t[:b].contiguous(), w, opt, pixel_weight=pw[:b].contiguous())
    assert abs(float(out[0]) - (float(others[0]) * b + 1.0) / B) < 1e-6


@pytest.mark.parametrize("opt", [None, (2.0, 0.0, 0.5, 0.5)])
def test_a_nan_logit_stays_loud_whatever_its_weight(ops, opt):
    C, hw, B = 5, 257, 3
    z, t, w, up, pw = device_case(C, hw, B, "random_ignore", "random")
    t[1, :, 0, 100] = torch.tensor([1.0, 0.0, 0.0, -1.0, 0.0]).cuda()
    t[1, :, 0, 99] = -1.0                                # its neighbour is void
    for weight in (3.0, 0.0):
        pw = pw.clone()
        pw[1, 0, 100] = weight
        for ch in (0, 1, 3):                             # a target-1 channel, a target-0 channel, an ignored channel
            zn = z.clone()
            zn[1, ch, 0, 100] = float("nan")
            out, coef = ops.loss_fwd(zn, t, w, opt, pixel_weight=pw)
            assert bool(torch.isnan(out[0])), (weight, ch, out)
            dz = ops.loss_bwd(zn, t, coef, up, options=opt, pixel_weight=pw)
            assert bool(torch.isnan(dz[1, :, 0, 100]).all()), (weight, ch)


def test_fused_ce_dice_with_pixel_weight_through_autograd(ops):
    from hrseg_amd.Metrics import losses as PL
    C, B, H, W = 4, 2, 13, 21
    x = LR.inputs(C, H * W, B, "random_ignore")
    pw = BR.pixel_weights("border_like", C, H * W, B, "random_ignore")
    ref = BR.run(C, H * W, B, "random_ignore", "border_like", LR.DEFAULTS, torch.float64)
    for shape in ((B, H, W), (B, 1, H, W)):
        z = x["z"].reshape(B, C, H, W).cuda().requires_grad_(True)
        res = PL.fused_ce_dice(z, x["t"].reshape(B, C, H, W).cuda(), x["w"], pixel_weight=pw.reshape(shape).cuda())
        (LR.LOSS_UPSTREAM[0] * res[0] + LR.LOSS_UPSTREAM[1] * res[1]).backward()
        assert R.absdiff(res[0], ref["ce"]) < LR.LOSS_BARS["ce"] and R.absdiff(res[1], ref["dice"]) < LR.LOSS_BARS["dice"]
        assert R.rel(z.grad.reshape(B, C, 1, H * W), ref["dz"]) < LR.LOSS_BARS["dz"]
    with pytest.raises(ValueError, match="pixel_weight is on"):
        PL.fused_ce_dice(z, x["t"].reshape(B, C, H, W).cuda(), x["w"], pixel_weight=pw.reshape(B, H, W))


def test_cross_entropy_border_through_get_loss_is_the_manual_composition(ops, deterministic):
    from hrseg_amd import train as PT
    from hrseg_amd.Metrics import losses as PL
    B, H, W = 2, 40, 70
    nc, weights = [3, 5], [[1.0, 2.0, 0.5], [1.0, 0.7, 1.3, 2.0, 0.4]]
    g = torch.Generator().manual_seed(8)
    targets = [torch.from_numpy(BR.planes(BR.voronoi(B, n, H, W, seed=20 + n), n, void=BR.voronoi(B, 1, H, W, seed=n) == 0)).cuda()
               for n in nc]
    bw = PL.BorderWeights(10.0, 2.0, 5)
    fns = [[PL.CrossEntropyLoss(border=bw if L == 1 else None, focal_gamma=2.0 * L), PL.SoftDiceLoss(num_classes=n)]
           for L, n in enumerate(nc)]
    zs = [torch.randn(B, n, H, W, generator=g).cuda().requires_grad_(True) for n in nc]
    loss, _, level = PT.get_loss(zs, targets, fns, [], weights)
    loss.backward()
    assert fns[0][0].last_border is None and fns[1][0].last_border is bw.last and tuple(bw.last.shape) == (B, H, W)
    ref_labels, ref_v, _ = BR.weight_map(targets[1].cpu().numpy(), 5, bw.table())
    assert torch.equal(bw.last.cpu().view(torch.int32), torch.from_numpy(ref_v).view(torch.int32))
    assert float(bw.last.max()) > 1.0
    # the manual composition: the map by hand, the loss ops by hand, the same fp32 adds in level order
    total, grads = 0.0, []
    up = torch.tensor([1.0, 1.0, 0.0]).cuda()
    for L, n in enumerate(nc):
        opt = PL.LossOptions.from_pair(*fns[L]).or_none()
        pw = ops.border_weights(targets[L], 5, bw.lut(targets[L].device))[1] if L == 1 else None
        out, coef = ops.loss_fwd(zs[L].detach(), targets[L], PL._weights(weights[L], zs[L].device), opt, pixel_weight=pw)
        total = total + out[0] + out[1]
        grads.append(ops.loss_bwd(zs[L].detach(), targets[L], coef, up, options=opt, pixel_weight=pw))
    assert torch.equal(loss.detach().view(torch.int32), total.view(torch.int32))
    for z, gz in zip(zs, grads):
        assert torch.equal(z.grad.view(torch.int32), gz.view(torch.int32))
    # CrossEntropyLoss.forward alone: the CE of the same composition
    ce = fns[1][0](zs[1].detach(), targets[1], logits_input=True, class_weight=weights[1])
    pw = ops.border_weights(targets[1], 5, bw.lut(targets[1].device))[1]
    out, _ = ops.loss_fwd(zs[1].detach(), targets[1], PL._weights(weights[1], zs[1].device), (2.0, 0.0, 0.5, 0.5), pixel_weight=pw)
    assert torch.equal(ce.view(torch.int32), out[0].view(torch.int32))
