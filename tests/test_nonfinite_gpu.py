"""Non-finite values stay loud on the activation path (include/hrseg.h): every ReLU, maximum and clamp of the library against
the float64 torch reference of the same operation on inputs that carry ONE NaN, +Inf or -Inf (tests/nonfinite_ref.py states
the contract; tests/test_nonfinite_cpu.py pins the reference side), and one train step of two golden models on a poisoned
batch and on a poisoned weight: FusedAdamW(skip_nonfinite=True) must void it.

fmaxf(v, 0.f) returns the operand that is not NaN: with it a NaN activation became 0 in the very kernel that produced it, the
loss stayed finite and the step was applied."""
import argparse
import math

import pytest
import torch

from tests import headloss_ref as R
from tests import nonfinite_ref as N
from tests.helpers import CASES, build_model, level_weights_for, load_golden, load_tree
from tests.test_presplit_gpu import _assert_bytes_are_the_model

pytestmark = pytest.mark.gpu

SPECIAL_NAMES = list(N.SPECIALS)


@pytest.fixture(scope="module")
def ops():
    from hrseg_amd import ops as o
    assert torch.cuda.is_available()
    return o


# ====================================================================================================== BatchNorm
def _bn_params(C, key):
    g = N._gen(C, key)
    return (torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.1, torch.randn(C, generator=g) * 0.1,
            torch.rand(C, generator=g) + 0.5)


def _mask_check(got_mask, ref, what):
    """bits of NaN elements are 0; every other bit is [pre > 0] wherever the float64 pre-activation is not within 1e-4 of 0
    (there float32 rounding may decide the sign)"""
    C = ref["pre"].shape[-1]
    pre = ref["pre"].reshape(-1, C // 4, 4)
    bits = (got_mask.cpu().to(torch.int32)[..., None] >> torch.arange(4, dtype=torch.int32)) & 1
    nan = torch.isnan(pre)
    assert not bool(bits[nan].any()), f"{what}: relu_mask bit set for a NaN element"
    sure = ~nan & (pre.abs() > 1e-4)
    assert torch.equal(bits[sure], (pre[sure] > 0).to(torch.int32)), f"{what}: relu_mask"


@pytest.mark.parametrize("special", SPECIAL_NAMES)
@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("C,shape", [(48, (2, 5, 7, 48)), (1024, (2, 3, 3, 1024))])
def test_bn_fwd_group_keeps_the_class_of_every_element(ops, C, shape, training, special):
    """C = 48: Q = 12 channel quads, 4 idle threads per block; C = 1024: one pixel lane.  Variants: no residual, residual +
    relu_mask, residual + z_split (its bytes against the pre-split model of the plain output); the special once in y and once in the residual, at an
    interior element and in the last quad of the last pixel.  Training: the whole channel and its running statistics go
    non-finite, every other channel stays within the 1e-5 bar."""
    gamma, beta, rm, rv = _bn_params(C, 1)
    y0 = N.base(shape, 11, scale=2.0, shift=0.5)
    r0 = N.base(shape, 12)
    npix = shape[0] * shape[1] * shape[2]
    for pname, pos in N.positions(shape).items():
        for variant, has_res, mask, split in (("plain", False, False, False), ("residual+mask", True, True, False),
                                              ("residual+z_split", True, False, True)):
            for where in (("y", "residual") if has_res else ("y",)):
                what = f"C={C} training={training} {special} in {where} at {pname}, {variant}"
                y = N.poisoned(y0, pos, special) if where == "y" else y0
                r = (N.poisoned(r0, pos, special) if where == "residual" else r0) if has_res else None
                ref = N.bn_ref(y, gamma, beta, rm, rv, training, residual=r, relu=True)
                it = dict(y=y.cuda(), gamma=gamma.cuda(), beta=beta.cuda(), rm=rm.cuda(), rv=rv.cuda(),
                          nbt=torch.zeros((), dtype=torch.int64, device="cuda"), momentum=0.1, eps=1e-5,
                          residual=r.cuda() if has_res else None, relu=True, z_split=split)
                if mask:
                    it["relu_mask"] = torch.full((npix, C // 4), 0xA5, dtype=torch.uint8, device="cuda")
                z, coef = ops.bn_fwd_group([it], training)[0]
                torch.cuda.synchronize()
                if split:
                    # the pre-split output is held to the plain fp32 output of the same problem, byte for byte through the
                    # format's model (tests/test_presplit_gpu.py: NaN pieces by NaN-ness), and the plain output to the bar:
                    # hi + lo of an infinity is Inf + (Inf - Inf) = NaN, so the joined tensor itself has no class to compare
                    plain = dict(it, rm=rm.cuda(), rv=rv.cuda(), nbt=torch.zeros((), dtype=torch.int64, device="cuda"), z_split=False)
                    zs, z = z, ops.bn_fwd_group([plain], training)[0][0]
                    torch.cuda.synchronize()
                    _assert_bytes_are_the_model(zs, z, what)
                N.check_classes(z, ref["z"], N.BAR_BN, what)
                if training:
                    N.check_classes(it["rm"], ref["rm"], N.BAR_BN, what + ": running_mean")
                    N.check_classes(it["rv"], ref["rv"], N.BAR_BN, what + ": running_var")
                    if where == "y":
                        assert bool((N.classes(z)[..., pos[3]] != N.FINITE).all()), what
                if mask:
                    _mask_check(it["relu_mask"], ref, what)


@pytest.mark.parametrize("F", [48, 772])
def test_head_bn_fwd_keeps_nan(ops, F):
    """the level heads on the un-normalised tensor (BatchNorm + ReLU recomputed per element): F = 48 keeps the weights in
    registers, F = 772 takes the LDS-weight loop.  Eval coefficients: the NaN pixel's logits are NaN, every other pixel is
    within the bar; training coefficients of the poisoned tensor: NaN everywhere (every logit sums over the NaN channel)"""
    shape, cout = (2, 5, 7, F), 4
    gamma, beta, rm, rv = _bn_params(F, 2)
    g = N._gen(F, 3)
    w, bias = torch.randn(cout, F, generator=g) / F ** 0.5, torch.randn(cout, generator=g)
    y0 = N.base(shape, 13, scale=2.0, shift=0.5)
    for pname, pos in N.positions(shape).items():
        y = N.poisoned(y0, pos, "nan")
        for training in (False, True):
            ref_bn = N.bn_ref(y, gamma, beta, rm, rv, training, relu=True)
            ref = N.nhwc(R.head(N.nchw(ref_bn["z"]), w.double(), bias.double()))
            yd = y.cuda()
            if training:
                coef = ops.bn_train_coef(yd, gamma.cuda(), beta.cuda(), rm.cuda(), rv.cuda(), None, 0.1, 1e-5)
            else:
                coef = ops.bn_eval_coef(gamma.cuda(), beta.cuda(), rm.cuda(), rv.cuda(), 1e-5)
            got = ops.head_bn_fwd(yd, coef, None, w.cuda(), bias.cuda())
            N.check_classes(got, ref, R.BAR_POINT, f"head_bn_fwd F={F} training={training} NaN at {pname}")
            assert bool(torch.isnan(got[pos[0], pos[1], pos[2]]).all())


# ====================================================================================================== pooling, glue
@pytest.mark.parametrize("special", SPECIAL_NAMES)
@pytest.mark.parametrize("H,W", [(5, 8), (31, 17)])
def test_maxpool2_fwd_propagates_nan_from_every_window_position(ops, H, W, special):
    shape = (2, H, W, 64)
    x0 = torch.relu(N.base(shape, 21))                 # exact ties at 0, as after a ReLU
    for k in range(4):
        for oy, ox, c in ((H // 4, W // 4, 5), (H // 2 - 1, W // 2 - 1, 63)):       # an interior window; the last window, last quad
            pos = (1, 2 * oy + (k >> 1), 2 * ox + (k & 1), c)
            x = N.poisoned(x0, pos, special)
            got = ops.maxpool2_fwd(x.cuda())
            N.check_classes(got, N.maxpool_ref(x), 0.0, f"maxpool {H}x{W} {special} in window position {k} of ({oy},{ox})")
            if special != "-inf":
                assert N.classes(got)[1, oy, ox, c] == {"nan": N.NAN, "+inf": N.POS_INF}[special]


@pytest.mark.parametrize("special", SPECIAL_NAMES)
def test_add_copy_relu_bwd(ops, special):
    shape = (2, 5, 7, 48)
    a0, b0 = N.base(shape, 31), N.base(shape, 32)
    for pname, pos in N.positions(shape).items():
        a = N.poisoned(a0, pos, special)
        what = f"{special} at {pname}"
        N.check_classes(ops.add(a.cuda(), b0.cuda(), relu=True), torch.relu(a.double() + b0.double()), R.BAR_POINT, "add+relu " + what)
        N.check_classes(ops.add(b0.cuda(), a.cuda(), relu=False), a.double() + b0.double(), R.BAR_POINT, "add " + what)
        # controls: no ReLU, no maximum -- these propagate by construction
        N.check_classes(ops.copy(a.cuda(), b0.cuda(), accumulate=True), a.double() + b0.double(), R.BAR_POINT, "copy " + what)
        N.check_classes(ops.copy(a.cuda(), torch.empty(shape, device="cuda")), a.double(), 0.0, "copy " + what)
        z = b0.clone()
        z[pos] = 1.5                                    # the poisoned gradient element passes the mask
        N.check_classes(ops.relu_bwd(a.cuda(), z.cuda()), torch.where(z > 0, a, torch.zeros(())).double(), 0.0, "relu_bwd " + what)
        # the one stated departure from torch (include/hrseg.h): the mask is [z > 0], so the gradient of an element whose
        # ACTIVATION is non-finite follows that comparison -- zeroed for NaN and -Inf, passed for +Inf
        zp = N.poisoned(b0, pos, special)
        N.check_classes(ops.relu_bwd(b0.cuda(), zp.cuda()), torch.where(zp > 0, b0, torch.zeros(())).double(), 0.0, "relu_bwd mask " + what)


def test_relu_of_negative_zero_and_of_the_extremes_has_fmaxf_bits(ops):
    """the NaN-keeping ReLU gives the bits fmaxf(v, 0) gave for every input that is not NaN: +0.0 for -0.0, for the smallest
    negative subnormal and for -FLT_MAX; subnormals, FLT_MAX and +0.0 pass unchanged"""
    vals = [-0.0, 0.0, -1e-45, 1e-45, -3.4028234663852886e38, 3.4028234663852886e38, -1.0, 1.0]
    a = torch.tensor(vals, dtype=torch.float32).repeat(2 * 3 * 5 * 2).reshape(2, 3, 5, 16).cuda()
    zero = torch.full_like(a, -0.0)                     # x + (-0.0) = x for every x, -0.0 included
    got = ops.add(a, zero, relu=True)
    want = torch.tensor([0.0, 0.0, 0.0, 1e-45, 0.0, 3.4028234663852886e38, 0.0, 1.0], dtype=torch.float32).repeat(60).reshape(2, 3, 5, 16)
    assert torch.equal(got.cpu().view(torch.int32), want.view(torch.int32))


@pytest.mark.parametrize("special", SPECIAL_NAMES)
@pytest.mark.parametrize("align", [True, False])
@pytest.mark.parametrize("case", N.RESIZE_CASES)
def test_bilinear_fwd_and_fuse_sum_with_relu(ops, case, align, special):
    """relu(base + up(x)) (bilinear_fwd accumulate + relu) and relu(s0 + s1 + up(l0) + up(l1)) (fuse_sum): the special in a
    same-resolution term is the pointwise contract, in a low-resolution term the must / may sets on the poisoned plane; every
    other plane stays within the 1e-5 bar"""
    Hi, Wi, Ho, Wo = case
    C, B = 48, 2
    lo_shape, hi_shape = (B, Hi, Wi, C), (B, Ho, Wo, C)
    x0, l1 = N.base(lo_shape, 41), N.base((B, 3, 4, C), 42)
    base, s1 = N.base(hi_shape, 43), N.base(hi_shape, 44)

    def ref(base_, x_):
        return torch.relu(base_.double() + N.resize_ref(x_, Ho, Wo, align))

    def ref_fuse(base_, x_):
        return torch.relu(base_.double() + s1.double() + N.resize_ref(x_, Ho, Wo, align) + N.resize_ref(l1, Ho, Wo, align))

    def run(base_, x_):
        out = base_.clone().cuda()
        ops.bilinear_fwd(x_.cuda(), out, Ho, Wo, align_corners=align, accumulate=True, relu=True)
        return out

    def run_fuse(base_, x_):
        return ops.fuse_sum([base_.cuda(), s1.cuda()], [x_.cuda(), l1.cuda()], relu=True, align_corners=align)

    for pname, pos in N.positions(hi_shape).items():
        b = N.poisoned(base, pos, special)
        N.check_classes(run(b, x0), ref(b, x0), R.BAR_POINT, f"bilinear_fwd: {special} in the same-resolution term at {pname}")
        N.check_classes(run_fuse(b, x0), ref_fuse(b, x0), R.BAR_POINT, f"fuse_sum: {special} in a same-resolution term at {pname}")
    for pname, pos in N.positions(lo_shape).items():
        x = N.poisoned(x0, pos, special)
        must, may = N.resize_sets(Hi, Wi, Ho, Wo, align, pos[1], pos[2])
        rest = torch.ones(B, Ho, Wo, C, dtype=torch.bool)
        rest[pos[0], :, :, pos[3]] = False
        for name, got, want in (("bilinear_fwd", run(base, x), ref(base, x)), ("fuse_sum", run_fuse(base, x), ref_fuse(base, x))):
            what = f"{name}: {special} in the low-resolution term at {pname}"
            got = got.cpu()
            N.check_sets(got[pos[0], :, :, pos[3]], must, may, what, relu_neg_inf=(special == "-inf"))
            assert bool(torch.isfinite(got[rest]).all()), what
            assert R.rel(got[rest], want[rest]) <= R.BAR_POINT, what


# ====================================================================================================== conv epilogues
def _conv_family_runs():
    """(family counter, precision name, tune knobs for the run, knobs that restore the defaults, Cin, Cout, k, H, W, B)"""
    return [
        ("f32", "f32", {}, {}, 32, 48, 3, 9, 11, 2),
        ("small_cin", "f32", {}, {}, 3, 64, 3, 9, 10, 2),                                     # the 3-channel first layer
        ("small_cin", "f32", dict(small_cin3=0), dict(small_cin3=1), 3, 64, 3, 9, 10, 2),     # the generic Cin <= 8 kernel
        ("sp_im2col", "fp16x2", {}, {}, 64, 64, 1, 9, 11, 2),
        ("patch_sp", "fp16x2", dict(sp_ws=0, sp_patch_min_tiles=1), dict(sp_ws=1, sp_patch_min_tiles=0), 48, 48, 3, 16, 16, 2),
        ("ws", "fp16x2", dict(sp_ws_min_tiles=1, sp_ws_waste=1000), dict(sp_ws_min_tiles=0, sp_ws_waste=200), 64, 64, 3, 20, 23, 3),
    ]


@pytest.mark.parametrize("special", SPECIAL_NAMES)
@pytest.mark.parametrize("run", _conv_family_runs(), ids=lambda r: f"{r[0]}-{r[1]}-{'-'.join(r[2]) or 'default'}")
def test_conv_epilogue_relu_keeps_the_class(ops, run, special):
    """conv_fwd(residual=, relu=True), every kernel family that has a fused epilogue (the launch counter proves the family).
    The special in the residual enters the epilogue only: the class map equals the reference's.  In x it passes the
    contraction first: exact-fp32 families keep the class; fp16x2 splits an infinity into Inf + (Inf - Inf) = NaN
    (hrseg.h: 'Inf or NaN'), so there the non-finite set must cover the reference's and stay inside the special's support"""
    from hrseg_amd import _lib
    fam, prec, knobs, restore, cin, cout, k, H, W, B = run
    g = N._gen(cin, cout, k, H, W)
    x0 = torch.randn(B, H, W, cin, generator=g)
    w = torch.randn(cout, k * k, cin, generator=g) / (cin * k * k) ** 0.5
    bias, r0 = torch.randn(cout, generator=g), torch.randn(B, H, W, cout, generator=g)
    bar = N.BAR_CONV["fp16x2" if prec == "fp16x2" else ("small_cin" if fam == "small_cin" else "f32")]
    code = _lib.CONV_PRECISION[prec]

    def conv(x, r):
        _lib.launch_count(None, reset=True)
        y = ops.conv_fwd(x.cuda(), w.cuda(), bias.cuda(), k, 1, prec=code, residual=r.cuda(), relu=True)
        assert _lib.launch_count(fam) == 1, (fam, {f: _lib.launch_count(f) for f in ("f32", "small_cin", "sp_im2col", "patch_sp", "ws", "sp_wide")})
        return y
    try:
        _lib.tune(**knobs) if knobs else None
        for pname, pos in N.positions((B, H, W, cout)).items():
            r = N.poisoned(r0, pos, special)
            N.check_classes(conv(x0, r), N.conv_ref(x0, w, bias, k, 1, r), bar, f"{fam}: {special} in the residual at {pname}")
        for pname, pos in N.positions((B, H, W, cin)).items():
            x = N.poisoned(x0, pos, special)
            got, ref = conv(x, r0), N.conv_ref(x, w, bias, k, 1, r0)
            what = f"{fam}: {special} in x at {pname}"
            if prec == "fp16x2" and special != "nan":
                support = torch.isnan(N.conv_ref(N.poisoned(x0, pos, "nan"), w, bias, k, 1, r0))
                bad = ~torch.isfinite(got.cpu())
                assert not bool((~torch.isfinite(ref) & ~bad).any()), what + ": finite where the reference is not"
                assert not bool((bad & ~support).any()), what + ": non-finite outside the support"
                assert R.rel(got.cpu()[~support], ref[~support]) <= bar, what
            else:
                N.check_classes(got, ref, bar, what)
    finally:
        if restore:
            _lib.tune(**restore)


# ====================================================================================================== composition / loss
KL_TREE = ([1, 0], [2, 3])


@pytest.mark.parametrize("special", SPECIAL_NAMES)
def test_compose_and_group_kl_keep_the_class(ops, special):
    """one poisoned logit: hrseg_compose_fwd, hrseg_group_kl (its clamp_min(1e-8) answered 1e-8 for NaN) and
    hrseg_group_kl_bwd against float64 torch; the softmax maxima of these kernels drop a NaN but the exponentials that follow
    bring it back, so they need no change -- this sweep is the evidence"""
    parents, sizes = KL_TREE
    B, H, W = 2, 5, 7
    g = N._gen(51)
    z0 = torch.randn(B, sum(sizes), H, W, generator=g)
    pp = torch.sigmoid(torch.randn(B, R.n_prev(parents), H, W, generator=g))
    for pos in ((1, 3, 2, 4), (B - 1, sum(sizes) - 1, H - 1, W - 1), (0, 0, 0, 0)):
        z = z0.clone()
        z[pos] = N.SPECIALS[special]
        what = f"{special} logit at {pos}"
        N.check_classes(ops.compose_fwd(z.cuda(), pp.cuda(), parents, sizes), R.compose(z.double(), pp.double(), parents, sizes),
                        R.BAR_POINT, "compose_fwd: " + what)
        sums, dz = N.group_kl_ref(z, pp, parents, sizes)
        N.check_classes(ops.group_kl_sums(z.cuda(), pp.cuda(), parents, sizes), sums, 1e-5, "group_kl_sums: " + what)
        got = ops.group_kl_bwd(z.cuda(), pp.cuda(), torch.ones(1, device="cuda"), 1.0, parents, sizes)
        N.check_classes(got, dz, 1e-5, "group_kl_bwd: " + what)


@pytest.mark.parametrize("special", ["nan", "+inf"])
@pytest.mark.parametrize("C", [4, 9])
def test_loss_fwd_is_nan_where_the_reference_is(ops, C, special):
    x = R.loss_inputs(C, 257, 3, "random_ignore")
    t = x["t"].clone()
    z = x["z"].clone()
    t[1, C - 1, 0, 100] = 1.0                          # not an ignored pixel
    z[1, C - 1, 0, 100] = N.SPECIALS[special]          # (+Inf: the softmax is Inf - Inf)
    ce, dice, nvalid = R.ce_dice(z.double(), t.double(), x["w"])
    out, _ = ops.loss_fwd(z.cuda(), t.cuda(), torch.tensor(x["w"]).cuda())
    assert math.isnan(float(ce)) and math.isnan(float(dice)), "the reference itself"
    N.check_classes(out[:2], torch.stack([ce, dice]), R.BAR_LOSS, f"loss_fwd C={C} {special}", absolute=True)


# ====================================================================================================== gradient absmax
@pytest.mark.parametrize("relu", [False, True])
def test_bn_bwd_dy_absmax_reports_nan_as_inf_and_the_fp16x2_gradients_are_loud(ops, relu):
    """one NaN in dz: the BatchNorm backward's sums of that channel are NaN, so is its dy; the 64 |dy| slots must say +Inf (as
    hrseg_absmax does for NaN), and a fp16x2 data / weight gradient scaled by that maximum must not come out finite"""
    from hrseg_amd import _lib
    C, shape = 64, (2, 20, 23, 64)
    gamma, beta, rm, rv = _bn_params(C, 6)
    yd = N.base(shape, 61, scale=2.0, shift=0.5).cuda()
    coef = ops.bn_train_coef(yd, gamma.cuda(), beta.cuda(), rm.cuda(), rv.cuda(), None, 0.1, 1e-5)
    z = ops.bn_apply(yd, coef, None, relu)
    dz = N.base(shape, 62)
    pos = tuple(int(v) for v in (z > 0.5).nonzero()[7])          # an element that passes the ReLU mask
    slots = torch.full((64,), 7.0, device="cuda")
    clean = ops.bn_bwd_group([dict(dz=dz.cuda(), z=None, relu=relu, y=yd, coef=coef, dgamma=torch.zeros(C, device="cuda"),
                                   dbeta=torch.zeros(C, device="cuda"), dres=None, dy_absmax=slots)], False)[0]
    assert float(slots.max()) == float(clean.abs().max()), "finite gradient: the slots hold max |dy| exactly"
    dzp = N.poisoned(dz, pos, "nan").cuda()
    dy = ops.bn_bwd_group([dict(dz=dzp, z=None, relu=relu, y=yd, coef=coef, dgamma=torch.zeros(C, device="cuda"),
                                dbeta=torch.zeros(C, device="cuda"), dres=None, dy_absmax=slots)], False)[0]
    assert bool(torch.isnan(dy[..., pos[3]]).all()) and float(slots.max()) == float("inf"), float(slots.max())
    assert float(ops.absmax(dy)) == float("inf")
    pr = _lib.CONV_PRECISION["fp16x2"]
    g = N._gen(63)
    w = (torch.randn(C, 9, C, generator=g) / 24).cuda()
    x = torch.randn(shape, generator=g).cuda()
    dx = ops.conv_dgrad(dy, ops.weight_transpose(w, C, 9, C), shape, 3, 1, prec=pr, gmax=slots)
    assert not bool(torch.isfinite(dx).all()), "fp16x2 data gradient of a NaN gradient came out finite"
    dw = torch.zeros_like(w)
    ops.conv_wgrad(x, dy, dw, 3, 1, prec=pr, gmax=slots)
    assert not bool(torch.isfinite(dw).all()), "fp16x2 weight gradient of a NaN gradient came out finite"


@pytest.mark.parametrize("F", [48, 720])
def test_fused_head_backward_keeps_nan_and_its_absmax_says_inf(ops, F):
    """hrseg_head_bn_bwd_reduce (F = 48: head_bn_bwd_reduce_kernel; F = 720: the LDS-ring kernel) and hrseg_head_bn_bwd_apply
    with one NaN in y, coefficients from the training statistics of that y: the recomputed relu(bn(y)) of the channel is NaN,
    so column `ch` of the head weight gradient is NaN and every other column finite; dy of the channel is NaN and the
    hrseg_head_bn_t.dy_absmax slots read +Inf"""
    shape, cout = (2, 13, 11, F), 3
    gamma, beta, rm, rv = _bn_params(F, 8)
    g = N._gen(F, 81)
    w = (torch.randn(cout, F, generator=g) * 0.1).cuda()
    dzl = (torch.randn(2, 13, 11, cout, generator=g) * 1e-3).cuda()
    pos = N.positions(shape)["interior"]
    ch = pos[3]
    y = N.poisoned(N.base(shape, 82, shift=0.3), pos, "nan").cuda()
    coef = ops.bn_train_coef(y, gamma.cuda(), beta.cuda(), rm.cuda(), rv.cuda(), None, 0.1, 1e-5)
    nch = ops.head_bn_chunks(2 * 13 * 11, F, 1)
    part = torch.empty((nch + 1) * 2 * F, dtype=torch.float64, device="cuda")
    slots = torch.full((64,), 7.0, device="cuda")
    heads = [dict(cout=cout, w=w, dzl=dzl, gb=None, dw=torch.zeros_like(w), dbias=torch.zeros(cout, device="cuda"), dgb=None)]
    ops.head_bn_bwd_reduce(y, coef, 1, part, nch, heads, dy_absmax=slots)
    dgamma, dbeta = torch.zeros(F, device="cuda"), torch.zeros(F, device="cuda")
    ops.bn_bwd_finalize(y, coef, 1, part, nch, dgamma, dbeta)
    dy = ops.head_bn_bwd_apply(y, coef, 1, part, nch, heads, dy_absmax=slots)
    torch.cuda.synchronize()
    others = [c for c in range(F) if c != ch]
    dw = heads[0]["dw"].cpu()
    assert bool(torch.isnan(dw[:, ch]).all()), f"dW of the NaN channel is finite: {dw[:, ch].tolist()}"
    assert bool(torch.isfinite(dw[:, others]).all()) and bool(torch.isfinite(heads[0]["dbias"]).all())
    assert bool(torch.isnan(dy[..., ch]).all()) and bool(torch.isfinite(dy[..., others]).all())
    assert float(slots.max()) == float("inf"), float(slots.max())


# ====================================================================================================== one train step
def _setup(name):
    from hrseg_amd.Models import models as PM
    from hrseg_amd.Metrics import losses as PL
    from hrseg_amd import train as PT
    kind, hier, tree_file, size, batch = CASES[name]
    g = load_golden(name)
    tree = load_tree(tree_file)
    nc = [int(v) for v in g["num_classes"]]
    args = argparse.Namespace(model_type=1 if hier else 0, model_select=0 if kind == "unet" else 1, num_classes=nc,
                              level_weights=level_weights_for(tree_file, hier), level0_pretrain_epochs=None, batch_size=batch)
    model = build_model(PM, kind, hier, tree, size).cuda()
    model.train()
    opt = PT.FusedAdamW(model, lr=[1e-3], skip_nonfinite=True)
    fns = [[PL.CrossEntropyLoss(), PL.SoftDiceLoss(num_classes=n)] for n in nc]
    return model, opt, fns, args, tree, g, size


@pytest.mark.parametrize("name", ["hrnet_hier_tl_64", "unet_flat_tl_32"])
def test_a_poisoned_step_is_void_and_a_clean_step_is_applied(name):
    """eager steps with FusedAdamW(skip_nonfinite=True): clean, (a) one input pixel NaN, clean, (b) one backbone convolution
    weight +Inf.  In (a) and (b) the loss or the gradient verdict is non-finite, the step is void (parameters and both moments
    bit for bit as before); the clean steps are applied.  (BatchNorm running statistics are poisoned by the forward pass of (a)
    before the step is voided, as in torch: known; a training step does not read them.)"""
    from hrseg_amd import train as PT
    model, opt, fns, args, tree, g, size = _setup(name)
    x, t = torch.from_numpy(g["x"]).cuda(), torch.from_numpy(g["target"]).cuda()
    flat = model.flatten_parameters()

    def step(xin):
        loss = float(PT.train_step(model, opt, xin, t, fns, args, tree, [])[0])
        norm, coef, finite, skipped = opt.grad_stats.tolist()
        return loss, finite, int(skipped)

    def state():
        return [v.clone() for v in (flat.data, opt._m, opt._v, opt._state)]

    def same(a, b):
        return all(torch.equal(p.view(torch.int32), q.view(torch.int32)) for p, q in zip(a, b))

    loss, finite, skipped = step(x)
    assert math.isfinite(loss) and finite == 1.0 and skipped == 0
    before = state()
    xp = x.clone()
    xp[1, 1, size // 2, size // 3] = float("nan")
    loss, finite, skipped = step(xp)
    print(f"{name} (a) NaN pixel: loss {loss}, finite verdict {finite}, skipped {skipped}")
    assert not math.isfinite(loss), f"the loss of a step on a NaN pixel is {loss}: the oracle's is NaN (test_nonfinite_cpu.py)"
    assert finite == 0.0 and skipped == 1, (loss, finite, skipped)
    assert same(state(), before), "a void step changed parameters or moments"
    loss, finite, skipped = step(x)
    assert math.isfinite(loss) and finite == 1.0 and skipped == 1
    after_clean = state()
    assert not torch.equal(after_clean[0], before[0]) and float(after_clean[3][0]) == 2.0, "the clean step in between is applied"
    # (b) the first element of a backbone convolution weight (4-D, at least 16 input channels: not the stem)
    p = next(q for _, q in model.named_parameters() if q.dim() == 4 and q.shape[1] >= 16 and q.shape[2] == 3)
    idx = (p.data_ptr() - flat.data.data_ptr()) // 4
    assert 0 <= idx < flat.numel
    flat.data[idx] = float("inf")
    before = state()
    loss, finite, skipped = step(x)
    print(f"{name} (b) +Inf weight: loss {loss}, finite verdict {finite}, skipped {skipped}")
    assert finite == 0.0 and skipped == 2, (loss, finite, skipped)
    assert same(state(), before), "a void step changed parameters or moments"


# ====================================================================================================== resize kernels without ReLU
@pytest.mark.parametrize("special", SPECIAL_NAMES)
@pytest.mark.parametrize("align", [True, False])
@pytest.mark.parametrize("case", N.RESIZE_CASES)
def test_resize_kernels_must_may_sets(ops, case, align, special):
    """bilinear_bwd, bilinear_bwd_multi (and its absmax: NaN counts as +Inf), logits_up_fwd / logits_up_bwd and head_mix: the
    poisoned element reaches every output it has a non-zero weight on and nothing outside its 2 x 2 support; other planes stay
    finite"""
    Hi, Wi, Ho, Wo = case
    B, C = 2, 48

    def planes_ok(got_nhwc, b, c, must, may, what):
        got_nhwc = got_nhwc.cpu()
        N.check_sets(got_nhwc[b, :, :, c], must, may, what)
        rest = torch.ones(got_nhwc.shape, dtype=torch.bool)
        rest[b, :, :, c] = False
        assert bool(torch.isfinite(got_nhwc[rest]).all()), what + ": another plane went non-finite"

    # forward direction: head_mix (y += up(low) + bias, in place) and logits_up_fwd (NHWC logits -> NCHW)
    low0, y0 = N.base((B, Hi, Wi, C), 71), N.base((B, Ho, Wo, C), 72)
    bias = torch.randn(C, generator=N._gen(73))
    for pname, pos in N.positions((B, Hi, Wi, C)).items():
        must, may = N.resize_sets(Hi, Wi, Ho, Wo, align, pos[1], pos[2])
        y = y0.clone().cuda()
        ops.head_mix(y, [N.poisoned(low0, pos, special).cuda()], bias.cuda(), align_corners=align)
        planes_ok(y, pos[0], pos[3], must, may, f"head_mix: {special} in the low-resolution term at {pname}")
    for pname, pos in N.positions((B, Ho, Wo, C)).items():
        y = N.poisoned(y0, pos, special).cuda()
        ops.head_mix(y, [low0.cuda()], bias.cuda(), align_corners=align)
        N.check_classes(y, N.poisoned(y0, pos, special).double() + N.resize_ref(low0, Ho, Wo, align) + bias.double(), R.BAR_POINT,
                        f"head_mix: {special} in y at {pname}")
    z0 = N.base((B, Hi, Wi, 8), 74)
    for pname, pos in N.positions((B, Hi, Wi, 8)).items():
        must, may = N.resize_sets(Hi, Wi, Ho, Wo, align, pos[1], pos[2])
        out = ops.logits_up_fwd(N.poisoned(z0, pos, special).cuda(), Ho, Wo, align_corners=align)
        planes_ok(out.permute(0, 2, 3, 1), pos[0], pos[3], must, may, f"logits_up_fwd: {special} at {pname}")
    # transpose direction: the upstream gradient is poisoned at an output-side pixel
    d0, dl0 = N.base((B, Ho, Wo, C), 75), N.base((B, Ho, Wo, 8), 76)
    for pname, pos in N.grad_positions((B, Ho, Wo, C)).items():
        must, may = N.resize_bwd_sets(Hi, Wi, Ho, Wo, align, pos[1], pos[2])
        d = N.poisoned(d0, pos, special).cuda()
        planes_ok(ops.bilinear_bwd(d, (B, Hi, Wi, C), Ho, Wo, align_corners=align), pos[0], pos[3], must, may,
                  f"bilinear_bwd: {special} at {pname}")
        dins, amax = ops.bilinear_bwd_multi(d, [(Hi, Wi)], align_corners=align, want_absmax=True)
        planes_ok(dins[0], pos[0], pos[3], must, may, f"bilinear_bwd_multi: {special} at {pname}")
        assert float(amax.max()) == float("inf"), "bilinear_bwd_multi absmax: a non-finite gradient reads +Inf"
        c8 = min(pos[3], 7)
        dl = N.poisoned(dl0, pos[:3] + (c8,), special)
        din = ops.logits_up_bwd(N.nchw(dl).cuda(), Hi, Wi, align_corners=align)
        planes_ok(din, pos[0], c8, must, may, f"logits_up_bwd: {special} at {pname}")
