"""The reference side of the non-finite contract (tests/nonfinite_ref.py), pinned where no GPU is needed: what torch does with
NaN / Inf in the operations the HIP kernels restate, the resize must / may sets, and the oracle's train step on a poisoned
batch -- the behaviour tests/test_nonfinite_gpu.py holds the port to.  A wrong reference cannot satisfy the GPU test unnoticed."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import nonfinite_ref as N
from tests.helpers import CASES, build_model, level_weights_for, load_golden, load_tree


def test_classes_codes():
    t = torch.tensor([0.0, -0.0, 1e38, float("inf"), float("-inf"), float("nan"), -3.0])
    assert N.classes(t).tolist() == [N.FINITE, N.FINITE, N.FINITE, N.POS_INF, N.NEG_INF, N.NAN, N.FINITE]
    with pytest.raises(AssertionError, match="differ in class"):
        N.check_classes(torch.tensor([0.0, 1.0]), torch.tensor([float("nan"), 1.0]), 1e-5, "relu that drops NaN")
    with pytest.raises(AssertionError, match="finite elements"):
        N.check_classes(torch.tensor([float("nan"), 1.1]), torch.tensor([float("nan"), 1.0]), 1e-5, "off value")
    assert N.check_classes(torch.tensor([float("nan"), 1.0]), torch.tensor([float("nan"), 1.0]), 1e-5, "same") == 0.0


def test_torch_relu_maxpool_clamp_keep_nan():
    nan, inf = float("nan"), float("inf")
    r = F.relu(torch.tensor([nan, inf, -inf, -0.0, -1.0, 2.0], dtype=torch.float64))
    assert math.isnan(float(r[0])) and r[1:].tolist() == [inf, 0.0, 0.0, 0.0, 2.0]
    assert math.copysign(1.0, float(r[3])) == 1.0 or float(r[3]) == 0.0
    for k in range(4):                                         # the NaN in each of the four window positions
        x = torch.arange(16, dtype=torch.float64).reshape(1, 1, 4, 4)
        x[0, 0, k >> 1, k & 1] = nan
        y = F.max_pool2d(x, 2)
        assert math.isnan(float(y[0, 0, 0, 0])) and bool(torch.isfinite(y.reshape(-1)[1:]).all())
    c = torch.tensor([nan, 1e-9, 0.5, -inf], dtype=torch.float64).clamp(min=1e-8)
    assert math.isnan(float(c[0])) and c[1:].tolist() == [1e-8, 0.5, 1e-8]


@pytest.mark.parametrize("special", list(N.SPECIALS))
def test_training_batch_norm_poisons_the_channel_and_its_running_statistics(special):
    shape = (2, 5, 7, 48)
    y = N.base(shape, 1, scale=2.0, shift=0.5)
    pos = N.positions(shape)["interior"]
    ch = pos[3]
    gamma, beta = torch.rand(48, generator=N._gen(2)) + 0.5, torch.randn(48, generator=N._gen(3)) * 0.1
    ref = N.bn_ref(N.poisoned(y, pos, special), gamma, beta, torch.zeros(48), torch.ones(48), True, relu=True)
    cls = N.classes(ref["z"])
    assert bool((cls[..., ch] == N.NAN).all()), "every pixel of the poisoned channel is NaN after BatchNorm + ReLU"
    others = [c for c in range(48) if c != ch]
    assert bool((cls[..., others] == N.FINITE).all())
    assert not math.isfinite(float(ref["rm"][ch])) and not math.isfinite(float(ref["rv"][ch]))
    assert bool(torch.isfinite(ref["rm"][others]).all()) and bool(torch.isfinite(ref["rv"][others]).all())
    assert bool((ref["mask"].reshape(-1, 12)[:, ch // 4] >> (ch % 4) & 1 == 0).all()), "mask bits of NaN elements are 0"
    # eval mode: only the poisoned element, and relu(-Inf) = 0
    ev = N.bn_ref(N.poisoned(y, pos, special), gamma, beta, torch.zeros(48), torch.ones(48), False, relu=True)
    want = torch.zeros(shape, dtype=torch.int8)
    want[pos] = {"nan": N.NAN, "+inf": N.POS_INF, "-inf": N.FINITE}[special]
    assert torch.equal(N.classes(ev["z"]), want)


@pytest.mark.parametrize("align", [True, False])
@pytest.mark.parametrize("case", N.RESIZE_CASES)
def test_resize_sets_bracket_torch_and_meet_the_cap(case, align):
    Hi, Wi, Ho, Wo = case
    shape = (2, Hi, Wi, 8)
    for name, pos in N.positions(shape).items():
        b, py, px, c = pos
        must, may = N.resize_sets(Hi, Wi, Ho, Wo, align, py, px)
        assert bool(must.any()) and not bool((must & ~may).any()), "must is a non-empty subset of may"
        extra = int((may & ~must).sum())
        print(f"{case} align={align} {name}: must {int(must.sum())}, may {int(may.sum())}, may \\ must {extra} of {Ho * Wo}")
        assert extra <= N.RESIZE_MAY_CAP * Ho * Wo
        for dtype in (torch.float64, torch.float32):           # torch itself (0 * NaN = NaN on every tap) lies between the sets
            out = F.interpolate(N.nchw(N.poisoned(N.base(shape, 4), pos, "nan")).to(dtype), size=(Ho, Wo), mode="bilinear",
                                align_corners=align)
            N.check_sets(out[b, c], must, may, f"torch {dtype}")
            rest = torch.ones(2, 8, dtype=torch.bool)
            rest[b, c] = False
            assert bool(torch.isfinite(out[rest]).all()), "other planes stay finite"
    # the transpose: a poisoned upstream-gradient pixel reaches exactly the inputs it interpolates from; the positions are the
    # ones the GPU test poisons (N.grad_positions), the cap is the same 5 %, of the Hi x Wi outputs of the plane
    for name, (b, oy, ox, c) in N.grad_positions((2, Ho, Wo, 8)).items():
        bm, bmay = N.resize_bwd_sets(Hi, Wi, Ho, Wo, align, oy, ox)
        extra = int((bmay & ~bm).sum())
        print(f"{case} align={align} transpose {name} ({oy},{ox}): must {int(bm.sum())}, may {int(bmay.sum())}, may \\ must {extra} of {Hi * Wi}")
        assert bool(bm.any()) and not bool((bm & ~bmay).any())
        assert extra <= N.RESIZE_MAY_CAP * Hi * Wi
        assert int(bm.sum()) == (4 if name == "interior" else 1), "interior: four taps of non-zero weight; tail: the clamped last pixel"
        x = N.nchw(N.base(shape, 5)).double().requires_grad_(True)
        d = torch.randn(2, 8, Ho, Wo, dtype=torch.float64, generator=N._gen(6))
        d[b, c, oy, ox] = float("nan")
        F.interpolate(x, size=(Ho, Wo), mode="bilinear", align_corners=align).backward(d)
        N.check_sets(x.grad[b, c], bm, bmay, "autograd")


def test_group_kl_reference_keeps_nan():
    z = torch.randn(2, 5, 3, 4, generator=N._gen(7))
    pp = torch.rand(2, 2, 3, 4, generator=N._gen(8))
    z[1, 3, 2, 1] = float("nan")
    sums, dz = N.group_kl_ref(z, pp, [0, 1], [2, 3])
    assert math.isfinite(float(sums[0])) and math.isnan(float(sums[1]))
    assert bool(torch.isnan(dz[1, 2:, 2, 1]).all()) and bool(torch.isfinite(dz[:, :2]).all())


@pytest.mark.parametrize("name", ["hrnet_hier_tl_64", "unet_flat_tl_32"])
def test_oracle_step_on_a_nan_pixel_gives_a_non_finite_loss(name):
    from oracle import models as OM
    from oracle import train_step as OT
    kind, hier, tree_file, size, batch = CASES[name]
    g = load_golden(name)
    tree = load_tree(tree_file)
    model = build_model(OM, kind, hier, tree, size)
    opt = torch.optim.AdamW(model.parameters(), lr=1e-4)
    x = torch.from_numpy(g["x"]).clone()
    x[1, 1, size // 2, size // 3] = float("nan")
    out = OT.train_step(model, opt, x, torch.from_numpy(g["target"]), [int(v) for v in g["num_classes"]],
                        level_weights_for(tree_file, hier), hierarchical=hier, is_unet=(kind == "unet"), with_metrics=False)
    loss = float(out["loss"].detach())
    assert not math.isfinite(loss), loss
