"""hrseg_logits_up_bwd with one thread per (pixel, channel) and the candidate ranges narrowed before the double loop.

Reference: the transpose of the forward, taken as the float64 autograd of torch.nn.functional.interpolate(mode="bilinear",
align_corners=True) on the CPU; the bar is the one tests/test_headloss_gpu.py holds this kernel to (headloss_ref.UP_BARS["din"]:
max |error| / max |reference| < 1e-5).  Shapes: an integer scale on odd sizes over several blocks, a non-integer scale with
C = 7, a one-row input (vertical scale 0: every output row lands on the row), and a row stride larger than C.  The kernel has
no atomics: two launches on one input give the same bits."""
import pytest
import torch

from tests import headloss_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = 7.25
# (B, C, Hi, Wi, Ho, Wo)
SHAPES = [(2, 4, 13, 11, 52, 44), (1, 7, 20, 20, 77, 80), (2, 4, 1, 5, 4, 20)]


def _reference(d, Hi, Wi):
    B, C, Ho, Wo = d.shape
    x = torch.zeros(B, C, Hi, Wi, dtype=torch.float64, requires_grad=True)
    out = torch.nn.functional.interpolate(x, size=(Ho, Wo), mode="bilinear", align_corners=True)
    out.backward(d.double())
    return x.grad                                           # [B, C, Hi, Wi]


def _input(shape):
    B, C, Hi, Wi, Ho, Wo = shape
    g = torch.Generator().manual_seed(31 * Hi + 7 * Wo + C)
    return torch.randn(B, C, Ho, Wo, generator=g)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"B{s[0]}C{s[1]}_{s[2]}x{s[3]}to{s[4]}x{s[5]}")
def test_logits_up_bwd_is_the_transpose_of_the_forward(shape):
    from hrseg_amd import ops
    B, C, Hi, Wi, Ho, Wo = shape
    d = _input(shape)
    ref = _reference(d, Hi, Wi)
    got = ops.logits_up_bwd(d.cuda(), Hi, Wi, True)         # NHWC
    again = ops.logits_up_bwd(d.cuda(), Hi, Wi, True)
    torch.cuda.synchronize()
    err = R.rel(got.permute(0, 3, 1, 2), ref)
    print(f"{shape}: max |error| / max |reference| {err:.3e} (bar {R.UP_BARS['din']:.0e})")
    assert err < R.UP_BARS["din"]
    assert torch.equal(got, again)


def test_logits_up_bwd_with_a_row_stride_larger_than_c():
    from hrseg_amd._lib import call, ptr
    shape = SHAPES[0]
    B, C, Hi, Wi, Ho, Wo = shape
    d = _input(shape)
    ref = _reference(d, Hi, Wi)
    dbuf = torch.full((B, Hi, Wi, 2 + C + 3), SENTINEL, device="cuda")
    din = dbuf[..., 2:2 + C]
    call("hrseg_logits_up_bwd", ptr(d.cuda()), B, Hi, Wi, C, ptr(din), 2 + C + 3, Ho, Wo, 1)
    torch.cuda.synchronize()
    assert bool((dbuf[..., :2] == SENTINEL).all()) and bool((dbuf[..., 2 + C:] == SENTINEL).all())
    err = R.rel(din.permute(0, 3, 1, 2), ref)
    print(f"{shape} lddin {2 + C + 3}: max |error| / max |reference| {err:.3e}")
    assert err < R.UP_BARS["din"]
