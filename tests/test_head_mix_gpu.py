"""hrseg_head_mix (ops.head_mix): y = t0 + sum_j up(t_j) + bias in place over t0, with the BatchNorm partial sums of y left
behind -- the forward glue of the HRNet head at branch resolution (engine.Recorder.head_conv_bn).

Against the existing kernels: hrseg_fuse_sum (relu = 0) on [t0] + lows, then the bias added in torch.  The kernel adds the same
fp32 terms with the bias last instead of in torch's own pass and may contract or order the four interpolation products
differently: at most four more or differently ordered fp32 additions per element than the composition, so per element
    |delta| <= 8 * 2^-24 * (|t0| + sum_j |interp_j| + |b|)
(each of at most 8 roundings of half an ulp relative to a partial sum that the magnitude sum bounds).  interp_j is evaluated by
hrseg_fuse_sum on a zero tensor + the one low term.

The partial sums: mean and rstd that the BatchNorm finalize phase derives from them, against those of the statistics phase run
on the produced y.  Both are sums of the same N = B * H * W fp32 terms per channel in different orders: they agree to the
project's summation floor sqrt(N) * 2^-24 (tests/test_head_bn_fused_gpu.py FLOOR), relative to the size of the summands -- the
channel's root mean square for the mean (a mean near zero has no relative accuracy in any summation order), rstd itself for
rstd (the inputs have unit variance around a 0.3 offset: no cancellation in the variance).

Two runs give the same bits (fixed chunk -> row assignment, fixed order inside a chunk, no atomics)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

B, H, W = 2, 5, 7
LOWS = [(3, 4), (2, 2), (1, 1)]             # the last one is the degenerate scale (every output pixel reads the one input pixel)
WIDTHS = [8, 24, 720]                       # 2 and 6 channel quads x 16 pixel lanes; 180 quads x 5 lanes (60 threads of 960 idle)
U = 2.0 ** -24


def _inputs(C, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)

    def rnd(*shape):
        return torch.randn(shape, generator=gen, device="cuda")
    t0 = rnd(B, H, W, C) + 0.3
    lows = [rnd(B, h, w, C) for h, w in LOWS]
    lows[1] = (rnd(B, LOWS[1][0], LOWS[1][1], C + 12))[..., 4:4 + C]      # a channel slice: row stride C + 12
    lows[1].copy_(rnd(B, LOWS[1][0], LOWS[1][1], C))
    bias = rnd(C) * 0.5
    return t0, lows, bias


@pytest.mark.parametrize("align", [True, False], ids=["align", "noalign"])
@pytest.mark.parametrize("C", WIDTHS)
def test_head_mix_against_fuse_sum_and_the_statistics_phase(C, align):
    from hrseg_amd import ops
    t0, lows, bias = _inputs(C, 100 * C + int(align))
    assert lows[1].stride(2) == C + 12
    want = ops.fuse_sum([t0], lows, relu=False, align_corners=align) + bias
    zero = ops.zeros(t0.shape, torch.float32, t0.device)
    mag = t0.abs() + bias.abs()
    for low in lows:
        mag = mag + ops.fuse_sum([zero], [low], relu=False, align_corners=align).abs()
    runs = []
    for _ in range(2):
        y = ops.clone(t0)
        part, nch = ops.head_mix(y, lows, bias, align_corners=align)
        runs.append((y, part.clone(), nch))
    torch.cuda.synchronize()
    y, part, nch = runs[0]
    if C == 720:
        assert nch > 1, "the 720-channel case spans several chunks"
    delta = (y.double() - want.double()).abs()
    bound = 8 * U * mag.double()
    print(f"C={C} align={align}: max |delta| {float(delta.max()):.3e}, max delta/bound {float((delta / bound).max()):.3f}, chunks {nch}")
    assert bool((delta <= bound).all())
    # the same bits in a second run: the tensor and the partial sums
    assert torch.equal(runs[1][0], y) and torch.equal(runs[1][1], part) and runs[1][2] == nch

    # finalize on the kernel's partial sums against statistics + finalize on the produced y
    def bn_args():
        return dict(y=y, gamma=torch.ones(C, device="cuda"), beta=torch.zeros(C, device="cuda"), rm=torch.zeros(C, device="cuda"),
                    rv=torch.ones(C, device="cuda"), nbt=torch.zeros(1, dtype=torch.int64, device="cuda"), momentum=0.1, eps=1e-5,
                    residual=None, relu=True, out=y)
    coef_p = ops.bn_fwd_group([dict(bn_args(), partial=(part, nch))], True, phases=2)[0][1]
    coef_s = ops.bn_fwd_group([bn_args()], True, phases=3)[0][1]
    torch.cuda.synchronize()
    N = B * H * W
    floor = N ** 0.5 * U
    yd = y.double().reshape(N, C)
    rms = (yd * yd).mean(0).sqrt()
    mean_p, mean_s = coef_p[:C].double(), coef_s[:C].double()
    rstd_p, rstd_s = coef_p[C:2 * C].double(), coef_s[C:2 * C].double()
    dm, dr = ((mean_p - mean_s).abs() / rms).max(), ((rstd_p - rstd_s).abs() / rstd_s).max()
    print(f"  mean: max deviation / rms {float(dm):.3e}; rstd: max relative deviation {float(dr):.3e}; floor {floor:.3e}")
    assert float(dm) <= floor and float(dr) <= floor
    # and both sit on the fp64 statistics of y
    assert float(((mean_p - yd.mean(0)).abs() / rms).max()) <= floor + U


def test_head_mix_refuses_bad_arguments():
    from hrseg_amd import ops
    t0, lows, bias = _inputs(8, 1)
    with pytest.raises(RuntimeError, match="hrseg_head_mix"):
        ops.head_mix(t0, lows + [lows[0]], bias)                       # four low-resolution terms
    with pytest.raises(RuntimeError, match="hrseg_head_mix"):
        ops.head_mix(t0[..., :6], [], None)                            # 6 channels: not a multiple of 4
