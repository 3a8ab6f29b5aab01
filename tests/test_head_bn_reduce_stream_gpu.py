"""The first pass of the fused head + BatchNorm backward (hrseg_head_bn_bwd_reduce) on chunks long enough to stream.

At 720 channels the pass runs as a loader / consumer kernel: 256 threads move the chunk's rows through a two-slot ring in LDS in
stages of 16 rows, 256 threads add.  tests/test_head_bn_fused_gpu.py holds the pass to equality with the unfused composition on
chunks of 9 and 37 pixels -- at most three stages, so a defect of the steady state (a slot read before it is written, a stage
consumed twice, the sample boundary met in the middle of the stream) would pass there.  The cases here:

  - 140 x 140, two samples per segment: 256 chunks of 154 pixels (ten stages; 154 is no multiple of 16: the last stage is short),
    19,600 pixels per sample is no multiple of 154 (one chunk meets the sample boundary in mid-stream, FiLM on: the dgb flush),
    the last chunk of the segment is short; run twice on different inputs in one process (nothing left over from a launch matters)
  - the same with two segments, one launch per level with the last level first as the model does, FiLM on one level only
  - 13 x 11: chunks shorter than one stage (the pipeline drains without ever filling)
  - row-padded y (ldy = F + 8) and row-padded logit gradients
  - Cout = 7 (the eight-output instance)
  - F = 64 (sixteen pixel lanes per block: the kernel small rows take)
  - F = 800 (200 channel quads: all four adding waves hold quads, the bias sum stays with thread 0)

Reference: ops.head_bwd into a zeroed buffer, then ops.bn_bwd_group -- unchanged code.  dy, dgamma, dbeta and max|dy| must be EQUAL
(the pass adds the same terms per thread in the same order); dW, dbias and dgb are atomic sums on both sides and are held to the
fp64-distance criterion of tests/test_head_bn_fused_gpu.py."""
import pytest
import torch

from tests.test_head_bn_fused_gpu import B, _no_further, _ref64

pytestmark = pytest.mark.gpu

# name -> (F, (H, W), Cout per segment, FiLM per segment, extra floats per row of y, one launch for all segments, seed)
CASES = {
    "stream_140x140": (720, (140, 140), [4], [True], 0, True, 1),
    "stream_140x140_again": (720, (140, 140), [4], [True], 0, True, 2),
    "two_levels_last_first": (720, (140, 140), [4, 3], [False, True], 0, False, 3),
    "shorter_than_a_stage": (720, (13, 11), [4], [True], 0, True, 4),
    "padded_rows": (720, (70, 67), [4], [True], 8, True, 5),
    "cout7": (720, (70, 67), [7], [True], 0, True, 6),
    "F64": (64, (70, 67), [4], [True], 0, True, 7),
    "F800": (800, (70, 67), [4], [True], 0, True, 8),
}


def _run(case):
    from hrseg_amd import ops
    F, (H, W), couts, films, pad, one_launch, seed = case
    nseg = len(couts)
    gen = torch.Generator(device="cuda").manual_seed(977 * seed + F)

    def rnd(*shape, scale=1.0):
        return torch.randn(shape, generator=gen, device="cuda") * scale
    ybuf = rnd(nseg * B, H, W, F + pad) + 0.3
    y = ybuf[..., :F]
    gamma, beta = 1.0 + 0.2 * rnd(F), 0.3 * rnd(F)
    rm, rv = torch.zeros(F, device="cuda"), torch.ones(F, device="cuda")
    nbt = torch.zeros(1, dtype=torch.int64, device="cuda")
    coef = ops.bn_train_coef(y, gamma, beta, rm, rv, nbt, 0.1, 1e-5)
    zbuf = torch.empty_like(ybuf)
    z = ops.bn_apply(y, coef, relu=True, out=zbuf[..., :F])
    heads = []
    for s in range(nseg):
        co = couts[s]
        dzbuf = rnd(B, H, W, co + (3 if pad else 0), scale=1e-3)
        heads.append(dict(cout=co, w=rnd(co, F, scale=0.1), bias=rnd(co, scale=0.1),
                          gb=torch.cat([1.0 + 0.1 * rnd(B, F), 0.1 * rnd(B, F)], dim=1).contiguous() if films[s] else None,
                          dzl=dzbuf[..., :co]))
    # the reference: head_bwd per segment into a zeroed buffer, then the grouped BatchNorm backward (in place)
    df = ops.zeros(ybuf.shape, torch.float32, ybuf.device)[..., :F]
    un = []
    for s, h in enumerate(heads):
        dw, dbias = torch.zeros_like(h["w"]), torch.zeros_like(h["bias"])
        dgb = torch.zeros_like(h["gb"]) if h["gb"] is not None else None
        ops.head_bwd(z[s * B:(s + 1) * B], h["gb"], h["w"], h["dzl"], dw, dbias, dgb, df=df[s * B:(s + 1) * B], cout=h["cout"])
        un.append((dw, dbias, dgb))
    dgamma_u, dbeta_u = torch.zeros(F, device="cuda"), torch.zeros(F, device="cuda")
    gmax_u = torch.empty(64, device="cuda")
    dy_u = ops.bn_bwd_group([dict(dz=df, z=None, relu=True, y=y, coef=coef, dgamma=dgamma_u, dbeta=dbeta_u, nseg=nseg,
                                  dy_absmax=gmax_u)], False)[0]
    # the fused passes
    npix = nseg * B * H * W
    nch = ops.head_bn_chunks(npix, F, nseg)
    part = torch.empty((nch + nseg) * 2 * F, dtype=torch.float64, device="cuda")
    gmax = torch.full((64,), 7.0, device="cuda")            # (the first pass resets it)
    fused = [dict(h, dw=torch.zeros_like(h["w"]), dbias=torch.zeros_like(h["bias"]),
                  dgb=torch.zeros_like(h["gb"]) if h["gb"] is not None else None) for h in heads]
    if one_launch:
        ops.head_bn_bwd_reduce(y, coef, nseg, part, nch, fused, dy_absmax=gmax)
    else:                                                   # as the model does: one launch per level, last level first
        for s in reversed(range(nseg)):
            ops.head_bn_bwd_reduce(y, coef, nseg, part, nch, fused, seg0=s, nsegs=1, dy_absmax=gmax)
    dgamma, dbeta = torch.zeros(F, device="cuda"), torch.zeros(F, device="cuda")
    ops.bn_bwd_finalize(y, coef, nseg, part, nch, dgamma, dbeta)
    dy = ops.head_bn_bwd_apply(y, coef, nseg, part, nch, fused, dy_absmax=gmax)
    torch.cuda.synchronize()
    per = -(-(B * H * W) // (nch // nseg))
    print(f"F={F} {H}x{W} nseg={nseg}: {nch // nseg} chunks of {per} pixels per segment")
    for name, got, want in (("dy", dy, dy_u), ("dgamma", dgamma, dgamma_u), ("dbeta", dbeta, dbeta_u)):
        print(f"  {name}: max |fused - unfused| {float((got - want).abs().max()):.3e} (max |unfused| {float(want.abs().max()):.3e})")
    print(f"  max|dy| fused {float(gmax.max()):.9e} unfused {float(gmax_u.max()):.9e}")
    assert torch.equal(dy, dy_u)
    assert torch.equal(dgamma, dgamma_u) and torch.equal(dbeta, dbeta_u)
    assert float(gmax.max()) == float(gmax_u.max()) == float(dy.abs().max())
    for s, (h, (dw_u, dbias_u, dgb_u)) in enumerate(zip(fused, un)):
        dw64, dbias64, dgb64 = _ref64(z[s * B:(s + 1) * B], h)
        _no_further(f"seg {s} dW", h["dw"], dw_u, dw64)
        _no_further(f"seg {s} dbias", h["dbias"], dbias_u, dbias64)
        if dgb64 is not None:
            _no_further(f"seg {s} dgb", h["dgb"], dgb_u, dgb64)


@pytest.mark.parametrize("name", list(CASES))
def test_streamed_first_pass_equals_the_unfused_composition(name):
    _run(CASES[name])
