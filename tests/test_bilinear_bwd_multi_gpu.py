"""hrseg_bilinear_bwd_multi (ops.bilinear_bwd_multi): the transpose of the bilinear resize of one gradient tensor onto up to
three targets in one launch -- the backward glue of the HRNet head at branch resolution.

Each target against hrseg_bilinear_bwd on the same dy: both kernels add the same n fp32 terms (wy * wx) * g per element, in
another order where the footprint rows are split over lanes.  Two orders of the same n fp32 terms differ by at most
2 * n * 2^-24 * A, A = the sum of the terms' magnitudes = hrseg_bilinear_bwd applied to |dy| (itself accurate to n * 2^-24
relative, absorbed by the factor 2) and n = the largest footprint count of the target (tests/head_branch_ref.py).

The adjoint identity <up(t), g> = <t, bwd(g)> in fp64 on the kernel's outputs, up() through the library's own fp32 weights:
every element of bwd(g) is within the bound above of the exact weighted sum, so the two sides differ by at most sum |t| * bound.

max|dt| per target, raised in the kernel, equals dt.abs().max() exactly (a maximum has no rounding), and two runs give the
same bits."""
import pytest
import torch

from tests.head_branch_ref import footprint_count, upsample_fp64

pytestmark = pytest.mark.gpu

B, H, W = 2, 9, 11
TARGETS = [(5, 6), (3, 3), (1, 2)]          # 1 x 2: a single row (scale 0 with align_corners: every output row reads it)
U = 2.0 ** -24


@pytest.mark.parametrize("align", [True, False], ids=["align", "noalign"])
@pytest.mark.parametrize("C", [8, 720])
def test_each_target_matches_the_single_target_kernel(C, align):
    from hrseg_amd import ops
    gen = torch.Generator(device="cuda").manual_seed(7 * C + int(align))
    dybuf = torch.randn((B, H, W, C + 8), generator=gen, device="cuda")
    dy = dybuf[..., 4:4 + C]                                             # a channel slice: row stride C + 8
    runs = [ops.bilinear_bwd_multi(dy, TARGETS, align, want_absmax=True) for _ in range(2)]
    torch.cuda.synchronize()
    dts, amax = runs[0]
    for j, (h, w) in enumerate(TARGETS):
        want = ops.bilinear_bwd(dy, (B, h, w, C), H, W, 0, 0, align)
        A = ops.bilinear_bwd(dy.abs(), (B, h, w, C), H, W, 0, 0, align)
        n = footprint_count(h, w, H, W, align)
        delta = (dts[j].double() - want.double()).abs()
        bound = 2 * n * U * A.double()
        print(f"C={C} align={align} target {h}x{w}: footprint {n}, max |delta| {float(delta.max()):.3e}, "
              f"max delta/bound {float((delta / bound.clamp_min(1e-300)).max()):.3f}")
        assert bool((delta <= bound).all())
        # adjoint identity in fp64
        t = torch.randn((B, h, w, C), generator=torch.Generator().manual_seed(j), dtype=torch.float64)
        lhs = float((upsample_fp64(t, H, W, align) * dy.double().cpu()).sum())
        rhs = float((t * dts[j].double().cpu()).sum())
        tol = float((t.abs() * bound.cpu()).sum())
        print(f"  <up(t), g> = {lhs:.9e}, <t, bwd(g)> = {rhs:.9e}, difference {abs(lhs - rhs):.3e} (tolerance {tol:.3e})")
        assert abs(lhs - rhs) <= tol
        assert float(amax[j].max()) == float(dts[j].abs().max())
        assert torch.equal(runs[1][0][j], dts[j])
    assert torch.equal(runs[1][1], amax)


def test_refusals_name_the_entry_point():
    from hrseg_amd import ops
    dy = torch.zeros((1, 4, 4, 8), device="cuda")
    with pytest.raises(RuntimeError, match="hrseg_bilinear_bwd_multi"):
        ops.bilinear_bwd_multi(dy, [(2, 2)] * 4)                         # four targets
    with pytest.raises(RuntimeError, match="hrseg_bilinear_bwd_multi"):
        ops.bilinear_bwd_multi(dy[..., :6], [(2, 2)])                    # 6 channels: not a multiple of 4
