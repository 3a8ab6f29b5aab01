"""torch-CPU model of the PRE-SPLIT activation format (include/hrseg.h: hrseg_bn_fwd_t.z_split writes it,
hrseg_conv_shape_t.x_split / hrseg_bn_fwd_t.residual_split read it; csrc/sp_arith.h: hrseg_split_f16x2 / hrseg_join_f16x2).

One fp32 value x becomes two fp16 pieces:

  hi = x rounded TOWARD ZERO to fp16 (a finite |x| > 65504 saturates at +-65504; Inf stays Inf, NaN stays NaN);
  lo = (x - float(hi)) rounded to NEAREST-even fp16 (the difference itself is exact in fp32).

Four consecutive channels of a pixel (one 16-byte granule, the same bytes the fp32 values took) are stored as the dwords
{hi0 | hi1 << 16, hi2 | hi3 << 16, lo0 | lo1 << 16, lo2 | lo3 << 16}.  The value a reader multiplies is hi + lo, exact in fp32.

Nothing here shares code with the library: the round-toward-zero cast is derived from torch's round-to-nearest cast."""
import torch


def split(x):
    """fp32 tensor -> (hi, lo) fp16 tensors of the same shape"""
    x = x.detach().to(torch.float32).cpu().contiguous()
    near = x.to(torch.float16)                                   # round to nearest even; overflows to Inf from 65520 on
    # one step toward zero wherever rounding went away from it: fp16 is sign-magnitude, so the bit pattern less one is the next
    # value of smaller magnitude for either sign, and Inf (0x7c00) less one is 65504 (0x7bff).  (Inf > Inf and every comparison
    # with NaN are false: a true Inf and NaN keep their pattern.)
    away = near.float().abs() > x.abs()
    hi = (near.view(torch.int16) - away.to(torch.int16)).view(torch.float16)
    lo = (x - hi.float()).to(torch.float16)
    return hi, lo


def pack(x_nhwc):
    """fp32 [..., C] (C a multiple of 4) -> int32 [..., C]: the stored granules"""
    hi, lo = split(x_nhwc)
    shape = hi.shape
    assert shape[-1] % 4 == 0, "the format is defined per 4 channels"
    q = shape[:-1] + (shape[-1] // 4, 4)
    halves = torch.cat([hi.reshape(q), lo.reshape(q)], dim=-1).contiguous()        # [..., C/4, 8]: hi0..hi3, lo0..lo3
    return halves.view(torch.int16).view(torch.int32).reshape(shape)               # (little-endian: the even half is the low one)


def unpack(packed):
    """int32 [..., C] -> (hi, lo) fp16 [..., C]"""
    packed = packed.detach().cpu().contiguous()
    shape = packed.shape
    halves = packed.reshape(shape[:-1] + (shape[-1] // 4, 4)).view(torch.int16).view(torch.float16)     # [..., C/4, 8]
    return halves[..., :4].reshape(shape), halves[..., 4:].reshape(shape)


def join(packed):
    """int32 [..., C] -> fp32 [..., C]: hi + lo"""
    hi, lo = unpack(packed)
    return hi.float() + lo.float()


def subnormal(h):
    """mask of the NONZERO fp16 subnormals of an fp16 tensor"""
    bits = h.view(torch.int16).to(torch.int32) & 0x7fff
    return (bits > 0) & (bits < 0x0400)


def as_f32_bytes(packed):
    """the packed granules as the fp32-typed tensor the C ABI takes (same bytes; a copy moves them unchanged)"""
    return packed.contiguous().view(torch.float32)
