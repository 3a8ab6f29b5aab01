"""The host model of the pre-split activation format (tests/split_ref.py) pinned on its own, without a GPU: the GPU tests
(tests/test_presplit_gpu.py) hold the BatchNorm writer to this model byte for byte, so the model must be right first."""
import math

import torch

from tests import split_ref as S

F16_MAX = 65504.0


def _inputs():
    """seeded fp32 values with |x| <= 65504: log-uniform magnitudes from 1e-6 up, unit normals, exact zeros, every fp16 value
    itself (hi = x, lo = 0) and the fp32 neighbours of fp16 values (where a wrong rounding direction shows)"""
    g = torch.Generator().manual_seed(20)
    mag = torch.exp(torch.empty(400_000).uniform_(math.log(1e-6), math.log(F16_MAX), generator=g))
    sign = torch.where(torch.rand(400_000, generator=g) < 0.5, -1.0, 1.0)
    grid = torch.arange(0, 0x7c00, dtype=torch.int32).to(torch.int16).view(torch.float16).float()      # every finite fp16 >= 0
    up = torch.nextafter(grid, torch.full_like(grid, float("inf")))
    down = torch.nextafter(grid, torch.full_like(grid, float("-inf")))
    x = torch.cat([mag * sign, torch.randn(200_000, generator=g), torch.zeros(16), grid, -grid, up, -up, down, -down])
    x = x[x.abs() <= F16_MAX]
    pad = (-x.numel()) % 4
    return torch.cat([x, torch.zeros(pad)]).reshape(-1, 4)


def test_hi_is_the_round_toward_zero_fp16():
    x = _inputs()
    hi, lo = S.split(x)
    assert hi.dtype == torch.float16 and lo.dtype == torch.float16
    h64, x64 = hi.double(), x.double()
    assert bool((h64.abs() <= x64.abs()).all()), "|hi| > |x|: not rounded toward zero"
    assert bool(((h64 == 0) | (torch.sign(h64) == torch.sign(x64))).all())
    assert bool((torch.signbit(hi.float()) == torch.signbit(x)).all()), "the sign bit of hi is the sign bit of x (-0.0 included)"
    # ... and the next fp16 of larger magnitude is already beyond x: hi is the LARGEST fp16 magnitude not above |x|
    nxt = (hi.view(torch.int16) + 1).view(torch.float16).double().abs()         # (65504 + one step = Inf)
    assert bool((nxt > x64.abs()).all())


def test_join_is_exact_and_within_the_bound():
    """join(pack(x)) = hi + lo without rounding, and |join - x| <= 2^-22 |x| + 2^-25.

    The bound, derived: hi keeps the leading 11 significand bits of x (or, below 2^-14, the multiples of 2^-24), so r = x - hi
    is exact in fp32 and |r| < ulp16(hi) = 2^(e-10) with 2^e <= |x|.  lo = RNE16(r).  If |r| >= 2^-14, lo is a normal fp16 and
    the rounding error is at most half an ulp of r's binade, 2^(E-11) with 2^E <= |r|, and E <= e - 11, i.e. at most
    2^(e-22) <= 2^-22 |x|.  If |r| < 2^-14, lo falls into the fp16 subnormals (spacing 2^-24) and the error is at most 2^-25
    whatever x is.  hi + lo spans at most 22 bits below hi's leading bit, so the fp32 sum is exact."""
    x = _inputs()
    hi, lo = S.split(x)
    packed = S.pack(x)
    assert packed.dtype == torch.int32 and packed.shape == x.shape
    j = S.join(packed)
    assert j.dtype == torch.float32
    assert torch.equal(j.double(), hi.double() + lo.double()), "hi + lo is not exact in fp32"
    err = (j.double() - x.double()).abs()
    bound = 2.0 ** -22 * x.double().abs() + 2.0 ** -25
    assert bool((err <= bound).all()), float((err - bound).max())
    # away from the subnormal pieces the relative term alone holds
    big = x.abs() >= 2.0 ** -3            # r's binade can still be below 2^-14 only when r rounds within 2^-25 <= 2^-22 |x|
    assert bool((err[big] <= 2.0 ** -22 * x.double().abs()[big]).all())


def test_pack_layout_and_round_trip():
    x = torch.tensor([[1.0, -2.0, 0.333251953125 + 2.0 ** -14, 1000.5, 3.0, 4.0, 5.0, 6.0]])
    hi, lo = S.split(x)
    p = S.pack(x)

    def u16(h):
        return int(h.view(torch.int16)) & 0xffff

    for q in range(2):
        want = [u16(hi[0, 4 * q]) | u16(hi[0, 4 * q + 1]) << 16, u16(hi[0, 4 * q + 2]) | u16(hi[0, 4 * q + 3]) << 16,
                u16(lo[0, 4 * q]) | u16(lo[0, 4 * q + 1]) << 16, u16(lo[0, 4 * q + 2]) | u16(lo[0, 4 * q + 3]) << 16]
        got = [int(v) & 0xffffffff for v in p[0, 4 * q:4 * q + 4]]
        assert got == want, (q, got, want)
    assert u16(hi[0, 0]) == 0x3c00 and u16(hi[0, 1]) == 0xc000 and u16(lo[0, 0]) == 0
    assert float(hi[0, 3]) == 1000.5 and float(lo[0, 3]) == 0.0            # 1000.5 is an fp16 value
    assert float(hi[0, 2]) == 0.333251953125 and float(lo[0, 2]) == 2.0 ** -14
    h2, l2 = S.unpack(p)
    assert torch.equal(h2.view(torch.int16), hi.view(torch.int16)) and torch.equal(l2.view(torch.int16), lo.view(torch.int16))
    assert torch.equal(S.as_f32_bytes(p).view(torch.int32), p)
    # N-d: the granule is over the last dimension only
    x4 = torch.randn(2, 3, 5, 8, generator=torch.Generator().manual_seed(1))
    assert torch.equal(S.pack(x4).reshape(-1, 8), S.pack(x4.reshape(-1, 8)))


def test_edge_values():
    inf, nan = float("inf"), float("nan")
    vals = [0.0, -0.0, 65504.0, 65519.9, 65520.0, 1e5, -1e5, 2.0 ** -14, 2.0 ** -24, 2.0 ** -25, 1e-40, inf, -inf, nan, 2e5, 65503.0]
    x = torch.tensor(vals, dtype=torch.float32)
    hi, lo = S.split(x)
    h, l = hi.tolist(), lo.tolist()
    hb = [int(v) & 0xffff for v in hi.view(torch.int16).tolist()]
    lb = [int(v) & 0xffff for v in lo.view(torch.int16).tolist()]
    assert hb[0] == 0x0000 and lb[0] == 0x0000
    assert hb[1] == 0x8000 and lb[1] == 0x0000              # -0.0 - (-0.0) = +0.0
    assert h[2] == 65504.0 and l[2] == 0.0
    assert h[3] == 65504.0 and l[3] == 15.8984375           # fp32(65519.9) = 65519.8984375: RNE16 stays at 65504
    assert h[4] == 65504.0 and l[4] == 16.0                 # RNE16(65520) is Inf: one step back
    assert h[5] == 65504.0 and l[5] == 34496.0 and h[6] == -65504.0 and l[6] == -34496.0
    assert h[7] == 2.0 ** -14 and l[7] == 0.0
    assert h[8] == 2.0 ** -24 and hb[8] == 0x0001 and l[8] == 0.0          # the smallest fp16 subnormal
    assert h[9] == 0.0 and l[9] == 0.0                      # 2^-25: hi truncates to 0, lo ties to even: the 2^-25 of the bound
    assert h[10] == 0.0 and l[10] == 0.0
    assert h[11] == inf and math.isnan(l[11]) and h[12] == -inf and math.isnan(l[12])      # Inf - Inf
    assert math.isnan(h[13]) and math.isnan(l[13])
    assert h[14] == 65504.0 and l[14] == inf                # beyond ~1.3e5 the low piece overflows: loud, as hrseg.h promises
    assert h[15] == 65472.0 and l[15] == 31.0
    j = S.join(S.pack(x.reshape(4, 4))).reshape(-1).tolist()
    assert j[5] == 1e5 and j[6] == -1e5 and j[3] == 65519.8984375 and j[4] == 65520.0
    assert math.isnan(j[11]) and math.isnan(j[12]) and math.isnan(j[13]) and j[14] == inf
    sub = S.subnormal(torch.tensor([0.0, -0.0, 2.0 ** -24, -(2.0 ** -15), 2.0 ** -14, 1.0, inf], dtype=torch.float16))
    assert sub.tolist() == [False, False, True, True, False, False, False]
