"""fp64 reference of the weight average FusedAdamW keeps (include/hrseg.h, "weight EMA"), and the cases of its tests.

    t = s - s0 - 1;  eff = warmup ? min(d, (1 + t) / (10 + t)) : d;  alpha = 1 - eff;  e = e + (p' - e) * alpha

p' = the parameter after the step's AdamW update, s = AdamW's step count after the step's tick, s0 = the count when
averaging began.  d enters as the fp32 value upcast: the reference computes on the number the kernel sees.

The bar for e is derived, not measured: 2^-20 * max(|e|, |p'|) per update against this reference evaluated on the kernel's own
p' and previous e (a single-step comparison, nothing accumulates).  With M = max(|e|, |p'|): p' - e contributes at most
2^-24 * 2M; alpha (division, min, subtraction) carries an absolute error of at most 3 * 2^-24, times |p' - e| <= 2M that is
6 * 2^-24 * M; the product 2 * 2^-24 * M; the final add 2^-24 * M: below 13 * 2^-24 * M < 2^-20 * M."""
import numpy as np
import torch

BAR = 2.0 ** -20

# tail and vector edges (1, 3: scalar tail alone; 4: one 16-byte group; 5, 1023: groups + tail; 1024: groups alone), and the size
# at which the cap of 8192 blocks x 256 threads x 4 elements makes threads take the grid-stride loop a second time, with a
# one-element tail
N_LARGE = 8192 * 256 * 4 + 5
SIZES = [1, 3, 4, 5, 1023, 1024, N_LARGE]
SIZE_IDS = [str(n) for n in SIZES[:-1]] + ["second_trip"]

# (1 + t) / (10 + t) crosses 0.5 at t = 8: both arms of the min are taken within 12 updates
WARMUP_CASE = dict(d=0.5, s0=5, steps=12)
WARMUP_EFF = [0.1, 2 / 11, 0.25, 4 / 13, 5 / 14, 0.4, 7 / 16, 8 / 17, 0.5, 0.5, 0.5, 0.5]


def f32(x):
    return float(np.float32(x))


def eff(d, warmup, s, s0):
    """effective decay of the update that follows AdamW's step number s (python floats are fp64)"""
    d = f32(d)
    t = float(s) - float(s0) - 1.0
    return min(d, (1.0 + t) / (10.0 + t)) if warmup else d


def alpha(d, warmup, s, s0):
    return 1.0 - eff(d, warmup, s, s0)


def update(e, p_new, d, warmup, s, s0):
    """-> the fp64 shadow after one update (any device)"""
    e64, p64 = e.detach().double(), p_new.detach().double()
    return e64 + (p64 - e64) * alpha(d, warmup, s, s0)


def bar_use(got, e_prev, p_new, d, warmup, s, s0):
    """largest |got - reference| / (max(|e_prev|, |p'|)) over the elements, as a fraction of BAR (<= 1 passes)"""
    want = update(e_prev, p_new, d, warmup, s, s0)
    scale = torch.maximum(e_prev.detach().double().abs(), p_new.detach().double().abs())
    err = (got.detach().double() - want).abs()
    # an element with e == p' == 0 has scale 0 and must be reproduced exactly
    frac = torch.where(scale > 0, err / (scale * BAR).clamp(min=1e-300), torch.where(err > 0, torch.full_like(err, np.inf), err))
    return float(frac.max())


def emacfg(d, warmup, s0, device="cpu"):
    return torch.tensor([d, float(bool(warmup)), float(s0)], dtype=torch.float32, device=device)


def inputs(n, seed=0):
    """random p, g, m, v (v >= 0) and a shadow that differs from p everywhere"""
    gen = torch.Generator().manual_seed(4200 + seed + n % 100003)
    p = torch.randn(n, generator=gen)
    g = 4.0 * torch.randn(n, generator=gen)
    m = 0.5 * torch.randn(n, generator=gen)
    v = torch.rand(n, generator=gen) + 1e-3
    e = p + 0.25 * torch.randn(n, generator=gen) + 0.5
    return dict(p=p, g=g, m=m, v=v, e=e)
