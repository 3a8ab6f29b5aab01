"""fp64 reference of FusedAdamW's gradient clipping and non-finite step skip (include/hrseg.h, 'gradient clipping'):

    S = sum (double)g_i^2      norm = |s| sqrt(S)      finite = isfinite(S) and isfinite(s)
    coef = min(1, max_norm / (norm + 1e-6))            (torch.nn.utils.clip_grad_norm_, norm_type 2)
    AdamW as tests/headloss_ref.adamw_step with the gradient g * s * coef; a step with skip set and finite == 0 is void:
    p, m, v and the step count stay, the skipped counter goes up by one.

g holds the fp32 values the kernels see; scalars the ABI carries as fp32 (grad_scale, max_norm -- and coef, which the
finalize kernel hands to the update kernel through an fp32 device word) are rounded to fp32 first, as headloss_ref does.
tests/test_gradclip_cpu.py pins this file against torch's own clip_grad_norm_ + AdamW; the GPU tests hold the kernels to it.
"""
import math

import torch

from tests import headloss_ref as R

f32 = R.f32


def verdict(g, gscale=1.0, max_norm=math.inf):
    """{"S", "norm", "coef" (fp64), "norm32", "coef32" (what the device stores), "finite"} of one flat gradient"""
    s = f32(gscale)
    S = float((g.detach().double().cpu() ** 2).sum())
    norm = abs(s) * math.sqrt(S) if not math.isnan(S) else math.nan
    finite = math.isfinite(S) and math.isfinite(s)
    q = f32(max_norm) / (norm + 1e-6)
    coef = 1.0 if q > 1.0 else q                       # clamp(max=1): a NaN quotient stays NaN, as in torch
    with_f32 = dict(norm32=f32(norm) if math.isfinite(norm) else norm, coef32=f32(coef) if math.isfinite(coef) else coef)
    return dict(S=S, norm=norm, coef=coef, finite=finite, **with_f32)


class Run:
    """p, m, v in `dtype` plus the counters of the device state; step() applies one gradient"""

    def __init__(self, p0, wd, dtype, gscale=R.ADAMW_GSCALE, beta1=R.ADAMW_BETA1, beta2=R.ADAMW_BETA2, eps=R.ADAMW_EPS):
        self.p = p0.to(dtype).clone()
        self.m, self.v = torch.zeros_like(self.p), torch.zeros_like(self.p)
        self.wd, self.gscale, self.betas, self.eps, self.dtype = f32(wd), f32(gscale), (beta1, beta2), eps, dtype
        self.steps = self.skipped = 0
        self.log = []

    def step(self, g, lr, max_norm=math.inf, skip=False):
        vd = verdict(g, self.gscale, max_norm)
        self.log.append(vd)
        if skip and not vd["finite"]:
            self.skipped += 1
            return vd
        self.steps += 1
        R.adamw_step(self.p, g.to(self.dtype) * vd["coef32"], self.m, self.v, self.steps, f32(lr), self.betas[0], self.betas[1],
                     self.eps, self.wd, self.gscale)
        return vd

    def state(self):
        """{step, 1 - beta1^step, 1 / sqrt(1 - beta2^step)} as the device holds it (all zero before the first step)"""
        return R.adamw_state(self.steps) if self.steps else [0.0, 0.0, 0.0]

    def tensors(self):
        return {"p": self.p, "m": self.m, "v": self.v}


def run(p0, grads, lrs, wd, dtype, max_norms=None, skip=False, gscale=R.ADAMW_GSCALE):
    r = Run(p0, wd, dtype, gscale)
    for k, (g, lr) in enumerate(zip(grads, lrs)):
        r.step(g, lr, math.inf if max_norms is None else max_norms[k], skip)
    return r
