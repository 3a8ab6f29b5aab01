"""Reference of the fused CE + Dice loss WITH its options -- focal exponent gamma on the CE, smoothing and Tversky weights
alpha / beta in the Dice term (include/hrseg.h, hrseg_loss_*_opt) -- in plain torch, any dtype, gradients from autograd, plus
the case list tests/test_loss_options_cpu.py and tests/test_loss_options_gpu.py share.

Per level, on the masked form of the reference project: valid pixels are t != -1, w the class weights.

  CE    per pixel -t (1-p)^gamma log p; mean over the valid pixels of (b, c), times w_c, summed over c, divided by C; an item with
        an empty class mask is the constant 1.0.  1 - p_c is exp(logsumexp of the OTHER channels - logsumexp of all): never a
        subtraction from 1, which is 0 in fp32 once a logit gap passes 17.  Its limit at 1-p -> 0 is 0, value and gradient:
        that covers C = 1 with gamma > 0, where there are no other channels.
  Dice  I, P, T = sum_c w_c sum (p t, p, t) over valid pixels; item = 1 - (2I + s) / (2(1-alpha-beta) I + 2 alpha P + 2 beta T + s);
        an item counts iff that denominator is not 0; the mean runs over the items that count (None when none does).

The shapes, ignore patterns, upstream gradients, bars and the seeded input maker are those of tests/headloss_ref.py (imported,
not copied); one pattern is added, `saturated`.  The options reach the kernels as fp32, so they are rounded to fp32 first.
"""
import torch
import torch.nn.functional as F

from tests.headloss_ref import (BAR_LOSS, BAR_REDUCED, LOSS_B, LOSS_C, LOSS_HW, LOSS_PATTERNS, LOSS_UPSTREAM, _gen, _leaf, f32,
                                loss_inputs)

__all__ = ["BAR_LOSS", "BAR_REDUCED", "LOSS_B", "LOSS_C", "LOSS_HW", "LOSS_PATTERNS", "LOSS_UPSTREAM"]

DEFAULTS = (0.0, 0.0, 0.5, 0.5)
# (gamma, smooth, alpha, beta)
OPTION_SETS = ((2.0, 0.0, 0.5, 0.5), (0.5, 1.0, 0.5, 0.5), (0.0, 1.0, 0.3, 0.7), (1.0, 0.0, 0.7, 0.3), DEFAULTS)
SATURATED = "saturated"
# logit gaps the saturated pattern must pass: beyond 17 fp32 rounds 1 - p to 0, beyond 104 the other exponentials are 0 in fp32
GAP_EPS, GAP_UNDERFLOW = 17.0, 104.0
SATURATED_SHARE = 0.3
SATURATED_SCALES = (10.0, 60.0)
SATURATED_SLACK = 4.0         # the kernel may be this many times the fp32 CPU evaluation's own dz error away from fp64
LOSS_BARS = {"ce": BAR_LOSS, "dice": BAR_LOSS, "dz": BAR_REDUCED}


def options_f32(options):
    return tuple(f32(v) for v in options)


def inputs(C, hw, B, pattern):
    """headloss_ref.loss_inputs; `saturated` = its random_ignore case with about 30 % of the pixels scaled by 10 or by 60
    (hw = 1 has nothing to scale)"""
    if pattern != SATURATED:
        return loss_inputs(C, hw, B, pattern)
    x = loss_inputs(C, hw, B, "random_ignore")
    g = _gen(C, hw, B, 77)
    u = torch.rand(B, 1, 1, hw, generator=g)
    scale = torch.ones(B, 1, 1, hw)
    scale[u < SATURATED_SHARE] = SATURATED_SCALES[0]
    scale[u < SATURATED_SHARE / 2] = SATURATED_SCALES[1]
    # every item keeps its first pixel unscaled: a Dice denominator that rests on underflowed probabilities alone (one
    # pixel, targets 0, the dominant channel ignored) is exactly 0 in fp32 and 1e-50 in fp64 -- whether that item counts is
    # then a property of the number format, not of the code under test
    scale[..., 0] = 1.0
    return dict(z=x["z"] * scale, t=x["t"], w=x["w"])


def one_minus_p(z):
    """[B,C,...] -> 1 - softmax(z) per channel, through logsumexp over the other channels: with L_c that logsumexp,
    1 - p_c = 1 / (1 + exp(z_c - L_c)) = exp(-softplus(z_c - L_c)).  (L_c - logsumexp of all is the same number, but where p_c
    is small it is the difference of two nearly equal ones, and autograd then sends two large cancelling gradients to the
    dominant channel: the fp32 evaluation lost a third of the dz bar to that at C=5, hw=256.)"""
    C = z.shape[1]
    if C == 1:
        return torch.zeros_like(z)
    eye = torch.eye(C, dtype=torch.bool, device=z.device).reshape((1, C, C) + (1,) * (z.dim() - 2))
    others = z.unsqueeze(1).expand(z.shape[0], C, *z.shape[1:]).masked_fill(eye, float("-inf"))
    return torch.exp(-F.softplus(z - torch.logsumexp(others, dim=2), threshold=40.0))     # (beyond 40: x itself, exact in fp64)


def ce_dice(z, t, w, options=DEFAULTS):
    """-> (CE, Dice or None, number of valid Dice items) in the dtype of z"""
    gamma, smooth, alpha, beta = options_f32(options)
    B, C = z.shape[:2]
    zf, tf = z.reshape(B, C, -1), t.reshape(B, C, -1)
    m = (tf != -1).to(z.dtype)
    wt = torch.tensor(w, dtype=torch.float32).to(z.dtype)
    logp, p = F.log_softmax(zf, dim=1), torch.softmax(zf, dim=1)
    term = tf * logp
    if gamma > 0:
        om = one_minus_p(zf)
        # (1-p)^gamma with its limit 0 at 1-p = 0 for value and gradient (pow's own gradient there is inf or nan for gamma < 1)
        safe = torch.where(om > 0, om, torch.ones_like(om))
        term = term * torch.where(om > 0, safe ** gamma, torch.zeros_like(om))
    n = m.sum(-1)
    s = (term * m).sum(-1)
    valid = (n > 0).all(1)
    item = (-(wt[None, :] * s) / torch.where(n > 0, n, torch.ones_like(n))).sum(1) / C
    ce = torch.where(valid, item, torch.ones_like(item)).mean()
    inter = (wt[None, :] * (p * tf * m).sum(-1)).sum(1)
    psum = (wt[None, :] * (p * m).sum(-1)).sum(1)
    tsum = (wt[None, :] * (tf * m).sum(-1)).sum(1)
    num = 2.0 * inter + smooth
    den = 2.0 * (1.0 - alpha - beta) * inter + 2.0 * alpha * psum + 2.0 * beta * tsum + smooth
    keep = den != 0
    nvalid = int(keep.sum())
    if nvalid == 0:
        return ce, None, 0
    dice = (1.0 - num / torch.where(keep, den, torch.ones_like(den)))[keep].mean()
    return ce, dice, nvalid


def run(C, hw, B, pattern, options, dtype):
    """the shared case through the reference: values, valid-item count and d(0.7 CE + 1.3 Dice)/dz"""
    x = inputs(C, hw, B, pattern)
    z = _leaf(x["z"], dtype)
    ce, dice, nvalid = ce_dice(z, x["t"].to(dtype), x["w"], options)
    loss = LOSS_UPSTREAM[0] * ce + (LOSS_UPSTREAM[1] * dice if dice is not None else 0.0)
    loss.backward()
    return {"ce": ce.detach(), "dice": dice.detach() if dice is not None else torch.zeros((), dtype=dtype),
            "nvalid": nvalid, "dz": z.grad if z.grad is not None else torch.zeros_like(z)}


def max_gaps(z):
    """per pixel: the largest logit minus the smallest"""
    return (z.max(dim=1).values - z.min(dim=1).values).reshape(-1)
