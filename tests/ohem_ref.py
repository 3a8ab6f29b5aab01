"""Reference of online hard example mining (OHEM) on the fused cross-entropy (include/hrseg.h, hrseg_ohem_* and
hrseg_loss_*_ohem) in plain torch, any dtype, gradients from autograd, plus the case list that
tests/test_ohem_cpu.py and tests/test_ohem_gpu.py share.

Per level, z = logits [B,C,...], t = targets with -1 = ignored per channel, p = softmax(z) over all C channels:

  candidate   a pixel with at least one channel t != -1; its score q = sum over those channels of t_c p_c; the others carry -1
  lam_k       with N candidates in the WHOLE batch: the min(min_kept, N)-th smallest candidate score (torch.sort: NaN last) when
              min_kept >= 1 and N >= 1, else -1
  kept        candidate and (isnan(q) or q < thresh or q <= lam_k): ties at lam_k are all kept, a NaN score is always kept
  CE          tests/loss_options_ref.ce_dice with every class mask intersected with the kept set -- evaluated by handing it
              the targets with -1 written over the pixels that are not kept (imported, not copied); an item whose class mask
              is empty after the selection is the constant 1.0
  Dice        untouched: the same function on the unchanged targets
  gradient    the selection is a constant (computed from detached logits)

thresh reaches the kernels as fp32, so it is rounded to fp32 first, as the other options are.
"""
import torch

from tests import loss_options_ref as LR
from tests.headloss_ref import BAR_POINT, LOSS_B, LOSS_C, LOSS_PATTERNS, LOSS_UPSTREAM, _leaf, f32

__all__ = ["BAR_POINT", "LOSS_B", "LOSS_C", "LOSS_UPSTREAM"]

OHEM_HW = (1, 255, 256, 257, 5000)
OHEM_PATTERNS = LOSS_PATTERNS + (LR.SATURATED,)
OHEM_GAMMAS = (0.0, 2.0)
LOSS_BARS = LR.LOSS_BARS
# a keep decision may differ between two evaluations only where the fp64 score is this close to thresh or to lam_k, and at
# no more than MAX_FLIPS pixels of a case
BAND, MAX_FLIPS = 2e-5, 2


def ohem_pairs(hw):
    """the (thresh, min_kept) pairs of a case: threshold alone; threshold and rank; a rank beyond a low threshold; min_kept >= N
    (everything kept); rank alone; nothing kept"""
    return ((0.7, 0), (0.7, hw // 2), (0.05, hw), (0.9, 10 ** 9), (0.0, max(1, hw // 4)), (0.0, 0))


def cases(C):
    """every case of one channel count: (C, hw, B, pattern, (thresh, min_kept), gamma)"""
    return [(C, hw, B, pattern, pair, gamma) for hw in OHEM_HW for B in LOSS_B for pattern in OHEM_PATTERNS
            for pair in ohem_pairs(hw) for gamma in OHEM_GAMMAS]


def options(gamma):
    return (gamma,) + LR.DEFAULTS[1:]


def scores(z, t):
    """[B,C,...] -> q [B, pixels] in the dtype of z: sum of t_c p_c over the valid channels, -1 where there is none"""
    B, C = z.shape[:2]
    zf, tf = z.reshape(B, C, -1), t.reshape(B, C, -1).to(z.dtype)
    valid = tf != -1
    q = (torch.softmax(zf, dim=1) * tf).masked_fill(~valid, 0.0).sum(1)
    return torch.where(valid.any(1), q, torch.full_like(q, -1.0))


def select(q, thresh, min_kept, ranked=None):
    """q (any shape; -1 = not a candidate) -> (lam_k as a 0-dim tensor of q's dtype, N, keep mask of q's shape).  `ranked`: the
    sorted candidate scores, torch.sort(q[q != -1]).values, when the caller selects from one q many times."""
    thresh = f32(thresh)
    cand = q != -1                                    # (a NaN score is a candidate)
    if ranked is None:
        ranked = torch.sort(q[cand]).values           # NaN last
    n = ranked.numel()
    lam = torch.full((), -1.0, dtype=q.dtype)
    if min_kept >= 1 and n >= 1:
        lam = ranked[min(int(min_kept), n) - 1]
    keep = cand & (torch.isnan(q) | (q < thresh) | (q <= lam))
    return lam, n, keep


def ce_dice(z, t, w, opts, thresh, min_kept, keep=None):
    """-> (CE over the kept pixels, Dice or None, valid Dice items, keep [B, pixels], q, lam_k); `keep` given: that mask instead
    of the reference's own selection (the GPU test hands in the mask the kernels produced)"""
    B, C = z.shape[:2]
    with torch.no_grad():
        q = scores(z.detach(), t)
        lam, _, own = select(q, thresh, min_kept)
    if keep is None:
        keep = own
    tf = t.reshape(B, C, -1).to(z.dtype)
    t_kept = torch.where(keep.reshape(B, 1, -1), tf, torch.full_like(tf, -1.0)).reshape(t.shape)
    ce = LR.ce_dice(z, t_kept, w, opts)[0]
    _, dice, nvalid = LR.ce_dice(z, t.to(z.dtype), w, opts)
    return ce, dice, nvalid, keep, q, lam


def run(C, hw, B, pattern, pair, gamma, dtype, keep=None):
    """the shared case through the reference: values, valid-item count, d(0.7 CE + 1.3 Dice)/dz, and the selection"""
    x = LR.inputs(C, hw, B, pattern)
    z = _leaf(x["z"], dtype)
    ce, dice, nvalid, keep, q, lam = ce_dice(z, x["t"], x["w"], options(gamma), pair[0], pair[1], keep)
    loss = LOSS_UPSTREAM[0] * ce + (LOSS_UPSTREAM[1] * dice if dice is not None else 0.0)
    loss.backward()
    return {"ce": ce.detach(), "dice": dice.detach() if dice is not None else torch.zeros((), dtype=dtype), "nvalid": nvalid,
            "dz": z.grad if z.grad is not None else torch.zeros_like(z), "keep": keep, "q": q, "lam": lam}


def run_parts(C, hw, B, pattern, pair, gamma, dtype, keep=None):
    """dz of the CE term alone and of the Dice term alone (upstream 0.7 and 1.3 as in `run`)"""
    x = LR.inputs(C, hw, B, pattern)
    out = {}
    for name in ("ce", "dice"):
        z = _leaf(x["z"], dtype)
        ce, dice, _, _, _, _ = ce_dice(z, x["t"], x["w"], options(gamma), pair[0], pair[1], keep)
        term = LOSS_UPSTREAM[0] * ce if name == "ce" else (LOSS_UPSTREAM[1] * dice if dice is not None else None)
        if term is not None and term.requires_grad:
            term.backward()
        out[name] = z.grad if z.grad is not None else torch.zeros_like(z)
    return out


def flips(keep_a, q_a, lam_a, keep_ref, q_ref, lam_ref, thresh):
    """Where the keep mask of an fp32 evaluation `a` (CPU or GPU: its mask, scores, lam_k) differs from the fp64 reference's:
    -> (pixels outside the band, i.e. with |q_ref - thresh| and |q_ref - lam_ref| both above BAND; pixels that differ and are
    no exact tie; pixels that differ and ARE an exact tie, q_a == lam_a bit for bit).

    The tie count is reported apart and is not held to MAX_FLIPS: where fp32 underflows (the `saturated` pattern: a true-class
    probability below 1e-45 is exactly 0), scores that are distinct in fp64 become ONE fp32 value; when lam_k is that value
    the rule keeps all of them (ties at lam_k are kept, by design) while fp64 keeps min_kept of them.  Measured on the fp32 CPU
    evaluation of this file: up to 701 such pixels in one case (C=5, hw=5000, B=3, saturated, thresh 0, min_kept 1250), every one
    inside the band; on the six patterns without saturation the two evaluations agree at every pixel."""
    diff = keep_a.reshape(-1) != keep_ref.reshape(-1)
    qd = q_ref.reshape(-1).double()[diff]
    near = ((qd - f32(thresh)).abs() <= BAND) | ((qd - float(lam_ref)).abs() <= BAND)
    tie = q_a.reshape(-1)[diff] == lam_a
    return int((~near).sum()), int((~tie).sum()), int(tie.sum())


def flips_ok(outside, plain, ties):
    return outside == 0 and plain <= MAX_FLIPS
