"""Class-weighted CE + soft-Dice + hierarchy-consistency losses on the GPU.

Call surface of the reference's Metrics/losses.py: ``CrossEntropyLoss(smooth)``,
``SoftDiceLoss(smooth, num_classes)`` called as ``loss(outs, targets,
logits_input=False, class_weight=None)`` and ``hierarchical_consistency_loss(
probs_per_level, levels, parent_of, reduction='mean')``.

One fused HIP pass over (logits, targets) (hrseg_loss_partials) produces the five
masked per-(b,c) sums both losses need; the reference walks B*C boolean-mask
gathers per loss (losses.py:52-59, :100-114), each a device->host sync.  The
gradient is one more pass (hrseg_loss_bwd).  Semantics kept: mask = target != -1,
CE item -> constant 1.0 when any class mask of the item is empty (:116), Dice
items with 0/0 dropped (:64), Dice -> None when no item survives (:66), Dice's
``smooth`` in numerator and denominator (:40).  Beyond the reference: a focal
exponent on the CE and Tversky weights in the Dice denominator (LossOptions); the
defaults are the reference's losses, bit for bit what they were without options.
Online hard example mining on the CE term (OhemOptions):
``CrossEntropyLoss(ohem_thresh=0.7, ohem_min_kept=100000)`` averages the CE over the
pixels of the level's batch whose true-class probability is below the threshold, and
over at least the ``ohem_min_kept`` hardest ones; the Dice term is untouched.
Border weights on the CE term (Metrics/border.py): ``CrossEntropyLoss(border=BorderWeights(w0, sigma))``
weighs every pixel's CE by 1 + w0 exp(-d^2 / (2 sigma^2)), d = its distance to the nearest border of the level's label map;
``fused_ce_dice(pixel_weight=)`` takes any per-pixel map.  The Dice term is untouched.
"""
from __future__ import annotations

import math
from typing import NamedTuple

import torch
import torch.nn as nn

from .. import ops
from .border import BorderOptions, BorderWeights  # noqa: F401  (re-exported)

_weight_cache = {}


def _weights(class_weight, device):
    if class_weight is None:
        # the reference fails here too (losses.py:56-59 / :103-112)
        raise TypeError("class_weight is required: the reference losses index it per class")
    key = (tuple(float(v) for v in class_weight), str(device))
    w = _weight_cache.get(key)
    if w is None:
        w = torch.tensor(key[0], dtype=torch.float32, device=device)
        _weight_cache[key] = w
    return w


def _option(name, value):
    """a loss option as a float: finite and >= 0, or ValueError"""
    v = float(value)
    if not (math.isfinite(v) and v >= 0.0):
        raise ValueError(f"{name} must be finite and >= 0, got {value!r}")
    return v


class LossOptions(NamedTuple):
    """What the fused loss kernels take by value besides the class weights (hrseg_loss_*_opt): the focal exponent of the CE
    term, -t (1-p)^gamma log p, and the Dice term's smoothing and Tversky weights,
    1 - (2I + smooth) / (2(1-alpha-beta) I + 2 alpha P + 2 beta T + smooth).  The defaults are the reference's losses."""
    gamma: float = 0.0
    smooth: float = 0.0
    alpha: float = 0.5
    beta: float = 0.5

    @classmethod
    def from_pair(cls, ce_fn=None, dice_fn=None):
        """the options of a (CrossEntropyLoss, SoftDiceLoss) pair; None = that loss at its defaults"""
        gamma = 0.0 if ce_fn is None else _option("focal_gamma", ce_fn.focal_gamma)
        if dice_fn is None:
            return cls(gamma=gamma)
        return cls(gamma, _option("smooth", dice_fn.smooth), _option("alpha", dice_fn.alpha), _option("beta", dice_fn.beta))

    def or_none(self):
        """None at the defaults -- ops.loss_fwd / loss_bwd then make the calls without options -- else the tuple"""
        return None if self == LossOptions() else self


def _ohem_thresh(value):
    """ohem_thresh as a float: finite and in [0, 1], or ValueError"""
    v = float(value)
    if not (math.isfinite(v) and 0.0 <= v <= 1.0):
        raise ValueError(f"ohem_thresh must be a finite number in [0, 1], got {value!r}")
    return v


def _ohem_min_kept(value):
    """ohem_min_kept as an int >= 0, or ValueError (a float is accepted only when it is a whole number)"""
    if isinstance(value, bool) or not isinstance(value, (int, float)) or (isinstance(value, float) and not math.isfinite(value)) \
            or int(value) != value or value < 0:
        raise ValueError(f"ohem_min_kept must be an integer >= 0, got {value!r}")
    return int(value)


class OhemOptions(NamedTuple):
    """Online hard example mining on the CE term of one level, by value into the recorded calls (hrseg_ohem_select,
    hrseg_loss_*_ohem): with q = the softmax probability of the true class among the valid channels of a pixel, the CE runs over
    the pixels with q < thresh, and over the min_kept hardest (smallest q) of the level's whole batch at least; ties at the
    min_kept-th score and NaN scores are kept.  Travels beside LossOptions, which stays the four-field tuple it is."""
    thresh: float
    min_kept: int = 0

    @classmethod
    def from_ce(cls, ce_fn=None):
        """the OHEM options of a CrossEntropyLoss; None = off (no loss object, or ohem_thresh=None)"""
        if ce_fn is None or getattr(ce_fn, "ohem_thresh", None) is None:
            return None
        return cls(_ohem_thresh(ce_fn.ohem_thresh), _ohem_min_kept(ce_fn.ohem_min_kept))


class _FusedLoss(torch.autograd.Function):
    """(logits, targets, w, options, ohem, record_to, pixel_weight) -> [ce, dice, n_valid_dice_items]"""

    @staticmethod
    def forward(ctx, z, t, w, options, ohem, record_to, pixel_weight=None):
        z = z.contiguous()
        t = t.contiguous()
        ctx.options = options
        ctx.ohem = None
        ctx.pixel_weight = pixel_weight         # a constant of the step: no gradient flows to it
        if pixel_weight is not None:
            out, coef = ops.loss_fwd(z, t, w, options, pixel_weight=pixel_weight)
        elif ohem is None:
            out, coef = ops.loss_fwd(z, t, w, options)
        else:
            out, coef, ctx.ohem = ops.loss_fwd(z, t, w, options, ohem=ohem)
            if record_to is not None:
                record_to.last_ohem = ctx.ohem.record
        ctx.save_for_backward(z, t, coef)
        return out

    @staticmethod
    def backward(ctx, g):
        z, t, coef = ctx.saved_tensors
        if ctx.pixel_weight is not None:
            dz = ops.loss_bwd(z, t, coef, g.contiguous(), options=ctx.options, pixel_weight=ctx.pixel_weight)
        else:
            dz = ops.loss_bwd(z, t, coef, g.contiguous(), options=ctx.options, ohem=ctx.ohem)
        return dz, None, None, None, None, None, None


def _pixel_weight(pixel_weight, logits):
    """pixel_weight as a contiguous [B,H,W] fp32 tensor on the logits' device, or ValueError"""
    B, _, H, W = logits.shape
    if not isinstance(pixel_weight, torch.Tensor) or tuple(pixel_weight.shape) not in ((B, H, W), (B, 1, H, W)):
        raise ValueError(f"pixel_weight must be a [B,H,W] or [B,1,H,W] tensor matching the logits ({B}, {H}, {W}), got "
                         f"{tuple(pixel_weight.shape) if isinstance(pixel_weight, torch.Tensor) else type(pixel_weight).__name__}")
    if pixel_weight.dtype != torch.float32:
        raise ValueError(f"pixel_weight must be float32, got {pixel_weight.dtype}")
    if pixel_weight.device != logits.device:
        raise ValueError(f"pixel_weight is on {pixel_weight.device}, the logits are on {logits.device}")
    return pixel_weight.detach().reshape(B, H, W).contiguous()


def fused_ce_dice(logits, targets, class_weight, options=None, ohem=None, record_to=None, pixel_weight=None):
    """-> tensor [3] = (CE, Dice, number of valid Dice items); differentiable w.r.t. logits.  `options`: a LossOptions
    (None = the defaults).  `ohem`: an OhemOptions / (thresh, min_kept) pair, None = off; the selection's device record
    (int32[4]: lam_k as fp32 bits, n_candidates, n_kept, reserved) is left in `record_to.last_ohem` when an object is given.
    `pixel_weight`: [B,H,W] or [B,1,H,W] fp32 on the logits' device, one weight per pixel on the CE term (finite and >= 0 is
    the caller's duty; no gradient flows to it); not together with `ohem`."""
    if logits.shape[1] != len(class_weight):
        raise ValueError(f"class_weight has {len(class_weight)} entries, logits have {logits.shape[1]} channels")
    if pixel_weight is not None and ohem is not None:
        raise ValueError("pixel_weight and ohem are not combined: pass one of them")
    options = None if options is None else LossOptions(*options).or_none()
    if ohem is not None:
        ohem = OhemOptions(_ohem_thresh(ohem[0]), _ohem_min_kept(ohem[1]))
    w = _weights(class_weight, logits.device)
    if pixel_weight is None:
        return _FusedLoss.apply(logits, targets, w, options, ohem, record_to)
    return _FusedLoss.apply(logits, targets, w, options, None, record_to, _pixel_weight(pixel_weight, logits))


def global_batch_dice(res, group=None):
    """Dice term of one level under data parallelism.  The reference computes Dice on the batch gathered on one GPU:
    mean over the items whose Dice is not 0/0 (losses.py:64-66), so the divisor is the GLOBAL number of valid items.
    A rank-local mean divides by the rank's own count, which differs from rank to rank as soon as one shard holds a
    sample with no valid pixel at this level.  With n_r = this rank's count and n = sum over ranks (ONE all-reduce of
    one float per level, stream-ordered, no host sync) the rank's term becomes

        dice_r * n_r * world / n      (0 when n == 0)

    whose average over the ranks -- what GradSync's summed gradient times AdamW's 1/world evaluates -- is
    sum_b dice_b / n: exactly the gathered-batch Dice and its gradient.  `res` = fused_ce_dice(...)."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
        return res[1]
    n_local = res[2].detach()
    n = n_local.clone().reshape(1)
    dist.all_reduce(n, op=dist.ReduceOp.SUM, group=group)
    world = float(dist.get_world_size(group))
    scale = torch.where(n > 0, n_local.reshape(1) * world / n.clamp(min=1.0), torch.zeros_like(n))
    return res[1] * scale.reshape(())


def _as_logits(outs, logits_input, log_domain):
    """The kernels take logits.  Already-normalised inputs are mapped back:
    log-probabilities are their own logits; probabilities go through log()."""
    if logits_input or log_domain:
        return outs
    return torch.log(outs)


class CrossEntropyLoss(nn.Module):
    """Masked class-weighted CE; ``focal_gamma`` > 0 multiplies each pixel's term by (1 - p)^gamma (focal loss), 0 is the
    reference's CE.  ``smooth`` is stored and never used, as in the reference (its CE has no smoothing term either).
    ``ohem_thresh`` (None = off) switches online hard example mining on: the CE then runs over the pixels of the level's batch
    whose true-class probability is below it, and over the ``ohem_min_kept`` hardest at least (OhemOptions).  ``last_ohem`` is
    the device record of the latest selection (int32[4]: lam_k as fp32 bits, n_candidates, n_kept, reserved; None before the
    first), written without a sync: ``kept_fraction()`` reads it.
    ``border`` (a BorderWeights, None = off) weighs every pixel's CE by the border weight map of the level's targets, computed
    per call on the device; ``last_border`` is the latest map ([B,H,W], None before the first).  Not together with
    ``ohem_thresh``."""

    def __init__(self, smooth=0.0, focal_gamma=0.0, ohem_thresh=None, ohem_min_kept=0, border=None):
        super().__init__()
        self.smooth = smooth
        self.focal_gamma = _option("focal_gamma", focal_gamma)
        self.ohem_thresh = None if ohem_thresh is None else _ohem_thresh(ohem_thresh)
        self.ohem_min_kept = _ohem_min_kept(ohem_min_kept)
        self.last_ohem = None
        if border is not None and not isinstance(border, BorderWeights):
            raise ValueError(f"border must be a BorderWeights or None, got {type(border).__name__}")
        if border is not None and self.ohem_thresh is not None:
            raise ValueError("CrossEntropyLoss: ohem_thresh and border are not combined: pass one of them")
        self.border = border
        self.last_border = None

    def border_map(self, targets):
        """the level's border weight map (None when the option is off), kept in ``last_border``"""
        if self.border is None:
            return None
        self.last_border = self.border(targets)
        return self.last_border

    def kept_fraction(self):
        """n_kept / n_candidates of the latest selection (a host read: for logging), None when there is none"""
        if self.last_ohem is None:
            return None
        _, n, kept, _ = self.last_ohem.tolist()
        return kept / n if n else 0.0

    def forward(self, outs, targets, logits_input=False, class_weight=None):
        return fused_ce_dice(_as_logits(outs, logits_input, True), targets, class_weight, LossOptions.from_pair(self, None),
                             ohem=OhemOptions.from_ce(self), record_to=self, pixel_weight=self.border_map(targets))[0]


class SoftDiceLoss(nn.Module):
    """Masked class-weighted soft Dice per item, (2I + smooth) / (U + smooth) as the reference computes it (losses.py:40):
    with smooth > 0 no item is 0/0, so every item counts.  ``alpha`` / ``beta`` weigh the false positives / false negatives
    in the denominator (Tversky); 0.5 / 0.5 is Dice."""

    def __init__(self, smooth=0, num_classes=3, alpha=0.5, beta=0.5):
        super().__init__()
        self.smooth = _option("smooth", smooth)
        self.alpha = _option("alpha", alpha)
        self.beta = _option("beta", beta)

    def forward(self, outs, targets, logits_input=False, class_weight=None):
        res = fused_ce_dice(_as_logits(outs, logits_input, False), targets, class_weight, LossOptions.from_pair(None, self))
        if float(res[2]) == 0.0:          # every item was 0/0: the reference returns None
            return None
        return res[1]


def _level_groups(levels, parent_of, L):
    """[(parent channel at L-1, [child channels at L])] for parents that have children at L"""
    out = []
    for p_idx, p_name in enumerate(levels[L - 1]):
        ch = [i for i, c in enumerate(levels[L]) if parent_of.get(c, None) == p_name]
        if ch:
            out.append((p_idx, ch))
    return out


class _LevelConsistency(torch.autograd.Function):
    """sum over the level's parent groups of (mean or sum over b,h,w of) |sum_children P - P_parent|"""

    @staticmethod
    def forward(ctx, cur, prev, gp, gs, scale):
        cur, prev = cur.contiguous(), prev.contiguous()
        sums = ops.consistency_sums(cur, prev, gp, gs)
        ctx.save_for_backward(cur, prev)
        ctx.meta = (gp, gs, scale)
        return (sums.sum() * scale).float()

    @staticmethod
    def backward(ctx, g):
        cur, prev = ctx.saved_tensors
        gp, gs, scale = ctx.meta
        dcur, dprev = ops.consistency_bwd(cur, prev, g.reshape(1).float().contiguous(), scale, gp, gs)
        return dcur, dprev, None, None, None


def hierarchical_consistency_loss(probs_per_level, levels, parent_of, reduction="mean"):
    """mean_{b,h,w} |sum_children P_c - P_p| averaged over parents (losses.py:150-177), forward and
    gradient on the GPU (hrseg_consistency, hrseg_consistency_bwd).  In the training loop the inputs
    are one-hot predictions without gradient; probabilities that require grad get theirs."""
    if probs_per_level is None or levels is None or parent_of is None:
        return probs_per_level[0].sum() * 0 if probs_per_level else 0.0
    total, count = None, 0
    for L in range(1, len(levels)):
        groups = _level_groups(levels, parent_of, L)
        if not groups:
            continue
        prev, cur = probs_per_level[L - 1], probs_per_level[L]
        contiguous = all(ch == list(range(ch[0], ch[0] + len(ch))) for _, ch in groups) and \
            [c for _, ch in groups for c in ch] == list(range(cur.shape[1]))
        if not contiguous:
            raise NotImplementedError("children of a parent must occupy consecutive channels (BFS channel order)")
        n = cur.shape[0] * cur.shape[2] * cur.shape[3]
        scale = 1.0 / n if reduction == "mean" else 1.0
        part = _LevelConsistency.apply(cur, prev, [p for p, _ in groups], [len(ch) for _, ch in groups], scale)
        total = part if total is None else total + part
        count += len(groups)
    if count == 0:
        return probs_per_level[0].sum() * 0
    return total / count


class _GroupKL(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, pprev, gp, gs):
        z, pprev = z.contiguous(), pprev.contiguous()
        sums = ops.group_kl_sums(z, pprev, gp, gs)
        n = z.shape[0] * z.shape[2] * z.shape[3]
        sizes = torch.tensor([float(v) for v in gs], dtype=torch.float64, device=z.device)
        ctx.save_for_backward(z, pprev)
        ctx.meta = (gp, gs, 1.0 / (n * len(gs)))
        return ((sums / sizes).sum() / (n * len(gs))).float()

    @staticmethod
    def backward(ctx, g):
        z, pprev = ctx.saved_tensors
        gp, gs, scale = ctx.meta
        return ops.group_kl_bwd(z, pprev, g.reshape(1).float().contiguous(), scale, gp, gs), None, None, None


def grouped_conditional_kl(z_children_all, probs_prev_level, groups, levels_prev):
    """The optional stabiliser the reference ships commented out (Metrics/losses.py:180-210), same signature: per parent
    group KL(Q_{c|p} || Uniform) with Q = softmax(z_g + log(P_p + 1e-6)).clamp_min(1e-8), `.mean()` per group, averaged
    over the groups that have children.  One fused HIP pass forward (hrseg_group_kl), one for the gradient w.r.t. the
    logits (hrseg_group_kl_bwd; the parent probabilities get none: the log-bias is constant inside a group).
    groups: [(parent_name, [child names])] of this level; levels_prev: parent names in channel order.  Opt-in:
    train.get_loss adds `lambda_kl` times it per level only when asked to."""
    if z_children_all is None or probs_prev_level is None or groups is None:
        return z_children_all.sum() * 0
    live = [(levels_prev.index(p), len(ch)) for p, ch in groups if len(ch) > 0]
    if not live:
        return z_children_all.sum() * 0
    if sum(g for _, g in live) != z_children_all.shape[1]:
        raise ValueError("group sizes do not add up to the level's channels")
    return _GroupKL.apply(z_children_all, probs_prev_level, [p for p, _ in live], [g for _, g in live])


class _TreeKL(torch.autograd.Function):
    """(student logits, teacher logits, parent probabilities or None, pixel weights or None, ...) -> scale * sum_g out[g][0] of one
    level (hrseg_tree_kl), differentiable w.r.t. the student logits only (hrseg_tree_kl_bwd)"""

    @staticmethod
    def forward(ctx, z, u, wprev, pw, inv_temp, thresh, gp, gs, scale, records):
        z = z.contiguous()
        out = ops.tree_kl_fwd(z, u, wprev, pw, inv_temp, thresh, gp, gs)
        if records is not None:
            records.append(out)
        ctx.save_for_backward(z, u)
        ctx.meta = (wprev, pw, inv_temp, thresh, gp, gs, scale)      # constants of the step: no gradient flows to them
        return (out[:, 0].sum() * scale).float()

    @staticmethod
    def backward(ctx, g):
        z, u = ctx.saved_tensors
        wprev, pw, inv_temp, thresh, gp, gs, scale = ctx.meta
        dz = ops.tree_kl_bwd(z, u, wprev, pw, inv_temp, thresh, g.reshape(1).float().contiguous(), scale, gp, gs)
        return (dz,) + (None,) * 9


def _per_level(name, value, n, check):
    """a scalar or one value per level -> a list of n checked floats"""
    vals = [value] * n if isinstance(value, (int, float)) else list(value)
    if len(vals) != n:
        raise ValueError(f"{name} has {len(vals)} entries, the tree has {n} levels")
    return [check(name, v) for v in vals]


def _temperature(name, v):
    v = float(v)
    if not (math.isfinite(v) and v > 0.0 and math.isfinite(1.0 / v)):
        raise ValueError(f"{name} must be finite and > 0, got {v!r}")
    return v


def _unit_interval(name, v):
    v = float(v)
    if not 0.0 <= v <= 1.0:
        raise ValueError(f"{name} must be in [0, 1], got {v!r}")
    return v


class TreeDistillation(nn.Module):
    """Tree distillation (include/hrseg.h, "tree distillation"): per level and sibling group the KL between
    the teacher's and the student's conditional distribution over the children at temperature T, weighted by the teacher's
    composed probability of the parent (``restrictive=True``; the soft form of the restrictive -1 mask, and with it the levels
    add up to the KL between the two composed leaf distributions) and kept only where the teacher's confidence
    omega / sum_c exp(u_c - max u) -- the hedged decode's T_L -- reaches ``thresh`` (the FixMatch threshold; 0 = no gate).

        forward(student_logits, teacher_logits, teacher_probs=None, pixel_weight=None)
            = sum_L level_weight_L * T_L^2 / (B*H*W) * sum_g out_L[g][0]          (a 0-dim tensor)

    One hrseg_tree_kl launch per level forward and one hrseg_tree_kl_bwd backward: the divisor and T^2 travel in the backward's
    ``scale``, so there is no finalize launch.  Differentiable w.r.t. the student logits only.

    ``groups``: per level a (group_parent, group_size) pair, or None = one group of all the level's channels (level 0, flat
    models); a level whose pair is empty is skipped.  ``for_model`` takes them from a model.  ``temperature`` and ``thresh``:
    scalars or one value per level.  ``restrictive=True`` needs ``teacher_probs``, the probabilities the teacher's forward returns
    beside its logits: level L >= 1 is weighted by ``teacher_probs[L-1]``.  ``last_records``: the per-level ``out`` tensors
    ([ngroups,3] float64, on the device; None for a skipped level) of the latest call; ``kept_fraction()`` reads them."""

    def __init__(self, temperature=1.0, thresh=0.0, restrictive=True, level_weights=None, groups=(None,)):
        super().__init__()
        self.groups = []
        for L, g in enumerate(groups):
            if g is not None:
                gp, gs = [int(v) for v in g[0]], [int(v) for v in g[1]]
                if len(gp) != len(gs) or any(v < 1 for v in gs) or any(v < 0 for v in gp) or sum(gs) > 16:
                    raise ValueError(f"level {L}: bad group table {g!r}")
                g = (gp, gs)
            self.groups.append(g)
        n = len(self.groups)
        if n < 1:
            raise ValueError("TreeDistillation needs at least one level")
        self.temperature = _per_level("temperature", temperature, n, _temperature)
        self.thresh = _per_level("thresh", thresh, n, _unit_interval)
        self.restrictive = bool(restrictive)
        self.level_weights = [1.0] * n if level_weights is None else _per_level("level_weights", level_weights, n, _option)
        self.last_records = None

    @classmethod
    def for_model(cls, model, temperature=1.0, thresh=0.0, restrictive=True, level_weights=None):
        """the groups of ``model.levels`` / ``model.child_groups``: level 0 is one group of its channels, level L >= 1 one group
        per parent that has children.  A flat model (no ``levels``) gets one level with one group."""
        groups = [None]
        if hasattr(model, "levels") and hasattr(model, "child_groups"):
            for L in range(1, len(model.levels)):
                live = [(model.levels[L - 1].index(p), len(ch)) for p, ch in model.child_groups[L - 1] if len(ch) > 0]
                groups.append(([p for p, _ in live], [n for _, n in live]))
        return cls(temperature, thresh, restrictive, level_weights, groups=groups)

    def kept_fraction(self):
        """kept (pixel, group) pairs over all pairs of the latest call, per level (None: skipped level, or no call yet).  The
        one host read: for logging."""
        if self.last_records is None:
            return None
        return [None if r is None else float(r[:, 2].sum().item()) / float(n) for r, n in zip(self.last_records, self._pairs)]

    def forward(self, student_logits, teacher_logits, teacher_probs=None, pixel_weight=None):
        if isinstance(student_logits, torch.Tensor):
            student_logits = [student_logits]
        if isinstance(teacher_logits, torch.Tensor):
            teacher_logits = [teacher_logits]
        if isinstance(teacher_probs, torch.Tensor):
            teacher_probs = [teacher_probs]
        n = len(self.groups)
        if len(student_logits) != n or len(teacher_logits) != n:
            raise ValueError(f"TreeDistillation has {n} levels, got {len(student_logits)} student and {len(teacher_logits)} "
                             "teacher logit tensors")
        if self.restrictive and n > 1 and (teacher_probs is None or len(teacher_probs) < n - 1):
            raise ValueError("restrictive=True needs teacher_probs, the probabilities the teacher's forward returns beside its logits")
        z0 = student_logits[0]
        pw = None if pixel_weight is None else _pixel_weight(pixel_weight, z0)
        records, pairs, total = [], [], None
        for L in range(n):
            z, u = student_logits[L], teacher_logits[L]
            if not isinstance(z, torch.Tensor) or not isinstance(u, torch.Tensor) or z.dim() != 4 or u.shape != z.shape:
                raise ValueError(f"level {L}: student and teacher logits must be [B,C,H,W] tensors of one shape")
            if z.shape[0] != z0.shape[0] or z.shape[2:] != z0.shape[2:]:
                raise ValueError(f"level {L}: logits are {tuple(z.shape)}, level 0 has {tuple(z0.shape)}")
            if z.dtype != torch.float32 or u.dtype != torch.float32:
                raise ValueError(f"level {L}: logits must be float32, got {z.dtype} and {u.dtype}")
            if u.device != z.device or not z.is_cuda:
                raise ValueError(f"level {L}: student logits are on {z.device}, teacher logits on {u.device}; both must be on one GPU")
            gp, gs = ([0], [z.shape[1]]) if self.groups[L] is None else self.groups[L]
            if not gs:
                records.append(None)
                pairs.append(0)
                continue
            if sum(gs) != z.shape[1]:
                raise ValueError(f"level {L}: group sizes {gs} do not add up to the logits' {z.shape[1]} channels")
            wprev = None
            if self.restrictive and L > 0:
                wprev = teacher_probs[L - 1]
                if not isinstance(wprev, torch.Tensor) or wprev.dim() != 4 or wprev.shape[0] != z.shape[0] or \
                        wprev.shape[2:] != z.shape[2:] or wprev.shape[1] <= max(gp):
                    raise ValueError(f"level {L}: teacher_probs[{L - 1}] must be [B,Cprev,H,W] with Cprev > {max(gp)} matching the logits")
                if wprev.dtype != torch.float32 or wprev.device != z.device:
                    raise ValueError(f"level {L}: teacher_probs[{L - 1}] must be float32 on the logits' device")
                wprev = wprev.detach().contiguous()
            T = self.temperature[L]
            npix = z.shape[0] * z.shape[2] * z.shape[3]
            lvl = []
            part = _TreeKL.apply(z, u.detach().contiguous(), wprev, pw, 1.0 / T, self.thresh[L], gp, gs,
                                 self.level_weights[L] * T * T / npix, lvl)
            records.append(lvl[0])
            pairs.append(npix * len(gs))
            total = part if total is None else total + part
        self.last_records, self._pairs = records, pairs
        return z0.sum() * 0 if total is None else total
