"""fp64 references of everything downstream of the backbone -- GAP, FiLM linear, the 1x1 heads, the logits resize, sigmoid and
probability composition over the class tree, the fused CE + soft-Dice loss, the consistency term and AdamW -- plus the ONE
case list and input builder per operation that tests/test_headloss_cpu.py and tests/test_headloss_gpu.py share.

The references are plain torch written from the operations' definitions (include/hrseg.h, the reference project's
formulas as oracle/ restates them); gradients come from autograd on them.  Every function works in the dtype of its
arguments: the GPU test evaluates it in float64, the CPU test also in float32 to measure how much room fp32 arithmetic
itself needs at exactly these inputs (it must stay within a quarter of the bar the GPU test applies).

Inputs are drawn in float32 -- the values the kernels see -- and cast to the evaluation dtype; hyper-parameters that the
ABI carries as fp32 (AdamW's lr, betas, eps, weight decay, gradient scale) are rounded to fp32 first for the same reason.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import losses as OL

# the bars of tests/test_kernels_gpu.py: rel = max |error| / max |reference|
BAR_POINT = 1e-5        # pointwise outputs and pointwise gradients
BAR_REDUCED = 2e-5      # gradients summed over pixels (dw, dbias, dgb) and dz of the loss
BAR_LOSS = 2e-6         # loss scalars, absolute
BAR_ADAMW = 1e-6
BAR_GAP = 1e-6
EPS_GATE = 1e-6


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-12))


def absdiff(a, b):
    return float((torch.as_tensor(a).detach().double().cpu() - torch.as_tensor(b).detach().double().cpu()).abs().max())


def _gen(*key):
    return torch.Generator().manual_seed(int(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31)))


# ============================================================================================ references
def gap(p):
    """[B,C,H,W] -> [B,C] mean over pixels"""
    return p.mean(dim=(2, 3))


def film_linear(cond, wl, bl):
    """gb[b][j] = bl[j] + sum_c cond[b][c] wl[j][c]"""
    return cond @ wl.t() + bl


def head(f, w, bias=None, gb=None):
    """z[b,c] = sum_k w[c][k] (f[b,k] gamma[b][k] + beta[b][k]) + bias[c];  gb = [gamma | beta] per sample, None = no FiLM"""
    nf = f.shape[1]
    if gb is not None:
        f = f * gb[:, :nf, None, None] + gb[:, nf:, None, None]
    z = torch.einsum("bkhw,ck->bchw", f, w)
    return z if bias is None else z + bias[None, :, None, None]


def logits_up(z, Ho, Wo, align_corners):
    return F.interpolate(z, size=(Ho, Wo), mode="bilinear", align_corners=align_corners)


def sigmoid(z):
    return torch.sigmoid(z)


def compose(z, pprev, parents, sizes):
    """P[children of g] = P_prev[parent_g] * softmax_children(z + log(P_prev[parent_g] + 1e-6)); groups take consecutive
    channels in the order given"""
    parts, start = [], 0
    for par, n in zip(parents, sizes):
        pp = pprev[:, par:par + 1]
        parts.append(pp * torch.softmax(z[:, start:start + n] + torch.log(pp + EPS_GATE), dim=1))
        start += n
    return torch.cat(parts, dim=1)


def ce_dice(z, t, w):
    """-> (CE, Dice or None, number of items whose Dice is not 0/0) of oracle.losses in the dtype of z"""
    ce = OL.cross_entropy_loss(z, t, True, w)
    dice = OL.soft_dice_loss(z, t, True, w)
    m = (t != -1).to(z.dtype)
    wt = torch.tensor(w, dtype=torch.float32)[None, :, None, None].to(z.dtype)
    union = (wt * (torch.softmax(z, 1) * m + t * m)).sum(dim=(1, 2, 3))
    return ce, dice, int((union != 0).sum())


def consistency_diffs(p, pprev, parents, sizes):
    """[B,G,H,W]: sum over the group's children of P minus P_prev[parent]"""
    out, start = [], 0
    for par, n in zip(parents, sizes):
        out.append(p[:, start:start + n].sum(1) - pprev[:, par])
        start += n
    return torch.stack(out, dim=1)


def consistency_sums(p, pprev, parents, sizes):
    """[G]: sum over batch and pixels of |sum_children P - P_parent|"""
    return consistency_diffs(p, pprev, parents, sizes).abs().sum(dim=(0, 2, 3))


def adamw_step(p, g, m, v, step, lr, beta1, beta2, eps, wd, gscale=1.0):
    """torch.optim.AdamW, single tensor, in place on (p, m, v); step counts from 1"""
    g = g * gscale
    p.mul_(1.0 - lr * wd)
    m.mul_(beta1).add_(g, alpha=1.0 - beta1)
    v.mul_(beta2).addcmul_(g, g, value=1.0 - beta2)
    bc1 = 1.0 - beta1 ** step
    bc2 = 1.0 - beta2 ** step
    denom = (v.sqrt() / math.sqrt(bc2)).add_(eps)
    p.addcdiv_(m, denom, value=-lr / bc1)


# ============================================================================================ head
# (F, Cout, FiLM, bias, H, W, channel-sliced buffers, df_accumulate); B = 2.  The branch each case takes follows from the
# host code of hrseg_head_fwd / hrseg_head_bwd (no launch counter exists for them):
#   forward: LP = 16 lanes per pixel for F <= 64, else 64; F <= 768 keeps the weights in registers, F = 772 and 1024 take the
#   LDS-weight loop; the grid is capped at 1024 blocks per sample (B = 2) of 256/LP pixels, so F=720 and F=772 at 70x67
#   (4690 > 4096) and F=64 at 129x131 (16899 > 16384) stride, every other case runs each loop once.
#   backward: P = 256 / (F/4) pixel lanes; F/4 = 3, 12, 17, 129, 193 do not divide 256 (idle threads), F = 4 gives P = 256,
#   F >= 516 gives P = 1.
HEAD_B = 2
HEAD_CASES = [
    (4, 1, False, True, 13, 11, False, False),
    (12, 3, True, True, 13, 11, True, True),
    (48, 4, False, True, 13, 11, False, True),
    (64, 5, True, True, 13, 11, True, False),
    (68, 8, False, True, 13, 11, True, True),
    (256, 2, True, True, 13, 11, False, False),
    (516, 4, False, False, 13, 11, True, False),
    (720, 7, True, True, 13, 11, False, True),
    (772, 4, True, True, 13, 11, True, False),
    (1024, 8, False, True, 13, 11, False, True),
    (64, 5, True, True, 1, 1, True, False),
    (720, 7, True, True, 70, 67, True, False),
    (64, 5, True, True, 129, 131, False, True),
    (772, 4, True, True, 70, 67, False, False),
]
HEAD_BARS = {"z": BAR_POINT, "df": BAR_POINT, "dw": BAR_REDUCED, "dbias": BAR_REDUCED, "dgb": BAR_REDUCED}


def head_inputs(case):
    nf, cout, film, bias, H, W = case[:6]
    g = _gen(nf, cout, H, W)
    return dict(f=torch.randn(HEAD_B, nf, H, W, generator=g), w=torch.randn(cout, nf, generator=g) / nf ** 0.5,
                bias=torch.randn(cout, generator=g) if bias else None,
                gb=torch.randn(HEAD_B, 2 * nf, generator=g) if film else None,
                dz=torch.randn(HEAD_B, cout, H, W, generator=g))


def _leaf(x, dtype):
    return None if x is None else x.to(dtype).clone().requires_grad_(True)


def head_run(case, dtype):
    x = head_inputs(case)
    f, w, bias, gb = (_leaf(x[k], dtype) for k in ("f", "w", "bias", "gb"))
    z = head(f, w, bias, gb)
    z.backward(x["dz"].to(dtype))
    out = {"z": z.detach(), "df": f.grad, "dw": w.grad}
    if bias is not None:
        out["dbias"] = bias.grad
    if gb is not None:
        out["dgb"] = gb.grad
    return out


# ============================================================================================ logits resize
UP_B = 2
UP_SIZES = [(16, 16, 62, 62), (39, 39, 155, 155), (7, 5, 20, 33), (1, 1, 9, 9), (5, 7, 1, 1), (20, 20, 20, 20), (31, 29, 10, 13)]
UP_C = (1, 3, 8, 16)
UP_BARS = {"out": BAR_POINT, "din": BAR_POINT}


def up_inputs(sizes, align, C):
    Hi, Wi, Ho, Wo = sizes
    g = _gen(Hi, Wi, Ho, Wo, int(align), C)
    # Logit maps are a smooth wave per channel plus a quarter-sigma of noise, not white noise: the source coordinate of an
    # output pixel carries ~1e-6 of fp32 rounding (scale * index, up to 155), which the interpolation multiplies by the
    # difference of NEIGHBOURING inputs.  With N(0,1) white noise that alone put fp32 torch-CPU 2.8e-6 from fp64 at
    # 39x39 -> 155x155 (align_corners, C=3), more than a quarter of the 1e-5 bar; the input was changed, not the bar.  An
    # index or weight that is off by one pixel still moves the result by ~1e-1 of its magnitude.
    # The backward's upstream gradient stays white noise: there the same coordinate rounding shifts weight between
    # neighbouring INPUT pixels, 2.5e-6 to 3e-6 of max |din| at 155 output pixels whatever the gradient looks like (smooth and
    # constant-plus-noise gradients were tried: 3.6e-6 to 3.9e-6) -- see HEADROOM_EXCEPTIONS in tests/test_headloss_cpu.py.
    def field(H, W):
        yy = torch.arange(H, dtype=torch.float32)[None, None, :, None]
        xx = torch.arange(W, dtype=torch.float32)[None, None, None, :]
        k = 0.6 * torch.rand(UP_B, C, 1, 1, generator=g)
        wave = 3.0 * torch.cos(k * yy + (0.6 - k) * xx + 6.28 * torch.rand(UP_B, C, 1, 1, generator=g))
        return wave + 0.25 * torch.randn(UP_B, C, H, W, generator=g)
    return dict(z=field(Hi, Wi), d=torch.randn(UP_B, C, Ho, Wo, generator=g))


def up_run(sizes, align, C, dtype):
    x = up_inputs(sizes, align, C)
    z = _leaf(x["z"], dtype)
    out = logits_up(z, sizes[2], sizes[3], align)
    out.backward(x["d"].to(dtype))
    return {"out": out.detach(), "din": z.grad}


# ============================================================================================ sigmoid / composition
TREES = [([1, 0], [2, 3]), ([2, 0, 1], [3, 1, 4]), ([0], [16]), (list(range(16))[::-1], [1] * 16)]
COMPOSE_SCALES = [(1.0, 1.0), (6.0, 1.0), (6.0, 20.0), (12.0, 30.0)]       # (parent logit scale, child logit scale)
COMPOSE_HW = [(9, 7), (1, 257)]
COMPOSE_B = 3
COMPOSE_BARS = {k: BAR_POINT for k in ("p", "dz", "dpprev", "dz_b", "dpprev_b")}
SIGMOID_SCALES = (1.0, 6.0, 12.0)
SIGMOID_BARS = {"p": BAR_GAP, "dz": BAR_POINT}
# three-level chain: level 1 = TREES[1] over 4 root channels, level 2 hangs under level-1 channels 7, 0 and 3
CHAIN = (TREES[1], ([7, 0, 3], [2, 2, 1]))
CHAIN_BARS = {k: BAR_POINT for k in ("p1", "p2", "dz2", "dz1", "dp0")}


def n_prev(parents):
    """one parent channel more than the tree uses (it must receive a zero gradient) where 16 channels allow it"""
    return min(16, max(parents) + 2)


def compose_inputs(tree, scales, hw):
    parents, sizes = tree
    H, W = hw
    C, Cp = sum(sizes), n_prev(parents)
    g = _gen(len(parents), C, int(scales[0]), int(scales[1]), H, W)
    pprev = torch.sigmoid(scales[0] * torch.randn(COMPOSE_B, Cp, H, W, generator=g))
    pprev[0, :, 0, 0:2] = 0.0                  # exact 0 and 1 parents in a few pixels
    pprev[1, :, 0, 2:4] = 1.0
    return dict(pprev=pprev, z=scales[1] * torch.randn(COMPOSE_B, C, H, W, generator=g),
                dp=torch.randn(COMPOSE_B, C, H, W, generator=g), dpb=torch.randn(COMPOSE_B, C, generator=g))


def compose_run(tree, scales, hw, dtype):
    x = compose_inputs(tree, scales, hw)
    out = {}
    for tag, dp in (("", x["dp"]), ("_b", x["dpb"][:, :, None, None].expand_as(x["dp"]))):
        z, pprev = _leaf(x["z"], dtype), _leaf(x["pprev"], dtype)
        p = compose(z, pprev, *tree)
        (p * dp.to(dtype)).sum().backward()
        out.update({"p": p.detach(), "dz" + tag: z.grad, "dpprev" + tag: pprev.grad})
    return out


def sigmoid_inputs(scale):
    g = _gen(int(scale), 3)
    return dict(z=scale * torch.randn(3, 5, 9, 7, generator=g), dp=torch.randn(3, 5, 9, 7, generator=g))


def sigmoid_run(scale, dtype):
    x = sigmoid_inputs(scale)
    z = _leaf(x["z"], dtype)
    p = sigmoid(z)
    p.backward(x["dp"].to(dtype))
    return {"p": p.detach(), "dz": z.grad}


def chain_inputs(scales, hw):
    H, W = hw
    (par1, siz1), (par2, siz2) = CHAIN
    g = _gen(99, int(scales[0]), int(scales[1]), H, W)
    return dict(p0=torch.sigmoid(scales[0] * torch.randn(COMPOSE_B, n_prev(par1), H, W, generator=g)),
                z1=scales[1] * torch.randn(COMPOSE_B, sum(siz1), H, W, generator=g),
                z2=scales[1] * torch.randn(COMPOSE_B, sum(siz2), H, W, generator=g),
                d1=torch.randn(COMPOSE_B, sum(siz1), H, W, generator=g), d2=torch.randn(COMPOSE_B, sum(siz2), H, W, generator=g))


def chain_run(scales, hw, dtype):
    x = chain_inputs(scales, hw)
    p0, z1, z2 = (_leaf(x[k], dtype) for k in ("p0", "z1", "z2"))
    p1 = compose(z1, p0, *CHAIN[0])
    p2 = compose(z2, p1, *CHAIN[1])
    ((p1 * x["d1"].to(dtype)).sum() + (p2 * x["d2"].to(dtype)).sum()).backward()
    return {"p1": p1.detach(), "p2": p2.detach(), "dz2": z2.grad, "dz1": z1.grad, "dp0": p0.grad}


# ============================================================================================ loss
# C = 9 and 16 select the 16-wide instances of the loss and metrics kernels (C <= 4 / <= 8 / else in the host code); hw = 5000
# splits into ceil(5000 / 256) = 20 blocks per sample, every other hw is one block
LOSS_C = (1, 4, 5, 8, 9, 16)
LOSS_HW = (1, 255, 256, 257, 5000)
LOSS_B = (1, 3)
LOSS_PATTERNS = ("no_ignore", "random_ignore", "plane_ignored", "item_ignored", "all_ignored", "zero_weight")
LOSS_UPSTREAM = (0.7, 1.3)
LOSS_BARS = {"ce": BAR_LOSS, "dice": BAR_LOSS, "dz": BAR_REDUCED}          # ce / dice absolute, dz rel


def loss_inputs(C, hw, B, pattern):
    g = _gen(C, hw, B, LOSS_PATTERNS.index(pattern))
    z = 2.0 * torch.randn(B, C, 1, hw, generator=g)
    if pattern == "no_ignore":
        t = torch.randint(0, 2, (B, C, 1, hw), generator=g).float()
    else:
        t = torch.randint(-1, 2, (B, C, 1, hw), generator=g).float()
    w = [float(v) for v in (0.25 + 1.5 * torch.rand(C, generator=g))]
    if pattern == "plane_ignored":
        t[B - 1, C - 1] = -1.0                 # CE item of that sample becomes the constant 1.0
    elif pattern == "item_ignored":
        t[0] = -1.0                            # its Dice item is 0/0: dropped, out[2] counts the rest
    elif pattern == "all_ignored":
        t[:] = -1.0
    elif pattern == "zero_weight":
        w[0] = 0.0
    return dict(z=z, t=t, w=w)


def loss_run(C, hw, B, pattern, dtype):
    x = loss_inputs(C, hw, B, pattern)
    z = _leaf(x["z"], dtype)
    ce, dice, nvalid = ce_dice(z, x["t"].to(dtype), x["w"])
    loss = LOSS_UPSTREAM[0] * ce + (LOSS_UPSTREAM[1] * dice if dice is not None else 0.0)
    loss.backward()
    return {"ce": ce.detach(), "dice": dice.detach() if dice is not None else torch.zeros((), dtype=dtype),
            "nvalid": nvalid, "dz": z.grad if z.grad is not None else torch.zeros_like(z)}


# ============================================================================================ consistency
CONS_HW = [(21, 19), (1, 257)]
CONS_B = 2
CONS_SCALE, CONS_G = 0.37, 1.7
CONS_TIE = 1e-5             # |sum - parent| below this in fp64: the fp32 sign is not determined, the pixel is left out
CONS_MAX_TIE_SHARE = 1e-3
CONS_BARS = {"mean": BAR_LOSS}


def cons_inputs(tree, hw):
    """soft probabilities whose child sums scatter around the parent's value (both signs occur in every group)"""
    parents, sizes = tree
    H, W = hw
    g = _gen(9, len(parents), sum(sizes), H, W)
    prev = 0.2 + 0.8 * torch.rand(CONS_B, n_prev(parents), H, W, generator=g)
    parts = []
    for par, n in zip(parents, sizes):
        share = torch.softmax(2.0 * torch.randn(CONS_B, n, H, W, generator=g), 1)
        # noise of either sign but at least 0.05 in size: a one-child group is then never near a tie, larger groups rarely
        noise = (0.05 + 0.2 * torch.rand(CONS_B, n, H, W, generator=g)) / n * (2.0 * torch.randint(0, 2, (CONS_B, n, H, W), generator=g) - 1.0)
        parts.append((prev[:, par:par + 1] * share + noise).clamp_min(0.0))
    return dict(prev=prev, cur=torch.cat(parts, 1))


def cons_onehot_inputs(tree, hw):
    """one-hot children whose parent map is their exact sum (ties: zero gradient) except on every third pixel column,
    where the parent is flipped (difference exactly +1 or -1)"""
    parents, sizes = tree
    H, W = hw
    g = _gen(8, len(parents), sum(sizes), H, W)
    C = sum(sizes)
    cur = F.one_hot(torch.randint(0, C, (CONS_B, H, W), generator=g), C).permute(0, 3, 1, 2).float().contiguous()
    prev = torch.zeros(CONS_B, n_prev(parents), H, W)
    start = 0
    for par, n in zip(parents, sizes):
        prev[:, par] = cur[:, start:start + n].sum(1)
        start += n
    prev[..., ::3] = 1.0 - prev[..., ::3]
    return dict(prev=prev, cur=cur)


def cons_run(x, tree, dtype):
    """-> per-group sums, their mean form (the loss scalar), d/dcur and d/dprev of CONS_G * CONS_SCALE * sum, the near-tie
    mask [B,G,H,W]"""
    cur, prev = _leaf(x["cur"], dtype), _leaf(x["prev"], dtype)
    sums = consistency_sums(cur, prev, *tree)
    (CONS_G * CONS_SCALE * sums.sum()).backward()
    n = cur.shape[0] * cur.shape[2] * cur.shape[3]
    diffs = consistency_diffs(cur.detach(), prev.detach(), *tree)
    return {"sums": sums.detach(), "mean": sums.detach() / n, "dcur": cur.grad, "dprev": prev.grad,
            "diffs": diffs, "tie": diffs.abs() < CONS_TIE}


# end to end through hierarchical_consistency_loss: three levels in BFS channel order (the product's wrapper requires it)
E2E_LEVELS = [["a", "b", "c"], ["a1", "a2", "a3", "b1", "c1", "c2", "c3", "c4"], ["a2x", "a2y", "c1x", "c1y", "c1z"]]
E2E_PARENT_OF = {"a": None, "b": None, "c": None, "a1": "a", "a2": "a", "a3": "a", "b1": "b", "c1": "c", "c2": "c", "c3": "c",
                 "c4": "c", "a2x": "a2", "a2y": "a2", "c1x": "c1", "c1y": "c1", "c1z": "c1"}
E2E_TREES = [([0, 1, 2], [3, 1, 4]), ([1, 4], [2, 3])]


def e2e_inputs():
    g = _gen(5, 5, 5)
    B, H, W = 2, 21, 19
    probs = [0.2 + 0.8 * torch.rand(B, 3, H, W, generator=g)]
    for parents, sizes in E2E_TREES:
        parts = []
        for par, n in zip(parents, sizes):
            share = torch.softmax(2.0 * torch.randn(B, n, H, W, generator=g), 1)
            noise = (0.05 + 0.2 * torch.rand(B, n, H, W, generator=g)) / n * (2.0 * torch.randint(0, 2, (B, n, H, W), generator=g) - 1.0)
            parts.append((probs[-1][:, par:par + 1] * share + noise).clamp_min(0.02))     # (no plateau at 0: exact ties)
        probs.append(torch.cat(parts, 1))
    return probs


def e2e_run(reduction, dtype):
    probs = [_leaf(p, dtype) for p in e2e_inputs()]
    loss = OL.hierarchical_consistency_loss(probs, E2E_LEVELS, E2E_PARENT_OF, reduction)
    (1.3 * loss).backward()
    return {"loss": loss.detach(), "grads": [p.grad for p in probs]}


def e2e_ties():
    """number of (pixel, group) entries of the end-to-end inputs closer to a tie than CONS_TIE (fp64)"""
    probs = [p.double() for p in e2e_inputs()]
    return sum(int((consistency_diffs(probs[L + 1], probs[L], *E2E_TREES[L]).abs() < CONS_TIE).sum()) for L in range(2))


# ============================================================================================ AdamW
# n = 8192*1024 + 5: n/4 = 2097153 quads need 8193 blocks of 256, the grid is capped at 8192, so the grid-stride loop takes a
# second trip and one element is left for the tail (hrseg_adamw / hrseg_adamw_dev host code)
ADAMW_N = (1, 2, 3, 4, 5, 7, 1023, 10007, 8192 * 1024 + 5)
ADAMW_LRS = (1e-3, 1e-3, 5e-4, 5e-4, 2e-3)        # changes before steps 3 and 5
ADAMW_WDS = (0.0, 0.01)
ADAMW_GSCALE = 0.25
ADAMW_BARS = {"p": BAR_ADAMW, "m": BAR_ADAMW, "v": BAR_ADAMW}


def f32(x):
    return float(np.float32(x))


ADAMW_BETA1, ADAMW_BETA2, ADAMW_EPS = f32(0.9), f32(0.999), f32(1e-8)


def adamw_inputs(n):
    g = _gen(14, n % 100003)
    return dict(p=torch.randn(n, generator=g), grads=[4.0 * torch.randn(n, generator=g) for _ in ADAMW_LRS])


def adamw_run(x, wd, dtype):
    p = x["p"].to(dtype).clone()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    for k, lr in enumerate(ADAMW_LRS):
        adamw_step(p, x["grads"][k].to(dtype), m, v, k + 1, f32(lr), ADAMW_BETA1, ADAMW_BETA2, ADAMW_EPS, f32(wd),
                   f32(ADAMW_GSCALE))
    return {"p": p, "m": m, "v": v}


def adamw_state(k):
    """{step, 1 - beta1^k, 1 / sqrt(1 - beta2^k)} after k steps, rounded to fp32"""
    return [f32(k), f32(1.0 - ADAMW_BETA1 ** k), f32(1.0 / math.sqrt(1.0 - ADAMW_BETA2 ** k))]


# ============================================================================================ GAP / FiLM linear
# 64 splits per row: hw < 64 leaves empty splits, 63 / 64 / 65 straddle one pixel per split, 620*620 is the headline size
GAP_HW = [(1, 1), (7, 9), (8, 8), (5, 13), (29, 37), (620, 620)]
GAP_BARS = {"cond": BAR_GAP}
FILM_CASES = [(1, 1, 8), (4, 4, 128), (2, 16, 1440), (3, 7, 1442)]       # (B, Cc, F2)
FILM_DCOND_SCALE = 0.5
FILM_BARS = {k: BAR_POINT for k in ("gb", "dcond", "dwl", "dbl")}


def gap_inputs(hw):
    return dict(p=torch.rand(2, 4, hw[0], hw[1], generator=_gen(13, hw[0], hw[1])))


def gap_run(hw, dtype):
    return {"cond": gap(gap_inputs(hw)["p"].to(dtype))}


def film_inputs(case):
    B, Cc, F2 = case
    g = _gen(17, B, Cc, F2)
    return dict(cond=torch.rand(B, Cc, generator=g), wl=torch.randn(F2, Cc, generator=g), bl=torch.randn(F2, generator=g),
                dgb=torch.randn(B, F2, generator=g))


def film_run(case, dtype):
    x = film_inputs(case)
    cond, wl, bl = (_leaf(x[k], dtype) for k in ("cond", "wl", "bl"))
    gb = film_linear(cond, wl, bl)
    gb.backward(x["dgb"].to(dtype))
    return {"gb": gb.detach(), "dcond": FILM_DCOND_SCALE * cond.grad, "dwl": wl.grad, "dbl": bl.grad}
