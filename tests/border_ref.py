"""References of the border weights (include/hrseg.h, "border weights") and the case lists tests/test_border_cpu.py,
tests/test_border_gpu.py and tests/test_loss_pw_gpu.py share.

Weight map of one level: `weight_map` is a numpy brute force of the header's semantics (shifted compares over the disc of
offsets), `weight_map_loops` an independent per-pixel double loop for tiny images.  Both are integer arithmetic up to the
table lookup, so a device result equals them bit for bit.

Per-pixel weights in the fused loss: `ce_dice` is tests/loss_options_ref.ce_dice with the weight on the two CE sums (the
weighted mass and the weighted sum of the terms of a class mask); the Dice term is that of the unweighted reference.
"""
import numpy as np
import torch
import torch.nn.functional as F

from tests import loss_options_ref as LR
from tests.headloss_ref import LOSS_UPSTREAM, _gen, _leaf

VOID = 255


# ============================================================================================ weight map
def table(w0, sigma, radius):
    """lut[0] = 1, lut[k] = (float)(1 + w0 exp(-k / (2 sigma^2))) in fp64 (written out here, not imported from the product)"""
    lut = np.empty(radius * radius + 1, dtype=np.float32)
    for k in range(radius * radius + 1):
        lut[k] = np.float32(1.0 + float(w0) * np.exp(-np.float64(k) / (2.0 * float(sigma) ** 2)))
    lut[0] = np.float32(1.0)
    return lut


def label_map(t):
    """t [B,C,H,W] float -> uint8 [B,H,W]: the first channel that is exactly 1, C when none is, 255 where every channel is -1"""
    t = np.asarray(t, dtype=np.float32)
    B, C, H, W = t.shape
    lab = np.full((B, H, W), C, dtype=np.int64)
    for c in range(C - 1, -1, -1):
        lab[t[:, c] == np.float32(1.0)] = c
    lab[(t == np.float32(-1.0)).all(axis=1)] = VOID
    return lab.astype(np.uint8)


def distances(labels, radius):
    """uint8 [B,H,W] -> int32 d2 [B,H,W]: shifted compares over the disc of offsets"""
    lab = labels.astype(np.int64)
    B, H, W = lab.shape
    big = radius * radius + 1
    best = np.full((B, H, W), big, dtype=np.int64)
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            d = dx * dx + dy * dy
            if d == 0 or d > radius * radius or abs(dy) >= H or abs(dx) >= W:
                continue
            ys, yd = (slice(dy, H), slice(0, H - dy)) if dy >= 0 else (slice(0, H + dy), slice(-dy, H))
            xs, xd = (slice(dx, W), slice(0, W - dx)) if dx >= 0 else (slice(0, W + dx), slice(-dx, W))
            src, dst = lab[:, ys, xs], lab[:, yd, xd]           # src = the pixel at (y + dy, x + dx) of dst's pixel
            hit = (src != VOID) & (dst != VOID) & (src != dst)
            view = best[:, yd, xd]
            view[hit & (view > d)] = d
    best[best == big] = 0
    return best.astype(np.int32)


def weight_map(t, radius, lut):
    """-> (labels uint8, v float32, d2 int32), each [B,H,W]"""
    labels = label_map(t)
    d2 = distances(labels, radius)
    return labels, np.asarray(lut, dtype=np.float32)[d2], d2


def weight_map_loops(t, radius, lut):
    """the same by a per-pixel double loop over every other pixel of the image (tiny images only)"""
    t = np.asarray(t, dtype=np.float32)
    B, C, H, W = t.shape
    labels = np.zeros((B, H, W), dtype=np.uint8)
    d2 = np.zeros((B, H, W), dtype=np.int32)
    for b in range(B):
        for y in range(H):
            for x in range(W):
                px = t[b, :, y, x]
                on = [c for c in range(C) if px[c] == 1.0]
                labels[b, y, x] = VOID if all(v == -1.0 for v in px) else (on[0] if on else C)
        for y in range(H):
            for x in range(W):
                me = labels[b, y, x]
                if me == VOID:
                    continue
                found = [(yy - y) ** 2 + (xx - x) ** 2 for yy in range(H) for xx in range(W)
                         if labels[b, yy, xx] != VOID and labels[b, yy, xx] != me and (yy - y) ** 2 + (xx - x) ** 2 <= radius * radius]
                d2[b, y, x] = min(found) if found else 0
    return labels, np.asarray(lut, dtype=np.float32)[d2], d2


def planes(labels, C, void=None):
    """label map [B,H,W] (values 0..C; C = nothing on) -> target planes [B,C,H,W] of 0 / 1, -1 everywhere where `void`"""
    labels = np.asarray(labels)
    t = np.zeros((labels.shape[0], C) + labels.shape[1:], dtype=np.float32)
    for c in range(C):
        t[:, c][labels == c] = 1.0
    if void is not None:
        t[np.broadcast_to(np.asarray(void, dtype=bool)[:, None], t.shape)] = -1.0
    return t


def voronoi(B, C, H, W, seed, nseeds=5, labels=None):
    """Voronoi blobs of a few seeds per image, labels drawn from 0..C (C = nothing on)"""
    rng = np.random.default_rng(seed)
    out = np.zeros((B, H, W), dtype=np.int64)
    yy, xx = np.mgrid[0:H, 0:W]
    for b in range(B):
        sy, sx = rng.integers(0, H, nseeds), rng.integers(0, W, nseeds)
        lab = rng.integers(0, C + 1, nseeds) if labels is None else np.asarray(labels)
        out[b] = lab[np.argmin((yy[None] - sy[:, None, None]) ** 2 + (xx[None] - sx[:, None, None]) ** 2, axis=0)]
    return out


# ============================================================================================ weighted loss
WEIGHT_KINDS = ("ones", "twos", "random", "border_like", "zeros", "plane_zero")
PW_OPTION_SETS = (LR.DEFAULTS, (2.0, 0.0, 0.5, 0.5), (0.5, 1.0, 0.5, 0.5))


def plane_zero_at(B, C):
    """(item, class) whose valid pixels all carry weight 0 in the `plane_zero` kind"""
    return B - 1, C // 2


def pixel_weights(kind, C, hw, B, pattern):
    """[B,1,hw] fp32 weights of the shared case (C, hw, B, pattern), seeded"""
    g = _gen(C, hw, B, 1000 + WEIGHT_KINDS.index(kind))
    if kind == "ones":
        return torch.ones(B, 1, hw)
    if kind == "twos":
        return torch.full((B, 1, hw), 2.0)
    u = torch.rand(B, 1, hw, generator=g)
    if kind == "random":
        return 0.5 + 10.5 * u
    if kind == "border_like":
        near = torch.rand(B, 1, hw, generator=g) < 0.2
        return torch.where(near, 1.0 + 10.0 * u.clamp(min=1e-3), torch.ones_like(u))
    w = 0.5 + 10.5 * u
    if kind == "zeros":
        return torch.where(torch.rand(B, 1, hw, generator=g) < 0.3, torch.zeros_like(w), w)
    assert kind == "plane_zero"
    b, c = plane_zero_at(B, C)
    t = LR.inputs(C, hw, B, pattern)["t"]
    w[b, 0][t[b, c, 0] != -1.0] = 0.0
    return w


def ce_dice(z, t, w, pw, options=LR.DEFAULTS):
    """loss_options_ref.ce_dice with pw [B,1,hw] on the two CE sums -> (CE, Dice or None, number of valid Dice items)"""
    gamma, smooth, alpha, beta = LR.options_f32(options)
    B, C = z.shape[:2]
    zf, tf = z.reshape(B, C, -1), t.reshape(B, C, -1)
    pwf = pw.reshape(B, 1, -1).to(z.dtype)
    m = (tf != -1).to(z.dtype)
    wt = torch.tensor(w, dtype=torch.float32).to(z.dtype)
    logp, p = F.log_softmax(zf, dim=1), torch.softmax(zf, dim=1)
    term = tf * logp
    if gamma > 0:
        om = LR.one_minus_p(zf)
        safe = torch.where(om > 0, om, torch.ones_like(om))
        term = term * torch.where(om > 0, safe ** gamma, torch.zeros_like(om))
    n = (pwf * m).sum(-1)
    s = (pwf * term * m).sum(-1)
    valid = (n > 0).all(1)
    item = (-(wt[None, :] * s) / torch.where(n > 0, n, torch.ones_like(n))).sum(1) / C
    ce = torch.where(valid, item, torch.ones_like(item)).mean()
    _, dice, nvalid = LR.ce_dice(z, t, w, options)
    return ce, dice, nvalid


def run(C, hw, B, pattern, kind, options, dtype):
    """the shared case through the weighted reference: values, valid-item count and d(0.7 CE + 1.3 Dice)/dz"""
    x = LR.inputs(C, hw, B, pattern)
    z = _leaf(x["z"], dtype)
    ce, dice, nvalid = ce_dice(z, x["t"].to(dtype), x["w"], pixel_weights(kind, C, hw, B, pattern), options)
    loss = LOSS_UPSTREAM[0] * ce + (LOSS_UPSTREAM[1] * dice if dice is not None else 0.0)
    loss.backward()
    return {"ce": ce.detach(), "dice": dice.detach() if dice is not None else torch.zeros((), dtype=dtype),
            "nvalid": nvalid, "dz": z.grad if z.grad is not None else torch.zeros_like(z)}
