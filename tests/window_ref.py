"""torch-CPU oracle of sliding-window inference (csrc/windows.hip, include/hrseg.h: hrseg_decode_windows), built on
tests/decode_ref.py.  It shares no table with the product: the window origins and the blend profile are computed here from
the rules of the header.

  1. the windows of one image are blended into canvas logits [C_L, Hc, Wc]:
       g = (sum_a sum_b (wy_a wx_b) z_ab) / ((sum_a wy_a) (sum_b wx_b)),  a, b ascending,
     in float64 (dtype=torch.float32 evaluates the same formula in fp32: the yardstick of the confidence comparison);
  2. F.interpolate(mode="bilinear", align_corners=False) Hc x Wc -> H x W;
  3. the decision walk of `decode_ref.decode_sample` (arg-max over level 0, top-down through the child group of the chosen node
     only, leaf pixel value, confidence sigmoid * prod group soft-max).

Near ties (gap of the deciding group below decode_ref.NEAR_TIE) are marked at EVERY geometry: where the output has the
canvas size the resize is exact, the device's fp32 blend of several windows is not.

The case list of the oracle-compared GPU tests lives here too, so that the CPU test can bound each case's near-tie share."""
import functools
import math

import torch
import torch.nn.functional as F

from tests import decode_ref as R
from tests.decode_views_ref import MASK_CAP, channels, wide_tree  # noqa: F401  (the project's cap; trees of the cases)

S = 32


def origins(n, size, stride):
    """window origins along a canvas axis of length n: [0] if n == size, else ceil((n - size) / stride) + 1 origins
    min(i * stride, n - size)"""
    if n == size:
        return [0]
    return [min(i * stride, n - size) for i in range(int(math.ceil((n - size) / stride)) + 1)]


def stride_of(size, overlap):
    return size - int(math.floor(overlap * size))


def profile(size, blend):
    if blend == "uniform":
        return torch.ones(size, dtype=torch.float32)
    return torch.tensor([0.5 - 0.5 * math.cos(2.0 * math.pi * (i + 0.5) / size) for i in range(size)],
                        dtype=torch.float64).to(torch.float32)


def blend_canvas(windows, ys, xs, Hc, Wc, prof, dtype=torch.float64):
    """windows: per level [ny * nx, C_L, s, s] of ONE image, row-major over ys x xs -> per level [C_L, Hc, Wc]"""
    p = prof.to(dtype)
    s = p.numel()
    sy, sx = torch.zeros(Hc, dtype=dtype), torch.zeros(Wc, dtype=dtype)
    for y0 in ys:
        sy[y0:y0 + s] += p
    for x0 in xs:
        sx[x0:x0 + s] += p
    assert bool((sy > 0).all()) and bool((sx > 0).all()), "every canvas row and column is covered"
    out = []
    for z in windows:
        num = torch.zeros(z.shape[1], Hc, Wc, dtype=dtype)
        for a, y0 in enumerate(ys):
            for b, x0 in enumerate(xs):
                num[:, y0:y0 + s, x0:x0 + s] += (p[:, None] * p[None, :]) * z[a * len(xs) + b].to(dtype)
        out.append(num / (sy[:, None] * sx[None, :]))
    return out


def walk(z, tree, class_map, model_type, near=R.NEAR_TIE):
    """the decision walk of decode_ref.decode_sample on logits already at the output size (per level [C_L, H, W]), near ties
    marked whatever the geometry -> (label uint8, confidence, near-tie mask, path)"""
    pix = R.name2pix(class_map)
    levels = R.bfs_levels(tree)
    H, W = z[0].shape[-2:]
    label = torch.zeros(H, W, dtype=torch.uint8)
    conf = torch.ones(H, W, dtype=z[0].dtype)
    tie = torch.zeros(H, W, dtype=torch.bool)

    def decide(vals, sel, sigmoid):
        win = torch.argmax(vals, dim=0)
        top = vals.gather(0, win[None])[0]
        if vals.shape[0] > 1:
            second = vals.topk(2, dim=0).values[1]
            tie.logical_or_(sel & ((top - second) < near))
        factor = torch.sigmoid(top) if sigmoid else torch.softmax(vals, dim=0).gather(0, win[None])[0]
        return win, factor

    if int(model_type) == 0:
        leaves = [n for lvl in levels for n, kids in lvl if not kids]
        assert z[0].shape[0] == len(leaves)
        win, factor = decide(z[0], torch.ones(H, W, dtype=torch.bool), sigmoid=False)
        return torch.tensor([pix[n] for n in leaves], dtype=torch.uint8)[win], factor, tie, [win]

    path, prev = [], None
    for L, nodes in enumerate(levels):
        cur = torch.full((H, W), -1, dtype=torch.int64)
        if L == 0:
            groups = [(None, 0, len(nodes))]
        else:
            groups, start = [], 0
            for pc, (_, kids) in enumerate(levels[L - 1]):
                if kids:
                    groups.append((pc, start, len(kids)))
                    start += len(kids)
        for pc, start, n in groups:
            sel = torch.ones(H, W, dtype=torch.bool) if pc is None else (prev == pc)
            if not bool(sel.any()):
                continue
            win, factor = decide(z[L][start:start + n], sel, sigmoid=(L == 0))
            cur = torch.where(sel, win + start, cur)
            conf = torch.where(sel, conf * factor, conf)
        for c, (name, kids) in enumerate(nodes):
            if not kids:
                label = torch.where(cur == c, torch.tensor(pix[name], dtype=torch.uint8), label)
        path.append(cur)
        prev = cur
    return label, conf, tie, path


def resize(z, H, W):
    return [F.interpolate(a[None], size=(H, W), mode="bilinear", align_corners=False, antialias=False)[0] for a in z]


def decode_windows_sample(windows, ys, xs, Hc, Wc, prof, tree, class_map, model_type, H, W, dtype=torch.float64):
    """windows of ONE image (per level [ny * nx, C_L, s, s], or the flat model's single tensor) -> (label [H,W] uint8,
    confidence [H,W] dtype, near-tie mask [H,W] bool, path)"""
    windows = [windows] if torch.is_tensor(windows) else list(windows)
    return walk(resize(blend_canvas(windows, ys, xs, Hc, Wc, prof, dtype), H, W), tree, class_map, model_type)


def oracle_batch(logits, canvases, sizes, size, stride, prof, tree, class_map, model_type):
    """logits: per level [N, C_L, size, size] of the whole batch, windows numbered image by image, row-major -> per image the
    fp64 oracle's (label, confidence, tie) and the fp32 evaluation's (label, confidence)"""
    logits = [logits] if torch.is_tensor(logits) else list(logits)
    out, n0 = [], 0
    for (Hc, Wc), (H, W) in zip(canvases, sizes):
        ys, xs = origins(Hc, size, stride), origins(Wc, size, stride)
        wins = [z[n0:n0 + len(ys) * len(xs)] for z in logits]
        n0 += len(ys) * len(xs)
        label, conf, tie, _ = decode_windows_sample(wins, ys, xs, Hc, Wc, prof, tree, class_map, model_type, H, W)
        label32, conf32, _, _ = decode_windows_sample(wins, ys, xs, Hc, Wc, prof, tree, class_map, model_type, H, W, torch.float32)
        out.append((label, conf, tie, label32, conf32))
    assert n0 == logits[0].shape[0]
    return out


def window_count(canvases, size, stride):
    return sum(len(origins(Hc, size, stride)) * len(origins(Wc, size, stride)) for Hc, Wc in canvases)


def cut_windows(field, ys, xs, size):
    """[C, Hc, Wc] -> [ny * nx, C, size, size], row-major"""
    return torch.stack([field[:, y0:y0 + size, x0:x0 + size] for y0 in ys for x0 in xs]).contiguous()


# ------------------------------------------------------------------------------------ the oracle-compared GPU cases
# two calls of four images each (so that the n0 offsets matter): canvas -> output size
BATCHES = [([(32, 33), (50, 70), (80, 64), (32, 100)], [(32, 33), (50, 70), (33, 47), (30, 100)]),
           ([(50, 70), (80, 64), (97, 40), (64, 64)], [(7, 3), (2, 260), (97, 40), (64, 64)])]   # (64,64) at overlap 0: abutting
OVERLAPS = [0.5, 0.25, 0.0]
BLENDS = ["hann", "uniform"]
# (tree key: "tl" | "ext" | "wide", model_type, overlap, blend)
CASES = [(key, mt, ov, bl) for key in ("tl", "ext") for mt in (1, 0) for ov in OVERLAPS for bl in BLENDS] + \
        [("wide", 1, 0.5, "hann")]


def case_logits(tree, model_type, overlap, batch):
    """the windows' logits of one call on the CPU: per level [N, C_L, S, S], seeded by the call, the overlap and the model type"""
    canvases, _ = BATCHES[batch]
    N = window_count(canvases, S, stride_of(S, overlap))
    return R.smooth_logits(N, channels(tree, model_type), S, 300 + 17 * batch + 5 * OVERLAPS.index(overlap) + model_type)


@functools.lru_cache(maxsize=None)
def case_oracle(key, model_type, overlap, blend, load):
    """(tree, class map, per call (logits, oracle_batch)) of one CASES entry, computed once per process; `load` maps "tl" /
    "ext" to (tree, class map)"""
    tree, cmap = wide_tree() if key == "wide" else load(key)
    calls = []
    for batch, (canvases, sizes) in enumerate(BATCHES):
        logits = case_logits(tree, model_type, overlap, batch)
        calls.append((logits, oracle_batch(logits, canvases, sizes, S, stride_of(S, overlap), profile(S, blend), tree, cmap,
                                           model_type)))
    return tree, cmap, calls
