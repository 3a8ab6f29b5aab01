"""torch-CPU oracle of the multi-view decode (csrc/decode_views.hip, include/hrseg.h: hrseg_decode_views), built on
tests/decode_ref.py: every view's logits are flipped back (torch.flip), resampled S_v x S_v -> H x W with
F.interpolate(mode="bilinear", align_corners=False), summed in view order and multiplied by 1/V; the mean logit then
takes the decision walk of `decode_ref.decode_sample` (arg-max over level 0, top-down through the child group of the
chosen node only, leaf pixel value, confidence sigmoid * prod group soft-max).  Evaluated in float64;
dtype=torch.float32 evaluates the same formula in fp32 (the yardstick of the confidence comparison).

Near ties (gap of the deciding group below decode_ref.NEAR_TIE) are marked as there, but with more than one view ALSO at
identity geometry: the resize is exact there, the fp32 mean of the device is not.

The case list of the oracle-compared GPU tests lives here too, so that the CPU test can bound each case's near-tie share."""
import functools

import torch
import torch.nn.functional as F

from tests import decode_ref as R
from tests.decode_harness import MASK_CAP, RAGGED  # noqa: F401  (the project's cap; output sizes of the cases)
from tests.decode_harness import _wide_tree as wide_tree

HFLIP, VFLIP = 1, 2


def flip(z, flags):
    """mirror the last two dimensions as the flags say (its own inverse)"""
    dims = [d for d, bit in ((-1, HFLIP), (-2, VFLIP)) if flags & bit]
    return torch.flip(z, dims) if dims else z


def mean_logits(views, H, W, dtype=torch.float64):
    """views: [(per-level [C_L,S_v,S_v] of one sample, flags)] -> per level [C_L,H,W]: ((r_0 + r_1) + ...) * (1 / V)"""
    inv = torch.tensor(1.0, dtype=dtype) / torch.tensor(float(len(views)), dtype=dtype)
    out = []
    for L in range(len(views[0][0])):
        acc = None
        for logits, flags in views:
            r = F.interpolate(flip(logits[L], flags)[None].to(dtype), size=(H, W), mode="bilinear", align_corners=False,
                              antialias=False)[0]
            acc = r if acc is None else acc + r
        out.append(acc * inv)
    return out


def decode_views_sample(views, tree, class_map, model_type, H, W, dtype=torch.float64, near=R.NEAR_TIE):
    """views: [(logits of ONE sample: per level [C_L,S_v,S_v], or the flat model's single tensor; flags)]
    -> (label [H,W] uint8, confidence [H,W] dtype, near-tie mask [H,W] bool, path: per level [H,W] int64 channel or -1)"""
    views = [(([z] if torch.is_tensor(z) else list(z)), f) for z, f in views]
    pix = R.name2pix(class_map)
    levels = R.bfs_levels(tree)
    identity = len(views) == 1 and all(H == z[0].shape[-1] == z[0].shape[-2] == W for z, _ in views)
    z = mean_logits(views, H, W, dtype)
    label = torch.zeros(H, W, dtype=torch.uint8)
    conf = torch.ones(H, W, dtype=dtype)
    tie = torch.zeros(H, W, dtype=torch.bool)

    def decide(vals, sel, sigmoid):
        win = torch.argmax(vals, dim=0)
        top = vals.gather(0, win[None])[0]
        if vals.shape[0] > 1 and not identity:
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


def channels(tree, model_type):
    """channels per level of a model's logits, straight from the tree"""
    levels = R.bfs_levels(tree)
    if int(model_type) == 0:
        return [sum(1 for lvl in levels for _, kids in lvl if not kids)]
    return [len(lvl) for lvl in levels]


# ------------------------------------------------------------------------------------ the oracle-compared GPU cases
VIEW_SETS = [[(62, 0), (62, 1), (46, 0)],
             [(62, 0), (62, 1), (62, 2), (62, 3)],
             [(62, 0), (78, 0), (46, 3)]]
EIGHT_VIEWS = [(62, f) for f in range(4)] + [(46, f) for f in range(4)]
# (tree key: "tl" | "ext" | "wide", model_type, view set)
CASES = [(key, mt, vs) for key in ("tl", "ext") for mt in (1, 0) for vs in range(len(VIEW_SETS))] + \
        [("wide", 1, 0), ("tl", 1, "eight")]


def case_views(tree, model_type, vs):
    """the case's views on the CPU: [(per-level [4,C_L,S_i,S_i], flags)], view i seeded 100 + 7 i + model_type"""
    Cs = channels(tree, model_type)
    sets = EIGHT_VIEWS if vs == "eight" else VIEW_SETS[vs]
    return [(R.smooth_logits(len(RAGGED), Cs, S, 100 + 7 * i + model_type), f) for i, (S, f) in enumerate(sets)]


def oracle_batch(views, tree, class_map, model_type, sizes):
    """per sample: the fp64 oracle's (label, confidence, tie) and the fp32 evaluation's (label, confidence)"""
    out = []
    for b, (H, W) in enumerate(sizes):
        vb = [([z[b] for z in logits], f) for logits, f in views]
        label, conf, tie, _ = decode_views_sample(vb, tree, class_map, model_type, H, W)
        label32, conf32, _, _ = decode_views_sample(vb, tree, class_map, model_type, H, W, dtype=torch.float32)
        out.append((label, conf, tie, label32, conf32))
    return out


@functools.lru_cache(maxsize=None)
def case_oracle(key, model_type, vs, load):
    """(tree, class map, views, oracle_batch over RAGGED) of one CASES entry, computed once per process; `load` maps
    "tl" / "ext" to (tree, class map)"""
    tree, cmap = wide_tree() if key == "wide" else load(key)
    views = case_views(tree, model_type, vs)
    return tree, cmap, views, oracle_batch(views, tree, cmap, model_type, RAGGED)
