"""torch-CPU oracle of the device output pipeline (csrc/decode.hip, Data/decode.py): the five steps of the restrictive
top-down decode, evaluated in float64 straight from the class tree (it shares no table with the product).

  1. every logit is resampled S x S -> H x W with F.interpolate(mode="bilinear", align_corners=False, antialias=False);
  2. level 0: arg-max over the level's channels (torch.argmax: lowest index wins ties);
  3. while the chosen node has children: arg-max over the consecutive channels of that child group at the next level;
  4. the label is the pixel value of the leaf that was reached;
  5. confidence = sigmoid(z_0[c_0]) * prod softmax_group(z_L)[c_L]  (flat models: softmax(z)[c]).

`decode_sample` also returns a near-tie mask: pixels where, at any level visited on the path, the best and second-best
logit of the deciding group are closer than NEAR_TIE.  torch's own fp32 bilinear resize differs from the fp64 one by up
to 2.4e-5 at 620 -> 1400x2900 for |z| <= 13; 2e-4 leaves about 4x room for two such errors.  At identity geometry the
resize is exact and nothing is marked.  dtype=torch.float32 evaluates the same formula in fp32 (the yardstick of the
confidence comparison)."""
import torch
import torch.nn.functional as F

NEAR_TIE = 2e-4


def name2pix(class_map):
    """class_map.csv rows / {name: value} dict -> {name: int pixel value} (parents have none)"""
    items = class_map.items() if isinstance(class_map, dict) else ((r["class_name"], r["pixel_val"]) for r in class_map)
    out = {}
    for name, v in items:
        if v is None or (isinstance(v, str) and v.strip().lower() in ("none", "nan", "")):
            continue
        out[name] = int(float(v))
    return out


def bfs_levels(tree):
    """[(name, [children names]) per node] per depth, breadth first"""
    levels, frontier = [], list(tree.items())
    while frontier:
        levels.append([(n, list(sub.keys()) if isinstance(sub, dict) else []) for n, sub in frontier])
        frontier = [(k, v) for _, sub in frontier if isinstance(sub, dict) for k, v in sub.items()]
    return levels


def decode_sample(logits, tree, class_map, model_type, H, W, dtype=torch.float64, near=NEAR_TIE):
    """logits: per level [C_L, S, S] (one sample; a flat model: one tensor over the leaves in BFS order)
    -> (label [H,W] uint8, confidence [H,W] dtype, near-tie mask [H,W] bool, path: per level [H,W] int64 channel or -1)"""
    pix = name2pix(class_map)
    levels = bfs_levels(tree)
    logits = [logits] if torch.is_tensor(logits) else list(logits)
    S = logits[0].shape[-1]
    identity = (H == S and W == S)
    z = [F.interpolate(a[None].to(dtype), size=(H, W), mode="bilinear", align_corners=False, antialias=False)[0] for a in logits]
    label = torch.zeros(H, W, dtype=torch.uint8)
    conf = torch.ones(H, W, dtype=dtype)
    tie = torch.zeros(H, W, dtype=torch.bool)

    def decide(vals, sel, sigmoid):
        """arg-max of vals [n,H,W] on the pixels of sel: (winner [H,W], confidence factor [H,W]); marks near ties"""
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
        everywhere = torch.ones(H, W, dtype=torch.bool)
        win, factor = decide(z[0], everywhere, sigmoid=False)
        lut = torch.tensor([pix[n] for n in leaves], dtype=torch.uint8)
        return lut[win], factor, tie, [win]

    path = []
    # groups of level L: (parent channel at L-1 or None, first channel, count); the channel order of a level is the
    # concatenation of its parents' child lists
    prev = None
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


def smooth_logits(B, Cs, S, seed, coarse=8):
    """synthetic per-level logits [B,C_L,S,S]: coarse 3*randn noise, bicubically upsampled, plus 0.05*randn"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for n in Cs:
        k = max(S // coarse, 2) + 2
        base = 3.0 * torch.randn(B, n, k, k, generator=g)
        out.append((F.interpolate(base, size=(S, S), mode="bicubic", align_corners=False) +
                    0.05 * torch.randn(B, n, S, S, generator=g)).contiguous())
    return out
