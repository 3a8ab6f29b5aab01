"""numpy reference of the device boundary scoring (csrc/boundary.hip, Data/boundary.py): the rule of include/hrseg.h
(hrseg_score_boundaries), evaluated straight from the class tree and the class map.  It builds none of the product's
tables: the mask of a node is the set of pixels whose value belongs to a leaf below (or at) the node.

For a predicted and a ground-truth map of one size:
  * a pixel whose ground truth is no leaf's value belongs to no node in either map; a predicted value that is no leaf's
    belongs to no predicted node;
  * a border pixel of a mask has one of its four neighbours outside the mask (the outside of the image counts as outside):
    shifted comparisons;
  * d2 of a border pixel = the least dy^2 + dx^2 to a border pixel of the same node in the other map: chunked all-pairs
    int64 differences;
  * record [2][5] per node, direction 0 = prediction -> truth: n, sum of math.isqrt(d2 << 32), max d2, count of
    d2 <= tau2, and the k-th smallest d2 with k = (percentile * n + 99) // 100 (np.sort); all but the two n are 0 when
    either n is 0.
"""
import math

import numpy as np

from tests.score_ref import bfs_levels, name2pix

FIELDS = ("n", "sum_q16", "max_d2", "within", "pk_d2")


def node_values(tree, class_map):
    """[(node name, sorted pixel values of the leaves below or at it)] for every node, breadth first"""
    pix = name2pix(class_map)
    below = {}

    def walk(node):
        for name, sub in node.items():
            if isinstance(sub, dict) and sub:
                walk(sub)
                below[name] = sorted(v for kid in sub for v in below[kid])
            else:
                below[name] = [pix[name]]
    walk(tree)
    return [(n, below[n]) for names in bfs_levels(tree) for n in names]


def border(mask):
    """border pixels of a boolean mask: pixels of it with a 4-neighbour outside it (or outside the image)"""
    m = np.pad(mask, 1, constant_values=False)
    inner = m[:-2, 1:-1] & m[2:, 1:-1] & m[1:-1, :-2] & m[1:-1, 2:]
    return mask & ~inner


def nearest_d2(queries, targets, chunk=2048):
    """[Q,2], [T,2] int64 pixel coordinates -> [Q] int64: least squared distance of every query to a target"""
    out = np.empty(len(queries), dtype=np.int64)
    for i in range(0, len(queries), chunk):
        q = queries[i:i + chunk]
        best = np.full(len(q), np.iinfo(np.int64).max, dtype=np.int64)
        for j in range(0, len(targets), chunk):
            d = q[:, None, :] - targets[None, j:j + chunk, :]
            best = np.minimum(best, (d * d).sum(-1).min(1))
        out[i:i + chunk] = best
    return out


def nearest_rank(values, percentile):
    """the k-th smallest of a non-empty integer array, k = ceil(percentile * n / 100) in integer arithmetic"""
    n = len(values)
    k = (int(percentile) * n + 99) // 100
    return int(np.sort(np.asarray(values))[k - 1])


def direction(d2, tau2, percentile):
    """the five fields of one direction from the d2 of its querying pixels"""
    return [len(d2), sum(math.isqrt(int(v) << 32) for v in d2.tolist()), int(d2.max()), int((d2 <= tau2).sum()),
            nearest_rank(d2, percentile)]


def masks(pred, gt, tree, class_map):
    """per node (breadth first) the boolean masks (prediction, ground truth)"""
    nodes = node_values(tree, class_map)
    valid = np.isin(gt, sorted({v for _, vals in nodes for v in vals}))          # the ground truth is some leaf's value
    return [(np.isin(pred, vals) & valid, np.isin(gt, vals) & valid) for _, vals in nodes]


def score_pair(pred, gt, tree, class_map, tau2, percentile):
    """pred, gt: uint8 arrays of one shape -> int64 [N, 2, 5]"""
    out = []
    for pm, gm in masks(np.asarray(pred), np.asarray(gt), tree, class_map):
        P, G = np.argwhere(border(pm)).astype(np.int64), np.argwhere(border(gm)).astype(np.int64)
        rec = [[len(P), 0, 0, 0, 0], [len(G), 0, 0, 0, 0]]
        if len(P) and len(G):
            rec = [direction(nearest_d2(P, G), tau2, percentile), direction(nearest_d2(G, P), tau2, percentile)]
        out.append(rec)
    return np.array(out, dtype=np.int64).reshape(len(out), 2, 5)


def score_batch(preds, gts, tree, class_map, tau2, percentile):
    """lists of maps -> int64 [B, N, 2, 5]"""
    return np.stack([score_pair(p, g, tree, class_map, tau2, percentile) for p, g in zip(preds, gts)])


def derived(records):
    """int64 [..., 2, 5] -> dict of fp64 arrays hausdorff, hd_percentile, assd, surface_dice (NaN where either n is 0)"""
    r = np.asarray(records).astype(object)                       # Python integers: no rounding before the division
    n0, n1 = r[..., 0, 0], r[..., 1, 0]
    both = (n0 > 0) & (n1 > 0)
    total = np.where(both, n0 + n1, 1)

    def f(v):
        return np.where(both, np.asarray(v, dtype=np.float64), np.nan)
    return dict(hausdorff=f(np.sqrt(np.maximum(r[..., 0, 2], r[..., 1, 2]).astype(np.float64))),
                hd_percentile=f(np.sqrt(np.maximum(r[..., 0, 4], r[..., 1, 4]).astype(np.float64))),
                assd=f((r[..., 0, 1] + r[..., 1, 1]).astype(np.float64) / 65536.0 / total.astype(np.float64)),
                surface_dice=f((r[..., 0, 3] + r[..., 1, 3]).astype(np.float64) / total.astype(np.float64)))


def blobby(rng, H, W, values, nblobs=6, background=0):
    """a map of `background` with `nblobs` filled ellipses of random values"""
    m = np.full((H, W), background, np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    for _ in range(nblobs):
        cy, cx = rng.integers(0, H), rng.integers(0, W)
        ry, rx = rng.integers(1, max(2, H // 3) + 1), rng.integers(1, max(2, W // 3) + 1)
        m[((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0] = values[rng.integers(0, len(values))]
    return m


def perturb(rng, m, values, flips=0.02):
    """the map rolled by a pixel or two with a few pixels redrawn: a plausible prediction of `m`"""
    out = np.roll(m, (int(rng.integers(-2, 3)), int(rng.integers(-2, 3))), (0, 1)).copy()
    hit = rng.random(m.shape) < flips
    out[hit] = np.asarray(values, dtype=np.uint8)[rng.integers(0, len(values), size=int(hit.sum()))]
    return out
