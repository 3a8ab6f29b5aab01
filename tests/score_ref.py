"""numpy reference of the device scoring pipeline (csrc/score.hip, Data/score.py): the per-pixel rule of
include/hrseg.h (hrseg_score_labels), evaluated straight from the class tree and the class map.  It builds no path
table of the product's: every pixel value is resolved by walking the tree.

For a ground-truth map and a predicted map of one size:
  * the path of a pixel value is the list of (level, channel) of the nodes from the root to the leaf with that value,
    channels being positions in the breadth-first levels of the tree; a value that is no leaf's has no path;
  * ground truth without a path: ignored[0] += 1; else prediction without a path: ignored[1] += 1; else
  * level 0: cm_0[g_0][p_0] += 1 (C_0 x C_0);
  * level L >= 1: K = C_L + 1, label 0 the synthetic background: t = 1 + g_L (0 when the ground-truth leaf is shallower),
    q = 1 + p_L (0 when shallower) if the two paths name the same node at level L - 1 (or both none), else 0;
    cm_L[t][q] += 1.
"""
import numpy as np


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
    """[names] per depth, breadth first"""
    levels, frontier = [], list(tree.items())
    while frontier:
        levels.append([n for n, _ in frontier])
        frontier = [(k, v) for _, sub in frontier if isinstance(sub, dict) for k, v in sub.items()]
    return levels


def leaf_paths(tree, class_map):
    """{pixel value: [channel at level 0, channel at level 1, ...]} of every leaf, by a depth-first walk"""
    pix = name2pix(class_map)
    levels = bfs_levels(tree)
    out = {}

    def walk(node, depth, prefix):
        for name, sub in node.items():
            here = prefix + [levels[depth].index(name)]
            if isinstance(sub, dict) and sub:
                walk(sub, depth + 1, here)
            else:
                out[pix[name]] = here
    walk(tree, 0, [])
    return out, [len(n) for n in levels]


def score_pair(pred, gt, tree, class_map):
    """pred, gt: uint8 arrays of one shape -> (per-level int64 matrices [K_L, K_L] (target, predicted), ignored [2])"""
    paths, C = leaf_paths(tree, class_map)
    K = [n + (1 if L else 0) for L, n in enumerate(C)]
    cms = [np.zeros((k, k), dtype=np.int64) for k in K]
    ignored = np.zeros(2, dtype=np.int64)
    pairs, n = np.unique(np.stack([gt.reshape(-1), pred.reshape(-1)], 1).astype(np.int64), axis=0, return_counts=True)
    for (gv, pv), cnt in zip(pairs.tolist(), n.tolist()):
        g, p = paths.get(gv), paths.get(pv)
        if g is None:
            ignored[0] += cnt
            continue
        if p is None:
            ignored[1] += cnt
            continue
        cms[0][g[0], p[0]] += cnt
        for L in range(1, len(C)):
            gl = g[L] if L < len(g) else None
            pl = p[L] if L < len(p) else None
            gprev = g[L - 1] if L - 1 < len(g) else None
            pprev = p[L - 1] if L - 1 < len(p) else None
            t = 0 if gl is None else 1 + gl
            q = (0 if pl is None else 1 + pl) if gprev == pprev else 0
            cms[L][t, q] += cnt
    return cms, ignored


def score_batch(preds, gts, tree, class_map):
    """lists of maps -> (counts [B, sum K^2] int64, levels side by side; ignored [B, 2] int64)"""
    rows, ign = [], []
    for p, g in zip(preds, gts):
        cms, i = score_pair(np.asarray(p), np.asarray(g), tree, class_map)
        rows.append(np.concatenate([m.reshape(-1) for m in cms]))
        ign.append(i)
    return np.stack(rows), np.stack(ign)


def metrics_of(counts_row, C):
    """oracle.metrics-style divisions (fp64, rounded to fp32, 0 for a zero denominator) of one row of counts ->
    {name: [sum C] fp32}; child levels drop the pixels whose target is the synthetic background"""
    out = {k: [] for k in ("accuracy", "iou", "dice", "precision", "recall")}
    off = 0

    def div(a, b):
        a, b = a.astype(np.float64), b.astype(np.float64)
        return np.where(b == 0, 0.0, a / np.where(b == 0, 1.0, b)).astype(np.float32)

    for L, n in enumerate(C):
        k = n + (1 if L else 0)
        cm = np.asarray(counts_row[off:off + k * k]).reshape(k, k)
        off += k * k
        if L:
            cm = cm.copy()
            cm[0, :] = 0
        tp = np.diag(cm)
        fp, fn = cm.sum(0) - tp, cm.sum(1) - tp
        s = slice(1, None) if L else slice(None)
        tp, fp, fn = tp[s], fp[s], fn[s]
        out["accuracy"].append(div(tp, tp + fn))
        out["recall"].append(div(tp, tp + fn))
        out["iou"].append(div(tp, tp + fp + fn))
        out["dice"].append(div(2 * tp, 2 * tp + fp + fn))
        out["precision"].append(div(tp, tp + fp))
    return {k: np.concatenate(v) for k, v in out.items()}


# ---- trees of the tests
def wide_tree():
    """level 1 has 16 channels (the kernel's limit, K = 17) in groups of 5, 5 and 6"""
    tree, cmap, v = {"background": {}}, {"background": 0}, 10
    for g, n in enumerate((5, 5, 6)):
        tree[f"group{g}"] = {}
        for k in range(n):
            tree[f"group{g}"][f"g{g}c{k}"] = {}
            cmap[f"g{g}c{k}"] = v
            v += 10
    return tree, cmap


def chain_tree(depth=8):
    """`depth` levels: every level holds one leaf and one parent, the last level two leaves"""
    cmap, v = {}, 3
    node = tree = {}
    for d in range(depth - 1):
        node[f"leaf{d}"] = {}
        cmap[f"leaf{d}"] = v
        v += 7
        node[f"more{d}"] = {}
        node = node[f"more{d}"]
    for n in ("last_a", "last_b"):
        node[n] = {}
        cmap[n] = v
        v += 7
    return tree, cmap


def flat_tree():
    """a single level of five leaves"""
    return {f"c{i}": {} for i in range(5)}, {f"c{i}": 20 * i + 1 for i in range(5)}


def uniform_tree():
    """every root has at least 2 children, every leaf sits at depth 1"""
    tree = {"a": {"a0": {}, "a1": {}}, "b": {"b0": {}, "b1": {}, "b2": {}}, "c": {"c0": {}, "c1": {}}}
    names = [k for sub in tree.values() for k in sub]
    return tree, {n: 11 + 30 * i for i, n in enumerate(names)}
