"""numpy reference of the device instance scoring (include/hrseg.h: hrseg_mask_void_labels, hrseg_score_instances), written
from the stated semantics alone: mask, label both maps with tests/components_ref.py, build the FULL table of (predicted
component, true component) pairs and apply the match test to every pair.  It knows nothing about votes or majorities."""
import numpy as np

from tests import components_ref as C

FIELDS = ("n_gt", "n_pred", "tp", "sum_iou_q30", "sum_inter", "sum_union", "tp_at0", "tp_at1", "tp_at2", "tp_at3")
N_GT, N_PRED, TP, SUM_IOU, SUM_INTER, SUM_UNION, TP_AT = 0, 1, 2, 3, 4, 5, 6


def mask(pred, gt, group):
    """pred where the ground truth's value has a group, else a byte of group 255 (the smallest: any of them gives the same
    components); a plain copy when every byte has a group"""
    group = np.asarray(group)
    free = np.nonzero(group == 255)[0]
    if len(free) == 0:
        return np.array(pred, dtype=np.uint8, copy=True)
    return np.where(group[gt] == 255, np.uint8(free[0]), pred).astype(np.uint8)


def score_pair(pred, gt, group, things, connectivity, thresholds=()):
    """one image -> dict(records [256,10] int64, pmatch, gmatch, ginter [H,W] int32, pm, proots, parea, groots, garea, pairs =
    [(first pixel of P, first pixel of G, inter)] of the matches).  things: 256 flags by group id; thresholds: per mille"""
    group = np.asarray(group, dtype=np.int64)
    pred, gt = np.asarray(pred, dtype=np.uint8), np.asarray(gt, dtype=np.uint8)
    assert pred.shape == gt.shape
    HW = pred.size
    pm = mask(pred, gt, group)
    proots, parea = C.label(pm, group, connectivity)
    groots, garea = C.label(gt, group, connectivity)
    pg, gg = group[pm].reshape(-1), group[gt].reshape(-1)
    pr, pa, gr, ga = (a.reshape(-1).astype(np.int64) for a in (proots, parea, groots, garea))

    def thing(g):
        return g != 255 and bool(things[g])

    records = [[0] * len(FIELDS) for _ in range(256)]                      # Python integers: no overflow anywhere
    pmatch, gmatch, ginter = np.full(HW, -2, np.int32), np.full(HW, -2, np.int32), np.zeros(HW, np.int32)
    for f in np.nonzero(pa)[0].tolist():
        if thing(pg[f]):
            records[pg[f]][N_PRED] += 1
            pmatch[f] = -1
    for f in np.nonzero(ga)[0].tolist():
        if thing(gg[f]):
            records[gg[f]][N_GT] += 1
            gmatch[f] = -1
    keys, counts = np.unique(pr * HW + gr, return_counts=True)             # every (P, G) pair that shares a pixel
    pairs = []
    for key, inter in zip(keys.tolist(), counts.tolist()):
        p, g = divmod(key, HW)
        if pg[p] != gg[g] or not thing(gg[g]):
            continue
        P, G = int(pa[p]), int(ga[g])
        if not 3 * inter > P + G:
            continue
        assert pmatch[p] == -1 and gmatch[g] == -1, "a component appears in two matches"
        union = P + G - inter
        pmatch[p], gmatch[g], ginter[g] = g, p, inter
        rec = records[gg[g]]
        rec[TP] += 1
        rec[SUM_IOU] += (inter << 30) // union
        rec[SUM_INTER] += inter
        rec[SUM_UNION] += union
        for k, t in enumerate(thresholds):
            if t and inter * 1000 >= t * union:
                rec[TP_AT + k] += 1
        pairs.append((p, g, inter))
    shape = pred.shape
    return dict(records=np.array(records, dtype=np.int64), pmatch=pmatch.reshape(shape), gmatch=gmatch.reshape(shape),
                ginter=ginter.reshape(shape), pm=pm, proots=proots, parea=parea, groots=groots, garea=garea, pairs=pairs)


def score_batch(preds, gts, group, things, connectivity, thresholds=(), per_image=True):
    """-> (records [B or 1, 256, 10] int64, the per-image dicts of score_pair)"""
    each = [score_pair(p, g, group, things, connectivity, thresholds) for p, g in zip(preds, gts)]
    records = np.stack([e["records"] for e in each])
    return (records if per_image else records.sum(axis=0, keepdims=True)), each


# ---------------------------------------------------------------------------------------------------------------- patterns
def rectangles(rng, H, W, value, lo=6, hi=10, pitch=14, background=0):
    """a grid of rectangles lo..hi pixels on a side, one per pitch x pitch cell -> (map, [(y, x, h, w)])"""
    m = np.full((H, W), background, np.uint8)
    boxes = []
    for y0 in range(1, H - hi, pitch):
        for x0 in range(1, W - hi, pitch):
            h, w = (int(v) for v in rng.integers(lo, hi + 1, 2))
            y, x = y0 + int(rng.integers(0, pitch - hi)), x0 + int(rng.integers(0, pitch - hi))
            m[y:y + h, x:x + w] = value
            boxes.append((y, x, h, w))
    return m, boxes


def perturbed(rng, shape, boxes, value, drop=0.15, shift=2, salt=0.004, salt_values=(), background=0):
    """the boxes shifted by up to `shift` pixels, resized by -1..1, `drop` of them left out, salt noise on top"""
    H, W = shape
    m = np.full((H, W), background, np.uint8)
    for y, x, h, w in boxes:
        if rng.random() < drop:
            continue
        dy, dx = (int(v) for v in rng.integers(-shift, shift + 1, 2))
        dh, dw = (int(v) for v in rng.integers(-1, 2, 2))
        y0, x0 = max(0, y + dy), max(0, x + dx)
        m[y0:min(H, y + dy + h + dh), x0:min(W, x + dx + w + dw)] = value
    if salt and len(salt_values):
        noise = rng.random((H, W)) < salt
        m[noise] = rng.choice(np.asarray(salt_values, dtype=np.uint8), size=int(noise.sum()))
    return m
