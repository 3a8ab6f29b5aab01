"""Device instance scoring: how many objects -- teeth, restorations, lesions -- were found, missed or invented, and how well
each found one overlaps its true one.  The connected components of the prediction and of the ground truth (the cut of the
class tree at a level, as in Data/postprocess.py) are matched one to one at IoU > 1/2 on the device; detection precision,
recall, recognition quality (F1), segmentation quality and panoptic quality PQ = SQ x RQ follow per group of the cut.
Kernels: csrc/instances.hip; the definitions are stated in include/hrseg.h (hrseg_mask_void_labels, hrseg_score_instances)
and DESIGN.md section 21.

The maps stay on the device; the records are integers (the same bytes in every run) and `InstanceScores.summary()` is the
one host read.  Pixels whose ground truth is no leaf's value are void in BOTH maps: a predicted region cut in two by a void
area counts as two components, one lying wholly in void does not exist.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import ops
from .._lib import require_gpu
from .postprocess import NO_GROUP, build_component_tables
from .score import DeviceScore

N_GT, N_PRED, TP, SUM_IOU, SUM_INTER, SUM_UNION, TP_AT = 0, 1, 2, 3, 4, 5, 6
Q30 = float(1 << 30)


def _ratio(a, b):
    return a / b if b else float("nan")


def summary_row(rec, thresholds):
    """the ten integers of one record row (ops.INSTANCE_FIELDS) -> the derived figures; NaN where a denominator is 0.
    pq = sq * rq is computed as sum_iou / (tp + fp / 2 + fn / 2): the same number wherever sq exists, and 0 -- not NaN -- for
    a group with objects but no match."""
    n_gt, n_pred, tp = int(rec[N_GT]), int(rec[N_PRED]), int(rec[TP])
    fp, fn = n_pred - tp, n_gt - tp
    sum_iou, denom = int(rec[SUM_IOU]) / Q30, tp + 0.5 * fp + 0.5 * fn
    return dict(n_gt=n_gt, n_pred=n_pred, tp=tp, fp=fp, fn=fn, precision=_ratio(tp, n_pred), recall=_ratio(tp, n_gt),
                rq=_ratio(tp, denom), sq=_ratio(sum_iou, tp), pq=_ratio(sum_iou, denom),
                mean_iou=_ratio(int(rec[SUM_INTER]), int(rec[SUM_UNION])),
                tp_at={t / 1000.0: int(rec[TP_AT + k]) for k, t in enumerate(thresholds)})


def summarize(records, names, thing_ids, thresholds):
    """records: integer array [R, 256, 10] on the host -> {thing group name: summary_row of the rows summed over R, "all": that
    of the counts summed over the thing groups, "mean_pq": mean pq over the groups with n_gt + n_pred > 0 (NaN: none)}"""
    total = np.asarray(records, dtype=np.int64).reshape(-1, 256, len(ops.INSTANCE_FIELDS)).sum(axis=0)
    out = {names[g]: summary_row(total[g], thresholds) for g in thing_ids}
    present = [out[names[g]]["pq"] for g in thing_ids if total[g, N_GT] + total[g, N_PRED] > 0]
    out["all"] = summary_row(total[list(thing_ids)].sum(axis=0) if len(thing_ids) else np.zeros(len(ops.INSTANCE_FIELDS), np.int64),
                             thresholds)
    out["mean_pq"] = float(np.mean(present)) if present else float("nan")
    return out


class InstanceScores:
    """What one or more `DeviceInstanceScore.score` calls left on the device.  `records` int64 [R, 256, 10] (row = image, or
    one row per call with per_image=False; group id; ops.INSTANCE_FIELDS).  Of a single call also: `pmatch` (indexed like the
    prediction buffer), `gmatch`, `ginter` (like the ground-truth buffer), `labels` (the masked prediction), `gt`, `proots`,
    `parea`, `groots`, `garea` and the descriptors `pdesc`, `pdesc_host`, `gdesc`, `gdesc_host`.  After `cat` these live in
    `parts`, one InstanceScores per call, in order."""

    MAPS = ("pmatch", "gmatch", "ginter", "labels", "gt", "proots", "parea", "groots", "garea", "pdesc", "pdesc_host", "gdesc",
            "gdesc_host")

    def __init__(self, records, scorer, parts=None, **maps):
        self.records, self.scorer = records, scorer
        for k in self.MAPS:
            setattr(self, k, maps.get(k))
        self.parts = [self] if parts is None else list(parts)

    def __len__(self):
        return self.records.shape[0]

    @staticmethod
    def cat(scores):
        """the scores of several batches as one: records row after row, the maps per call in `parts`"""
        first = scores[0]
        return InstanceScores(torch.cat([s.records for s in scores]), first.scorer, parts=[p for s in scores for p in s.parts])

    def summary(self):
        """{thing group name: dict(n_gt, n_pred, tp, fp, fn, precision, recall, rq, sq, pq, mean_iou, tp_at {threshold: pairs
        at IoU >= threshold}), "all": the same from the counts summed over the thing groups, "mean_pq": the mean pq of the
        groups with an object in either map}, over all rows; NaN where a denominator is 0.  One device-to-host copy."""
        s = self.scorer
        return summarize(self.records.cpu().numpy(), s.tables.names, s.thing_ids, s.thresholds)

    def instances(self):
        """the true thing components, one list per image in order: dict(group, first=(y, x), area, matched, iou, partner =
        (y, x) of the matched predicted component's first pixel or None).  Gathered on the device; one device-to-host copy."""
        names, rows, widths = self.scorer.tables.names, [], []
        for part in self.parts:
            group = self.scorer.device_tables(part.gt.device)[0]
            for (goff, H, W, _), (poff, _, _, _) in zip(part.gdesc_host.tolist(), part.pdesc_host.tolist()):
                match = part.gmatch[goff:goff + H * W]
                first = (match >= -1).nonzero().flatten()
                match = match[first].long()
                cols = [torch.full_like(first, len(widths)), first, part.garea[goff + first].long(), match,
                        part.ginter[goff + first].long(), part.parea[poff + match.clamp(min=0)].long(),
                        group[part.gt[goff + first].long()].long()]
                rows.append(torch.stack(cols, dim=1))
                widths.append(W)
        out = [[] for _ in widths]
        for b, first, area, match, inter, parea, g in (torch.cat(rows).tolist() if rows else []):
            W, hit = widths[b], match >= 0
            out[b].append(dict(group=names[g], first=(first // W, first % W), area=area, matched=hit,
                               iou=inter / (area + parea - inter) if hit else 0.0, partner=(match // W, match % W) if hit else None))
        return out


class DeviceInstanceScore:
    """`inst = DeviceInstanceScore(class_tree, class_map, level=0, things=["tooth"]); scores = inst.score(pred, gt)` ->
    InstanceScores.  The groups are the cut of the tree at `level` (build_component_tables, no rules); `things`: names of
    the cut nodes that are scored as instances, None = every group of the cut (KeyError / ValueError for a name that is not
    in the cut); connectivity 4 or 8; thresholds: up to 4 IoU values in (0.5, 1], kept as round(1000 t) per mille, at which
    matched pairs are counted besides (`tp_at`)."""

    def __init__(self, class_tree, class_map, level=0, things=None, connectivity=8, thresholds=(0.75, 0.9)):
        self.tables = build_component_tables(class_tree, class_map, level, None, connectivity)
        names = self.tables.names
        if things is None:
            self.thing_ids = list(range(len(names)))
        else:
            # (a name outside the tree, or inside it but not in the cut, is refused the way a rule on it is)
            build_component_tables(class_tree, class_map, level, {n: {} for n in things}, connectivity)
            self.thing_ids = sorted({names.index(n) for n in things})
        self.thing_names = [names[g] for g in self.thing_ids]
        thresholds = list(thresholds)
        if len(thresholds) > ops.INSTANCE_MAX_THRESHOLDS:
            raise ValueError(f"DeviceInstanceScore: {len(thresholds)} thresholds, at most {ops.INSTANCE_MAX_THRESHOLDS}")
        self.thresholds = []
        for t in thresholds:
            pm = int(round(float(t) * 1000.0)) if 0.5 < float(t) <= 1.0 else 0
            if not 501 <= pm <= 1000:
                raise ValueError(f"DeviceInstanceScore: threshold {t} must lie in (0.5, 1] (501..1000 per mille)")
            self.thresholds.append(pm)
        self.things = [1 if g in self.thing_ids else 0 for g in range(256)]
        assert not self.things[NO_GROUP]
        self._dev = {}

    def device_tables(self, device):
        """(group, things): the two [256] uint8 tables on the device, cached per device"""
        key = str(device)
        if key not in self._dev:
            self._dev[key] = (self.tables.device(device)[0], torch.tensor(self.things, dtype=torch.uint8, device=device))
        return self._dev[key]

    @staticmethod
    def _ground_truth(gt):
        if isinstance(gt, (list, tuple)) and len(gt) and all(isinstance(m, np.ndarray) for m in gt):
            from .decode import pack_images
            buf, host = pack_images(gt)
            if any(ch != 1 for _, _, _, ch in host.tolist()):
                raise ValueError("DeviceInstanceScore.score: ground-truth label maps are single-channel uint8 images")
            return buf, host, host
        return DeviceScore._triple(gt, ("label", "ldesc", "ldesc_host"))

    def score(self, pred, gt, per_image=True, out=None, workspace=None) -> InstanceScores:
        """pred: a RaggedLabels or a (buffer, desc, desc_host) triple; gt: such a triple, a RaggedBatch with label maps, or a
        list of numpy uint8 label maps.  out: the InstanceScores of an earlier call over maps of the same layout -- its records
        are added to, its match maps rewritten, and it is returned; workspace: see ops.score_instances.
        One masked copy, two labellings, ops.SCORE_INSTANCES_CALL_LAUNCHES scoring launches; no synchronisation."""
        require_gpu()
        pbuf, pdesc, phost = DeviceScore._triple(pred, ("labels", "desc", "desc_host"))
        gbuf, gdesc, ghost = self._ground_truth(gt)
        device = pbuf.device
        gbuf, pdesc, gdesc = (t.to(device, non_blocking=True) for t in (gbuf, pdesc, gdesc))
        group, things = self.device_tables(device)
        conn = self.tables.connectivity
        pm = ops.mask_void_labels(pbuf, pdesc, phost, gbuf, gdesc, ghost, group, self.tables.group)
        proots, parea = ops.label_components(pm, pdesc, phost, group, conn)
        groots, garea = ops.label_components(gbuf, gdesc, ghost, group, conn)
        given = None if out is None else (out.records, out.pmatch, out.gmatch, out.ginter)
        records, pmatch, gmatch, ginter = ops.score_instances(pm, pdesc, phost, proots, parea, gbuf, gdesc, ghost, groots, garea, group,
                                                              things, self.thresholds, per_image, given, workspace)
        maps = dict(pmatch=pmatch, gmatch=gmatch, ginter=ginter, labels=pm, gt=gbuf, proots=proots, parea=parea, groots=groots,
                    garea=garea, pdesc=pdesc, pdesc_host=phost, gdesc=gdesc, gdesc_host=ghost)
        if out is None:
            return InstanceScores(records, self, **maps)
        for k, v in maps.items():
            setattr(out, k, v)
        return out
