"""Device scoring pipeline: label maps at the source's own size against ground-truth label maps, both in the pixel
values of class_map.csv -> per-level confusion counts and the reference's per-class metrics.  Kernel: csrc/score.hip;
the semantics are stated in include/hrseg.h (hrseg_score_labels).

Levels are the tree's depths in breadth-first channel order, whatever model produced the map: a flat model's leaf map is
scored per hierarchy level the same way.  A prediction competes at level L only where it agreed with the ground truth
at the level above (the restrictive masking of the train loop, applied to decoded paths).  Pixels whose ground truth is
no leaf's value are ignored and counted, and so are predictions outside the class map -- at network size the reference
puts an unlabelled pixel into row 0 of level 0 instead (the arg-max of an all-zero target); here that is a deliberate
deviation.

The tables are built on the host without a GPU; only `score` launches.
"""
from __future__ import annotations

import torch

from .. import ops
from .._lib import require_gpu
from ..Metrics.performance_metrics import METRIC_NAMES
from ..utils.hierarchy import TreeIndex
from .dataset import TargetEncoder


class ScoreTables:
    """What hrseg_score_labels reads: `path` (256 ints: byte L = 1 + channel of the level-L node on the way to the leaf
    with that pixel value, 0 below the leaf; 0 = no leaf), `C` channels per level, `K` = C + 1 on child levels (label 0 is
    the synthetic background), `offsets` of the level matrices in a row of counts, `total` = sum K^2, `names` per level."""

    def __init__(self, path, C, names=None):
        self.path = [int(e) for e in path]
        self.C = [int(n) for n in C]
        self.K = [n + (1 if L else 0) for L, n in enumerate(self.C)]
        self.offsets = [sum(k * k for k in self.K[:L]) for L in range(len(self.K))]
        self.total = sum(k * k for k in self.K)
        self.names = names
        self._lut = {}

    def device_lut(self, device):
        """the path table as a [256] int64 device tensor (bit patterns of the uint64 entries), cached per device"""
        key = str(device)
        if key not in self._lut:
            self._lut[key] = torch.tensor([e - (1 << 64) if e >= (1 << 63) else e for e in self.path], dtype=torch.int64,
                                          device=device)
        return self._lut[key]


def build_score_tables(class_tree, class_map, internal_values=None) -> ScoreTables:
    """class_tree + class_map (any form TargetEncoder accepts) -> ScoreTables.  KeyError for a leaf without a pixel value,
    ValueError for one outside uint8 (both as Data.decode.build_tables) and for two leaves sharing a value.
    internal_values ({internal node name: byte}, e.g. a Data.Hedge's `values`): each such byte gets a path entry that ENDS
    at that node, with zero bytes below it -- a prediction of that byte competes down to the node and falls into the
    synthetic-background column of the levels below, as hrseg_score_labels states it for a path that ends above the ground
    truth's leaf.  The consequence on the other side: such a byte in a GROUND-TRUTH map then counts as labelled down to that
    node (row 0 of the levels below) instead of being ignored.  None builds exactly the leaf-only table."""
    name2pix = TargetEncoder._name2pix(class_map)
    index = TreeIndex(class_tree)
    levels = index.levels
    chan = {n: c for names in levels for c, n in enumerate(names)}
    path, owner = [0] * 256, {}
    for leaf in index.leaf_names:
        if leaf not in name2pix:
            raise KeyError(f"Class '{leaf}' not found in class_map.")
        v = int(name2pix[leaf])
        if not 0 <= v <= 255:
            raise ValueError(f"pixel value {v} of class '{leaf}' does not fit a uint8 label image")
        if v in owner:
            raise ValueError(f"classes '{owner[v]}' and '{leaf}' share the pixel value {v}")
        owner[v] = leaf
        node = leaf
        while node is not None:
            if index.depth[node] < 8:                   # (deeper trees are refused below, by their level count)
                path[v] |= (1 + chan[node]) << (8 * index.depth[node])
            node = index.parent[node]
    for name, v in (internal_values or {}).items():
        if name not in chan or not index.children[name]:
            raise ValueError(f"internal value for '{name}', which is no internal node of the class tree")
        v = int(v)
        if not 0 <= v <= 255:
            raise ValueError(f"value {v} of internal node '{name}' does not fit a uint8 label image")
        if v in owner:
            raise ValueError(f"classes '{owner[v]}' and '{name}' share the pixel value {v}")
        owner[v] = name
        node = name
        while node is not None:
            if index.depth[node] < 8:
                path[v] |= (1 + chan[node]) << (8 * index.depth[node])
            node = index.parent[node]
    tables = ScoreTables(path, [len(n) for n in levels], [list(n) for n in levels])
    ops.check_score_tables(tables)
    return tables


class SourceScores:
    """Counts of one or more `DeviceScore.score` calls: `counts` [R, tables.total] int64 (device; row = image, or one row
    of totals), `ignored` [R, 2] int64 (unlabelled ground truth, predictions outside the class map)."""

    def __init__(self, counts, ignored, tables):
        self.counts, self.ignored, self.tables = counts, ignored, tables

    def __len__(self):
        return self.counts.shape[0]

    def _row(self, image):
        return self.counts.sum(0) if image is None else self.counts[image]

    def confusion(self, level, image=None):
        """[K_L, K_L] int64 (target, predicted) of one image, or summed over all rows"""
        o, k = self.tables.offsets[level], self.tables.K[level]
        return self._row(image)[o:o + k * k].reshape(k, k)

    def metric_vectors(self, image=None):
        """dict over METRIC_NAMES of [sum C_L] fp32 device tensors (ops.metric_vectors: one launch), per tree node in
        breadth-first order; of one image, or of the counts summed over all rows"""
        row = self._row(image).contiguous()
        t = self.tables
        cms = [row[o:o + k * k].reshape(k, k) for o, k in zip(t.offsets, t.K)]
        vec = ops.metric_vectors(cms, [L > 0 for L in range(len(cms))])
        return {k: vec[i] for i, k in enumerate(METRIC_NAMES)}

    def total(self):
        """the same scores summed over the images: one row"""
        return SourceScores(self.counts.sum(0, keepdim=True), self.ignored.sum(0, keepdim=True), self.tables)


class DeviceScore:
    """`sc = DeviceScore(class_tree, class_map); scores = sc.score(pred, gt)` with `pred` a RaggedLabels (DeviceDecode /
    Predictor) or a (buffer, desc, desc_host) triple, `gt` a RaggedBatch (its label / ldesc / ldesc_host) or such a triple
    -> SourceScores.  out: a SourceScores of an earlier call with the same per_image and batch size, which is added to.
    internal_values: bytes of internal nodes (build_score_tables), for scoring hedged maps (Data.Hedge.values)."""

    def __init__(self, class_tree, class_map, internal_values=None):
        self.class_tree = class_tree
        self.tables = build_score_tables(class_tree, class_map, internal_values)

    @staticmethod
    def _triple(x, fields):
        if isinstance(x, (tuple, list)):
            buf, desc, host = x
        else:
            buf, desc, host = (getattr(x, f) for f in fields)
        if host is None:
            if desc.is_cuda:
                raise ValueError("a device descriptor table needs its host copy")
            host = desc
        return buf, desc, host

    def score(self, pred, gt, out=None, per_image=True) -> SourceScores:
        require_gpu()
        pbuf, pdesc, phost = self._triple(pred, ("labels", "desc", "desc_host"))
        gbuf, gdesc, ghost = self._triple(gt, ("label", "ldesc", "ldesc_host"))
        device = pbuf.device
        gbuf, pdesc, gdesc = (t.to(device, non_blocking=True) for t in (gbuf, pdesc, gdesc))
        counts, ignored = ops.score_labels(pbuf, pdesc, phost, gbuf, gdesc, ghost, self.tables,
                                           None if out is None else (out.counts, out.ignored), per_image)
        return out if out is not None else SourceScores(counts, ignored, self.tables)
