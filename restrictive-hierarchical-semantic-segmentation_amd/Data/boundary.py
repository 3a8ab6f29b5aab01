"""Device boundary scoring: how far the predicted outline of every tree node lies from the true one, at the source's own
size -- Hausdorff distance, its nearest-rank percentile (HD95), average symmetric surface distance and surface Dice at a
tolerance, per image and tree node.  Kernels: csrc/boundary.hip; the definitions are stated in include/hrseg.h
(hrseg_score_boundaries) and DESIGN.md section 20.

The maps stay on the device; the records are integers (the same bytes in every run), the four derived tensors are
fp64 device tensors, and `BoundaryScores.summary()` is the one host read.  Unlike Data/score.py there is no restrictive
masking: the mask of a node is every valid pixel whose leaf lies below it, in each map on its own.  The percentile is the
larger of the two directions' nearest-rank percentiles, not an interpolated percentile of the concatenated distances.
"""
from __future__ import annotations

import math

import torch

from .. import ops
from .._lib import require_gpu
from .score import DeviceScore, build_score_tables

METRICS = ("hausdorff", "hd_percentile", "assd", "surface_dice")


class BoundaryScores:
    """Records of one or more `DeviceBoundaryScore.score` calls: `records` [R, N, 2, 5] int64 (device; image, node in
    breadth-first order, direction 0 = prediction -> truth, fields ops.BOUNDARY_FIELDS) and the derived fp64 [R, N]
    device tensors `hausdorff`, `hd_percentile`, `assd`, `surface_dice` (pixels; NaN where the node is absent from either
    map)."""

    def __init__(self, records, tables, tolerance, percentile):
        self.records, self.tables, self.tolerance, self.percentile = records, tables, tolerance, percentile
        self.names = [x for lvl in tables.names for x in lvl]
        r = records
        n = r[..., 0]
        both = (n[..., 0] > 0) & (n[..., 1] > 0)
        total = (n[..., 0] + n[..., 1]).to(torch.float64)
        nan = torch.full_like(total, float("nan"))

        def defined(v):
            return torch.where(both, v, nan)
        self.hausdorff = defined(torch.maximum(r[..., 0, 2], r[..., 1, 2]).to(torch.float64).sqrt())
        self.hd_percentile = defined(torch.maximum(r[..., 0, 4], r[..., 1, 4]).to(torch.float64).sqrt())
        self.assd = defined((r[..., 0, 1] + r[..., 1, 1]).to(torch.float64) / 65536.0 / total)
        self.surface_dice = defined((r[..., 0, 3] + r[..., 1, 3]).to(torch.float64) / total)

    def __len__(self):
        return self.records.shape[0]

    @staticmethod
    def cat(scores):
        """the scores of several batches as one (rows in order)"""
        first = scores[0]
        return BoundaryScores(torch.cat([s.records for s in scores]), first.tables, first.tolerance, first.percentile)

    def summary(self):
        """{node name: dict(hausdorff, hd_percentile, assd, surface_dice: mean over the images where the node is in both
        maps, NaN when there is none; images: their number; missed: images with the node in the truth only; spurious: in
        the prediction only)}.  One device-to-host copy."""
        n = self.records[..., 0].cpu()                                        # [R, N, 2]
        values = torch.stack([getattr(self, k) for k in METRICS]).cpu()     # [4, R, N]
        pred, truth = n[..., 0] > 0, n[..., 1] > 0
        out = {}
        for j, name in enumerate(self.names):
            both = pred[:, j] & truth[:, j]
            row = {k: (float(values[i, both, j].mean()) if bool(both.any()) else float("nan")) for i, k in enumerate(METRICS)}
            row.update(images=int(both.sum()), missed=int((truth[:, j] & ~pred[:, j]).sum()),
                       spurious=int((pred[:, j] & ~truth[:, j]).sum()))
            out[name] = row
        return out


class DeviceBoundaryScore:
    """`bs = DeviceBoundaryScore(class_tree, class_map, tolerance=2.0, percentile=95); scores = bs.score(pred, gt)` with the
    argument forms of DeviceScore.score -> BoundaryScores.  tolerance: pixels, the surface Dice counts border pixels within
    it (tau2 = floor(tolerance^2) is what the kernel compares the squared integer distances with); percentile: 1..100."""

    def __init__(self, class_tree, class_map, tolerance=2.0, percentile=95):
        self.class_tree = class_tree
        self.tables = build_score_tables(class_tree, class_map)
        self.tolerance, self.percentile = float(tolerance), int(percentile)
        if not (self.tolerance >= 0.0 and self.tolerance < 2.0 ** 31):
            raise ValueError(f"DeviceBoundaryScore: tolerance {tolerance} must be a non-negative number of pixels")
        if self.percentile != percentile or not 1 <= self.percentile <= 100:
            raise ValueError(f"DeviceBoundaryScore: percentile {percentile} must be an integer in 1..100")
        self.tau2 = int(math.floor(self.tolerance * self.tolerance))

    def score(self, pred, gt, workspace=None) -> BoundaryScores:
        require_gpu()
        pbuf, pdesc, phost = DeviceScore._triple(pred, ("labels", "desc", "desc_host"))
        gbuf, gdesc, ghost = DeviceScore._triple(gt, ("label", "ldesc", "ldesc_host"))
        device = pbuf.device
        gbuf, pdesc, gdesc = (t.to(device, non_blocking=True) for t in (gbuf, pdesc, gdesc))
        records = ops.score_boundaries(pbuf, pdesc, phost, gbuf, gdesc, ghost, self.tables, self.tau2, self.percentile,
                                       workspace=workspace)
        return BoundaryScores(records, self.tables, self.tolerance, self.percentile)
