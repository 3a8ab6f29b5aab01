"""Device calibration scoring: how often is the model right when it says p?  Per-level logits at network size against
ground-truth label maps at the source's own size -> per tree node, and per level for the decoded path's top label, a
reliability histogram from which the expected and the maximum calibration error and the Brier score follow.  Kernel:
csrc/calibration.hip; the semantics are stated in include/hrseg.h (hrseg_score_calibration) and DESIGN.md section 22.

The probability that is scored is the model's own composition down the class tree, P_child = P_parent * softmax_group(z)
on the logits resampled to the source size exactly as the decode resamples them, optionally divided by a temperature per
level first.  No full-size probability plane exists at any point: the kernel bins every (probability, outcome) event into
exact integers (probabilities on a 2^-24 grid), so the same bytes come out of every run, a dataset total accumulates in
place, and `CalibrationScores.summary()` is the one host read.  Nothing is fitted on the device: `sweep` scores a list of
temperatures, one launch each, and the caller picks.

The tables are built on the host without a GPU; only `score` / `sweep` launch.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import ops
from .._lib import require_gpu
from ..utils.hierarchy import TreeIndex
from .dataset import TargetEncoder
from .decode import build_tables
from .score import DeviceScore, ScoreTables, build_score_tables

Q = 1 << 24                     # the probability grid of the records
N, POS, SUM_Q, SUM_E2 = range(4)
METRICS = ("n", "prevalence", "mean_confidence", "ece", "mce", "brier", "nonfinite")


def inverse_temperatures(temperature, nlevels):
    """None, a positive scalar or one positive value per level -> [nlevels] fp32 numpy array of 1 / T, the division done in
    fp32 (T = 1 gives exactly 1.0f: the kernel's multiplication is then the identity).  ValueError for a non-positive or
    non-finite temperature or a wrong count."""
    if temperature is None:
        return np.ones(nlevels, dtype=np.float32)
    t = np.asarray(temperature, dtype=np.float32).reshape(-1)
    if t.size == 1:
        t = np.repeat(t, nlevels)
    if t.size != nlevels:
        raise ValueError(f"temperature: {t.size} values for {nlevels} levels")
    if not bool(np.all(np.isfinite(t)) and np.all(t > 0)):
        raise ValueError(f"temperature: {t.tolist()} must be finite and positive")
    with np.errstate(over="ignore"):
        inv = (np.float32(1.0) / t).astype(np.float32)
    if not bool(np.all(np.isfinite(inv)) and np.all(inv > 0)):
        raise ValueError(f"temperature: 1 / {t.tolist()} is not a finite positive fp32 number")
    return inv


def flat_score_tables(class_tree, class_map) -> ScoreTables:
    """the path table of a flat model's single level over the leaves: byte 0 of entry v = 1 + the channel of the leaf with
    pixel value v (the leaves in the order Data.decode.build_tables gives them channels)"""
    name2pix = TargetEncoder._name2pix(class_map)
    leaves = TreeIndex(class_tree).leaf_names
    path = [0] * 256
    for c, leaf in enumerate(leaves):
        if leaf not in name2pix:
            raise KeyError(f"Class '{leaf}' not found in class_map.")
        v = int(name2pix[leaf])
        if not 0 <= v <= 255:
            raise ValueError(f"pixel value {v} of class '{leaf}' does not fit a uint8 label image")
        if path[v]:
            raise ValueError(f"classes '{leaves[path[v] - 1]}' and '{leaf}' share the pixel value {v}")
        path[v] = 1 + c
    tables = ScoreTables(path, [len(leaves)], [list(leaves)])
    ops.check_score_tables(tables)
    return tables


def metrics_from_records(rec):
    """one row's records [n_bins + 1, 4] (integers: n, pos, sum_q, sum_e2 per bin, the last bin the non-finite events) -> dict
    over METRICS, every figure from the integers in fp64; a row without a binned event reports NaN, not 0"""
    rec = np.asarray(rec)
    proper = rec[:-1].astype(np.int64)
    n, pos, sq = proper[:, N], proper[:, POS], proper[:, SUM_Q]
    total, nonfinite = int(n.sum()), int(rec[-1][N])
    if total == 0:
        nan = float("nan")
        return dict(n=0, prevalence=nan, mean_confidence=nan, ece=nan, mce=nan, brier=nan, nonfinite=nonfinite)
    gap = np.abs(pos * Q - sq)                      # |pos 2^24 - sum_q| per bin: exact in int64 (< 2^55 up to 2^31 events)
    full = n > 0
    return dict(n=total, prevalence=float(int(pos.sum()) / total), mean_confidence=float(int(sq.sum()) / (Q * float(total))),
                ece=float(int(gap.sum()) / (Q * float(total))),
                mce=float(np.max(gap[full].astype(np.float64) / (Q * n[full].astype(np.float64)))),
                brier=float(int(proper[:, SUM_E2].sum()) / (Q * float(total))), nonfinite=nonfinite)


class CalibrationScores:
    """Records of one or more `DeviceCalibrationScore.score` calls: `hist` [R, rows, n_bins + 1, 4] int64 (device; R = images,
    or one record of totals; rows = the tree's nodes in breadth-first order, then "top@L" per level; the last bin holds the
    non-finite events; (n, pos, sum_q, sum_e2)), `ignored` [R] int64 (pixels of unlabelled ground truth), `names` of the rows."""

    def __init__(self, hist, ignored, names, n_bins):
        self.hist, self.ignored, self.names, self.n_bins = hist, ignored, list(names), int(n_bins)

    def __len__(self):
        return self.hist.shape[0]

    def total(self):
        """the same scores summed over the images: one record"""
        return CalibrationScores(self.hist.sum(0, keepdim=True), self.ignored.sum(0, keepdim=True), self.names, self.n_bins)

    def _row(self, row):
        return self.names.index(row) if isinstance(row, str) else int(row)

    def summary(self):
        """{row name: dict(n, prevalence, mean_confidence, ece, mce, brier, nonfinite), "ignored": pixels} over all records.
        ece = sum_b |pos_b 2^24 - sum_q_b| / (2^24 N), mce = max over non-empty bins of |pos_b / n_b - sum_q_b / (2^24 n_b)|,
        brier = sum_e2 / (2^24 N), all over the n_bins proper bins; nonfinite = events whose probability was NaN (they are
        in no other figure).  One device-to-host copy."""
        host = torch.cat([self.hist.sum(0).reshape(-1), self.ignored.sum(0, keepdim=True)]).cpu().numpy()
        rec = host[:-1].reshape(len(self.names), self.n_bins + 1, 4)
        out = {name: metrics_from_records(rec[r]) for r, name in enumerate(self.names)}
        out["ignored"] = int(host[-1])
        return out

    def reliability(self, row, image=None):
        """the reliability diagram of one row (name or index) of one record, or summed over all: dict(edges [n_bins + 1], n
        [n_bins], accuracy = pos / n and confidence = sum_q / (2^24 n) per bin, NaN where a bin is empty)"""
        r = self._row(row)
        rec = (self.hist.sum(0) if image is None else self.hist[image])[r, :-1].cpu().numpy().astype(np.float64)
        n = rec[:, N]
        with np.errstate(divide="ignore", invalid="ignore"):
            acc, conf = rec[:, POS] / n, rec[:, SUM_Q] / (Q * n)
        return dict(edges=np.arange(self.n_bins + 1, dtype=np.float64) / self.n_bins, n=n.astype(np.int64), accuracy=acc,
                    confidence=conf)


class DeviceCalibrationScore:
    """`cal = DeviceCalibrationScore(class_tree, class_map, model_type); scores = cal.score(output_logits, gt)` with the
    models' `output_logits` (a list of per-level [B,C_L,S,S] tensors, or the flat model's single tensor) and `gt` a
    RaggedBatch (its label / ldesc / ldesc_host) or a (buffer, desc, desc_host) triple, as DeviceScore.score takes it ->
    CalibrationScores.  n_bins: 1..32 equal-width bins; temperature: None, a positive scalar or one per level (the logits
    of level L are divided by it -- multiplied by fp32 1 / T -- before the soft-max; 1 changes no bit).  A flat model
    (model_type 0) is scored on its one level over the leaves."""

    def __init__(self, class_tree, class_map, model_type=1, n_bins=15, temperature=None):
        self.class_tree, self.model_type, self.n_bins = class_tree, int(model_type), int(n_bins)
        if not 1 <= self.n_bins <= ops.CALIBRATION_MAX_BINS:
            raise ValueError(f"n_bins={n_bins}, supported 1..{ops.CALIBRATION_MAX_BINS}")
        self.tables = build_tables(class_tree, class_map, self.model_type)
        self.score_tables = flat_score_tables(class_tree, class_map) if self.model_type == 0 else \
            build_score_tables(class_tree, class_map)
        ops.check_calibration_tables(self.tables, self.score_tables)
        self.temperature = temperature
        self.inv_temp = inverse_temperatures(temperature, len(self.tables.C))
        self.names = [n for level in self.tables.names for n in level] + [f"top@{L}" for L in range(len(self.tables.C))]

    def _launch(self, output_logits, gt, inv_temp, out, per_image):
        require_gpu()
        logits = [output_logits] if torch.is_tensor(output_logits) else list(output_logits)
        gbuf, gdesc, ghost = DeviceScore._triple(gt, ("label", "ldesc", "ldesc_host"))
        device = logits[0].device
        gbuf, gdesc = gbuf.to(device, non_blocking=True), gdesc.to(device, non_blocking=True)
        hist, ignored = ops.score_calibration(logits, self.tables, (gbuf, gdesc, ghost), self.score_tables, inv_temp, self.n_bins,
                                              None if out is None else (out.hist, out.ignored), per_image)
        return out if out is not None else CalibrationScores(hist, ignored, self.names, self.n_bins)

    def score(self, output_logits, gt, out=None, per_image=False) -> CalibrationScores:
        """out: a CalibrationScores of an earlier call with the same per_image (and batch size, where per_image), which is
        added to: a dataset total accumulates in place"""
        return self._launch(output_logits, gt, self.inv_temp, out, per_image)

    def sweep(self, output_logits, gt, temperatures):
        """{T: summary of the batch scored at temperature T} for every T of `temperatures` (each a scalar or one value per
        level, given as a tuple): one launch per temperature.  A helper for choosing a temperature on held-out data."""
        out = {}
        for T in temperatures:
            key = tuple(float(v) for v in T) if isinstance(T, (tuple, list)) else float(T)
            inv = inverse_temperatures(T, len(self.tables.C))
            out[key] = self._launch(output_logits, gt, inv, None, False).summary()
        return out
