"""Hedged decode policy: where the model is unsure between the children of a node it is sure of, answer with the node.

The model composes its probabilities down the class tree, P_child = P_parent * softmax_group(z), and the decode carries the
composed confidence T_L of its path level by level.  A `Hedge` gives every node a threshold: the walk enters node (L, c)
only where T_L >= tau[L][c]; otherwise the pixel is labelled with the byte of the node it stands on -- an internal node's
own pixel value, which `class_map.csv` does not have and this class assigns -- or, where level 0 itself fails, with the
reject value.  That is a correct, less specific answer instead of a coin flip at the leaf.  Kernel: csrc/decode_hedged.hip;
the semantics are stated in include/hrseg.h (hrseg_decode_hedged) and DESIGN.md section 23.

`Hedge.from_calibration` fits one threshold per child level from the "top@L" reliability records of a
`Data.CalibrationScores`.  The tables are built and validated on the host without a GPU; `DeviceDecode.decode_hedged`
launches.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import ops
from .decode import build_tables


class Hedge:
    """`Hedge(class_tree, class_map, thresholds, internal_values=None, reject_value=None)`.
    thresholds: a scalar (every node of every child level; level 0 stays 0), a list of one value per level (the first is
      level 0's), or a dict {node name: threshold} (nodes not named get 0).  0 never stops.
    internal_values: {internal node name: byte}; the internal nodes it does not name get the smallest uint8 values that
      nothing else uses, in breadth-first order.  The full assignment is `hedge.values`.
    reject_value: the byte written where level 0 itself is below its threshold; None: no rejection, and then every level-0
      threshold must be 0.
    `tables` (Data.decode.DecodeTables), `tau` and `stop_val` (per level and channel; -1 for leaves) and `reject_val` (-1:
    none) are what ops.decode_hedged reads; `value_names` maps every byte a hedged map can hold to its node name (the reject
    value to "rejected").  ValueError for everything hrseg_decode_hedged refuses, with the nodes' names."""

    def __init__(self, class_tree, class_map, thresholds, internal_values=None, reject_value=None):
        self.class_tree, self.class_map = class_tree, class_map
        self.tables = t = build_tables(class_tree, class_map, 1)
        where = {n: (L, c) for L, names in enumerate(t.names) for c, n in enumerate(names)}
        internal = [n for L, names in enumerate(t.names) for c, n in enumerate(names) if t.n_children[L][c]]
        # ---- thresholds
        self.tau = [[0.0] * n for n in t.C]
        if isinstance(thresholds, dict):
            for name, v in thresholds.items():
                if name not in where:
                    raise ValueError(f"Hedge: threshold for '{name}', which is no node of the class tree")
                L, c = where[name]
                self.tau[L][c] = float(v)
        elif isinstance(thresholds, (list, tuple, np.ndarray)):
            if len(thresholds) != len(t.C):
                raise ValueError(f"Hedge: {len(thresholds)} per-level thresholds for {len(t.C)} levels")
            self.tau = [[float(v)] * n for v, n in zip(thresholds, t.C)]
        else:
            self.tau = [[float(thresholds) if L else 0.0] * n for L, n in enumerate(t.C)]
        # ---- byte values of the internal nodes
        given = dict(internal_values or {})
        for name in given:
            if name not in where:
                raise ValueError(f"Hedge: internal value for '{name}', which is no node of the class tree")
            if name not in internal:
                raise ValueError(f"Hedge: internal value for '{name}', which is a leaf (its value is the class map's)")
        self.reject_val = -1 if reject_value is None else int(reject_value)
        used = {v for row, kids in zip(t.pixel_val, t.n_children) for v, k in zip(row, kids) if k == 0}
        used |= {int(v) for v in given.values()}
        if self.reject_val >= 0:
            used.add(self.reject_val)
        free = (v for v in range(256) if v not in used)
        self.values = {}
        for name in internal:
            if name in given:
                self.values[name] = int(given[name])
            else:
                v = next(free, None)
                if v is None:
                    raise ValueError(f"Hedge: no unused uint8 value is left for internal node '{name}'")
                self.values[name] = v
        self.stop_val = [[self.values[n] if t.n_children[L][c] else -1 for c, n in enumerate(names)]
                         for L, names in enumerate(t.names)]
        ops.check_hedge(self)
        self.unmet_levels = []
        self.value_names = {int(t.pixel_val[L][c]): n for n, (L, c) in where.items() if not t.n_children[L][c]}
        self.value_names.update({v: n for n, v in self.values.items()})
        if self.reject_val >= 0:
            self.value_names[self.reject_val] = "rejected"

    @property
    def node_names(self):
        """the tree's nodes in breadth-first channel order: the order of the `stops` cells (then "rejected", "nonfinite")"""
        return [n for names in self.tables.names for n in names]

    @classmethod
    def from_calibration(cls, scores, class_tree, class_map, min_accuracy, min_events=1, **kw):
        """One threshold per child level from the "top@L" rows of a Data.CalibrationScores (all its records summed; one
        device-to-host copy): for level L >= 1 the smallest bin edge k / n_bins such that the events of the bins >= k have
        pos / n >= min_accuracy and n >= min_events.  Level 0 keeps 0.  A level where no edge qualifies gets tau = 1.0 (the
        walk enters it only at full confidence) and is listed in `hedge.unmet_levels`.  **kw: internal_values, reject_value.

        What the fitted figure means: a top row only counts pixels whose ground truth HAS a node at that level (DESIGN.md
        section 22), so `min_accuracy` is the accuracy of the decoded level-L node among those pixels, not among all pixels
        that reach level L.  And an edge is exact only up to the records' quantisation: an event was binned by its
        probability rounded to the 2^-24 grid, so an event whose T_L lies within 2^-25 of k / n_bins (plus the device's own
        fp32 error, section 22) may sit on either side of the threshold that is fitted from it."""
        rows, n_bins = list(scores.names), int(scores.n_bins)
        hist = torch.as_tensor(scores.hist).sum(0).cpu().numpy().astype(np.int64)        # [rows, n_bins + 1, 4]
        nlevels = sum(1 for r in rows if r.startswith("top@"))
        if not 0.0 <= float(min_accuracy) <= 1.0:
            raise ValueError(f"Hedge.from_calibration: min_accuracy {min_accuracy} not in 0..1")
        taus, unmet = [0.0], []
        for L in range(1, nlevels):
            rec = hist[rows.index(f"top@{L}"), :n_bins]
            n, pos = rec[::-1, 0].cumsum()[::-1], rec[::-1, 1].cumsum()[::-1]            # events of the bins >= k
            ok = [k for k in range(n_bins) if n[k] >= max(int(min_events), 1) and int(pos[k]) / int(n[k]) >= float(min_accuracy)]
            if ok:
                taus.append(ok[0] / n_bins)
            else:
                taus.append(1.0)
                unmet.append(L)
        hedge = cls(class_tree, class_map, taus, **kw)
        hedge.unmet_levels = unmet
        return hedge
