"""Border weights for the CE term: the U-Net weight map w(x) = 1 + w0 exp(-d(x)^2 / (2 sigma^2)), d = the distance to the
nearest border of the level's label map, computed on the device from the level's target planes after augmentation and
mixing (hrseg_border_weights; the semantics are stated once, in include/hrseg.h under "border weights"; DESIGN.md section
27).  ``CrossEntropyLoss(border=BorderWeights(...))`` switches it on; the map then weighs the CE of that level per pixel
(``fused_ce_dice(pixel_weight=)``), the Dice term is untouched.
"""
from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np
import torch

from .. import ops

MAX_RADIUS = ops.BORDER_MAX_RADIUS


def _w0(value):
    v = float(value)
    if not (math.isfinite(v) and v >= 0.0):
        raise ValueError(f"w0 must be finite and >= 0, got {value!r}")
    return v


def _sigma(value):
    v = float(value)
    if not (math.isfinite(v) and v > 0.0):
        raise ValueError(f"sigma must be finite and > 0, got {value!r}")
    return v


def _radius(value, sigma):
    if value is None:
        return min(MAX_RADIUS, int(math.ceil(3.0 * sigma)))
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or not 1 <= int(value) <= MAX_RADIUS:
        raise ValueError(f"radius must be an integer in 1..{MAX_RADIUS}, got {value!r}")
    return int(value)


def border_table(w0, sigma, radius):
    """the host table of radius^2 + 1 floats: lut[0] = 1, lut[k] = (float)(1 + w0 exp(-k / (2 sigma^2))) evaluated in fp64"""
    k = np.arange(radius * radius + 1, dtype=np.float64)
    lut = (1.0 + np.float64(w0) * np.exp(-k / (2.0 * np.float64(sigma) ** 2))).astype(np.float32)
    lut[0] = np.float32(1.0)
    return lut


class BorderOptions(NamedTuple):
    """What a border weight map is computed with, by value into the recorded calls: travels beside LossOptions and
    OhemOptions in the key of a recorded step."""
    w0: float
    sigma: float
    radius: int

    @classmethod
    def from_ce(cls, ce_fn=None):
        """the border options of a CrossEntropyLoss; None = off (no loss object, or border=None)"""
        bw = None if ce_fn is None else getattr(ce_fn, "border", None)
        return None if bw is None else bw.options


class BorderWeights:
    """bw(t) -> the [B,H,W] weight map of the target planes t [B,C,H,W] (-1 / 0 / 1) on t's device, made of ops calls only
    (one hrseg_border_weights call; the table is built once per device).  ``radius``: how far a border is looked for,
    default min(32, ceil(3 sigma)); beyond it the weight is 1.  ``labels`` / ``last`` are the label map and the weight map
    of the latest call (device tensors, no sync)."""

    def __init__(self, w0=10.0, sigma=5.0, radius=None):
        self.w0, self.sigma = _w0(w0), _sigma(sigma)
        self.radius = _radius(radius, self.sigma)
        self.labels = self.last = None
        self._luts = {}

    @property
    def options(self):
        return BorderOptions(self.w0, self.sigma, self.radius)

    def table(self):
        return border_table(self.w0, self.sigma, self.radius)

    def lut(self, device):
        """the table on `device` (copied there once)"""
        key = str(device)
        lut = self._luts.get(key)
        if lut is None:
            lut = self._luts[key] = torch.from_numpy(self.table()).to(device)
        return lut

    def __call__(self, t):
        self.labels, self.last = ops.border_weights(t if t.is_contiguous() else t.contiguous(), self.radius, self.lut(t.device))
        return self.last

    def __repr__(self):
        return f"BorderWeights(w0={self.w0}, sigma={self.sigma}, radius={self.radius})"
