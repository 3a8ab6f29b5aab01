"""Torch-CPU restatement of the partial-label targets (test infrastructure, not product).

include/hrseg.h ("partial labels") written out with the oracle's own tree helpers and tests/augment_ref's primitives, without
the product's bit tables: per node an `on` mask and an `unk` mask of the label image, the four-step channel rule, and for the
resized path the antialiased resize of the stacked `on` and `on | unk` masks, the 0.5 threshold, the nearest warp of both
thresholded sets with the fill of the chosen mode, and the encode."""
from __future__ import annotations

import numpy as np
import torch

from oracle.targets import is_leaf, level_order_names, node_masks, parent_map
from tests import augment_ref as R


def descendants(tree, name):
    """every node strictly below `name`"""
    par = parent_map(tree)
    out = []
    for n in level_order_names(tree):
        a = par[n]
        while a is not None and a != name:
            a = par[a]
        if a == name:
            out.append(n)
    return out


def node_sets(tree, label, name2pix, internal_values=None, ignore_values=()):
    """name -> bool mask, twice: where the node is on, where it is unknown (every node of the tree)"""
    label = np.asarray(label)
    par = parent_map(tree)
    names = level_order_names(tree)
    on = {n: m.copy() for n, m in node_masks(tree, label, name2pix).items()}
    unk = {n: np.zeros(label.shape, dtype=bool) for n in names}
    for n, v in (internal_values or {}).items():
        hit = label == int(v)
        a = n
        while a is not None:
            on[a] |= hit
            a = par[a]
        for d in descendants(tree, n):
            unk[d] |= hit
    for v in ignore_values:
        hit = label == int(v)
        for n in names:
            unk[n] |= hit
    return on, unk


def emitted(tree, model_type):
    """(channel names, channel of the direct parent or -1) as the targets are laid out"""
    names = level_order_names(tree)
    emit = names if model_type == 1 else [n for n in names if is_leaf(tree, n)]
    par = parent_map(tree)
    idx = {n: i for i, n in enumerate(emit)}
    return emit, [(-1 if (model_type == 0 or par[n] is None) else idx[par[n]]) for n in emit]


def encode_sets(on, unk, parent):
    """bool [C, ...] x 2 -> fp32 [C, ...]: 1 on; else -1 unknown; else 0 for a root / inside the parent; else -1"""
    out = torch.empty(on.shape, dtype=torch.float32)
    for c, p in enumerate(parent):
        zero = torch.ones_like(on[c]) if p < 0 else on[p]
        out[c] = torch.where(on[c], 1.0, torch.where(unk[c], -1.0, torch.where(zero, 0.0, -1.0)))
    return out


def stacks(tree, label, class_map, model_type, internal_values, ignore_values):
    emit, parent = emitted(tree, model_type)
    on, unk = node_sets(tree, label, R.name2pix(class_map), internal_values, ignore_values)
    return (torch.from_numpy(np.stack([on[n] for n in emit])), torch.from_numpy(np.stack([unk[n] for n in emit])), parent)


def encode(label, tree, class_map, model_type, internal_values=None, ignore_values=()):
    """label [B,H,W] uint8 -> [B,C,H,W] fp32 targets (no resize)"""
    out = []
    for lab in np.asarray(label):
        on, unk, parent = stacks(tree, lab, class_map, model_type, internal_values, ignore_values)
        out.append(encode_sets(on, unk, parent))
    return torch.stack(out)


def augment_targets(label_u8, S, tree, class_map, model_type, internal_values=None, ignore_values=(), p=None,
                    target_antialias=True, fill="reference"):
    """one sample's targets through resize, threshold, flips, warp and encode.  p: None = eval, else this sample's draws
    (augment_ref.sample_dict).  Returns y [C,S,S], the exclusion mask [S,S] (pixels where a coverage of either stack lies
    within 1e-5 of 0.5, plus augment_ref's warp ties) and the near-0.5 part of that mask alone."""
    on, unk, parent = stacks(tree, label_u8, class_map, model_type, internal_values, ignore_values)
    cov_on = R.resize(on.float(), S, antialias=target_antialias)
    cov_may = R.resize((on | unk).float(), S, antialias=target_antialias)
    near = (((cov_on - 0.5).abs() < 1e-5) | ((cov_may - 0.5).abs() < 1e-5)).any(dim=0)
    ON, MAY = (cov_on >= 0.5).float(), (cov_may >= 0.5).float()
    tie = torch.zeros(S, S, dtype=torch.bool)
    if p is not None:
        if p["hflip"]:
            ON, MAY, near = ON.flip(-1), MAY.flip(-1), near.flip(-1)
        if p["vflip"]:
            ON, MAY, near = ON.flip(-2), MAY.flip(-2), near.flip(-2)
        if p["affine"]:
            mat = R.inverse_affine_matrix(p["angle"], (p["tx"], p["ty"]), p["scale"], p["shear"])
            C = ON.shape[0]
            top0 = float(cov_on[0].max())
            if fill == "ignore":
                fill_on, fill_may = [0.0] * C, [1.0] * C
            else:
                fill_on = [1.0 if top0 >= 0.5 else 0.0] + [0.0] * (C - 1)
                fill_may = fill_on
            ON, grid = R.affine_nearest(ON, mat, fill_on)
            MAY, _ = R.affine_nearest(MAY, mat, fill_may)
            ix, iy = R.source_coords(grid, S)
            tie = (((ix - ix.floor()) - 0.5).abs() < 1e-4) | (((iy - iy.floor()) - 0.5).abs() < 1e-4)
            nw, _ = R.affine_nearest(near[None].float(), mat, [1.0 if (fill != "ignore" and abs(top0 - 0.5) < 1e-5) else 0.0])
            near = nw[0] > 0.5
    ON, MAY = ON > 0.5, MAY > 0.5
    return encode_sets(ON, MAY & ~ON, parent), near | tie, near
