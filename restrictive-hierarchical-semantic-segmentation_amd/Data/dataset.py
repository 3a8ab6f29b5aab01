"""Label image -> model targets on the GPU (the input side of the train step).

Mirror of the target preparation in the reference's `SegDataset` (Data/dataset.py):
`separate_masks`/`traverse_tree` (:41-124, per-node masks, parents = OR of their children, emitted
in level order; leaves only when model_type == 0) followed by `process_ignore_values` (:227-265,
ternary {1, 0, -1} relative to the direct parent) -- for label images that are already at the
training resolution.  The reference does this per sample on the CPU inside the DataLoader with one
full-size mask image per node; here the whole batch is ONE kernel (`hrseg_encode_targets`): a
256-entry bit table maps a pixel value to the set of nodes it switches on, 1 byte read and 4*C bytes
written per pixel, so the label map can travel to the device as uint8 (C*4 times less PCIe traffic
than the float target tensor).

Label maps may also hold an ignore byte and the bytes of internal nodes ("partial labels": what hedged decode writes, and
what cheaper annotation higher up the tree looks like).  `build_target_luts` then fills a second table, the channels a
byte says nothing about, and the encoder launches `hrseg_encode_targets_partial`; include/hrseg.h states the semantics.

Image decoding, resizing and augmentation (dataset.py:397-447, dataloaders.py) stay outside the path.
"""
from __future__ import annotations

import torch

from .. import ops
from .._lib import require_gpu
from ..utils.hierarchy import level_order_names, _find


def _name2pix(class_map):
    if isinstance(class_map, dict):
        items = class_map.items()
    elif hasattr(class_map, "iterrows"):
        items = ((row["class_name"], row["pixel_val"]) for _, row in class_map.iterrows())
    else:
        items = ((row["class_name"], row["pixel_val"]) for row in class_map)
    out = {}
    for name, v in items:
        if v is None or (isinstance(v, str) and v.strip().lower() in ("none", "nan", "")):
            continue
        if isinstance(v, float) and v != v:
            continue
        out[name] = int(float(v))
    return out


def build_target_luts(class_tree, class_map, model_type, internal_values=None, ignore_values=()):
    """-> (names, parent, on_lut, unk_lut): the emitted channel names (every node breadth first for model_type 1, the leaves
    for 0), the channel of every channel's direct parent (-1: a root, and every channel in flat mode) and the two 256-entry
    bit tables, as Python ints, that hrseg_encode_targets[_partial] and hrseg_augment_targets[_partial] read.  Host only.

    internal_values: {internal node name: byte}, the form of `Hedge.values`; ignore_values: bytes of pixels that take no part
    in loss or gradient.  What a byte of either kind means is stated once, in include/hrseg.h ("partial labels").
    KeyError for a leaf the class map does not have (as the reference); ValueError, naming the classes, for a value outside
    0..255, a name that is no internal node and a byte that an internal node or an ignore value shares with anything else
    (two leaves of one byte stay what they were: a pixel that is both)."""
    model_type = int(model_type)
    name2pix = _name2pix(class_map)
    order = level_order_names(class_tree)
    leaf = {n: not _find(class_tree, n) for n in order}
    names = order if model_type == 1 else [n for n in order if leaf[n]]
    if len(names) > 64:
        raise ValueError("TargetEncoder supports at most 64 target channels")
    chan = {n: i for i, n in enumerate(names)}

    up = {}

    def link(node, p):
        for k, v in node.items():
            up[k] = p
            if isinstance(v, dict) and v:
                link(v, k)
    link(class_tree, None)
    parent = [(-1 if (model_type == 0 or up[n] is None) else chan[up[n]]) for n in names]

    def chain(n):                                   # the channels of n and its ancestors
        bits = 0
        while n is not None:
            if n in chan:
                bits |= 1 << chan[n]
            n = up[n]
        return bits

    def below(n):                                   # the channels strictly below n
        bits = 0
        for k in _find(class_tree, n):
            bits |= ((1 << chan[k]) if k in chan else 0) | below(k)
        return bits

    on_lut, unk_lut = [0] * 256, [0] * 256
    owner = {}                                      # byte -> what an internal node or ignore value would collide with
    for n in order:
        if not leaf[n]:
            continue
        if n not in name2pix:
            raise KeyError(f"Class '{n}' not found in class_map.")      # as dataset.py:62-64
        v = int(name2pix[n])
        if not 0 <= v <= 255:
            raise ValueError(f"pixel value {v} of class '{n}' does not fit a uint8 label image")
        on_lut[v] |= chain(n)                       # the leaf switches on itself and all its ancestors
        owner.setdefault(v, f"class '{n}'")
    for n, v in dict(internal_values or {}).items():
        if n not in leaf:
            raise ValueError(f"internal value for '{n}', which is no node of the class tree")
        if leaf[n]:
            raise ValueError(f"internal value for '{n}', which is a leaf (its value is the class map's), not an internal node")
        if int(v) != v or not 0 <= int(v) <= 255:
            raise ValueError(f"value {v} of internal node '{n}' does not fit a uint8 label image")
        v = int(v)
        if v in owner:
            raise ValueError(f"value {v} of internal node '{n}' is already the value of {owner[v]}")
        owner[v] = f"internal node '{n}'"
        on_lut[v], unk_lut[v] = chain(n), below(n)
    for v in ignore_values:
        if int(v) != v or not 0 <= int(v) <= 255:
            raise ValueError(f"ignore value {v} does not fit a uint8 label image")
        v = int(v)
        if v in owner:
            raise ValueError(f"ignore value {v} is already the value of {owner[v]}")
        owner[v] = f"ignore value {v}"
        on_lut[v], unk_lut[v] = 0, (1 << len(names)) - 1
    return names, parent, on_lut, unk_lut


def _lut_tensor(lut, device):
    """bit patterns as int64 (two's complement for bit 63)"""
    return torch.tensor([x - (1 << 64) if x >= (1 << 63) else x for x in lut], dtype=torch.int64, device=device)


class TargetEncoder:
    """`enc = TargetEncoder(class_tree, class_map, model_type); target = enc(label_u8)`.

    class_tree: the nested dict of class_tree_*.json; class_map: the reference's class_map.csv as a
    pandas DataFrame, a list of row dicts, or a {class_name: pixel_val} dict (parents have no value);
    model_type 1 = hierarchical ternary targets for every node, 0 = one-hot over the leaves.

    Partial labels (include/hrseg.h): internal_values {internal node name: byte} lets a label map say "this node, child
    unknown", ignore_values lists bytes of pixels that take no part in loss or gradient; with a `Hedge` h,
    `TargetEncoder(tree, cmap, 1, internal_values=h.values, ignore_values=[h.reject_val])` reads hedged maps.  With neither
    the object is what it was: one table, `hrseg_encode_targets`."""

    def __init__(self, class_tree: dict, class_map, model_type: int = 1, device="cuda", internal_values=None, ignore_values=()):
        require_gpu()
        self.class_tree, self.model_type = class_tree, int(model_type)
        ignore_values = tuple(ignore_values)
        self.names, self.parent, on, unk = build_target_luts(class_tree, class_map, model_type, internal_values, ignore_values)
        self.on_lut = _lut_tensor(on, device)
        self.partial = bool(internal_values) or len(ignore_values) > 0
        self.unk_lut = _lut_tensor(unk, device) if self.partial else None

    _name2pix = staticmethod(_name2pix)

    def __call__(self, label: torch.Tensor) -> torch.Tensor:
        """label [B,H,W] (or [H,W]) uint8 pixel values -> [B,C,H,W] fp32 targets on the device"""
        if label.dim() == 2:
            label = label[None]
        if label.dtype != torch.uint8:
            raise TypeError("label image must be uint8 pixel values")
        label = label.to(self.on_lut.device, non_blocking=True)
        if self.partial:
            return ops.encode_targets_partial(label, self.on_lut, self.unk_lut, self.parent)
        return ops.encode_targets(label, self.on_lut, self.parent)
