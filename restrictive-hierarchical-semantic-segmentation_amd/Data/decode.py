"""Device output pipeline: per-level logits at network size -> one label map per source image, at the source's own
size, in the pixel values of class_map.csv -- the format `TargetEncoder` / `DeviceAugment` read.  Kernel: csrc/decode.hip.

The decode is restrictive and top-down: arg-max over the level-0 channels, then at every level only the child group of
the node chosen above it competes.  The model composes a child's probability as P_parent * softmax_group(z) (the
log(P_parent + eps) bias is constant inside a group), so the arg-max of the group's logits is the arg-max of the
model's own probabilities and the decoded path is always a path of the tree -- which the reference's independent
per-level arg-max does not guarantee.  The logits are resampled bilinearly (F.interpolate, align_corners=False) to each
image's own H x W inside the kernel; no full-size fp32 tensor exists at any point.

`decode_views` does the same on the mean logit of several views of the batch (mirrored and/or rescaled network inputs:
test-time augmentation, predictEval.TestTimeAugment), still in one launch (csrc/decode_views.hip).

`decode_windows` decodes the logits of overlapping network-size windows of each image (sliding-window inference,
predictEval.SlidingWindow), blended where they overlap, in one launch and without a canvas-size tensor (csrc/windows.hip);
`plan_windows` lays the windows out on the host.

`decode_hedged` is `decode` with a policy (Data/hedge.py): where the composed confidence of the path falls below a node's
threshold the pixel keeps the byte of the node above it, and the call counts how many pixels ended on every node
(csrc/decode_hedged.hip) -> HedgedLabels.

The tables are built on the host without a GPU; only `decode` / `decode_views` / `decode_windows` / `decode_hedged` launch.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from .. import ops
from .._lib import require_gpu
from ..utils.hierarchy import TreeIndex
from .dataset import TargetEncoder


class DecodeTables:
    """The tree as hrseg_decode_labels reads it, per level and channel: `first_child` (channel of the first child at the
    next level, -1 for leaves), `n_children` (0 for leaves), `pixel_val` (leaves; -1 for parents); `C` channels per
    level, `names` per level, `root_softmax` (flat models: the level-0 confidence is a soft-max, not a sigmoid)."""

    def __init__(self, C, first_child, n_children, pixel_val, root_softmax, names=None):
        self.C = [int(n) for n in C]
        self.first_child = [list(r) for r in first_child]
        self.n_children = [list(r) for r in n_children]
        self.pixel_val = [list(r) for r in pixel_val]
        self.root_softmax = bool(root_softmax)
        self.names = names


def build_tables(class_tree, class_map, model_type=1) -> DecodeTables:
    """class_tree + class_map (any form TargetEncoder accepts) -> DecodeTables.  model_type 1: one level per tree depth,
    channels in breadth-first order; model_type 0: one level over the leaves.  KeyError for a leaf without a pixel value,
    ValueError for one outside uint8, NotImplementedError when a parent's children are not consecutive channels."""
    name2pix = TargetEncoder._name2pix(class_map)
    index = TreeIndex(class_tree)

    def pixel(n):
        if n not in name2pix:
            raise KeyError(f"Class '{n}' not found in class_map.")
        v = int(name2pix[n])
        if not 0 <= v <= 255:
            raise ValueError(f"pixel value {v} of class '{n}' does not fit a uint8 label image")
        return v

    if int(model_type) == 0:
        leaves = index.leaf_names
        tables = DecodeTables([len(leaves)], [[-1] * len(leaves)], [[0] * len(leaves)], [[pixel(n) for n in leaves]], True,
                              [leaves])
    else:
        levels = index.levels
        first, count, pix = [], [], []
        for L, names in enumerate(levels):
            f, c, p = [], [], []
            for n in names:
                kids = index.children[n]
                if not kids:
                    f.append(-1)
                    c.append(0)
                    p.append(pixel(n))
                    continue
                chans = [levels[L + 1].index(k) for k in kids]
                if chans != list(range(chans[0], chans[0] + len(chans))):
                    raise NotImplementedError("children of a parent must occupy consecutive channels (BFS channel order)")
                f.append(chans[0])
                c.append(len(chans))
                p.append(-1)
            first.append(f)
            count.append(c)
            pix.append(p)
        tables = DecodeTables([len(n) for n in levels], first, count, pix, False, [list(n) for n in levels])
    ops.check_decode_tables(tables)
    return tables


def label_desc(sizes) -> torch.Tensor:
    """[(H, W), ...] -> the [B,4] int64 host descriptor table of a densely packed batch of label maps"""
    rows, off = [], 0
    for H, W in sizes:
        rows.append([off, int(H), int(W), 1])
        off += int(H) * int(W)
    return torch.tensor(rows, dtype=torch.int64).reshape(-1, 4)


def window_origins(n, S, stride):
    """origins of the windows of size S along a canvas axis of length n >= S: [0] where n == S, else
    ceil((n - S) / stride) + 1 origins min(i * stride, n - S) -- the last window is shifted back to end at the edge"""
    n, S, stride = int(n), int(S), int(stride)
    if n < S or stride < 1:
        raise ValueError(f"window_origins: axis of {n} for windows of {S}, stride {stride}")
    if n == S:
        return [0]
    return [min(i * stride, n - S) for i in range(-(-(n - S) // stride) + 1)]


def window_profile(S, blend="hann"):
    """the blend weight of a window's rows and columns, S strictly positive fp32 entries: "hann" =
    float32(0.5 - 0.5 cos(2 pi (i + 0.5) / S)) evaluated in fp64, "uniform" = all ones"""
    S = int(S)
    if blend == "uniform":
        return torch.ones(S, dtype=torch.float32)
    if blend != "hann":
        raise ValueError(f"window_profile: blend '{blend}', supported 'hann' and 'uniform'")
    i = torch.arange(S, dtype=torch.float64)
    return (0.5 - 0.5 * torch.cos(2.0 * math.pi * (i + 0.5) / S)).to(torch.float32)


class WindowPlan:
    """The windows of a batch as hrseg_window_crops / hrseg_decode_windows read them (include/hrseg.h), on the host:
    `wdesc` [B,8] int64 (Hc, Wc, ny, nx, n0, offset of the image's origins, 0, 0), `origins` int32 (per image ny row origins
    then nx column origins), `nwindows`, `S`.  Any tables that pass ops.check_window_plan are accepted, not only
    `plan_windows`'."""

    def __init__(self, wdesc, origins, nwindows, S):
        self.wdesc = torch.as_tensor(wdesc, dtype=torch.int64).reshape(-1, 8)
        self.origins = torch.as_tensor(origins, dtype=torch.int32).reshape(-1)
        self.nwindows, self.S = int(nwindows), int(S)

    def __len__(self):
        return self.wdesc.shape[0]

    def canvas(self, m):
        return tuple(self.wdesc[m, :2].tolist())

    def axes(self, m):
        """(row origins, column origins) of image m"""
        _, _, ny, nx, _, oo, _, _ = self.wdesc[m].tolist()
        o = self.origins[oo:oo + ny + nx].tolist()
        return o[:ny], o[ny:]

    def first_window(self, m):
        return int(self.wdesc[m, 4])


def plan_windows(canvases, S, stride) -> WindowPlan:
    """[(Hc, Wc), ...] -> the WindowPlan of window_origins along both axes of every canvas: the windows of an image are the
    tensor product rows x columns, row-major, numbered from the image's n0 on"""
    rows, org, n0 = [], [], 0
    for Hc, Wc in canvases:
        ys, xs = window_origins(Hc, S, stride), window_origins(Wc, S, stride)
        rows.append([int(Hc), int(Wc), len(ys), len(xs), n0, len(org), 0, 0])
        org += ys + xs
        n0 += len(ys) * len(xs)
    return WindowPlan(torch.tensor(rows, dtype=torch.int64).reshape(-1, 8), torch.tensor(org, dtype=torch.int32), n0, S)


class RaggedLabels:
    """A decoded batch: `labels` packed uint8 (device), `confidence` packed fp32 (device) or None, `desc` [B,4] int64
    (device) and `desc_host` (byte offset, H, W, 1)."""

    def __init__(self, labels, confidence, desc, desc_host):
        self.labels, self.confidence, self.desc, self.desc_host = labels, confidence, desc, desc_host

    def __len__(self):
        return self.desc_host.shape[0]

    def _split(self, flat):
        return [flat[off:off + H * W].reshape(H, W) for off, H, W, _ in self.desc_host.tolist()]

    def unpack(self):
        """list of H x W uint8 numpy arrays (views of ONE device-to-host copy)"""
        return self._split(self.labels.cpu().numpy())

    def unpack_confidence(self):
        """list of H x W fp32 numpy arrays, or None when the decode did not keep the confidence"""
        return None if self.confidence is None else self._split(self.confidence.cpu().numpy())


class HedgedLabels(RaggedLabels):
    """A hedged decode (`DeviceDecode.decode_hedged`): a RaggedLabels whose maps may hold internal nodes' bytes and the
    reject value (`hedge.value_names`), plus `stops` [B, sum C + 2] int64 (device): the pixels ended per tree node in
    breadth-first order, then "rejected", then "nonfinite" -- of this call, or of every call it was accumulated over."""

    def __init__(self, labels, confidence, desc, desc_host, stops, hedge):
        super().__init__(labels, confidence, desc, desc_host)
        self.stops, self.hedge = stops, hedge

    def summary(self):
        """the counters summed over the batch, from ONE device-to-host copy: dict(
        pixels: all pixels counted;
        ended {node: pixels whose label is that node's byte};
        abstained {internal node: ended[node] / (ended[node] + pixels ended below it)} -- of the pixels that entered the
          node, the share that the hedge kept there (NaN where none entered);
        coverage [per level]: the share of the pixels whose path was not cut before it settled on a node of that level --
          1 - rejected / pixels at level 0, then minus the pixels the hedge stopped on the level above (a pixel whose path
          ends in a shallower LEAF is not cut);
        rejected, nonfinite: pixels)"""
        t = self.hedge.tables
        host = self.stops.sum(0).cpu().tolist()
        nodes = sum(t.C)
        cell0 = [sum(t.C[:L]) for L in range(len(t.C))]
        total = sum(host[:nodes]) + host[nodes]
        below = [[0] * n for n in t.C]                      # pixels ended on the node or anywhere below it
        for L in range(len(t.C) - 1, -1, -1):
            for c in range(t.C[L]):
                kids = range(t.first_child[L][c], t.first_child[L][c] + t.n_children[L][c]) if t.n_children[L][c] else ()
                below[L][c] = host[cell0[L] + c] + sum(below[L + 1][k] for k in kids)
        ended, abstained, coverage, cut = {}, {}, [], host[nodes]
        for L, names in enumerate(t.names):
            coverage.append(1.0 - cut / total if total else float("nan"))
            for c, name in enumerate(names):
                ended[name] = host[cell0[L] + c]
                if t.n_children[L][c]:
                    abstained[name] = host[cell0[L] + c] / below[L][c] if below[L][c] else float("nan")
                    cut += host[cell0[L] + c]
        return dict(pixels=total, ended=ended, abstained=abstained, coverage=coverage, rejected=host[nodes],
                    nonfinite=host[nodes + 1])


class DeviceDecode:
    """`dec = DeviceDecode(class_tree, class_map, model_type); out = dec.decode(output_logits, desc, desc_host)` with
    the models' `output_logits` (a list of per-level [B,C_L,S,S] tensors, or the flat model's single tensor) and the label
    descriptors of the wanted sizes (`label_desc`, or a RaggedBatch's `ldesc`) -> RaggedLabels."""

    def __init__(self, class_tree, class_map, model_type=1):
        self.class_tree, self.model_type = class_tree, int(model_type)
        self.tables = build_tables(class_tree, class_map, self.model_type)
        self.leaf_values = sorted(v for row, kids in zip(self.tables.pixel_val, self.tables.n_children)
                                  for v, k in zip(row, kids) if k == 0)

    @staticmethod
    def _descriptors(desc, desc_host, logits):
        """(desc on the device of the first logit tensor, desc_host): a host table is its own host copy"""
        if desc_host is None:
            if desc.is_cuda:
                raise ValueError("a device descriptor table needs its host copy (desc_host)")
            desc_host = desc
        if logits and torch.is_tensor(logits[0]):
            desc = desc.to(logits[0].device, non_blocking=True)
        return desc, desc_host

    def decode(self, output_logits, desc, desc_host=None, want_confidence=False) -> RaggedLabels:
        require_gpu()
        logits = [output_logits] if torch.is_tensor(output_logits) else list(output_logits)
        desc, desc_host = self._descriptors(desc, desc_host, logits)
        labels, conf = ops.decode_labels(logits, self.tables, desc, desc_host, want_confidence)
        return RaggedLabels(labels, conf, desc, desc_host)

    def decode_sizes(self, output_logits, sizes, want_confidence=False) -> RaggedLabels:
        """decode to a densely packed batch of the given [(H, W), ...]"""
        return self.decode(output_logits, label_desc(sizes), None, want_confidence)

    def decode_hedged(self, output_logits, hedge, desc, desc_host=None, want_confidence=False, out=None) -> HedgedLabels:
        """`decode` that stops at the parent where the child is unsure: `hedge` is a Data.Hedge of this decoder's tree
        (model_type 1 only).  With all-zero thresholds the maps and the confidence are `decode`'s, bit for bit.  out: a
        HedgedLabels of an earlier call with the same batch size, whose counters this call adds to (the returned object
        shares them): a dataset total accumulates in place.  One launch (csrc/decode_hedged.hip)."""
        require_gpu()
        if self.model_type == 0:
            raise ValueError("decode_hedged: model_type 0 (a flat model) has no path to shorten")
        if hedge.tables.names != self.tables.names or hedge.tables.pixel_val != self.tables.pixel_val:
            raise ValueError("decode_hedged: the hedge was built for another class tree or class map")
        logits = [output_logits] if torch.is_tensor(output_logits) else list(output_logits)
        desc, desc_host = self._descriptors(desc, desc_host, logits)
        labels, conf, stops = ops.decode_hedged(logits, hedge, desc, desc_host, want_confidence,
                                                None if out is None else out.stops)
        return HedgedLabels(labels, conf, desc, desc_host, stops, hedge)

    def decode_hedged_sizes(self, output_logits, hedge, sizes, want_confidence=False, out=None) -> HedgedLabels:
        """decode_hedged to a densely packed batch of the given [(H, W), ...]"""
        return self.decode_hedged(output_logits, hedge, label_desc(sizes), None, want_confidence, out)

    def decode_views(self, views, desc, desc_host=None, want_confidence=False) -> RaggedLabels:
        """test-time augmentation: `views` is a list of (output_logits, flags), each the logits of the same batch as the
        network saw it mirrored by flags (0, ops.VIEW_HFLIP, ops.VIEW_VFLIP or both) and resized to the view's own
        S_v x S_v; the mean logit of the views (each flipped back and resampled to the image's size) is decoded as
        `decode` decodes one set of logits.  One launch (csrc/decode_views.hip)."""
        require_gpu()
        views = [(([z] if torch.is_tensor(z) else list(z)), f) for z, f in views]
        desc, desc_host = self._descriptors(desc, desc_host, views[0][0] if views else [])
        labels, conf = ops.decode_views(views, self.tables, desc, desc_host, want_confidence)
        return RaggedLabels(labels, conf, desc, desc_host)

    def decode_views_sizes(self, views, sizes, want_confidence=False) -> RaggedLabels:
        """decode_views to a densely packed batch of the given [(H, W), ...]"""
        return self.decode_views(views, label_desc(sizes), None, want_confidence)

    def decode_windows(self, output_logits, plan, profile, desc, desc_host=None, want_confidence=False) -> RaggedLabels:
        """sliding-window inference: `output_logits` are the logits of the plan's N windows ([N,C_L,S,S] per level, window
        order of the WindowPlan), `profile` the blend weights (`window_profile`); the windows' blend on each image's canvas is
        resampled to the wanted sizes and decoded as `decode` decodes one set of logits.  One launch (csrc/windows.hip)."""
        require_gpu()
        logits = [output_logits] if torch.is_tensor(output_logits) else list(output_logits)
        desc, desc_host = self._descriptors(desc, desc_host, logits)
        labels, conf = ops.decode_windows(logits, self.tables, plan, profile, desc, desc_host, want_confidence)
        return RaggedLabels(labels, conf, desc, desc_host)

    def decode_windows_sizes(self, output_logits, plan, profile, sizes, want_confidence=False) -> RaggedLabels:
        """decode_windows to a densely packed batch of the given [(H, W), ...]"""
        return self.decode_windows(output_logits, plan, profile, label_desc(sizes), None, want_confidence)


def pack_images(images):
    """list of uint8 HxW / HxWx3 arrays -> (packed uint8 tensor, [B,4] int64 descriptors), on the host"""
    flat, rows, off = [], [], 0
    for img in images:
        a = torch.as_tensor(np.ascontiguousarray(img))
        if a.dtype != torch.uint8:
            raise TypeError("sources must be uint8")
        if a.dim() == 3 and a.shape[2] == 1:
            a = a[:, :, 0]
        if not (a.dim() == 2 or (a.dim() == 3 and a.shape[2] == 3)):
            raise ValueError(f"image of shape {tuple(a.shape)}: expected HxW or HxWx3")
        rows.append([off, a.shape[0], a.shape[1], 1 if a.dim() == 2 else 3])
        flat.append(a.reshape(-1))
        off += flat[-1].numel()
    return torch.cat(flat), torch.tensor(rows, dtype=torch.int64)
