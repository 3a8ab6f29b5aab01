"""Evaluation-side level synthesis for flat (model_type 0) models on the MI355X path.

Call surface of the reference's predictEval.py helpers (:36-185): ``children_map``, ``bfs_order``, ``levels_bfs``,
``descendant_leaves``, ``get_parent_masks``, ``combine_levels``.  A flat model predicts leaf classes only; to
score it per hierarchy level the reference synthesises every parent channel as the union of its descendant
leaves ("any > 0") and stitches per-level tensors from leaf and parent channels.  Both steps are one HIP kernel
here (hrseg_combine_levels: per output channel a bit mask over the input channels and a copy/union flag); the
tree walks run over one shared index (utils/hierarchy.TreeIndex).  The per-batch body of predict() (:305-573) --
prediction prep, metrics, the PNG dump and metrics.csv -- is below; only the CLI / fold / dataset plumbing is out of scope.
"""
from __future__ import annotations

import math

import torch

from . import ops
from .Metrics.performance_metrics import METRIC_NAMES
from .utils.hierarchy import TreeIndex


def children_map(tree):
    """node -> list of direct children (empty for leaves), for every node of the nested dict (predictEval.py:36-47)"""
    return {name: list(kids) for name, kids in TreeIndex(tree).children.items()}


def bfs_order(tree):
    """node names breadth first (predictEval.py:49-58)"""
    return list(TreeIndex(tree).order)


def levels_bfs(tree):
    """names per depth, breadth first (predictEval.py:61-72)"""
    return [list(lvl) for lvl in TreeIndex(tree).levels]


def descendant_leaves(node, children, is_leaf):
    """leaves below `node` given a children map and a leaf predicate map (predictEval.py:74-83), depth first"""
    found, todo = [], [node]
    while todo:
        cur = todo.pop()
        if is_leaf[cur]:
            found.append(cur)
        else:
            todo.extend(reversed(children[cur]))
    return found


def _channel_mask(channels):
    m = 0
    for c in channels:
        m |= 1 << c
    return m


def get_parent_masks(in_out, target, tree, leaf_index):
    """([X], [Y], tree, {leaf name: channel}) -> ([parents of X], [parents of Y], parent names in BFS order);
    X, Y are [B, n_leaves, H, W]; a parent channel is 1 where any of its descendant leaves is > 0
    (predictEval.py:85-129; same exception types and messages)."""
    X, Y = in_out[0], target[0]
    n_ch = X.shape[1]
    index = TreeIndex(tree)
    parents = index.parent_names
    masks = []
    for p in parents:
        below = index.leaves[p]
        if not below:
            raise ValueError(f"Parent '{p}' has no descendant leaves.")
        unknown = [leaf for leaf in below if leaf not in leaf_index]
        if unknown:
            raise KeyError(f"Missing leaf_index entries for {unknown} (needed by parent '{p}').")
        idxs = [leaf_index[leaf] for leaf in below]
        if any(i < 0 or i >= n_ch for i in idxs):
            raise IndexError(f"Parent '{p}' has leaf indices out of bounds: {idxs} with C={n_ch}.")
        masks.append(_channel_mask(idxs))
    union = [1] * len(masks)
    return ([ops.combine_levels(X, None, masks, union).to(X.dtype)], [ops.combine_levels(Y, None, masks, union).to(Y.dtype)],
            parents)


def combine_levels(leaves_list, parents_list, tree: dict, leaf_order=None, parent_order=None):
    """([X_leaves], [X_parents], tree) -> one [B, C_level, H, W] tensor per depth, channels in BFS order, each a
    copy of its leaf or parent channel (predictEval.py:134-185; same KeyErrors)"""
    X_leaves, X_par = leaves_list[0], parents_list[0]
    B, n_leaf_ch, H, W = X_leaves.shape
    index = TreeIndex(tree)
    leaf_order = index.leaf_names if leaf_order is None else leaf_order
    parent_order = index.parent_names if parent_order is None else parent_order
    where = {n: i for i, n in enumerate(leaf_order)}
    where_parent = {n: n_leaf_ch + i for i, n in enumerate(parent_order)}
    absent = [n for n in index.leaf_names if n not in where]
    if absent:
        raise KeyError(f"leaf_order is missing leaves: {absent}")
    absent = [n for n in index.parent_names if n not in where_parent]
    if absent:
        raise KeyError(f"parent_order is missing parents: {absent}")
    where.update(where_parent)                      # input channel of every node: leaves first, parents behind them
    out = []
    for names in index.levels:
        copy_masks = [1 << where[n] for n in names]
        out.append(ops.combine_levels(X_leaves, X_par, copy_masks, [0] * len(copy_masks)).to(X_leaves.dtype))
    return out


# ----------------------------------------------------------------------------- predict(): batch body, loop, writers
def prediction_prep(output_logits, target, args, class_tree):
    """The per-batch prediction prep of the reference's predict() (predictEval.py:336-441) for one batch:
    (model logits, raw target [B, sum C, H, W]) -> (output_class per level, eval_targets per level), both zeroed where
    the level's target is -1.  Hierarchical models: soft-max -> arg-max -> one-hot per level (:426-432, one
    hrseg_predict_metrics launch per level).  Flat models: one-hot over the leaves, parents synthesised as the union of
    their descendant leaves and the per-level tensors stitched in BFS order (:381-386)."""
    from .train import split_targets
    if args.model_type == 0:
        logits = output_logits if torch.is_tensor(output_logits) else output_logits[0]
        # the leaf one-hot is NOT masked here: the reference synthesises the parents from the plain arg-max one-hot
        # (predictEval.py:361-386) and masks every level afterwards (:435-439) -- a parent's target is never -1, so its
        # prediction keeps the pixels whose LEAF target is -1.  (An all-zero target makes the kernel's mask a no-op.)
        onehot, _ = ops.predict_metrics(logits.detach(), ops.zeros(logits.shape, torch.float32, logits.device), child=False,
                                        mask_pred=True)
        index = TreeIndex(class_tree)
        name_to_index = {n: i for i, n in enumerate(index.leaf_names)}
        parent_class, parent_target, _ = get_parent_masks([onehot], [target], class_tree, name_to_index)
        output_class = combine_levels([onehot], parent_class, class_tree, index.leaf_names, index.parent_names)
        targets = combine_levels([target], parent_target, class_tree, index.leaf_names, index.parent_names)
        output_class = [torch.where(t == -1, torch.zeros_like(o), o) for o, t in zip(output_class, targets)]
    else:
        targets = split_targets(target, args)
        output_class = [ops.predict_metrics(z.detach(), t, child=(L > 0), mask_pred=True)[0]
                        for L, (z, t) in enumerate(zip(output_logits, targets))]
    eval_targets = [t.clamp_min(0.0) for t in targets]              # -1 -> 0 (:435-439)
    return output_class, eval_targets


def write_png_gray(path, mask_u8):
    """8-bit grayscale PNG of a [H, W] uint8 array (what the reference writes with cv2.imwrite, predictEval.py:512;
    cv2 is not a dependency here: the format is 30 lines of zlib + struct)"""
    import struct
    import zlib
    import numpy as np
    a = np.ascontiguousarray(mask_u8, dtype=np.uint8)
    h, w = a.shape
    raw = b"".join(b"\x00" + a[r].tobytes() for r in range(h))

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 0, 0, 0, 0)) +
                chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))


def save_prediction_images(output_class, save_dir, filename):
    """first image of the batch, one 0/255 PNG per class under <save_dir>/<class index>/<filename> (predictEval.py:500-513)"""
    import os
    k = 0
    for level in output_class:
        planes = (level[0] > 0.5).to(torch.uint8).mul_(255).cpu().numpy()
        for plane in planes:
            os.makedirs(os.path.join(save_dir, str(k)), exist_ok=True)
            write_png_gray(os.path.join(save_dir, str(k), filename), plane)
            k += 1


def save_label_maps(save_dir, names, ragged_labels):
    """one 8-bit grayscale PNG per image of a decoded batch (Data.decode.RaggedLabels), at the image's own size and in the
    pixel values of class_map.csv: <save_dir>/<name>; one device-to-host copy for the whole batch"""
    import os
    maps = ragged_labels.unpack()
    if len(names) != len(maps):
        raise ValueError(f"{len(names)} file names for {len(maps)} label maps")
    os.makedirs(save_dir, exist_ok=True)
    paths = []
    for name, m in zip(names, maps):
        paths.append(os.path.join(save_dir, name))
        write_png_gray(paths[-1], m)
    return paths


class TestTimeAugment:
    """Flip and multi-scale ensembling at inference (the reference's HRNet configuration names it TEST.FLIP_TEST /
    TEST.MULTI_SCALE / TEST.SCALE_LIST): the views a Predictor averages.  `views(size)` -> the ordered list of
    (S, flags): scale-major in the order given, S = int(round(size * scale)); within a scale the flags run 0, HFLIP,
    VFLIP, HFLIP|VFLIP as enabled (ops.VIEW_HFLIP = 1, ops.VIEW_VFLIP = 2).  At most ops.DECODE_MAX_VIEWS views."""
    __test__ = False        # (not a test class, whatever its name starts with)

    def __init__(self, hflip=True, vflip=False, scales=(1.0,)):
        self.hflip, self.vflip = bool(hflip), bool(vflip)
        self.scales = tuple(float(s) for s in scales)
        if not self.scales:
            raise ValueError("TestTimeAugment: no scales")
        if any(not s > 0.0 or s == float("inf") for s in self.scales):
            raise ValueError(f"TestTimeAugment: scales {self.scales} must be positive")
        if len(set(self.scales)) != len(self.scales):
            raise ValueError(f"TestTimeAugment: duplicate scale in {self.scales}")
        self.flags = [f for f in (0, ops.VIEW_HFLIP, ops.VIEW_VFLIP, ops.VIEW_HFLIP | ops.VIEW_VFLIP)
                      if (self.hflip or not f & ops.VIEW_HFLIP) and (self.vflip or not f & ops.VIEW_VFLIP)]
        if len(self.scales) * len(self.flags) > ops.DECODE_MAX_VIEWS:
            raise ValueError(f"TestTimeAugment: {len(self.scales)} scales x {len(self.flags)} flips are more than "
                             f"{ops.DECODE_MAX_VIEWS} views")

    def views(self, size):
        out = []
        for scale in self.scales:
            S = int(round(int(size) * scale))
            if not 1 <= S <= ops.DECODE_MAX_SIZE:
                raise ValueError(f"TestTimeAugment: scale {scale} of size {size} gives {S}, supported 1..{ops.DECODE_MAX_SIZE}")
            out.extend((S, f) for f in self.flags)
        return out


class SlidingWindow:
    """Tiled inference at (or near) the sources' own resolution: the network runs on overlapping network-size windows of a
    canvas of each image and the windows' logits are blended where they overlap (include/hrseg.h, sliding-window inference).
    `plan(sizes, S)` lays the windows out on the host (Data.decode.WindowPlan; no GPU):
      canvas of an image (H, W): Hc = max(S, int(round(H * scale))), Wc likewise -- an image smaller than a window is
        enlarged to one;
      stride = S - floor(overlap * S) with 0 <= overlap <= 0.5, so stride >= ceil(S / 2) and every canvas row or column is
        covered by at least 1 and at most 3 windows per axis (at most two regular origins lie in any half-open span of
        length S, plus the last window, which is shifted back to end at the edge);
      blend: "hann" (weights 0.5 - 0.5 cos(2 pi (i + 0.5) / S), strictly positive in fp32) or "uniform" (a plain mean).
    window_batch: windows per eval-mode forward of a Predictor."""

    def __init__(self, overlap=0.5, scale=1.0, blend="hann", window_batch=8):
        self.overlap, self.scale, self.blend, self.window_batch = float(overlap), float(scale), blend, int(window_batch)
        if not 0.0 <= self.overlap <= 0.5:
            raise ValueError(f"SlidingWindow: overlap {overlap} not in 0..0.5")
        if not (self.scale > 0.0 and self.scale != float("inf")):
            raise ValueError(f"SlidingWindow: scale {scale} must be positive")
        if blend not in ("hann", "uniform"):
            raise ValueError(f"SlidingWindow: blend '{blend}', supported 'hann' and 'uniform'")
        if self.window_batch < 1:
            raise ValueError(f"SlidingWindow: window_batch {window_batch} must be at least 1")

    def stride(self, S):
        return int(S) - int(math.floor(self.overlap * int(S)))

    def canvas(self, H, W, S):
        return max(int(S), int(round(H * self.scale))), max(int(S), int(round(W * self.scale)))

    def profile(self, S):
        from .Data.decode import window_profile
        return window_profile(S, self.blend)

    def plan(self, sizes, S):
        from .Data.decode import plan_windows
        S = int(S)
        if not 1 <= S <= ops.DECODE_MAX_SIZE:
            raise ValueError(f"SlidingWindow: window size {S}, supported 1..{ops.DECODE_MAX_SIZE}")
        plan = plan_windows([self.canvas(H, W, S) for H, W in sizes], S, self.stride(S))
        ops.check_window_plan("SlidingWindow", plan, len(plan), S)       # (e.g. more than 64 windows along an axis)
        return plan


class Predictor:
    """Deployment-side inference: `labels = Predictor(model, class_tree, class_map, args)(images)` with a list of ragged
    uint8 HxW / HxWx3 sources (or a RaggedBatch) -> RaggedLabels, one label map per source at the source's own size.
    Eval-mode resize + normalise to args.img_size on the device (ops.augment_image), the eval-mode forward, then the
    restrictive top-down decode of the logits (Data/decode.py).  args: img_size, model_type, model_select.
    The model runs in eval mode for the call and gets its previous mode back afterwards.  keep_logits=True keeps the
    latest call's logits (what the decode read) alive in `last_logits`; by default nothing of a batch is held.
    `scores = predictor.score(images, labels)` decodes at the ground-truth maps' own sizes instead and scores the maps
    against them on the device (Data/score.py) -> SourceScores; the decoded maps of that call stay in `last_labels`.
    tta=TestTimeAugment(...): per scale one eval-mode resize to S, ops.flip_views and ONE forward of all the scale's
    flip views as a batch (eval-mode BatchNorm uses the running statistics: samples do not interact), then one
    decode of the mean logit over all views (Data.DeviceDecode.decode_views); keep_logits=True then keeps
    `last_view_logits`, the list of (logits, flags) the decode read.  tta=None: exactly the calls described above.
    window=SlidingWindow(...): the windows are planned from the source sizes, cut by ONE ops.window_crops launch, run
    through eval-mode forwards of `window_batch` windows at a time (the last chunk shorter; eval-mode BatchNorm: windows do
    not interact) and their per-level logits, gathered into [N,C_L,S,S], are blended and decoded by ONE
    Data.DeviceDecode.decode_windows launch at the sizes asked for; keep_logits=True then keeps `last_window_logits` =
    (logits, plan).  window=None: exactly the calls described above.  window together with tta is refused.
    postprocess=Data.DevicePostprocess(...): the connected-component clean-up (Data/postprocess.py) of the decoded maps,
    behind whichever of the three decodes ran: the call returns the cleaned maps and `score` scores them.  Its min_area
    counts pixels of the map being produced -- the source's size in a call, the ground truth's size in `score` -- not
    pixels at network size.  postprocess=None: exactly the calls described above, no launch and no allocation more.
    `predictor.score_boundaries(images, labels)` decodes as `score` does and scores the outlines (Data/boundary.py);
    `predictor.score_instances(images, labels)` likewise matches the objects of the two maps (Data/instances.py);
    `predictor.score_calibration(images, labels)` scores the plain path's logits themselves: reliability, ECE and Brier per
    tree node (Data/calibration.py).
    hedge=Data.Hedge(...): the plain path decodes hedged (Data.DeviceDecode.decode_hedged): a pixel whose composed
    confidence falls below a node's threshold keeps the byte of the node above it (`hedge.value_names`).  The call returns
    a HedgedLabels (the maps plus the `stops` counters of the call), `score` scores the hedged maps with a DeviceScore
    built with `hedge.values` and `last_labels` is the HedgedLabels.  hedge together with tta, window or postprocess is
    refused (multi-view, window and cleaned-up hedged maps are not implemented), and so is model_type 0.  hedge=None:
    exactly the calls described above."""

    def __init__(self, model, class_tree, class_map, args, want_confidence=False, keep_logits=False, tta=None, window=None,
                 postprocess=None, hedge=None):
        from .Data.decode import DeviceDecode
        if hedge is not None:
            for what, on in (("tta", tta), ("window", window), ("postprocess", postprocess)):
                if on is not None:
                    raise ValueError(f"Predictor: hedge together with {what} is not supported")
            if int(args.model_type) == 0:
                raise ValueError("Predictor: hedge needs a hierarchical model; model_type 0 has no path to shorten")
        self.hedge = hedge
        self.model, self.class_tree, self.class_map, self.args = model, class_tree, class_map, args
        self.scorer, self.boundary_scorer, self.last_labels = None, None, None
        self.instance_scorer, self._instance_key = None, None
        self.calibration_scorer, self._calibration_key = None, None
        self.size = int(args.img_size)
        self.decoder = DeviceDecode(class_tree, class_map, args.model_type)
        self.want_confidence = bool(want_confidence)
        self.keep_logits = bool(keep_logits)
        self.last_logits = None
        self.tta, self.last_view_logits = tta, None
        if tta is not None:
            tta.views(self.size)                    # refuses sizes the decode cannot take before any image is seen
        self.postprocess = postprocess
        self.window, self.last_window_logits = window, None
        if window is not None:
            if tta is not None:
                raise ValueError("Predictor: window together with tta is not supported")
            self.window_profile = window.profile(self.size)
            window.plan([], self.size)              # refuses a window size the decode cannot take before any image is seen

    def __call__(self, images):
        return self._predict(images, None)

    @torch.no_grad()
    def score(self, images, labels=None, out=None, per_image=True):
        """images as for the call; labels: a list of uint8 HxW ground-truth maps in class_map pixel values (None: the
        RaggedBatch's own label maps) -> SourceScores of the maps decoded at the labels' sizes"""
        from .Data.score import DeviceScore
        if self.scorer is None:
            self.scorer = DeviceScore(self.class_tree, self.class_map, None if self.hedge is None else self.hedge.values)
        gt = self._ground_truth("Predictor.score", images, labels)
        self.last_labels = self._predict(images, [(H, W) for _, H, W, _ in gt[2].tolist()])
        return self.scorer.score(self.last_labels, gt, out, per_image)

    @torch.no_grad()
    def score_boundaries(self, images, labels=None, tolerance=2.0, percentile=95):
        """images and labels as for `score`: the maps are decoded at the labels' sizes through the same window / TTA /
        postprocess path (they stay in `last_labels`), then their outlines are scored against the labels' on the device
        (Data/boundary.py) -> BoundaryScores"""
        from .Data.boundary import DeviceBoundaryScore
        key = (float(tolerance), int(percentile))
        if self.boundary_scorer is None or (self.boundary_scorer.tolerance, self.boundary_scorer.percentile) != key:
            self.boundary_scorer = DeviceBoundaryScore(self.class_tree, self.class_map, tolerance, percentile)
        gt = self._ground_truth("Predictor.score_boundaries", images, labels)
        self.last_labels = self._predict(images, [(H, W) for _, H, W, _ in gt[2].tolist()])
        return self.boundary_scorer.score(self.last_labels, gt)

    @torch.no_grad()
    def score_instances(self, images, labels=None, level=0, things=None, connectivity=8, thresholds=(0.75, 0.9)):
        """images and labels as for `score`: the maps are decoded at the labels' sizes through the same window / TTA /
        postprocess path (they stay in `last_labels`), then their connected components are matched with the labels' on the
        device (Data/instances.py; the options are DeviceInstanceScore's, the scorer is kept per option set)
        -> InstanceScores"""
        from .Data.instances import DeviceInstanceScore
        key = (int(level), None if things is None else tuple(things), int(connectivity), tuple(float(t) for t in thresholds))
        if self.instance_scorer is None or self._instance_key != key:
            self.instance_scorer = DeviceInstanceScore(self.class_tree, self.class_map, level, things, connectivity, thresholds)
            self._instance_key = key
        gt = self._ground_truth("Predictor.score_instances", images, labels)
        self.last_labels = self._predict(images, [(H, W) for _, H, W, _ in gt[2].tolist()])
        return self.instance_scorer.score(self.last_labels, gt)

    @torch.no_grad()
    def score_calibration(self, images, labels=None, n_bins=15, temperature=None, out=None, per_image=False):
        """images and labels as for `score`: the eval-mode resize and forward of the plain path, then the logits -- not a
        decoded map -- are scored against the labels on the device (Data/calibration.py; the scorer is kept per (n_bins,
        temperature)) -> CalibrationScores; out accumulates a dataset total in place.  keep_logits=True keeps the logits in
        `last_logits`.  The kernel reads single-view logits: with tta or window set the call is refused.  postprocess does
        not matter to it (no map is produced)."""
        from . import train as T
        from .Data.calibration import DeviceCalibrationScore
        from .Data.decode import pack_images
        from .Data.loader import RaggedBatch
        for what, on in (("tta", self.tta), ("window", self.window)):
            if on is not None:
                raise ValueError(f"Predictor.score_calibration: {what} is set, but the calibration kernel reads single-view "
                                 "logits (multi-view and window variants are not implemented)")
        key = (int(n_bins), tuple(float(v) for v in temperature) if isinstance(temperature, (tuple, list)) else
               (None if temperature is None else float(temperature)))
        if self.calibration_scorer is None or self._calibration_key != key:
            self.calibration_scorer = DeviceCalibrationScore(self.class_tree, self.class_map, self.args.model_type, n_bins,
                                                             temperature)
            self._calibration_key = key
        gt = self._ground_truth("Predictor.score_calibration", images, labels)
        device = next(self.model.parameters()).device
        if isinstance(images, RaggedBatch):
            src, desc, desc_host = images.src, images.desc, images.desc_host
        else:
            src, desc_host = pack_images(images)
            desc = desc_host
        src, desc = src.to(device, non_blocking=True), desc.to(device, non_blocking=True)
        was_training = self.model.training
        self.model.eval()
        try:
            x = ops.augment_image(src, desc, desc_host, None, self.size, False)
            _, output_logits = T._model_call(self.model, x, self.args, self.class_tree)
        finally:
            self.model.train(was_training)
        if self.keep_logits:
            self.last_logits = output_logits
        return self.calibration_scorer.score(output_logits, gt, out, per_image)

    @staticmethod
    def _ground_truth(who, images, labels):
        """the (buffer, desc, desc_host) triple of the ground-truth maps of `score` / `score_boundaries`"""
        from .Data.decode import pack_images
        from .Data.loader import RaggedBatch
        if labels is None:
            if not isinstance(images, RaggedBatch) or images.label is None:
                raise ValueError(f"{who}: no ground-truth label maps")
            gt = (images.label, images.ldesc, images.ldesc_host)
        else:
            buf, host = pack_images(labels)
            if any(ch != 1 for _, _, _, ch in host.tolist()):
                raise ValueError(f"{who}: ground-truth label maps are single-channel uint8 images")
            gt = (buf, host, host)
        if gt[2].shape[0] != len(images):
            raise ValueError(f"{who}: {len(images)} images, {gt[2].shape[0]} label maps")
        return gt

    @torch.no_grad()
    def _predict(self, images, sizes):
        from . import train as T
        from .Data.decode import label_desc, pack_images
        from .Data.loader import RaggedBatch
        device = next(self.model.parameters()).device
        if isinstance(images, RaggedBatch):
            src, desc, desc_host = images.src, images.desc, images.desc_host
        else:
            src, desc_host = pack_images(images)
            desc = desc_host
        src, desc = src.to(device, non_blocking=True), desc.to(device, non_blocking=True)
        was_training = self.model.training
        self.model.eval()
        views, plan = [], None
        try:
            if self.window is not None:
                plan = self.window.plan([(H, W) for _, H, W, _ in desc_host.tolist()], self.size)
                x = ops.window_crops(src, desc, desc_host, plan, self.size)
                chunks = []
                for i in range(0, plan.nwindows, self.window.window_batch):
                    _, z = T._model_call(self.model, x[i:i + self.window.window_batch], self.args, self.class_tree)
                    chunks.append([z] if torch.is_tensor(z) else list(z))
                output_logits = [torch.cat(level) if len(level) > 1 else level[0] for level in zip(*chunks)]
            elif self.tta is None:
                x = ops.augment_image(src, desc, desc_host, None, self.size, False)
                _, output_logits = T._model_call(self.model, x, self.args, self.class_tree)
            else:
                B, flags = desc_host.shape[0], self.tta.flags
                for S, _ in self.tta.views(self.size)[::len(flags)]:                    # one forward per scale
                    x = ops.augment_image(src, desc, desc_host, None, S, False)
                    if flags != [0]:
                        x = ops.flip_views(x, flags)
                    _, z = T._model_call(self.model, x, self.args, self.class_tree)
                    z = [z] if torch.is_tensor(z) else list(z)
                    views.extend(([a[i * B:(i + 1) * B] for a in z], f) for i, f in enumerate(flags))
        finally:
            self.model.train(was_training)
        ldesc = label_desc([(H, W) for _, H, W, _ in desc_host.tolist()] if sizes is None else sizes)
        if self.window is not None:
            self.last_window_logits = (output_logits, plan) if self.keep_logits else None
            maps = self.decoder.decode_windows(output_logits, plan, self.window_profile, ldesc, None, self.want_confidence)
        elif self.tta is not None:
            self.last_view_logits = views if self.keep_logits else None
            maps = self.decoder.decode_views(views, ldesc, None, self.want_confidence)
        else:
            if self.keep_logits:
                self.last_logits = output_logits
            if self.hedge is not None:
                return self.decoder.decode_hedged(output_logits, self.hedge, ldesc, None, self.want_confidence)
            maps = self.decoder.decode(output_logits, ldesc, None, self.want_confidence)
        return maps if self.postprocess is None else self.postprocess.apply(maps)


class EnsemblePredictor:
    """Several predictors, one answer: `out = EnsemblePredictor(predictors, cons)(images)` runs every member `Predictor` on the
    batch and votes their label maps down the class tree (Data.DeviceConsensus, one launch) -> ConsensusLabels.  The members
    may differ in model, `tta`, `window`, `hedge` and `postprocess` -- folds of one recipe, checkpoints of one run, the EMA
    and the live weights; they share the class tree, and `cons` must know the bytes of every hedged member
    (`DeviceConsensus.from_hedge(h)`).  The members' own maps of the latest call stay in `last_members`.
    `scores = ensemble.score(images, labels)` decodes every member at the ground-truth maps' own sizes, votes, and scores the
    consensus maps against them with a DeviceScore that knows the internal bytes (`cons.scorer`) -> SourceScores; the voted
    maps of that call stay in `last_labels`.  A pixel without a consensus counts as a prediction outside the class map."""

    def __init__(self, predictors, cons):
        self.predictors, self.cons = list(predictors), cons
        if not 1 <= len(self.predictors) <= ops.CONSENSUS_MAX_MEMBERS:
            raise ValueError(f"EnsemblePredictor: {len(self.predictors)} members, supported 1..{ops.CONSENSUS_MAX_MEMBERS}")
        for m, p in enumerate(self.predictors):
            if p.hedge is not None and any(cons.values.get(n) != v for n, v in p.hedge.values.items()):
                raise ValueError(f"EnsemblePredictor: member {m} writes internal bytes the consensus does not know "
                                 "(build it with DeviceConsensus.from_hedge)")
        self.last_members, self.last_labels = None, None

    def _vote(self, images, sizes, per_image, want_support):
        self.last_members = [p._predict(images, sizes) for p in self.predictors]
        return self.cons(self.last_members, per_image=per_image, want_support=want_support)

    def __call__(self, images, per_image=False, want_support=False):
        return self._vote(images, None, per_image, want_support)

    def score(self, images, labels=None, out=None, per_image=True):
        """images and labels as for Predictor.score -> SourceScores of the consensus maps"""
        gt = Predictor._ground_truth("EnsemblePredictor.score", images, labels)
        self.last_labels = self._vote(images, [(H, W) for _, H, W, _ in gt[2].tolist()], False, False)
        return self.cons.scorer.score(self.last_labels, gt, out, per_image)


def write_metrics_csv(path, accuracy, iou, dice, precision, recall, class_metrics):
    """metrics.csv of predict() (predictEval.py:556-573): one "Average" row, one row per class"""
    import csv
    import numpy as np
    with open(path, "w", newline="") as f:
        wr = csv.writer(f)
        wr.writerow(["Type", "Class", "Accuracy", "IoU", "Dice", "Precision", "Recall"])
        wr.writerow(["Average", "All"] + [float(np.mean(v)) for v in (accuracy, iou, dice, precision, recall)])
        for c, m in enumerate(class_metrics):
            wr.writerow(["Class", c] + [float(np.mean(np.asarray(m[k]))) for k in ("accuracy", "iou", "dice", "precision", "recall")])


@torch.no_grad()
def predict_loop(model, device, test_loader, args, class_tree, Accuracy, Iou, perf_measure, Precision, Recall,
                 save_dir=None, target_paths=None, label_dir=None, class_map=None, score_sources=False, postprocess=None,
                 boundary=None, instances=None, calibration=None, hedge=None):
    """The per-fold body of the reference's predict() (predictEval.py:305-573) on a built model and loader: eval-mode
    forward, prediction_prep, get_metrics per batch, optional PNG dump of each batch's first image and metrics.csv.
    -> dict(accuracy, iou, dice, precision, recall, class_metrics, performance).
    label_dir (with class_map): the loader yields (data, target, sources) -- DeviceAugmentLoader(with_sources=True) -- and
    EVERY image's label map, decoded from the batch's logits at the source's own size, is written to
    <label_dir>/<basename of its target path, or its running index>.png.  target_paths then holds one path per IMAGE, and
    save_dir names a batch's dump after the batch's first image; without label_dir it holds one path per batch, as before.
    score_sources (with class_map, same loader): every batch's logits are also decoded at the sizes of the sources' OWN
    label maps and scored against them on the device (Data/score.py; the decode of label_dir is reused where the sizes
    agree).  The result gains the key "source": dict(names per tree node in breadth-first order, per_image {metric: one
    list over the nodes per image}, total {metric: list over the nodes, from the counts summed over the dataset}, ignored
    [unlabelled ground truth, predictions outside the class map] per image), and save_dir gets metrics_source.csv (the
    dataset totals, one row per node).  Everything else is returned and written as without it.
    postprocess (a Data.DevicePostprocess; with label_dir or score_sources): every decoded source-size map goes through the
    connected-component clean-up before it is written or scored, as in Predictor(postprocess=...).
    boundary (a Data.DeviceBoundaryScore; needs score_sources): the maps that are scored also have their outlines scored
    against the sources' label maps on the device (Data/boundary.py).  The result gains the key "boundary" -- the
    BoundaryScores.summary() of the dataset, {node name: mean hausdorff / hd_percentile / assd / surface_dice, images,
    missed, spurious} -- and save_dir gets metrics_boundary.csv, one row per node.  boundary=None: exactly the launches and
    files described above.
    instances (a Data.DeviceInstanceScore; needs score_sources): the maps that are scored also have their connected
    components matched with those of the sources' label maps on the device (Data/instances.py).  The result gains the key
    "instances" -- the InstanceScores.summary() of the dataset -- and save_dir gets metrics_instances.csv, one row per thing
    group plus "all".  instances=None: exactly the launches and files described above.
    calibration (a Data.DeviceCalibrationScore; needs score_sources): every batch's logits are also scored against the
    sources' label maps on the device (Data/calibration.py), one launch per batch into one dataset total.  The result gains
    the key "calibration" -- the CalibrationScores.summary() of the dataset -- and save_dir gets metrics_calibration.csv,
    one row per tree node and "top@L" row.  calibration=None: exactly the launches and files described above.
    hedge (a Data.Hedge; with label_dir or score_sources): every source-size map is decoded hedged
    (Data.DeviceDecode.decode_hedged) before it is written or scored; the scorer is built with `hedge.values`, so a
    prediction that ends on an internal node competes down to that node.  The `stops` counters accumulate over the
    dataset (batch rows summed; every hedged decode that ran is counted, so where label_dir and score_sources decode one
    batch at different sizes, both maps are); the result gains the key "hedge" -- their HedgedLabels.summary() -- and save_dir gets
    metrics_hedge.csv, one row per tree node, then "rejected" and "nonfinite".  hedge together with postprocess, boundary or
    instances is refused (they read leaf maps), and so is model_type 0.  hedge=None: exactly the launches and files
    described above."""
    import os
    import numpy as np
    from . import train as T
    model.eval()
    n_cls = sum(args.num_classes_full) if hasattr(args, "num_classes_full") else sum(args.num_classes)
    acc2, iou2, dice2, prec2, rec2, perf = [], [], [], [], [], []
    cls2 = T._new_class_metrics(n_cls)
    decoder, n_images = None, 0
    hedge_stops = None
    if hedge is not None:
        for what, on in (("postprocess", postprocess), ("boundary", boundary), ("instances", instances)):
            if on is not None:
                raise ValueError(f"predict_loop: hedge together with {what} is not supported")
        if int(args.model_type) == 0:
            raise ValueError("predict_loop: hedge needs a hierarchical model; model_type 0 has no path to shorten")
        if label_dir is None and not score_sources:
            raise ValueError("hedge needs label_dir or score_sources=True (a source-size decode to hedge)")

    def decode_maps(dec, logits, ldesc):
        nonlocal hedge_stops
        if hedge is None:
            return dec.decode(logits, ldesc)
        maps = dec.decode_hedged(logits, hedge, ldesc)
        total = maps.stops.sum(0, keepdim=True)
        hedge_stops = total if hedge_stops is None else hedge_stops + total
        return maps
    if label_dir is not None:
        from .Data.decode import DeviceDecode, label_desc
        if class_map is None:
            raise ValueError("label_dir needs the class_map (leaf pixel values)")
        decoder = DeviceDecode(class_tree, class_map, args.model_type)
    scorer, source_decoder, scored = None, decoder, []
    if score_sources:
        from .Data.decode import DeviceDecode, label_desc
        from .Data.score import DeviceScore, SourceScores
        if class_map is None:
            raise ValueError("score_sources needs the class_map (leaf pixel values)")
        scorer = DeviceScore(class_tree, class_map, None if hedge is None else hedge.values)
        if source_decoder is None:
            source_decoder = DeviceDecode(class_tree, class_map, args.model_type)
    outlines = []
    if boundary is not None and not score_sources:
        raise ValueError("boundary needs score_sources=True (the sources' own label maps)")
    matched = []
    if instances is not None and not score_sources:
        raise ValueError("instances needs score_sources=True (the sources' own label maps)")
    calibrated = None
    if calibration is not None and not score_sources:
        raise ValueError("calibration needs score_sources=True (the sources' own label maps)")
    for i, batch in enumerate(test_loader):
        data, target = batch[0].to(device), batch[1].to(device)
        _, output_logits = T._model_call(model, data, args, class_tree)
        output_class, eval_targets = prediction_prep(output_logits, target, args, class_tree)
        cls2, acc2, iou2, dice2, prec2, rec2, no_bg = T.get_metrics(output_class, eval_targets, acc2, iou2, dice2, prec2, rec2,
                                                                    Accuracy, Iou, perf_measure, Precision, Recall, device,
                                                                    cls2, args)
        perf.append(float(no_bg.mean()))
        if save_dir is not None:
            first = i if decoder is None else n_images
            name = os.path.basename(target_paths[first]) if target_paths is not None else f"{i:05d}.png"
            save_prediction_images(output_class, save_dir, name)
        if decoder is not None:
            if len(batch) < 3:
                raise ValueError("label_dir: the loader must yield (data, target, sources), e.g. "
                                 "DeviceAugmentLoader(..., with_sources=True)")
            sizes = [(H, W) for _, H, W, _ in batch[2].desc_host.tolist()]
            names = [os.path.basename(target_paths[n_images + j]) if target_paths is not None else f"{n_images + j:05d}.png"
                     for j in range(len(sizes))]
            decoded = decode_maps(decoder, output_logits, label_desc(sizes))
            if postprocess is not None:
                decoded = postprocess.apply(decoded)
            save_label_maps(label_dir, names, decoded)
            n_images += len(sizes)
        if scorer is not None:
            if len(batch) < 3 or batch[2].label is None:
                raise ValueError("score_sources: the loader must yield (data, target, sources) with the sources' label maps, "
                                 "e.g. DeviceAugmentLoader(..., with_sources=True)")
            gt_sizes = [(H, W) for _, H, W, _ in batch[2].ldesc_host.tolist()]
            if decoder is None or gt_sizes != sizes:
                decoded = decode_maps(source_decoder, output_logits, label_desc(gt_sizes))
                if postprocess is not None:
                    decoded = postprocess.apply(decoded)
            scored.append(scorer.score(decoded, batch[2]))
            if boundary is not None:
                outlines.append(boundary.score(decoded, batch[2]))
            if instances is not None:
                matched.append(instances.score(decoded, batch[2]))
            if calibration is not None:
                calibrated = calibration.score(output_logits, batch[2], out=calibrated)
    if save_dir is not None:
        os.makedirs(save_dir, exist_ok=True)
        write_metrics_csv(os.path.join(save_dir, "metrics.csv"), acc2, iou2, dice2, prec2, rec2, cls2)
    result = dict(accuracy=float(np.mean(acc2)), iou=float(np.mean(iou2)), dice=float(np.mean(dice2)),
                  precision=float(np.mean(prec2)), recall=float(np.mean(rec2)), class_metrics=cls2, performance=perf)
    if scorer is not None:
        result["source"] = _source_summary(SourceScores(torch.cat([s.counts for s in scored]),
                                                        torch.cat([s.ignored for s in scored]), scorer.tables))
        if save_dir is not None:
            tot = result["source"]["total"]
            write_metrics_csv(os.path.join(save_dir, "metrics_source.csv"), *[tot[k] for k in METRIC_NAMES],
                              [{k: [tot[k][c]] for k in METRIC_NAMES} for c in range(len(tot["accuracy"]))])
    if boundary is not None:
        from .Data.boundary import BoundaryScores
        result["boundary"] = BoundaryScores.cat(outlines).summary()
        if save_dir is not None:
            write_boundary_csv(os.path.join(save_dir, "metrics_boundary.csv"), result["boundary"])
    if instances is not None:
        from .Data.instances import InstanceScores
        result["instances"] = InstanceScores.cat(matched).summary()
        if save_dir is not None:
            write_instances_csv(os.path.join(save_dir, "metrics_instances.csv"), result["instances"])
    if calibration is not None:
        result["calibration"] = calibrated.summary()
        if save_dir is not None:
            write_calibration_csv(os.path.join(save_dir, "metrics_calibration.csv"), result["calibration"])
    if hedge is not None:
        from .Data.decode import HedgedLabels
        result["hedge"] = HedgedLabels(None, None, None, None, hedge_stops, hedge).summary()
        if save_dir is not None:
            write_hedge_csv(os.path.join(save_dir, "metrics_hedge.csv"), result["hedge"])
    return result


def write_hedge_csv(path, summary):
    """metrics_hedge.csv: one row per tree node of a HedgedLabels.summary() (pixels ended there, its share of all pixels, the
    abstained share of an internal node; empty cells where a share has no denominator), then "rejected" and "nonfinite",
    then the coverage per level"""
    import csv
    total = summary["pixels"]
    share = lambda n: n / total if total else ""        # noqa: E731
    with open(path, "w", newline="") as f:
        wr = csv.writer(f)
        wr.writerow(["Row", "Pixels", "Share", "Abstained"])
        for name, n in summary["ended"].items():
            a = summary["abstained"].get(name, "")
            wr.writerow([name, n, share(n), "" if isinstance(a, float) and math.isnan(a) else a])
        for name in ("rejected", "nonfinite"):
            wr.writerow([name, summary[name], share(summary[name]), ""])
        for L, c in enumerate(summary["coverage"]):
            wr.writerow([f"coverage@{L}", "", "" if math.isnan(c) else c, ""])


def write_consensus_csv(path, summary):
    """metrics_consensus.csv of a ConsensusLabels.summary(): one "node" row per tree node (pixels ended there, voters, the
    unanimous share, mean votes, Fleiss' kappa), the "none" row, one "pair" row per member pair and node (both, the two areas,
    Dice, IoU, fn, fp, agreement), one "member" row per member (its abstained share); empty cells where a figure has no
    denominator"""
    import csv
    blank = lambda v: "" if isinstance(v, float) and math.isnan(v) else v        # noqa: E731
    with open(path, "w", newline="") as f:
        wr = csv.writer(f)
        wr.writerow(["Row", "Name", "Members", "Pixels", "Voters", "Unanimous", "MeanVotes", "Kappa", "Both", "AreaI", "AreaJ", "Dice",
                     "IoU", "FN", "FP", "Agreement", "Abstained"])
        for name, r in summary["nodes"].items():
            wr.writerow(["node", name, "", r["ended"], r["voters"], blank(r["unanimous"]), blank(r["mean_votes"]), blank(r["kappa"])] +
                        [""] * 9)
        wr.writerow(["none", "none", "", summary["none"]] + [""] * 13)
        for (i, j), rows in summary["pairs"].items():
            for name, r in rows.items():
                wr.writerow(["pair", name, f"{i}-{j}"] + [""] * 5 + [r["both"], r["area_i"], r["area_j"]] +
                            [blank(r[k]) for k in ("dice", "iou", "fn", "fp", "agreement")] + [""])
        for m, a in enumerate(summary["abstained"]):
            wr.writerow(["member", "", m] + [""] * 13 + [blank(a)])


def write_calibration_csv(path, summary):
    """metrics_calibration.csv: one row per tree node and "top@L" row of a CalibrationScores.summary() (empty cells where a
    row had no event), then the ignored pixels"""
    import csv
    keys = ("n", "prevalence", "mean_confidence", "ece", "mce", "brier", "nonfinite")
    with open(path, "w", newline="") as f:
        wr = csv.writer(f)
        wr.writerow(["Row", "Events", "Prevalence", "MeanConfidence", "ECE", "MCE", "Brier", "NonFinite"])
        for name, row in summary.items():
            if isinstance(row, dict):
                wr.writerow([name] + ["" if isinstance(row[k], float) and math.isnan(row[k]) else row[k] for k in keys])
        wr.writerow(["ignored", summary["ignored"]] + [""] * 6)


def write_instances_csv(path, summary):
    """metrics_instances.csv: one row per thing group of an InstanceScores.summary() and one for "all" (empty cells where a
    denominator was 0; one TPAt column per threshold)"""
    import csv
    rows = {k: v for k, v in summary.items() if isinstance(v, dict)}
    at = list(rows["all"]["tp_at"])
    keys = ("n_gt", "n_pred", "tp", "fp", "fn", "precision", "recall", "rq", "sq", "pq", "mean_iou")
    with open(path, "w", newline="") as f:
        wr = csv.writer(f)
        wr.writerow(["Group", "GT", "Predicted", "TP", "FP", "FN", "Precision", "Recall", "RQ", "SQ", "PQ", "MeanIoU"] +
                    [f"TPAt{t:g}" for t in at])
        for name, row in rows.items():
            wr.writerow([name] + ["" if isinstance(row[k], float) and math.isnan(row[k]) else row[k] for k in keys] +
                        [row["tp_at"][t] for t in at])


def write_boundary_csv(path, summary):
    """metrics_boundary.csv: one row per tree node of a BoundaryScores.summary() (distances in pixels; empty cells where a
    node was in both maps of no image)"""
    import csv
    from .Data.boundary import METRICS
    with open(path, "w", newline="") as f:
        wr = csv.writer(f)
        wr.writerow(["Class", "Hausdorff", "HDPercentile", "ASSD", "SurfaceDice", "Images", "Missed", "Spurious"])
        for name, row in summary.items():
            wr.writerow([name] + ["" if math.isnan(row[k]) else row[k] for k in METRICS] +
                        [row["images"], row["missed"], row["spurious"]])


def _source_summary(scores):
    """SourceScores of a dataset (one row per image) -> the "source" entry of predict_loop; one device-to-host copy"""
    n = len(scores)
    vecs = [scores.metric_vectors(b) for b in range(n)] + [scores.metric_vectors()]
    host = torch.stack([torch.stack([v[k] for k in METRIC_NAMES]) for v in vecs]).tolist()
    return dict(names=[x for lvl in scores.tables.names for x in lvl], images=n,
                per_image={k: [host[b][i] for b in range(n)] for i, k in enumerate(METRIC_NAMES)},
                total={k: host[n][i] for i, k in enumerate(METRIC_NAMES)}, ignored=scores.ignored.tolist())
