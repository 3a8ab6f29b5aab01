"""Device post-processing: connected-component clean-up of decoded label maps -- small islands removed, only the largest
region of a class kept, small holes closed -- without a map leaving the device.  Kernels: csrc/components.hip; the
semantics are stated in include/hrseg.h (hrseg_label_components, hrseg_filter_components).

The components are those of a chosen LEVEL of the class tree while the map keeps its leaf values: at level 0 of the
shipped tree a tooth is one region whatever pulp, dentin, enamel and composite it is made of, and `min_area` judges the
tooth, not its pulp chamber.  The groups are the CUT of the tree at the level: the nodes at that depth plus the leaves
shallower than it, in breadth-first order.

The tables are built on the host without a GPU; only `apply` and `components` launch.
"""
from __future__ import annotations

import torch

from .. import ops
from .._lib import require_gpu
from ..utils.hierarchy import TreeIndex
from .dataset import TargetEncoder
from .decode import RaggedLabels
from .score import DeviceScore

NO_GROUP = 255          # pixel values outside the class map: no rule, always copied


class ComponentTables:
    """What the component kernels read: `names` of the cut, `group` (256 ints: pixel value -> group id = position in
    `names`, 255 for values that are no leaf's), `rules` (256 rows (min_area, keep_largest, fill); fill -1 = the neighbour
    rule; rows of groups without a rule are (0, 0, -1): nothing is removed), `connectivity`."""

    def __init__(self, names, group, rules, connectivity):
        self.names, self.group = list(names), [int(g) for g in group]
        self.rules = [tuple(int(v) for v in r) for r in rules]
        self.connectivity = int(connectivity)
        self._dev = {}

    def device(self, device):
        """(group [256] uint8, rules [256,3] int32) on the device, cached per device"""
        key = str(device)
        if key not in self._dev:
            self._dev[key] = (torch.tensor(self.group, dtype=torch.uint8, device=device),
                              torch.tensor(self.rules, dtype=torch.int32, device=device))
        return self._dev[key]


def build_component_tables(class_tree, class_map, level=0, rules=None, connectivity=8) -> ComponentTables:
    """class_tree + class_map (any form TargetEncoder accepts) -> ComponentTables of the cut at `level`.
    rules: {name of a cut node: dict(min_area=0, keep_largest=False, fill="neighbour")}; fill may also be a pixel value
    0..255 or a leaf's name.  min_area is in pixels of the map that is filtered.
    KeyError for an unknown node or leaf name and for a leaf without a pixel value; ValueError for a pixel value outside
    uint8, a rule on a node that is not in the cut, a negative min_area, an unknown rule key, more than 255 groups, a
    negative level and a connectivity other than 4 and 8."""
    if connectivity not in (4, 8):
        raise ValueError(f"connectivity {connectivity}, supported 4 and 8")
    if int(level) < 0:
        raise ValueError(f"level {level} must not be negative")
    name2pix = TargetEncoder._name2pix(class_map)
    index = TreeIndex(class_tree)

    def pixel(leaf):
        if leaf not in name2pix:
            raise KeyError(f"Class '{leaf}' not found in class_map.")
        v = int(name2pix[leaf])
        if not 0 <= v <= 255:
            raise ValueError(f"pixel value {v} of class '{leaf}' does not fit a uint8 label image")
        return v

    names = [n for n in index.order if index.depth[n] == level or (index.depth[n] < level and index.is_leaf(n))]
    if len(names) > NO_GROUP:
        raise ValueError(f"the cut at level {level} has {len(names)} groups, at most {NO_GROUP}")
    gid = {n: i for i, n in enumerate(names)}
    group = [NO_GROUP] * 256
    for n in names:
        for leaf in index.leaves[n]:
            group[pixel(leaf)] = gid[n]
    table = [(0, 0, -1)] * 256
    for name, rule in (rules or {}).items():
        if name not in index.depth:
            raise KeyError(f"rule for '{name}': no such node in the class tree")
        if name not in gid:
            raise ValueError(f"rule for '{name}': the node is not in the cut at level {level} ({', '.join(names)})")
        unknown = set(rule) - {"min_area", "keep_largest", "fill"}
        if unknown:
            raise ValueError(f"rule for '{name}': unknown keys {sorted(unknown)}")
        min_area, fill = int(rule.get("min_area", 0)), rule.get("fill", "neighbour")
        if min_area < 0:
            raise ValueError(f"rule for '{name}': min_area {min_area} is negative")
        if isinstance(fill, str):
            if fill == "neighbour":
                fill = -1
            elif fill in index.depth and index.is_leaf(fill):
                fill = pixel(fill)
            else:
                raise KeyError(f"rule for '{name}': fill '{fill}' is no leaf of the class tree")
        elif not 0 <= int(fill) <= 255:
            raise ValueError(f"rule for '{name}': fill {fill} does not fit a uint8 label image")
        table[gid[name]] = (min(min_area, (1 << 31) - 1), int(bool(rule.get("keep_largest", False))), int(fill))
    return ComponentTables(names, group, table, connectivity)


class DevicePostprocess:
    """`pp = DevicePostprocess(class_tree, class_map, level=0, rules={"tooth": dict(min_area=200)}); clean = pp.apply(maps)`
    with `maps` a RaggedLabels (DeviceDecode / Predictor) or a (buffer, desc, desc_host) triple -> a new RaggedLabels with
    the same descriptors and the same confidence object.  min_area counts pixels of the maps given, at whatever size they
    were decoded.  `last_stats`: int64 [B,256,3] on the device (per image and group: components found, removed, pixels
    rewritten) of the latest apply; `components(maps)` -> (roots, area), the instance maps alone."""

    def __init__(self, class_tree, class_map, level=0, rules=None, connectivity=8):
        self.tables = build_component_tables(class_tree, class_map, level, rules, connectivity)
        self.last_stats = None

    @staticmethod
    def _maps(ragged):
        buf, desc, host = DeviceScore._triple(ragged, ("labels", "desc", "desc_host"))
        return buf, desc.to(buf.device, non_blocking=True), host

    def components(self, ragged):
        """(roots, area): int32 device tensors indexed like the label buffer (hrseg_label_components); 3 launches"""
        require_gpu()
        buf, desc, host = self._maps(ragged)
        return ops.label_components(buf, desc, host, self.tables.device(buf.device)[0], self.tables.connectivity)

    def apply(self, ragged) -> RaggedLabels:
        require_gpu()
        buf, desc, host = self._maps(ragged)
        group, rules = self.tables.device(buf.device)
        roots, area = ops.label_components(buf, desc, host, group, self.tables.connectivity)
        out, self.last_stats = ops.filter_components(buf, desc, host, group, rules, roots, area)
        return RaggedLabels(out, getattr(ragged, "confidence", None), desc, host)

    def stats_by_name(self):
        """last_stats on the host: {image: {group name: (found, removed, pixels)}}, groups that occur only (one copy)"""
        if self.last_stats is None:
            raise RuntimeError("DevicePostprocess.stats_by_name: nothing was applied yet")
        rows = self.last_stats.tolist()
        names = {i: n for i, n in enumerate(self.tables.names)}
        names[NO_GROUP] = "<outside the class map>"
        return {b: {names[g]: tuple(r) for g, r in enumerate(row) if r[0] and g in names} for b, row in enumerate(rows)}
