"""torch-CPU oracle of the hedged decode (csrc/decode_hedged.hip, Data/hedge.py), the case list of the GPU test and the ONE
comparison rule, written straight from the class tree (it shares no table with the product).

Oracle, in float64, on tests/decode_ref.decode_sample's path c_0, c_1, ... and near-tie mask:
  T_L = sigmoid(z_0[c_0]) * prod_{l <= L} softmax_group(z_l)[c_l], recomputed per level from the resampled logits;
  walk from level 0: T_L < tau(c_L) (a NaN is not below) stops the pixel -- at level 0 with the reject value and T_0, deeper
  with the byte and the T of the node above; a leaf that is entered ends it with the leaf's value and T_L.
  `stop` is the counter cell: the node's position in breadth-first order, or the node count for "rejected".

Exempt pixels: the near ties (there the device may walk another path), plus the pixels where some visited |T_L - tau| is within
`band` = 4 x the largest distance of torch-CPU's own fp32 evaluation of the same T_L from the fp64 one over the case's visited
levels, floor 2^-22 (the rule of tests/calibration_ref.py).

Comparison rule (`check`):
  outside the exempt mask the labels are equal and the confidence is within the bar of tests/decode_harness.check: 4 x the
    largest distance of the fp32 torch-CPU confidence from the fp64 one there, floor 1e-6;
  on threshold-exempt pixels that are no near ties the device's label must still be a node of the oracle's full decode path
    (or the reject value);
  exempt pixels are at most decode_harness.MASK_CAP = 0.5 % of a case (`exempt_share`; asserted on the oracle alone, CPU)."""
import numpy as np
import torch
import torch.nn.functional as F

from tests import decode_ref
from tests.calibration_ref import tree_levels
from tests.decode_harness import EDGE, MASK_CAP, RAGGED, STRIDED, _tree, _wide_tree

BAND_FLOOR = 2.0 ** -22

# name -> dict(tree "tl" / "ext" / "wide", S, sizes, seed, thresholds: a scalar (child levels), a per-level list or a dict of
# node names, internal: {name: byte} given by hand (the rest is assigned), reject: byte or None).  Thresholds stay away from 0
# and 1 and the logits are decode_ref.smooth_logits, so that few T_L fall within the band of a threshold.
CASES = {
    "tl_scalar_ragged": dict(tree="tl", S=62, sizes=RAGGED, seed=3, thresholds=0.6, internal={}, reject=None),
    "tl_dict_edge": dict(tree="tl", S=12, sizes=EDGE, seed=4, thresholds={"pulp": 0.3, "dentin": 0.5, "enamel": 0.7,
                                                                            "composite": 0.45}, internal={"tooth": 200}, reject=None),
    "tl_reject_ragged": dict(tree="tl", S=8, sizes=RAGGED, seed=5, thresholds=[0.6, 0.35], internal={}, reject=7),
    "tl_scalar_strided": dict(tree="tl", S=12, sizes=STRIDED, seed=6, thresholds=0.5, internal={}, reject=None),
    "ext_scalar_ragged": dict(tree="ext", S=12, sizes=RAGGED, seed=7, thresholds=0.45, internal={}, reject=None),
    "ext_dict_edge": dict(tree="ext", S=62, sizes=EDGE, seed=8, thresholds={"tooth": 0.4, "healthy": 0.35, "enamel": 0.3,
                                                                            "upper": 0.25}, internal={"healthy": 99}, reject=None),
    "ext_reject_strided": dict(tree="ext", S=62, sizes=STRIDED, seed=9, thresholds=[0.55, 0.3, 0.2, 0.15], internal={},
                               reject=201),
    "wide_scalar_ragged": dict(tree="wide", S=62, sizes=RAGGED, seed=10, thresholds=0.3, internal={}, reject=None),
    "wide_reject_edge": dict(tree="wide", S=8, sizes=EDGE, seed=11, thresholds=[0.5, 0.25], internal={"group1": 5}, reject=1),
}


def case_tree(key):
    return _wide_tree() if key == "wide" else _tree(key)


def resolve(tree, class_map, thresholds, internal=None, reject=None):
    """-> (names per level, tau {name: threshold}, byte {name: the byte written when the walk ends on the node}, reject byte
    or None); internal nodes without a given byte get the smallest unused uint8 values in breadth-first order"""
    names, _, _ = tree_levels(tree, 1)
    kids = {n: k for lvl in decode_ref.bfs_levels(tree) for n, k in lvl}
    tau = {n: 0.0 for lvl in names for n in lvl}
    if isinstance(thresholds, dict):
        tau.update({n: float(v) for n, v in thresholds.items()})
    elif isinstance(thresholds, (list, tuple)):
        assert len(thresholds) == len(names)
        tau = {n: float(thresholds[L]) for L, lvl in enumerate(names) for n in lvl}
    else:
        tau = {n: (float(thresholds) if L else 0.0) for L, lvl in enumerate(names) for n in lvl}
    pix = decode_ref.name2pix(class_map)
    byte = {n: pix[n] for lvl in names for n in lvl if not kids[n]}
    used = set(byte.values()) | set((internal or {}).values()) | ({reject} if reject is not None else set())
    free = (v for v in range(256) if v not in used)
    for lvl in names:
        for n in lvl:
            if kids[n]:
                byte[n] = internal[n] if internal and n in internal else next(free)
    return names, tau, byte, reject


def path_confidence(logits, tree, path, H, W, dtype):
    """one sample's logits (per level [C_L, S, S]) and its decoded path (per level [H, W] channel or -1) -> per level T_L
    [H, W] in `dtype` (1 where the path does not reach the level: unused)"""
    _, groups, _ = tree_levels(tree, 1)
    T, run = [], torch.ones(H, W, dtype=dtype)
    for L, a in enumerate(logits):
        v = F.interpolate(a[None].to(dtype), size=(H, W), mode="bilinear", align_corners=False, antialias=False)[0]
        if L == 0:
            p = torch.sigmoid(v)
        else:
            p = torch.empty_like(v)
            for _, first, n in groups[L]:
                p[first:first + n] = torch.softmax(v[first:first + n], dim=0)
        on = path[L] >= 0
        run = torch.where(on, run * p.gather(0, path[L].clamp_min(0)[None])[0], run)
        T.append(torch.where(on, run, torch.ones_like(run)))
    return T


def hedge_sample(logits, tree, class_map, H, W, thresholds, internal=None, reject=None):
    """-> dict(label [H,W] uint8, conf [H,W] fp64, conf32 (the fp32 T at the same node), stop [H,W] int64 counter cell, tie,
    visited: per level the pixels whose walk tested that level, T / T32 per level, tauL per level [H,W], path, nodes: on-path
    bytes per level [H,W] (-1 off the path), d32: the largest |T32 - T| over visited levels outside the near ties)"""
    names, tau, byte, reject = resolve(tree, class_map, thresholds, internal, reject)
    kids = {n: k for lvl in decode_ref.bfs_levels(tree) for n, k in lvl}
    _, _, tie, path = decode_ref.decode_sample(logits, tree, class_map, 1, H, W)
    T = path_confidence(logits, tree, path, H, W, torch.float64)
    T32 = path_confidence(logits, tree, path, H, W, torch.float32)
    cell0 = np.concatenate([[0], np.cumsum([len(n) for n in names])])
    rejected = int(cell0[-1])
    label = torch.zeros(H, W, dtype=torch.uint8)
    conf = torch.ones(H, W, dtype=torch.float64)
    conf32 = torch.ones(H, W, dtype=torch.float32)
    stop = torch.full((H, W), -1, dtype=torch.int64)
    walking = torch.ones(H, W, dtype=torch.bool)
    visited, tauL, nodes = [], [], []
    d32 = 0.0
    for L, lvl in enumerate(names):
        c = path[L].clamp_min(0)
        tl = torch.tensor([tau[n] for n in lvl], dtype=torch.float64)[c]
        bl = torch.tensor([byte[n] for n in lvl], dtype=torch.int64)[c]
        leaf = torch.tensor([not kids[n] for n in lvl])[c]
        here = walking & (path[L] >= 0)
        visited.append(here)
        tauL.append(tl)
        nodes.append(torch.where(path[L] >= 0, bl, torch.full_like(bl, -1)))
        sel = here & ~tie
        if bool(sel.any()):
            d = (T32[L].double() - T[L]).abs()[sel]
            d = d[~torch.isnan(d)]
            d32 = max(d32, float(d.max()) if d.numel() else 0.0)
        fail = here & (T[L] < tl)
        if L == 0:
            assert reject is not None or not bool(fail.any())
            label = torch.where(fail, torch.tensor(reject if reject is not None else 0, dtype=torch.uint8), label)
            conf, conf32 = torch.where(fail, T[0], conf), torch.where(fail, T32[0], conf32)
            stop = torch.where(fail, torch.tensor(rejected), stop)
        # (L >= 1: label, confidence and cell of the node above are already in place)
        enter = here & ~fail
        label = torch.where(enter, bl.to(torch.uint8), label)
        conf, conf32 = torch.where(enter, T[L], conf), torch.where(enter, T32[L], conf32)
        stop = torch.where(enter, int(cell0[L]) + c, stop)
        walking = enter & ~leaf
    assert not bool(walking.any()) and bool((stop >= 0).all())
    return dict(label=label, conf=conf, conf32=conf32, stop=stop, tie=tie, visited=visited, T=T, tauL=tauL, path=path,
                nodes=nodes, d32=d32, reject=reject, cells=rejected + 2)


def case_inputs(name):
    """-> (case dict, tree, class map, logits per level [B, C_L, S, S] fp32)"""
    case = CASES[name]
    tree, cmap = case_tree(case["tree"])
    names, _, _ = tree_levels(tree, 1)
    return case, tree, cmap, decode_ref.smooth_logits(len(case["sizes"]), [len(n) for n in names], case["S"], case["seed"])


def finish(samples):
    """per-sample hedge_sample dicts of one case -> the case's reference: band from the largest d32, the exempt mask per sample"""
    d32 = max(s["d32"] for s in samples)
    band = max(4.0 * d32, BAND_FLOOR)
    for s in samples:
        close = torch.zeros_like(s["tie"])
        for here, T, tl in zip(s["visited"], s["T"], s["tauL"]):
            close |= here & ((T - tl).abs() <= band)
        s["close"] = close
        s["exempt"] = close | s["tie"]
    return dict(samples=samples, band=band, d32=d32)


_REFS = {}


def case_reference(name):
    """the oracle of a case, computed once per process and shared (callers must not change it)"""
    if name not in _REFS:
        case, tree, cmap, logits = case_inputs(name)
        _REFS[name] = finish([hedge_sample([z[b] for z in logits], tree, cmap, H, W, case["thresholds"], case["internal"],
                                           case["reject"]) for b, (H, W) in enumerate(case["sizes"])])
    return _REFS[name]


def exempt_share(ref):
    return sum(int(s["exempt"].sum()) for s in ref["samples"]) / sum(s["exempt"].numel() for s in ref["samples"])


def check(out, ref, what):
    """a HedgedLabels (or anything with unpack / unpack_confidence) against a case reference by the rule above; prints every
    figure it asserts"""
    maps, confs = out.unpack(), out.unpack_confidence()
    exempt = total = 0
    d32 = dgot = 0.0
    for b, s in enumerate(ref["samples"]):
        got = torch.from_numpy(maps[b])
        assert got.shape == s["label"].shape and got.dtype == torch.uint8
        keep = ~s["exempt"]
        wrong = int(((got != s["label"]) & keep).sum())
        soft = s["close"] & ~s["tie"]
        on_path = torch.zeros_like(soft) if s["reject"] is None else (got == s["reject"])
        for nb in s["nodes"]:
            on_path |= got.long() == nb
        off = int((soft & ~on_path).sum())
        print(f"{what} sample {b} {tuple(got.shape)}: {int(s['tie'].sum())} near ties, {int(s['close'].sum())} within the band of a "
              f"threshold, {wrong} labels differ outside them, {off} threshold-exempt labels off the oracle's path")
        assert wrong == 0 and off == 0, (what, b, wrong, off)
        exempt += int(s["exempt"].sum())
        total += got.numel()
        if bool(keep.any()):
            d32 = max(d32, float((s["conf32"].double() - s["conf"]).abs()[keep].max()))
            if confs is not None:
                dgot = max(dgot, float((torch.from_numpy(confs[b]).double() - s["conf"]).abs()[keep].max()))
    print(f"{what}: exempt {exempt}/{total}, band {ref['band']:.3e}")
    assert exempt <= MASK_CAP * total, (what, exempt, total)
    bar = max(4.0 * d32, 1e-6)
    print(f"{what}: confidence distance from fp64: device {dgot:.3e}, torch-CPU fp32 {d32:.3e}, bar {bar:.3e}")
    assert dgot <= bar, (what, dgot, d32)
