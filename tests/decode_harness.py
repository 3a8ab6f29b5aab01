"""What the decode test modules share (plain decode, test-time augmentation, sliding windows; CPU and GPU): the shipped
trees and a tree at the kernels' channel limit, synthetic source images, the size sets and the ONE rule of oracle parity.

Oracle parity (`check`): labels must be equal outside the oracle's near-tie mask (gap of the deciding group below
decode_ref.NEAR_TIE = 2e-4), which may cover at most MASK_CAP = 0.5 % of a case's pixels.  The confidence is compared
outside the mask with a bar of 4x the largest distance of the fp32 torch-CPU evaluation of the same formula from the fp64
one on the same inputs (floor 1e-6)."""
import csv
import os

import numpy as np
import torch

from tests.helpers import DATA, load_tree

TREES = {"tl": ("class_tree_tl.json", "class_map.csv"), "ext": ("class_tree_tl_extended.json", "class_map_extended.csv")}
MASK_CAP = 0.005

# output sizes (H, W) of one call, one image each
RAGGED = [(50, 70), (80, 64), (62, 62), (30, 100)]     # up- and downsampling from 62 x 62, and the identity
EDGE = [(7, 3), (1, 1), (3, 9), (2, 260)]              # misaligned rows, rows narrower than a lane, a row crossing a tile
IDENTITY = [(62, 62)] * 3
STRIDED = [(4100, 250)]                                # B = 1: 1025 tiles for 1024 blocks, a block's tile loop runs twice


def _tree(key):
    """"tl" / "ext" -> (class tree, class map rows) as shipped"""
    t, m = TREES[key]
    with open(os.path.join(DATA, m)) as f:
        return load_tree(t), list(csv.DictReader(f))


def _wide_tree():
    """level 1 has 16 channels (the kernel's limit) in groups of 5, 5 and 6"""
    tree, cmap, v = {"background": {}}, {"background": 0}, 10
    for g, n in enumerate((5, 5, 6)):
        tree[f"group{g}"] = {}
        for k in range(n):
            tree[f"group{g}"][f"g{g}c{k}"] = {}
            cmap[f"g{g}c{k}"] = v
            v += 10
    return tree, cmap


def _source(rng, H, W, ch):
    """a uint8 H x W (ch == 1) or H x W x 3 source image: a smooth pattern plus noise"""
    yy, xx = np.mgrid[0:H, 0:W]
    base = (96 + 80 * np.sin(xx / (7.0 + W / 40)) * np.cos(yy / (5.0 + H / 50)))[..., None]
    noise = rng.integers(-60, 61, size=(H, W, ch))
    img = np.clip(base + noise + np.array([0, 25, -25][:ch]), 0, 255).astype(np.uint8)
    return img[..., 0] if ch == 1 else img


def check(out, samples, what):
    """a RaggedLabels against the oracle's per-sample (label, confidence, near-tie mask, <unused>, fp32 confidence), the first
    three evaluated in fp64; prints every figure it asserts"""
    maps, confs = out.unpack(), out.unpack_confidence()
    masked = total = 0
    d32 = dgot = 0.0
    for b, (want, conf, tie, _, conf32) in enumerate(samples):
        H, W = want.shape
        assert maps[b].shape == (H, W) and maps[b].dtype == np.uint8
        keep = ~tie
        wrong = int(((torch.from_numpy(maps[b]) != want) & keep).sum())
        print(f"{what} sample {b} {H}x{W}: {int(tie.sum())} near ties, {wrong} labels differ outside them")
        assert wrong == 0, (what, b, wrong)
        masked += int(tie.sum())
        total += H * W
        d32 = max(d32, float((conf32.double() - conf).abs()[keep].max()))
        dgot = max(dgot, float((torch.from_numpy(confs[b]).double() - conf).abs()[keep].max()))
    print(f"{what}: mask {masked}/{total}")
    assert masked <= MASK_CAP * total, (what, masked, total)
    bar = max(4.0 * d32, 1e-6)
    print(f"{what}: confidence distance from fp64: device {dgot:.3e}, torch-CPU fp32 {d32:.3e}, bar {bar:.3e}")
    assert dgot <= bar, (what, dgot, d32)
