"""Torch-CPU restatement of the mixing augmentation (test infrastructure, not product).

include/hrseg.h ("mixing") written out with plain indexing, without the product's bit sets: counts, the node choice as a
sorted list, the mask from slices of the moved donor planes, and the gather on the int32 views.  Also the named inputs that
tests/test_mix_cpu.py and tests/test_mix_gpu.py share: label maps, images with non-finite values, the draws of every case."""
from __future__ import annotations

import csv
import math
import os

import numpy as np
import torch

from tests import augment_ref as R
from tests import partial_ref as PR
from tests.helpers import DATA, load_tree

TREES = {"tl": ("class_tree_tl.json", "class_map.csv"), "ext": ("class_tree_tl_extended.json", "class_map_extended.csv")}
SPECIALS = [0x7FC01234, -0x3FFFFF, 0x7F800000, -0x800000, -0x80000000]   # two NaN payloads, +inf, -inf, -0.0 (int32 bit patterns)


def wide_tree():
    """64 nodes: 8 groups of 7 children (56 leaves)"""
    tree, cmap = {}, []
    for g in range(8):
        tree[f"group{g}"] = {}
        cmap.append({"class_name": f"group{g}", "pixel_val": "None"})
    v = 1
    for g in range(8):
        for k in range(7):
            tree[f"group{g}"][f"g{g}c{k}"] = {}
            cmap.append({"class_name": f"g{g}c{k}", "pixel_val": str(v)})
            v += 1
    return tree, cmap


def tree_of(key):
    if key == "wide":
        return wide_tree()
    t, m = TREES[key]
    with open(os.path.join(DATA, m)) as f:
        return load_tree(t), list(csv.DictReader(f))


# ------------------------------------------------------------------------------------------------ the restatement
def k_of_n(share):
    return [0] + [min(n, max(1, math.ceil(share * n))) for n in range(1, 65)]


def candidates(tree, model_type, level=0, nodes=None):
    """channel indices: the nodes at depth `level` (every leaf in flat mode), or the named ones"""
    names, parent = PR.emitted(tree, model_type)
    if nodes is not None:
        return [names.index(n) for n in nodes]
    if model_type == 0:
        return list(range(len(names)))
    depth = {}
    for c, p in enumerate(parent):
        depth[c] = 0 if p < 0 else depth[p] + 1
    return [c for c in range(len(names)) if depth[c] == level]


def moved(t, dx, dy):
    """t [K,S,S] moved by (dx, dy): out[k][r][c] = t[k][r-dy][c-dx]; -> (moved planes, zero outside), (inside [S,S] bool)"""
    K, S, _ = t.shape
    out, inside = torch.zeros_like(t), torch.zeros(S, S, dtype=torch.bool)
    if abs(dx) < S and abs(dy) < S:
        r_lo, r_hi, c_lo, c_hi = max(0, dy), min(S, S + dy), max(0, dx), min(S, S + dx)
        out[:, r_lo:r_hi, c_lo:c_hi] = t[:, r_lo - dy:r_hi - dy, c_lo - dx:c_hi - dx]
        inside[r_lo:r_hi, c_lo:c_hi] = True
    return out, inside


def mix(x, y, p, cand, kn, min_pixels=1):
    """-> dict counts [B,C] int32, chosen (list of sorted channel lists), mask [B,S,S] uint8, x2, y2 (bits of x / y)"""
    B, C, S, _ = y.shape
    counts = (y == 1.0).sum(dim=(2, 3)).to(torch.int32)
    xi, yi = x.view(torch.int32), y.view(torch.int32)
    x2, y2 = xi.clone(), yi.clone()
    mask = torch.zeros(B, S, S, dtype=torch.uint8)
    chosen = []
    for b in range(B):
        chosen.append([])
        if not bool(p["apply"][b]):
            continue
        d, dx, dy = int(p["donor"][b]), int(p["dx"][b]), int(p["dy"][b])
        ym, inside = moved(y[d], dx, dy)
        if bool(p["boxed"][b]):
            r0, c0, r1, c1 = (int(v) for v in p["box"][b])
            m = torch.zeros(S, S, dtype=torch.bool)
            m[r0:r1, c0:c1] = True
            m &= inside
        else:
            present = [c for c in cand if int(counts[d, c]) >= min_pixels]
            k = kn[len(present)]
            chosen[b] = sorted(sorted(present, key=lambda c: int(p["prio"][b][c]))[:k])
            m = torch.zeros(S, S, dtype=torch.bool)
            for c in chosen[b]:
                m |= inside & (ym[c] == 1.0)
        mask[b] = m.to(torch.uint8)
        x2[b] = torch.where(m[None], moved(xi[d], dx, dy)[0], xi[b])
        y2[b] = torch.where(m[None], moved(yi[d], dx, dy)[0], yi[b])
    return {"counts": counts, "chosen": chosen, "mask": mask, "x2": x2.view(torch.float32), "y2": y2.view(torch.float32)}


def chosen_bits(chosen):
    """the channel lists as the int64 bit sets the device writes"""
    out = []
    for cs in chosen:
        v = sum(1 << c for c in cs)
        out.append(v - (1 << 64) if v >= (1 << 63) else v)
    return torch.tensor(out, dtype=torch.int64)


# ------------------------------------------------------------------------------------------------ inputs
def blocky(rng, values, S, block):
    coarse = rng.choice(np.asarray(values, dtype=np.uint8), size=(S // block + 1, S // block + 1))
    return np.ascontiguousarray(np.repeat(np.repeat(coarse, block, 0), block, 1)[:S, :S])


def image(B, K, S, seed):
    """random fp32 with the five special bit patterns at fixed positions of every sample"""
    x = torch.randn(B, K, S, S, generator=torch.Generator().manual_seed(seed))
    xi = x.view(torch.int32)
    for i in range(40):
        pos = (i * 97 + 13) % (S * S)
        xi[:, i % K, pos // S, pos % S] = SPECIALS[i % 5]
    return x


def draws(B, C, seed, donor, shifts, apply=None, boxes=None):
    """a params dict as Data.mix.sample_params returns it, with the named donors, shifts (dx, dy) and boxes"""
    g = torch.Generator().manual_seed(seed)
    return {"apply": torch.tensor([True] * B if apply is None else apply), "donor": torch.tensor(donor, dtype=torch.int64),
            "prio": torch.stack([torch.randperm(C, generator=g) for _ in range(B)]),
            "dx": torch.tensor([s[0] for s in shifts], dtype=torch.int64), "dy": torch.tensor([s[1] for s in shifts], dtype=torch.int64),
            "boxed": torch.tensor([boxes is not None] * B),
            "box": torch.tensor(boxes if boxes is not None else [[0, 0, 0, 0]] * B, dtype=torch.int64)}


A_SHIFTS = [(0, 0), (1, 0), (-3, 2), (0, -61), (62, 0)]
A_DONORS = [1, 2, 3, 4, 0]
A_APPLY = [True, True, True, False, True]
G_BOXES = [[0, 0, 62, 62], [10, 7, 10, 30], [61, 61, 62, 62], [10, 5, 50, 40]]


def _labels(key, S, B, seed, internal=None, ignore=(), without=None):
    """B blocky maps (blocks of 7 and 11) of the tree's leaf bytes plus the internal and ignore bytes; sample `without[0]` holds
    no byte of the classes `without[1]`"""
    _, cmap = tree_of(key)
    n2p = R.name2pix(cmap)
    values = sorted(n2p.values()) + sorted((internal or {}).values()) + list(ignore)
    rng = np.random.default_rng(seed)
    maps = []
    for b in range(B):
        vals = values
        if without is not None and b == without[0]:
            vals = [v for n, v in sorted(n2p.items()) if n not in without[1]]
        maps.append(blocky(rng, vals, S, (7, 11)[b % 2]))
    return np.stack(maps)


TOOTH_LEAVES = ("pulp", "dentin", "enamel", "composite")


def _case(key, model_type, labels, p, seed, internal=None, ignore=(), **mix_kw):
    return {"tree": key, "model_type": model_type, "labels": labels, "params": p, "x_seed": seed, "internal": internal,
            "ignore": tuple(ignore), "mix": mix_kw}


def _build_cases():
    c = {}
    # A: rows off the 16-byte grid, every sample donor and recipient; sample 2's map holds no tooth
    labA = _labels("tl", 62, 5, 101, without=(2, TOOTH_LEAVES))
    pA = draws(5, 8, 102, A_DONORS, A_SHIFTS, A_APPLY)
    c["A"] = _case("tl", 1, labA, pA, 103, level=0)
    c["A_tooth"] = _case("tl", 1, labA, pA, 103, nodes=["tooth"])
    pA3 = draws(5, 8, 102, A_DONORS, A_SHIFTS)                           # (sample 3 applied too: one row comes in from below)
    c["A_all"] = _case("tl", 1, labA, pA3, 103, level=0)
    # B: aligned rows, three levels deep
    labB = _labels("ext", 64, 2, 111)
    c["B_0"] = _case("ext", 1, labB, draws(2, 11, 112, [1, 0], [(0, 0), (0, 0)]), 113, level=2)
    c["B_shift"] = _case("ext", 1, labB, draws(2, 11, 112, [1, 0], [(5, -7), (5, -7)]), 113, level=2)
    # C: selection over 64 channels
    rng = np.random.default_rng(121)
    labC = np.stack([blocky(rng, list(range(1, 57)), 16, 2) for _ in range(2)])
    pC = draws(2, 64, 122, [1, 0], [(0, 0), (1, -2)])
    kids = [f"g{g}c{k}" for g in range(8) for k in range(7)]
    c["C_half"] = _case("wide", 1, labC, pC, 123, level=0, share=0.5, min_pixels=1)
    c["C_all_40"] = _case("wide", 1, labC, pC, 123, level=0, share=1.0, min_pixels=40)
    c["C_kids_all"] = _case("wide", 1, labC, pC, 123, nodes=kids, share=1.0, min_pixels=1)
    c["C_kids_half"] = _case("wide", 1, labC, pC, 123, nodes=kids, share=0.5, min_pixels=1)
    # D: flat model
    c["D"] = _case("tl", 0, _labels("tl", 13, 3, 131), draws(3, 7, 132, [1, 2, 0], [(0, 0), (2, -1), (-1, 3)]), 133, level=0)
    # E: the smallest frames
    c["E_1"] = _case("tl", 1, _labels("tl", 1, 2, 141), draws(2, 8, 142, [1, 0], [(0, 0), (0, 0)]), 143, level=0, share=1.0)
    c["E_3"] = _case("tl", 1, _labels("tl", 3, 2, 144), draws(2, 8, 145, [1, 0], [(0, 0), (1, 0)]), 146, level=0, share=1.0)
    # F: self-paste
    c["F"] = _case("tl", 1, _labels("tl", 30, 1, 151), draws(1, 8, 152, [0], [(2, 1)]), 153, level=0)
    # G: boxes
    c["G"] = _case("tl", 1, _labels("tl", 62, 4, 161), draws(4, 8, 162, [1, 2, 3, 0], [(0, 0), (0, 0), (0, 0), (-5, 9)], boxes=G_BOXES),
                   163, mode="cutmix")
    # H: A with partial labels
    labH = _labels("tl", 62, 5, 171, internal={"tooth": 9}, ignore=[254], without=(2, TOOTH_LEAVES))
    c["H"] = _case("tl", 1, labH, pA, 173, internal={"tooth": 9}, ignore=[254], level=0)
    return c


CASES = _build_cases()
_RESOLVED = {}


def resolved(name):
    """the case with its tensors and the reference's results, computed once and shared (callers must not change them):
    adds x [B,3,S,S], y [B,C,S,S], cand, k_of_n, min_pixels, ref"""
    if name not in _RESOLVED:
        case = dict(CASES[name])
        tree, cmap = tree_of(case["tree"])
        lab = case["labels"]
        case["y"] = PR.encode(lab, tree, cmap, case["model_type"], case["internal"], case["ignore"])
        case["x"] = image(lab.shape[0], 3, lab.shape[1], case["x_seed"])
        kw = case["mix"]
        case["cand"] = candidates(tree, case["model_type"], kw.get("level", 0), kw.get("nodes"))
        case["k_of_n"] = k_of_n(kw.get("share", 0.5))
        case["min_pixels"] = kw.get("min_pixels", 1)
        case["ref"] = mix(case["x"], case["y"], case["params"], case["cand"], case["k_of_n"], case["min_pixels"])
        _RESOLVED[name] = case
    return _RESOLVED[name]
