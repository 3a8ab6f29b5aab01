#!/usr/bin/env python
"""Mixing augmentation on the MI355X: device time of `DeviceMix` and of its three kernels against a torch composition that
computes the same outputs, for B = 4 samples of 620 x 620, the tl tree (C = 8) and a 21-node tree (4 groups of 4 children),
ClassMix at level 0, shift 0 and shift (37, -11):

    mix          the whole `mix(x, y)` through Python: table packing, two small uploads, counts, masks, two gathers
    counts       hrseg_mix_counts on y
    masks        hrseg_mix_masks
    gather_x     hrseg_mix_gather on x [B,3,S,S]
    gather_y     hrseg_mix_gather on y [B,C,S,S]
    torch        index_select of the donors, roll for the shift, `==` / `any` for the mask, `where` on x and y (the chosen
                 channels handed in as a ready [B,C] bool table: the composition pays for no counting and no selection)

    python tools/mix_bench.py [--S 620 --B 4 --rounds 7 --calls 20]

Device events around `calls` back-to-back calls of one variant behind a blocker (a large memset that lets the host run ahead,
so the events see the device's time, not Python's); the variants alternate round by round after a warm-up of each; median,
min and max over the rounds of the per-call time.  The inputs rotate over copies whose footprint is larger than the 256 MiB
Infinity Cache, so the rates are HBM rates.  Bytes per second are taken against the byte floor: one read of y for the
counts; the chosen channels of the applied samples plus the mask for the masks (an upper bound: a pixel stops at its first
hit); one read plus one write of the tensor plus the mask for a gather.  The tool asserts that the composition's outputs equal
the mix's bit for bit before it times anything.  Prints one JSON line."""
from __future__ import annotations

import argparse
import csv
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def log(msg):
    print("[mix_bench] " + msg, file=sys.stderr, flush=True)


def wide_tree():
    """21 nodes: background and 4 groups of 4 children"""
    tree, cmap, v = {"background": {}}, [{"class_name": "background", "pixel_val": "0"}], 10
    for g in range(4):
        tree[f"group{g}"] = {}
        cmap.append({"class_name": f"group{g}", "pixel_val": "None"})
        for k in range(4):
            tree[f"group{g}"][f"g{g}c{k}"] = {}
            cmap.append({"class_name": f"g{g}c{k}", "pixel_val": str(v)})
            v += 10
    return tree, cmap


def label_maps(B, S, values, seed, block=31):
    rng = np.random.default_rng(seed)
    coarse = rng.choice(np.asarray(values, dtype=np.uint8), size=(B, S // block + 1, S // block + 1))
    return torch.from_numpy(np.ascontiguousarray(np.repeat(np.repeat(coarse, block, 1), block, 2)[:, :S, :S]))


def stock(x, y, donor, sel, inframe, dx, dy):
    """the same outputs with stock torch ops: several full-size passes and temporaries"""
    xd = torch.roll(x.index_select(0, donor), shifts=(dy, dx), dims=(2, 3))
    yd = torch.roll(y.index_select(0, donor), shifts=(dy, dx), dims=(2, 3))
    mask = ((yd == 1.0) & sel[:, :, None, None]).any(dim=1) & inframe
    return torch.where(mask[:, None], xd, x), torch.where(mask[:, None], yd, y), mask


def rounds_of(variants, rounds, calls, blocker):
    """{name: [per-call microseconds, one per round]}; the variants alternate round by round"""
    for fn in variants.values():
        for i in range(3):
            fn(i)
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            blocker.zero_()
            blocker.zero_()
            e0.record()
            for i in range(calls):
                fn(i)
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / calls)
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--S", type=int, default=620)
    ap.add_argument("--B", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    a = ap.parse_args()
    from hrseg_amd import _lib, ops
    from hrseg_amd.Data import DeviceMix, TargetEncoder
    from hrseg_amd.Data.dataset import _name2pix
    data_dir = os.path.join(ROOT, "restrictive-hierarchical-semantic-segmentation_amd", "data")
    with open(os.path.join(data_dir, "class_tree_tl.json")) as f:
        tl = json.load(f)
    with open(os.path.join(data_dir, "class_map.csv")) as f:
        tl_map = list(csv.DictReader(f))
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    B, S = a.B, a.S
    blocker = torch.empty(1 << 30, dtype=torch.uint8, device=device)
    res = {"what": f"mixing augmentation, B={B}, {S}x{S}, ClassMix at level 0, share 0.5", "rounds": a.rounds, "calls": a.calls,
           "cases": {}}
    for key, (tree, cmap) in {"tl_C8": (tl, tl_map), "wide_C21": wide_tree()}.items():
        enc = TargetEncoder(tree, cmap, 1)
        Cn = len(enc.names)
        y0 = enc(label_maps(B, S, sorted(_name2pix(cmap).values()), 5).to(device))
        x0 = torch.randn(B, 3, S, S, generator=torch.Generator().manual_seed(6)).to(device)
        copies = max(2, -(-(320 << 20) // (8 * y0.numel())))                    # inputs + outputs beyond the Infinity Cache
        xs, ys = [x0.clone() for _ in range(copies)], [y0.clone() for _ in range(copies)]
        xo, yo = [torch.empty_like(x0) for _ in range(copies)], [torch.empty_like(y0) for _ in range(copies)]
        for shift in ((0, 0), (37, -11)):
            mix = DeviceMix(tree, cmap, 1, level=0, seed=3)
            p = mix.sample(B)
            p["dx"][:], p["dy"][:] = shift
            x2, y2 = mix(x0, y0, params=p)
            table, prio = (t.to(device) for t in mix.pack_params(p, S))
            counts, mask, chosen = mix.last_counts, mix.last_mask, mix.last_chosen.tolist()
            # the composition computes the same bytes
            donor = p["donor"].to(device)
            sel = torch.tensor([[(bits >> c) & 1 for c in range(Cn)] for bits in chosen], dtype=torch.bool, device=device)
            inframe = torch.zeros(S, S, dtype=torch.bool, device=device)
            dx, dy = shift
            inframe[max(0, dy):min(S, S + dy), max(0, dx):min(S, S + dx)] = True
            xs_, ys_, ms_ = stock(x0, y0, donor, sel, inframe, dx, dy)
            assert torch.equal(ms_, mask.bool()) and bool(ms_.any()) and not bool(ms_.all())
            assert torch.equal(xs_.view(torch.int32), x2.view(torch.int32)) and torch.equal(ys_.view(torch.int32), y2.view(torch.int32))
            _lib.launch_count("mix", reset=True)
            mix(x0, y0, params=p)
            launches = _lib.launch_count("mix", reset=True)
            n = copies
            variants = {
                "mix": lambda i: mix(xs[i % n], ys[i % n], params=p),
                "counts": lambda i: ops.mix_counts(ys[i % n]),
                "masks": lambda i: ops.mix_masks(ys[i % n], counts, table, prio, mix.k_of_n, mix.cand, 1),
                "gather_x": lambda i: ops.mix_gather(xs[i % n], mask, table, out=xo[i % n]),
                "gather_y": lambda i: ops.mix_gather(ys[i % n], mask, table, out=yo[i % n]),
                "torch": lambda i: stock(xs[i % n], ys[i % n], donor, sel, inframe, dx, dy),
            }
            hw = S * S
            floor = {"counts": 4 * B * Cn * hw, "masks": B * hw + 4 * hw * sum(bin(b & (2**64 - 1)).count("1") for b in chosen),
                     "gather_x": 8 * B * 3 * hw + B * hw, "gather_y": 8 * B * Cn * hw + B * hw}
            floor["mix"] = sum(floor.values())
            times = rounds_of(variants, a.rounds, a.calls, blocker)
            out = {"launches": launches, "pasted_share": round(float(mask.float().mean()), 3),
                   "chosen": mix.chosen_names(), "input_copies": copies}
            for name, ts in times.items():
                us = statistics.median(ts)
                out[name] = dict(us_median=round(us, 2), us_min=round(min(ts), 2), us_max=round(max(ts), 2))
                if name in floor:
                    out[name]["floor_bytes"] = floor[name]
                    out[name]["tb_per_s"] = round(floor[name] / (us * 1e-6) / 1e12, 3)
            res["cases"][f"{key}_shift_{dx}_{dy}"] = out
            log(json.dumps({f"{key}_shift_{dx}_{dy}": out}))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
