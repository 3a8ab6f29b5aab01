#!/usr/bin/env python
"""Device scoring pipeline on the MI355X: (1) the scoring kernel for a batch of four 1400x2900 label-map pairs on the tl
tree (events around each call, warm-up, median of --batches), on a BLOBBY pair (label regions tens of pixels wide: long
runs of one pair, what a trained model and a ground truth look like) and on a UNIFORMLY RANDOM pair (no runs at all: the
worst case of the run folding), (2) the same counts composed from stock torch GPU ops (table gathers plus one
torch.bincount per level), timed the same way in the same process -- the yardstick; its counts must equal the kernel's.

    python tools/score_bench.py [--batches 60]

The events bracket ops.score_labels as a whole (descriptor checks, the launch; the output tensors are allocated once
outside), so a median may hold a host gap.  Kernel durations without it: run the same command under
`rocprofv3 --kernel-trace --stats -- python ...` (in a run of its own) and read score_labels_kernel there.
Prints one JSON line."""
from __future__ import annotations

import argparse
import csv
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

HBM_PEAK_TBS = 8.0          # MI355X_MICROARCH.md: HBM3E peak


def log(msg):
    print("[score_bench] " + msg, file=sys.stderr, flush=True)


def timed(fn, n, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return ts


def blobby(B, H, W, vals, seed, device):
    """arg-max of coarse noise upsampled bicubically: regions tens of pixels wide"""
    g = torch.Generator().manual_seed(seed)
    base = torch.randn(B, len(vals), H // 48 + 2, W // 48 + 2, generator=g).to(device)
    idx = F.interpolate(base, size=(H, W), mode="bicubic", align_corners=False).argmax(1)
    return vals[idx].reshape(-1).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=60)
    a = ap.parse_args()
    from hrseg_amd import ops
    from hrseg_amd.Data import DeviceScore
    from hrseg_amd.Data.decode import label_desc
    data_dir = os.path.join(ROOT, "restrictive-hierarchical-semantic-segmentation_amd", "data")
    with open(os.path.join(data_dir, "class_tree_tl.json")) as f:
        tree = json.load(f)
    with open(os.path.join(data_dir, "class_map.csv")) as f:
        cmap = list(csv.DictReader(f))
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    B, H, W = 4, 1400, 2900
    sc = DeviceScore(tree, cmap)
    t = sc.tables
    vals = torch.tensor(sorted(v for v in range(256) if t.path[v]), dtype=torch.uint8, device=device)
    host = label_desc([(H, W)] * B)
    desc = host.to(device)
    lut = t.device_lut(device)
    res = {"what": "device scoring, B=4 1400x2900 uint8 label-map pairs, tl tree, per-image counts", "pixels": B * H * W,
           "bytes_per_batch": 2 * B * H * W, "batches": a.batches}

    def stock(pred, gt):
        """the per-pixel rule from table gathers, one bincount per level and image"""
        g, p = lut[gt.long()], lut[pred.long()]
        ok = (g != 0) & (p != 0)
        rows = []
        for b in range(B):
            s = slice(b * H * W, (b + 1) * H * W)
            gb, pb, okb = g[s], p[s], ok[s]
            row = []
            for L, (C, K) in enumerate(zip(t.C, t.K)):
                gl, pl = (gb >> (8 * L)) & 0xFF, (pb >> (8 * L)) & 0xFF
                if L == 0:
                    cell = (gl - 1) * C + (pl - 1)
                else:
                    agree = ((gb >> (8 * (L - 1))) & 0xFF) == ((pb >> (8 * (L - 1))) & 0xFF)
                    cell = gl * K + torch.where(agree, pl, torch.zeros_like(pl))
                row.append(torch.bincount(cell[okb], minlength=K * K))
            rows.append(torch.cat(row))
        return torch.stack(rows)

    g = torch.Generator().manual_seed(1)
    maps = {"blobby": (blobby(B, H, W, vals, 2, device), blobby(B, H, W, vals, 3, device)),
            "random": (vals[torch.randint(0, len(vals), (B * H * W,), generator=g).to(device)],
                       vals[torch.randint(0, len(vals), (B * H * W,), generator=g).to(device)])}
    counts = ops.zeros((B, t.total), torch.int64, device)
    ignored = ops.zeros((B, 2), torch.int64, device)
    for name, (pred, gt) in maps.items():
        def kernel():
            ops.score_labels(pred, desc, host, gt, desc, host, t, (counts, ignored))

        ts = timed(kernel, a.batches)
        tt = timed(lambda: stock(pred, gt), max(a.batches // 6, 3), warmup=1)
        fresh, _ = ops.score_labels(pred, desc, host, gt, desc, host, t)
        same = bool(torch.equal(fresh, stock(pred, gt)))
        ms, mst = statistics.median(ts), statistics.median(tt)
        res[name] = dict(score_ms_median=round(ms, 4), score_ms_min=round(min(ts), 4),
                         achieved_tb_s=round(2 * B * H * W / (ms * 1e-3) / 1e12, 3),
                         fraction_of_hbm_peak=round(2 * B * H * W / (ms * 1e-3) / 1e12 / HBM_PEAK_TBS, 4),
                         stock_torch_ms_median=round(mst, 4), stock_torch_ms_min=round(min(tt), 4),
                         speedup_over_stock=round(mst / ms, 2), counts_equal_stock=same)
        log(json.dumps({name: res[name]}))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
