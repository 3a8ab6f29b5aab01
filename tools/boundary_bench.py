#!/usr/bin/env python
"""Device boundary scoring on the MI355X: median device time of one ops.score_boundaries call (all its launches) for a
batch of four 1400x2900 label-map pairs, on a BLOBBY pair (two unrelated maps with regions tens of pixels wide: outlines
tens of pixels apart, the searches are long) and on a SHIFTED COPY (the truth moved by one row and two columns: what a
good prediction looks like, every search ends in its first round).

    python tools/boundary_bench.py [--batches 30] [--tree tl|ext]

The events bracket ops.score_boundaries as a whole (descriptor checks, the launches; records and workspace are allocated
once outside), so a median may hold a host gap.  Kernel durations without it: run the same command under
`rocprofv3 --kernel-trace --stats -- python ...` (in a run of its own) and read the bd_*_kernel rows there.
There is no stock-torch counterpart to compare with: a distance transform per node and image is what this stage replaces.
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

TREES = {"tl": ("class_tree_tl.json", "class_map.csv"), "ext": ("class_tree_tl_extended.json", "class_map_extended.csv")}


def log(msg):
    print("[boundary_bench] " + msg, file=sys.stderr, flush=True)


def timed(fn, n, warmup=3):
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
    return vals[idx].contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=30)
    ap.add_argument("--tree", choices=sorted(TREES), default="tl")
    a = ap.parse_args()
    from hrseg_amd import ops
    from hrseg_amd.Data import DeviceBoundaryScore
    from hrseg_amd.Data.decode import label_desc
    data_dir = os.path.join(ROOT, "restrictive-hierarchical-semantic-segmentation_amd", "data")
    with open(os.path.join(data_dir, TREES[a.tree][0])) as f:
        tree = json.load(f)
    with open(os.path.join(data_dir, TREES[a.tree][1])) as f:
        cmap = list(csv.DictReader(f))
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    B, H, W = 4, 1400, 2900
    bs = DeviceBoundaryScore(tree, cmap, tolerance=2.0, percentile=95)
    t = bs.tables
    vals = torch.tensor(sorted(v for v in range(256) if t.path[v]), dtype=torch.uint8, device=device)
    host = label_desc([(H, W)] * B)
    desc = host.to(device)
    need = ops.boundary_workspace_bytes(host, t)
    work = torch.empty((need + 7) // 8, dtype=torch.int64, device=device)
    records = torch.empty((B, sum(t.C), 2, len(ops.BOUNDARY_FIELDS)), dtype=torch.int64, device=device)
    res = {"what": f"device boundary scoring, B=4 1400x2900 uint8 label-map pairs, {a.tree} tree ({sum(t.C)} nodes)",
           "pixels": B * H * W, "workspace_mb": round(need / 2 ** 20, 1), "launches_per_call": ops.SCORE_BOUNDARIES_LAUNCHES,
           "batches": a.batches}
    truth = blobby(B, H, W, vals, 2, device)
    shifted = truth.clone()                          # moved down a row and right two columns; the vacated rim keeps the truth
    shifted[:, 1:, 2:] = truth[:, :-1, :-2]
    maps = {"blobby": (blobby(B, H, W, vals, 3, device).reshape(-1), truth.reshape(-1)),
            "shifted": (shifted.reshape(-1).contiguous(), truth.reshape(-1))}
    for name, (pred, gt) in maps.items():
        def kernel():
            ops.score_boundaries(pred, desc, host, gt, desc, host, t, bs.tau2, bs.percentile, out=records, workspace=work)

        ts = timed(kernel, a.batches)
        first = records.clone()
        kernel()
        n = records[..., 0]
        both = (n[..., 0] > 0) & (n[..., 1] > 0)
        ms = statistics.median(ts)
        res[name] = dict(call_ms_median=round(ms, 4), call_ms_min=round(min(ts), 4), border_pixels=int(n.sum()),
                         mpix_per_s=round(B * H * W / (ms * 1e-3) / 1e6, 1),
                         hausdorff_max=round(float(records[..., 2].max()) ** 0.5, 2),
                         nodes_in_both_maps=int(both.sum()), same_bytes_again=bool(torch.equal(first, records)))
        log(json.dumps({name: res[name]}))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
