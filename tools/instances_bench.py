#!/usr/bin/env python
"""Device instance scoring on the MI355X: median device time of one DeviceInstanceScore.score call (the masked copy, two
labellings, the four scoring launches and the allocation of its outputs) for a batch of four label-map pairs with about 32
elliptical "teeth" each -- the prediction is the truth's blobs moved by a few pixels, a few of them dropped -- next to one
ops.label_components and one ops.score_boundaries call on the same maps.

    python tools/instances_bench.py --size 620 [--batches 30]        # four maps of 620 x 620
    python tools/instances_bench.py --size 1400                      # four maps of 1400 x 2800

One size per run, so that a caller can give every run its own time limit.  The events bracket the Python call as a whole,
so a median may hold a host gap; kernel durations without it: the same command under
`rocprofv3 --kernel-trace --stats -- python ...` (in a run of its own), the in_*_kernel and cc_*_kernel rows.
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

SIZES = {620: (620, 620), 1400: (1400, 2800)}


def log(msg):
    print("[instances_bench] " + msg, file=sys.stderr, flush=True)


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


def blobs(B, H, W, value, seed, device, shift=0, drop=0.0):
    """8 x 4 ellipses per map on a jittered grid (the same grid for one seed), moved by up to `shift` pixels, `drop` of them
    left out -> [B, H, W] uint8"""
    g = torch.Generator().manual_seed(seed)
    gy, gx = 4, 8
    cy = (torch.arange(gy) + 0.5)[None, :, None] * (H / gy) + (torch.rand(B, gy, gx, generator=g) - 0.5) * (H / gy) * 0.2
    cx = (torch.arange(gx) + 0.5)[None, None, :] * (W / gx) + (torch.rand(B, gy, gx, generator=g) - 0.5) * (W / gx) * 0.2
    ry = (0.28 + 0.1 * torch.rand(B, gy, gx, generator=g)) * (H / gy)
    rx = (0.28 + 0.1 * torch.rand(B, gy, gx, generator=g)) * (W / gx)
    g2 = torch.Generator().manual_seed(seed + 1000)
    keep = torch.rand(B, gy, gx, generator=g2) >= drop
    cy = cy + (torch.rand(B, gy, gx, generator=g2) * 2 - 1) * shift
    cx = cx + (torch.rand(B, gy, gx, generator=g2) * 2 - 1) * shift
    cy, cx, ry, rx, keep = (t.reshape(B, -1, 1, 1).to(device) for t in (cy, cx, ry, rx, keep))
    yy = torch.arange(H, device=device, dtype=torch.float32).view(1, 1, H, 1)
    xx = torch.arange(W, device=device, dtype=torch.float32).view(1, 1, 1, W)
    out = torch.zeros((B, H, W), dtype=torch.uint8, device=device)
    for k in range(gy * gx):                                         # (one ellipse at a time: no [B, 32, H, W] tensor)
        inside = (((yy - cy[:, k:k + 1]) / ry[:, k:k + 1]) ** 2 + ((xx - cx[:, k:k + 1]) / rx[:, k:k + 1]) ** 2 <= 1.0) & keep[:, k:k + 1]
        out[inside[:, 0]] = value
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, choices=sorted(SIZES), default=620)
    ap.add_argument("--batches", type=int, default=30)
    a = ap.parse_args()
    from hrseg_amd import ops
    from hrseg_amd.Data import DeviceBoundaryScore, DeviceInstanceScore
    from hrseg_amd.Data.decode import label_desc
    data_dir = os.path.join(ROOT, "restrictive-hierarchical-semantic-segmentation_amd", "data")
    with open(os.path.join(data_dir, "class_tree_tl.json")) as f:
        tree = json.load(f)
    with open(os.path.join(data_dir, "class_map.csv")) as f:
        cmap = list(csv.DictReader(f))
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    B, (H, W) = 4, SIZES[a.size]
    inst = DeviceInstanceScore(tree, cmap, 0, ["tooth"])
    bs = DeviceBoundaryScore(tree, cmap)
    host = label_desc([(H, W)] * B)
    desc = host.to(device)
    gt = blobs(B, H, W, 170, 5, device).reshape(-1)
    pred = blobs(B, H, W, 170, 5, device, shift=max(2, H // 150), drop=0.1).reshape(-1)
    group = inst.device_tables(device)[0]
    need = ops.instances_workspace_bytes(host, host)
    work = torch.empty((need + 7) // 8, dtype=torch.int64, device=device)
    bneed = ops.boundary_workspace_bytes(host, bs.tables)
    bwork = torch.empty((bneed + 7) // 8, dtype=torch.int64, device=device)
    res = {"what": f"device instance scoring, B={B} {H}x{W} uint8 label-map pairs, 32 blobs each, things = tooth", "pixels": B * H * W,
           "workspace_mb": round(need / 2 ** 20, 1), "launches_per_score": ops.SCORE_INSTANCES_LAUNCHES + 2 * ops.LABEL_COMPONENTS_LAUNCHES,
           "batches": a.batches}
    steps = {"score_instances": lambda: inst.score((pred, desc, host), (gt, desc, host), workspace=work),
             "label_components": lambda: ops.label_components(gt, desc, host, group, 8),
             "score_boundaries": lambda: ops.score_boundaries(pred, desc, host, gt, desc, host, bs.tables, bs.tau2, bs.percentile,
                                                              workspace=bwork)}
    for name, fn in steps.items():
        ts = timed(fn, a.batches)
        ms = statistics.median(ts)
        res[name] = dict(call_ms_median=round(ms, 4), call_ms_min=round(min(ts), 4), mpix_per_s=round(B * H * W / (ms * 1e-3) / 1e6, 1))
        log(json.dumps({name: res[name]}))
    first = inst.score((pred, desc, host), (gt, desc, host), workspace=work)
    again = inst.score((pred, desc, host), (gt, desc, host), workspace=work)
    res["same_bytes_again"] = all(bool(torch.equal(getattr(first, k), getattr(again, k))) for k in ("records", "pmatch", "gmatch", "ginter"))
    s = first.summary()["tooth"]
    res["tooth"] = {k: s[k] for k in ("n_gt", "n_pred", "tp", "fp", "fn", "rq", "sq", "pq")}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
