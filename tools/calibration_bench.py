#!/usr/bin/env python
"""Device calibration scoring on the MI355X: median device time of one DeviceCalibrationScore.score call (one launch plus
the allocation of its records) for a batch of four sets of tl-tree logits at S x S against label maps at H x W, next to the
stock composition of the same figures in torch on the same card: F.interpolate of every level to H x W, sigmoid / group
soft-max composition, and per tree node two torch.histc calls (all events, positive events) -- which is LESS than the kernel
accumulates (no sum of confidences, no squared error, no top-label rows).

    python tools/calibration_bench.py [--S 620 --H 1400 --W 2900 --batches 20 --bins 15]

The logits are confident where the label map says so (about 32 elliptical "teeth" on background, as tools/instances_bench.py
draws them) plus unit noise: most lanes of a wave then hit the same histogram cell, which is the kernel's hard case.  The
events bracket the Python call as a whole, so a median may hold a host gap.  Prints one JSON line."""
from __future__ import annotations

import argparse
import csv
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from instances_bench import blobs, timed  # noqa: E402


def log(msg):
    print("[calibration_bench] " + msg, file=sys.stderr, flush=True)


def stock(logits, gt, sizes, lut0, lut1, bins):
    """the same reliability counts the stock way: full-size fp32 probability planes, then histc per node"""
    B, out = logits[0].shape[0], []
    H, W = sizes
    z0 = F.interpolate(logits[0], size=(H, W), mode="bilinear", align_corners=False)
    z1 = F.interpolate(logits[1], size=(H, W), mode="bilinear", align_corners=False)
    p0 = torch.sigmoid(z0)
    p1 = p0[:, 3:4] * torch.softmax(z1, dim=1)
    g = gt.reshape(B, H, W).long()
    g0, g1 = lut0[g], lut1[g]
    valid = g0 >= 0
    for p, gl in ((p0, g0), (p1, g1)):
        for c in range(p.shape[1]):
            pc = p[:, c]
            out.append(torch.histc(pc[valid], bins=bins, min=0.0, max=1.0))
            out.append(torch.histc(pc[valid & (gl == c)], bins=bins, min=0.0, max=1.0))
    return torch.stack(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--S", type=int, default=620)
    ap.add_argument("--H", type=int, default=1400)
    ap.add_argument("--W", type=int, default=2900)
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--bins", type=int, default=15)
    a = ap.parse_args()
    from hrseg_amd.Data import DeviceCalibrationScore
    from hrseg_amd.Data.decode import label_desc
    data_dir = os.path.join(ROOT, "restrictive-hierarchical-semantic-segmentation_amd", "data")
    with open(os.path.join(data_dir, "class_tree_tl.json")) as f:
        tree = json.load(f)
    with open(os.path.join(data_dir, "class_map.csv")) as f:
        cmap = list(csv.DictReader(f))
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    B, S, H, W = 4, a.S, a.H, a.W
    cal = DeviceCalibrationScore(tree, cmap, 1, n_bins=a.bins)
    host = label_desc([(H, W)] * B)
    desc = host.to(device)
    gt = blobs(B, H, W, 170, 5, device)                              # dentin on background
    small = F.interpolate(gt[:, None].float(), size=(S, S), mode="nearest")[:, 0] > 0
    g = torch.Generator(device="cpu").manual_seed(7)
    z0 = torch.randn(B, 4, S, S, generator=g).to(device) - 3.0
    z0[:, 0] += 6.0 * (~small)
    z0[:, 3] += 6.0 * small
    z1 = torch.randn(B, 4, S, S, generator=g).to(device)
    z1[:, 1] += 4.0 * small
    logits = [z0.contiguous(), z1.contiguous()]
    gt = gt.reshape(-1)
    lut0 = torch.full((256,), -1, dtype=torch.long, device=device)
    lut1 = torch.full((256,), -1, dtype=torch.long, device=device)
    for v, e in enumerate(cal.score_tables.path):
        if e:
            lut0[v], lut1[v] = (e & 0xFF) - 1, ((e >> 8) & 0xFF) - 1
    rows = sum(cal.tables.C) + len(cal.tables.C)
    moved = 4 * B * S * S * sum(cal.tables.C) + B * H * W + 8 * rows * (a.bins + 1) * 4
    res = {"what": f"device calibration scoring, B={B} logits {S}x{S} (tl tree, 4 + 4 channels) -> maps {H}x{W}, {a.bins} bins",
           "pixels": B * H * W, "bytes_per_batch": moved, "batches": a.batches}
    steps = {"score_calibration": lambda: cal.score(logits, (gt, desc, host)),
             "stock_torch": lambda: stock(logits, gt, (H, W), lut0, lut1, a.bins)}
    for name, fn in steps.items():
        ts = timed(fn, a.batches)
        ms = statistics.median(ts)
        res[name] = dict(call_ms_median=round(ms, 4), call_ms_min=round(min(ts), 4), mpix_per_s=round(B * H * W / (ms * 1e-3) / 1e6, 1))
        log(json.dumps({name: res[name]}))
    res["speedup_over_stock"] = round(res["stock_torch"]["call_ms_median"] / res["score_calibration"]["call_ms_median"], 2)
    first, again = cal.score(logits, (gt, desc, host)), cal.score(logits, (gt, desc, host))
    res["same_bytes_again"] = bool(torch.equal(first.hist, again.hist))
    s = first.summary()
    res["background"] = {k: s["background"][k] for k in ("n", "prevalence", "mean_confidence", "ece", "brier")}
    res["top@0"] = {k: s["top@0"][k] for k in ("n", "prevalence", "mean_confidence", "ece", "brier")}
    # the stock counts agree with the kernel's up to events on a bin edge (fp32 histc bins by p * bins, the kernel by q)
    counts = stock(logits, gt, (H, W), lut0, lut1, a.bins)[0::2].sum(1).long().tolist()
    res["stock_events_per_node"] = counts[0]
    res["events_per_node"] = int(first.hist[0, 0, :, 0].sum())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
