#!/usr/bin/env python
"""Hedged decode on the MI355X: median device time between events of 20 calls each, for a batch of four sets of tl-tree
logits at S x S decoded to H x W:

    (a) DeviceDecode.decode(want_confidence=True)            -- the plain decode, the yardstick of the same run
    (b) DeviceDecode.decode_hedged at tau = 0, with confidence and counters (the same labels and confidence as (a))
    (c) DeviceDecode.decode_hedged at tau = 0.5
    (d) the stock route in torch: F.interpolate of all logits to H x W, composition, thresholding with torch.where, bincount

    python tools/hedge_bench.py [--S 620 --H 1400 --W 2900 --calls 20]

The logits are those of tools/calibration_bench.py: confident where a label map says so (about 32 elliptical "teeth" on
background) plus unit noise, so most lanes of a wave count into the same cell.  The four routes alternate call by call after a
warm-up of each; the events bracket the Python call as a whole (its allocations included), so a median may hold a host gap.
Prints one JSON line; (a)'s min-max spread is in it: a difference between (a) and (b) inside that spread is not a finding."""
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
    print("[hedge_bench] " + msg, file=sys.stderr, flush=True)


def stock(logits, sizes, tau, leaf0, leaf1, tooth_byte, cell0, cell1):
    """the tl tree's hedged decode the stock way: full-size fp32 planes of every logit, then the composition"""
    H, W = sizes
    z0 = F.interpolate(logits[0], size=(H, W), mode="bilinear", align_corners=False)
    z1 = F.interpolate(logits[1], size=(H, W), mode="bilinear", align_corners=False)
    c0 = z0.argmax(1)
    t0 = torch.sigmoid(z0.gather(1, c0[:, None])[:, 0])
    p1 = torch.softmax(z1, dim=1)
    c1 = z1.argmax(1)
    t1 = t0 * p1.gather(1, c1[:, None])[:, 0]
    tooth = c0 == 3
    deep = tooth & ~(t1 < tau)
    labels = torch.where(deep, leaf1[c1], torch.where(tooth, tooth_byte, leaf0[c0]))
    conf = torch.where(deep, t1, t0)
    cells = torch.where(deep, cell1[c1], cell0[c0])
    stops = torch.stack([torch.bincount(cells[b].reshape(-1), minlength=10) for b in range(cells.shape[0])])
    return labels, conf, stops


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--S", type=int, default=620)
    ap.add_argument("--H", type=int, default=1400)
    ap.add_argument("--W", type=int, default=2900)
    ap.add_argument("--calls", type=int, default=20)
    a = ap.parse_args()
    from hrseg_amd.Data import DeviceDecode, Hedge
    from hrseg_amd.Data.decode import label_desc
    data_dir = os.path.join(ROOT, "restrictive-hierarchical-semantic-segmentation_amd", "data")
    with open(os.path.join(data_dir, "class_tree_tl.json")) as f:
        tree = json.load(f)
    with open(os.path.join(data_dir, "class_map.csv")) as f:
        cmap = list(csv.DictReader(f))
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    B, S, H, W = 4, a.S, a.H, a.W
    dec = DeviceDecode(tree, cmap, 1)
    zero, half = Hedge(tree, cmap, 0.0), Hedge(tree, cmap, 0.5)
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
    t = dec.tables
    leaf0 = torch.tensor([max(v, 0) for v in t.pixel_val[0]], dtype=torch.uint8, device=device)
    leaf1 = torch.tensor(t.pixel_val[1], dtype=torch.uint8, device=device)
    tooth_byte = torch.tensor(half.values["tooth"], dtype=torch.uint8, device=device)
    cell0, cell1 = torch.arange(4, device=device), torch.arange(4, 8, device=device)
    moved = 4 * B * S * S * sum(t.C) + 5 * B * H * W + 8 * B * (sum(t.C) + 2)
    res = {"what": f"hedged decode, B={B} logits {S}x{S} (tl tree, 4 + 4 channels) -> maps {H}x{W} with confidence",
           "pixels": B * H * W, "bytes_per_batch_if_every_logit_is_read_once": moved, "calls": a.calls}
    steps = {"a_decode_plain": lambda: dec.decode(logits, desc, host, True),
             "b_decode_hedged_tau0": lambda: dec.decode_hedged(logits, zero, desc, host, True),
             "c_decode_hedged_tau05": lambda: dec.decode_hedged(logits, half, desc, host, True),
             "d_stock_torch": lambda: stock(logits, (H, W), 0.5, leaf0, leaf1, tooth_byte, cell0, cell1)}
    # the four routes alternate call by call, so that a drift of the box hits them alike
    for fn in steps.values():
        timed(fn, 0)                                                     # (warm-up only)
    times = {name: [] for name in steps}
    for _ in range(a.calls):
        for name, fn in steps.items():
            times[name] += timed(fn, 1, warmup=0)
    for name in steps:
        ts = times[name]
        ms = statistics.median(ts)
        res[name] = dict(call_ms_median=round(ms, 4), call_ms_min=round(min(ts), 4), call_ms_max=round(max(ts), 4),
                         mpix_per_s=round(B * H * W / (ms * 1e-3) / 1e6, 1))
        log(json.dumps({name: res[name]}))
    plain, hz, hh = dec.decode(logits, desc, host, True), dec.decode_hedged(logits, zero, desc, host, True), \
        dec.decode_hedged(logits, half, desc, host, True)
    res["tau0_is_the_plain_decode"] = bool(torch.equal(plain.labels, hz.labels) and
                                           torch.equal(plain.confidence.view(torch.int32), hz.confidence.view(torch.int32)))
    labels, conf, stops = stock(logits, (H, W), 0.5, leaf0, leaf1, tooth_byte, cell0, cell1)
    res["stock_labels_differing"] = int((labels.reshape(-1) != hh.labels).sum())      # (fp32 resize of torch vs the kernel's: near ties)
    res["summary_tau05"] = hh.summary()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
