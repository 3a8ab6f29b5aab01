#!/usr/bin/env python
"""Sliding-window inference on the MI355X: two 1400x2900 three-channel sources, windows of 620, overlap 0.5 (4 x 9 windows
per image, 72 in all; tl tree, model_type 1).  Device events around each call, a warm-up, medians of --batches:
(1) ops.window_crops (sources -> [72,3,620,620]); (2) ops.decode_windows of synthetic window logits to the two 1400x2900
label maps, with and without the confidence; (3) in the same process and alternating with (2), ops.decode_labels of two
620x620 logit sets to the same output size -- what a label map costs without windows (tools/decode_bench.py).

    python tools/window_bench.py [--batches 40]

The events bracket the Python wrappers as a whole (table checks, small host-to-device copies, allocations, the launch), so
a median may hold a host gap.  Prints one JSON line."""
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

import numpy as np  # noqa: E402
import torch  # noqa: E402

from decode_bench import smooth_logits, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=40)
    a = ap.parse_args()
    from hrseg_amd import ops
    from hrseg_amd.Data import DeviceDecode
    from hrseg_amd.Data.decode import label_desc, pack_images
    from hrseg_amd.predictEval import SlidingWindow
    data_dir = os.path.join(ROOT, "restrictive-hierarchical-semantic-segmentation_amd", "data")
    with open(os.path.join(data_dir, "class_tree_tl.json")) as f:
        tree = json.load(f)
    with open(os.path.join(data_dir, "class_map.csv")) as f:
        cmap = list(csv.DictReader(f))
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    B, S, H, W = 2, 620, 1400, 2900
    window = SlidingWindow(overlap=0.5)
    plan, prof = window.plan([(H, W)] * B, S), window.profile(S)
    assert plan.wdesc[:, 2:4].tolist() == [[4, 9]] * B and plan.nwindows == 72
    dec = DeviceDecode(tree, cmap, 1)
    rng = np.random.default_rng(0)
    src, shost = pack_images([rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8) for _ in range(B)])
    src, sdesc = src.to(device), shost.to(device)
    zw = smooth_logits(plan.nwindows, dec.tables.C, S, 0, device)
    z1 = smooth_logits(B, dec.tables.C, S, 1, device)
    host = label_desc([(H, W)] * B)
    desc = host.to(device)
    out = {}

    def crops():
        out["x"] = ops.window_crops(src, sdesc, shost, plan, S)

    def windows(conf=False):
        out["wl"], out["wc"] = ops.decode_windows(zw, dec.tables, plan, prof, desc, host, conf)

    def single(conf=False):
        out["l"], out["c"] = ops.decode_labels(z1, dec.tables, desc, host, conf)

    n = max(a.batches // 4, 1)
    tc = timed(crops, a.batches)
    tw, ts, twc, tsc = [], [], [], []
    for _ in range(4):                       # alternate, so that both decodes see the same machine state
        tw += timed(windows, n)
        ts += timed(single, n)
        twc += timed(lambda: windows(True), n)
        tsc += timed(lambda: single(True), n)
    med = statistics.median
    res = dict(what="sliding-window inference, 2 sources of 1400x2900x3, S=620, overlap 0.5: 72 windows (tl tree, model_type 1)",
               batches=a.batches, window_crops_ms_median=round(med(tc), 4), window_crops_ms_min=round(min(tc), 4),
               crops_bytes_written=plan.nwindows * 3 * S * S * 4,
               decode_windows_ms_median=round(med(tw), 4), decode_windows_ms_min=round(min(tw), 4),
               decode_windows_with_confidence_ms_median=round(med(twc), 4),
               decode_labels_ms_median=round(med(ts), 4), decode_labels_ms_min=round(min(ts), 4),
               decode_labels_with_confidence_ms_median=round(med(tsc), 4),
               windows_over_plain=round(med(tw) / med(ts), 2), windows_over_plain_with_confidence=round(med(twc) / med(tsc), 2),
               pixels=B * H * W)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
