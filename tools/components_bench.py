#!/usr/bin/env python
"""Device post-processing on the MI355X: DevicePostprocess.apply (connected components + filter, 6 launches) on a batch of
four 1500x3000 label maps decoded from 620x620 synthetic logits of the tl tree (smooth label regions tens of pixels wide,
as tools/decode_bench.py makes them), beside ops.decode_labels for the same maps in the same run.  Events around each call,
warm-up, median of --batches; both figures per megapixel.  The labelling and the filter are also timed on their own, and on
two hard inputs of the same size: a checkerboard and independent noise.

    python tools/components_bench.py [--batches 40] [--connectivity 8]

The events bracket the Python calls as a whole (descriptor checks, allocations, the launches), so a median may hold a host
gap; kernel durations without it: the same command under `rocprofv3 --kernel-trace --stats -- python ...` in a run of its
own.  Prints one JSON line."""
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

from decode_bench import smooth_logits, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=40)
    ap.add_argument("--connectivity", type=int, default=8, choices=(4, 8))
    a = ap.parse_args()
    from hrseg_amd import ops
    from hrseg_amd.Data import DeviceDecode, DevicePostprocess, RaggedLabels
    from hrseg_amd.Data.decode import label_desc
    data_dir = os.path.join(ROOT, "restrictive-hierarchical-semantic-segmentation_amd", "data")
    with open(os.path.join(data_dir, "class_tree_tl.json")) as f:
        tree = json.load(f)
    with open(os.path.join(data_dir, "class_map.csv")) as f:
        cmap = list(csv.DictReader(f))
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    B, S, H, W = 4, 620, 1500, 3000
    mpix = B * H * W / 1e6
    dec = DeviceDecode(tree, cmap, 1)
    z = smooth_logits(B, dec.tables.C, S, 0, device)
    host = label_desc([(H, W)] * B)
    desc = host.to(device)
    rules = {"tooth": dict(min_area=200), "upper": dict(keep_largest=True), "lower": dict(keep_largest=True),
             "background": dict(min_area=200)}
    pp = DevicePostprocess(tree, cmap, 0, rules, a.connectivity)
    group, rule_table = pp.tables.device(device)
    out = {}

    def decode():
        out["labels"], _ = ops.decode_labels(z, dec.tables, desc, host, False)

    decode()
    maps = RaggedLabels(out["labels"], None, desc, host)

    def apply():
        out["clean"] = pp.apply(maps)

    def label(buf=None):
        out["roots"], out["area"] = ops.label_components(maps.labels if buf is None else buf, desc, host, group, a.connectivity)

    def filt():
        ops.filter_components(maps.labels, desc, host, group, rule_table, out["roots"], out["area"])

    td, ta, tl = timed(decode, a.batches), timed(apply, a.batches), timed(label, a.batches)
    label()
    tf = timed(filt, a.batches)
    stats = pp.last_stats.sum(0)[:4].tolist()
    res = {"what": f"DevicePostprocess.apply, B=4 1500x3000 maps decoded from 620x620 logits (tl tree, level 0, "
                   f"{a.connectivity}-connectivity)", "batches": a.batches, "megapixels": mpix}
    for key, ts in (("decode_labels", td), ("apply", ta), ("label_components", tl), ("filter_components", tf)):
        res[key + "_ms_median"] = round(statistics.median(ts), 4)
        res[key + "_us_per_megapixel"] = round(1e3 * statistics.median(ts) / mpix, 2)
    res["components_found_removed_pixels_by_group"] = stats
    # hard inputs at the same size: every pixel its own component / two components / noise
    yy, xx = torch.meshgrid(torch.arange(H, device=device), torch.arange(W, device=device), indexing="ij")
    board = torch.where((yy + xx) % 2 == 0, 0, 212).to(torch.uint8).reshape(-1).repeat(B)
    noise = torch.tensor([0, 212, 255, 127], dtype=torch.uint8, device=device)[torch.randint(0, 4, (B * H * W,), device=device)]
    for key, buf in (("checkerboard", board), ("noise4", noise)):
        ts = timed(lambda: label(buf), max(a.batches // 4, 5), warmup=2)
        res[f"label_components_{key}_ms_median"] = round(statistics.median(ts), 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
