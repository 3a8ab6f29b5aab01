#!/usr/bin/env python
"""Device output pipeline on the MI355X: (1) the decode kernel for a batch of four 1400x2900 label maps from 620x620
logits of the tl tree (events around each call, warm-up, median of --batches; bytes moved over that time against the
HBM peak), with and without the confidence, (2) the same labels composed from stock torch GPU ops (F.interpolate per
level, argmax, where, a LUT gather) timed the same way in the same process -- the yardstick --, (3) the host time of
one predictEval.Predictor call (sources -> label maps) on the flagship hierarchical HRNet.

    python tools/decode_bench.py [--batches 60] [--skip-predictor] [--views N]

--views N (1..4) adds test-time augmentation at the same geometry: N flip views (flags 0, H, V, H|V) of 620x620 logits,
(4) the median device time of the fused ops.decode_views, with and without the confidence, (5) beside it N x the median
of the single-view ops.decode_labels on the same inputs (that kernel does not change with this option: the figure is the
taps' cost in N separate launches, each of which also writes the labels), (6) the stock-torch composition of the same
ensemble: flip every view back, F.interpolate every level to the source size, mean, then arg-max, where and the LUT
gather as in (2) (hrseg_decode_labels takes square logits, so it cannot stand in for that last step at 1400x2900).

The events bracket ops.decode_labels as a whole (descriptor check, two allocations, the launch), so a median may hold
a host gap.  Kernel durations without it: run the same command under `rocprofv3 --kernel-trace --stats -- python ...`
(in a run of its own) and read decode_labels_kernel there.  Prints one JSON line."""
from __future__ import annotations

import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

HBM_PEAK_TBS = 8.0          # MI355X_MICROARCH.md: HBM3E peak


def log(msg):
    print("[decode_bench] " + msg, file=sys.stderr, flush=True)


def smooth_logits(B, Cs, S, seed, device):
    """coarse 3*randn noise, bicubically upsampled, plus 0.05*randn: label regions tens of pixels wide, as a trained model's"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for n in Cs:
        base = 3.0 * torch.randn(B, n, S // 8 + 2, S // 8 + 2, generator=g)
        out.append((F.interpolate(base, size=(S, S), mode="bicubic", align_corners=False) +
                    0.05 * torch.randn(B, n, S, S, generator=g)).contiguous().to(device))
    return out


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


def bench_views(a, dec, z, desc, host, B, S, H, W, timed, out):
    """N flip views of the 620 -> 1400x2900 batch: fused decode_views vs N single-view launches vs stock torch"""
    from hrseg_amd import ops
    device = z[0].device
    Cs = dec.tables.C
    dims = {0: [], 1: [-1], 2: [-2], 3: [-2, -1]}
    views = []
    for f in range(a.views):                     # view f: its own logits, as the network would return them for a mirrored input
        zv = smooth_logits(B, Cs, S, 10 + f, device)
        views.append(([torch.flip(t, dims[f]).contiguous() if dims[f] else t for t in zv], f))

    def fused(conf=False):
        out["vlabels"], out["vconf"] = ops.decode_views(views, dec.tables, desc, host, conf)

    def single(conf=False):
        out["labels"], out["conf"] = ops.decode_labels(views[0][0], dec.tables, desc, host, conf)

    n = a.batches
    # alternate the fused and the single-view launches so that both see the same machine state
    tf, ts1, tfc, ts1c = [], [], [], []
    for _ in range(4):
        tf += timed(fused, n // 4 or 1)
        ts1 += timed(single, n // 4 or 1)
        tfc += timed(lambda: fused(True), n // 4 or 1)
        ts1c += timed(lambda: single(True), n // 4 or 1)
    res = dict(views=a.views,
               decode_views_ms_median=round(statistics.median(tf), 4), decode_views_ms_min=round(min(tf), 4),
               decode_views_with_confidence_ms_median=round(statistics.median(tfc), 4),
               single_view_ms_median=round(statistics.median(ts1), 4),
               n_single_view_launches_ms=round(a.views * statistics.median(ts1), 4),
               n_single_view_launches_with_confidence_ms=round(a.views * statistics.median(ts1c), 4),
               views_bytes_per_batch=a.views * B * S * S * 4 * sum(Cs) + B * H * W)
    res["fused_over_n_single"] = round(res["decode_views_ms_median"] / res["n_single_view_launches_ms"], 3)

    # stock torch: the mean logit at source size (flip, interpolate, add, scale per level), then arg-max / where / LUT as above
    parent = [c for c, k in enumerate(dec.tables.n_children[0]) if k][0]
    lut = torch.tensor([v if v >= 0 else 0 for v in dec.tables.pixel_val[0]] + dec.tables.pixel_val[1], dtype=torch.uint8, device=device)

    def stock_views():
        arg = []
        for L in range(len(Cs)):
            acc = None
            for zv, f in views:
                r = F.interpolate(torch.flip(zv[L], dims[f]) if dims[f] else zv[L], size=(H, W), mode="bilinear", align_corners=False)
                acc = r if acc is None else acc + r
            arg.append((acc * (1.0 / len(views))).argmax(1))
        out["slabels"] = lut[torch.where(arg[0] == parent, arg[1] + Cs[0], arg[0])]

    tt = timed(stock_views, max(n // 6, 5), warmup=2)
    fused()
    res.update(stock_torch_views_ms_median=round(statistics.median(tt), 4),
               views_speedup_over_stock=round(statistics.median(tt) / statistics.median(tf), 2),
               views_labels_differing_from_stock=int((out["vlabels"].reshape(B, H, W) != out["slabels"]).sum()))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=60)
    ap.add_argument("--skip-predictor", action="store_true")
    ap.add_argument("--views", type=int, default=0, help="also time the fused decode of N flip views (1..4)")
    a = ap.parse_args()
    if not 0 <= a.views <= 4:
        ap.error("--views takes 1..4 (the four flips of one scale)")
    from hrseg_amd import ops
    from hrseg_amd.Data import DeviceDecode
    from hrseg_amd.Data.decode import label_desc
    data_dir = os.path.join(ROOT, "restrictive-hierarchical-semantic-segmentation_amd", "data")
    with open(os.path.join(data_dir, "class_tree_tl.json")) as f:
        tree = json.load(f)
    with open(os.path.join(data_dir, "class_map.csv")) as f:
        cmap = list(csv.DictReader(f))
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    B, S, H, W = 4, 620, 1400, 2900
    dec = DeviceDecode(tree, cmap, 1)
    Cs = dec.tables.C
    z = smooth_logits(B, Cs, S, 0, device)
    host = label_desc([(H, W)] * B)
    desc = host.to(device)
    res = {"what": "device decode, B=4 1400x2900 uint8 label maps from 620x620 logits (tl tree, model_type 1)"}

    out = {}

    def kernel(conf=False):
        out["labels"], out["conf"] = ops.decode_labels(z, dec.tables, desc, host, conf)

    # the same labels from stock torch ops: resize every level, arg-max per level, descend where level 0 chose the parent
    parent = [c for c, k in enumerate(dec.tables.n_children[0]) if k][0]
    lut = torch.tensor([v if v >= 0 else 0 for v in dec.tables.pixel_val[0]] + dec.tables.pixel_val[1], dtype=torch.uint8,
                       device=device)

    def stock():
        a0 = F.interpolate(z[0], size=(H, W), mode="bilinear", align_corners=False).argmax(1)
        a1 = F.interpolate(z[1], size=(H, W), mode="bilinear", align_corners=False).argmax(1)
        out["stock"] = lut[torch.where(a0 == parent, a1 + Cs[0], a0)]

    ts = timed(kernel, a.batches)
    tc = timed(lambda: kernel(True), a.batches)
    tt = timed(stock, max(a.batches // 3, 5), warmup=2)
    kernel()
    differ = int((out["labels"].reshape(B, H, W) != out["stock"]).sum())
    ms, msc, mst = statistics.median(ts), statistics.median(tc), statistics.median(tt)
    moved = B * S * S * 4 * sum(Cs) + B * H * W               # every level set read once, labels written
    res.update(decode_ms_median=round(ms, 4), decode_ms_min=round(min(ts), 4), batches=a.batches, bytes_per_batch=moved,
               achieved_tb_s=round(moved / (ms * 1e-3) / 1e12, 3),
               fraction_of_hbm_peak=round(moved / (ms * 1e-3) / 1e12 / HBM_PEAK_TBS, 4),
               decode_with_confidence_ms_median=round(msc, 4), bytes_per_batch_with_confidence=moved + 4 * B * H * W,
               stock_torch_ms_median=round(mst, 4), stock_torch_ms_min=round(min(tt), 4), speedup_over_stock=round(mst / ms, 2),
               labels_differing_from_stock=differ, pixels=B * H * W)
    log(json.dumps(res))

    if a.views:
        res.update(bench_views(a, dec, z, desc, host, B, S, H, W, timed, out))
        log(json.dumps(res))

    if not a.skip_predictor:
        from hrseg_amd import predictEval as PE
        from hrseg_amd.Models import models as PM
        from hrseg_amd.utils import synth
        from hrseg_amd.utils.config import hrnet_w48_config
        model = synth.fill_state_dict(PM.HighResolutionNet(hrnet_w48_config(), hierarchy=tree, model_type=1)).to(device)
        args = argparse.Namespace(img_size=S, model_type=1, model_select=1)
        predictor = PE.Predictor(model, tree, cmap, args)
        rng = np.random.default_rng(0)
        imgs = [rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8) for _ in range(B)]
        from hrseg_amd.Data.decode import pack_images
        from hrseg_amd.Data.loader import RaggedBatch
        src, dh = pack_images(imgs)
        batch = RaggedBatch(src.to(device), dh.to(device), None, None, dh, None)
        for _ in range(2):
            predictor(batch)
        torch.cuda.synchronize()
        th, tw = [], []
        for _ in range(8):
            t0 = time.perf_counter()
            predictor(batch)
            th.append(time.perf_counter() - t0)
            torch.cuda.synchronize()
            tw.append(time.perf_counter() - t0)
        res.update(predictor_host_ms_per_call=round(1e3 * statistics.median(th), 3),
                   predictor_wall_ms_per_call=round(1e3 * statistics.median(tw), 3))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
