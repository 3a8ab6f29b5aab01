#!/usr/bin/env python
"""Device input pipeline on the MI355X: (1) the augmentation kernels of one B=4 620x620 train batch from 1400x2900 RGB
sources (events around each batch, warm-up, median of --batches; bytes moved over that time against the HBM peak),
(2) the flagship train step (bench.py's model, launch tape) fed by DeviceAugmentLoader from pre-decoded in-memory
sources vs the same step on device-resident synthetic input, measured in the same process in alternating blocks.

    python tools/augment_bench.py [--batches 60] [--steps 30] [--rounds 3] [--workers 4] [--skip-train]

Kernel durations without host gaps: run the same command under `rocprofv3 --kernel-trace --stats -- python ...`
(in a run of its own).  Prints one JSON line."""
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

HBM_PEAK_TBS = 8.0          # MI355X_MICROARCH.md: HBM3E peak


def log(msg):
    print("[augment_bench] " + msg, file=sys.stderr, flush=True)


class Pool(torch.utils.data.Dataset):
    """`n` samples cycling over a few pre-decoded sources: one loader pass covers the whole measurement, so the loader
    blocks time the prefetch overlap of a long epoch, not worker start-up"""

    def __init__(self, samples, n):
        self.samples, self.n = samples, n

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        return self.samples[i % len(self.samples)]


def sources(n, H, W, class_map, seed=0):
    rng = np.random.default_rng(seed)
    vals = np.array(sorted({int(float(r["pixel_val"])) for r in class_map if r["pixel_val"] not in ("None", "")}),
                    dtype=np.uint8)
    out = []
    for _ in range(n):
        img = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
        coarse = rng.choice(vals, size=(H // 50 + 1, W // 50 + 1))
        lab = np.ascontiguousarray(np.repeat(np.repeat(coarse, 50, 0), 50, 1)[:H, :W])
        out.append((img, lab))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=60)
    ap.add_argument("--steps", type=int, default=30, help="train steps per block and mode")
    ap.add_argument("--rounds", type=int, default=3, help="alternating blocks per mode")
    ap.add_argument("--workers", type=int, default=4)
    ap.add_argument("--skip-train", action="store_true")
    a = ap.parse_args()
    from hrseg_amd import ops
    from hrseg_amd.Data import DeviceAugment, DeviceAugmentLoader, ragged_collate
    from hrseg_amd.Data.augment import pack_params
    data_dir = os.path.join(ROOT, "restrictive-hierarchical-semantic-segmentation_amd", "data")
    tree = json.load(open(os.path.join(data_dir, "class_tree_tl.json")))
    cmap = list(csv.DictReader(open(os.path.join(data_dir, "class_map.csv"))))
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    B, S, H, W = 4, 620, 1400, 2900
    aug = DeviceAugment(S, tree, cmap, 1, train=True, seed=0)
    samples = sources(8, H, W, cmap)
    batch = ragged_collate(samples[:B]).to(device)
    table = pack_params(aug.sample(B), S).to(device)
    res = {"what": "device augmentation, B=4 620x620 from 1400x2900x3 uint8 (tl tree, model_type 1)"}

    def kernels():
        x = ops.augment_image(batch.src, batch.desc, batch.desc_host, table, S, True)
        y = ops.augment_targets(batch.label, batch.ldesc, batch.ldesc_host, aug.encoder.on_lut, aug.encoder.parent, table,
                                S, True, True)
        return x, y

    for _ in range(5):
        kernels()
    torch.cuda.synchronize()
    ts = []
    for _ in range(a.batches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        kernels()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    ms = statistics.median(ts)
    C = len(aug.names)
    src_bytes = B * H * W * 3 + B * H * W
    plane = S * S
    moved = src_bytes + B * plane * (3 * 4 * 2 + 3 * 4 + 8 * 2 + C * 4)   # sources, state w+r, x, node bits w+r, y
    res.update(augment_ms_median=round(ms, 4), augment_ms_min=round(min(ts), 4), batches=a.batches,
               bytes_per_batch=moved, achieved_tb_s=round(moved / (ms * 1e-3) / 1e12, 3),
               fraction_of_hbm_peak=round(moved / (ms * 1e-3) / 1e12 / HBM_PEAK_TBS, 4))
    th = []
    for _ in range(20):
        t0 = time.perf_counter()
        aug(batch)
        th.append(time.perf_counter() - t0)
    torch.cuda.synchronize()
    res["host_ms_per_call"] = round(1e3 * statistics.median(th), 3)     # sampling + parameter table + launches
    log(json.dumps(res))

    if not a.skip_train:
        import bench
        from hrseg_amd import train as T
        from hrseg_amd.utils import synth
        bargs = argparse.Namespace(tree="class_tree_tl.json", flat=False, model="hrnet", size=S, batch=B)
        tree_b, model, ns, loss_fns, opt = bench.build(bargs, device)
        x_np, t_np = synth.synthetic_batch(tree_b, B, S, seed=100, hierarchical=True)
        x, t = torch.from_numpy(x_np).to(device), torch.from_numpy(t_np).to(device)
        model.train()
        log("model built; recording the launch tape")
        taped = T.TapedTrainStep(model, opt, loss_fns, ns, tree_b, x, t)
        log("tape recorded")
        n_batches = 3 + a.rounds * a.steps + 1
        loader = DeviceAugmentLoader(Pool(samples, n_batches * B), batch_size=B, shuffle=True, num_workers=a.workers,
                                     augment=aug, drop_last=True)
        batches = iter(loader)

        def resident(n):
            for _ in range(n):
                taped(x, t)[0].tolist()

        def fed(n):
            for _ in range(n):
                xb, yb = next(batches)
                taped(xb, yb)[0].tolist()

        resident(3)
        log("resident warm-up done")
        fed(3)
        log("loader warm-up done")
        blocks = {"resident": [], "loader": []}
        for _ in range(a.rounds):
            for name, fn in (("resident", resident), ("loader", fed)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn(a.steps)
                torch.cuda.synchronize()
                blocks[name].append(1e3 * (time.perf_counter() - t0) / a.steps)
                log("%s block: %.3f ms/step" % (name, blocks[name][-1]))
        batches.close()
        r, f = statistics.median(blocks["resident"]), statistics.median(blocks["loader"])
        res.update(step_ms_resident=round(r, 3), step_ms_loader=round(f, 3), loader_overhead=round(f / r - 1, 4),
                   step_blocks_ms={k: [round(v, 3) for v in vs] for k, vs in blocks.items()}, loader_workers=a.workers)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
