#!/usr/bin/env python
"""Border weights on the MI355X: device time of

    border   hrseg_border_weights (label extraction + search, two launches) per level of the tl tree at [B,4,S,S], radius 15
             and 32, on augmented synthetic targets, with the share of search tiles that took the early-out (one non-void
             label in the tile and its halo; recomputed on the host from the label map the call wrote);
    loss     hrseg_loss_partials_pw / hrseg_loss_bwd_pw against hrseg_loss_partials_opt / hrseg_loss_bwd_opt at the same shape
             in the same run, with the byte ratios (2C+1)/2C and (3C+1)/3C beside the measured ones and the min-max spread of
             the unweighted calls over the rounds;
    step     (--step) the taped train step of the hierarchical HRNet-W48 with CrossEntropyLoss(border=BorderWeights(10, 5))
             on both levels against the same step without, same process, alternating.

    python tools/border_bench.py [--S 620 --B 4 --rounds 7 --calls 20] [--step --steps 12]

The targets are those of train.SyntheticDataset, augmented on the device the way the input pipeline moves borders: a seeded
affine warp per sample (rotation, scale, shift; nearest neighbour) and a horizontal flip for every other sample, with what the
warp brings in from outside the frame unlabelled (-1 in every channel).  Device events around `calls` back-to-back calls of one
variant behind a blocker (a large memset that lets the host run ahead); the variants alternate round by round after a warm-up
of each; median, min and max over the rounds of the per-call time.  Prints one JSON line."""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def log(msg):
    print("[border_bench] " + msg, file=sys.stderr, flush=True)


def augmented_targets(tree, B, S, seed, device):
    """train.SyntheticDataset targets [B,Ctot,S,S], warped per sample; outside the source frame: -1 in every channel"""
    import torch.nn.functional as F
    from hrseg_amd import train as T
    ds = T.SyntheticDataset(tree, B, S, hierarchical=True, seed=seed)
    y = ds.y.to(device)
    g = torch.Generator().manual_seed(seed)
    theta = torch.zeros(B, 2, 3)
    for b in range(B):
        ang = math.radians(float(torch.empty(1).uniform_(-20.0, 20.0, generator=g)))
        sc = float(torch.empty(1).uniform_(0.8, 1.2, generator=g))
        tx, ty = (float(v) for v in torch.empty(2).uniform_(-0.15, 0.15, generator=g))
        flip = -1.0 if b % 2 else 1.0
        theta[b] = torch.tensor([[flip * sc * math.cos(ang), -sc * math.sin(ang), tx], [flip * sc * math.sin(ang), sc * math.cos(ang), ty]])
    grid = F.affine_grid(theta.to(device), list(y.shape), align_corners=False)
    inside = ((grid.abs() <= 1.0).all(dim=-1))[:, None]
    warped = F.grid_sample(y, grid, mode="nearest", padding_mode="zeros", align_corners=False)
    return torch.where(inside, warped, torch.full_like(warped, -1.0)).contiguous()


def early_out_share(labels, radius, tile):
    """share of the search kernel's tiles whose window (tile + radius rows + the halo columns) holds at most one non-void
    label: csrc/border_weight.hip, BW_HALO_X"""
    lab = labels.cpu().numpy()
    TW, TH = tile
    hx = (radius + 9) & ~3
    B, H, W = lab.shape
    n = out = 0
    for b in range(B):
        for y0 in range(0, H, TH):
            for x0 in range(0, W, TW):
                win = lab[b, max(0, y0 - radius):y0 + TH + radius, max(0, x0 - hx):x0 + TW + hx]
                n += 1
                out += len(np.setdiff1d(np.unique(win), [255])) <= 1
    return out / n, n


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


def summary(ts):
    return dict(us_median=round(statistics.median(ts), 2), us_min=round(min(ts), 2), us_max=round(max(ts), 2))


def bench_border(a, tree, nc, device, blocker, res):
    from hrseg_amd import _lib, ops
    from hrseg_amd.Metrics.border import border_table
    y = augmented_targets(tree, a.B, a.S, 7, device)
    levels, s = [], 0
    for n in nc:
        levels.append(y[:, s:s + n].contiguous())
        s += n
    tile = _lib.border_tile()
    variants, meta = {}, {}
    for radius in (15, 32):
        lut = torch.from_numpy(border_table(10.0, radius / 3.0, radius)).to(device)
        for L, t in enumerate(levels):
            labels, v = ops.border_weights(t, radius, lut)
            share, ntiles = early_out_share(labels, radius, tile)
            key = f"level{L}_r{radius}"
            meta[key] = dict(C=t.shape[1], radius=radius, tiles=ntiles, early_out_share=round(share, 3),
                             void_share=round(float((labels == 255).float().mean()), 3),
                             weighted_share=round(float((v > 1.0).float().mean()), 3))
            variants[key] = (lambda i, t=t, radius=radius, lut=lut: ops.border_weights(t, radius, lut))
    times = rounds_of(variants, a.rounds, a.calls, blocker)
    for key, ts in times.items():
        meta[key].update(summary(ts))
        log(json.dumps({key: meta[key]}))
    res["border"] = meta
    return levels


def bench_loss(a, levels, device, blocker, res):
    from hrseg_amd import ops
    t = levels[0]
    B, Cn, H, W = t.shape
    z = torch.randn(t.shape, generator=torch.Generator().manual_seed(3)).to(device)
    w = torch.ones(Cn, device=device)
    pw = (1.0 + 10.0 * torch.rand(B, H, W, generator=torch.Generator().manual_seed(4))).to(device)
    up = torch.tensor([1.0, 1.0, 0.0], device=device)
    opt = (0.0, 0.0, 0.5, 0.5)
    _, coef = ops.loss_fwd(z, t, w, opt)
    _, coef_pw = ops.loss_fwd(z, t, w, opt, pixel_weight=pw)
    dz = torch.empty_like(z)
    part = torch.empty(B * Cn * 5, dtype=torch.float64, device=device)
    p, hw = _ptr, H * W
    from hrseg_amd._lib import call
    variants = {
        "partials_opt": lambda i: call("hrseg_loss_partials_opt", p(z), p(t), p(part), B, Cn, hw, 0.0),
        "partials_pw": lambda i: call("hrseg_loss_partials_pw", p(z), p(t), p(pw), p(part), B, Cn, hw, 0.0),
        "bwd_opt": lambda i: call("hrseg_loss_bwd_opt", p(z), p(t), p(coef), p(up), p(dz), 0, B, Cn, hw, 0.0),
        "bwd_pw": lambda i: call("hrseg_loss_bwd_pw", p(z), p(t), p(pw), p(coef_pw), p(up), p(dz), 0, B, Cn, hw, 0.0),
    }
    times = rounds_of(variants, a.rounds, a.calls, blocker)
    out = {k: summary(ts) for k, ts in times.items()}
    for kind, byte_ratio in (("partials", (2 * Cn + 1) / (2 * Cn)), ("bwd", (3 * Cn + 1) / (3 * Cn))):
        base, mine = out[kind + "_opt"], out[kind + "_pw"]
        out[kind + "_ratio"] = dict(measured=round(mine["us_median"] / base["us_median"], 3), bytes=round(byte_ratio, 3),
                                    unweighted_spread=round(base["us_max"] / base["us_min"], 3))
    res["loss"] = dict(shape=list(t.shape), **out)
    log(json.dumps(res["loss"]))


def _ptr(t):
    return t.data_ptr()


def bench_step(a, tree, nc, device, res):
    """taped train step, border on both levels against off: two recordings of the same model configuration, alternating"""
    from hrseg_amd import _lib, train as T
    from hrseg_amd.Metrics import losses
    from hrseg_amd.Models import models
    from hrseg_amd.utils import synth
    from hrseg_amd.utils.config import hrnet_w48_config
    x_np, t_np = synth.synthetic_batch(tree, a.B, a.S, seed=100, hierarchical=True)
    x, t = torch.from_numpy(x_np).to(device), torch.from_numpy(t_np).to(device)
    ns = argparse.Namespace(model_type=1, model_select=1, num_classes=nc, level_weights=synth.README_LEVEL_WEIGHTS_TL,
                            level0_pretrain_epochs=None, batch_size=a.B)
    steps = {}
    for name, border in (("off", None), ("on", (10.0, 5.0))):
        torch.manual_seed(0)
        model = models.HighResolutionNet(hrnet_w48_config(), hierarchy=tree, model_type=1).to(device)
        model.train()
        opt = T.FusedAdamW(model, lr=[1e-4])
        fns = [[losses.CrossEntropyLoss(border=None if border is None else losses.BorderWeights(*border)),
                losses.SoftDiceLoss(num_classes=n)] for n in nc]
        steps[name] = T.TapedTrainStep(model, opt, fns, ns, tree, x, t)
        for _ in range(3):
            steps[name](x, t)
    torch.cuda.synchronize()
    times = {name: [] for name in steps}
    counts = {}
    for _ in range(a.rounds):
        for name, step in steps.items():
            _lib.launch_count("border_weights", reset=True)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                step(x, t)
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) / a.steps)
            counts[name] = _lib.launch_count("border_weights", reset=True) / a.steps
    out = {name: dict(ms_median=round(statistics.median(ts), 3), ms_min=round(min(ts), 3), ms_max=round(max(ts), 3),
                      border_launches_per_step=counts[name]) for name, ts in times.items()}
    out["delta_ms"] = round(out["on"]["ms_median"] - out["off"]["ms_median"], 3)
    res["step"] = out
    log(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--S", type=int, default=620)
    ap.add_argument("--B", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--step", action="store_true", help="also time the taped HRNet-W48 train step with the option on and off")
    ap.add_argument("--steps", type=int, default=12)
    a = ap.parse_args()
    from hrseg_amd.utils.hierarchy import get_classes
    with open(os.path.join(ROOT, "restrictive-hierarchical-semantic-segmentation_amd", "data", "class_tree_tl.json")) as f:
        tree = json.load(f)
    nc = get_classes(tree, full=True)
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    blocker = torch.empty(1 << 30, dtype=torch.uint8, device=device)
    res = {"what": f"border weights, B={a.B}, {a.S}x{a.S}, tl tree (levels of {nc} channels)", "rounds": a.rounds, "calls": a.calls}
    levels = bench_border(a, tree, nc, device, blocker, res)
    bench_loss(a, levels, device, blocker, res)
    if a.step:
        del blocker
        bench_step(a, tree, nc, device, res)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
