#!/usr/bin/env python
"""Tree distillation on the MI355X: device time of

    kernels  hrseg_tree_kl / hrseg_tree_kl_bwd per level of the tl tree at [B,C,S,S] -- restrictive (parents read) with the gate
             off and on, accumulating and not -- beside the time the bytes each call must move (z, u, the parents it reads, dz
             written or read-modify-written) take at the 6.3 TB/s a streaming copy reaches on this chip, and beside
             hrseg_group_kl / hrseg_group_kl_bwd at the same shape in the same run (they read one tensor less);
    step     (--step) the eager train step of the hierarchical HRNet-W48 with and without the distillation loss, alternating, on
             a teacher computed once outside the timed region, and the ema_teacher forward on its own.

    python tools/distill_bench.py [--S 620 --B 4 --rounds 7 --calls 20] [--step --steps 8]

Random logits; the parents are a softmax over the level above.  Device events around `calls` back-to-back calls of one variant
behind a blocker (a large memset that lets the host run ahead); the variants alternate round by round after a warm-up of each;
median, min and max over the rounds of the per-call time.  Prints one JSON line."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

STREAM_TBS = 6.3        # what a float4 copy reaches on the MI355X (8.0 TB/s is the specification)


def log(msg):
    print("[distill_bench] " + msg, file=sys.stderr, flush=True)


def rounds_of(variants, rounds, calls, blocker):
    """{name: [per-call microseconds, one per round]}; the variants alternate round by round"""
    for fn in variants.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            blocker.zero_()
            blocker.zero_()
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / calls)
    return times


def summary(ts):
    return dict(us_median=round(statistics.median(ts), 2), us_min=round(min(ts), 2), us_max=round(max(ts), 2))


def bench_kernels(a, model, device, blocker, res):
    from hrseg_amd import ops
    from hrseg_amd.Metrics import losses as PL
    d = PL.TreeDistillation.for_model(model)
    gen = torch.Generator(device="cpu").manual_seed(11)
    prev = None
    for L, names in enumerate(model.levels):
        C = len(names)
        gp, gs = ([0], [C]) if d.groups[L] is None else d.groups[L]
        if not gs:
            continue
        u = (2.0 * torch.randn(a.B, C, a.S, a.S, generator=gen)).to(device)
        z = (u.cpu() + torch.randn(a.B, C, a.S, a.S, generator=gen)).to(device)
        wprev = prev if L > 0 else None
        prev = torch.softmax(u, dim=1).contiguous()
        g = torch.ones(1, device=device)
        out = torch.zeros(len(gs), 3, dtype=torch.float64, device=device)
        dz = torch.zeros_like(z)
        npix = a.B * a.S * a.S
        reads = 4 * npix * (2 * C + (len(set(gp)) if wprev is not None else 0))
        variants = {
            "fwd": lambda: ops.tree_kl_fwd(z, u, wprev, None, 1.0, 0.0, gp, gs, out=out),
            "fwd_gated": lambda: ops.tree_kl_fwd(z, u, wprev, None, 0.5, 0.6, gp, gs, out=out),
            "bwd": lambda: ops.tree_kl_bwd(z, u, wprev, None, 1.0, 0.0, g, 1.0, gp, gs, dz=dz),
            "bwd_gated": lambda: ops.tree_kl_bwd(z, u, wprev, None, 0.5, 0.6, g, 1.0, gp, gs, dz=dz),
            "bwd_acc": lambda: ops.tree_kl_bwd(z, u, wprev, None, 1.0, 0.0, g, 1e-3, gp, gs, dz=dz, accumulate=True),
        }
        bytes_of = {"fwd": reads, "fwd_gated": reads, "bwd": reads + 4 * npix * C, "bwd_gated": reads + 4 * npix * C,
                    "bwd_acc": reads + 8 * npix * C}
        if L > 0:
            variants["group_kl"] = lambda: ops.group_kl_sums(z, wprev, gp, gs)
            variants["group_kl_bwd"] = lambda: ops.group_kl_bwd(z, wprev, g, 1.0, gp, gs)
            bytes_of["group_kl"] = 4 * npix * (C + len(set(gp)))
            bytes_of["group_kl_bwd"] = 4 * npix * (2 * C + len(set(gp)))
        times = rounds_of(variants, a.rounds, a.calls, blocker)
        level = {}
        for name, ts in times.items():
            s = summary(ts)
            s["bytes"] = bytes_of[name]
            s["us_at_stream_rate"] = round(bytes_of[name] / (STREAM_TBS * 1e12) * 1e6, 2)
            s["times_stream"] = round(s["us_median"] / s["us_at_stream_rate"], 2)
            level[name] = s
        res[f"level{L}"] = dict(C=C, groups=gs, parents=gp if wprev is not None else None, **level)
        log(f"level {L}: " + json.dumps(level))


def bench_step(a, device, res):
    import bench as B
    from hrseg_amd import train as T
    from hrseg_amd.Metrics import losses as PL
    from hrseg_amd.utils import synth
    ns0 = argparse.Namespace(model="hrnet", size=a.S, flat=False, tree="class_tree_tl.json", batch=a.B)
    tree, model, ns, loss_fns, _ = B.build(ns0, device)
    opt = T.FusedAdamW(model, lr=[1e-4], ema_decay=0.999)
    model.train()
    x, t = synth.synthetic_batch(tree, a.B, a.S, seed=0, hierarchical=True)
    x, t = torch.from_numpy(x).to(device), torch.from_numpy(t).to(device)
    d = PL.TreeDistillation.for_model(model, temperature=2.0, thresh=0.5)
    for _ in range(2):
        T.train_step(model, opt, x, t, loss_fns, ns, tree, [])
    teacher = T.ema_teacher(model, opt, x, ns, tree)
    variants = {"plain": lambda: T.train_step(model, opt, x, t, loss_fns, ns, tree, []),
                "distilled": lambda: T.train_step(model, opt, x, t, loss_fns, ns, tree, [], distill=d, teacher=teacher),
                "ema_teacher": lambda: T.ema_teacher(model, opt, x, ns, tree)}
    for fn in variants.values():
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(a.steps):
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1))
    res["step_ms"] = {k: dict(median=round(statistics.median(v), 2), min=round(min(v), 2), max=round(max(v), 2)) for k, v in times.items()}
    res["kept_fraction"] = d.kept_fraction()
    log("step: " + json.dumps(res["step_ms"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--S", type=int, default=620)
    ap.add_argument("--B", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--steps", type=int, default=8)
    a = ap.parse_args()
    from hrseg_amd import _lib
    _lib.require_gpu()
    device = torch.device("cuda")
    from hrseg_amd.Models import models
    tree = json.load(open(os.path.join(ROOT, "restrictive-hierarchical-semantic-segmentation_amd", "data", "class_tree_tl.json")))
    res = dict(S=a.S, B=a.B, rounds=a.rounds, calls=a.calls, stream_TBs=STREAM_TBS)
    blocker = torch.empty(256 << 20, dtype=torch.uint8, device=device)
    shell = models.UNet(size=32, n_channels=3, hierarchy=tree, model_type=1)       # (for its levels and groups only)
    bench_kernels(a, shell, device, blocker, res)
    if a.step:
        bench_step(a, device, res)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
