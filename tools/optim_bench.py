"""Times the optimizer's launches in isolation over flat buffers of the two models' sizes (hier HRNet-W48: 65,858,648
parameters, UNet: 13,396,424): plain adamw_dev next to the clipping path's three launches (grad_sumsq, grad_clip_finalize,
adamw_dev_clip), each alone and as the sequence a step issues; and the weight average: adamw_dev_ema (the update that also
advances the shadow), the unfused sequence adamw_dev + ema_update it replaces, ema_update alone and swap.  Device events around REPS back-to-back calls after a
warm-up, median of ROUNDS such windows; the gradient alternates between two buffers so that a 53 MB UNet gradient is not
simply re-read from the last-level cache.  Bytes are what the algorithm needs: 4n read for the reduction, 16n read + 12n
written for AdamW, 20n + 16n with the shadow fused in, 28n + 12n unfused, 8n + 8n for the swap.  adamw_dev is timed a second
time at the end: the difference between its two medians is the run-to-run spread the other figures are read against.  One
JSON line per size at the end."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import hrseg_amd  # noqa: F401
from hrseg_amd import _lib, ops

SIZES = {"hrnet_hier_w48": 65_858_648, "unet": 13_396_424}
REPS, ROUNDS = 20, 9


def timeit(f):
    """median over ROUNDS windows of REPS calls -> microseconds per call"""
    for _ in range(3):
        f()
    torch.cuda.synchronize()
    out = []
    for _ in range(ROUNDS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(REPS):
            f()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / REPS * 1000.0)
    return statistics.median(out), min(out), max(out)


def main():
    _lib.require_gpu()
    dev = "cuda"
    for name, n in SIZES.items():
        gen = torch.Generator(device=dev).manual_seed(1)
        p = torch.randn(n, device=dev, generator=gen)
        gs = [1e-3 * torch.randn(n, device=dev, generator=gen) for _ in range(2)]
        m, v = torch.zeros_like(p), torch.zeros_like(p)
        hyper = torch.tensor([1e-4, 0.9, 0.999, 1e-8, 0.01, 1.0], device=dev)
        cfg = torch.tensor([1.0, 1.0], device=dev)
        state, clip = torch.zeros(3, device=dev), torch.zeros(4, device=dev)
        partial = torch.empty(_lib.grad_sumsq_chunks(n), dtype=torch.float64, device=dev)
        e = p.clone() + 0.5
        emacfg = torch.tensor([0.999, 1.0, 0.0], device=dev)
        ops.grad_sumsq(gs[0], partial)
        ops.grad_clip_finalize(partial, hyper, cfg, state, clip)          # a valid verdict for the update kernel alone
        k = [0]

        def g():
            k[0] ^= 1
            return gs[k[0]]

        def three():
            gg = g()
            ops.grad_sumsq(gg, partial)
            ops.grad_clip_finalize(partial, hyper, cfg, state, clip)
            ops.adamw_dev_clip(p, gg, m, v, hyper, state, cfg, clip)

        def unfused():
            ops.adamw_dev(p, g(), m, v, hyper, state)
            ops.ema_update(e, p, state, emacfg)

        res = {
            "adamw_dev": timeit(lambda: ops.adamw_dev(p, g(), m, v, hyper, state)),
            "grad_sumsq": timeit(lambda: ops.grad_sumsq(g(), partial)),
            "grad_clip_finalize": timeit(lambda: ops.grad_clip_finalize(partial, hyper, cfg, state, clip)),
            "adamw_dev_clip": timeit(lambda: ops.adamw_dev_clip(p, g(), m, v, hyper, state, cfg, clip)),
            "three_launches": timeit(three),
            "adamw_dev_ema": timeit(lambda: ops.adamw_dev_ema(p, g(), m, v, e, hyper, state, emacfg)),
            "adamw_dev+ema_update": timeit(unfused),
            "ema_update": timeit(lambda: ops.ema_update(e, p, state, emacfg)),
            "swap": timeit(lambda: ops.swap(p, e)),
            "adamw_dev_again": timeit(lambda: ops.adamw_dev(p, g(), m, v, hyper, state)),
        }
        assert clip[2].item() == 1.0 and torch.isfinite(p).all() and torch.isfinite(e).all()
        print(f"{name}: n = {n:,} ({partial.numel()} chunks of {_lib.grad_sumsq_chunk_len()})")
        for key, (med, lo, hi) in res.items():
            print(f"  {key:20s} {med:9.1f} us   (min {lo:.1f}, max {hi:.1f})")
        bw = 4.0 * n / (res["grad_sumsq"][0] * 1e-6)
        bw_adam = 28.0 * n / (res["adamw_dev"][0] * 1e-6)
        added = res["three_launches"][0] - res["adamw_dev"][0]
        print(f"  reduction: {bw / 1e12:.2f} TB/s achieved (4n bytes read); adamw_dev: {bw_adam / 1e12:.2f} TB/s (28n bytes); "
              f"clipping path adds {added:.1f} us per step")
        base, fused, unf = res["adamw_dev"][0], res["adamw_dev_ema"][0], res["adamw_dev+ema_update"][0]
        spread = abs(res["adamw_dev_again"][0] - base)
        print(f"  weight average: fused {fused:.1f} us = {fused / base:.3f} x adamw_dev (bytes: 36/28 = {36 / 28:.3f}), "
              f"{36.0 * n / (fused * 1e-6) / 1e12:.2f} TB/s; unfused {unf:.1f} us = {unf / base:.3f} x (bytes: 40/28 = "
              f"{40 / 28:.3f}); adamw_dev measured twice: {spread:.1f} us apart; swap {16.0 * n / (res['swap'][0] * 1e-6) / 1e12:.2f} TB/s")
        print(json.dumps({"model": name, "n": n, "us": {k_: round(v_[0], 2) for k_, v_ in res.items()},
                          "grad_sumsq_bytes_per_s": bw, "adamw_dev_bytes_per_s": bw_adam, "added_us_per_step": round(added, 2), "ema_fused_over_adamw_dev": round(fused / base, 4),
                          "ema_unfused_over_adamw_dev": round(unf / base, 4), "adamw_dev_spread_us": round(spread, 2)}))
        del p, gs, m, v, e


if __name__ == "__main__":
    main()
