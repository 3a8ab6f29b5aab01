"""hrseg_bilinear_bwd_multi at the shapes of one HRNet train step (B = 8, 620 x 620 input): the head's transpose (720 channels,
155 x 155 onto 78 / 39 / 20) and the three distinct fuse-layer shapes, isolated (events on the launch stream, 20 launches).
Per shape: one hrseg_bilinear_bwd launch per target (the fuse layers' route with hrseg_tune fuse_bwd_multi = 0), the gather
body (bwd_multi_slab = -1), and the streaming body under every (bwd_multi_bands, bwd_multi_slab) pair given:
    python tools/bwd_multi_bench.py [--bands 0,2,4,8] [--slabs 0,48,96]       (0 = the library's plan)"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from hrseg_amd import _lib, ops

ap = argparse.ArgumentParser()
ap.add_argument("--bands", default="0,2,4,8")
ap.add_argument("--slabs", default="0")
ap.add_argument("--launches", type=int, default=20)
ap.add_argument("--shapes", default="", help="only the shapes whose name contains this")
args = ap.parse_args()
dev = torch.device("cuda:0")
B = 8
SHAPES = [("head 720ch 155->78/39/20", 720, 155, [78, 39, 20]),
          ("fuse  48ch 155->78/39/20", 48, 155, [78, 39, 20]),
          ("fuse  48ch 155->78/39", 48, 155, [78, 39]),
          ("fuse  48ch 155->78", 48, 155, [78]),
          ("fuse  96ch 78->39/20", 96, 78, [39, 20]),
          ("fuse  96ch 78->39", 96, 78, [39]),
          ("fuse 192ch 39->20", 192, 39, [20])]


def timeit(fn, n):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


for name, C, H, ts in SHAPES:
    if args.shapes not in name:
        continue
    dy = torch.randn(B, H, H, C, device=dev)
    sizes = [(t, t) for t in ts]
    mb = (dy.numel() + sum(B * t * t * C for t in ts)) * 4 / 1e6
    single = timeit(lambda: [ops.bilinear_bwd(dy, (B, t, t, C), H, H) for t in ts], args.launches)
    _lib.tune(bwd_multi_slab=-1)
    gather = timeit(lambda: ops.bilinear_bwd_multi(dy, sizes), args.launches)
    print(f"{name}: {mb:.0f} MB once; per-target launches {single:.1f} us, gather body {gather:.1f} us")
    for slab in [int(v) for v in args.slabs.split(",")]:
        row = []
        for bands in [int(v) for v in args.bands.split(",")]:
            _lib.tune(bwd_multi_slab=slab, bwd_multi_bands=bands)
            row.append(f"{bands}: {timeit(lambda: ops.bilinear_bwd_multi(dy, sizes), args.launches):.1f}")
        print(f"    streaming, slab {slab:3d} ch, bands -> us   " + "   ".join(row))
    _lib.tune(bwd_multi_slab=0, bwd_multi_bands=0)
    del dy
