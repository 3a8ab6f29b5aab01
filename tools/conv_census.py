"""Which convolution calls does one train step make, and what does each cost?  Records every grouped ops.conv_* call
of one step of the bench model (shapes only), then times each distinct call in isolation (same arithmetic mode, plain fp32
inputs: a call that read a pre-split input in the step is timed on the fp32 form).
    python tools/conv_census.py [--size 620] [--batch 4]"""
import argparse
import collections
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bench
from hrseg_amd import _lib, ops
from hrseg_amd import train as T
from hrseg_amd.utils import synth

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=620)
ap.add_argument("--batch", type=int, default=4)
a = ap.parse_args()
args = argparse.Namespace(model="hrnet", size=a.size, batch=a.batch, flat=False, tree="class_tree_tl.json")
dev = torch.device("cuda:0")
tree, model, ns, loss_fns, opt = bench.build(args, dev)
x, t = synth.synthetic_batch(tree, a.batch, a.size, seed=1, hierarchical=True)
x, t = torch.from_numpy(x).to(dev), torch.from_numpy(t).to(dev)
model.train()
T.train_step(model, opt, x, t, loss_fns, ns, tree, [])          # warm-up (allocations)
torch.cuda.synchronize()

calls = collections.Counter()
# every convolution of the engine goes through the three grouped wrappers (the single-problem forms of ops.py are groups of
# one); the wrappers below note the shapes and hand everything else through untouched
orig = {n: getattr(ops, n) for n in ("conv_fwd_group", "conv_dgrad_group", "conv_wgrad_group")}


def w_fwd_g(xs, ws, biases, k, s, couts, prec=0, **kw):
    calls[("fwd", tuple(tuple(x.shape) for x in xs), tuple(couts), k, s, prec)] += 1
    return orig["conv_fwd_group"](xs, ws, biases, k, s, couts, prec=prec, **kw)


def w_dgrad_g(dys, wts, x_shapes, k, s, outs, accumulate, prec=0, **kw):
    calls[("dgrad", tuple(tuple(xs) for xs in x_shapes), tuple(d.shape[3] for d in dys), k, s, prec)] += 1
    return orig["conv_dgrad_group"](dys, wts, x_shapes, k, s, outs, accumulate, prec=prec, **kw)


def w_wgrad_g(xs, dys, dws, k, s, prec=0, **kw):
    calls[("wgrad", tuple(tuple(x.shape) for x in xs), tuple(d.shape[3] for d in dys), k, s, prec)] += 1
    return orig["conv_wgrad_group"](xs, dys, dws, k, s, prec=prec, **kw)


ops.conv_fwd_group, ops.conv_dgrad_group, ops.conv_wgrad_group = w_fwd_g, w_dgrad_g, w_wgrad_g
T.train_step(model, opt, x, t, loss_fns, ns, tree, [])
torch.cuda.synchronize()
for n, f in orig.items():
    setattr(ops, n, f)


def timeit(fn, n=10):
    for _ in range(2):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


rows = []
for (kind, xshapes, couts, k, s, prec), cnt in calls.items():
    xs = [torch.randn(sh, device=dev) for sh in xshapes]
    ws = [torch.randn(co, k * k, sh[3], device=dev) * 0.05 for co, sh in zip(couts, xshapes)]
    ys = [ops.conv_fwd(x_, w_, None, k, s) for x_, w_ in zip(xs, ws)]
    fl = sum(2.0 * y.numel() * sh[3] * k * k for y, sh in zip(ys, xshapes))
    n = len(xs)
    dys = [torch.randn_like(y) for y in ys]
    gms = [d.abs().max().reshape(1).repeat(64) for d in dys]
    if kind == "fwd":
        fn = lambda: ops.conv_fwd_group(xs, ws, [None] * n, k, s, list(couts), prec=prec)
    elif kind == "dgrad":
        wts = [ops.weight_transpose(w_, co, k * k, sh[3]) for w_, co, sh in zip(ws, couts, xshapes)]
        fn = lambda: ops.conv_dgrad_group(dys, wts, list(xshapes), k, s, [None] * n, [False] * n, prec=prec, gmaxs=gms)
    else:
        dws = [torch.zeros_like(w_) for w_ in ws]
        fn = lambda: ops.conv_wgrad_group(xs, dys, dws, k, s, prec=prec, gmaxs=gms)
    try:
        t_us = timeit(fn)
    except Exception:               # a shape the library refuses in isolation
        t_us = float("nan")
    rows.append((cnt * t_us, kind, cnt, t_us, fl, xshapes, couts, k, s))
    del xs, ws, ys, dys
rows.sort(reverse=True)
tot = sum(r[0] for r in rows if r[0] == r[0])
print("total %.2f ms of conv calls per step" % (tot / 1e3))
for tt, kind, cnt, t_us, fl, xshapes, couts, k, s in rows[:45]:
    desc = " + ".join("%dx%dx%d->%d" % (sh[1], sh[2], sh[3], co) for sh, co in zip(xshapes, couts))
    print("%6.2f ms  %-5s x%3d  %8.1f us  %6.1f TF  k%d s%d B%d  %s" % (tt / 1e3, kind, cnt, t_us, fl / t_us / 1e6, k, s, xshapes[0][0], desc))
