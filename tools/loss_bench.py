"""The fused loss launches (csrc/loss.hip: hrseg_loss_partials_opt, _finalize_opt, _bwd_opt) at the headline's level shapes --
batch 4, 620 x 620, the tl tree's channel counts -- with the focal exponent off (gamma = 0, the instances without options) and
on (gamma = 2), alternating in one process after a warm-up; events on the launch stream, medians over --rounds rounds of
--launches launches.  The bytes are what the algorithm needs: the forward reads two planes (logits, targets), the backward reads
the same two and writes one (dz); achieved bytes/s = those bytes over the measured time, next to the 8 TB/s HBM peak.  One
level's three planes are 74 MB, less than the 256 MB last-level cache, so the launches rotate over --sets copies of the tensors
(default 8, 590 MB): every launch then finds its planes in HBM, as in a train step, where the whole backbone ran in between.
With --ohem THRESH,MIN_KEPT (default 0.7,100000; "off" = none) the launches of online hard example mining ride in the same
rounds, per gamma: the score pass (two planes in, the score buffer q of B*hw floats out), the selection (seven launches, q read
three times), the masked partials and backward (the plain launches' bytes plus q), and forward + backward as ops issues them
with OHEM on, next to the plain sequence of the same process.
    python tools/loss_bench.py [--batch 4] [--size 620] [--launches 48] [--rounds 7] [--sets 8] [--ohem 0.7,100000]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from hrseg_amd import ops
from hrseg_amd._lib import call, ohem_workspace_bytes, ptr
from hrseg_amd.utils.hierarchy import get_classes

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=4)
ap.add_argument("--size", type=int, default=620)
ap.add_argument("--launches", type=int, default=48)
ap.add_argument("--sets", type=int, default=8)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--gammas", default="0,2")
ap.add_argument("--ohem", default="0.7,100000")
args = ap.parse_args()
OHEM = None if args.ohem == "off" else (float(args.ohem.split(",")[0]), int(args.ohem.split(",")[1]))
dev = torch.device("cuda:0")
HBM_PEAK = 8.0e12
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "restrictive-hierarchical-semantic-segmentation_amd", "data", "class_tree_tl.json")) as f:
    LEVELS = get_classes(json.load(f), full=True)
B, hw = args.batch, args.size * args.size
gammas = [float(v) for v in args.gammas.split(",")]


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3         # us per launch


for L, C in enumerate(LEVELS):
    g = torch.Generator(device=dev).manual_seed(L)
    sets = []
    for _ in range(args.sets):
        z = 2.0 * torch.randn(B, C, args.size, args.size, device=dev, generator=g)
        t = torch.randint(-1, 2, (B, C, args.size, args.size), device=dev, generator=g).float()
        sets.append((z, t, torch.empty_like(z), torch.empty(B * hw, device=dev)))
    turn = [0]

    def planes():
        turn[0] = (turn[0] + 1) % len(sets)
        return sets[turn[0]]

    w = torch.ones(C, device=dev)
    seed = torch.tensor([1.0, 1.0, 0.0], device=dev)
    part = torch.empty(B * C * 5, dtype=torch.float64, device=dev)
    out, coef = torch.empty(3, device=dev), torch.empty(B * C * 4, device=dev)
    plane = B * C * hw * 4

    def partials(gamma):
        z, t, _, _ = planes()
        call("hrseg_loss_partials_opt", ptr(z), ptr(t), ptr(part), B, C, hw, gamma)

    def finalize():
        call("hrseg_loss_finalize_opt", ptr(part), ptr(w), B, C, 0.0, 0.5, 0.5, ptr(out), ptr(coef))

    def bwd(gamma):
        z, t, dz, _ = planes()
        call("hrseg_loss_bwd_opt", ptr(z), ptr(t), ptr(coef), ptr(seed), ptr(dz), 0, B, C, hw, gamma)

    def fwd_bwd(opt):                       # the three launches as ops issues them in a step
        z, t, dz, _ = planes()
        ops.loss_bwd(z, t, ops.loss_fwd(z, t, w, opt)[1], seed, dz=dz, options=opt)

    # online hard example mining: every set has its own score buffer (filled once, below); one record and workspace
    record = torch.zeros(4, dtype=torch.int32, device=dev)
    work = torch.empty(ohem_workspace_bytes() // 4, dtype=torch.int32, device=dev)
    qbytes = B * hw * 4

    def ohem_scores():
        z, t, _, q = planes()
        call("hrseg_ohem_scores", ptr(z), ptr(t), ptr(q), B, C, hw)

    def ohem_select():
        q = planes()[3]
        call("hrseg_ohem_select", ptr(q), B * hw, OHEM[0], OHEM[1], ptr(work), ptr(record))

    def ohem_partials(gamma):
        z, t, _, q = planes()
        call("hrseg_loss_partials_ohem", ptr(z), ptr(t), ptr(q), ptr(record), OHEM[0], ptr(part), B, C, hw, gamma)

    def ohem_bwd(gamma):
        z, t, dz, q = planes()
        call("hrseg_loss_bwd_ohem", ptr(z), ptr(t), ptr(q), ptr(record), OHEM[0], ptr(coef), ptr(seed), ptr(dz), 0, B, C, hw, gamma)

    def ohem_fwd_bwd(opt):                  # scores, selection, masked partials, finalize, masked backward as ops issues them
        z, t, dz, _ = planes()
        _, cf, state = ops.loss_fwd(z, t, w, opt, ohem=OHEM)
        ops.loss_bwd(z, t, cf, seed, dz=dz, options=opt, ohem=state)

    runs = {}
    for gamma in gammas:
        runs[gamma] = {"partials": (lambda gm=gamma: partials(gm), 2 * plane), "finalize": (finalize, 0),
                       "bwd": (lambda gm=gamma: bwd(gm), 3 * plane),
                       "fwd+bwd": (lambda o=(gamma, 0.0, 0.5, 0.5): fwd_bwd(o), 5 * plane)}
        if OHEM is not None:
            runs[gamma].update({"ohem_scores": (ohem_scores, 2 * plane + qbytes), "ohem_select": (ohem_select, 3 * qbytes),
                                "ohem_partials": (lambda gm=gamma: ohem_partials(gm), 2 * plane + qbytes),
                                "ohem_bwd": (lambda gm=gamma: ohem_bwd(gm), 3 * plane + qbytes),
                                "ohem_fwd+bwd": (lambda o=(gamma, 0.0, 0.5, 0.5): ohem_fwd_bwd(o), 7 * plane + 6 * qbytes)})
    partials(0.0)
    finalize()                              # coef holds finite coefficients before the first backward
    if OHEM is not None:                    # every set's scores and the record exist before the masked launches are timed
        for _ in sets:
            ohem_scores()
        ohem_select()
    times = {(gamma, k): [] for gamma in gammas for k in runs[gamma]}
    for gamma in gammas:                      # warm-up: every instance loaded, every buffer touched
        for fn, _ in runs[gamma].values():
            timed(fn, 5)
    for _ in range(args.rounds):              # the gammas alternate inside every round
        for k in runs[gammas[0]]:
            for gamma in gammas:
                times[(gamma, k)].append(timed(runs[gamma][k][0], args.launches))
    for gamma in gammas:
        for k, (_, nbytes) in runs[gamma].items():
            v = times[(gamma, k)]
            med = statistics.median(v)
            line = dict(level=L, C=C, B=B, size=args.size, gamma=gamma, ohem=list(OHEM) if k.startswith("ohem") else None, launch=k, us_median=round(med, 2), us_min=round(min(v), 2),
                        us_max=round(max(v), 2), mbytes=round(nbytes / 1e6, 1))
            if nbytes:
                line["tbytes_per_s"] = round(nbytes / (med * 1e-6) / 1e12, 3)
                line["share_of_hbm_peak"] = round(nbytes / (med * 1e-6) / HBM_PEAK, 3)
            print(json.dumps(line))
