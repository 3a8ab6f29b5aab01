#!/usr/bin/env python
"""Device consensus on the MI355X: device time of

    consensus   hrseg_consensus_labels (one launch: the voted map and every counter block) at M = 2, 3, 5 and 8 members, with
                and without the support output;
    yardstick   what the pairwise figures alone cost without it: hrseg_score_labels run M (M - 1) / 2 times on the same maps
                (member i as prediction, member j as ground truth), in the same run;

on a batch of four panoramic-size maps (1400 x 2900, the sizes of the scoring section), once on SMOOTH maps (64-pixel blocks
of leaf values, the members shifted against each other by a few pixels: long runs of one member tuple, disagreement along
the block borders) and once on SALT-NOISE maps (every pixel of every member drawn on its own: no run folds, no two lanes of
a wave share a key).  Beside each time: the bytes-moved lower bound (M + 1 [+ 1 with support]) * pixels / HBM rate.

    python tools/consensus_bench.py [--H 1400 --W 2900 --B 4 --rounds 7 --calls 10]

Device events around `calls` back-to-back calls of one variant behind a blocker (a large memset that lets the host run
ahead); the variants alternate round by round after a warm-up of each; median, min and max over the rounds of the per-call
time.  Prints one JSON line."""
from __future__ import annotations

import argparse
import csv
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

HBM_BYTES_PER_S = 6.29e12          # measured float4 copy rate of the MI355X (79 % of the 8 TB/s specification)
MEMBERS = (2, 3, 5, 8)


def log(msg):
    print("[consensus_bench] " + msg, file=sys.stderr, flush=True)


def member_maps(kind, vals, B, H, W, M, device):
    """M packed batches of B maps H x W -> [(buffer, desc, desc_host)]"""
    from hrseg_amd.Data.decode import label_desc
    g = torch.Generator().manual_seed(5)
    vals = torch.tensor(vals, dtype=torch.uint8)
    host = label_desc([(H, W)] * B)
    out = []
    if kind == "smooth":
        block = 64
        coarse = vals[torch.randint(len(vals), (B, (H + block - 1) // block + 1, (W + block - 1) // block + 1), generator=g)]
        base = coarse.repeat_interleave(block, 1).repeat_interleave(block, 2)
        for m in range(M):
            out.append(base[:, 3 * m:3 * m + H, 5 * m:5 * m + W].contiguous().reshape(-1))
    else:
        for m in range(M):
            out.append(vals[torch.randint(len(vals), (B * H * W,), generator=g)])
    return [(buf.to(device), host.to(device), host) for buf in out]


def rounds_of(variants, rounds, calls, blocker):
    """{name: [per-call microseconds, one per round]}; the variants alternate round by round"""
    for fn in variants.values():
        for _ in range(2):
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
    return dict(us_median=round(statistics.median(ts), 1), us_min=round(min(ts), 1), us_max=round(max(ts), 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--H", type=int, default=1400)
    ap.add_argument("--W", type=int, default=2900)
    ap.add_argument("--B", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    a = ap.parse_args()
    from hrseg_amd import _lib, ops
    from hrseg_amd.Data import DeviceConsensus
    data = os.path.join(ROOT, "restrictive-hierarchical-semantic-segmentation_amd", "data")
    with open(os.path.join(data, "class_tree_tl.json")) as f:
        tree = json.load(f)
    with open(os.path.join(data, "class_map.csv")) as f:
        cmap = list(csv.DictReader(f))
    cons = DeviceConsensus(tree, cmap)
    leaves = sorted(v for v, n in cons.value_names.items() if n not in cons.values and n != "none")
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    blocker = torch.empty(1 << 30, dtype=torch.uint8, device=device)
    pixels = a.B * a.H * a.W
    res = {"what": f"consensus, B={a.B}, {a.H}x{a.W}, tl tree ({len(cons.node_names)} nodes)", "rounds": a.rounds, "calls": a.calls,
           "pixels": pixels}
    for kind in ("smooth", "salt"):
        members = member_maps(kind, leaves, a.B, a.H, a.W, max(MEMBERS), device)
        variants, meta, keep = {}, {}, []
        for M in MEMBERS:
            ms, q = members[:M], M // 2 + 1
            total, _ = ops.consensus_cells(len(cons.node_names), M)
            counts = torch.zeros(1, total, dtype=torch.int64, device=device)
            labels = torch.empty(pixels, dtype=torch.uint8, device=device)
            support = torch.empty(pixels, dtype=torch.uint8, device=device)
            sc = (torch.zeros(1, cons.tables.total, dtype=torch.int64, device=device), torch.zeros(1, 2, dtype=torch.int64, device=device))
            pairs = [(i, j) for i in range(M) for j in range(i + 1, M)]

            # the entry points themselves, on tables built once: what is timed is the launch, not the wrapper's host checks
            host = torch.stack([h for _, _, h in ms]).contiguous()
            desc = host.to(device)
            struct = ops._consensus_struct(cons.tables, cons.out_val, cons.none_val, q)
            bufs = _lib.ptr_array([buf for buf, _, _ in ms])
            lut, Cs = cons.tables.device_lut(device), _lib.int_array(list(cons.tables.C))
            keep.append((host, desc, struct, bufs, Cs))
            p = _lib.ptr

            def vote(M=M, bufs=bufs, desc=desc, host=host, struct=struct, labels=labels, counts=counts, support=None):
                _lib.call("hrseg_consensus_labels", M, bufs, p(desc), host.data_ptr(), p(lut), ctypes.byref(struct), p(labels), p(support),
                          p(counts), a.B, 0)

            def vote_support(vote=vote, support=support):
                vote(support=support)

            def yardstick(ms=ms, pairs=pairs, sc=sc, Cs=Cs):
                for i, j in pairs:
                    _lib.call("hrseg_score_labels", p(ms[i][0]), p(ms[i][1]), p(ms[j][0]), p(ms[j][1]), p(lut), len(cons.tables.C), Cs,
                              p(sc[0]), p(sc[1]), a.B, 0)
            variants[f"M{M}_consensus"], variants[f"M{M}_consensus_support"], variants[f"M{M}_score_pairs"] = vote, vote_support, yardstick
            meta[f"M{M}"] = dict(pairs=len(pairs), bound_us=round((M + 1) * pixels / HBM_BYTES_PER_S * 1e6, 1),
                                 bound_support_us=round((M + 2) * pixels / HBM_BYTES_PER_S * 1e6, 1),
                                 yardstick_bound_us=round(2 * len(pairs) * pixels / HBM_BYTES_PER_S * 1e6, 1))
        _lib.launch_count("consensus_labels", reset=True)
        times = rounds_of(variants, a.rounds, a.calls, blocker)
        for M in MEMBERS:
            row = meta[f"M{M}"]
            for what in ("consensus", "consensus_support", "score_pairs"):
                row[what] = summary(times[f"M{M}_{what}"])
            row["consensus_over_yardstick"] = round(row["consensus"]["us_median"] / row["score_pairs"]["us_median"], 3)
            log(json.dumps({kind: {f"M{M}": row}}))
        res[kind] = meta
    print(json.dumps(res))


if __name__ == "__main__":
    main()
