"""torch-CPU oracle of the device calibration scoring (csrc/calibration.hip, Data/calibration.py), the case list of the GPU
test and the ONE comparison rule, written straight from the class tree (it shares no table with the product).

Oracle, in float64:
  1. every logit is resampled S x S -> H x W with F.interpolate(mode="bilinear", align_corners=False) and divided by the
     level's temperature;
  2. P_0 = sigmoid (flat models: soft-max over the leaves), P_L[c] = P_{L-1}[parent(c)] * softmax over c's sibling group;
  3. the decoded path and its near-tie mask are decode_ref.decode_sample's (gap of a deciding group < 2e-4); T_L = P_L[c_L];
  4. events: node row (L, c): (P_L[c], gt's level-L channel == c) on every labelled pixel; top row L: (T_L, c_L == gt's
     channel) where the path reaches L and the ground truth has a node there;
  5. the integer rule of hrseg_score_calibration step 6 on the fp64 p: q = rint(clip(p, 0, 1) * 2^24), bin = min(n_bins - 1,
     (q * n_bins) >> 24), e = y ? 2^24 - q : q, e12 = (e + 2048) >> 12; (n, pos, sum_q, sum_e2) += (1, y, q, e12^2); a NaN p
     counts n and pos in the extra bin n_bins.

Comparison rule (`compare`), per record (image or batch) and row:
  band    4 x the largest distance of torch-CPU's own fp32 evaluation of the same composition from the fp64 one over the
          case's events, floor 2^-22 (the convention of the decode's confidence).
  movers  events whose p64 lies within `band` of an interior bin edge k / n_bins; on top rows also every labelled pixel of
          the near-tie mask (there the device may decode another path: another p, another y, or no event at all).
  counts  sum over bins of |n_dev - n_ref| <= 2 * movers, and the same for pos (a mover leaves one bin and enters another).
  sums    an event that is no near-tie has |p_dev - p64| <= band, so with D = band * 2^24 + 1 (two roundings to the grid,
          half a step each):   |q_dev - q_ref| <= D,   |e_dev - e_ref| <= D,   |e12_dev - e12_ref| <= D / 4096 + 1 (two
          roundings again), and since e12 <= 4096:   |e12_dev^2 - e12_ref^2| <= 8192 (D / 4096 + 1).  A near-tie top event
          may move by the whole range, 2^24 in either sum.  Hence per row with N binned events and t near-tie pixels:
              |sum_q_dev - sum_q_ref|   <= N D + t 2^24
              |sum_e2_dev - sum_e2_ref| <= N 8192 (D / 4096 + 1) + t 2^24.
          `compare` prints the largest share of either bound that was used.
  nan     the extra bin is compared exactly.
  cap     movers <= 0.5 % of a row's events over the case (`mover_share`); asserted on the oracle alone, on the CPU."""
import numpy as np
import torch
import torch.nn.functional as F

from tests import decode_ref

Q = 1 << 24
BAND_FLOOR = 2.0 ** -22
MOVER_CAP = 0.005

# name -> dict(tree "tl" / "ext", model_type, S, sizes [(H, W)], n_bins, temperature, seed, gap: guard bytes around the maps,
# start: bytes in front of the first map (odd: the maps start at odd bytes)).  Sizes: 1x1, 1x5 and 7x3 (rows narrower than a
# wave, fewer rows than a tile), 37x53 (W no multiple of 4), 5x261 (five tiles across), 70x300 (tiles both ways); S 8 / 12 /
# 24 gives up- and down-scaling and, at 24x24 -> 24x24 and 12x12 -> 12x12, the identity.
CASES = {
    "tl_ragged": dict(tree="tl", model_type=1, S=12, sizes=[(37, 53), (1, 1), (7, 3)], n_bins=15, temperature=None, seed=11,
                      start=1, gap=5),
    "tl_wide": dict(tree="tl", model_type=1, S=24, sizes=[(70, 300), (1, 5), (24, 24)], n_bins=10, temperature=None, seed=12,
                    start=3, gap=7),
    "tl_temp": dict(tree="tl", model_type=1, S=8, sizes=[(5, 261), (37, 53), (12, 9)], n_bins=32, temperature=(2.0, 0.5), seed=13,
                    start=5, gap=3),
    "ext_ragged": dict(tree="ext", model_type=1, S=12, sizes=[(37, 53), (12, 12), (5, 261)], n_bins=15, temperature=None, seed=14,
                       start=7, gap=9),
    "ext_one_bin": dict(tree="ext", model_type=1, S=24, sizes=[(7, 3), (70, 300), (1, 1)], n_bins=1, temperature=None, seed=15,
                        start=1, gap=1),
    "flat_tl": dict(tree="tl", model_type=0, S=12, sizes=[(37, 53), (1, 5), (5, 261)], n_bins=15, temperature=None, seed=16,
                    start=9, gap=11),
    "flat_ext_temp": dict(tree="ext", model_type=0, S=8, sizes=[(70, 300), (7, 3), (8, 8)], n_bins=10, temperature=1.5, seed=17,
                          start=3, gap=5),
}


def tree_levels(tree, model_type):
    """-> (names per level, groups per level [(parent channel at the level above or None, first, count)], leaves {name:
    path of (level, channel)}).  model_type 0: one level over the leaves in breadth-first order, one group."""
    levels = decode_ref.bfs_levels(tree)
    if int(model_type) == 0:
        leaves = [n for lvl in levels for n, kids in lvl if not kids]
        return [leaves], [[(None, 0, len(leaves))]], {n: [(0, c)] for c, n in enumerate(leaves)}
    names = [[n for n, _ in lvl] for lvl in levels]
    groups, parent = [[(None, 0, len(names[0]))]], {}
    for L in range(1, len(levels)):
        g, start = [], 0
        for pc, (pn, kids) in enumerate(levels[L - 1]):
            if kids:
                g.append((pc, start, len(kids)))
                for k in kids:
                    parent[k] = pn
                start += len(kids)
        groups.append(g)
    where = {n: (L, c) for L, lvl in enumerate(names) for c, n in enumerate(lvl)}
    leaves = {}
    for lvl in levels:
        for n, kids in lvl:
            if not kids:
                chain, cur = [], n
                while cur is not None:
                    chain.append(where[cur])
                    cur = parent.get(cur)
                leaves[n] = chain[::-1]
    return names, groups, leaves


def temperatures(temperature, nlevels):
    if temperature is None:
        return [1.0] * nlevels
    t = list(temperature) if isinstance(temperature, (tuple, list)) else [temperature] * nlevels
    assert len(t) == nlevels
    return [float(v) for v in t]


def compose(logits, groups, root_softmax, H, W, temps, dtype):
    """one sample's logits (per level [C_L, S, S]) -> per level P [C_L, H, W] in `dtype`.  fp32: torch's own fp32 resize, one
    multiplication by fp32 1 / T (as the product states it), fp32 sigmoid / soft-max and products."""
    out = []
    for L, a in enumerate(logits):
        v = F.interpolate(a[None].to(dtype), size=(H, W), mode="bilinear", align_corners=False, antialias=False)[0]
        if dtype == torch.float64:
            v = v / temps[L]
        elif temps[L] != 1.0:
            v = v * float(np.float32(1.0) / np.float32(temps[L]))
        if L == 0 and not root_softmax:
            out.append(torch.sigmoid(v))
            continue
        p = torch.empty_like(v)
        for pc, first, n in groups[L]:
            sm = torch.softmax(v[first:first + n], dim=0)
            p[first:first + n] = sm if pc is None else out[L - 1][pc][None] * sm
        out.append(p)
    return out


def gt_channels(gt, leaves, class_map, nlevels):
    """a uint8 label map -> (valid [H,W] bool, per level the ground truth's channel [H,W] int64, -1 where its leaf is shallower)"""
    pix = decode_ref.name2pix(class_map)
    g = torch.from_numpy(np.ascontiguousarray(gt)).long()
    valid = torch.zeros(g.shape, dtype=torch.bool)
    chans = [torch.full(g.shape, -1, dtype=torch.int64) for _ in range(nlevels)]
    for name, chain in leaves.items():
        m = g == pix[name]
        valid |= m
        for L, c in chain:
            chans[L][m] = c
    return valid, chans


def bin_events(rec, p, y, n_bins):
    """step 6 on fp64 probabilities p and outcomes y (1-D arrays) into rec [n_bins + 1, 4] int64"""
    p, y = np.asarray(p, dtype=np.float64), np.asarray(y, dtype=np.int64)
    nan = np.isnan(p)
    rec[n_bins, 0] += int(nan.sum())
    rec[n_bins, 1] += int(y[nan].sum())
    p, y = p[~nan], y[~nan]
    q = np.rint(np.clip(p, 0.0, 1.0) * Q).astype(np.int64)
    b = np.minimum(n_bins - 1, (q * n_bins) >> 24)
    e = np.where(y == 1, Q - q, q)
    e12 = (e + 2048) >> 12
    for col, val in ((0, np.ones_like(q)), (1, y), (2, q), (3, e12 * e12)):
        np.add.at(rec[:, col], b, val)


def oracle(logits, tree, class_map, model_type, gts, n_bins, temperature=None):
    """logits: per level [B, C_L, S, S] fp32 (a flat model: one tensor in a list); gts: B uint8 label maps -> dict(hist [B, R,
    n_bins + 1, 4] int64, ignored [B], names, band, events: per image and row dict(p64, y, ties = near-tie labelled pixels (top
    rows; 0 on node rows)))"""
    names, groups, leaves = tree_levels(tree, model_type)
    nl, root_softmax = len(names), int(model_type) == 0
    temps = temperatures(temperature, nl)
    row0 = np.concatenate([[0], np.cumsum([len(n) for n in names])])
    R = int(row0[-1]) + nl
    B = len(gts)
    hist, ignored = np.zeros((B, R, n_bins + 1, 4), dtype=np.int64), np.zeros(B, dtype=np.int64)
    events, d32 = [], 0.0
    for b, gt in enumerate(gts):
        H, W = gt.shape
        zb = [a[b] for a in logits]
        P = compose(zb, groups, root_softmax, H, W, temps, torch.float64)
        P32 = compose(zb, groups, root_softmax, H, W, temps, torch.float32)
        _, _, tie, path = decode_ref.decode_sample(zb if model_type else zb[0], tree, class_map, model_type, H, W)
        valid, chans = gt_channels(gt, leaves, class_map, nl)
        ignored[b] = int((~valid).sum())
        ties = int((tie & valid).sum())
        rows = []
        for L in range(nl):
            for c in range(len(names[L])):
                p, y = P[L][c][valid].numpy(), (chans[L][valid] == c).numpy()
                d = np.abs(P32[L][c][valid].double().numpy() - p)
                d32 = max(d32, float(np.nanmax(d)) if d.size and not np.all(np.isnan(d)) else 0.0)
                bin_events(hist[b, row0[L] + c], p, y, n_bins)
                rows.append(dict(p64=p, y=y, ties=0))
        for L in range(nl):
            sel = valid & (path[L] >= 0) & (chans[L] >= 0)
            top = P[L].gather(0, path[L].clamp_min(0)[None])[0]
            p, y = top[sel].numpy(), (path[L][sel] == chans[L][sel]).numpy()
            bin_events(hist[b, row0[-1] + L], p, y, n_bins)
            rows.append(dict(p64=p, y=y, ties=ties))
        events.append(rows)
    flat = [n for lvl in names for n in lvl] + [f"top@{L}" for L in range(nl)]
    return dict(hist=hist, ignored=ignored, names=flat, band=max(4.0 * d32, BAND_FLOOR), d32=d32, events=events, n_bins=n_bins)


def edge_movers(p64, n_bins, band):
    """events (not NaN) within `band` of an interior bin edge"""
    p = np.asarray(p64, dtype=np.float64)
    p = p[~np.isnan(p)]
    if n_bins == 1 or p.size == 0:
        return 0
    k = np.rint(p * n_bins)
    return int(((k >= 1) & (k <= n_bins - 1) & (np.abs(p - k / n_bins) <= band)).sum())


def row_movers(ref, images, r):
    ev = [ref["events"][b][r] for b in images]
    return sum(edge_movers(e["p64"], ref["n_bins"], ref["band"]) + e["ties"] for e in ev), sum(e["ties"] for e in ev)


def mover_share(ref):
    """the largest share of movers among a row's events over the whole case (rows without events: 0)"""
    B, worst = len(ref["events"]), 0.0
    for r in range(len(ref["names"])):
        n = sum(len(ref["events"][b][r]["p64"]) for b in range(B))
        movers, _ = row_movers(ref, range(B), r)
        if movers:
            worst = max(worst, movers / n if n else float("inf"))
    return worst


def compare(got, ref, images, what):
    """got [R, n_bins + 1, 4] int64 (numpy) of the images `images` of the case against the oracle, by the rule above; prints
    every figure it asserts"""
    nb, band = ref["n_bins"], ref["band"]
    want = ref["hist"][list(images)].sum(0)
    D = band * Q + 1.0
    used = 0.0
    for r, name in enumerate(ref["names"]):
        movers, ties = row_movers(ref, images, r)
        dn = int(np.abs(got[r, :, 0] - want[r, :, 0]).sum())
        dp = int(np.abs(got[r, :, 1] - want[r, :, 1]).sum())
        assert dn <= 2 * movers and dp <= 2 * movers, (what, name, dn, dp, movers)
        assert np.array_equal(got[r, nb, :2], want[r, nb, :2]) and not got[r, nb, 2:].any(), (what, name, "non-finite bin")
        N = int(want[r, :nb, 0].sum())
        bq, be = N * D + ties * Q, N * 8192.0 * (D / 4096.0 + 1.0) + ties * Q
        dq = abs(int(got[r, :nb, 2].sum()) - int(want[r, :nb, 2].sum()))
        de = abs(int(got[r, :nb, 3].sum()) - int(want[r, :nb, 3].sum()))
        assert dq <= bq and de <= be, (what, name, dq, bq, de, be)
        if N:
            used = max(used, dq / bq, de / be)
        print(f"{what} {name}: {N} events, {movers} movers ({ties} near ties): bins off by {dn} (n) {dp} (pos); "
              f"sum_q off {dq} of {bq:.0f}, sum_e2 off {de} of {be:.0f}")
    print(f"{what}: band {band:.3e} (torch-CPU fp32 {ref['d32']:.3e}), largest share of a sum's bound used {used:.3f}")


def metrics_direct(p, y, n_bins):
    """ECE / MCE / Brier of events evaluated directly in fp64 from the quantised probabilities (no integer sums)"""
    p, y = np.asarray(p, dtype=np.float64), np.asarray(y, dtype=np.float64)
    q = np.rint(np.clip(p, 0, 1) * Q)
    b = np.minimum(n_bins - 1, np.floor(q * n_bins / Q)).astype(np.int64)
    pq = q / Q
    ece, mce = 0.0, 0.0
    for k in range(n_bins):
        m = b == k
        if m.any():
            gap = abs(y[m].mean() - pq[m].mean())
            ece += gap * m.sum() / p.size
            mce = max(mce, gap)
    e = np.where(y == 1, Q - q, q)
    e12 = np.floor((e + 2048) / 4096)
    return dict(ece=ece, mce=mce, brier=float((e12 * e12).sum() / (Q * p.size)))


def case_inputs(name):
    """-> (case dict, tree, class map rows, logits per level [B, C_L, S, S] fp32 ~ N(0, 2^2), gts: B uint8 maps of 4 x 4 blocks
    of leaf values with one unlabelled value (9) among them)"""
    from tests.decode_harness import _tree
    case = CASES[name]
    tree, cmap = _tree(case["tree"])
    names, _, leaves = tree_levels(tree, case["model_type"])
    g = torch.Generator().manual_seed(case["seed"])
    B, S = len(case["sizes"]), case["S"]
    logits = [(2.0 * torch.randn(B, len(n), S, S, generator=g)).contiguous() for n in names]
    rng = np.random.default_rng(case["seed"])
    pix = decode_ref.name2pix(cmap)
    vals = np.array(sorted(pix[n] for n in leaves) + [9], dtype=np.uint8)
    gts = []
    for H, W in case["sizes"]:
        m = rng.choice(vals, size=((H + 3) // 4, (W + 3) // 4), p=[0.95 / (len(vals) - 1)] * (len(vals) - 1) + [0.05])
        gts.append(np.ascontiguousarray(np.kron(m, np.ones((4, 4), np.uint8))[:H, :W]))
    return case, tree, cmap, logits, gts


_REFS = {}


def case_reference(name):
    """the oracle of a case, computed once per process and shared (callers must not change it)"""
    if name not in _REFS:
        case, tree, cmap, logits, gts = case_inputs(name)
        _REFS[name] = oracle(logits, tree, cmap, case["model_type"], gts, case["n_bins"], case["temperature"])
    return _REFS[name]
