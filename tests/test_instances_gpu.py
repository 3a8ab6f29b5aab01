"""Device instance scoring (csrc/instances.hip, Data/instances.py, predictEval) against the numpy reference
tests/instances_ref.py, which tests every pair of components and knows nothing about votes.  Records, match maps and
overlaps are integers: every comparison is torch.equal."""
import argparse
import csv
import os

import numpy as np
import pytest
import torch

from tests import instances_ref as R
from tests.decode_harness import _source
from tests.decode_harness import _tree
from tests.helpers import build_model

pytestmark = pytest.mark.gpu

SENTINEL = -7
IDENT = np.arange(256, dtype=np.uint8)
PAIRS = IDENT.copy()                   # values 2k and 2k + 1 form one group (values 0..253), 254 and 255 are group 255
PAIRS[:254] = (np.arange(254) // 2).astype(np.uint8)
PAIRS[254:] = 255
ALL = np.ones(256, dtype=np.uint8)
THR = (750, 900, 0, 501)


def _things(*groups):
    t = np.zeros(256, dtype=np.uint8)
    t[list(groups)] = 1
    return t


def _tile():
    from hrseg_amd import ops
    return ops.components_tile()


def _pack(maps, start, gap):
    """maps -> (packed uint8 host buffer, [B,4] host descriptors, mask of the bytes inside a span).  `start` bytes lie in
    front of the first map, `gap` bytes between two maps and behind the last; they hold the values next to them (in front
    of a map its first pixel's, behind it its last pixel's): a read outside a span, or a run carried across a seam, changes
    components, votes and overlaps."""
    n = start + sum(m.size + gap for m in maps)
    buf = np.zeros(n, dtype=np.uint8)
    inside = np.zeros(n, dtype=bool)
    rows, off = [], start
    for k, m in enumerate(maps):
        flat = m.reshape(-1)
        front = off - (start if k == 0 else gap - gap // 2)
        buf[front:off] = flat[0]
        buf[off:off + m.size] = flat
        inside[off:off + m.size] = True
        behind = gap if k == len(maps) - 1 else gap // 2
        buf[off + m.size:off + m.size + behind] = flat[-1]
        rows.append([off, m.shape[0], m.shape[1], 1])
        off += m.size + gap
    return buf, torch.tensor(rows, dtype=torch.int64), inside


_REF = {}


def _ref(pred, gt, group, things, conn, thr):
    """the reference of one pair, computed once per (maps, tables, parameters) and never changed"""
    key = (pred.shape, pred.tobytes(), gt.tobytes(), group.tobytes(), things.tobytes(), conn, tuple(thr))
    if key not in _REF:
        _REF[key] = R.score_pair(pred, gt, group, things, conn, thr)
    return _REF[key]


def _equal(got, want, what):
    got, want = got.cpu(), torch.from_numpy(np.ascontiguousarray(want))
    bad = (got != want).nonzero().tolist()[:6]
    assert torch.equal(got, want), (what, [(i, int(got[tuple(i)]), int(want[tuple(i)])) for i in bad])


def _run(preds, gts, group, things, conn=8, thr=THR, pstart=0, pgap=0, gstart=0, ggap=0, per_image=True, out=None, workspace=None,
         base=None):
    """mask + two labellings + score on the packed maps, everything compared with the reference: the masked copy, the
    records (added to `base`, the host copy of out's records before the call), the three maps inside the spans and the
    sentinel outside -> (records, pmatch, gmatch, ginter) device tensors and the per-image references"""
    from hrseg_amd import ops
    pbuf, ph, pin = _pack(preds, pstart, pgap)
    gbuf, gh, gin = _pack(gts, gstart, ggap)
    refs = [_ref(p, g, group, things, conn, thr) for p, g in zip(preds, gts)]
    dp, dg = torch.from_numpy(pbuf).cuda(), torch.from_numpy(gbuf).cuda()
    dph, dgh = ph.cuda(), gh.cuda()
    dgroup, dthings = torch.from_numpy(group).cuda(), torch.from_numpy(things).cuda()
    pm = torch.from_numpy(pbuf ^ 0x5A).cuda()                      # what must survive outside the spans
    got = ops.mask_void_labels(dp, dph, ph, dg, dgh, gh, dgroup, group.tolist(), out=pm)
    assert got is pm
    want_pm = pbuf ^ 0x5A
    for (off, H, W, _), r in zip(ph.tolist(), refs):
        want_pm[off:off + H * W] = r["pm"].reshape(-1)
    # (the reference writes the smallest byte of group 255 at void pixels, the wrapper the largest: compared by group there)
    void = np.zeros(pbuf.size, dtype=bool)
    for (off, H, W, _), (goff, _, _, _) in zip(ph.tolist(), gh.tolist()):
        void[off:off + H * W] = group[gbuf[goff:goff + H * W]] == 255
    got_pm = pm.cpu().numpy()
    assert np.array_equal(got_pm[~void], want_pm[~void]) and (group[got_pm[void]] == 255).all()
    assert torch.equal(dp.cpu(), torch.from_numpy(pbuf)) and torch.equal(dg.cpu(), torch.from_numpy(gbuf)), "inputs are not written"
    proots, parea = ops.label_components(pm, dph, ph, dgroup, conn)
    groots, garea = ops.label_components(dg, dgh, gh, dgroup, conn)
    R_ = len(preds) if per_image else 1
    if out is None:
        out = (torch.zeros((R_, 256, 10), dtype=torch.int64, device="cuda"),
               torch.full((pbuf.size,), SENTINEL, dtype=torch.int32, device="cuda"),
               torch.full((gbuf.size,), SENTINEL, dtype=torch.int32, device="cuda"),
               torch.full((gbuf.size,), SENTINEL, dtype=torch.int32, device="cuda"))
        base = np.zeros((R_, 256, 10), dtype=np.int64)
    res = ops.score_instances(pm, dph, ph, proots, parea, dg, dgh, gh, groots, garea, dgroup, dthings, thr, per_image, out, workspace)
    assert all(a is b for a, b in zip(res, out)), "out= tensors are returned as given"
    records = np.stack([r["records"] for r in refs])
    _equal(res[0], base + (records if per_image else records.sum(axis=0, keepdims=True)), "records")
    want_p = np.full(pbuf.size, SENTINEL, dtype=np.int32)
    want_g, want_i = np.full(gbuf.size, SENTINEL, dtype=np.int32), np.full(gbuf.size, SENTINEL, dtype=np.int32)
    for (poff, H, W, _), (goff, _, _, _), r in zip(ph.tolist(), gh.tolist(), refs):
        want_p[poff:poff + H * W] = r["pmatch"].reshape(-1)
        want_g[goff:goff + H * W] = r["gmatch"].reshape(-1)
        want_i[goff:goff + H * W] = r["ginter"].reshape(-1)
    _equal(res[1], want_p, "pmatch")
    _equal(res[2], want_g, "gmatch")
    _equal(res[3], want_i, "ginter")
    return res, refs


def _totals(refs, g):
    rec = sum(r["records"][g] for r in refs)
    return int(rec[R.TP]), int(rec[R.N_PRED] - rec[R.TP]), int(rec[R.N_GT] - rec[R.TP])        # tp, fp, fn


# ---------------------------------------------------------------------------------------------------------------- patterns
def _blob_pair(rng, H, W):
    """ground truth: rectangles of the values 4 and 6 on 0; prediction: each one as it is, shifted by a pixel, eroded by a
    pixel or dropped, in the other value of its group (PAIRS: 4, 5 -> group 2; 6, 7 -> group 3)"""
    gt, pred = np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8)
    for _ in range(max(1, H * W // 150)):
        h, w = int(rng.integers(1, min(H, 9) + 1)), int(rng.integers(1, min(W, 12) + 1))
        y, x = int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1))
        v = int(rng.choice([4, 6]))
        gt[y:y + h, x:x + w] = v
        kind = int(rng.integers(0, 4))
        if kind == 0:
            pred[y:y + h, x:x + w] = v + 1
        elif kind == 1:
            dy, dx = (int(d) for d in rng.integers(-1, 2, 2))
            pred[max(0, y + dy):max(0, y + dy + h), max(0, x + dx):max(0, x + dx + w)] = v + 1
        elif kind == 2 and h > 2 and w > 2:
            pred[y + 1:y + h - 1, x + 1:x + w - 1] = v + 1
    return pred, gt


@pytest.mark.parametrize("conn", [4, 8])
def test_every_shape_around_the_tile_and_the_wave(conn):
    """one ragged batch of the 30 shapes (H and W at 1, tile - 1, tile, tile + 1, two tiles and a bit); the two buffers laid
    out differently, guard bytes of the neighbouring values between the maps"""
    TW, TH = _tile()
    rng = np.random.default_rng(61)
    pairs = [_blob_pair(rng, H, W) for H in (1, TH - 1, TH, TH + 1, 2 * TH + 1) for W in (1, 3, TW - 1, TW, TW + 1, 2 * TW + 3)]
    res, refs = _run([p for p, _ in pairs], [g for _, g in pairs], PAIRS, _things(2, 3), conn, pstart=5, pgap=3, gstart=2, ggap=7)
    assert _totals(refs, 2)[0] + _totals(refs, 3)[0] >= 30, "the batch has matches to find"


def test_every_start_alignment_of_both_buffers():
    TW, TH = _tile()
    rng = np.random.default_rng(67)
    pairs = [_blob_pair(rng, 3, TW + 5), _blob_pair(rng, TH + 1, 19)]
    preds, gts = [p for p, _ in pairs], [g for _, g in pairs]
    for s in range(16):
        _run(preds, gts, PAIRS, _things(2, 3), 8, pstart=s, pgap=5, gstart=15 - s, ggap=2)
    for s in (0, 7):
        _run(preds, gts, PAIRS, _things(2, 3), 4, pstart=s, pgap=1, gstart=s, ggap=0)


# ---------------------------------------------------------------------------------------------------- the exact boundary
def test_known_answers_at_the_exact_boundary():
    """IoU exactly 1/2 does not match, 2/3 and 3/4 do; 3/4 counts at 750 per mille and not at 751; and the same around
    components of one row that cross two tile borders"""
    TW, TH = _tile()
    gt, pred = np.zeros((7, 9), np.uint8), np.zeros((7, 9), np.uint8)
    gt[1, 1:5], pred[1, 1:3] = 9, 9
    gt[3, 2:5], pred[3, 3:5] = 9, 9
    gt[5, 4:8], pred[5, 4:7] = 9, 9
    n = 2 * TW + 1
    wide_g, wide_p = np.zeros((7, 2 * TW + 3), np.uint8), np.zeros((7, 2 * TW + 3), np.uint8)
    wide_g[1, 0:n], wide_p[1, 0:TW + 1] = 9, 9                      # 65 of 129: 195 > 194, the smallest majority
    wide_g[3, 0:n], wide_p[3, 0:TW] = 9, 9                          # 64 of 129: no match
    wide_g[5, 0:n + 1], wide_p[5, n + 1 - (TW + 1):n + 1] = 9, 9    # 65 of 130: exactly 1/2, no match
    res, refs = _run([pred, wide_p], [gt, wide_g], IDENT, _things(9), 8, thr=(750, 751, 0, 667), pstart=1, gstart=3, ggap=2)
    q23, q34 = (2 << 30) // 3, (3 << 30) // 4
    assert res[0][0, 9].tolist() == [3, 3, 2, q23 + q34, 5, 7, 1, 0, 0, 1]
    assert res[0][1, 9].tolist() == [3, 3, 1, ((TW + 1) << 30) // n, TW + 1, n, 0, 0, 0, 0]


# ---------------------------------------------------------------------------------------------------------------- the vote
def _comb_case(share):
    """G: 24 x 160 pixels of value 4.  The prediction inside it: a comb of value 5 (a spine and teeth three rows thick, the
    rows between them of another group), trimmed at the tips of its teeth to exactly `share` pixels, and 228 one-pixel
    components of G's group, kept apart by the other group"""
    H, W = 26, 164
    gt, pred = np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8)
    gt[1:25, 2:162] = 4
    box = pred[1:25, 2:162]
    box[:] = 6
    box[:, 0] = 5
    teeth = [r for r in range(24) if r % 4 != 3]
    box[teeth, 0:120] = 5
    box[0::2, 122::2] = 4                                          # confetti: even rows, every other column
    extra = int((box[:, :120] == 5).sum()) - share
    assert extra >= 0
    for c in range(119, 0, -1):
        for r in teeth:
            if extra:
                box[r, c] = 6
                extra -= 1
    assert int((box[:, :120] == 5).sum()) == share
    return pred, gt


def test_the_vote():
    """(a) a comb holds 51 % of G, hundreds of one-pixel components share the rest: a match; (b) the comb at exactly 50 %: none;
    (c) G shared in thirds: no majority, no match; (d) P holds all of G but is so large that IoU < 1/2; (e) many true
    components inside one huge predicted one"""
    area = 24 * 160
    a = _comb_case(int(0.51 * area))
    b = _comb_case(area // 2)
    gt_c, pred_c = np.zeros((11, 35), np.uint8), np.full((11, 35), 6, np.uint8)
    gt_c[1:10, 2:33] = 4
    for x0 in (2, 13, 24):
        pred_c[1:10, x0:x0 + 9] = 4
    gt_d, pred_d = np.zeros((44, 50), np.uint8), np.zeros((44, 50), np.uint8)
    gt_d[10:20, 10:20] = 4
    pred_d[2:42, 2:42] = 5
    gt_e, _ = R.rectangles(np.random.default_rng(71), 64, 140, 4, 3, 6, 9)
    pred_e = np.zeros((64, 140), np.uint8)
    pred_e[0:62, 0:136] = 5
    cases = [a, b, (pred_c, gt_c), (pred_d, gt_d), (pred_e, gt_e)]
    res, refs = _run([p for p, _ in cases], [g for _, g in cases], PAIRS, _things(2), 8, pstart=3, pgap=1, gstart=0, ggap=4)
    rec = res[0][:, 2, :3].tolist()
    assert rec[0] == [1, 229, 1] and rec[1] == [1, 229, 0], "the comb matches at 51 %, not at exactly 50 %"
    assert rec[2] == [1, 3, 0] and rec[3] == [1, 1, 0]
    assert rec[4][0] > 50 and rec[4][1:] == [1, 0]
    assert int(res[3].max()) == int(0.51 * area)
    # the same with every group a thing: the background and the other group vote and match as well
    _run([p for p, _ in cases], [g for _, g in cases], PAIRS, ALL, 4)


# ------------------------------------------------------------------------------------------------------- void and things
def test_void_and_values_outside_the_class_map():
    gt = np.full((20, 70), 4, np.uint8)
    gt[:, 30:33] = 254                                             # a void band: cuts the predicted region in two
    gt[15:20, 50:60] = 255                                         # a void patch that holds a whole predicted region
    gt[0:3, 0:3] = 0
    pred = np.zeros((20, 70), np.uint8)
    pred[2:12, 5:60] = 5                                           # group 2 as the truth's 4: the kernels compare groups
    pred[16:19, 52:58] = 4
    pred[4:6, 8:12] = 255                                          # outside the class map: a hole in the predicted region
    pred[13, 0:30] = 254
    res, refs = _run([pred], [gt], PAIRS, _things(0, 2), 8, pstart=2, gstart=9)
    # the truth's group 2 and the predicted region are both cut in two; the predicted background in three (the band, and the
    # row of 254 on its left); the region in the void patch is gone
    assert res[0][0, 2, :3].tolist() == [2, 2, 0] and res[0][0, 0, :2].tolist() == [1, 3]
    full = IDENT.copy()                                            # no byte of group 255: nothing is void, a plain copy
    _run([pred], [gt], full, ALL, 8)


def test_one_thing_group_of_four_leaves_the_other_rows_alone():
    rng = np.random.default_rng(73)
    gt, boxes = R.rectangles(rng, 50, 90, 4)
    pred = R.perturbed(rng, gt.shape, boxes, 5, salt=0.01, salt_values=(2, 6, 8))
    gt[40:48, 10:80] = 6
    gt[2:5, 70:88] = 8
    from hrseg_amd import ops
    base = np.arange(2 * 256 * 10, dtype=np.int64).reshape(2, 256, 10) + 1000
    out = (torch.from_numpy(base.copy()).cuda(), torch.full((2 * gt.size,), SENTINEL, dtype=torch.int32, device="cuda"),
           torch.full((2 * gt.size,), SENTINEL, dtype=torch.int32, device="cuda"),
           torch.full((2 * gt.size,), SENTINEL, dtype=torch.int32, device="cuda"))
    res, refs = _run([pred, gt], [gt, gt], PAIRS, _things(2), 8, out=out, base=base)
    rows = [g for g in range(256) if g != 2]
    assert torch.equal(res[0][:, rows].cpu(), torch.from_numpy(base[:, rows])), "rows of groups that are no things are not touched"
    assert _totals(refs[:1], 2)[0] >= 5 and refs[1]["records"][2, R.TP] == refs[1]["records"][2, R.N_GT] > 10
    firsts = {int(i) for i in (res[2][:gt.size] != -2).nonzero().flatten()}
    assert firsts == {int(i) for i in np.nonzero((refs[0]["garea"].reshape(-1) > 0) & (PAIRS[gt.reshape(-1)] == 2))[0]}
    assert ops.SCORE_INSTANCES_LAUNCHES == 5


# ------------------------------------------------------------------------------------------------------ realistic maps
def _noisy(seed):
    """a grid of rectangles 6..10 pixels on a side at (2 TH + 1) x (2 TW + 3) = 65 x 131; the prediction: shifted by up to 2
    pixels, resized by +-1, 15 % dropped, 0.4 % salt noise; a void rectangle in the truth"""
    TW, TH = _tile()
    H, W = 2 * TH + 1, 2 * TW + 3
    rng = np.random.default_rng(seed)
    gt, boxes = R.rectangles(rng, H, W, 4)
    pred = R.perturbed(rng, (H, W), boxes, 5, drop=0.15, shift=2, salt=0.004, salt_values=(0, 4, 5, 7))
    gt[20:30, 60:75] = 254
    return pred, gt


NOISY_SEEDS = (101, 102, 103)


def test_noisy_maps():
    pairs = [_noisy(s) for s in NOISY_SEEDS]
    assert pairs[0][0].shape == (65, 131)
    for conn in (4, 8):
        for pred, gt in pairs:
            tp, fp, fn = _totals([_ref(pred, gt, PAIRS, _things(2), conn, THR)], 2)
            print(f"noisy map, connectivity {conn}: tp {tp} fp {fp} fn {fn}")
            assert tp >= 10 and fp >= 10 and fn >= 10, "a degenerate input proves nothing"
        _run([p for p, _ in pairs], [g for _, g in pairs], PAIRS, _things(2), conn, pstart=6, pgap=9, gstart=1, ggap=3)


def test_accumulation_dirty_workspace_and_per_image():
    from hrseg_amd import ops
    pairs = [_noisy(s) for s in NOISY_SEEDS[:2]]
    preds, gts = [p for p, _ in pairs], [g for _, g in pairs]
    things = _things(0, 2)
    first, refs = _run(preds, gts, PAIRS, things, 8)
    want = first[0].cpu().numpy()
    # a second call adds to the records; a workspace full of 0xFF gives the same bytes
    need = ops.instances_workspace_bytes(*(2 * [torch.tensor([[0, 65, 131, 1], [65 * 131, 65, 131, 1]], dtype=torch.int64)]))
    dirty = torch.full(((need + 7) // 8,), -1, dtype=torch.int64, device="cuda")
    again, _ = _run(preds, gts, PAIRS, things, 8, out=first, base=want.copy(), workspace=dirty)
    assert torch.equal(again[0].cpu(), torch.from_numpy(2 * want))
    assert not torch.equal(dirty.cpu(), torch.full_like(dirty, -1).cpu()), "the workspace was used"
    # per_image = 0: one row, the sum over the images; twice into the same row
    one, _ = _run(preds, gts, PAIRS, things, 8, per_image=False)
    assert tuple(one[0].shape) == (1, 256, 10) and torch.equal(one[0].cpu()[0], torch.from_numpy(want.sum(axis=0)))
    _run(preds, gts, PAIRS, things, 8, per_image=False, out=one, base=want.sum(axis=0, keepdims=True))
    with pytest.raises(ValueError, match="workspace"):
        ops.score_instances(*_args_for_refusal(preds, gts), workspace=torch.empty(8, dtype=torch.int64, device="cuda"))


def _args_for_refusal(preds, gts):
    from hrseg_amd import ops
    pbuf, ph, _ = _pack(preds, 0, 0)
    gbuf, gh, _ = _pack(gts, 0, 0)
    dp, dg, dgroup = torch.from_numpy(pbuf).cuda(), torch.from_numpy(gbuf).cuda(), torch.from_numpy(PAIRS).cuda()
    pr, pa = ops.label_components(dp, ph.cuda(), ph, dgroup, 8)
    gr, ga = ops.label_components(dg, gh.cuda(), gh, dgroup, 8)
    return dp, ph.cuda(), ph, pr, pa, dg, gh.cuda(), gh, gr, ga, dgroup, torch.from_numpy(ALL).cuda()


def test_five_runs_give_identical_bytes():
    pairs = [_noisy(s) for s in NOISY_SEEDS]
    first = None
    for _ in range(5):
        res, _ = _run([p for p, _ in pairs], [g for _, g in pairs], PAIRS, ALL, 8, pstart=3, gstart=5, ggap=2)
        got = [t.cpu() for t in res]
        first = got if first is None else first
        assert all(torch.equal(a, b) for a, b in zip(first, got))
    from hrseg_amd import _lib
    _lib.set_deterministic(True)                                   # integers throughout: the knob changes nothing
    try:
        res, _ = _run([p for p, _ in pairs], [g for _, g in pairs], PAIRS, ALL, 8, pstart=3, gstart=5, ggap=2)
    finally:
        _lib.set_deterministic(False)
    assert all(torch.equal(a, t.cpu()) for a, t in zip(first, res))


def test_one_larger_map():
    """512 x 768 with a few hundred blobs: hundreds of tiles, hundreds of waves of the vote"""
    rng = np.random.default_rng(79)
    gt, boxes = R.rectangles(rng, 512, 768, 4, 8, 24, 30)
    pred = R.perturbed(rng, gt.shape, boxes, 5, drop=0.1, shift=3, salt=0.0005, salt_values=(4, 7))
    res, refs = _run([pred], [gt], PAIRS, ALL, 8, pstart=3, gstart=1)
    tp, fp, fn = _totals(refs, 2)
    assert len(boxes) > 300 and tp > 100 and fp > 10 and fn > 10


# ------------------------------------------------------------------------------------------------------ the Python layer
def _check_scores(scores, inst, maps, labels):
    """an InstanceScores of one call against the reference on the host maps"""
    group, things = np.array(inst.tables.group, dtype=np.uint8), np.array(inst.things, dtype=np.uint8)
    refs = [_ref(m, l, group, things, inst.tables.connectivity, tuple(inst.thresholds)) for m, l in zip(maps, labels)]
    _equal(scores.records, np.stack([r["records"] for r in refs]), "records")
    for name, key in (("pmatch", "pmatch"), ("gmatch", "gmatch"), ("ginter", "ginter"), ("proots", "proots"), ("groots", "groots")):
        _equal(getattr(scores, name), np.concatenate([r[key].reshape(-1) for r in refs]), name)
    return refs


def test_launch_counters_summary_and_instances():
    from hrseg_amd import _lib, ops
    from hrseg_amd.Data import DeviceInstanceScore, InstanceScores, RaggedLabels
    from hrseg_amd.Data.instances import summarize
    tree, cmap = _tree("tl")
    inst = DeviceInstanceScore(tree, cmap, 0, ["tooth", "upper"], thresholds=(0.75,))
    rng = np.random.default_rng(83)
    gts, preds = [], []
    for H, W in ((40, 70), (33, 47)):
        gt, boxes = R.rectangles(rng, H, W, 170)
        gt[0:3, :] = 212
        gt[H - 1, 0:9] = 7                                         # no leaf's value: void
        gts.append(gt)
        preds.append(R.perturbed(rng, (H, W), boxes, 127, salt=0.01, salt_values=(212, 42, 9)))
    pbuf, ph, _ = _pack(preds, 0, 0)
    maps = RaggedLabels(torch.from_numpy(pbuf).cuda(), None, ph.cuda(), ph)
    inst.device_tables(torch.device("cuda", 0))
    torch.cuda.synchronize()
    families = ["score_instances", "label_components", "score_labels", "score_boundaries", "decode_labels", "filter_components"]
    before = {f: _lib.launch_count(f) for f in families}
    total = _lib.launch_count()
    scores = inst.score(maps, gts)
    after = {f: _lib.launch_count(f) for f in families}
    assert after["score_instances"] == before["score_instances"] + ops.SCORE_INSTANCES_LAUNCHES
    assert after["label_components"] == before["label_components"] + 6
    assert all(after[f] == before[f] for f in families[2:]) and _lib.launch_count() == total
    assert isinstance(scores, InstanceScores) and len(scores) == 2
    refs = _check_scores(scores, inst, preds, gts)
    records = np.stack([r["records"] for r in refs])
    summary = scores.summary()
    assert list(summary) == ["upper", "tooth", "all", "mean_pq"]
    want = summarize(records, inst.tables.names, inst.thing_ids, inst.thresholds)
    assert summary["tooth"] == want["tooth"] and summary["tooth"]["tp"] >= 5 and summary["tooth"]["tp_at"].keys() == {0.75}
    tp, fp, fn = _totals(refs, 3)
    siou = sum(inter / (int(r["parea"].reshape(-1)[p]) + int(r["garea"].reshape(-1)[g]) - inter) for r in refs
               for p, g, inter in r["pairs"] if inst.tables.group[int(r["pm"].reshape(-1)[p])] == 3)
    assert summary["tooth"]["pq"] == pytest.approx(siou / (tp + fp / 2 + fn / 2), rel=1e-6)
    # the list of true objects, per image
    listed = scores.instances()
    assert len(listed) == 2
    for objs, r, gt in zip(listed, refs, gts):
        W = gt.shape[1]
        firsts = np.nonzero(r["gmatch"].reshape(-1) >= -1)[0].tolist()
        assert [o["first"] for o in objs] == [(f // W, f % W) for f in firsts]
        for o, f in zip(objs, firsts):
            m = int(r["gmatch"].reshape(-1)[f])
            assert o["area"] == int(r["garea"].reshape(-1)[f]) and o["matched"] == (m >= 0)
            assert o["group"] == inst.tables.names[inst.tables.group[int(gt.reshape(-1)[f])]]
            assert o["partner"] == ((m // W, m % W) if m >= 0 else None)
            if m >= 0:
                inter, pa = int(r["ginter"].reshape(-1)[f]), int(r["parea"].reshape(-1)[m])
                assert o["iou"] == inter / (o["area"] + pa - inter) > 0.5
    # out=: the records are added to, the object is returned; cat
    again = inst.score(maps, gts, out=scores)
    assert again is scores and torch.equal(scores.records.cpu(), torch.from_numpy(2 * records))
    both = InstanceScores.cat([scores, inst.score(maps, gts, per_image=False)])
    assert len(both) == 3 and both.summary()["tooth"]["tp"] == 3 * tp


@pytest.fixture(scope="module")
def small_model():
    from hrseg_amd.Models import models as PM
    tree, cmap = _tree("tl")
    return build_model(PM, "hrnet", True, tree, 64).cuda(), tree, cmap


def _blocky(rng, vals, H, W):
    m = rng.choice(np.asarray(vals, dtype=np.uint8), size=((H + 7) // 8, (W + 7) // 8))
    return np.ascontiguousarray(np.kron(m, np.ones((8, 8), np.uint8))[:H, :W])


def test_predictor_score_instances_with_and_without_postprocess(small_model):
    from hrseg_amd import predictEval as PE
    from hrseg_amd.Data import DeviceInstanceScore, DevicePostprocess
    model, tree, cmap = small_model
    rng = np.random.default_rng(89)
    vals = sorted(R.C.name2pix(cmap).values())
    imgs = [_source(rng, 50, 70, 3), _source(rng, 60, 100, 1), _source(rng, 64, 64, 3)]
    labels = [_blocky(rng, vals, 50, 70), _blocky(rng, vals, 60, 100), _blocky(rng, vals + [9], 33, 47)]
    args = argparse.Namespace(img_size=64, model_type=1, model_select=1)
    plain = PE.Predictor(model, tree, cmap, args)
    scores = plain.score_instances(imgs, labels)
    raw = plain.last_labels
    assert [m.shape for m in raw.unpack()] == [l.shape for l in labels]
    inst = DeviceInstanceScore(tree, cmap)
    direct = inst.score(raw, labels)
    for k in ("records", "pmatch", "gmatch", "ginter"):
        assert torch.equal(getattr(scores, k), getattr(direct, k)), k
    _check_scores(scores, inst, raw.unpack(), labels)
    scorer = plain.instance_scorer
    plain.score_instances(imgs, labels)
    assert plain.instance_scorer is scorer, "one scorer per option set"
    plain.score_instances(imgs, labels, things=["tooth"], connectivity=4, thresholds=(0.6,))
    assert plain.instance_scorer is not scorer and plain.instance_scorer.thing_names == ["tooth"]
    pp = DevicePostprocess(tree, cmap, 0, {"background": dict(min_area=40, fill="upper"), "upper": dict(min_area=40, fill="lower"),
                                            "lower": dict(min_area=40, fill=0), "tooth": dict(keep_largest=True, fill="background")})
    cleaning = PE.Predictor(model, tree, cmap, args, postprocess=pp)
    cleaned = cleaning.score_instances(imgs, labels, level=0, things=["tooth", "upper"])
    assert torch.equal(cleaning.last_labels.labels, pp.apply(raw).labels)
    _check_scores(cleaned, cleaning.instance_scorer, cleaning.last_labels.unpack(), labels)


def test_predict_loop_instances_option(small_model, tmp_path):
    from hrseg_amd import _lib
    from hrseg_amd import predictEval as PE
    from hrseg_amd.Data import DeviceAugment, DeviceInstanceScore
    from hrseg_amd.Data.instances import summarize
    from hrseg_amd.Data.loader import ragged_collate
    from hrseg_amd.Metrics import performance_metrics as PP
    from hrseg_amd.utils.hierarchy import get_classes
    model, tree, cmap = small_model
    size = 64
    rng = np.random.default_rng(97)
    vals = sorted(R.C.name2pix(cmap).values())
    data = []
    for i in range(3):
        img = _source(rng, 40 + 6 * i, 36 + 5 * i, 3 if i % 2 else 1)
        data.append((img, _blocky(rng, vals, img.shape[0], img.shape[1])))
    nc = get_classes(tree, full=True)
    args = argparse.Namespace(model_type=1, model_select=1, num_classes=nc, num_classes_full=nc, batch_size=2, img_size=size)
    aug = DeviceAugment(size, tree, cmap, 1, train=False)
    families = ["score_instances", "score_boundaries", "score_labels", "decode_labels", "label_components", "filter_components",
                "augment_image", "augment_targets", "decode_views", None]

    def batches():
        """what DeviceAugmentLoader(data, batch_size=2, augment=aug, with_sources=True) yields, uploaded on the current stream"""
        for k in range(0, len(data), 2):
            dev = ragged_collate(data[k:k + 2]).to(aug.device)
            yield (*aug(dev), dev)

    def run(save, **kw):
        mets = [PP.Accuracy(), PP.Jaccardindex(), PP.DiceScore(), PP.Precision(), PP.Recall()]
        start = [_lib.launch_count(f) for f in families]
        res = PE.predict_loop(model, torch.device("cuda"), batches(), args, tree, *mets, save_dir=str(tmp_path / save), class_map=cmap,
                              score_sources=True, **kw)
        return res, [_lib.launch_count(f) - s for f, s in zip(families, start)], sorted(os.listdir(tmp_path / save))

    today, launches, files = run("today")                          # the call as it is without the option
    assert launches[0] == 0 and "instances" not in today and "metrics_instances.csv" not in files
    inst = DeviceInstanceScore(tree, cmap, things=["tooth", "upper", "lower"])
    with_i, launches_i, files_i = run("with", instances=inst)
    none, launches_n, files_n = run("none", instances=None)
    assert launches_n == launches and files_n == files and list(none) == list(today)
    assert none["source"] == today["source"] and none["performance"] == today["performance"]
    assert launches_i[0] == 2 * 5 and launches_i[4] == launches[4] + 2 * 6, "two batches: the stage's launches and two labellings each"
    assert [n for k, n in enumerate(launches_i) if k not in (0, 4)] == [n for k, n in enumerate(launches) if k not in (0, 4)]
    assert files_i == sorted(files + ["metrics_instances.csv"]) and list(with_i) == list(today) + ["instances"]
    assert with_i["source"] == today["source"]
    # the same numbers from the predictor's maps through the reference
    predictor = PE.Predictor(model, tree, cmap, args)
    maps = predictor([d[0] for d in data[:2]]).unpack() + predictor([d[0] for d in data[2:]]).unpack()
    group, things = np.array(inst.tables.group, dtype=np.uint8), np.array(inst.things, dtype=np.uint8)
    records, _ = R.score_batch(maps, [d[1] for d in data], group, things, 8, inst.thresholds)
    want = summarize(records, inst.tables.names, inst.thing_ids, inst.thresholds)
    got = with_i["instances"]
    assert list(got) == ["upper", "lower", "tooth", "all", "mean_pq"]
    for name in ("upper", "lower", "tooth", "all"):
        assert {k: v for k, v in got[name].items() if v == v} == {k: v for k, v in want[name].items() if v == v}, name
    with open(tmp_path / "with" / "metrics_instances.csv") as f:
        rows = list(csv.reader(f))
    assert rows[0] == ["Group", "GT", "Predicted", "TP", "FP", "FN", "Precision", "Recall", "RQ", "SQ", "PQ", "MeanIoU", "TPAt0.75",
                       "TPAt0.9"]
    assert [r[0] for r in rows[1:]] == ["upper", "lower", "tooth", "all"]
    for r in rows[1:]:
        assert [int(v) for v in r[1:6]] == [got[r[0]][k] for k in ("n_gt", "n_pred", "tp", "fp", "fn")]
        assert r[10] == ("" if got[r[0]]["pq"] != got[r[0]]["pq"] else str(got[r[0]]["pq"]))
    with pytest.raises(ValueError, match="instances needs score_sources"):
        mets = [PP.Accuracy(), PP.Jaccardindex(), PP.DiceScore(), PP.Precision(), PP.Recall()]
        PE.predict_loop(model, torch.device("cuda"), batches(), args, tree, *mets, class_map=cmap, instances=inst)
