"""Device boundary scoring (csrc/boundary.hip, Data/boundary.py, predictEval) against the numpy reference
tests/boundary_ref.py.  The records are integers: every comparison is torch.equal / np.array_equal."""
import argparse
import csv
import os

import numpy as np
import pytest
import torch

from tests import boundary_ref as R
from tests import score_ref
from tests.decode_harness import _source
from tests.decode_harness import _tree
from tests.helpers import build_model

pytestmark = pytest.mark.gpu

NODES_TL = ["background", "upper", "lower", "tooth", "pulp", "dentin", "enamel", "composite"]
N_, SUM, MAX, WITHIN, PK = range(5)
WIDTHS = (1, 31, 32, 33, 64, 65)                 # bitmap rows of 1, 1, 1, 2, 2, 3 words: full and partial tail words
HEIGHTS = (1, 2, 5, 33, 65)                      # a block's four waves take four rows of a narrow map at a time: 5 is one
#                                                  more; 33 and 65 are one more than one and two rounds of 32 row offsets


def _values(cmap):
    return sorted(score_ref.name2pix(cmap).values())


def _pack(maps, start, gap):
    """maps -> (packed uint8 host buffer, [B,4] host descriptors).  `start` bytes lie in front of the first map, `gap`
    bytes between two maps and behind the last, and they hold valid classes: in front of a map its first pixel's value,
    behind it its last pixel's (a gap is split between its two maps).  A kernel that took such a byte for the pixel above
    the first row or below the last would find the mask going on there and lose border pixels."""
    n = start + sum(m.size + gap for m in maps)
    buf = np.zeros(n, dtype=np.uint8)
    rows, off = [], start
    for k, m in enumerate(maps):
        flat = m.reshape(-1)
        front = off - (start if k == 0 else gap - gap // 2)
        buf[front:off] = flat[0]
        buf[off:off + m.size] = flat
        behind = gap if k == len(maps) - 1 else gap // 2
        buf[off + m.size:off + m.size + behind] = flat[-1]
        rows.append([off, m.shape[0], m.shape[1], 1])
        off += m.size + gap
    return torch.from_numpy(buf), torch.tensor(rows, dtype=torch.int64)


_REF = {}


def _ref(pred, gt, tree_key, tree, cmap, tau2, pct):
    """the reference record of one pair, computed once per (maps, tree, parameters)"""
    key = (pred.shape, pred.tobytes(), gt.tobytes(), tree_key, tau2, pct)
    if key not in _REF:
        _REF[key] = R.score_pair(pred, gt, tree, cmap, tau2, pct)
    return _REF[key]


def _tables(tree, cmap):
    from hrseg_amd.Data import build_score_tables
    return build_score_tables(tree, cmap)


def _run(preds, gts, tree_key, tree, cmap, tau2=4, pct=95, pstart=0, pgap=0, gstart=0, ggap=0, out=None, workspace=None, check=True):
    """ops.score_boundaries on the packed maps -> records (device), after comparing them with the reference"""
    from hrseg_amd import ops
    pbuf, ph = _pack(preds, pstart, pgap)
    gbuf, gh = _pack(gts, gstart, ggap)
    got = ops.score_boundaries(pbuf.cuda(), ph.cuda(), ph, gbuf.cuda(), gh.cuda(), gh, _tables(tree, cmap), tau2, pct, out=out,
                               workspace=workspace)
    assert got.dtype == torch.int64 and got.shape[0] == len(preds) and got.shape[2:] == (2, 5)
    if check:
        want = torch.from_numpy(np.stack([_ref(p, g, tree_key, tree, cmap, tau2, pct) for p, g in zip(preds, gts)]))
        bad = (got.cpu() != want).nonzero().tolist()[:8]
        assert torch.equal(got.cpu(), want), [(i, int(got.cpu()[tuple(i)]), int(want[tuple(i)])) for i in bad]
    return got


def _pair(rng, H, W, vals, extra=()):
    gt = R.blobby(rng, H, W, vals, nblobs=5)
    return R.perturb(rng, gt, list(vals) + list(extra), 0.03), gt


# --------------------------------------------------------------------------------------------------------------------- sizes
def test_every_shape_around_the_words_and_rows():
    """one ragged batch of the 30 shapes, guard bytes around every map; 1 x 1 is among them"""
    tree, cmap = _tree("tl")
    rng = np.random.default_rng(101)
    vals = _values(cmap)
    pairs = [_pair(rng, H, W, vals, extra=(9,)) for H in HEIGHTS for W in WIDTHS]
    got = _run([p for p, _ in pairs], [g for _, g in pairs], "tl", tree, cmap, pstart=3, pgap=5, gstart=1, ggap=2)
    assert int((got[:, :, :, MAX] > 0).sum()) > 20, "the batch has distances to measure"


def test_one_pixel_images():
    tree, cmap = _tree("tl")
    one = lambda v: np.full((1, 1), v, np.uint8)                                    # noqa: E731
    preds, gts = [one(212), one(212), one(0), one(9), one(212)], [one(212), one(255), one(0), one(0), one(9)]
    got = _run(preds, gts, "tl", tree, cmap, tau2=0, pct=100, pstart=1, pgap=1, gstart=2, ggap=3).cpu()
    assert got[0, 1].tolist() == [[1, 0, 0, 1, 0]] * 2 and got[1, 1].tolist() == [[1, 0, 0, 0, 0], [0, 0, 0, 0, 0]]
    assert got[3, 0].tolist() == [[0, 0, 0, 0, 0], [1, 0, 0, 0, 0]] and not got[4].any()


# -------------------------------------------------------------------------------------------------------------- radix digits
def test_distances_in_every_radix_digit():
    """d2 below 256 (the last digit only), around 9 * 10^4 (three digits) and above 2^24 (all four)"""
    tree, cmap = _tree("tl")
    rng = np.random.default_rng(103)
    near_p, near_g = _pair(rng, 12, 15, [0, 212, 255])
    far_p, far_g = np.zeros((40, 300), np.uint8), np.zeros((40, 300), np.uint8)
    far_p[5:30, 2:9] = 212
    far_g[8:36, 290:299] = 212
    far_p[10:14, 140:150] = far_g[11:16, 143:152] = 255                             # (and a near pair in the same map)
    # one row, labelled at its two ends only (the all-pairs reference stays small): dentin against background and back
    line_p, line_g = np.zeros((1, 4200), np.uint8), np.full((1, 4200), 9, np.uint8)
    line_p[0, 0] = line_g[0, 4199] = 170
    line_g[0, 0] = 0
    for pct in (95, 50, 1, 100):
        got = _run([near_p, far_p, line_p], [near_g, far_g, line_g], "tl", tree, cmap, tau2=9, pct=pct, pstart=2, pgap=7, gstart=5, ggap=1)
    got = got.cpu()
    assert int(got[0, :, :, MAX].max()) < 256
    assert 80000 < int(got[1, 1, 0, MAX]) < 100000 and int(got[1, 1, 0, PK]) > 65536
    assert got[2, 5].tolist() == got[2, 0].tolist()[::-1] == [[1, 4199 << 16, 4199 ** 2, 0, 4199 ** 2]] * 2 and 4199 ** 2 > 1 << 24


# ------------------------------------------------------------------------------------------------------------- map contents
def _contents():
    """(pred, gt) pairs of the tl tree: masks touching the image edge; a ring inside a ring; a node absent from the truth,
    from the prediction and from both; values outside the class map; unlabelled truth next to a mask; salt noise"""
    rng = np.random.default_rng(107)
    out = []
    gt = np.full((20, 37), 212, np.uint8)                            # one mask fills the image: its border is the image's rim
    pred = gt.copy()
    pred[:, 30:] = 255
    pred[0:2, :] = 0
    out.append((pred, gt))
    gt = np.zeros((41, 45), np.uint8)                                # ring inside a ring, the inner one thinner in the prediction
    gt[4:37, 4:41] = 170
    gt[8:33, 8:37] = 0
    gt[14:27, 14:31] = 170
    gt[18:23, 18:27] = 0
    pred = np.zeros_like(gt)
    pred[5:36, 5:40] = 170
    pred[8:33, 8:37] = 0
    pred[14:27, 14:31] = 170
    pred[16:25, 16:29] = 0
    out.append((pred, gt))
    gt = np.zeros((18, 33), np.uint8)                                # enamel only predicted, pulp only true, composite nowhere
    gt[3:9, 3:12] = 127
    gt[10:15, 20:30] = 255
    pred = np.zeros_like(gt)
    pred[3:9, 3:12] = 85
    pred[11:16, 19:29] = 255
    out.append((pred, gt))
    gt = R.blobby(rng, 30, 34, [0, 212, 255, 170])                   # foreign values in both maps, unlabelled truth beside masks
    pred = R.perturb(rng, gt, [0, 212, 255, 170, 9, 200], 0.05)
    gt[10:14, 5:20] = 7
    gt[rng.random(gt.shape) < 0.03] = 254
    out.append((pred, gt))
    gt = np.zeros((64, 64), np.uint8)                                # salt: every pixel of the noisy class is a border pixel
    gt[rng.random(gt.shape) < 0.1] = 212
    pred = np.zeros((64, 64), np.uint8)
    pred[rng.random(pred.shape) < 0.1] = 212
    out.append((pred, gt))
    return out


def test_map_contents():
    tree, cmap = _tree("tl")
    pairs = _contents()
    got = _run([p for p, _ in pairs], [g for _, g in pairs], "tl", tree, cmap, tau2=2, pct=95, pstart=1, pgap=3, gstart=2, ggap=5).cpu()
    assert got[0, 1, 1, N_] == 2 * 20 + 2 * 37 - 4, "the rim of the image is the border of a mask that fills it"
    enamel, pulp, composite = 6, 4, 7
    assert got[2, enamel, 0, N_] > 0 and got[2, enamel, 1, N_] == 0 and not got[2, enamel, :, 1:].any()
    assert got[2, pulp, 1, N_] > 0 and got[2, pulp, 0, N_] == 0 and not got[2, pulp, :, 1:].any()
    assert not got[2, composite].any()
    assert got[4, 1, 0, N_] == int((pairs[4][0] == 212).sum()), "salt: every pixel of the class is a border pixel"


# ---------------------------------------------------------------------------------------------------- packing and batching
def test_ragged_batch_of_five_at_every_pair_of_start_alignments():
    tree, cmap = _tree("tl")
    rng = np.random.default_rng(109)
    vals = _values(cmap)
    pairs = [_pair(rng, H, W, vals) for H, W in ((7, 33), (1, 65), (34, 5), (12, 64), (3, 3))]
    for p, g in pairs:                                               # uniform first and last rows: the guard bytes go on with them
        p[0] = g[0] = 212
        p[-1] = g[-1] = 255
    preds, gts = [p for p, _ in pairs], [g for _, g in pairs]
    for ps in range(4):
        for gs in range(4):
            _run(preds, gts, "tl", tree, cmap, pstart=ps, pgap=1 + gs, gstart=gs, ggap=3 - ps + 1)


# --------------------------------------------------------------------------------------------------------------------- trees
def _synthetic(key):
    return {"wide": score_ref.wide_tree, "chain": score_ref.chain_tree}[key]()


@pytest.mark.parametrize("key", ["tl", "ext", "wide", "chain"])
def test_trees(key):
    """both shipped trees, 16 channels in a level, 8 levels"""
    tree, cmap = _tree(key) if key in ("tl", "ext") else _synthetic(key)
    vals = _values(cmap)
    rng = np.random.default_rng(113)
    pairs = [_pair(rng, H, W, vals, extra=(1,)) for H, W in ((23, 70), (40, 31))]
    got = _run([p for p, _ in pairs], [g for _, g in pairs], key, tree, cmap, tau2=1, pct=90, pstart=3, gstart=2, pgap=2, ggap=1)
    C = _tables(tree, cmap).C
    assert got.shape[1] == sum(C) and (key != "wide" or max(C) == 16) and (key != "chain" or len(C) == 8)
    assert int((got[:, :, 0, N_] > 0).sum()) >= 4


# -------------------------------------------------------------------------------------------- repeatability and workspace
def test_repeatable_bytes_dirty_workspace_and_rewritten_records():
    from hrseg_amd import _lib, ops
    tree, cmap = _tree("ext")
    rng = np.random.default_rng(127)
    vals = _values(cmap)
    a = [_pair(rng, 50, 70, vals), _pair(rng, 33, 47, vals)]
    b = [_pair(rng, 50, 70, [0, 212]), _pair(rng, 33, 47, [0, 42])]                   # fewer nodes: records must go back to zero
    first = _run([p for p, _ in a], [g for _, g in a], "ext", tree, cmap).cpu()
    again = _run([p for p, _ in a], [g for _, g in a], "ext", tree, cmap, check=False).cpu()
    assert torch.equal(first, again)
    _lib.set_deterministic(True)
    try:
        det = _run([p for p, _ in a], [g for _, g in a], "ext", tree, cmap, check=False).cpu()
    finally:
        _lib.set_deterministic(False)
    assert torch.equal(first, det)
    # one records tensor and one workspace for three calls; the workspace starts as garbage
    host = torch.tensor([[0, 50, 70, 1], [3500, 33, 47, 1]], dtype=torch.int64)
    need = ops.boundary_workspace_bytes(host, _tables(tree, cmap))
    work = torch.full(((need + 7) // 8,), -1, dtype=torch.int64, device="cuda")
    out = torch.full((2, 11, 2, 5), -7, dtype=torch.int64, device="cuda")
    got = _run([p for p, _ in a], [g for _, g in a], "ext", tree, cmap, out=out, workspace=work)
    assert got is out
    _run([p for p, _ in b], [g for _, g in b], "ext", tree, cmap, out=out, workspace=work)
    assert int((out[:, :, :, N_] == 0).sum()) > 8, "nodes of the first call are absent from the second"
    _run([p for p, _ in a], [g for _, g in a], "ext", tree, cmap, out=out, workspace=work)
    assert torch.equal(out.cpu(), first)
    with pytest.raises(ValueError, match="workspace must be"):
        _run([p for p, _ in a], [g for _, g in a], "ext", tree, cmap, workspace=work[:100], check=False)


def test_launch_counters_and_argument_checks():
    from hrseg_amd import _lib, ops
    tree, cmap = _tree("tl")
    rng = np.random.default_rng(131)
    p, g = _pair(rng, 20, 40, _values(cmap))
    _run([p], [g], "tl", tree, cmap)
    torch.cuda.synchronize()
    families = ["score_boundaries", "score_labels", "label_components", "filter_components", "decode_labels"]
    before = {f: _lib.launch_count(f) for f in families}
    total = _lib.launch_count()
    _run([p], [g], "tl", tree, cmap, check=False)
    assert ops.SCORE_BOUNDARIES_LAUNCHES == 11
    assert _lib.launch_count("score_boundaries") == before["score_boundaries"] + ops.SCORE_BOUNDARIES_LAUNCHES
    assert all(_lib.launch_count(f) == before[f] for f in families[1:]) and _lib.launch_count() == total
    # the refusals of the binding launch nothing
    count = _lib.launch_count("score_boundaries")
    tables = _tables(tree, cmap)
    (pbuf, ph), (gbuf, gh) = _pack([p], 0, 0), _pack([g.T.copy()], 0, 0)
    with pytest.raises(ValueError, match="predicted map 20x40, ground truth 40x20"):
        ops.score_boundaries(pbuf.cuda(), ph.cuda(), ph, gbuf.cuda(), gh.cuda(), gh, tables, 4)
    with pytest.raises(ValueError, match="percentile 0"):
        ops.score_boundaries(pbuf.cuda(), ph.cuda(), ph, pbuf.cuda(), ph.cuda(), ph, tables, 4, 0)
    with pytest.raises(ValueError, match="tau2 -1"):
        ops.score_boundaries(pbuf.cuda(), ph.cuda(), ph, pbuf.cuda(), ph.cuda(), ph, tables, -1)
    with pytest.raises(ValueError, match="out must be"):
        ops.score_boundaries(pbuf.cuda(), ph.cuda(), ph, pbuf.cuda(), ph.cuda(), ph, tables, 4,
                             out=torch.zeros(1, 8, 2, 4, dtype=torch.int64, device="cuda"))
    assert _lib.launch_count("score_boundaries") == count


# ----------------------------------------------------------------------------------------------------------- end to end
def _blocky(rng, vals, H, W):
    coarse = rng.choice(vals, size=(H // 6 + 1, W // 6 + 1))
    return np.ascontiguousarray(np.repeat(np.repeat(coarse, 6, 0), 6, 1)[:H, :W]).astype(np.uint8)


def _check_scores(scores, maps, labels, tree, cmap, tau2, pct):
    """a BoundaryScores against the reference: the records exactly; the four derived tensors are one fp64 square root or
    two fp64 divisions of exact integers away from them: 1e-14 relative covers the rounding of either, NaN where NaN"""
    want = R.score_batch(maps, labels, tree, cmap, tau2, pct)
    assert np.array_equal(scores.records.cpu().numpy(), want)
    for k, v in R.derived(want).items():
        got = getattr(scores, k)
        assert got.dtype == torch.float64 and got.is_cuda and tuple(got.shape) == want.shape[:2]
        assert np.allclose(got.cpu().numpy(), v, rtol=1e-14, atol=0.0, equal_nan=True), k
    return want


@pytest.fixture(scope="module")
def small_model():
    from hrseg_amd.Models import models as PM
    tree, cmap = _tree("tl")
    return build_model(PM, "hrnet", True, tree, 64).cuda(), tree, cmap


def test_device_boundary_score_on_decoded_maps(small_model):
    from hrseg_amd import predictEval as PE
    from hrseg_amd.Data import BoundaryScores, DeviceBoundaryScore
    from hrseg_amd.Data.decode import pack_images
    model, tree, cmap = small_model
    rng = np.random.default_rng(137)
    vals = _values(cmap)
    imgs = [_source(rng, 50, 70, 3), _source(rng, 33, 47, 1)]
    labels = [_blocky(rng, vals, 50, 70), _blocky(rng, vals, 33, 47)]
    args = argparse.Namespace(img_size=64, model_type=1, model_select=1)
    decoded = PE.Predictor(model, tree, cmap, args)(imgs)                        # RaggedLabels of the DeviceDecode
    gbuf, ghost = pack_images(labels)
    bs = DeviceBoundaryScore(tree, cmap, tolerance=2.5, percentile=90)
    assert bs.tau2 == 6
    scores = bs.score(decoded, (gbuf, ghost, ghost))
    assert isinstance(scores, BoundaryScores) and len(scores) == 2 and scores.names == NODES_TL
    want = _check_scores(scores, decoded.unpack(), labels, tree, cmap, 6, 90)
    summary = scores.summary()
    assert list(summary) == NODES_TL
    d = R.derived(want)
    for j, name in enumerate(NODES_TL):
        both = (want[:, j, 0, 0] > 0) & (want[:, j, 1, 0] > 0)
        row = summary[name]
        assert row["images"] == int(both.sum())
        assert row["missed"] == int(((want[:, j, 1, 0] > 0) & (want[:, j, 0, 0] == 0)).sum())
        assert row["spurious"] == int(((want[:, j, 0, 0] > 0) & (want[:, j, 1, 0] == 0)).sum())
        for k in ("hausdorff", "hd_percentile", "assd", "surface_dice"):
            if both.any():
                assert row[k] == pytest.approx(float(d[k][both, j].mean()), rel=1e-12), (name, k)
            else:
                assert np.isnan(row[k])
    with pytest.raises(ValueError, match="percentile"):
        DeviceBoundaryScore(tree, cmap, percentile=0)
    with pytest.raises(ValueError, match="tolerance"):
        DeviceBoundaryScore(tree, cmap, tolerance=-1.0)


def test_predictor_score_boundaries_with_and_without_postprocess(small_model):
    from hrseg_amd import predictEval as PE
    from hrseg_amd.Data import DevicePostprocess
    model, tree, cmap = small_model
    rng = np.random.default_rng(139)
    vals = _values(cmap)
    imgs = [_source(rng, 50, 70, 3), _source(rng, 60, 100, 1), _source(rng, 64, 64, 3)]
    labels = [_blocky(rng, vals, 50, 70), _blocky(rng, vals, 60, 100), _blocky(rng, vals, 33, 47)]
    args = argparse.Namespace(img_size=64, model_type=1, model_select=1)
    plain = PE.Predictor(model, tree, cmap, args)
    scores = plain.score_boundaries(imgs, labels)
    raw = plain.last_labels
    assert [m.shape for m in raw.unpack()] == [l.shape for l in labels]
    _check_scores(scores, raw.unpack(), labels, tree, cmap, 4, 95)
    pp = DevicePostprocess(tree, cmap, 0, {"background": dict(min_area=40, fill="upper"), "upper": dict(min_area=40, fill="lower"),
                                            "lower": dict(min_area=40, fill=0), "tooth": dict(keep_largest=True, fill="background")})
    cleaning = PE.Predictor(model, tree, cmap, args, postprocess=pp)
    cleaned = cleaning.score_boundaries(imgs, labels, tolerance=1.0, percentile=50)
    assert torch.equal(cleaning.last_labels.labels, pp.apply(raw).labels)
    _check_scores(cleaned, cleaning.last_labels.unpack(), labels, tree, cmap, 1, 50)


def test_clean_up_removes_a_speck_and_only_its_nodes_change():
    """a 3-pixel dentin speck far from the tooth: min_area on the tooth removes it, the Hausdorff distance of tooth and
    dentin falls from the speck's distance to the outline's; the speck was a hole in the background, so that node changes
    too; every other node keeps its records"""
    from hrseg_amd.Data import DeviceBoundaryScore, DevicePostprocess, RaggedLabels
    tree, cmap = _tree("tl")
    gt = np.zeros((48, 90), np.uint8)
    gt[10:30, 8:26] = 170
    gt[14:22, 12:20] = 127
    gt[10:13, 8:26] = 85
    gt[36:44, 4:86] = 255
    gt[2:6, 4:86] = 212
    pred = np.roll(gt, 1, 1)
    pred[24, 70:73] = 170                                            # the speck, 44 columns from the tooth
    buf, host = _pack([pred], 0, 0)
    maps = RaggedLabels(buf.cuda(), None, host.cuda(), host)
    gbuf, ghost = _pack([gt], 0, 0)
    bs = DeviceBoundaryScore(tree, cmap)
    before = bs.score(maps, (gbuf, ghost, ghost))
    pp = DevicePostprocess(tree, cmap, 0, {"tooth": dict(min_area=4)})
    clean = pp.apply(maps)
    after = bs.score(clean, (gbuf, ghost, ghost))
    _check_scores(before, [pred], [gt], tree, cmap, 4, 95)
    _check_scores(after, clean.unpack(), [gt], tree, cmap, 4, 95)
    tooth, dentin, touched = 3, 5, [0, 3, 5]
    for node in (tooth, dentin):
        assert float(before.hausdorff[0, node]) >= 44.0 and float(after.hausdorff[0, node]) == 1.0
    rest = [n for n in range(8) if n not in touched]
    assert torch.equal(before.records[:, rest], after.records[:, rest])
    assert not torch.equal(before.records[:, touched], after.records[:, touched])


def test_predict_loop_boundary_option(small_model, tmp_path):
    from hrseg_amd import _lib
    from hrseg_amd import predictEval as PE
    from hrseg_amd.Data import DeviceAugment, DeviceBoundaryScore
    from hrseg_amd.Data.loader import ragged_collate
    from hrseg_amd.Metrics import performance_metrics as PP
    from hrseg_amd.utils.hierarchy import get_classes
    model, tree, cmap = small_model
    size = 64
    rng = np.random.default_rng(149)
    vals = _values(cmap)
    data = []
    for i in range(3):
        img = _source(rng, 40 + 6 * i, 36 + 5 * i, 3 if i % 2 else 1)
        data.append((img, _blocky(rng, vals, img.shape[0], img.shape[1])))
    nc = get_classes(tree, full=True)
    args = argparse.Namespace(model_type=1, model_select=1, num_classes=nc, num_classes_full=nc, batch_size=2, img_size=size)
    aug = DeviceAugment(size, tree, cmap, 1, train=False)
    families = ["score_boundaries", "score_labels", "decode_labels", "label_components", "filter_components", "augment_image",
                "augment_targets", "decode_views", None]

    def batches():
        """what DeviceAugmentLoader(data, batch_size=2, augment=aug, with_sources=True) yields, uploaded on the current
        stream.  The loader takes a new side stream per epoch; a test that only wants batches must not move the streams
        that the tests after it are handed"""
        for k in range(0, len(data), 2):
            dev = ragged_collate(data[k:k + 2]).to(aug.device)
            yield (*aug(dev), dev)

    def run(save, **kw):
        loader = batches()
        mets = [PP.Accuracy(), PP.Jaccardindex(), PP.DiceScore(), PP.Precision(), PP.Recall()]
        start = [_lib.launch_count(f) for f in families]
        res = PE.predict_loop(model, torch.device("cuda"), loader, args, tree, *mets, save_dir=str(tmp_path / save), class_map=cmap,
                              score_sources=True, **kw)
        return res, [_lib.launch_count(f) - s for f, s in zip(families, start)], sorted(os.listdir(tmp_path / save))

    today, launches, files = run("today")                          # the call as it is without the option
    assert launches[0] == 0 and "boundary" not in today and "metrics_boundary.csv" not in files
    with_b, launches_b, files_b = run("with", boundary=DeviceBoundaryScore(tree, cmap, tolerance=1.5, percentile=90))
    none, launches_n, files_n = run("none", boundary=None)
    assert launches_n == launches and files_n == files and list(none) == list(today)
    assert none["source"] == today["source"] and none["performance"] == today["performance"]
    assert launches_b[0] == 2 * 11 and launches_b[1:] == launches[1:], "two batches, nothing else launched"
    assert files_b == sorted(files + ["metrics_boundary.csv"]) and list(with_b) == list(today) + ["boundary"]
    assert with_b["source"] == today["source"]
    # the same numbers from the predictor's maps through the reference
    predictor = PE.Predictor(model, tree, cmap, args)
    maps = predictor([d[0] for d in data[:2]]).unpack() + predictor([d[0] for d in data[2:]]).unpack()
    want = R.score_batch(maps, [d[1] for d in data], tree, cmap, 2, 90)
    d = R.derived(want)
    summary = with_b["boundary"]
    assert list(summary) == NODES_TL
    with open(tmp_path / "with" / "metrics_boundary.csv") as f:
        rows = list(csv.reader(f))
    assert rows[0] == ["Class", "Hausdorff", "HDPercentile", "ASSD", "SurfaceDice", "Images", "Missed", "Spurious"]
    assert [r[0] for r in rows[1:]] == NODES_TL
    for j, name in enumerate(NODES_TL):
        both = (want[:, j, 0, 0] > 0) & (want[:, j, 1, 0] > 0)
        assert summary[name]["images"] == int(both.sum()) == int(rows[1 + j][5])
        if both.any():
            assert summary[name]["hausdorff"] == pytest.approx(float(d["hausdorff"][both, j].mean()), rel=1e-12)
            assert float(rows[1 + j][1]) == summary[name]["hausdorff"]
        else:
            assert rows[1 + j][1] == ""
    with pytest.raises(ValueError, match="boundary needs score_sources"):
        mets = [PP.Accuracy(), PP.Jaccardindex(), PP.DiceScore(), PP.Precision(), PP.Recall()]
        PE.predict_loop(model, torch.device("cuda"), batches(), args, tree, *mets, class_map=cmap,
                        boundary=DeviceBoundaryScore(tree, cmap))
