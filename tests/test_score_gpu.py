"""Device scoring pipeline (csrc/score.hip, Data/score.py, predictEval) against the numpy reference tests/score_ref.py.
The result is integer counts: every comparison is torch.equal on int64."""
import argparse
import csv
import os

import numpy as np
import pytest
import torch

from tests import score_ref as R
from tests.decode_harness import _source
from tests.decode_harness import _tree as _shipped_tree
from tests.helpers import build_model

pytestmark = pytest.mark.gpu


def _tree(key):
    if key in ("wide", "chain", "flat", "uniform"):
        return {"wide": R.wide_tree, "chain": R.chain_tree, "flat": R.flat_tree, "uniform": R.uniform_tree}[key]()
    return _shipped_tree(key)


def _values(cmap):
    return np.array(sorted(R.name2pix(cmap).values()), dtype=np.uint8)


def _pack(maps, start, gap, guard):
    """maps -> (packed uint8 host buffer, [B,4] host descriptors): the first map starts at byte `start`, `gap` bytes lie
    between two maps and behind the last; every byte outside the maps holds `guard`"""
    n = start + sum(m.size + gap for m in maps)
    buf = np.full(n, guard, dtype=np.uint8)
    rows, off = [], start
    for m in maps:
        buf[off:off + m.size] = m.reshape(-1)
        rows.append([off, m.shape[0], m.shape[1], 1])
        off += m.size + gap
    return torch.from_numpy(buf), torch.tensor(rows, dtype=torch.int64)


def _run(tables, preds, gts, pstart=0, gstart=0, gap=0, guards=(0, 0), out=None, per_image=True):
    from hrseg_amd import ops
    pbuf, ph = _pack(preds, pstart, gap, guards[0])
    gbuf, gh = _pack(gts, gstart, gap, guards[1])
    return ops.score_labels(pbuf.cuda(), ph.cuda(), ph, gbuf.cuda(), gh.cuda(), gh, tables, out, per_image)


def _want(preds, gts, tree, cmap):
    counts, ignored = R.score_batch(preds, gts, tree, cmap)
    return torch.from_numpy(counts), torch.from_numpy(ignored)


def _equal(got, want):
    assert got[0].dtype == got[1].dtype == torch.int64
    assert torch.equal(got[0].cpu(), want[0]), (got[0].cpu() - want[0]).nonzero().tolist()[:8]
    assert torch.equal(got[1].cpu(), want[1]), (got[1].cpu().tolist(), want[1].tolist())


def _tables(tree, cmap):
    from hrseg_amd.Data import build_score_tables
    return build_score_tables(tree, cmap)


def test_every_start_alignment_with_guard_bytes():
    """one 1x37 image; the prediction span starts at every byte of a 16-byte line (the kernel's aligned loads are 16 bytes
    wide), the ground-truth span at every byte of a dword.  The bytes in front of and behind each span hold a valid but
    different class (upper 212 / lower 255, which the maps do not use): a read outside a span changes the counts."""
    tree, cmap = _tree("tl")
    tables = _tables(tree, cmap)
    rng = np.random.default_rng(1)
    inside = np.array([0, 127, 170, 85, 42], dtype=np.uint8)
    gt, pred = rng.choice(inside, size=(1, 37)), rng.choice(inside, size=(1, 37))
    want = _want([pred], [gt], tree, cmap)
    for pa in range(16):
        for ga in range(4):
            got = _run(tables, [pred], [gt], pstart=32 + pa, gstart=16 + ga, gap=40, guards=(212, 255))
            assert torch.equal(got[0].cpu(), want[0]) and torch.equal(got[1].cpu(), want[1]), (pa, ga)


@pytest.mark.parametrize("pstart,gstart", [(0, 0), (5, 3), (15, 2)])
def test_edge_sizes(pstart, gstart):
    """1x1, 1x3, 3x5 and H*W at one lane-step, wave-step and block-step of the kernel, each minus 1, exact and plus 1"""
    from hrseg_amd import ops
    assert (ops.SCORE_LANE_STEP, ops.SCORE_WAVE_STEP, ops.SCORE_BLOCK_STEP) == (16, 1024, 4096)
    tree, cmap = _tree("tl")
    vals = _values(cmap)
    rng = np.random.default_rng(2)
    shapes = [(1, 1), (1, 3), (3, 5)]
    for s in (ops.SCORE_LANE_STEP, ops.SCORE_WAVE_STEP, ops.SCORE_BLOCK_STEP):
        shapes += [(1, s - 1), (1, s), (1, s + 1)]
    gts = [rng.choice(vals, size=s) for s in shapes]
    preds = [np.where(rng.random(s) < 0.6, g, rng.choice(vals, size=s)) for s, g in zip(shapes, gts)]
    got = _run(_tables(tree, cmap), preds, gts, pstart, gstart, gap=7, guards=(212, 255))
    _equal(got, _want(preds, gts, tree, cmap))


def _ragged_five(vals, seed):
    """the five images of the batch test: (preds, gts)"""
    rng = np.random.default_rng(seed)
    outside = np.array([v for v in range(256) if v not in set(vals.tolist())][:9], dtype=np.uint8)
    a_g, a_p = np.full((300, 500), vals[0], np.uint8), np.full((300, 500), vals[-1], np.uint8)     # one pair everywhere
    n = len(vals)                                                  # every pair, and no two neighbours equal in either map
    idx = rng.integers(0, n, size=(300, 500))
    for x in range(1, 500):
        same = idx[:, x] == idx[:, x - 1]
        idx[same, x] = (idx[same, x] + 1) % n
    b_g, b_p = vals[idx], vals[(idx + rng.integers(0, n, size=idx.shape)) % n]
    xs = np.arange(257) // 3                                       # vertical stripes 3 pixels wide: runs cross lanes
    c_g = np.broadcast_to(vals[xs % n], (64, 257)).copy()
    c_p = np.broadcast_to(vals[(xs // 2) % n], (64, 257)).copy()
    d_g, d_p = rng.choice(vals, size=(50, 70)), rng.choice(vals, size=(50, 70))
    d_g = np.where(rng.random((50, 70)) < 0.1, rng.choice(outside, size=(50, 70)), d_g)
    d_p = np.where(rng.random((50, 70)) < 0.1, rng.choice(outside, size=(50, 70)), d_p)
    e_g, e_p = vals[:1].reshape(1, 1), vals[-1:].reshape(1, 1)
    return [a_p, b_p, c_p, d_p, e_p], [a_g, b_g, c_g, d_g, e_g]


@pytest.mark.parametrize("key", ["tl", "ext", "wide", "chain", "flat"])
def test_ragged_batch_of_five(key):
    tree, cmap = _tree(key)
    tables = _tables(tree, cmap)
    if key == "wide":
        assert tables.K == [4, 17]
    if key == "chain":
        assert len(tables.C) == 8
    if key == "flat":
        assert len(tables.C) == 1
    preds, gts = _ragged_five(_values(cmap), 3)
    want = _want(preds, gts, tree, cmap)
    assert int(want[1][3].min()) > 0, "the fourth image has ignored pixels of both kinds"
    got = _run(tables, preds, gts, pstart=3, gstart=9, gap=5, guards=(int(_values(cmap)[1]), int(_values(cmap)[2])))
    _equal(got, want)
    # += : a second call into the same tensors doubles them; per_image=False is the sum over the rows
    again = _run(tables, preds, gts, pstart=1, gstart=2, out=got)
    assert again[0].data_ptr() == got[0].data_ptr()
    _equal(again, (2 * want[0], 2 * want[1]))
    total = _run(tables, preds, gts, per_image=False)
    _equal(total, (want[0].sum(0, keepdim=True), want[1].sum(0, keepdim=True)))


def test_blocks_stride_over_an_image():
    """64 samples: every sample gets 16 blocks, the 300x500 one has 37 block-steps"""
    tree, cmap = _tree("tl")
    vals = _values(cmap)
    rng = np.random.default_rng(4)
    shapes = [(300, 500)] + [(1 + i % 3, 2 + i % 5) for i in range(63)]
    gts = [rng.choice(vals, size=s) for s in shapes]
    preds = [rng.choice(vals, size=s) for s in shapes]
    _equal(_run(_tables(tree, cmap), preds, gts, pstart=2, gstart=1), _want(preds, gts, tree, cmap))


def test_launch_counts_and_deterministic_mode():
    from hrseg_amd import _lib
    tree, cmap = _tree("ext")
    tables = _tables(tree, cmap)
    preds, gts = _ragged_five(_values(cmap), 6)
    tables.device_lut(torch.device("cuda", 0))
    torch.cuda.synchronize()
    _lib.launch_count(reset=True)
    before, decode = _lib.launch_count("score_labels"), _lib.launch_count("decode_labels")
    out = torch.zeros(5, tables.total, dtype=torch.int64, device="cuda"), torch.zeros(5, 2, dtype=torch.int64, device="cuda")
    plain = _run(tables, preds, gts, out=out)
    assert _lib.launch_count("score_labels") == before + 1
    was = _lib.deterministic()
    _lib.set_deterministic(True)
    try:
        out2 = torch.zeros_like(out[0]), torch.zeros_like(out[1])
        det = _run(tables, preds, gts, out=out2)
    finally:
        _lib.set_deterministic(was)
    assert _lib.launch_count("score_labels") == before + 2
    assert _lib.launch_count() == 0 and _lib.launch_count("decode_labels") == decode
    assert torch.equal(plain[0], det[0]) and torch.equal(plain[1], det[1])
    _equal(det, _want(preds, gts, tree, cmap))


def test_uniform_depth_tree_against_the_network_size_kernels():
    """independent of score_ref: on a tree with every leaf at depth 1 and every pixel labelled the summed counts are those
    of hrseg_predict_metrics (train-loop masking) on the encoded planes of the two maps"""
    from hrseg_amd import ops
    from hrseg_amd.Data import TargetEncoder
    tree, cmap = _tree("uniform")
    tables = _tables(tree, cmap)
    vals = _values(cmap)
    rng = np.random.default_rng(7)
    gt, pred = rng.choice(vals, size=(3, 41, 53)), rng.choice(vals, size=(3, 41, 53))
    got = _run(tables, list(pred), list(gt), per_image=False)
    enc = TargetEncoder(tree, cmap, 1)
    tp, tg = enc(torch.from_numpy(pred).cuda()), enc(torch.from_numpy(gt).cuda())
    s = 0
    for L, n in enumerate(tables.C):
        z = (tp[:, s:s + n] == 1).float().contiguous()
        _, cm = ops.predict_metrics(z, tg[:, s:s + n].contiguous(), child=(L > 0), mask_pred=True, want_onehot=False)
        o, k = tables.offsets[L], tables.K[L]
        assert torch.equal(got[0][0, o:o + k * k].reshape(k, k), cm), L
        s += n
    assert int(got[1].sum()) == 0


def test_argument_checks_raise_without_launching():
    from hrseg_amd import _lib, ops
    tree, cmap = _tree("tl")
    tables = _tables(tree, cmap)
    a, b = np.zeros((4, 6), np.uint8), np.zeros((6, 4), np.uint8)
    (pbuf, ph), (gbuf, gh) = _pack([a], 0, 0, 0), _pack([b], 0, 0, 0)
    before = _lib.launch_count("score_labels")
    with pytest.raises(ValueError, match="predicted map 4x6, ground truth 6x4"):
        ops.score_labels(pbuf.cuda(), ph.cuda(), ph, gbuf.cuda(), gh.cuda(), gh, tables)
    past = ph.clone()
    past[0, 0] = 1
    with pytest.raises(ValueError, match="does not fit"):
        ops.score_labels(pbuf.cuda(), past.cuda(), past, pbuf.cuda(), ph.cuda(), ph, tables)
    with pytest.raises(ValueError, match="out must hold"):
        ops.score_labels(pbuf.cuda(), ph.cuda(), ph, pbuf.cuda(), ph.cuda(), ph, tables,
                         out=(torch.zeros(2, tables.total, dtype=torch.int64, device="cuda"),
                              torch.zeros(1, 2, dtype=torch.int64, device="cuda")))
    assert _lib.launch_count("score_labels") == before


# ----------------------------------------------------------------------------------------------------------- end to end
def _blocky(rng, vals, H, W):
    coarse = rng.choice(vals, size=(H // 6 + 1, W // 6 + 1))
    return np.ascontiguousarray(np.repeat(np.repeat(coarse, 6, 0), 6, 1)[:H, :W])


@pytest.fixture(scope="module")
def small_model():
    from hrseg_amd.Models import models as PM
    tree, cmap = _tree("tl")
    return build_model(PM, "hrnet", True, tree, 64).cuda(), tree, cmap


def test_predictor_score_end_to_end(small_model):
    from hrseg_amd import predictEval as PE
    model, tree, cmap = small_model
    rng = np.random.default_rng(41)
    vals = _values(cmap)
    imgs = [_source(rng, 50, 70, 3), _source(rng, 80, 64, 1), _source(rng, 64, 64, 3)]
    labels = [_blocky(rng, vals, 50, 70), _blocky(rng, vals, 80, 64), _blocky(rng, vals, 33, 47)]   # the last at its own size
    labels[0][:3, :5] = 9                                          # unlabelled ground truth
    args = argparse.Namespace(img_size=64, model_type=1, model_select=1)
    predictor = PE.Predictor(model, tree, cmap, args)
    scores = predictor.score(imgs, labels)
    maps = predictor.last_labels.unpack()
    assert [m.shape for m in maps] == [l.shape for l in labels]
    want = _want(maps, labels, tree, cmap)
    _equal((scores.counts, scores.ignored), want)
    assert scores.ignored[0].tolist() == [15, 0]
    C = scores.tables.C
    for image in (None, 0, 1, 2):
        row = want[0].sum(0) if image is None else want[0][image]
        ref = R.metrics_of(row.numpy(), C)
        got = scores.metric_vectors(image)
        for k in ref:
            assert got[k].dtype == torch.float32 and np.array_equal(got[k].cpu().numpy(), ref[k]), (image, k)
    assert torch.equal(scores.confusion(1, 2).cpu(), want[0][2, 16:].reshape(5, 5))
    assert torch.equal(scores.total().counts.cpu(), want[0].sum(0, keepdim=True))


def test_predict_loop_scores_sources_and_keeps_everything_else(small_model, tmp_path):
    from hrseg_amd import predictEval as PE
    from hrseg_amd.Data import DeviceAugment, DeviceAugmentLoader
    from hrseg_amd.Metrics import performance_metrics as PP
    from hrseg_amd.utils.hierarchy import get_classes
    model, tree, cmap = small_model
    size = 64
    rng = np.random.default_rng(43)
    vals = _values(cmap)
    data = []
    for i in range(3):
        img = _source(rng, 40 + 6 * i, 36 + 5 * i, 3 if i % 2 else 1)
        data.append((img, _blocky(rng, vals, img.shape[0], img.shape[1])))
    nc = get_classes(tree, full=True)
    args = argparse.Namespace(model_type=1, model_select=1, num_classes=nc, num_classes_full=nc, batch_size=2, img_size=size)
    aug = DeviceAugment(size, tree, cmap, 1, train=False)

    def run(save, **kw):
        loader = DeviceAugmentLoader(data, batch_size=2, augment=aug, with_sources=bool(kw))
        mets = [PP.Accuracy(), PP.Jaccardindex(), PP.DiceScore(), PP.Precision(), PP.Recall()]
        return PE.predict_loop(model, torch.device("cuda"), loader, args, tree, *mets, save_dir=str(tmp_path / save), **kw)

    plain = run("plain")
    scored = run("scored", class_map=cmap, score_sources=True)
    both = run("both", class_map=cmap, score_sources=True, label_dir=str(tmp_path / "maps"))
    assert "source" not in plain
    for k in ("accuracy", "iou", "dice", "precision", "recall", "class_metrics", "performance"):
        assert plain[k] == scored[k] == both[k], k
    with open(tmp_path / "plain" / "metrics.csv", "rb") as f0, open(tmp_path / "scored" / "metrics.csv", "rb") as f1:
        assert f0.read() == f1.read()
    assert not os.path.exists(tmp_path / "plain" / "metrics_source.csv")
    with open(tmp_path / "scored" / "metrics_source.csv") as f:
        rows = list(csv.reader(f))
    assert rows[0] == ["Type", "Class", "Accuracy", "IoU", "Dice", "Precision", "Recall"] and rows[1][:2] == ["Average", "All"]
    assert [r[:2] for r in rows[2:]] == [["Class", str(c)] for c in range(8)], "one row per tree node"
    src = scored["source"]
    assert src == both["source"], "the decode of label_dir is reused and scores the same"
    assert src["images"] == 3 and src["names"] == ["background", "upper", "lower", "tooth", "pulp", "dentin", "enamel", "composite"]
    # the same numbers from the predictor's maps through the reference
    predictor = PE.Predictor(model, tree, cmap, args)
    maps = predictor([d[0] for d in data[:2]]).unpack() + predictor([d[0] for d in data[2:]]).unpack()
    counts, ignored = R.score_batch(maps, [d[1] for d in data], tree, cmap)
    assert src["ignored"] == ignored.tolist()
    for k, v in R.metrics_of(counts.sum(0), [4, 4]).items():
        assert np.array_equal(np.asarray(src["total"][k], dtype=np.float32), v), k
        assert [float(r[2 + ["accuracy", "iou", "dice", "precision", "recall"].index(k)]) for r in rows[2:]] == [float(x) for x in v]
    for b in range(3):
        for k, v in R.metrics_of(counts[b], [4, 4]).items():
            assert np.array_equal(np.asarray(src["per_image"][k][b], dtype=np.float32), v), (b, k)
