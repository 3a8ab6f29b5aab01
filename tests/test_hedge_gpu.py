"""Hedged decode on the device (csrc/decode_hedged.hip, Data/hedge.py, predictEval) against the fp64 torch-CPU oracle
tests/hedge_ref.py by the one rule written there, plus torch.equal identities that need no oracle: all-zero thresholds are the
plain decode bit for bit, hedged labels are prefix nodes of the plain path, thresholds are monotone, the counters are a
bincount of the device's own map, accumulate and repeat, NaN stays loud, guard bytes stay, one launch per call."""
import argparse
import csv
import os

import numpy as np
import pytest
import torch

from tests import hedge_ref as R
from tests.decode_harness import _source, _tree
from tests.helpers import build_model

pytestmark = pytest.mark.gpu

_INPUTS = {}


def _hedge(name, raise_by=0.0):
    from hrseg_amd.Data import Hedge
    case, tree, cmap, _ = R.case_inputs(name)
    names, tau, byte, reject = R.resolve(tree, cmap, case["thresholds"], case["internal"], case["reject"])
    thresholds = {n: (min(1.0, t + raise_by) if t > 0.0 else 0.0) for n, t in tau.items()}
    return Hedge(tree, cmap, thresholds, internal_values=case["internal"], reject_value=reject)


def _inputs(name):
    """(case, tree, class map, device logits, the case's Hedge, a DeviceDecode), uploaded once per case"""
    if name not in _INPUTS:
        from hrseg_amd.Data import DeviceDecode
        case, tree, cmap, logits = R.case_inputs(name)
        _INPUTS[name] = (case, tree, cmap, [z.cuda() for z in logits], _hedge(name), DeviceDecode(tree, cmap, 1))
    return _INPUTS[name]


def _byte_tables(hedge):
    """(cell [256] int64: the counter cell of the node that writes the byte, the reject value -> `nodes`, other bytes -> -1;
    above [256, 256] bool: above[v, w] = w is the byte of v's node or of one of its ancestors, or the reject value)"""
    t = hedge.tables
    cell = torch.full((256,), -1, dtype=torch.int64)
    above = torch.zeros(256, 256, dtype=torch.bool)
    cell0 = [sum(t.C[:L]) for L in range(len(t.C))]
    byte = [[t.pixel_val[L][c] if not t.n_children[L][c] else hedge.stop_val[L][c] for c in range(t.C[L])] for L in range(len(t.C))]

    def walk(L, c, chain):
        v = byte[L][c]
        cell[v] = cell0[L] + c
        chain = chain + [v]
        above[v, chain] = True
        for k in range(t.n_children[L][c]):
            walk(L + 1, t.first_child[L][c] + k, chain)
    for c in range(t.C[0]):
        walk(0, c, [])
    if hedge.reject_val >= 0:
        cell[hedge.reject_val] = sum(t.C)
        above[:, hedge.reject_val] = cell >= 0
    return cell, above


@pytest.mark.parametrize("name", list(R.CASES))
def test_against_the_oracle(name):
    case, tree, cmap, logits, hedge, dec = _inputs(name)
    out = dec.decode_hedged_sizes(logits, hedge, case["sizes"], want_confidence=True)
    R.check(out, R.case_reference(name), name)
    plain = dec.decode_hedged_sizes(logits, hedge, case["sizes"])                 # the kernel without the confidence store
    assert plain.confidence is None and torch.equal(plain.labels, out.labels) and torch.equal(plain.stops, out.stops)
    assert set(np.unique(out.labels.cpu().numpy()).tolist()) <= set(hedge.value_names)


@pytest.mark.parametrize("name", list(R.CASES))
def test_identities_that_need_no_oracle(name):
    from hrseg_amd.Data import Hedge
    case, tree, cmap, logits, hedge, dec = _inputs(name)
    sizes = case["sizes"]
    plain = dec.decode_sizes(logits, sizes, want_confidence=True)
    zero = dec.decode_hedged_sizes(logits, Hedge(tree, cmap, 0.0, internal_values=case["internal"]), sizes, want_confidence=True)
    assert torch.equal(zero.labels, plain.labels), "all-zero thresholds: the labels of hrseg_decode_labels"
    assert torch.equal(zero.confidence.view(torch.int32), plain.confidence.view(torch.int32)), "... and its confidence, bit for bit"
    out = dec.decode_hedged_sizes(logits, hedge, sizes, want_confidence=True)
    cell, above = (t.cuda() for t in _byte_tables(hedge))
    assert bool(above[plain.labels.long(), out.labels.long()].all()), "every hedged label is a prefix node of the plain path"
    assert bool((out.labels != plain.labels).any()), "and the case hedges somewhere"
    same = out.labels == plain.labels
    assert torch.equal(out.confidence[same].view(torch.int32), plain.confidence[same].view(torch.int32))
    assert bool((out.confidence[~same] >= plain.confidence[~same]).all()), "a shorter path has fewer factors <= 1"
    higher = dec.decode_hedged_sizes(logits, _hedge(name, raise_by=0.2), sizes)
    assert bool(above[out.labels.long(), higher.labels.long()].all()), "raising thresholds moves labels to ancestors only"
    assert bool((higher.labels != out.labels).any())
    # the counters are a bincount of the device's own map through the value table
    nodes = sum(hedge.tables.C)
    assert out.stops.shape == (len(sizes), nodes + 2) and out.stops.dtype == torch.int64
    for b, (off, H, W, _) in enumerate(out.desc_host.tolist()):
        cells = cell[out.labels[off:off + H * W].long()]
        assert int(cells.min()) >= 0
        assert torch.equal(torch.bincount(cells, minlength=nodes + 1), out.stops[b, :nodes + 1]), (name, b)
        assert int(out.stops[b, :nodes + 1].sum()) == H * W and int(out.stops[b, nodes + 1]) == 0
    assert (int(out.stops[:, nodes].sum()) > 0) == (case["reject"] is not None)
    again = dec.decode_hedged_sizes(logits, hedge, sizes, want_confidence=True)
    assert torch.equal(again.labels, out.labels) and torch.equal(again.stops, out.stops), "two runs, the same bytes"
    assert torch.equal(again.confidence.view(torch.int32), out.confidence.view(torch.int32))
    twice = dec.decode_hedged_sizes(logits, hedge, sizes, out=again)
    assert twice.stops is again.stops and torch.equal(again.stops, 2 * out.stops) and torch.equal(twice.labels, out.labels)
    assert again.summary()["pixels"] == 2 * sum(h * w for h, w in sizes)
    from hrseg_amd import ops
    with pytest.raises(ValueError, match="stops must be a contiguous int64 device tensor"):
        ops.decode_hedged(logits, hedge, out.desc, out.desc_host, False, again.stops[:, :-1].contiguous())


def test_one_nan_logit_stays_loud():
    """NaN in a level-1 channel (all of it in image 0, one element in image 2): where the walk reaches level 1 near such a tap
    the group's soft-max, T_1 and the plain decode's confidence are NaN; NaN is not below a threshold, so there the walk goes
    on to the plain decode's leaf and the pixel is counted as non-finite"""
    name = "tl_scalar_ragged"
    case, tree, cmap, logits, hedge, dec = _inputs(name)
    poisoned = [logits[0], logits[1].clone()]
    poisoned[1][0, 2] = float("nan")
    poisoned[1][2, 1, 7, 50] = float("nan")
    plain = dec.decode_sizes(poisoned, case["sizes"], want_confidence=True)
    out = dec.decode_hedged_sizes(poisoned, hedge, case["sizes"], want_confidence=True)
    bad = torch.isnan(plain.confidence)
    assert torch.equal(torch.isnan(out.confidence), bad)
    assert torch.equal(out.labels[bad], plain.labels[bad]), "where the confidence is NaN the label is the plain decode's"
    want = [int(bad[off:off + H * W].sum()) for off, H, W, _ in out.desc_host.tolist()]
    assert out.stops[:, -1].tolist() == want and want[0] > 0 and want[1] == want[3] == 0
    nodes = sum(hedge.tables.C)
    assert out.stops[:, :nodes + 1].sum(1).tolist() == [h * w for h, w in case["sizes"]], "on top of the node cells"
    assert out.summary()["nonfinite"] == sum(want)
    clean = dec.decode_hedged_sizes(logits, hedge, case["sizes"])
    assert torch.equal(out.labels[~bad], clean.labels[~bad]), "and nothing else moves"
    labels_only = dec.decode_hedged_sizes(poisoned, hedge, case["sizes"])
    assert torch.equal(labels_only.stops, out.stops), "counted whether or not the confidence is stored"


def test_ragged_offsets_at_odd_bytes_and_guard_bytes():
    """the entry point itself on buffers of our own: maps at odd offsets with gaps between them; every byte and float outside
    the maps comes back unchanged, the maps and the counters are those of the densely packed call"""
    from hrseg_amd import _lib, ops
    name = "ext_dict_edge"
    case, tree, cmap, logits, hedge, dec = _inputs(name)
    dense = dec.decode_hedged_sizes(logits, hedge, case["sizes"], want_confidence=True)
    rows, off = [], 3
    for H, W in case["sizes"]:
        rows.append([off, H, W, 1])
        off += H * W + 5
    n = off + 16
    host = torch.tensor(rows, dtype=torch.int64)
    labels = torch.full((n,), 0xAB, dtype=torch.uint8, device="cuda")
    conf = torch.full((n,), -7.0, dtype=torch.float32, device="cuda")
    stops = torch.zeros(len(rows), sum(hedge.tables.C) + 2, dtype=torch.int64, device="cuda")
    z = [a.contiguous() for a in logits]
    _lib.call("hrseg_decode_hedged", len(z), _lib.ptr_array(z), _lib.int_array(list(hedge.tables.C)),
              ctypes_ref(ops._decode_tree_struct(hedge.tables)), ctypes_ref(ops._hedge_struct(hedge)), _lib.ptr(host.cuda()),
              _lib.ptr(labels), _lib.ptr(conf), _lib.ptr(stops), len(rows), case["S"])
    inside = torch.zeros(n, dtype=torch.bool, device="cuda")
    for (o, H, W, _), (do, _, _, _) in zip(rows, dense.desc_host.tolist()):
        inside[o:o + H * W] = True
        assert torch.equal(labels[o:o + H * W], dense.labels[do:do + H * W])
        assert torch.equal(conf[o:o + H * W].view(torch.int32), dense.confidence[do:do + H * W].view(torch.int32))
    assert bool((labels[~inside] == 0xAB).all()) and bool((conf[~inside] == -7.0).all()), "guard bytes come back unchanged"
    assert torch.equal(stops, dense.stops)


def ctypes_ref(struct):
    import ctypes
    return ctypes.byref(struct)


def test_launch_counts_and_argument_checks():
    from hrseg_amd import _lib, ops
    from hrseg_amd.Data import DeviceDecode, Hedge
    from hrseg_amd.Data.decode import label_desc
    name = "tl_dict_edge"
    case, tree, cmap, logits, hedge, dec = _inputs(name)
    families = ["decode_hedged", "decode_labels", "decode_views", "decode_windows", "score_labels", "score_calibration", None]
    start = [_lib.launch_count(f) for f in families]
    dec.decode_hedged_sizes(logits, hedge, case["sizes"])
    dec.decode_hedged_sizes(logits, hedge, case["sizes"], want_confidence=True)
    assert [_lib.launch_count(f) - s for f, s in zip(families, start)] == [2, 0, 0, 0, 0, 0, 0], "one launch per call, its own family"
    dec.decode_sizes(logits, case["sizes"])
    assert [_lib.launch_count(f) - s for f, s in zip(families, start)] == [2, 1, 0, 0, 0, 0, 0]
    before = _lib.launch_count("decode_hedged")
    host = label_desc(case["sizes"])
    past = host.clone()
    past[-1, 0] += 1
    with pytest.raises(ValueError, match="does not fit"):
        ops.decode_hedged(logits, hedge, past.cuda(), past)
    with pytest.raises(ValueError, match="1 logit levels for a 2-level table"):
        ops.decode_hedged(logits[:1], hedge, host.cuda(), host)
    with pytest.raises(ValueError, match="model_type 0"):
        DeviceDecode(tree, cmap, 0).decode_hedged_sizes(logits[:1], hedge, case["sizes"])
    other_tree, other_map = _tree("ext")
    with pytest.raises(ValueError, match="another class tree"):
        dec.decode_hedged_sizes(logits, Hedge(other_tree, other_map, 0.5), case["sizes"])
    assert _lib.launch_count("decode_hedged") == before


# ------------------------------------------------------------------------------------------------------------ scoring
def _blocky(rng, vals, H, W, block=8):
    m = rng.choice(np.asarray(vals, dtype=np.uint8), size=((H + block - 1) // block, (W + block - 1) // block))
    return np.ascontiguousarray(np.kron(m, np.ones((block, block), np.uint8))[:H, :W])


def _triple(maps):
    from hrseg_amd.Data.decode import pack_images
    buf, host = pack_images(maps)
    return buf, host, host


@pytest.mark.parametrize("name", ["tl_scalar_ragged", "ext_scalar_ragged", "tl_reject_ragged"])
def test_scores_of_a_hedged_map_against_the_plain_maps(name):
    """DeviceScore(internal_values=...) on the hedged map: a path that ends above the ground truth's leaf falls into column 0
    (the synthetic background) of the levels below it, and nothing else moves"""
    from hrseg_amd.Data import DeviceScore
    case, tree, cmap, logits, hedge, dec = _inputs(name)
    rng = np.random.default_rng(case["seed"])
    vals = sorted(R.decode_ref.name2pix(cmap).values()) + [9]                  # 9: unlabelled
    gt = _triple([_blocky(rng, vals, H, W) for H, W in case["sizes"]])
    plain = DeviceScore(tree, cmap).score(dec.decode_sizes(logits, case["sizes"]), gt)
    hedged_maps = dec.decode_hedged_sizes(logits, hedge, case["sizes"])
    scorer = DeviceScore(tree, cmap, hedge.values)
    hedged = scorer.score(hedged_maps, gt)
    rejects = case["reject"] is not None
    nodes = sum(hedge.tables.C)
    assert torch.equal(hedged.ignored[:, 0], plain.ignored[:, 0])
    if not rejects:
        assert torch.equal(hedged.ignored, plain.ignored)
        assert torch.equal(hedged.confusion(0), plain.confusion(0)), "level 0 does not reject: the same matrix"
    else:
        assert bool((hedged.ignored[:, 1] <= hedged_maps.stops[:, nodes]).all()) and int(hedged.ignored[:, 1].sum()) > 0, \
            "a rejected pixel is a prediction outside the class map (where its ground truth is labelled)"
    moved = 0
    for L in range(1, len(hedge.tables.C)):
        h, p = hedged.confusion(L), plain.confusion(L)
        if not rejects:
            assert torch.equal(h.sum(1), p.sum(1)), (name, L, "row sums: every labelled pixel is still counted once")
            assert torch.equal(h[:, 0] - p[:, 0], (p[:, 1:] - h[:, 1:]).sum(1)), "column 0 gains exactly the difference"
        assert bool((h[:, 1:] <= p[:, 1:]).all()), (name, L, "an off-background column only loses")
        moved += int((p[:, 1:] - h[:, 1:]).sum())
    assert moved > 0
    # the leaf-only table would ignore the internal bytes instead
    leaf_only = DeviceScore(tree, cmap).score(hedged_maps, gt)
    assert int(leaf_only.ignored[:, 1].sum()) > int(hedged.ignored[:, 1].sum())


# ------------------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def small_model():
    from hrseg_amd.Models import models as PM
    tree, cmap = _tree("tl")
    return build_model(PM, "hrnet", True, tree, 64).cuda(), tree, cmap


def test_predictor_with_a_hedge(small_model):
    from hrseg_amd import _lib
    from hrseg_amd import predictEval as PE
    from hrseg_amd.Data import DevicePostprocess, DeviceScore, Hedge, HedgedLabels
    from hrseg_amd.Data.decode import label_desc
    model, tree, cmap = small_model
    rng = np.random.default_rng(101)
    vals = sorted(R.decode_ref.name2pix(cmap).values())
    imgs = [_source(rng, 50, 70, 3), _source(rng, 60, 100, 1), _source(rng, 64, 64, 3)]
    labels = [_blocky(rng, vals, 50, 70), _blocky(rng, vals, 60, 100), _blocky(rng, vals + [9], 33, 47)]
    args = argparse.Namespace(img_size=64, model_type=1, model_select=1)
    hedge = Hedge(tree, cmap, 0.3, internal_values={"tooth": 60})
    predictor = PE.Predictor(model, tree, cmap, args, want_confidence=True, keep_logits=True, hedge=hedge)
    start = [_lib.launch_count(f) for f in ("decode_hedged", "decode_labels")]
    out = predictor(imgs)
    assert [_lib.launch_count(f) - s for f, s in zip(("decode_hedged", "decode_labels"), start)] == [1, 0]
    assert isinstance(out, HedgedLabels) and [(H, W) for _, H, W, _ in out.desc_host.tolist()] == [m.shape[:2] for m in imgs]
    direct = predictor.decoder.decode_hedged(predictor.last_logits, hedge, label_desc([m.shape[:2] for m in imgs]), None, True)
    assert torch.equal(out.labels, direct.labels) and torch.equal(out.stops, direct.stops)
    assert torch.equal(out.confidence.view(torch.int32), direct.confidence.view(torch.int32))
    assert set(np.unique(out.labels.cpu().numpy()).tolist()) <= set(vals) | {60}
    s = out.summary()
    assert s["pixels"] == sum(m.shape[0] * m.shape[1] for m in imgs) and s["rejected"] == 0 and list(s["abstained"]) == ["tooth"]
    scores = predictor.score(imgs, labels)
    assert isinstance(predictor.last_labels, HedgedLabels) and predictor.scorer.tables.path[60] == 4
    want = DeviceScore(tree, cmap, hedge.values).score(predictor.last_labels, _triple(labels))
    assert torch.equal(scores.counts, want.counts) and torch.equal(scores.ignored, want.ignored)
    assert int(scores.ignored[2, 0]) > 0 and int(scores.ignored[:, 1].sum()) == 0, "an internal byte is inside the class map now"
    # hedge=None: the calls of before
    start = _lib.launch_count("decode_hedged")
    plain = PE.Predictor(model, tree, cmap, args)(imgs)
    assert not isinstance(plain, HedgedLabels) and _lib.launch_count("decode_hedged") == start
    for kw, what in ((dict(tta=PE.TestTimeAugment()), "tta"), (dict(window=PE.SlidingWindow()), "window"),
                     (dict(postprocess=DevicePostprocess(tree, cmap, 0, {"tooth": dict(min_area=4)})), "postprocess")):
        with pytest.raises(ValueError, match=f"hedge together with {what} is not supported"):
            PE.Predictor(model, tree, cmap, args, hedge=hedge, **kw)
    with pytest.raises(ValueError, match="model_type 0"):
        PE.Predictor(model, tree, cmap, argparse.Namespace(img_size=64, model_type=0, model_select=1), hedge=hedge)


def test_predict_loop_hedge_option(small_model, tmp_path):
    from hrseg_amd import _lib
    from hrseg_amd import predictEval as PE
    from hrseg_amd.Data import DeviceAugment, DeviceBoundaryScore, Hedge
    from hrseg_amd.Data.loader import ragged_collate
    from hrseg_amd.Metrics import performance_metrics as PP
    from hrseg_amd.utils.hierarchy import get_classes
    model, tree, cmap = small_model
    size = 64
    rng = np.random.default_rng(103)
    vals = sorted(R.decode_ref.name2pix(cmap).values())
    data = []
    for i in range(3):
        img = _source(rng, 40 + 6 * i, 36 + 5 * i, 3 if i % 2 else 1)
        data.append((img, _blocky(rng, vals, img.shape[0], img.shape[1])))
    nc = get_classes(tree, full=True)
    args = argparse.Namespace(model_type=1, model_select=1, num_classes=nc, num_classes_full=nc, batch_size=2, img_size=size)
    aug = DeviceAugment(size, tree, cmap, 1, train=False)
    families = ["decode_hedged", "decode_labels", "score_labels", "score_calibration", "augment_image", None]

    def batches():
        for k in range(0, len(data), 2):
            dev = ragged_collate(data[k:k + 2]).to(aug.device)
            yield (*aug(dev), dev)

    def run(save, **kw):
        mets = [PP.Accuracy(), PP.Jaccardindex(), PP.DiceScore(), PP.Precision(), PP.Recall()]
        start = [_lib.launch_count(f) for f in families]
        res = PE.predict_loop(model, torch.device("cuda"), batches(), args, tree, *mets, save_dir=str(tmp_path / save), class_map=cmap,
                              score_sources=True, label_dir=str(tmp_path / save / "maps"), **kw)
        return res, [_lib.launch_count(f) - s for f, s in zip(families, start)], sorted(os.listdir(tmp_path / save))

    today, launches, files = run("today")
    assert launches[:2] == [0, 2] and "hedge" not in today and "metrics_hedge.csv" not in files
    none, launches_n, files_n = run("none", hedge=None)
    assert launches_n == launches and files_n == files and list(none) == list(today)
    hedge = Hedge(tree, cmap, 0.3)
    with_h, launches_h, files_h = run("with", hedge=hedge)
    assert launches_h == [2, 0] + launches[2:], "two batches: the hedged decode takes the plain one's place, nothing else changes"
    assert files_h == sorted(files + ["metrics_hedge.csv"]) and list(with_h) == list(today) + ["hedge"]
    assert with_h["performance"] == today["performance"], "the network-size metrics do not see the hedge"
    got = with_h["hedge"]
    assert got["pixels"] == sum(d[1].size for d in data) and got["rejected"] == 0 and got["nonfinite"] == 0
    assert sum(got["ended"].values()) == got["pixels"] and list(got["ended"]) == hedge.node_names
    with open(tmp_path / "with" / "metrics_hedge.csv") as f:
        rows = list(csv.reader(f))
    assert rows[0] == ["Row", "Pixels", "Share", "Abstained"]
    assert [r[0] for r in rows[1:]] == hedge.node_names + ["rejected", "nonfinite", "coverage@0", "coverage@1"]
    assert [int(r[1]) for r in rows[1:9]] == list(got["ended"].values())
    from PIL import Image
    written = set()
    for f in os.listdir(tmp_path / "with" / "maps"):
        with Image.open(tmp_path / "with" / "maps" / f) as im:
            written |= set(np.unique(np.array(im)).tolist())
    assert written <= set(hedge.value_names)
    mets = [PP.Accuracy(), PP.Jaccardindex(), PP.DiceScore(), PP.Precision(), PP.Recall()]
    with pytest.raises(ValueError, match="hedge needs label_dir or score_sources"):
        PE.predict_loop(model, torch.device("cuda"), batches(), args, tree, *mets, class_map=cmap, hedge=hedge)
    with pytest.raises(ValueError, match="hedge together with boundary is not supported"):
        PE.predict_loop(model, torch.device("cuda"), batches(), args, tree, *mets, class_map=cmap, score_sources=True, hedge=hedge,
                        boundary=DeviceBoundaryScore(tree, cmap))
