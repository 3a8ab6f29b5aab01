"""Device calibration scoring (csrc/calibration.hip, Data/calibration.py, predictEval) against the fp64 torch-CPU oracle
tests/calibration_ref.py by the one rule written there, plus exact integer identities that need no oracle: event counts,
the decode's arg-max through hrseg_score_labels' confusion counts, accumulation, reproducibility and NaN."""
import argparse
import csv
import os

import numpy as np
import pytest
import torch

from tests import calibration_ref as R
from tests.decode_harness import _source, _tree
from tests.helpers import build_model

pytestmark = pytest.mark.gpu

HIER = ["tl_ragged", "tl_wide", "ext_ragged", "ext_one_bin"]           # hierarchical cases at temperature 1


def _pack(maps, start, gap, fill):
    """maps -> (packed uint8 host buffer, [B,4] host descriptors): `start` bytes in front of the first map and `gap` bytes
    behind every map, all holding the leaf value `fill`: a read outside a span would be counted"""
    n = start + sum(m.size + gap for m in maps)
    buf = np.full(n, fill, dtype=np.uint8)
    rows, off = [], start
    for m in maps:
        buf[off:off + m.size] = m.reshape(-1)
        rows.append([off, m.shape[0], m.shape[1], 1])
        off += m.size + gap
    return torch.from_numpy(buf), torch.tensor(rows, dtype=torch.int64)


_INPUTS = {}


def _inputs(name):
    """(case, tree, class map, device logits, device ground-truth triple, the maps), uploaded once per case"""
    if name not in _INPUTS:
        case, tree, cmap, logits, gts = R.case_inputs(name)
        buf, host = _pack(gts, case["start"], case["gap"], 255)
        _INPUTS[name] = (case, tree, cmap, [z.cuda() for z in logits], (buf.cuda(), host.cuda(), host), gts)
    return _INPUTS[name]


def _scorer(name, **over):
    from hrseg_amd.Data import DeviceCalibrationScore
    case, tree, cmap = _inputs(name)[:3]
    kw = dict(n_bins=case["n_bins"], temperature=case["temperature"])
    kw.update(over)
    return DeviceCalibrationScore(tree, cmap, case["model_type"], **kw)


@pytest.mark.parametrize("name", list(R.CASES))
def test_against_the_oracle(name):
    case, _, _, logits, gt, gts = _inputs(name)
    ref = R.case_reference(name)
    scores = _scorer(name).score(logits, gt, per_image=True)
    assert scores.names == ref["names"] and len(scores) == len(gts)
    got = scores.hist.cpu().numpy()
    assert scores.ignored.tolist() == ref["ignored"].tolist()
    for b in range(len(gts)):
        R.compare(got[b], ref, [b], f"{name} image {b}")
    R.compare(got.sum(0), ref, range(len(gts)), f"{name} batch")


@pytest.mark.parametrize("name", list(R.CASES))
def test_event_counts_accumulation_and_reproducibility(name):
    case, _, _, logits, gt, gts = _inputs(name)
    cal = _scorer(name)
    per = cal.score(logits, gt, per_image=True)
    nodes = len(per.names) - len(cal.tables.C)
    n = per.hist[..., 0].sum(-1)                                     # [B, rows]: events per row, over all n_bins + 1 bins
    pixels = torch.tensor([m.size for m in gts], device=n.device)
    assert torch.equal(n[:, :nodes], (pixels - per.ignored)[:, None].expand(-1, nodes)), "one event per labelled pixel and node"
    assert bool((n[:, nodes:] <= (pixels - per.ignored)[:, None]).all()) and not bool(per.hist[:, :, -1, 2:].any())
    assert not bool(per.hist[:, :, -1].any()), "finite logits: nothing in the non-finite bin"
    batch = cal.score(logits, gt)
    assert batch.hist.shape[0] == 1 and torch.equal(per.hist.sum(0, keepdim=True), batch.hist)
    assert torch.equal(per.ignored.sum(0, keepdim=True), batch.ignored)
    assert torch.equal(per.total().hist, batch.hist) and torch.equal(per.total().ignored, batch.ignored)
    again = cal.score(logits, gt)
    assert torch.equal(again.hist, batch.hist) and torch.equal(again.ignored, batch.ignored), "two runs, the same bytes"
    twice = cal.score(logits, gt, out=again)
    assert twice is again and torch.equal(again.hist, 2 * batch.hist) and torch.equal(again.ignored, 2 * batch.ignored)
    if case["temperature"] is None:
        one = _scorer(name, temperature=1.0).score(logits, gt)
        assert torch.equal(one.hist, batch.hist), "temperature 1 changes no bit"


@pytest.mark.parametrize("name", HIER)
def test_positives_are_the_decodes_confusion_counts(name):
    """node-row positives = row sums of hrseg_score_labels' matrices, top-row positives = their (child levels: labelled)
    diagonals, for the maps hrseg_decode_labels makes of the same logits: this kernel's arg-max is the decode's, bit for bit"""
    from hrseg_amd.Data import DeviceDecode, DeviceScore
    case, tree, cmap, logits, gt, gts = _inputs(name)
    cal = _scorer(name)
    pos = cal.score(logits, gt).hist[0, :, :, 1].sum(-1)
    maps = DeviceDecode(tree, cmap, 1).decode_sizes(logits, [m.shape for m in gts])
    scores = DeviceScore(tree, cmap).score(maps, gt, per_image=False)
    row = 0
    nodes = sum(cal.tables.C)
    for L, C in enumerate(cal.tables.C):
        cm = scores.confusion(L)
        body = cm if L == 0 else cm[1:]
        assert torch.equal(pos[row:row + C], body.sum(1)), (name, L)
        diag = torch.diagonal(cm).sum() if L == 0 else torch.diagonal(cm)[1:].sum()
        assert int(pos[nodes + L]) == int(diag), (name, L, int(pos[nodes + L]), int(diag))
        row += C


def test_one_nan_logit_stays_loud():
    """NaN in one level-1 channel of image 0: its whole sibling group is NaN around the tap, in the oracle and on the device
    alike; those events are counted in the extra bin and nowhere else"""
    name = "tl_ragged"
    case, tree, cmap, logits, gt, gts = _inputs(name)
    _, _, _, host_logits, _ = R.case_inputs(name)
    host_logits[1][0, 2, 5, 5] = float("nan")
    ref = R.oracle(host_logits, tree, cmap, 1, gts, case["n_bins"])
    poisoned = [logits[0], host_logits[1].cuda()]
    clean = _scorer(name).score(logits, gt, per_image=True)
    scores = _scorer(name).score(poisoned, gt, per_image=True)
    got, nb = scores.hist.cpu().numpy(), case["n_bins"]
    want_nan = np.array([[int(np.isnan(ref["events"][b][r]["p64"]).sum()) for r in range(8)] for b in range(3)])
    want_pos = np.array([[int(ref["events"][b][r]["y"][np.isnan(ref["events"][b][r]["p64"])].sum()) for r in range(8)] for b in range(3)])
    assert want_nan[0, 4:].min() > 0 and not want_nan[0, :4].any() and not want_nan[1:].any()
    assert np.array_equal(got[:, :8, nb, 0], want_nan) and np.array_equal(got[:, :8, nb, 1], want_pos)
    assert not got[:, :, nb, 2:].any(), "a NaN event adds to no sum"
    assert torch.equal(scores.hist[..., 0].sum(-1)[:, :8], clean.hist[..., 0].sum(-1)[:, :8]), "and it is still an event"
    assert np.array_equal(got[:, :4], clean.hist.cpu().numpy()[:, :4]), "level 0 does not see it"
    # the path reaches level 1 where 'tooth' wins level 0, NaN or not, and T_1 is NaN for every member of the poisoned group
    top_nan = [int(np.isnan(ref["events"][b][9]["p64"]).sum()) for b in range(3)]
    assert got[:, 9, nb, 0].tolist() == top_nan and not got[:, 8, nb].any()
    summary = scores.summary()
    assert summary["pulp"]["nonfinite"] == int(want_nan[:, 4].sum()) > 0 and summary["background"]["nonfinite"] == 0
    assert summary["top@1"]["nonfinite"] == sum(top_nan)


def test_one_launch_and_the_host_side_views():
    from hrseg_amd import _lib
    name = "tl_wide"
    case, _, _, logits, gt, gts = _inputs(name)
    cal = _scorer(name)
    families = ["score_calibration", "score_labels", "decode_labels", "score_boundaries", "score_instances", "label_components",
                "filter_components", "augment_image", "augment_targets", "decode_views", "flip_views", "window_crops",
                "decode_windows", "ohem", None]
    start = [_lib.launch_count(f) for f in families]
    scores = cal.score(logits, gt, per_image=True)
    assert [_lib.launch_count(f) - s for f, s in zip(families, start)] == [1] + [0] * (len(families) - 1)
    ref = R.case_reference(name)
    summary = scores.summary()
    assert list(summary) == ref["names"] + ["ignored"] and summary["ignored"] == int(ref["ignored"].sum())
    from hrseg_amd.Data.calibration import metrics_from_records
    host = scores.hist.sum(0).cpu().numpy()
    for r, row in enumerate(ref["names"]):
        assert summary[row] == metrics_from_records(host[r])
    rel = scores.reliability("tooth")
    assert rel["edges"].tolist() == [k / 10 for k in range(11)] and rel["n"].tolist() == host[3, :10, 0].tolist()
    full = rel["n"] > 0
    assert np.array_equal(rel["accuracy"][full], host[3, :10, 1][full] / host[3, :10, 0][full])
    assert np.array_equal(rel["confidence"][full], host[3, :10, 2][full] / (2.0 ** 24 * host[3, :10, 0][full]))
    assert scores.reliability(3, image=0)["n"].tolist() == scores.hist[0, 3, :10, 0].tolist()
    sweep = cal.sweep(logits, gt, [1.0, (2.0, 0.5)])
    assert list(sweep) == [1.0, (2.0, 0.5)] and sweep[1.0] == cal.score(logits, gt).summary()
    assert sweep[(2.0, 0.5)] == _scorer(name, temperature=(2.0, 0.5)).score(logits, gt).summary() != sweep[1.0]
    with pytest.raises(ValueError, match="out must hold"):
        cal.score(logits, gt, out=scores, per_image=False)


@pytest.fixture(scope="module")
def small_model():
    from hrseg_amd.Models import models as PM
    tree, cmap = _tree("tl")
    return build_model(PM, "hrnet", True, tree, 64).cuda(), tree, cmap


def _blocky(rng, vals, H, W):
    m = rng.choice(np.asarray(vals, dtype=np.uint8), size=((H + 7) // 8, (W + 7) // 8))
    return np.ascontiguousarray(np.kron(m, np.ones((8, 8), np.uint8))[:H, :W])


def test_predictor_score_calibration(small_model):
    from hrseg_amd import predictEval as PE
    from hrseg_amd.Data import DeviceCalibrationScore
    model, tree, cmap = small_model
    rng = np.random.default_rng(89)
    vals = sorted(R.decode_ref.name2pix(cmap).values())
    imgs = [_source(rng, 50, 70, 3), _source(rng, 60, 100, 1), _source(rng, 64, 64, 3)]
    labels = [_blocky(rng, vals, 50, 70), _blocky(rng, vals, 60, 100), _blocky(rng, vals + [9], 33, 47)]
    args = argparse.Namespace(img_size=64, model_type=1, model_select=1)
    predictor = PE.Predictor(model, tree, cmap, args, keep_logits=True)
    scores = predictor.score_calibration(imgs, labels, per_image=True)
    logits = predictor.last_logits
    direct = DeviceCalibrationScore(tree, cmap, 1).score(logits, labels_triple(labels), per_image=True)
    assert torch.equal(scores.hist, direct.hist) and torch.equal(scores.ignored, direct.ignored)
    assert int(scores.ignored[2]) > 0 and scores.hist.shape == (3, 10, 16, 4)
    # (two forwards of one batch need not give the same bits -- the convolutions may add in another order -- so every call is
    # compared through the logits it kept)
    scorer = predictor.calibration_scorer
    total = predictor.score_calibration(imgs, labels)
    want = scorer.score(predictor.last_logits, labels_triple(labels))
    predictor.score_calibration(imgs, labels, out=total)
    scorer.score(predictor.last_logits, labels_triple(labels), out=want)
    assert predictor.calibration_scorer is scorer and torch.equal(total.hist, want.hist) and torch.equal(total.ignored, want.ignored)
    assert int(total.hist[0, 0, :, 0].sum()) == 2 * int(scores.hist[:, 0, :, 0].sum())
    cooled = predictor.score_calibration(imgs, labels, n_bins=10, temperature=2.0)
    assert predictor.calibration_scorer is not scorer and cooled.hist.shape == (1, 10, 11, 4)
    direct = DeviceCalibrationScore(tree, cmap, 1, 10, 2.0).score(predictor.last_logits, labels_triple(labels))
    assert torch.equal(cooled.hist, direct.hist)


def labels_triple(labels):
    from hrseg_amd.Data.decode import pack_images
    buf, host = pack_images(labels)
    return buf, host, host


def test_predict_loop_calibration_option(small_model, tmp_path):
    from hrseg_amd import _lib
    from hrseg_amd import predictEval as PE
    from hrseg_amd.Data import DeviceAugment, DeviceCalibrationScore
    from hrseg_amd.Data.loader import ragged_collate
    from hrseg_amd.Metrics import performance_metrics as PP
    from hrseg_amd.utils.hierarchy import get_classes
    model, tree, cmap = small_model
    size = 64
    rng = np.random.default_rng(97)
    vals = sorted(R.decode_ref.name2pix(cmap).values())
    data = []
    for i in range(3):
        img = _source(rng, 40 + 6 * i, 36 + 5 * i, 3 if i % 2 else 1)
        data.append((img, _blocky(rng, vals, img.shape[0], img.shape[1])))
    nc = get_classes(tree, full=True)
    args = argparse.Namespace(model_type=1, model_select=1, num_classes=nc, num_classes_full=nc, batch_size=2, img_size=size)
    aug = DeviceAugment(size, tree, cmap, 1, train=False)
    families = ["score_calibration", "score_instances", "score_boundaries", "score_labels", "decode_labels", "label_components",
                "filter_components", "augment_image", "augment_targets", "decode_views", None]

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
    assert launches[0] == 0 and "calibration" not in today and "metrics_calibration.csv" not in files
    cal = DeviceCalibrationScore(tree, cmap, 1, n_bins=10)
    with_c, launches_c, files_c = run("with", calibration=cal)
    none, launches_n, files_n = run("none", calibration=None)
    assert launches_n == launches and files_n == files and list(none) == list(today)
    assert launches_c == [2] + launches[1:], "two batches: one launch each, nothing else changes"
    assert files_c == sorted(files + ["metrics_calibration.csv"]) and list(with_c) == list(today) + ["calibration"]
    assert with_c["source"] == today["source"] and with_c["performance"] == today["performance"]
    # the same figures from the predictor's route, batch by batch into one total.  Two forwards of one batch need not give
    # the same bits (the convolutions may add in another order, logits move by a few ulp): what depends on the labels alone is
    # equal, the means move by far less than 1e-5, and an event that changes its bin moves the ECE by 1 / n at most
    predictor, total = PE.Predictor(model, tree, cmap, args), None
    for k in (0, 2):
        total = predictor.score_calibration([d[0] for d in data[k:k + 2]], [d[1] for d in data[k:k + 2]], n_bins=10, out=total)
    got = with_c["calibration"]
    want = total.summary()
    assert list(got) == list(want) and got["ignored"] == want["ignored"] == 0
    for name in cal.names[:8]:
        assert (got[name]["n"], got[name]["prevalence"], got[name]["nonfinite"]) == \
            (want[name]["n"], want[name]["prevalence"], 0), name
        assert abs(got[name]["mean_confidence"] - want[name]["mean_confidence"]) < 1e-5, name
        assert abs(got[name]["brier"] - want[name]["brier"]) < 1e-5 and abs(got[name]["ece"] - want[name]["ece"]) < 1e-3, name
    assert got["background"]["n"] == sum(d[1].size for d in data)
    with open(tmp_path / "with" / "metrics_calibration.csv") as f:
        rows = list(csv.reader(f))
    assert rows[0] == ["Row", "Events", "Prevalence", "MeanConfidence", "ECE", "MCE", "Brier", "NonFinite"]
    assert [r[0] for r in rows[1:]] == cal.names + ["ignored"]
    for r in rows[1:-1]:
        assert int(r[1]) == got[r[0]]["n"] and int(r[7]) == 0
        assert r[4] == ("" if got[r[0]]["ece"] != got[r[0]]["ece"] else str(got[r[0]]["ece"]))
        assert r[6] == ("" if got[r[0]]["brier"] != got[r[0]]["brier"] else str(got[r[0]]["brier"]))
    with pytest.raises(ValueError, match="calibration needs score_sources"):
        mets = [PP.Accuracy(), PP.Jaccardindex(), PP.DiceScore(), PP.Precision(), PP.Recall()]
        PE.predict_loop(model, torch.device("cuda"), batches(), args, tree, *mets, class_map=cmap, calibration=cal)
