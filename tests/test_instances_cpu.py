"""Device instance scoring, the parts that need no GPU: the numpy reference (tests/instances_ref.py) against an independent
scipy.ndimage.label computation and hand-worked answers, the summary arithmetic, the table building, and the new entry
points' exports, workspace bound and refusals through the C ABI."""
import ctypes
import math

import numpy as np
import pytest

from tests import instances_ref as R
from tests.decode_harness import _tree

IDENT = np.arange(256, dtype=np.uint8)
PAIRS = IDENT.copy()                   # values 2k and 2k + 1 form one group (values 0..253), 254 and 255 are group 255
PAIRS[:254] = (np.arange(254) // 2).astype(np.uint8)
PAIRS[254:] = 255
ALL = np.ones(256, dtype=np.uint8)


def _things(*groups):
    t = np.zeros(256, dtype=np.uint8)
    t[list(groups)] = 1
    return t


# ------------------------------------------------------------------------------------------------- scipy cross-check
def _scipy_records(pred, gt, group, things, conn):
    """n_gt, n_pred, tp, sum_inter, sum_union per group through scipy.ndimage.label: one binary labelling per group and map,
    every overlapping pair tested"""
    ndi = pytest.importorskip("scipy.ndimage")
    structure = np.ones((3, 3), int) if conn == 8 else ndi.generate_binary_structure(2, 1)
    valid = group[gt] != 255
    out = np.zeros((256, 5), dtype=np.int64)
    for g in np.nonzero(things)[0].tolist():
        if g == 255:
            continue
        lp, n_pred = ndi.label((group[pred] == g) & valid, structure)
        lg, n_gt = ndi.label(group[gt] == g, structure)
        out[g, 0], out[g, 1] = n_gt, n_pred
        both = (lp > 0) & (lg > 0)
        keys, inter = np.unique(lp[both].astype(np.int64) * (n_gt + 1) + lg[both], return_counts=True)
        ap, ag = np.bincount(lp.reshape(-1), minlength=n_pred + 1), np.bincount(lg.reshape(-1), minlength=n_gt + 1)
        for key, n in zip(keys.tolist(), inter.tolist()):
            p, t = divmod(key, n_gt + 1)
            if 3 * n > ap[p] + ag[t]:
                out[g, 2] += 1
                out[g, 3] += n
                out[g, 4] += ap[p] + ag[t] - n
    return out


@pytest.mark.parametrize("conn", [4, 8])
def test_reference_agrees_with_scipy_label(conn):
    rng = np.random.default_rng(3)
    seen = 0
    for H, W in ((40, 57), (65, 131)):
        gt, boxes = R.rectangles(rng, H, W, 4)
        gt[rng.random((H, W)) < 0.02] = 6                          # specks of another group, some of them diagonal neighbours
        gt[5:9, 20:40] = 254                                        # a void band
        pred = R.perturbed(rng, (H, W), boxes, 5, salt=0.01, salt_values=(4, 6, 7, 255))
        things = _things(2, 3)                                      # PAIRS: values 4, 5 -> group 2; 6, 7 -> group 3
        got = R.score_pair(pred, gt, PAIRS, things, conn)["records"]
        want = _scipy_records(pred, gt, PAIRS, things, conn)
        assert np.array_equal(got[:, [R.N_GT, R.N_PRED, R.TP, R.SUM_INTER, R.SUM_UNION]], want)
        assert not got[[g for g in range(256) if g not in (2, 3)]].any(), "rows of groups that are no things stay zero"
        seen += int(want[:, 2].sum())
    assert seen >= 10


# ---------------------------------------------------------------------------------------------------------- hand cases
def _known_answers():
    """three true components of one row each (value 9 on 0) and a predicted one inside each: 2 of 4 pixels (IoU exactly 1/2),
    2 of 3 (2/3), 3 of 4 (3/4)"""
    gt, pred = np.zeros((7, 9), np.uint8), np.zeros((7, 9), np.uint8)
    gt[1, 1:5] = 9
    pred[1, 1:3] = 9
    gt[3, 2:5] = 9
    pred[3, 3:5] = 9
    gt[5, 4:8] = 9
    pred[5, 4:7] = 9
    return pred, gt


def test_known_answers_at_the_exact_boundary():
    pred, gt = _known_answers()
    r = R.score_pair(pred, gt, IDENT, _things(9), 8, thresholds=(750, 751, 0, 667))
    rec = r["records"][9]
    q23, q34 = (2 << 30) // 3, (3 << 30) // 4
    assert (q23, q34) == (715827882, 805306368)
    assert rec.tolist() == [3, 3, 2, q23 + q34, 5, 7, 1, 0, 0, 1], "IoU 1/2 does not match; 3/4 counts at 750, not at 751; 2/3 < 0.667"
    W = 9
    assert r["gmatch"][1, 1] == -1 and r["pmatch"][1, 1] == -1 and r["ginter"][1, 1] == 0
    assert r["gmatch"][3, 2] == 3 * W + 3 and r["pmatch"][3, 3] == 3 * W + 2 and r["ginter"][3, 2] == 2
    assert r["gmatch"][5, 4] == 5 * W + 4 and r["pmatch"][5, 4] == 5 * W + 4 and r["ginter"][5, 4] == 3
    assert (r["gmatch"] == -2).sum() == gt.size - 3 and (r["pmatch"] == -2).sum() == gt.size - 3
    assert not r["records"][0].any(), "the background is no thing here"
    # with every group a thing the background matches too: 63 - 11 true, 63 - 7 predicted pixels, 52 shared
    rec0 = R.score_pair(pred, gt, IDENT, ALL, 8)["records"][0]
    assert rec0.tolist() == [1, 1, 1, (52 << 30) // 56, 52, 56, 0, 0, 0, 0]


def test_void_cuts_and_removes_predicted_components():
    gt = np.full((5, 12), 4, np.uint8)
    gt[:, 5:7] = 254                                               # a void band through the middle (PAIRS: group 255)
    pred = np.zeros((5, 12), np.uint8)
    pred[1:3, 2:10] = 5                                            # crosses the band: two components of group 2
    pred[4, 5:7] = 5                                               # wholly in void: does not exist
    pred[0, 0] = 255                                               # outside the class map: no predicted component
    r = R.score_pair(pred, gt, PAIRS, _things(2), 8)
    assert r["records"][2, :3].tolist() == [2, 2, 0]
    assert np.array_equal(r["pm"][:, 5:7], np.full((5, 2), 254)) and r["pm"][0, 0] == 255


def test_no_component_appears_in_two_matches():
    rng = np.random.default_rng(11)
    gt, boxes = R.rectangles(rng, 65, 131, 7)
    pred = R.perturbed(rng, gt.shape, boxes, 7, salt=0.004, salt_values=(0, 7))
    r = R.score_pair(pred, gt, IDENT, ALL, 8)                       # (the reference asserts uniqueness while it matches)
    ps, gs = [p for p, _, _ in r["pairs"]], [g for _, g, _ in r["pairs"]]
    assert len(set(ps)) == len(ps) == len(set(gs)) >= 10
    pm, gm = r["pmatch"].reshape(-1), r["gmatch"].reshape(-1)
    for p, g, inter in r["pairs"]:
        assert pm[p] == g and gm[g] == p and r["ginter"].reshape(-1)[g] == inter
    assert (gm >= 0).sum() == (pm >= 0).sum() == len(ps)


# ------------------------------------------------------------------------------------------------------------- summary
def test_summary_arithmetic():
    from hrseg_amd import ops
    from hrseg_amd.Data.instances import summarize, summary_row
    assert ops.INSTANCE_FIELDS == R.FIELDS
    q = 1 << 30
    rec = np.zeros((2, 256, 10), dtype=np.int64)
    rec[0, 1] = [4, 5, 3, 2 * q + q // 2, 30, 40, 2, 1, 0, 0]       # tp 3, fp 2, fn 1; sum_iou 2.5
    rec[1, 1] = [1, 0, 0, 0, 0, 0, 0, 0, 0, 0]                     # a second image: one more missed object
    rec[0, 2] = [0, 2, 0, 0, 0, 0, 0, 0, 0, 0]                     # only inventions
    rec[0, 5] = [9, 9, 9, 9 * q, 90, 90, 9, 9, 0, 0]               # no thing: must not show
    s = summarize(rec, ["a", "b", "c", "d"], [1, 2, 3], [750, 900])
    assert list(s) == ["b", "c", "d", "all", "mean_pq"]
    b = s["b"]
    assert (b["n_gt"], b["n_pred"], b["tp"], b["fp"], b["fn"]) == (5, 5, 3, 2, 2)
    assert b["precision"] == 0.6 and b["recall"] == 0.6 and b["rq"] == 3 / 5 and b["sq"] == 2.5 / 3
    assert b["pq"] == pytest.approx(b["sq"] * b["rq"], rel=1e-15) and b["pq"] == 2.5 / 5 and b["mean_iou"] == 0.75
    assert b["tp_at"] == {0.75: 2, 0.9: 1}
    c = s["c"]
    assert (c["fp"], c["fn"], c["precision"], c["rq"], c["pq"]) == (2, 0, 0.0, 0.0, 0.0)
    assert math.isnan(c["recall"]) and math.isnan(c["sq"]) and math.isnan(c["mean_iou"])
    d = s["d"]
    assert d["n_gt"] == d["n_pred"] == 0 and all(math.isnan(d[k]) for k in ("precision", "recall", "rq", "sq", "pq", "mean_iou"))
    a = s["all"]
    assert (a["n_gt"], a["n_pred"], a["tp"], a["fp"], a["fn"]) == (5, 7, 3, 4, 2) and a["pq"] == 2.5 / 6
    assert s["mean_pq"] == (0.5 + 0.0) / 2, "the mean is over the groups with an object in either map"
    assert math.isnan(summarize(np.zeros((1, 256, 10), np.int64), ["a"], [0], [])["mean_pq"])
    assert summary_row(rec[0, 1], [])["tp_at"] == {}


def test_tables_and_refusals():
    from hrseg_amd.Data import DeviceInstanceScore, InstanceScores
    tree, cmap = _tree("tl")
    inst = DeviceInstanceScore(tree, cmap)
    assert inst.tables.names == ["background", "upper", "lower", "tooth"] and inst.thing_ids == [0, 1, 2, 3]
    assert inst.thresholds == [750, 900] and inst.tables.connectivity == 8 and sum(inst.things) == 4
    tooth = DeviceInstanceScore(tree, cmap, 0, ["tooth"], 4, (0.501, 1.0, 0.6666))
    assert tooth.thing_ids == [3] and tooth.thing_names == ["tooth"] and tooth.thresholds == [501, 1000, 667]
    assert tooth.things[3] == 1 and sum(tooth.things) == 1 and tooth.tables.connectivity == 4
    deep = DeviceInstanceScore(tree, cmap, 1, ["dentin", "upper"], thresholds=())
    assert [deep.tables.names[g] for g in deep.thing_ids] == ["upper", "dentin"] and deep.thresholds == []
    with pytest.raises((KeyError, ValueError)):
        DeviceInstanceScore(tree, cmap, things=["no such node"])
    with pytest.raises((KeyError, ValueError)):
        DeviceInstanceScore(tree, cmap, 0, things=["dentin"])       # in the tree, not in the cut at level 0
    with pytest.raises(ValueError, match="at most 4"):
        DeviceInstanceScore(tree, cmap, thresholds=(0.6, 0.7, 0.8, 0.9, 0.95))
    for bad in (0.5, 1.2, 0.5004, 0.0, -1.0):
        with pytest.raises(ValueError, match="threshold"):
            DeviceInstanceScore(tree, cmap, thresholds=(bad,))
    with pytest.raises(ValueError, match="connectivity"):
        DeviceInstanceScore(tree, cmap, connectivity=6)
    assert hasattr(InstanceScores, "cat") and hasattr(InstanceScores, "summary") and hasattr(InstanceScores, "instances")


def test_instance_scores_cat_and_summary_on_host_tensors():
    """cat and summary read nothing but `records`: host tensors stand in for the device's"""
    import torch
    from hrseg_amd.Data import DeviceInstanceScore, InstanceScores
    tree, cmap = _tree("tl")
    inst = DeviceInstanceScore(tree, cmap, things=["tooth", "upper"])
    a, b = torch.zeros((2, 256, 10), dtype=torch.int64), torch.zeros((1, 256, 10), dtype=torch.int64)
    a[0, 3, :3] = torch.tensor([2, 2, 1])
    a[1, 3, :3] = torch.tensor([1, 0, 0])
    b[0, 3, :3] = torch.tensor([3, 3, 3])
    b[0, 3, 3] = 3 << 29
    both = InstanceScores.cat([InstanceScores(a, inst), InstanceScores(b, inst)])
    assert len(both) == 3 and len(both.parts) == 2
    s = both.summary()
    assert list(s) == ["upper", "tooth", "all", "mean_pq"]
    assert (s["tooth"]["n_gt"], s["tooth"]["n_pred"], s["tooth"]["tp"]) == (6, 5, 4) and s["tooth"]["sq"] == 1.5 / 4
    assert all(s["all"][k] == s["tooth"][k] for k in ("n_gt", "n_pred", "tp", "fp", "fn", "rq", "sq", "pq"))
    assert s["mean_pq"] == s["tooth"]["pq"] == 1.5 / 5.5 and math.isnan(s["tooth"]["mean_iou"])


# --------------------------------------------------------------------------------------------------------------------- ABI
def _desc(*rows):
    return (ctypes.c_long * (4 * len(rows)))(*[v for r in rows for v in r])


def test_new_symbols_are_exported_and_the_abi_version_stays():
    import torch
    from hrseg_amd import _lib, ops
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("hrseg_mask_void_labels", "hrseg_score_instances", "hrseg_instances_workspace_bytes"):
        assert hasattr(lib, name), name
    assert _lib.abi_version() == 17
    assert _lib.launch_count("score_instances") >= 0, "the family is registered"
    total = _lib.launch_count()
    assert ops.SCORE_INSTANCES_LAUNCHES == ops.MASK_VOID_LABELS_LAUNCHES + ops.SCORE_INSTANCES_CALL_LAUNCHES == 5
    assert _lib.launch_count() == total
    # the workspace: at most 16 bytes per byte of the ground-truth buffer's extent plus a constant, whatever the prediction's
    for prow, grow in (([(0, 1, 1, 1)], [(0, 1, 1, 1)]), ([(0, 3, 33, 1), (500, 7, 64, 1)], [(5, 3, 33, 1), (200, 7, 64, 1)]),
                       ([(0, 1400, 2800, 1)] * 4, [(k * 1400 * 2800, 1400, 2800, 1) for k in range(4)]),
                       ([(1 << 40, 46340, 46340, 1)], [(0, 46340, 46340, 1)])):
        extent = max(off + H * W for off, H, W, _ in grow)
        got = _lib.instances_workspace_bytes(_desc(*(prow + grow)), len(prow))
        assert 12 * extent <= got <= 16 * extent + 64, (grow, got)
        assert got % 8 == 0
    ph = torch.tensor([[0, 50, 70, 1], [3500, 9, 31, 1]], dtype=torch.int64)
    gh = torch.tensor([[7, 50, 70, 1], [4000, 9, 31, 1]], dtype=torch.int64)
    assert ops.instances_workspace_bytes(ph, gh) == 12 * (4000 + 9 * 31) + 4
    with pytest.raises(RuntimeError, match="hrseg_instances_workspace_bytes: ground-truth image 0: bad descriptor"):
        _lib.instances_workspace_bytes(_desc((0, 1, 1, 1), (0, 0, 1, 1)), 1)
    with pytest.raises(RuntimeError, match="hrseg_instances_workspace_bytes: bad arguments"):
        _lib.instances_workspace_bytes(_desc((0, 1, 1, 1), (0, 1, 1, 1)), 0)
    assert ops.void_value(PAIRS.tolist()) == 255 and ops.void_value(list(range(256))) == 255 and ops.void_value([0] * 256) == -1
    # group[void_value] == 255 is the wrapper's check (the library sees device memory only): refused before any tensor is read
    for void, table in ((4, PAIRS.tolist()), (256, PAIRS.tolist()), (-2, PAIRS.tolist()), (-1, PAIRS.tolist()), (7, [0] * 256)):
        with pytest.raises(ValueError, match="mask_void_labels: void value"):
            ops.mask_void_labels(None, None, None, None, None, None, None, table, void=void)


def test_refusals_are_reported_without_a_gpu():
    """every refusal returns -1 with a message under the entry point's own name before anything is launched (placeholder
    pointers, never dereferenced; the descriptors' host copy and the thresholds are real host memory)"""
    from hrseg_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    lib.hrseg_last_error_string.restype = ctypes.c_char_p
    lib.hrseg_score_instances.argtypes = _lib.PROTOTYPES["hrseg_score_instances"]
    lib.hrseg_mask_void_labels.argtypes = _lib.PROTOTYPES["hrseg_mask_void_labels"]
    P = 1 << 20
    good = ((0, 4, 4, 1), (16, 4, 4, 1))

    def score(host=None, thr=(750, 0, 0, 0), B=1, no_host=False, no_thr=False, **over):
        a = dict(pm=P, pdesc=P, proots=P, parea=P, gt=P, gdesc=P, groots=P, garea=P, group=P, things=P, records=2 * P, pmatch=P,
                 gmatch=P, ginter=P, work=3 * P)
        a.update(over)
        host = _desc(*good) if host is None else host
        rc = lib.hrseg_score_instances(a["pm"], a["pdesc"], a["proots"], a["parea"], a["gt"], a["gdesc"], a["groots"], a["garea"],
                                       None if no_host else host, a["group"], a["things"], None if no_thr else _lib.int_array(list(thr)),
                                       a["records"], a["pmatch"], a["gmatch"], a["ginter"], a["work"], B, 1, None)
        return rc, lib.hrseg_last_error_string().decode()

    def mask(host=None, void=254, B=1, no_host=False, **over):
        a = dict(pred=P, pdesc=P, gt=P, gdesc=P, group=P, out=2 * P)
        a.update(over)
        host = _desc(*good) if host is None else host
        rc = lib.hrseg_mask_void_labels(a["pred"], a["pdesc"], a["gt"], a["gdesc"], None if no_host else host, a["group"], void, a["out"],
                                        B, None)
        return rc, lib.hrseg_last_error_string().decode()

    who = "hrseg_score_instances"
    for null in ("pm", "pdesc", "proots", "parea", "gt", "gdesc", "groots", "garea", "group", "things", "records", "pmatch", "gmatch",
                 "ginter", "work"):
        assert score(**{null: None}) == (-1, f"{who}: null pointer"), null
    assert score(no_host=True) == (-1, f"{who}: null pointer") and score(no_thr=True) == (-1, f"{who}: null pointer")
    for B in (0, -1, 65536):
        assert score(B=B) == (-1, f"{who}: B={B} not in 1..65535")
    for name in ("proots", "parea", "groots", "garea", "pmatch", "gmatch", "ginter"):
        for off in (1, 2):
            rc, msg = score(**{name: P + off})
            assert rc == -1 and msg.startswith(f"{who}: ") and "4-byte aligned" in msg, name
    for bad in (dict(records=2 * P + 4), dict(work=3 * P + 4), dict(work=3 * P + 1)):
        rc, msg = score(**bad)
        assert rc == -1 and msg.startswith(f"{who}: ") and "8-byte aligned" in msg, bad
    for k, t in ((0, 500), (1, 1001), (3, -1), (2, 1)):
        thr = [0, 0, 0, 0]
        thr[k] = t
        assert score(thr=thr) == (-1, f"{who}: thresholds[{k}]={t} is neither 0 nor in 501..1000")
    wm = "hrseg_mask_void_labels"
    for null in ("pred", "pdesc", "gt", "gdesc", "group", "out"):
        assert mask(**{null: None}) == (-1, f"{wm}: null pointer"), null
    assert mask(no_host=True) == (-1, f"{wm}: null pointer")
    for B in (0, 65536):
        assert mask(B=B) == (-1, f"{wm}: B={B} not in 1..65535")
    for v in (-2, 256):
        assert mask(void=v) == (-1, f"{wm}: void_value {v} is neither a byte nor -1")
    for out in (P, P + 15, P - 15):
        assert mask(out=out) == (-1, f"{wm}: out overlaps pred"), out
    # the descriptor rules of hrseg_label_components on either table, a size the tables disagree on: both entry points
    for fn, name in ((score, who), (mask, wm)):
        for row in ((-1, 4, 4, 1), (0, 0, 4, 1), (0, 4, 0, 1), (0, 4, 4, 3)):
            for host, what in ((_desc(row, good[1]), "predicted"), (_desc(good[0], row), "ground-truth")):
                rc, msg = fn(host=host)
                assert rc == -1 and msg.startswith(f"{name}: {what} image 0: bad descriptor"), (name, row, msg)
        big = (0, 1 << 16, 1 << 15, 1)
        rc, msg = fn(host=_desc(big, big))
        assert rc == -1 and msg.startswith(f"{name}: ") and "2^31 pixels or more" in msg
        two = _desc((0, 4, 4, 1), (16, 5, 6, 1), (0, 4, 4, 1), (16, 6, 5, 1))
        assert fn(host=two, B=2) == (-1, f"{name}: image 1: predicted map 5 x 6, ground truth 6 x 5")
