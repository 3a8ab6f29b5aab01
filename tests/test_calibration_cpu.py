"""Calibration scoring without a GPU: the oracle tests/calibration_ref.py against hand cases, the mover cap of every GPU
case on the oracle alone, the host-side metrics against a direct evaluation, and every refusal that happens before a
launch (C ABI, ops, Predictor)."""
import argparse
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import calibration_ref as R
from tests.decode_harness import _tree

Q = 1 << 24
TWO = ({"a": {}, "b": {"c": {}, "d": {}}}, {"a": 10, "c": 20, "d": 30})


def _metrics(ref, name):
    from hrseg_amd.Data.calibration import metrics_from_records
    return metrics_from_records(ref["hist"].sum(0)[ref["names"].index(name)])


def test_oracle_one_pixel():
    """1 x 1 logits -> a 1 x 1 image labelled 'pulp': every row's single event, worked out by hand"""
    tree, cmap = _tree("tl")
    z0, z1 = torch.tensor([0.5, -1.0, 2.0, 1.0]), torch.tensor([0.25, 0.0, -0.5, 1.5])
    ref = R.oracle([z0.reshape(1, 4, 1, 1), z1.reshape(1, 4, 1, 1)], tree, cmap, 1, [np.array([[127]], np.uint8)], 10)
    assert ref["names"] == ["background", "upper", "lower", "tooth", "pulp", "dentin", "enamel", "composite", "top@0", "top@1"]
    assert ref["ignored"].tolist() == [0]
    p0 = [1.0 / (1.0 + math.exp(-v)) for v in z0.tolist()]
    den = sum(math.exp(v) for v in z1.tolist())
    p1 = [p0[3] * math.exp(v) / den for v in z1.tolist()]
    # the path: lower (2.0) wins level 0 and is a leaf; the ground truth is tooth / pulp
    events = [(p, c == 3) for c, p in enumerate(p0)] + [(p, c == 0) for c, p in enumerate(p1)] + [(p0[2], False)]
    for r, (p, y) in enumerate(events):
        q = int(round(p * Q))
        e12 = ((Q - q if y else q) + 2048) >> 12
        want = np.zeros((11, 4), dtype=np.int64)
        want[min(9, (q * 10) >> 24)] = [1, int(y), q, e12 * e12]
        assert np.array_equal(ref["hist"][0, r], want), (r, p, y)
    assert not ref["hist"][0, 9].any(), "the path ends at level 0: no top-label event at level 1"
    unlabelled = R.oracle([z0.reshape(1, 4, 1, 1), z1.reshape(1, 4, 1, 1)], tree, cmap, 1, [np.array([[9]], np.uint8)], 10)
    assert unlabelled["ignored"].tolist() == [1] and not unlabelled["hist"].any()


def _two_level(gt_values):
    tree, cmap = TWO
    gt = np.array(gt_values, dtype=np.uint8).reshape(2, 2)
    return R.oracle([torch.zeros(1, 2, 2, 2), torch.zeros(1, 2, 2, 2)], tree, cmap, 1, [gt], 4)


def test_oracle_two_levels_by_hand():
    """all logits 0: P(a) = P(b) = 1/2, P(c) = P(d) = 1/4, the path is 'a' everywhere; labels a, a, a, c"""
    ref = _two_level([10, 10, 10, 20])
    assert ref["names"] == ["a", "b", "c", "d", "top@0", "top@1"]
    want = {"a": (0.75, 0.5, 0.25, 0.25), "b": (0.25, 0.5, 0.25, 0.25), "c": (0.25, 0.25, 0.0, (3 * 0.0625 + 0.5625) / 4),
            "d": (0.0, 0.25, 0.25, 0.0625), "top@0": (0.75, 0.5, 0.25, 0.25)}
    for name, (prev, conf, ece, brier) in want.items():
        m = _metrics(ref, name)
        assert (m["n"], m["prevalence"], m["mean_confidence"], m["ece"], m["mce"], m["brier"], m["nonfinite"]) == \
            (4, prev, conf, ece, ece, brier, 0), (name, m)
    top1 = _metrics(ref, "top@1")
    assert top1["n"] == 0 and all(math.isnan(top1[k]) for k in ("prevalence", "mean_confidence", "ece", "mce", "brier"))
    # the cells themselves: p = 1/2 opens bin 2 of 4, p = 1/4 bin 1
    assert ref["hist"][0, 0, 2].tolist() == [4, 3, 4 * (Q // 2), 3 * 2048 ** 2 + 2048 ** 2]
    assert ref["hist"][0, 2, 1].tolist() == [4, 1, 4 * (Q // 4), 3 * 1024 ** 2 + 3072 ** 2]


def test_oracle_perfectly_calibrated_case_has_zero_ece():
    """labels a, a, c, d: every row's accuracy equals its confidence, and the integers say so exactly"""
    ref = _two_level([10, 10, 20, 30])
    for name in ("a", "b", "c", "d", "top@0"):
        m = _metrics(ref, name)
        assert m["ece"] == 0.0 and m["mce"] == 0.0 and m["n"] == 4, (name, m)


@pytest.mark.parametrize("name", list(R.CASES))
def test_mover_cap_and_metrics_of_the_gpu_cases(name):
    """on the oracle alone: movers stay under 0.5 % of every row's events, so the GPU comparison cannot hide behind them;
    ECE / MCE / Brier from the integers equal a direct fp64 evaluation of the same events"""
    from hrseg_amd.Data.calibration import metrics_from_records
    ref = R.case_reference(name)
    share = R.mover_share(ref)
    print(f"{name}: band {ref['band']:.3e}, largest mover share {share:.5f}")
    assert share <= R.MOVER_CAP, (name, share)
    B = len(ref["events"])
    for r, row in enumerate(ref["names"]):
        p = np.concatenate([ref["events"][b][r]["p64"] for b in range(B)])
        y = np.concatenate([ref["events"][b][r]["y"] for b in range(B)])
        got = metrics_from_records(ref["hist"].sum(0)[r])
        assert got["n"] == p.size and got["nonfinite"] == 0
        if p.size == 0:
            assert math.isnan(got["ece"]) and math.isnan(got["brier"])
            continue
        want = R.metrics_direct(p, y, ref["n_bins"])
        for k in ("ece", "mce", "brier"):
            assert abs(got[k] - want[k]) <= 1e-12, (name, row, k, got[k], want[k])
        assert got["prevalence"] == float(y.sum()) / p.size


def test_nan_probability_goes_to_the_extra_bin():
    rec = np.zeros((5, 4), dtype=np.int64)
    R.bin_events(rec, [float("nan"), 0.3, float("nan")], [1, 0, 0], 4)
    assert rec[4].tolist() == [2, 1, 0, 0] and rec[1, 0] == 1 and rec[:, 0].sum() == 3
    from hrseg_amd.Data.calibration import metrics_from_records
    assert metrics_from_records(rec)["nonfinite"] == 2 and metrics_from_records(rec)["n"] == 1


def test_temperatures_on_the_host():
    from hrseg_amd.Data.calibration import DeviceCalibrationScore, inverse_temperatures
    assert inverse_temperatures(None, 2).tolist() == [1.0, 1.0] and inverse_temperatures(1.0, 3).tolist() == [1.0] * 3
    inv = inverse_temperatures((2.0, 3.0), 2)
    assert inv.dtype == np.float32 and inv.tolist() == [0.5, float(np.float32(1.0) / np.float32(3.0))]
    for bad in (0.0, -1.0, float("nan"), float("inf"), (1.0, 0.0), 1e-45):
        with pytest.raises(ValueError, match="temperature"):
            inverse_temperatures(bad, 2)
    with pytest.raises(ValueError, match="3 values for 2 levels"):
        inverse_temperatures((1.0, 2.0, 3.0), 2)
    tree, cmap = _tree("ext")
    cal = DeviceCalibrationScore(tree, cmap, 1, n_bins=7, temperature=2.0)
    assert cal.names[:2] == ["background", "tooth+alveolar"] and cal.names[-4:] == ["top@0", "top@1", "top@2", "top@3"]
    assert len(cal.names) == 11 + 4 and cal.inv_temp.tolist() == [0.5] * 4
    flat = DeviceCalibrationScore(tree, cmap, 0)
    assert flat.names == ["background", "upper", "lower", "composite", "pulp", "dentin", "enamel", "top@0"]
    assert flat.score_tables.path[212] == 2 and flat.score_tables.path[0] == 1 and flat.score_tables.path[9] == 0
    with pytest.raises(ValueError, match="n_bins=33"):
        DeviceCalibrationScore(tree, cmap, 1, n_bins=33)


def test_c_abi_refusals_need_no_gpu():
    """hrseg_score_calibration refuses before any launch, each time with its message (placeholder pointers, never read)"""
    from hrseg_amd import _lib, ops
    from hrseg_amd.Data.decode import build_tables
    lib = ctypes.CDLL(_lib.LIB_PATH)
    lib.hrseg_last_error_string.restype = ctypes.c_char_p
    fn = lib.hrseg_score_calibration
    fn.argtypes = _lib.PROTOTYPES["hrseg_score_calibration"]
    fn.restype = ctypes.c_int
    tree, cmap = _tree("tl")
    tables = build_tables(tree, cmap, 1)
    P = ctypes.c_void_p(4096)
    launched = _lib.launch_count("score_calibration")

    def refused(**over):
        a = dict(nlevels=2, z=(ctypes.c_void_p * 2)(4096, 4096), C=_lib.int_array([4, 4]), tree=ops._decode_tree_struct(tables),
                 inv=(ctypes.c_float * 2)(1.0, 1.0), gt=P, gdesc=P, lut=P, n_bins=15, hist=P, ignored=P, B=1, S=8)
        a.update(over)
        rc = fn(a["nlevels"], a["z"], a["C"], None if a["tree"] is None else ctypes.byref(a["tree"]), a["inv"], a["gt"], a["gdesc"],
                a["lut"], a["n_bins"], a["hist"], a["ignored"], a["B"], a["S"], 0, None)
        return rc, lib.hrseg_last_error_string().decode()

    for bad, want in ((dict(n_bins=0), "n_bins=0 not in 1..32"), (dict(n_bins=33), "n_bins=33 not in 1..32"),
                      (dict(inv=(ctypes.c_float * 2)(1.0, 0.0)), "inv_temp[1]=0 is not a finite positive number"),
                      (dict(inv=(ctypes.c_float * 2)(-2.0, 1.0)), "inv_temp[0]=-2 is not a finite positive number"),
                      (dict(inv=(ctypes.c_float * 2)(float("nan"), 1.0)), "inv_temp[0]=nan is not a finite positive number"),
                      (dict(inv=(ctypes.c_float * 2)(1.0, float("inf"))), "inv_temp[1]=inf is not a finite positive number"),
                      (dict(B=0), "B=0 not in 1..65535"), (dict(B=65536), "B=65536 not in 1..65535"), (dict(S=32769), "S=32769"),
                      (dict(gt=None), "null pointer"), (dict(hist=None), "null pointer"), (dict(ignored=None), "null pointer"),
                      (dict(lut=None), "null pointer"), (dict(gdesc=None), "null pointer"), (dict(inv=None), "null pointer"),
                      (dict(tree=None), "null pointer"), (dict(z=(ctypes.c_void_p * 2)(4096, None)), "level 1 has no logits"),
                      (dict(hist=ctypes.c_void_p(4100)), "8-byte aligned"), (dict(nlevels=9), "nlevels=9 not in 1..8"),
                      (dict(C=_lib.int_array([4, 17])), "C[1]=17 not in 1..16")):
        rc, msg = refused(**bad)
        assert rc == -1 and msg.startswith("hrseg_score_calibration: ") and want in msg, (bad, rc, msg)
    # a level-1 channel that no level-0 node owns: 'tooth' keeps three of the four children
    t = ops._decode_tree_struct(tables)
    t.n_children[0][3] = 3
    rc, msg = refused(tree=t)
    assert rc == -1 and msg == "hrseg_score_calibration: channel 3 of level 1 is in no child group", msg
    t.n_children[0][3], t.first_child[0][2], t.n_children[0][2] = 4, 3, 1
    rc, msg = refused(tree=t)
    assert rc == -1 and "channel 3 of level 1 is in the child groups of channels 2 and 3" in msg, msg
    assert _lib.launch_count("score_calibration") == launched, "a refused call launches nothing"


def test_ops_refusals_need_no_gpu():
    from hrseg_amd import ops
    from hrseg_amd.Data.calibration import flat_score_tables
    from hrseg_amd.Data.decode import build_tables
    from hrseg_amd.Data.score import build_score_tables
    tree, cmap = _tree("tl")
    tables, st = build_tables(tree, cmap, 1), build_score_tables(tree, cmap)
    ops.check_calibration_tables(tables, st)
    with pytest.raises(ValueError, match=r"decode tables have \[4, 4\] channels per level, the path table \[7\]"):
        ops.check_calibration_tables(tables, flat_score_tables(tree, cmap))
    tables.n_children[0][3] = 3
    with pytest.raises(ValueError, match="channel 3 of level 1 is in no child group"):
        ops.check_calibration_tables(tables, st)


def test_predictor_refuses_views_and_windows():
    from hrseg_amd import predictEval as PE
    tree, cmap = _tree("tl")
    args = argparse.Namespace(img_size=64, model_type=1, model_select=1)
    img = [np.zeros((8, 8), np.uint8)]
    with pytest.raises(ValueError, match="score_calibration: tta is set.*single-view"):
        PE.Predictor(None, tree, cmap, args, tta=PE.TestTimeAugment()).score_calibration(img, img)
    with pytest.raises(ValueError, match="score_calibration: window is set.*single-view"):
        PE.Predictor(None, tree, cmap, args, window=PE.SlidingWindow()).score_calibration(img, img)
