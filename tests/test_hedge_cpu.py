"""Hedged decode, the parts that need no GPU: the fp64 oracle (tests/hedge_ref.py) on hand-computed pixels and its
monotonicity, the policy object Data.Hedge (tables, auto-assignment, refusals, the fit from calibration records), the score
tables with internal values, the C entry point's refusals, HedgedLabels.summary, and the exempt share of every GPU case."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import hedge_ref as R
from tests.decode_harness import MASK_CAP, _tree, _wide_tree

TWO = ({"bg": {}, "fg": {"a": {}, "b": {}}}, {"bg": 0, "a": 100, "b": 200})


def _sig(v):
    return 1.0 / (1.0 + math.exp(-v))


def _one_pixel(tree, cmap, levels, thresholds, **kw):
    logits = [torch.tensor(v, dtype=torch.float32).reshape(-1, 1, 1) for v in levels]
    s = R.hedge_sample(logits, tree, cmap, 1, 1, thresholds, **kw)
    return int(s["label"][0, 0]), float(s["conf"][0, 0]), int(s["stop"][0, 0])


def test_one_pixel_on_both_sides_of_a_threshold():
    """two levels: fg wins level 0 with sigmoid(2), a wins its group with e / (e + 1): T_1 = 0.8808 * 0.7311 = 0.6439"""
    tree, cmap = TWO
    t0, t1 = _sig(2.0), _sig(2.0) * math.e / (math.e + 1.0)
    assert abs(t1 - 0.6439) < 1e-4
    label, conf, stop = _one_pixel(tree, cmap, [[-1.0, 2.0], [1.0, 0.0]], 0.6)
    assert (label, stop) == (100, 2) and abs(conf - t1) < 1e-12                     # T_1 >= 0.6: the leaf a, cell of (1, 0)
    label, conf, stop = _one_pixel(tree, cmap, [[-1.0, 2.0], [1.0, 0.0]], 0.7)
    assert (label, stop) == (1, 1) and abs(conf - t0) < 1e-12                       # T_1 < 0.7: fg's byte (smallest unused), T_0
    label, conf, stop = _one_pixel(tree, cmap, [[-1.0, 2.0], [1.0, 0.0]], {"a": 0.7}, internal={"fg": 33})
    assert (label, stop) == (33, 1)
    label, conf, stop = _one_pixel(tree, cmap, [[-1.0, 2.0], [1.0, 0.0]], {"b": 0.99})
    assert (label, stop) == (100, 2), "the threshold of the node that is entered counts, not its sibling's"
    label, conf, stop = _one_pixel(tree, cmap, [[2.0, -1.0], [1.0, 0.0]], 0.99)
    assert (label, stop) == (0, 0) and abs(conf - t0) < 1e-12                       # a level-0 leaf: level 0 has no threshold
    label, conf, stop = _one_pixel(tree, cmap, [[-1.0, 2.0], [float("nan"), 0.0]], 0.99)
    assert label in (100, 200) and math.isnan(conf), "a NaN confidence is not below a threshold: the walk goes on"


def test_the_extended_tree_stops_at_healthy():
    tree, cmap = _tree("ext")
    levels = [[-3.0, 3.0], [-2.0, 2.0], [0.0, 0.0, 0.0, 3.0], [0.125, 0.0, 0.0]]
    t1 = _sig(3.0) * _sig(4.0)                       # tooth against alveolar: softmax([-2, 2])[1] = sigmoid(4)
    t2 = t1 * _sig(3.0)                              # healthy against composite: softmax([0, 3])[1]
    t3 = t2 * math.exp(0.125) / (math.exp(0.125) + 2.0)
    assert t2 > 0.5 > t3
    names, _, byte, _ = R.resolve(tree, cmap, 0.5)
    label, conf, stop = _one_pixel(tree, cmap, levels, 0.5)
    assert label == byte["healthy"] and abs(conf - t2) < 1e-12 and stop == 2 + 2 + 3
    assert [byte[n] for n in ("tooth+alveolar", "alveolar", "tooth", "healthy")] == [1, 2, 3, 4], "breadth-first, smallest unused"
    label, conf, stop = _one_pixel(tree, cmap, levels, 0.3)
    assert label == 127 and abs(conf - t3) < 1e-12 and stop == 8                    # pulp
    label, conf, stop = _one_pixel(tree, cmap, levels, [0.0, 0.95, 0.0, 0.0])
    assert label == byte["tooth+alveolar"] and abs(conf - _sig(3.0)) < 1e-12 and stop == 1


def test_level_0_rejection():
    tree, cmap = _tree("tl")
    levels = [[0.125, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0]]
    label, conf, stop = _one_pixel(tree, cmap, levels, [0.6, 0.0], reject=9)
    assert (label, stop) == (9, 8) and abs(conf - _sig(0.125)) < 1e-12
    label, conf, stop = _one_pixel(tree, cmap, levels, [0.5, 0.0], reject=9)
    assert (label, stop) == (0, 0)


@pytest.mark.parametrize("name", ["tl_scalar_ragged", "ext_scalar_ragged", "wide_scalar_ragged"])
def test_raising_a_threshold_moves_labels_to_ancestors_only(name):
    case, tree, cmap, logits = R.case_inputs(name)
    names = R.resolve(tree, cmap, 0.0)[0]
    cell0 = np.concatenate([[0], np.cumsum([len(n) for n in names])])
    depth = torch.from_numpy(np.concatenate([np.repeat(np.arange(len(names)), [len(n) for n in names]), [-1, -1]]))
    moved = 0
    for b, (H, W) in enumerate(case["sizes"]):
        zb = [z[b] for z in logits]
        lo, hi = (R.hedge_sample(zb, tree, cmap, H, W, t) for t in (0.3, 0.7))
        plain = R.hedge_sample(zb, tree, cmap, H, W, 0.0)
        assert torch.equal(plain["label"], R.decode_ref.decode_sample(zb, tree, cmap, 1, H, W)[0]), "no threshold: the plain decode"
        d_lo, d_hi = depth[lo["stop"]], depth[hi["stop"]]
        assert bool((d_hi <= d_lo).all()) and bool((d_lo <= depth[plain["stop"]]).all())
        on_path = torch.zeros(H, W, dtype=torch.bool)
        for nb in lo["nodes"]:
            on_path |= hi["label"].long() == nb
        assert bool(on_path.all()), "the label under the higher threshold is a node of the same path"
        assert bool(((d_hi == d_lo) == (hi["label"] == lo["label"])).all())
        moved += int((d_hi < d_lo).sum())
    assert moved > 0 and int(cell0[-1]) == sum(len(n) for n in names)


# ------------------------------------------------------------------------------------------------------------ the policy object
def test_hedge_tables_and_auto_assignment():
    from hrseg_amd.Data import Hedge
    tree, cmap = _tree("ext")
    h = Hedge(tree, cmap, 0.5)
    assert h.tau == [[0.0, 0.0], [0.5, 0.5], [0.5] * 4, [0.5] * 3] and h.reject_val == -1
    assert h.values == {"tooth+alveolar": 1, "alveolar": 2, "tooth": 3, "healthy": 4}
    assert h.stop_val == [[-1, 1], [2, 3], [-1, -1, -1, 4], [-1, -1, -1]]
    assert h.node_names[:4] == ["background", "tooth+alveolar", "alveolar", "tooth"] and h.unmet_levels == []
    h = Hedge(tree, cmap, [0.25, 0.5, 0.0, 1.0], internal_values={"tooth": 1, "healthy": 250}, reject_value=2)
    assert h.values == {"tooth+alveolar": 3, "alveolar": 4, "tooth": 1, "healthy": 250} and h.reject_val == 2
    assert h.tau[0] == [0.25, 0.25] and h.tau[3] == [1.0] * 3
    assert h.value_names[2] == "rejected" and h.value_names[250] == "healthy" and h.value_names[127] == "pulp"
    h = Hedge(tree, cmap, {"enamel": 0.75, "tooth": 0.5})
    assert h.tau == [[0.0, 0.0], [0.0, 0.5], [0.0] * 4, [0.0, 0.0, 0.75]]
    tl, tlmap = _tree("tl")
    assert Hedge(tl, tlmap, 0.5).values == {"tooth": 1}
    wide, wmap = _wide_tree()
    assert Hedge(wide, wmap, 0.5, reject_value=1).values == {"group0": 2, "group1": 3, "group2": 4}


def test_hedge_refusals_name_the_nodes():
    from hrseg_amd.Data import Hedge
    tree, cmap = _tree("tl")
    for bad, match in ((dict(thresholds=1.5), "threshold 1.5 of 'pulp' is not in 0..1"),
                       (dict(thresholds=float("nan")), "threshold nan of 'pulp' is not in 0..1"),
                       (dict(thresholds={"enamel": -0.1}), "threshold -0.1 of 'enamel'"),
                       (dict(thresholds={"molar": 0.5}), "threshold for 'molar', which is no node"),
                       (dict(thresholds=[0.5]), "1 per-level thresholds for 2 levels"),
                       (dict(thresholds=[0.5, 0.5]), "'background' has the level-0 threshold 0.5, but there is no reject value"),
                       (dict(thresholds=0.5, internal_values={"tooth": 256}), "internal node 'tooth' has the stop value 256"),
                       (dict(thresholds=0.5, internal_values={"tooth": 85}), "'tooth' and 'enamel' share the byte 85"),
                       (dict(thresholds=0.5, internal_values={"tooth": 212}), "'upper' and 'tooth' share the byte 212"),
                       (dict(thresholds=0.5, internal_values={"enamel": 3}), "internal value for 'enamel', which is a leaf"),
                       (dict(thresholds=0.5, internal_values={"molar": 3}), "internal value for 'molar', which is no node"),
                       (dict(thresholds=0.5, reject_value=300), "reject value 300 not in -1..255"),
                       (dict(thresholds=0.5, reject_value=0), "the reject value and 'background' share the byte 0"),
                       (dict(thresholds=0.5, internal_values={"tooth": 9}, reject_value=9), "the reject value and 'tooth' share the byte 9")):
        with pytest.raises(ValueError, match=match):
            Hedge(tree, cmap, **bad)
    from hrseg_amd import ops
    from hrseg_amd.Data.decode import build_tables
    h = Hedge(tree, cmap, 0.5)
    h.tables = build_tables(tree, cmap, 0)
    with pytest.raises(ValueError, match="model_type 0"):
        ops.check_hedge(h)


def _records(n_bins, rows):
    """{row name: [(n, pos) per bin]} -> a CalibrationScores on the host (sum_q / sum_e2 are not read by the fit)"""
    from hrseg_amd.Data import CalibrationScores
    names = ["background", "upper", "lower", "tooth", "pulp", "dentin", "enamel", "composite", "top@0", "top@1"]
    hist = torch.zeros(2, len(names), n_bins + 1, 4, dtype=torch.int64)
    for name, bins in rows.items():
        for k, (n, pos) in enumerate(bins):
            hist[k % 2, names.index(name), k, 0] = n                                   # spread over two records: the fit sums them
            hist[k % 2, names.index(name), k, 1] = pos
    return CalibrationScores(hist, torch.zeros(2, dtype=torch.int64), names, n_bins)


def test_from_calibration_on_hand_made_records():
    from hrseg_amd.Data import Hedge
    tree, cmap = _tree("tl")
    # top@1, 5 bins (n, pos): tails from bin k: k=0 (100, 64), k=1 (90, 62), k=2 (70, 55), k=3 (40, 36), k=4 (10, 10)
    scores = _records(5, {"top@1": [(10, 2), (20, 7), (30, 19), (30, 26), (10, 10)], "top@0": [(50, 0)] * 5})
    fit = lambda acc, **kw: Hedge.from_calibration(scores, tree, cmap, acc, **kw)          # noqa: E731
    h = fit(0.6)
    assert h.tau == [[0.0] * 4, [0.0] * 4] and h.unmet_levels == []                        # 64 / 100 already qualifies
    assert fit(0.65).tau[1] == [0.2] * 4                                                    # 62 / 90 = 0.689
    assert fit(0.75).tau[1] == [0.4] * 4                                                    # 55 / 70 = 0.786
    assert fit(0.9).tau[1] == [0.6] * 4                                                     # 36 / 40 = 0.9: >= counts
    assert fit(0.95).tau[1] == [0.8] * 4
    assert fit(0.95, min_events=11).tau[1] == [1.0] * 4 and fit(0.95, min_events=11).unmet_levels == [1]
    assert fit(0.9, min_events=41).unmet_levels == [1]
    h = fit(0.75, internal_values={"tooth": 77}, reject_value=5)
    assert h.values == {"tooth": 77} and h.reject_val == 5 and h.tau[0] == [0.0] * 4, "level 0 is never fitted"
    empty = _records(5, {})
    assert Hedge.from_calibration(empty, tree, cmap, 0.5).unmet_levels == [1]
    with pytest.raises(ValueError, match="min_accuracy"):
        fit(1.5)


# ------------------------------------------------------------------------------------------------------------ score tables
def test_score_tables_with_internal_values():
    from hrseg_amd import ops
    from hrseg_amd.Data import Hedge, build_score_tables
    tree, cmap = _tree("ext")
    plain = build_score_tables(tree, cmap)
    assert build_score_tables(tree, cmap, None).path == plain.path == build_score_tables(tree, cmap, {}).path
    h = Hedge(tree, cmap, 0.5)
    t = build_score_tables(tree, cmap, h.values)
    ops.check_score_tables(t)
    # byte L of an entry = 1 + the channel of the level-L node on the way; zero below the node the byte stands for
    assert t.path[1] == 2                                            # tooth+alveolar: level 0 channel 1
    assert t.path[2] == 2 | (1 << 8)                                 # alveolar: (0, 1) -> (1, 0)
    assert t.path[3] == 2 | (2 << 8)                                 # tooth: (0, 1) -> (1, 1)
    assert t.path[4] == 2 | (2 << 8) | (4 << 16)                     # healthy: ... -> (2, 3)
    assert t.path[85] == 2 | (2 << 8) | (4 << 16) | (3 << 24) == plain.path[85]       # enamel goes through healthy
    assert [v for v in range(256) if t.path[v] != plain.path[v]] == [1, 2, 3, 4]
    assert (t.C, t.K, t.total) == (plain.C, plain.K, plain.total)
    for bad, match in (({"tooth": 85}, "'enamel' and 'tooth' share the pixel value 85"), ({"enamel": 9}, "no internal node"),
                       ({"tooth": 256}, "does not fit a uint8"), ({"tooth": 9, "healthy": 9}, "share the pixel value 9")):
        with pytest.raises(ValueError, match=match):
            build_score_tables(tree, cmap, bad)


# ------------------------------------------------------------------------------------------------------------ the C entry point
def test_c_entry_point_refusals_without_a_gpu():
    """every refusal of hrseg_decode_hedged, before anything is launched (placeholder pointers, never dereferenced; every
    call has exactly one defect, or the one named first where the order is stated)"""
    from hrseg_amd import _lib, ops
    from hrseg_amd.Data import Hedge
    from hrseg_amd.Data.decode import build_tables
    lib = ctypes.CDLL(_lib.LIB_PATH)
    lib.hrseg_last_error_string.restype = ctypes.c_char_p
    lib.hrseg_decode_hedged.argtypes = _lib.PROTOTYPES["hrseg_decode_hedged"]
    tree, cmap = _tree("tl")
    good = Hedge(tree, cmap, 0.5, reject_value=9)
    P = 4096

    def refused(hedge=None, edit=None, tree_edit=None, nlevels=2, C=(4, 4), z=(P, P), labels=P, conf=None, stops=P, B=2, S=32):
        h = ops._hedge_struct(hedge or good)
        t = ops._decode_tree_struct((hedge or good).tables)
        if edit:
            edit(h)
        if tree_edit:
            tree_edit(t)
        zs = (ctypes.c_void_p * 8)(*z)
        rc = lib.hrseg_decode_hedged(nlevels, zs, _lib.int_array(list(C)), ctypes.byref(t), ctypes.byref(h), P, labels, conf, stops,
                                     B, S, None)
        assert rc == -1
        return lib.hrseg_last_error_string().decode()

    def put(field, L, c, v):
        def edit(h):
            getattr(h, field)[L][c] = v
        return edit

    def reject(v):
        def edit(h):
            h.reject_val = v
        return edit

    # the limits and alignment rules of hrseg_decode_labels, under this entry point's name
    assert "hrseg_decode_hedged: bad arguments" in refused(B=0)
    assert "hrseg_decode_hedged: bad arguments" in refused(S=40000)
    assert "hrseg_decode_hedged: nlevels=9 not in 1..8" in refused(nlevels=9)
    assert "hrseg_decode_hedged: C[1]=17 not in 1..16" in refused(C=(4, 17))
    assert "hrseg_decode_hedged: labels must be 4-byte and confidence 16-byte aligned" in refused(labels=P + 2)
    assert "hrseg_decode_hedged: labels must be 4-byte and confidence 16-byte aligned" in refused(conf=P + 8)
    assert "hrseg_decode_hedged: level 1 has no logits" in refused(z=(P, None))

    def no_children(t):
        t.n_children[0][3] = 5
    assert "are not channels of the next level" in refused(tree_edit=no_children)

    def flat(t):
        t.root_softmax = 1
    assert "root_softmax is set: a flat model has no path to shorten" in refused(tree_edit=flat)
    # the hedge table
    assert "tau of (level 1, channel 2) is 1.5, not in 0..1" in refused(edit=put("tau", 1, 2, 1.5))
    assert "tau of (level 1, channel 0) is -0.25, not in 0..1" in refused(edit=put("tau", 1, 0, -0.25))
    assert "tau of (level 0, channel 1) is nan, not in 0..1" in refused(edit=put("tau", 0, 1, float("nan")))
    assert "internal node (level 0, channel 3) has stop value 256" in refused(edit=put("stop_val", 0, 3, 256))
    assert "internal node (level 0, channel 3) has stop value -1" in refused(edit=put("stop_val", 0, 3, -1))
    assert "reject_val=256 not in -1..255" in refused(edit=reject(256))
    assert "reject_val=-2 not in -1..255" in refused(edit=reject(-2))
    with_level0 = Hedge(tree, cmap, [0.5, 0.5], reject_value=9)
    assert "reject_val=-1 (no rejection), but (level 0, channel 0) has the threshold 0.5" in refused(with_level0, edit=reject(-1))
    assert "(level 0, channel 3) and (level 1, channel 2) share the byte 85" in refused(edit=put("stop_val", 0, 3, 85))
    assert "(level 0, channel 1) and (level 0, channel 3) share the byte 212" in refused(edit=put("stop_val", 0, 3, 212))
    assert "(level 0, channel 0) and reject_val share the byte 0" in refused(edit=reject(0))
    assert "(level 0, channel 3) and reject_val share the byte 9" in refused(edit=put("stop_val", 0, 3, 9))

    def two_leaves(t):
        t.pixel_val[1][1] = 127
    assert "(level 1, channel 0) and (level 1, channel 1) share the byte 127" in refused(tree_edit=two_leaves)
    assert "stops must be 8-byte aligned" in refused(stops=P + 4)
    # entries beyond the tree's channels are not read
    assert "stops must be 8-byte aligned" in refused(edit=put("tau", 1, 9, 7.0), stops=P + 4)
    assert "stops must be 8-byte aligned" in refused(edit=put("tau", 5, 0, 7.0), stops=P + 4)
    # and the host wrapper mirrors them with names (no GPU either)
    bad = Hedge(tree, cmap, 0.5)
    bad.tau[1][2] = 2.0
    with pytest.raises(ValueError, match="threshold 2.0 of 'enamel'"):
        ops.check_hedge(bad)
    assert build_tables(tree, cmap, 1).names == good.tables.names


# ------------------------------------------------------------------------------------------------------------ summary
def test_summary_of_hand_made_counters():
    from hrseg_amd.Data import HedgedLabels, Hedge
    tree, cmap = _tree("ext")
    h = Hedge(tree, cmap, [0.5, 0.5, 0.5, 0.5], reject_value=9)
    # cells: background, tooth+alveolar | alveolar, tooth | upper, lower, composite, healthy | pulp, dentin, enamel | rejected, nonfinite
    stops = torch.tensor([[40, 5, 3, 4, 6, 2, 8, 7, 1, 2, 2, 20, 3], [0] * 13], dtype=torch.int64)
    s = HedgedLabels(None, None, None, None, stops, h).summary()
    assert s["pixels"] == 100 and s["rejected"] == 20 and s["nonfinite"] == 3
    assert s["ended"]["background"] == 40 and s["ended"]["healthy"] == 7 and list(s["ended"]) == h.node_names
    assert s["abstained"] == {"tooth+alveolar": 5 / 40, "alveolar": 3 / 11, "tooth": 4 / 24, "healthy": 7 / 12}
    assert s["coverage"] == [1 - 20 / 100, 1 - 25 / 100, 1 - 32 / 100, 1 - 39 / 100]
    empty = HedgedLabels(None, None, None, None, torch.zeros(1, 13, dtype=torch.int64), h).summary()
    assert empty["pixels"] == 0 and all(math.isnan(v) for v in empty["abstained"].values()) and math.isnan(empty["coverage"][0])


# ------------------------------------------------------------------------------------------------------------ the GPU cases
@pytest.mark.parametrize("name", list(R.CASES))
def test_exempt_share_of_every_gpu_case_stays_under_the_cap(name):
    ref = R.case_reference(name)
    share = R.exempt_share(ref)
    stops = torch.cat([s["stop"].reshape(-1) for s in ref["samples"]])
    cells = ref["samples"][0]["cells"]
    hist = torch.bincount(stops, minlength=cells)
    print(f"{name}: exempt share {share:.5f}, band {ref['band']:.3e} (torch-CPU fp32 {ref['d32']:.3e}), cells {hist.tolist()}")
    assert share <= MASK_CAP
    case, tree, cmap, _ = R.case_inputs(name)
    names, _, byte, reject = R.resolve(tree, cmap, case["thresholds"], case["internal"], case["reject"])
    kids = {n: k for lvl in R.decode_ref.bfs_levels(tree) for n, k in lvl}
    internal = [i for i, n in enumerate(n for lvl in names for n in lvl) if kids[n]]
    assert int(hist[internal].sum()) > 0, "the case hedges somewhere"
    assert (reject is None) == (int(hist[cells - 2]) == 0), "and rejects where it has a reject value"
