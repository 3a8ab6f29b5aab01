"""Device scoring pipeline, the parts that need no GPU: the numpy reference (tests/score_ref.py) pinned against the
oracle's train-loop masking and against hand-computed answers, its invariants, the path tables of
Data.score.build_score_tables against a brute-force walk, the table errors, and the argument checks of
hrseg_score_labels through the C ABI."""
import csv
import ctypes
import os
import re

import numpy as np
import pytest

from oracle import metrics as OM
from oracle import targets as OT
from tests import score_ref as R
from tests.helpers import DATA, ROOT, load_tree

TREES = {"tl": ("class_tree_tl.json", "class_map.csv"), "ext": ("class_tree_tl_extended.json", "class_map_extended.csv")}


def _tree(key):
    if key == "wide":
        return R.wide_tree()
    if key == "chain":
        return R.chain_tree(8)
    t, m = TREES[key]
    with open(os.path.join(DATA, m)) as f:
        return load_tree(t), list(csv.DictReader(f))


def test_reference_equals_the_oracle_masking_on_a_uniform_depth_tree():
    """every leaf at depth 1, every pixel labelled: the rule is the train loop's (oracle/metrics.py train_step_metrics:
    predictions and targets zeroed where the target is -1, then process_classes), on oracle/targets.py planes"""
    tree, cmap = R.uniform_tree()
    rng = np.random.default_rng(5)
    vals = np.array(sorted(cmap.values()), dtype=np.uint8)
    gt, pred = rng.choice(vals, size=(2, 17, 23)), rng.choice(vals, size=(2, 17, 23))
    tg, tp = OT.encode(gt, tree, cmap, 1), OT.encode(pred, tree, cmap, 1)
    C = [3, 7]
    want = []
    for L, (lo, hi) in enumerate(((0, 3), (3, 10))):
        t = tg[:, lo:hi]
        onehot = (tp[:, lo:hi] == 1).astype(np.float32)
        p_in = np.where(t == -1, 0.0, onehot).astype(np.float32)
        t_in = np.where(t == -1, 0.0, t).astype(np.float32)
        pl, tl = OM.process_classes(p_in, t_in, child_classes=(L > 0))
        k = C[L] + (1 if L else 0)
        want.append(np.bincount((tl * k + pl).reshape(-1), minlength=k * k))
    counts, ignored = R.score_batch(list(pred), list(gt), tree, cmap)
    assert np.array_equal(counts.sum(0), np.concatenate(want))
    assert not ignored.any()
    assert counts.sum(0)[:9].sum() == counts.sum(0)[9:].sum() == gt.size


def test_hand_computed_2x3_on_the_tl_tree():
    """tl tree: level 0 = background 0, upper 212, lower 255, tooth; level 1 (children of tooth) = pulp 127, dentin 170,
    enamel 85, composite 42.  Cells (gt -> pred):
      (0,0) 0 -> 0       level 0 [bg][bg];        level 1 [0][0]
      (0,1) 212 -> 255   level 0 [upper][lower];  level 1 [0][0]
      (0,2) 212 -> 170   level 0 [upper][tooth];  level 1 [0][0]   a tooth child under a non-tooth ground truth: it does
                                                                   not compete (level 0 disagrees)
      (1,0) 127 -> 0     level 0 [tooth][bg];     level 1 [pulp][0] the reverse: the prediction has no level-1 node
      (1,1) 127 -> 85    level 0 [tooth][tooth];  level 1 [pulp][enamel]
      (1,2) 7 -> 42      ground truth 7 is no class: ignored[0]"""
    tree, cmap = _tree("tl")
    gt = np.array([[0, 212, 212], [127, 127, 7]], dtype=np.uint8)
    pred = np.array([[0, 255, 170], [0, 85, 42]], dtype=np.uint8)
    cms, ignored = R.score_pair(pred, gt, tree, cmap)
    want0 = np.zeros((4, 4), dtype=np.int64)
    want0[0, 0] = want0[1, 2] = want0[1, 3] = want0[3, 0] = want0[3, 3] = 1
    want1 = np.zeros((5, 5), dtype=np.int64)
    want1[0, 0] = 3
    want1[1, 0] = 1
    want1[1, 3] = 1
    assert np.array_equal(cms[0], want0) and np.array_equal(cms[1], want1)
    assert ignored.tolist() == [1, 0]
    _, ignored = R.score_pair(np.array([[9]], dtype=np.uint8), np.array([[42]], dtype=np.uint8), tree, cmap)
    assert ignored.tolist() == [0, 1]


def _brute_path_entry(tree, cmap, v):
    """the uint64 path entry of pixel value v by a walk that searches the tree for the leaf"""
    pix = R.name2pix(cmap)
    levels = R.bfs_levels(tree)

    def find(node, trail):
        for name, sub in node.items():
            if isinstance(sub, dict) and sub:
                r = find(sub, trail + [name])
                if r is not None:
                    return r
            elif pix.get(name) == v:
                return trail + [name]
        return None
    trail = find(tree, [])
    if trail is None:
        return 0
    return sum((1 + levels[d].index(n)) << (8 * d) for d, n in enumerate(trail))


@pytest.mark.parametrize("key", ["tl", "ext", "wide", "chain"])
def test_invariants_on_random_maps_and_table_bytes(key):
    from hrseg_amd.Data import build_score_tables
    tree, cmap = _tree(key)
    tables = build_score_tables(tree, cmap)
    assert tables.path == [_brute_path_entry(tree, cmap, v) for v in range(256)]
    levels = R.bfs_levels(tree)
    assert tables.C == [len(n) for n in levels] and tables.names == levels
    assert tables.K == [n + (1 if L else 0) for L, n in enumerate(tables.C)]
    assert tables.total == sum(k * k for k in tables.K) and tables.offsets[0] == 0
    rng = np.random.default_rng(11)
    vals = np.array(sorted(R.name2pix(cmap).values()) + [1, 2], dtype=np.uint8)      # 1 and 2 are no class of any tree
    gt, pred = rng.choice(vals, size=(31, 45)), rng.choice(vals, size=(31, 45))
    cms, ignored = R.score_pair(pred, gt, tree, cmap)
    bad_gt = np.isin(gt, [1, 2])
    bad_pred = np.isin(pred, [1, 2]) & ~bad_gt
    assert ignored.tolist() == [int(bad_gt.sum()), int(bad_pred.sum())]
    valid = gt.size - int(ignored.sum())
    assert [int(m.sum()) for m in cms] == [valid] * len(cms)
    assert [m.shape[0] for m in cms] == tables.K


def test_table_errors():
    from hrseg_amd.Data import build_score_tables
    tree, cmap = _tree("tl")
    with pytest.raises(KeyError, match="Class 'enamel' not found in class_map"):
        build_score_tables(tree, [r for r in cmap if r["class_name"] != "enamel"])
    with pytest.raises(ValueError, match="does not fit a uint8"):
        build_score_tables(tree, [dict(r, pixel_val="300") if r["class_name"] == "pulp" else r for r in cmap])
    with pytest.raises(ValueError, match="share the pixel value 170"):
        build_score_tables(tree, [dict(r, pixel_val="170") if r["class_name"] == "pulp" else r for r in cmap])
    with pytest.raises(ValueError, match="9 levels"):
        build_score_tables(*R.chain_tree(9))
    wide = {f"c{i}": {} for i in range(17)}
    with pytest.raises(ValueError, match="17 channels"):
        build_score_tables(wide, {f"c{i}": i for i in range(17)})


def test_check_score_tables_refuses_a_path_outside_its_level():
    from hrseg_amd import ops
    from hrseg_amd.Data import build_score_tables
    tables = build_score_tables(*_tree("tl"))
    ops.check_score_tables(tables)
    tables.path[9] = 5                              # channel 4 of a 4-channel level 0
    with pytest.raises(ValueError, match="pixel value 9"):
        ops.check_score_tables(tables)


def test_step_sizes_of_ops_are_the_header_s():
    from hrseg_amd import ops
    src = open(os.path.join(ROOT, "include", "hrseg.h")).read()
    got = {k: int(v) for k, v in re.findall(r"#define HRSEG_SCORE_(\w+_STEP) (\d+)", src)}
    assert got == {"LANE_STEP": ops.SCORE_LANE_STEP, "WAVE_STEP": ops.SCORE_WAVE_STEP, "BLOCK_STEP": ops.SCORE_BLOCK_STEP}


def test_argument_checks_through_the_abi_without_a_gpu():
    from hrseg_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    lib.hrseg_last_error_string.restype = ctypes.c_char_p
    f = lib.hrseg_score_labels
    f.argtypes = _lib.PROTOTYPES["hrseg_score_labels"]
    f.restype = ctypes.c_int
    some = ctypes.c_void_p(4096)                   # never dereferenced: every call below is refused before the launch
    lib.hrseg_launch_count.restype = ctypes.c_long
    lib.hrseg_launch_count.argtypes = [ctypes.c_char_p, ctypes.c_int]
    before = lib.hrseg_launch_count(b"score_labels", 0)

    def call(nlevels, C, pred=some):
        return f(pred, some, some, some, some, nlevels, _lib.int_array(C), some, some, 1, 1, None)

    assert call(2, [4, 4], pred=None) == -1
    assert b"hrseg_score_labels: bad arguments" in lib.hrseg_last_error_string()
    assert call(9, [2] * 9) == -1
    assert b"hrseg_score_labels: nlevels=9" in lib.hrseg_last_error_string()
    assert call(2, [4, 17]) == -1
    assert b"hrseg_score_labels: C[1]=17" in lib.hrseg_last_error_string()
    assert call(5, [16] * 5) == -1
    assert b"hrseg_score_labels: 80 channels" in lib.hrseg_last_error_string()
    assert lib.hrseg_launch_count(b"score_labels", 0) == before
