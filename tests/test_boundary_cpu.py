"""Device boundary scoring, the parts that need no GPU: the numpy reference (tests/boundary_ref.py) pinned by hand-worked
answers and against scipy's Euclidean distance transform, the nearest-rank percentile at its boundaries, and the new entry
points' exports, workspace formula and refusals through the C ABI."""
import ctypes
import math

import numpy as np
import pytest

from tests import boundary_ref as R
from tests import score_ref
from tests.decode_harness import _tree

NODES_TL = ["background", "upper", "lower", "tooth", "pulp", "dentin", "enamel", "composite"]
UPPER, TOOTH, DENTIN = 1, 3, 5                   # breadth-first node indices of the shipped tree
N, SUM, MAX, WITHIN, PK = range(5)


# ---------------------------------------------------------------------------------------------------------------- hand cases
def test_nodes_are_the_tree_breadth_first():
    tree, cmap = _tree("tl")
    nodes = R.node_values(tree, cmap)
    assert [n for n, _ in nodes] == NODES_TL
    assert dict(nodes)["tooth"] == [42, 85, 127, 170] and dict(nodes)["upper"] == [212]
    tree, cmap = _tree("ext")
    nodes = dict(R.node_values(tree, cmap))
    assert list(nodes) == ["background", "tooth+alveolar", "alveolar", "tooth", "upper", "lower", "composite", "healthy", "pulp",
                           "dentin", "enamel"]
    assert nodes["healthy"] == [85, 127, 170] and nodes["tooth+alveolar"] == [42, 85, 127, 170, 212, 255]


def test_two_single_pixels():
    tree, cmap = _tree("tl")
    pred, gt = np.zeros((6, 7), np.uint8), np.zeros((6, 7), np.uint8)
    pred[0, 0] = gt[3, 4] = 212
    rec = R.score_pair(pred, gt, tree, cmap, tau2=4, percentile=95)
    assert rec.shape == (8, 2, 5) and rec.dtype == np.int64
    assert rec[UPPER].tolist() == [[1, 5 << 16, 25, 0, 25]] * 2
    d = R.derived(rec)
    assert d["hausdorff"][UPPER] == 5.0 and d["hd_percentile"][UPPER] == 5.0 and d["assd"][UPPER] == 5.0
    assert d["surface_dice"][UPPER] == 0.0
    # the background has a hole at another place in each map.  Prediction: the image's rim (22 pixels) without the corner
    # itself, whose two neighbours lie on the rim; truth: the rim and the four neighbours of the inner hole
    # (3, 3), say, is 3 rows from the rim
    assert rec[0, 0, N] == 21 and rec[0, 1, N] == 26 and rec[0, 0, MAX] == 0 and rec[0, 1, MAX] == 4
    assert not rec[[2, 3, 4, 5, 6, 7]].any(), "absent nodes: all zeros"


def test_square_against_the_square_two_columns_on():
    """4 x 4 squares at columns 2..5 and 4..7: the rim of a square is 12 pixels.  Prediction -> truth: column 2 (4 pixels)
    is 2 columns from the truth's column 4: d2 = 4; (3,3), (6,3) are one column from it and (4,5), (5,5) lie inside the
    truth's square, one pixel from its rim: d2 = 1; (3,4), (3,5), (6,4), (6,5) lie on the truth's rim: d2 = 0.  The other
    direction is the mirror image."""
    tree, cmap = _tree("tl")
    pred, gt = np.zeros((10, 12), np.uint8), np.zeros((10, 12), np.uint8)
    pred[3:7, 2:6] = 212
    gt[3:7, 4:8] = 212
    assert int(R.border(pred == 212).sum()) == 12
    want_sum = 4 * (2 << 16) + 4 * (1 << 16)
    for tau2, within in ((0, 4), (1, 8), (3, 8), (4, 12)):
        rec = R.score_pair(pred, gt, tree, cmap, tau2, 95)
        assert rec[UPPER].tolist() == [[12, want_sum, 4, within, 4]] * 2, tau2
    assert R.score_pair(pred, gt, tree, cmap, 1, 50)[UPPER, :, PK].tolist() == [1, 1]       # k = 6 of 0 0 0 0 1 1 1 1 4 4 4 4
    assert R.score_pair(pred, gt, tree, cmap, 1, 33)[UPPER, :, PK].tolist() == [0, 0]       # k = 4
    d = R.derived(R.score_pair(pred, gt, tree, cmap, 1, 95))
    assert d["hausdorff"][UPPER] == 2.0 and d["assd"][UPPER] == 1.0 and d["surface_dice"][UPPER] == 16 / 24


def test_identical_maps_and_a_node_absent_from_one():
    tree, cmap = _tree("tl")
    rng = np.random.default_rng(3)
    vals = sorted(score_ref.name2pix(cmap).values())
    m = R.blobby(rng, 24, 31, vals)
    rec = R.score_pair(m, m, tree, cmap, 0, 95)
    present = rec[:, 0, N] > 0
    assert present.sum() >= 3
    assert (rec[:, 0, N] == rec[:, 1, N]).all() and not rec[:, :, [SUM, MAX, PK]].any()
    assert (rec[:, :, WITHIN] == rec[:, :, N]).all()
    d = R.derived(rec)
    assert (d["surface_dice"][present] == 1.0).all() and (d["hausdorff"][present] == 0.0).all()
    assert np.isnan(d["surface_dice"][~present]).all()
    # dentin only in the truth: n[1] counts its rim, everything else is 0, the derived figures are NaN; the tooth above
    # it is in both maps (the prediction says enamel there)
    pred, gt = np.zeros((9, 9), np.uint8), np.zeros((9, 9), np.uint8)
    gt[2:6, 2:6] = 170
    pred[2:6, 2:6] = 85
    rec = R.score_pair(pred, gt, tree, cmap, 1, 95)
    assert rec[DENTIN].tolist() == [[0, 0, 0, 0, 0], [12, 0, 0, 0, 0]]
    assert rec[TOOTH].tolist() == [[12, 0, 0, 12, 0]] * 2
    d = R.derived(rec)
    assert all(np.isnan(d[k][DENTIN]) for k in d) and d["surface_dice"][TOOTH] == 1.0


def test_unlabelled_truth_and_foreign_predictions_belong_to_no_node():
    tree, cmap = _tree("tl")
    gt = np.full((7, 9), 212, np.uint8)
    pred = gt.copy()
    gt[3, 4] = 7                                                   # no leaf's value: a hole in BOTH maps
    pred[1, 1] = 9                                                 # outside the class map: a hole in the prediction only
    pm, gm = R.masks(pred, gt, tree, cmap)[UPPER]
    assert not pm[3, 4] and not gm[3, 4] and not pm[1, 1] and gm[1, 1]
    rim = 2 * 7 + 2 * 9 - 4
    rec = R.score_pair(pred, gt, tree, cmap, 0, 100)
    # the four neighbours of a hole are border pixels; (1,1) itself is a border pixel of the truth only
    assert rec[UPPER, 1, N] == rim + 4 and rec[UPPER, 0, N] == rim + 4 + 2, rec[UPPER]
    assert rec[UPPER, 1, MAX] == 0 and rec[UPPER, 0, MAX] == 1


# ------------------------------------------------------------------------------------------------- distance transform
@pytest.mark.parametrize("key", ["tl", "ext"])
def test_all_pairs_distances_equal_the_distance_transform(key):
    ndi = pytest.importorskip("scipy.ndimage")
    tree, cmap = _tree(key)
    rng = np.random.default_rng(5)
    vals = sorted(score_ref.name2pix(cmap).values())
    checked = 0
    for H, W in ((37, 53), (64, 40)):
        gt = R.blobby(rng, H, W, vals)
        pred = R.perturb(rng, gt, vals + [9])
        for pm, gm in R.masks(pred, gt, tree, cmap):
            bp, bg = R.border(pm), R.border(gm)
            if not bp.any() or not bg.any():
                continue
            for q, t in ((bp, bg), (bg, bp)):
                edt = np.rint(ndi.distance_transform_edt(~t) ** 2).astype(np.int64)
                d2 = R.nearest_d2(np.argwhere(q).astype(np.int64), np.argwhere(t).astype(np.int64))
                assert np.array_equal(d2, edt[q])
                checked += len(d2)
    assert checked > 500


# ------------------------------------------------------------------------------------------------------- nearest rank
@pytest.mark.parametrize("n", [1, 19, 20, 21, 100, 101])
def test_nearest_rank_boundaries(n):
    values = np.random.default_rng(n).permutation(np.arange(10, 10 + n))
    for p in (1, 5, 50, 95, 99, 100):
        k = math.ceil(p * n / 100)
        assert (p * n + 99) // 100 == k and 1 <= k <= n
        assert R.nearest_rank(values, p) == 10 + k - 1
    assert R.nearest_rank(values, 100) == 10 + n - 1
    # 95 %: the largest value up to n = 19 (k = ceil(18.05) = 19), the one before it at 20 (k = 19) and 21 (k = 20)
    assert R.nearest_rank(values, 95) == 10 + n - 1 - (1 if n >= 20 else 0) - (4 if n >= 100 else 0)


def test_nearest_rank_with_ties_at_the_kth_value():
    values = np.array([7] * 18 + [3] * 1 + [9] * 1)                   # sorted: 3, 7 x 18, 9
    assert [R.nearest_rank(values, p) for p in (1, 5, 6, 95, 96, 100)] == [3, 3, 7, 7, 9, 9]
    assert R.nearest_rank(np.array([4, 4, 4]), 50) == 4


def test_isqrt_is_the_floor_in_q16():
    for d2 in (0, 1, 2, 3, 25, 2 ** 24 + 1, 2 * 32767 ** 2):
        s = math.isqrt(d2 << 32)
        assert s * s <= d2 << 32 < (s + 1) * (s + 1)
    assert math.isqrt(2 << 32) == 92681                              # sqrt(2) = 1.41421356..., 92681 / 65536 = 1.414199...


# --------------------------------------------------------------------------------------------------------------------- ABI
def _formula(rows, C):
    """hrseg.h: 16 B + 4 (B 2N 260 + even(sum 2N H ceil(W / 32)) + sum 2 nlevels H W)"""
    Nn, B = sum(C), len(rows)
    bitmaps = sum(2 * Nn * H * ((W + 31) // 32) for _, H, W, _ in rows)
    maps = sum(2 * len(C) * H * W for _, H, W, _ in rows)
    return 16 * B + 4 * (B * 2 * Nn * 260 + bitmaps + bitmaps % 2 + maps)


def _desc(*rows):
    return (ctypes.c_long * (4 * len(rows)))(*[v for r in rows for v in r])


def test_new_symbols_are_exported_and_the_abi_version_stays():
    import torch
    from hrseg_amd import _lib, ops
    from hrseg_amd.Data import build_score_tables
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("hrseg_score_boundaries", "hrseg_boundary_workspace_bytes"):
        assert hasattr(lib, name), name
    assert _lib.abi_version() == 17
    assert _lib.launch_count("score_boundaries") >= 0
    assert ops.SCORE_BOUNDARIES_LAUNCHES == 11 and ops.BOUNDARY_FIELDS == R.FIELDS
    for rows, C in (([(0, 1, 1, 1)], [1]), ([(5, 3, 33, 1), (200, 7, 64, 1), (1000, 1, 65, 1)], [4, 4]),
                    ([(0, 1400, 2900, 1)] * 4, [2, 2, 5, 3]), ([(0, 32768, 32768, 1)], [16] * 4)):
        table = _desc(*rows)                                        # (kept alive across the call)
        got = _lib.boundary_workspace_bytes(table, len(rows), C)
        assert got == _formula(rows, C), (rows, C)
    tree, cmap = _tree("ext")
    tables = build_score_tables(tree, cmap)
    host = torch.tensor([[0, 50, 70, 1], [3500, 9, 31, 1]], dtype=torch.int64)
    assert ops.boundary_workspace_bytes(host, tables) == _formula(host.tolist(), tables.C)
    with pytest.raises(RuntimeError, match="a side above 32768"):
        _lib.boundary_workspace_bytes(_desc((0, 1, 32769, 1)), 1, [4])
    with pytest.raises(RuntimeError, match="bad arguments"):
        _lib.boundary_workspace_bytes(_desc((0, 1, 1, 1)), 0, [4])


def test_refusals_are_reported_without_a_gpu():
    """every refusal returns -1 with its message before anything is launched (placeholder pointers, never dereferenced;
    the descriptors' host copy and C are real host memory)"""
    from hrseg_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    lib.hrseg_last_error_string.restype = ctypes.c_char_p
    lib.hrseg_score_boundaries.argtypes = _lib.PROTOTYPES["hrseg_score_boundaries"]
    P = 1 << 20
    who = "hrseg_score_boundaries"

    def run(pred=P, pdesc=P, gt=P, gdesc=P, host=None, lut=P, C=(4, 4), nlevels=None, tau2=4, pct=95, records=2 * P, work=3 * P,
            B=1, no_host=False, no_C=False):
        host = _desc((0, 4, 4, 1), (16, 4, 4, 1)) if host is None else host
        rc = lib.hrseg_score_boundaries(pred, pdesc, gt, gdesc, None if no_host else host, lut, len(C) if nlevels is None else nlevels,
                                        None if no_C else _lib.int_array(list(C)), tau2, pct, records, work, B, None)
        return rc, lib.hrseg_last_error_string().decode()

    for null in ("pred", "pdesc", "gt", "gdesc", "lut", "records", "work"):
        assert run(**{null: None}) == (-1, f"{who}: null pointer"), null
    assert run(no_host=True) == (-1, f"{who}: null pointer") and run(no_C=True) == (-1, f"{who}: null pointer")
    for B in (0, -1, 65536):
        rc, msg = run(B=B)
        assert rc == -1 and f"B={B} not in 1..65535" in msg
    for bad in (dict(records=2 * P + 4), dict(work=3 * P + 4), dict(work=3 * P + 1), dict(lut=P + 4)):
        rc, msg = run(**bad)
        assert rc == -1 and "8-byte aligned" in msg, bad
    for pct in (0, -5, 101):
        rc, msg = run(pct=pct)
        assert rc == -1 and f"percentile {pct} not in 1..100" in msg
    rc, msg = run(tau2=-1)
    assert rc == -1 and "tau2 -1 is negative" in msg
    for bad, text in ((dict(C=(), nlevels=0), "nlevels=0"), (dict(C=(1,) * 9), "nlevels=9"), (dict(C=(4, 17)), "C[1]=17"),
                      (dict(C=(4, 0)), "C[1]=0"), (dict(C=(16, 16, 16, 16, 1)), "65 nodes")):
        rc, msg = run(**bad)
        assert rc == -1 and text in msg, (bad, msg)
    # the descriptor rules of hrseg_label_components, on either table
    for row in ((-1, 4, 4, 1), (0, 0, 4, 1), (0, 4, 0, 1), (0, 4, 4, 3)):
        for host in (_desc(row, (0, 4, 4, 1)), _desc((0, 4, 4, 1), row)):
            rc, msg = run(host=host)
            assert rc == -1 and "bad descriptor" in msg, row
    rc, msg = run(host=_desc((0, 1 << 16, 1 << 15, 1), (0, 1 << 16, 1 << 15, 1)))
    assert rc == -1 and "2^31 pixels or more" in msg
    for row in ((0, 32769, 2, 1), (0, 2, 32769, 1)):
        rc, msg = run(host=_desc(row, row))
        assert rc == -1 and "a side above 32768" in msg
    two = _desc((0, 4, 4, 1), (16, 5, 6, 1), (0, 4, 4, 1), (16, 6, 5, 1))
    rc, msg = run(host=two, B=2)
    assert rc == -1 and "image 1: predicted map 5 x 6, ground truth 6 x 5" in msg
