"""Device post-processing, the parts that need no GPU: the numpy reference (tests/components_ref.py) pinned against
scipy.ndimage.label and hand-written answers, the tables of Data.postprocess.build_component_tables on both shipped trees,
and the refusals of the new entry points through the C ABI."""
import ctypes

import numpy as np
import pytest

from tests import components_ref as R
from tests.decode_harness import _tree

IDENT = np.arange(256, dtype=np.uint8)


def _adversarial(H, W):
    return {"uniform": np.full((H, W), 3, np.uint8), "checkerboard": R.checkerboard(H, W), "serpentine": R.serpentine(H, W),
            "spiral": R.spiral(H, W), "vstripes": R.stripes(H, W, True), "hstripes": R.stripes(H, W, False),
            "diagonal": R.diagonal(H, W, False, 8), "antidiagonal": R.diagonal(H, W, True, 8)}


def _scipy_roots(img, group, connectivity):
    ndi = pytest.importorskip("scipy.ndimage")
    structure = np.ones((3, 3), int) if connectivity == 8 else np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]])
    g = np.asarray(group)[img]
    roots = np.full(img.shape, -1, dtype=np.int64)
    flat = roots.reshape(-1)
    for gid in np.unique(g):
        lab, n = ndi.label(g == gid, structure=structure)
        lab = lab.reshape(-1)
        first = np.full(n + 1, flat.size, dtype=np.int64)
        idx = np.nonzero(lab)[0]
        np.minimum.at(first, lab[idx], idx)                    # the smallest index of every scipy label
        flat[idx] = first[lab[idx]]
    return roots


@pytest.mark.parametrize("connectivity", [4, 8])
def test_reference_partition_equals_scipy(connectivity):
    pytest.importorskip("scipy")
    rng = np.random.default_rng(11)
    group = IDENT.copy()
    group[[5, 6]] = 5                                          # two values of one group
    maps = list(_adversarial(17, 23).values()) + list(_adversarial(1, 9).values()) + list(_adversarial(9, 1).values())
    maps += [R.random_map(rng, 19, 31, [1, 2]), R.random_map(rng, 19, 31, [1, 2], 0.75), R.random_map(rng, 23, 17, [1, 5, 6]),
             R.random_map(rng, 16, 40, [0, 1, 2, 3, 4, 5, 6, 7]), R.random_map(rng, 40, 16, [1, 2], 0.35)]
    for m in maps:
        roots, area = R.label(m, group, connectivity)
        assert np.array_equal(roots, _scipy_roots(m, group, connectivity))
        flat = roots.reshape(-1)
        assert np.array_equal(area.reshape(-1), np.where(flat == np.arange(flat.size), np.bincount(flat, minlength=flat.size), 0))


def test_diagonal_pair_is_one_component_under_8_and_two_under_4():
    m = np.zeros((5, 5), np.uint8)
    m[1, 1] = m[2, 2] = 7
    r8, a8 = R.label(m, IDENT, 8)
    r4, a4 = R.label(m, IDENT, 4)
    assert r8[1, 1] == r8[2, 2] == 6 and a8[1, 1] == 2 and a8[2, 2] == 0
    assert r4[1, 1] == 6 and r4[2, 2] == 12 and a4[1, 1] == a4[2, 2] == 1
    assert a8[0, 0] == a4[0, 0] == 23 and (r8 == 0).sum() == 23
    # min_area 2 removes both singles under 4-connectivity and nothing under 8; the fill is the west neighbour's value
    out4, s4 = R.filter(m, IDENT, {7: (2, 0, -1)}, 4)
    out8, s8 = R.filter(m, IDENT, {7: (2, 0, -1)}, 8)
    assert not out4.any() and s4[7].tolist() == [2, 2, 2] and s4[0].tolist() == [1, 0, 0]
    assert np.array_equal(out8, m) and s8[7].tolist() == [1, 0, 0]


def test_keep_largest_tie_keeps_the_earlier_component():
    m = np.zeros((6, 6), np.uint8)
    m[0, 3:5] = 9                                              # area 2, first pixel 3
    m[3, 0:2] = 9                                              # area 2, first pixel 18
    m[5, 5] = 9                                                # area 1
    out, stats = R.filter(m, IDENT, {9: (0, 1, 4)}, 8)
    want = m.copy()
    want[3, 0:2] = want[5, 5] = 4
    assert np.array_equal(out, want) and stats[9].tolist() == [3, 2, 3]


def test_neighbour_fill_at_column_0_and_at_the_origin():
    m = np.full((5, 6), 1, np.uint8)
    m[0, 0] = 8                                                # the origin: stays, not counted as removed
    m[2, 0] = 8                                                # column 0: the north neighbour (1)
    m[1, 2] = 3
    m[1, 3] = 8                                                # the west neighbour (3), an input value
    out, stats = R.filter(m, IDENT, {8: (5, 0, -1), 3: (5, 0, 77)}, 4)
    want = m.copy()
    want[2, 0], want[1, 3], want[1, 2] = 1, 3, 77              # 3 is removed too: the fill of (1,3) does not cascade
    assert np.array_equal(out, want)
    assert stats[8].tolist() == [3, 2, 2] and stats[3].tolist() == [1, 1, 1] and stats[1].tolist() == [1, 0, 0]


def test_two_leaves_of_a_group_are_one_component_at_level_0_and_two_at_level_1():
    tree, cmap = _tree("tl")
    names0, g0 = R.cut_groups(tree, cmap, 0)
    names1, g1 = R.cut_groups(tree, cmap, 1)
    assert names0 == ["background", "upper", "lower", "tooth"]
    assert names1 == ["background", "upper", "lower", "pulp", "dentin", "enamel", "composite"]
    m = np.zeros((5, 7), np.uint8)
    m[1:4, 1:4] = 170                                          # dentin
    m[2, 2] = 127                                              # a pulp chamber of one pixel
    m[1:4, 4] = 85                                             # enamel beside it
    r0, a0 = R.label(m, g0, 8)
    assert a0[1, 1] == 12 and (r0[1:4, 1:5] == 8).all()
    r1, a1 = R.label(m, g1, 8)
    assert a1[1, 1] == 8 and a1[2, 2] == 1 and a1[1, 4] == 3
    # min_area on the tooth leaves the pulp alone at level 0 and deletes it at level 1
    assert np.array_equal(R.filter(m, g0, {3: (5, 0, 0)}, 8)[0], m)
    assert R.filter(m, g1, {3: (5, 0, 0)}, 8)[0][2, 2] == 0


# ------------------------------------------------------------------------------------------------------------------ tables
def test_component_tables_on_the_shipped_trees():
    from hrseg_amd.Data import build_component_tables
    want = {("tl", 0): ["background", "upper", "lower", "tooth"],
            ("tl", 1): ["background", "upper", "lower", "pulp", "dentin", "enamel", "composite"],
            ("ext", 0): ["background", "tooth+alveolar"],
            ("ext", 1): ["background", "alveolar", "tooth"],
            ("ext", 2): ["background", "upper", "lower", "composite", "healthy"],
            ("ext", 3): ["background", "upper", "lower", "composite", "pulp", "dentin", "enamel"]}
    for (key, level), names in want.items():
        tree, cmap = _tree(key)
        t = build_component_tables(tree, cmap, level)
        ref_names, ref_group = R.cut_groups(tree, cmap, level)
        assert t.names == names == ref_names, (key, level)
        assert t.group == ref_group.tolist(), (key, level)
        assert t.group[7] == t.group[254] == 255, "values outside the class map form group 255"
        assert t.rules == [(0, 0, -1)] * 256 and t.connectivity == 8
    tree, cmap = _tree("tl")
    t = build_component_tables(tree, cmap, 0, {"tooth": dict(min_area=30, keep_largest=False),
                                               "upper": dict(keep_largest=True, fill="background"),
                                               "lower": dict(min_area=2, fill=212)}, connectivity=4)
    assert t.group[127] == t.group[170] == t.group[85] == t.group[42] == 3 and t.group[0] == 0
    assert t.rules[3] == (30, 0, -1) and t.rules[1] == (0, 1, 0) and t.rules[2] == (2, 0, 212) and t.rules[0] == (0, 0, -1)
    assert t.rules[255] == (0, 0, -1) and t.connectivity == 4


def test_component_table_errors():
    from hrseg_amd.Data import build_component_tables
    tree, cmap = _tree("tl")
    pix = R.name2pix(cmap)
    with pytest.raises(KeyError):
        build_component_tables(tree, cmap, 0, {"molar": dict(min_area=3)})
    with pytest.raises(KeyError):
        build_component_tables(tree, cmap, 0, {"tooth": dict(fill="molar")})
    with pytest.raises(KeyError):
        build_component_tables(tree, cmap, 0, {"tooth": dict(fill="tooth")})          # a branch has no pixel value
    with pytest.raises(KeyError):
        build_component_tables(tree, {k: v for k, v in pix.items() if k != "enamel"}, 0)
    with pytest.raises(ValueError, match="uint8"):
        build_component_tables(tree, dict(pix, enamel=300), 0)
    with pytest.raises(ValueError, match="uint8"):
        build_component_tables(tree, cmap, 0, {"tooth": dict(fill=256)})
    with pytest.raises(ValueError, match="not in the cut"):
        build_component_tables(tree, cmap, 0, {"pulp": dict(min_area=3)})
    with pytest.raises(ValueError, match="not in the cut"):
        build_component_tables(tree, cmap, 1, {"tooth": dict(min_area=3)})
    with pytest.raises(ValueError, match="negative"):
        build_component_tables(tree, cmap, 0, {"tooth": dict(min_area=-1)})
    with pytest.raises(ValueError, match="connectivity"):
        build_component_tables(tree, cmap, 0, connectivity=6)
    wide = {f"c{i}": {} for i in range(256)}
    with pytest.raises(ValueError, match="at most 255"):
        build_component_tables(wide, {f"c{i}": i for i in range(256)}, 0)


# --------------------------------------------------------------------------------------------------------------------- ABI
def test_new_symbols_are_exported_and_the_abi_version_stays():
    from hrseg_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("hrseg_label_components", "hrseg_filter_components", "hrseg_filter_components_workspace_bytes",
                 "hrseg_components_tile"):
        assert hasattr(lib, name), name
    assert _lib.abi_version() == 17
    tw, th = _lib.components_tile()
    assert tw >= 16 and th >= 2 and tw % 16 == 0
    assert _lib.filter_components_workspace_bytes(3) >= 3 * 256 * 8
    assert _lib.launch_count("label_components") >= 0 and _lib.launch_count("filter_components") >= 0


def test_refusals_are_reported_without_a_gpu():
    """every refusal returns -1 with its message before anything is launched (placeholder pointers, never dereferenced;
    the descriptor's host copy is real host memory)"""
    from hrseg_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    lib.hrseg_last_error_string.restype = ctypes.c_char_p
    lib.hrseg_label_components.argtypes = _lib.PROTOTYPES["hrseg_label_components"]
    lib.hrseg_filter_components.argtypes = _lib.PROTOTYPES["hrseg_filter_components"]
    P = 1 << 20

    def desc(*rows):
        return (ctypes.c_long * (4 * len(rows)))(*[v for r in rows for v in r])

    def label(labels=P, d=P, host=None, B=1, group=P, conn=8, roots=2 * P, area=3 * P):
        host = desc((0, 4, 4, 1)) if host is None else host
        rc = lib.hrseg_label_components(labels, d, host, B, group, conn, roots, area, None)
        return rc, lib.hrseg_last_error_string().decode()

    def filt(labels=P, d=P, host=None, B=1, group=P, rules=P, roots=2 * P, area=3 * P, out=4 * P, stats=5 * P, work=6 * P):
        host = desc((0, 4, 4, 1)) if host is None else host
        rc = lib.hrseg_filter_components(labels, d, host, B, group, rules, roots, area, out, stats, work, None)
        return rc, lib.hrseg_last_error_string().decode()

    for conn in (0, 6, -8, 9):
        rc, msg = label(conn=conn)
        assert rc == -1 and f"hrseg_label_components: connectivity {conn}" in msg
    for null in ("labels", "d", "group", "roots", "area"):
        rc, msg = label(**{null: None})
        assert rc == -1 and msg == "hrseg_label_components: null pointer", null
    rc, msg = lib.hrseg_label_components(P, P, None, 1, P, 8, P, P, None), lib.hrseg_last_error_string().decode()
    assert rc == -1 and msg == "hrseg_label_components: null pointer"
    for B in (0, 65536):
        rc, msg = label(B=B)
        assert rc == -1 and "not in 1..65535" in msg
    rc, msg = label(roots=2 * P + 2)
    assert rc == -1 and "4-byte aligned" in msg
    rc, msg = label(area=3 * P + 1)
    assert rc == -1 and "4-byte aligned" in msg
    for rows in ([(0, 1 << 16, 1 << 15, 1)], [(0, 4, 4, 1), (16, 3, (1 << 31) // 3 + 1, 1)]):
        rc, msg = label(host=desc(*rows), B=len(rows))
        assert rc == -1 and "2^31 pixels or more" in msg, rows
        rc, msg = filt(host=desc(*rows), B=len(rows))
        assert rc == -1 and "hrseg_filter_components" in msg and "2^31 pixels or more" in msg, rows
    for row in ((-1, 4, 4, 1), (0, 0, 4, 1), (0, 4, 0, 1), (0, 4, 4, 3)):
        rc, msg = label(host=desc(row))
        assert rc == -1 and "bad descriptor" in msg, row

    for null in ("labels", "d", "group", "rules", "roots", "area", "out", "stats", "work"):
        rc, msg = filt(**{null: None})
        assert rc == -1 and msg == "hrseg_filter_components: null pointer", null
    rc, msg = filt(stats=5 * P + 4)
    assert rc == -1 and "8-byte aligned" in msg
    # overlap: two images, the second ends at byte 100 + 6 * 7 = 142: out must keep 142 bytes away from labels
    two = desc((3, 4, 4, 1), (100, 6, 7, 1))
    for out in (P, P + 141, P - 141, P + 1):
        rc, msg = filt(host=two, B=2, out=out)
        assert rc == -1 and msg == "hrseg_filter_components: out overlaps labels", out
    assert lib.hrseg_components_tile(None, None) == -1
