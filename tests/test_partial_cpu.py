"""Partial labels on the host: the two bit tables of Data.dataset.build_target_luts against hand-written expectations, its
refusals, and the four-step channel rule of tests/partial_ref.py against a per-pixel walk of the tree (no GPU)."""
import csv
import os

import numpy as np
import pytest

from oracle.targets import level_order_names, node_masks, parent_map
from tests import partial_ref as PR
from tests.helpers import DATA, load_tree

TREES = {"tl": ("class_tree_tl.json", "class_map.csv"), "ext": ("class_tree_tl_extended.json", "class_map_extended.csv")}


def _tree(key):
    t, m = TREES[key]
    with open(os.path.join(DATA, m)) as f:
        return load_tree(t), list(csv.DictReader(f))


def _bits(names, *on):
    return sum(1 << names.index(n) for n in on)


def test_tables_of_the_tl_tree():
    from hrseg_amd.Data.dataset import build_target_luts
    tree, cmap = _tree("tl")
    names, parent, on, unk = build_target_luts(tree, cmap, 1, internal_values={"tooth": 9}, ignore_values=[254])
    assert names == ["background", "upper", "lower", "tooth", "pulp", "dentin", "enamel", "composite"]
    assert parent == [-1, -1, -1, -1, 3, 3, 3, 3]
    assert len(on) == len(unk) == 256 and all(type(v) is int for v in on + unk)
    assert (on[127], unk[127]) == (_bits(names, "pulp", "tooth"), 0)                               # a leaf byte
    assert (on[9], unk[9]) == (_bits(names, "tooth"), _bits(names, "pulp", "dentin", "enamel", "composite"))
    assert (on[254], unk[254]) == (0, 0xFF)                                                        # the ignore byte
    assert (on[1], unk[1]) == (0, 0)                                                               # any other byte
    # flat mode: the leaves only; the byte of tooth switches nothing on and leaves the leaves below it unknown
    names, parent, on, unk = build_target_luts(tree, cmap, 0, internal_values={"tooth": 9}, ignore_values=[254])
    assert names == ["background", "upper", "lower", "pulp", "dentin", "enamel", "composite"] and parent == [-1] * 7
    assert (on[127], unk[127]) == (_bits(names, "pulp"), 0)
    assert (on[9], unk[9]) == (0, _bits(names, "pulp", "dentin", "enamel", "composite"))
    assert (on[254], unk[254]) == (0, 0x7F)


def test_tables_of_the_extended_tree():
    from hrseg_amd.Data.dataset import build_target_luts
    tree, cmap = _tree("ext")
    names, parent, on, unk = build_target_luts(tree, cmap, 1, internal_values={"tooth": 7, "healthy": 9, "tooth+alveolar": 11},
                                               ignore_values=[3, 4])
    assert names == ["background", "tooth+alveolar", "alveolar", "tooth", "upper", "lower", "composite", "healthy", "pulp",
                     "dentin", "enamel"]
    assert parent == [-1, -1, 1, 1, 2, 2, 3, 3, 7, 7, 7]
    assert (on[85], unk[85]) == (_bits(names, "enamel", "healthy", "tooth", "tooth+alveolar"), 0)
    assert (on[7], unk[7]) == (_bits(names, "tooth", "tooth+alveolar"),
                               _bits(names, "composite", "healthy", "pulp", "dentin", "enamel"))
    assert (on[9], unk[9]) == (_bits(names, "healthy", "tooth", "tooth+alveolar"), _bits(names, "pulp", "dentin", "enamel"))
    assert (on[11], unk[11]) == (_bits(names, "tooth+alveolar"), 0x7FF & ~_bits(names, "background", "tooth+alveolar"))
    assert (on[3], unk[3]) == (on[4], unk[4]) == (0, 0x7FF)
    names, parent, on, unk = build_target_luts(tree, cmap, 0, internal_values={"tooth": 7}, ignore_values=[3])
    assert names == ["background", "upper", "lower", "composite", "pulp", "dentin", "enamel"] and parent == [-1] * 7
    assert (on[7], unk[7]) == (0, _bits(names, "composite", "pulp", "dentin", "enamel"))
    assert (on[212], unk[212]) == (_bits(names, "upper"), 0) and (on[3], unk[3]) == (0, 0x7F)


@pytest.mark.parametrize("key", ["tl", "ext"])
@pytest.mark.parametrize("model_type", [0, 1])
def test_without_partial_values_the_tables_are_the_old_ones(key, model_type):
    """on_lut is the table of fully labelled maps, restated here from the oracle's node masks of the 256 byte values (bit c
    of entry v: value v lies in channel c's mask), and unk_lut is all zero"""
    from hrseg_amd.Data.dataset import build_target_luts
    tree, cmap = _tree(key)
    names, parent, on, unk = build_target_luts(tree, cmap, model_type)
    emit, want_parent = PR.emitted(tree, model_type)
    masks = node_masks(tree, np.arange(256), PR.R.name2pix(cmap))
    want = [sum(1 << c for c, n in enumerate(emit) if masks[n][v]) for v in range(256)]
    assert names == emit and parent == want_parent and on == want and unk == [0] * 256


def test_refusals_name_the_classes():
    from hrseg_amd.Data.dataset import build_target_luts
    tree, cmap = _tree("ext")
    for key in ("tl", "ext"):                          # 255 is a real class in both shipped maps
        with pytest.raises(ValueError, match="ignore value 255 is already the value of class 'lower'"):
            build_target_luts(*_tree(key), 1, ignore_values=[255])
    with pytest.raises(ValueError, match="value 42 of internal node 'tooth' is already the value of class 'composite'"):
        build_target_luts(tree, cmap, 1, internal_values={"tooth": 42})
    with pytest.raises(ValueError, match="value 7 of internal node 'healthy' is already the value of internal node 'tooth'"):
        build_target_luts(tree, cmap, 1, internal_values={"tooth": 7, "healthy": 7})
    with pytest.raises(ValueError, match="ignore value 7 is already the value of internal node 'tooth'"):
        build_target_luts(tree, cmap, 1, internal_values={"tooth": 7}, ignore_values=[7])
    with pytest.raises(ValueError, match="ignore value 3 is already the value of ignore value 3"):
        build_target_luts(tree, cmap, 1, ignore_values=[3, 3])
    with pytest.raises(ValueError, match="internal value for 'molar', which is no node of the class tree"):
        build_target_luts(tree, cmap, 1, internal_values={"molar": 7})
    with pytest.raises(ValueError, match="internal value for 'pulp', which is a leaf"):
        build_target_luts(tree, cmap, 1, internal_values={"pulp": 7})
    with pytest.raises(ValueError, match="value 256 of internal node 'tooth' does not fit"):
        build_target_luts(tree, cmap, 1, internal_values={"tooth": 256})
    with pytest.raises(ValueError, match="ignore value -1 does not fit"):
        build_target_luts(tree, cmap, 1, ignore_values=[-1])
    with pytest.raises(ValueError, match="ignore value 300 does not fit"):
        build_target_luts(tree, cmap, 0, ignore_values=[300])


def test_a_hedge_supplies_the_values():
    """`Hedge.values` and `Hedge.reject_val` are the arguments' form: every byte a hedged map can hold has a table entry"""
    from hrseg_amd.Data.dataset import build_target_luts
    from hrseg_amd.Data.hedge import Hedge
    tree, cmap = _tree("ext")
    h = Hedge(tree, cmap, 0.5, reject_value=200)
    names, _, on, unk = build_target_luts(tree, cmap, 1, internal_values=h.values, ignore_values=[h.reject_val])
    for v, name in h.value_names.items():
        if name == "rejected":
            assert (on[v], unk[v]) == (0, (1 << len(names)) - 1)
        else:
            assert on[v] >> names.index(name) & 1 and not unk[v] >> names.index(name) & 1


def test_entry_points_refuse_bad_arguments_under_their_own_name():
    """C in 1..64, the parent range and the workspace size, before anything is launched (placeholder pointers, never
    dereferenced); the workspace of the partial warp holds two words per pixel where the old one holds one"""
    import ctypes
    from hrseg_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    lib.hrseg_last_error_string.restype = ctypes.c_char_p
    P = ctypes.c_void_p(4096)
    enc, aug = lib.hrseg_encode_targets_partial, lib.hrseg_augment_targets_partial
    enc.argtypes, aug.argtypes = (_lib.PROTOTYPES[n] for n in ("hrseg_encode_targets_partial", "hrseg_augment_targets_partial"))

    def encode(C=4, parent=(-1, -1, 0, 0), unk=P):
        return enc(P, P, unk, _lib.int_array(list(parent)), P, 1, C, 16, None), lib.hrseg_last_error_string().decode()

    def augment(C=4, parent=(-1, -1, 0, 0), unk=P, warp=0, work=None, nbytes=0):
        rc = aug(P, P, P, unk, _lib.int_array(list(parent)), P, P, 2, C, 62, warp, 1, 0, work, nbytes, None)
        return rc, lib.hrseg_last_error_string().decode()
    for fn, name in ((encode, "hrseg_encode_targets_partial"), (augment, "hrseg_augment_targets_partial")):
        assert fn(unk=None) == (-1, f"{name}: bad arguments")
        assert fn(C=0) == (-1, f"{name}: C=0 not in 1..64") and fn(C=65) == (-1, f"{name}: C=65 not in 1..64")
        assert fn(parent=(-1, -1, 4, 0)) == (-1, f"{name}: parent[2]=4 out of range")
        assert fn(parent=(-2, -1, 0, 0)) == (-1, f"{name}: parent[0]=-2 out of range")
    old_i, old_t, new_t = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_size_t(0)
    _lib.call_raw("hrseg_augment_workspace", 2, 62, ctypes.byref(old_i), ctypes.byref(old_t))
    _lib.call_raw("hrseg_augment_workspace_partial", 2, 62, ctypes.byref(new_t))
    def up(n):
        return (n + 255) // 256 * 256                           # both parts are rounded up to 256 bytes
    flags = up(2 * 16 * 4)                                      # one int per block of 256 pixels
    assert old_t.value == up(2 * 62 * 62 * 8) + flags and new_t.value == up(2 * 62 * 62 * 16) + flags
    assert augment(warp=1) == (-1, "hrseg_augment_targets_partial: the warp needs params and a workspace")
    assert augment(warp=1, work=P, nbytes=old_t.value) == \
        (-1, f"hrseg_augment_targets_partial: workspace {old_t.value} bytes, needs {new_t.value}")
    with pytest.raises(RuntimeError, match="hrseg_augment_workspace_partial: bad arguments"):
        _lib.call_raw("hrseg_augment_workspace_partial", 0, 62, ctypes.byref(new_t))


# ---- the four-step rule against a per-pixel walk
TREE3 = {"a": {}, "b": {"b0": {}, "b1": {"b10": {}, "b11": {}}}, "c": {"c0": {}, "c1": {}}}
MAP3 = [{"class_name": n, "pixel_val": v} for n, v in
        [("a", "0"), ("b", "None"), ("b0", "10"), ("b1", "None"), ("b10", "20"), ("b11", "30"), ("c", "None"), ("c0", "40"),
         ("c1", "50")]]
INTERNAL3 = {"b": 101, "b1": 102, "c": 103}
IGNORE3 = (250, 251)


def _walk(v, tree, model_type):
    """one pixel of byte v by the definition: its node (or ignore / nothing), then every channel in turn"""
    par = parent_map(tree)
    names = level_order_names(tree)
    emit, _ = PR.emitted(tree, model_type)
    node = {int(r["pixel_val"]): r["class_name"] for r in MAP3 if r["pixel_val"] != "None"}
    node.update({b: n for n, b in INTERNAL3.items()})
    here = node.get(v)

    def chain(n):
        out = []
        while n is not None:
            out.append(n)
            n = par[n]
        return out
    out = []
    for c in emit:
        if here is not None and c in chain(here):
            out.append(1.0)                                                 # 1: the node or an ancestor of it
        elif v in IGNORE3 or (here is not None and here in chain(c)):
            out.append(-1.0)                                                # 2: unknown (ignored, or strictly below the node)
        elif model_type == 0 or par[c] is None or (here is not None and par[c] in chain(here)):
            out.append(0.0)                                                 # 3: a root, or the direct parent is on
        else:
            out.append(-1.0)                                                # 4: outside the parent
    assert len(names) == 9
    return out


@pytest.mark.parametrize("model_type", [0, 1])
def test_four_step_rule_against_a_per_pixel_walk(model_type):
    rng = np.random.default_rng(5)
    vals = [0, 10, 20, 30, 40, 50, 101, 102, 103, 250, 251, 7]              # leaves, internal nodes, ignore, an unused byte
    lab = rng.choice(np.array(vals, dtype=np.uint8), size=(2, 9, 13))
    lab[0, 0, :len(vals)] = vals
    got = PR.encode(lab, TREE3, MAP3, model_type, INTERNAL3, IGNORE3).numpy()
    want = np.array([[[_walk(int(v), TREE3, model_type) for v in row] for row in img] for img in lab], dtype=np.float32)
    assert np.array_equal(got, want.transpose(0, 3, 1, 2))
    # and the product's tables say the same through the same rule
    from hrseg_amd.Data.dataset import build_target_luts
    names, parent, on, unk = build_target_luts(TREE3, MAP3, model_type, INTERNAL3, IGNORE3)
    for v in vals:
        import torch
        C = len(names)
        o = torch.tensor([bool(on[v] >> c & 1) for c in range(C)])
        u = torch.tensor([bool(unk[v] >> c & 1) for c in range(C)])
        assert PR.encode_sets(o, u, parent).tolist() == _walk(v, TREE3, model_type), v


def test_consequences_stated_in_the_header():
    """a "tooth" pixel of the tl tree: tooth 1, the other roots 0, everything below level 0 -1; an ignored pixel: -1 in every
    channel; flat mode: -1 on the leaves below the node and 0 on the others"""
    tree, cmap = _tree("tl")
    lab = np.array([[[9, 254]]], dtype=np.uint8)
    y = PR.encode(lab, tree, cmap, 1, {"tooth": 9}, [254])[0, :, 0]
    assert y[:, 0].tolist() == [0, 0, 0, 1, -1, -1, -1, -1] and y[:, 1].tolist() == [-1] * 8
    y = PR.encode(lab, tree, cmap, 0, {"tooth": 9}, [254])[0, :, 0]
    assert y[:, 0].tolist() == [0, 0, 0, -1, -1, -1, -1] and y[:, 1].tolist() == [-1] * 7
