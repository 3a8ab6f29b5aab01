"""Device output pipeline, the parts that need no GPU: the tree tables of Data.decode.DeviceDecode, their error cases,
and the float64 oracle (tests/decode_ref.py) on a round trip through the target encoding and on a hand-computed case."""
import numpy as np
import pytest
import torch

from oracle import targets as OT
from tests import decode_ref as R
from tests.decode_harness import _tree


def _decoder(tree, cmap, model_type):
    from hrseg_amd.Data import DeviceDecode
    return DeviceDecode(tree, cmap, model_type)


def test_tables_of_the_tl_tree():
    tree, cmap = _tree("tl")
    t = _decoder(tree, cmap, 1).tables
    assert t.C == [4, 4] and not t.root_softmax
    assert t.names == [["background", "upper", "lower", "tooth"], ["pulp", "dentin", "enamel", "composite"]]
    assert t.first_child == [[-1, -1, -1, 0], [-1, -1, -1, -1]]
    assert t.n_children == [[0, 0, 0, 4], [0, 0, 0, 0]]
    assert t.pixel_val == [[0, 212, 255, -1], [127, 170, 85, 42]]
    f = _decoder(tree, cmap, 0).tables
    assert f.C == [7] and f.root_softmax
    assert f.names == [["background", "upper", "lower", "pulp", "dentin", "enamel", "composite"]]
    assert f.n_children == [[0] * 7] and f.pixel_val == [[0, 212, 255, 127, 170, 85, 42]]


def test_tables_of_the_extended_tree():
    tree, cmap = _tree("ext")
    t = _decoder(tree, cmap, 1).tables
    assert t.C == [2, 2, 4, 3]
    assert t.names == [["background", "tooth+alveolar"], ["alveolar", "tooth"], ["upper", "lower", "composite", "healthy"],
                       ["pulp", "dentin", "enamel"]]
    assert t.first_child == [[-1, 0], [0, 2], [-1, -1, -1, 0], [-1, -1, -1]]
    assert t.n_children == [[0, 2], [2, 2], [0, 0, 0, 3], [0, 0, 0]]
    assert t.pixel_val == [[0, -1], [-1, -1], [212, 255, 42, -1], [127, 170, 85]]
    f = _decoder(tree, cmap, 0).tables
    assert f.C == [7] and f.pixel_val == [[0, 212, 255, 42, 127, 170, 85]]
    assert _decoder(tree, cmap, 1).leaf_values == sorted([0, 212, 255, 42, 127, 170, 85])


def test_class_map_forms_agree():
    tree, cmap = _tree("tl")
    as_dict = {r["class_name"]: r["pixel_val"] for r in cmap}
    assert _decoder(tree, as_dict, 1).tables.pixel_val == _decoder(tree, cmap, 1).tables.pixel_val


def test_table_errors():
    tree, cmap = _tree("tl")
    with pytest.raises(KeyError, match="Class 'enamel' not found in class_map"):
        _decoder(tree, [r for r in cmap if r["class_name"] != "enamel"], 1)
    with pytest.raises(ValueError, match="does not fit a uint8"):
        _decoder(tree, [dict(r, pixel_val="300") if r["class_name"] == "pulp" else r for r in cmap], 0)
    # the channel of a node is its position in its level BY NAME (as the models look their parents up): a name used under
    # two parents scatters the second parent's children
    twice = {"a": {"x": {}, "y": {}}, "b": {"x": {}, "z": {}}}
    with pytest.raises(NotImplementedError, match="consecutive channels"):
        _decoder(twice, {"x": 1, "y": 2, "z": 3}, 1)
    wide = {f"c{i}": {} for i in range(17)}
    with pytest.raises(ValueError, match="17 channels"):
        _decoder(wide, {f"c{i}": i for i in range(17)}, 1)


def _split(target, Cs):
    out, s = [], 0
    for n in Cs:
        out.append(target[:, s:s + n])
        s += n
    return out


@pytest.mark.parametrize("key", ["tl", "ext"])
@pytest.mark.parametrize("model_type", [0, 1])
def test_round_trip_through_the_target_encoding(key, model_type):
    """label map -> oracle/targets.py targets -> logits 10 * target (-1 -> -10) -> decode at identity geometry = label map"""
    tree, cmap = _tree(key)
    pix = R.name2pix(cmap)
    rng = np.random.default_rng(3)
    vals = np.array(sorted(pix.values()), dtype=np.uint8)
    label = rng.choice(vals, size=(2, 24, 24))
    target = torch.from_numpy(OT.encode(label, tree, pix, model_type))
    Cs = _decoder(tree, cmap, model_type).tables.C
    assert sum(Cs) == target.shape[1]
    logits = _split(10.0 * target, Cs)
    for b in range(2):
        got, conf, tie, _ = R.decode_sample([z[b] for z in logits], tree, cmap, model_type, 24, 24)
        assert np.array_equal(got.numpy(), label[b])
        assert not bool(tie.any())
        assert float(conf.min()) > 0.99


def test_oracle_on_a_hand_computed_example():
    """2x2 -> 3x5.  Rows: scale 2/3, source coordinates (-1/6 -> 0, 1/2, 7/6 -> row 1 at weight 1 after the clamp of the
    second tap): weights of row 1 = [0, 1/2, 1].  Columns: scale 2/5, coordinates -0.3 -> 0, 0.1, 0.5, 0.9, 1.3 -> column
    1 at weight 1 (second tap clamped): weights of column 1 = [0, 0.1, 0.5, 0.9, 1]."""
    tree = {"bg": {}, "fg": {"a": {}, "b": {}}}
    cmap = {"bg": 0, "a": 100, "b": 200}
    wy = torch.tensor([0.0, 0.5, 1.0], dtype=torch.float64)
    wx = torch.tensor([0.0, 0.1, 0.5, 0.9, 1.0], dtype=torch.float64)

    def resized(q):         # q [2,2] -> [3,5] by the separable weights above
        q = q.double()
        rows = q[0][None, :] * (1 - wy)[:, None] + q[1][None, :] * wy[:, None]            # [3,2]
        return rows[:, 0:1] * (1 - wx)[None, :] + rows[:, 1:2] * wx[None, :]

    z0 = torch.tensor([[[2.0, -2.0], [2.0, -2.0]], [[-1.0, 1.0], [-1.0, 1.0]]])             # bg left, fg right
    z1 = torch.tensor([[[1.0, 1.0], [-3.0, -3.0]], [[0.0, 0.0], [0.0, 0.0]]])               # a on top, b below
    r0 = torch.stack([resized(z0[0]), resized(z0[1])])
    r1 = torch.stack([resized(z1[0]), resized(z1[1])])
    # level 0 by hand: bg = 2 - 4 wx, fg = -1 + 2 wx: fg wins where wx > 0.5 (tie at 0.5 -> bg, the lower index)
    assert torch.allclose(r0[0], (2 - 4 * wx)[None, :].expand(3, 5)) and torch.allclose(r0[1], (-1 + 2 * wx)[None, :].expand(3, 5))
    # level 1 by hand: a = 1 - 4 wy, b = 0: a wins on row 0 only
    want = np.array([[0, 0, 0, 100, 100], [0, 0, 0, 200, 200], [0, 0, 0, 200, 200]], dtype=np.uint8)
    label, conf, tie, path = R.decode_sample([z0, z1], tree, cmap, 1, 3, 5)
    assert np.array_equal(label.numpy(), want)
    assert path[0].tolist() == [[0, 0, 0, 1, 1]] * 3 and path[1].tolist() == [[-1, -1, -1, 0, 0], [-1, -1, -1, 1, 1], [-1, -1, -1, 1, 1]]
    sig = lambda v: 1.0 / (1.0 + np.exp(-v))      # noqa: E731
    assert abs(float(conf[0, 0]) - sig(2.0)) < 1e-12                                    # bg: sigmoid only
    assert abs(float(conf[0, 4]) - sig(1.0) * np.exp(1.0) / (np.exp(1.0) + 1.0)) < 1e-12  # fg(1) -> a: softmax([1, 0])[0]
    assert abs(float(conf[1, 3]) - sig(-1 + 1.8) * 1.0 / (np.exp(-1.0) + 1.0)) < 1e-12    # fg(0.8) -> b: softmax([-1, 0])[1]
    # the exact tie of level 0 at wx = 0.5 (both 0) is marked, and nothing else is
    assert tie.tolist() == [[False, False, True, False, False]] * 3
    # the flat decode of the same leaves: softmax over all of them
    zf = torch.tensor([[[3.0, 0.0], [0.0, 0.0]], [[0.0, 3.0], [0.0, 0.0]], [[0.0, 0.0], [3.0, 3.0]]])
    lf, cf, _, _ = R.decode_sample(zf, tree, cmap, 0, 2, 2)
    assert lf.tolist() == [[0, 100], [200, 200]]
    assert abs(float(cf[0, 0]) - np.exp(3.0) / (np.exp(3.0) + 2.0)) < 1e-12
