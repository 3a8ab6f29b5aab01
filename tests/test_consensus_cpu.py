"""The consensus reference (tests/consensus_ref.py) and the host side of Data/consensus.py, without a GPU: the vectorised
reference against a brute-force per-pixel walk, the worked examples of include/hrseg.h as literals, the exact identities
between the counter blocks, table building and refusals, summary() against hand-computed figures, and the round trip of a
consensus map through the oracle's partial-label rule."""
import itertools
import math

import numpy as np
import pytest
import torch

from tests import consensus_ref as R

TREE_KEYS = ["tl", "wide", "chain", "flat", "uniform"]


def _random_members(rng, nodes, M, H, W):
    vals = R.palette(nodes)
    return [R.blob_map(rng, vals, H, W, block=2) if m % 2 else rng.choice(vals, size=(H, W)).astype(np.uint8) for m in range(M)]


@pytest.mark.parametrize("key", TREE_KEYS)
def test_vectorised_reference_is_the_brute_force_walk(key):
    _, _, _, nodes = R.setup(key)
    rng = np.random.default_rng(5)
    for M in (1, 2, 3, 5, 8):
        members = _random_members(rng, nodes, M, 5, 7)
        for q in R.quorums(M):
            labels, support, ended = R.vote(members, nodes, R.NONE_VAL, q)
            for y in range(5):
                for x in range(7):
                    want = R.vote_pixel([m[y, x] for m in members], nodes, R.NONE_VAL, q)
                    assert (int(labels[y, x]), int(support[y, x]), int(ended[y, x])) == want, (key, M, q, y, x)


def test_worked_examples_on_the_shipped_tree():
    tree, cmap = R.tl_tree()
    tooth, reject, none = 60, 61, 62
    nodes = R.Nodes(tree, cmap, {"tooth": tooth})
    upper, lower, enamel, dentin = 212, 255, 85, 170
    assert R.vote_pixel([tooth, enamel, enamel], nodes, none, 2) == (enamel, 2, nodes.index["enamel"])
    assert R.vote_pixel([enamel, dentin, tooth], nodes, none, 2) == (tooth, 3, nodes.index["tooth"])
    assert R.vote_pixel([upper, lower, reject], nodes, none, 2) == (none, 0, len(nodes.names))
    members = [np.array([[tooth, enamel, upper]], np.uint8), np.array([[enamel, dentin, lower]], np.uint8),
               np.array([[enamel, tooth, reject]], np.uint8)]
    labels, support, _ = R.vote(members, nodes, none, 2)
    assert labels.tolist() == [[enamel, tooth, none]] and support.tolist() == [[2, 3, 0]]
    # with the quorum at M the first two fall back to the parent, where all three agree
    labels, support, _ = R.vote(members, nodes, none, 3)
    assert labels.tolist() == [[tooth, tooth, none]] and support.tolist() == [[3, 3, 0]]


@pytest.mark.parametrize("key", TREE_KEYS)
def test_identities_between_the_counter_blocks(key):
    _, _, _, nodes = R.setup(key)
    rng = np.random.default_rng(11)
    N = len(nodes.names)
    for M in (1, 2, 3, 5, 8):
        members = _random_members(rng, nodes, M, 9, 13)
        has = R.has_masks(members, nodes)
        total, first = R.cells(nodes, M)
        P = M * (M - 1) // 2
        for q in R.quorums(M):
            row, labels, _ = R.count(members, nodes, R.NONE_VAL, q)
            assert row.shape == (total,)
            ended = row[:N + 1]
            votes = row[first["votes"]:first["area"]].reshape(N, M)
            area = row[first["area"]:first["both"]].reshape(M, N)
            both = row[first["both"]:first["abstain"]].reshape(P, N)
            assert int(ended.sum()) == 9 * 13
            for n, name in enumerate(nodes.names):
                assert sum((k + 1) * int(votes[n, k]) for k in range(M)) == int(area[:, n].sum()), (key, M, name)
                assert int(both[:, n].sum()) == sum(math.comb(k + 1, 2) * int(votes[n, k]) for k in range(M)), (key, M, name)
                reach = sum(has[m][n].astype(np.int64) for m in range(M)) >= q
                below = int(ended[n]) + sum(int(ended[nodes.index[d]]) for d in nodes.descendants(name))
                assert int(reach.sum()) == below, (key, M, q, name)


@pytest.mark.parametrize("key", TREE_KEYS)
def test_copies_of_one_map_give_the_map_back(key):
    _, _, _, nodes = R.setup(key)
    rng = np.random.default_rng(13)
    one = rng.choice(R.palette(nodes), size=(6, 11)).astype(np.uint8)
    known = np.isin(one, sorted(nodes.byte.values()))
    assert known.any() and not known.all()
    for M, q in [(1, 1)] + [(M, q) for M in (2, 3, 8) for q in R.quorums(M)]:
        labels, support, _ = R.vote([one] * M, nodes, R.NONE_VAL, q)
        assert np.array_equal(labels[known], one[known]) and bool((labels[~known] == R.NONE_VAL).all()), (key, M, q)
        assert bool((support[known] == M).all()) and bool((support[~known] == 0).all()), (key, M, q)


# ------------------------------------------------------------------------------------------------ the host side
@pytest.mark.parametrize("key", TREE_KEYS)
def test_tables_and_auto_assigned_bytes_are_the_hedges(key):
    from hrseg_amd.Data import DeviceConsensus, Hedge
    tree, cmap = R.TREES[key]()
    cons = DeviceConsensus(tree, cmap)
    assert cons.values == Hedge(tree, cmap, 0.0).values == R.auto_internal(tree, cmap)
    nodes = R.Nodes(tree, cmap, cons.values)
    assert cons.node_names == nodes.names
    used = set(nodes.byte.values())
    assert cons.none_val == min(v for v in range(256) if v not in used) and cons.tables.path[cons.none_val] == 0
    flat_out = [v for row in cons.out_val for v in row]
    assert flat_out == [nodes.byte[n] for n in nodes.names]
    for name in nodes.names:                                   # the path of a node's byte holds the node and its ancestors, nothing else
        e, n, on = cons.tables.path[nodes.byte[name]], name, set()
        while n is not None:
            on.add(n)
            n = nodes.parent[n]
        got = {cons.tables.names[L][((e >> (8 * L)) & 0xFF) - 1] for L in range(8) if (e >> (8 * L)) & 0xFF}
        assert got == on, name
    assert cons.resolve_quorum(1) == 1 and cons.resolve_quorum(4) == 3 and cons.resolve_quorum(5) == 3
    assert DeviceConsensus(tree, cmap, quorum=4).resolve_quorum(5) == 4
    given = {n: 200 + i for i, n in enumerate(cons.values)}
    assert DeviceConsensus(tree, cmap, internal_values=given, ignore_value=199).values == given


def test_from_hedge_takes_the_hedges_bytes():
    from hrseg_amd.Data import DeviceConsensus, Hedge
    tree, cmap = R.tl_tree()
    h = Hedge(tree, cmap, 0.4, internal_values={"tooth": 60}, reject_value=200)
    cons = DeviceConsensus.from_hedge(h, quorum=2)
    assert cons.values == {"tooth": 60} and cons.none_val == 200 and cons.quorum == 2
    assert cons.value_names[60] == "tooth" and cons.value_names[200] == "none" and cons.value_names[85] == "enamel"
    assert DeviceConsensus.from_hedge(Hedge(tree, cmap, 0.4)).none_val == 2          # 0 background, 1 tooth


def test_refusals_by_name():
    from hrseg_amd import ops
    from hrseg_amd.Data import DeviceConsensus
    from tests import score_ref as S
    tree, cmap = R.tl_tree()
    with pytest.raises(ValueError, match="ignore value and 'enamel' share the byte 85"):
        DeviceConsensus(tree, cmap, ignore_value=85)
    with pytest.raises(ValueError, match="ignore value and 'tooth' share the byte 60"):
        DeviceConsensus(tree, cmap, internal_values={"tooth": 60}, ignore_value=60)
    with pytest.raises(ValueError, match="ignore value 256 not in 0..255"):
        DeviceConsensus(tree, cmap, ignore_value=256)
    with pytest.raises(ValueError, match="'enamel', which is a leaf"):
        DeviceConsensus(tree, cmap, internal_values={"enamel": 7})
    with pytest.raises(ValueError, match="'nobody', which is no node"):
        DeviceConsensus(tree, cmap, internal_values={"nobody": 7})
    with pytest.raises(ValueError, match="share the byte 85"):
        DeviceConsensus(tree, cmap, internal_values={"tooth": 85})
    with pytest.raises(ValueError, match="9 levels"):
        DeviceConsensus(*S.chain_tree(9))
    too_wide = ({f"c{i}": {} for i in range(17)}, {f"c{i}": i for i in range(17)})
    with pytest.raises(ValueError, match="17 channels"):
        DeviceConsensus(*too_wide)
    cons = DeviceConsensus(tree, cmap)
    for M, q in ((2, 1), (3, 1), (3, 4), (4, 2), (1, 0), (8, 4)):
        with pytest.raises(ValueError, match=f"quorum {q} of {M} members"):
            ops.check_consensus(cons.tables, cons.out_val, cons.none_val, q, M)
    for M in (0, 9):
        with pytest.raises(ValueError, match=f"{M} members, supported 1..8"):
            ops.check_consensus(cons.tables, cons.out_val, cons.none_val, M, M)
    out = [list(r) for r in cons.out_val]
    out[1][0] = cons.out_val[0][1]
    with pytest.raises(ValueError, match="'upper' and 'pulp' share the byte 212"):
        ops.check_consensus(cons.tables, out, cons.none_val, 2, 3)
    with pytest.raises(ValueError, match="the none value and 'lower' share the byte 255"):
        ops.check_consensus(cons.tables, cons.out_val, 255, 2, 3)
    out[1][0] = 300
    with pytest.raises(ValueError, match="'pulp' has the output value 300"):
        ops.check_consensus(cons.tables, out, cons.none_val, 2, 3)
    # a byte whose path does not end at its node is refused when the object is built
    broken = DeviceConsensus(tree, cmap)
    broken.out_val[1][2] = 170                                  # enamel writes dentin's byte
    with pytest.raises(ValueError, match="of 'enamel' does not end at that node"):
        broken._check_tables()
    assert ops.consensus_cells(64, 8)[0] == 2889 and ops.consensus_cells(8, 3)[0] == 9 + 48 + 24 + 3
    assert ops.consensus_cells(8, 3) == R.cells(R.Nodes(tree, cmap), 3)


def test_summary_against_a_hand_computed_example():
    """2 x 3 pixels, three members, quorum 2 on the shipped tree (tooth = 1, none = 2 by the automatic rule):
       pixel   0       1       2       3      4       5
       m0      enamel  enamel  dentin  bg     upper   tooth
       m1      enamel  dentin  dentin  bg     lower   enamel
       m2      enamel  tooth   bg      bg     (none)  enamel
       vote    enamel  tooth   dentin  bg     none    enamel"""
    from hrseg_amd.Data import ConsensusLabels, DeviceConsensus
    tree, cmap = R.tl_tree()
    cons = DeviceConsensus(tree, cmap)
    assert cons.values == {"tooth": 1} and cons.none_val == 2
    bg, upper, lower, dentin, enamel, tooth = 0, 212, 255, 170, 85, 1
    members = [np.array([[enamel, enamel, dentin], [bg, upper, tooth]], np.uint8),
               np.array([[enamel, dentin, dentin], [bg, lower, enamel]], np.uint8),
               np.array([[enamel, tooth, bg], [bg, 2, enamel]], np.uint8)]
    nodes = R.Nodes(tree, cmap, cons.values)
    row, labels, support = R.count(members, nodes, cons.none_val, 2)
    assert labels.tolist() == [[enamel, tooth, dentin], [bg, 2, enamel]] and support.tolist() == [[3, 3, 2], [3, 0, 2]]
    out = ConsensusLabels(None, None, None, None, torch.from_numpy(row[None]), cons, 3)
    s = out.summary()
    assert (s["members"], s["quorum"], s["pixels"], s["none"]) == (3, 2, 6, 1)
    assert {n: r["ended"] for n, r in s["nodes"].items() if r["ended"]} == {"background": 1, "tooth": 1, "dentin": 1, "enamel": 2}
    t = s["nodes"]["tooth"]                                     # yes votes per pixel: 3 3 2 0 0 3
    assert t["voters"] == 4 and t["unanimous"] == 3 / 4 and t["mean_votes"] == 11 / 4
    assert t["kappa"] == pytest.approx(118 / 154, rel=1e-14, abs=0)
    b = s["nodes"]["background"]                                # 0 0 1 3 0 0: P = (1 + 1 + 1/3 + 1 + 1 + 1) / 6, p = 4 / 18
    assert b["unanimous"] == 1 / 2 and b["mean_votes"] == 2.0
    assert b["kappa"] == pytest.approx((8 / 9 - (16 + 196) / 324) / (1 - (16 + 196) / 324), rel=1e-14, abs=0)
    assert math.isnan(s["nodes"]["pulp"]["kappa"]) and math.isnan(s["nodes"]["pulp"]["unanimous"]), "nobody names it: no chance term"
    e01 = s["pairs"][(0, 1)]["enamel"]                          # m0: pixels 0 1, m1: pixels 0 5
    assert (e01["both"], e01["area_i"], e01["area_j"]) == (1, 2, 2)
    assert (e01["dice"], e01["iou"], e01["fn"], e01["fp"], e01["agreement"]) == (0.5, 1 / 3, 0.5, 0.5, 0.5)
    t01 = s["pairs"][(0, 1)]["tooth"]                           # both name tooth at 0 1 2 5: perfect agreement is 1, not the reference's 0
    assert (t01["both"], t01["dice"], t01["iou"], t01["fn"], t01["fp"], t01["agreement"]) == (4, 1.0, 1.0, 0.0, 0.0, 1.0)
    u02 = s["pairs"][(0, 2)]["upper"]                           # m0 once, m2 never
    assert (u02["dice"], u02["iou"], u02["fn"]) == (0.0, 0.0, 1.0) and math.isnan(u02["fp"]) and math.isnan(u02["agreement"])
    assert s["abstained"] == [0.0, 0.0, 1 / 6]
    m = out.pairwise("enamel")
    assert m["dice"].shape == (3, 3) and m["dice"][0, 1] == 0.5 == m["dice"][1, 0] and m["dice"][0, 0] == 1.0
    assert m["fn"][0, 2] == 0.5 and m["fp"][0, 2] == 0.5 and m["fn"][2, 0] == 0.5       # m2: pixels 0 5
    assert torch.equal(m["agreement"], m["agreement"].T)
    # M = 1: no kappa
    row1, _, _ = R.count(members[:1], nodes, cons.none_val, 1)
    s1 = ConsensusLabels(None, None, None, None, torch.from_numpy(row1[None]), cons, 1).summary()
    assert all(math.isnan(r["kappa"]) for r in s1["nodes"].values()) and s1["pairs"] == {}


@pytest.mark.parametrize("key", ["tl", "chain", "uniform"])
def test_consensus_maps_read_back_as_partial_label_targets(key):
    """disagreeing members -> consensus maps -> the oracle's partial-label rule with the consensus' own bytes: per pixel the
    consensus node and its ancestors are 1, everything below an internal consensus node is -1, a none pixel is -1 everywhere"""
    from hrseg_amd.Data import DeviceConsensus
    from tests import partial_ref
    tree, cmap = R.TREES[key]()
    cons = DeviceConsensus(tree, cmap)
    nodes = R.Nodes(tree, cmap, cons.values)
    rng = np.random.default_rng(17)
    vals = R.palette(nodes, extra=(cons.none_val, R.FOREIGN))
    members = [R.blob_map(rng, vals, 12, 15, block=3) for _ in range(3)]
    labels, _, ended = R.vote(members, nodes, cons.none_val, 2)
    assert len(np.unique(ended)) > 3 and (ended == len(nodes.names)).any()
    assert any(nodes.children[nodes.names[n]] for n in np.unique(ended) if n < len(nodes.names)), "no vote ended on a parent"
    rows = cmap if isinstance(cmap, list) else [dict(class_name=n, pixel_val=v) for n, v in cmap.items()]
    t = partial_ref.encode(labels[None], tree, rows, 1, internal_values=cons.values, ignore_values=[cons.none_val])[0].numpy()
    assert t.shape[0] == len(nodes.names)
    for n, name in enumerate(nodes.names):
        here = ended == n
        chain, a = [], name
        while a is not None:
            chain.append(nodes.index[a])
            a = nodes.parent[a]
        assert bool((t[chain][:, here] == 1).all()), name
        below = [nodes.index[d] for d in nodes.descendants(name)]
        if below:
            assert bool((t[below][:, here] == -1).all()), name
    assert bool((t[:, ended == len(nodes.names)] == -1).all())


def test_ops_refuses_on_the_host_before_any_launch():
    """the wrapper's own checks need no GPU: they fail on the first thing that is wrong"""
    from hrseg_amd import ops
    from hrseg_amd.Data import DeviceConsensus
    cons = DeviceConsensus(*R.tl_tree())
    with pytest.raises(ValueError, match="0 members, supported 1..8"):
        ops.consensus_labels([], cons.tables, cons.out_val, cons.none_val, 1)
    with pytest.raises(ValueError, match="9 members, supported 1..8"):
        ops.consensus_labels([None] * 9, cons.tables, cons.out_val, cons.none_val, 5)
    assert list(itertools.combinations(range(3), 2)) == [(0, 1), (0, 2), (1, 2)], "the pair order of the counters"
