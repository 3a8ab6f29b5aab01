"""Device consensus (csrc/consensus.hip, Data/consensus.py, predictEval.EnsemblePredictor) against the integer numpy
reference tests/consensus_ref.py.  Every comparison is torch.equal on uint8 or int64: there is no tolerance anywhere.
Alignment of every member span and of the output span with guard bytes, a ragged batch around the block step, every member
count with the quorum at both ends of its range on three trees and three content regimes, abstentions, accumulation and
repetition, the pairwise cells against hrseg_score_labels, the ensemble wrapper, and the loop through TargetEncoder."""
import argparse
import csv
import itertools

import numpy as np
import pytest
import torch

from tests import consensus_ref as R

pytestmark = pytest.mark.gpu

_SETUPS = {}


def _setup(key):
    """(tree, class map, Nodes, DeviceConsensus) of a test tree, built once"""
    if key not in _SETUPS:
        from hrseg_amd.Data import DeviceConsensus
        tree, cmap, internal, nodes = R.setup(key)
        _SETUPS[key] = (tree, cmap, nodes, DeviceConsensus(tree, cmap, internal_values=internal, ignore_value=R.NONE_VAL))
    return _SETUPS[key]


def _place(maps, offsets, n, guard):
    """maps at the given byte offsets of an n-byte buffer filled with `guard` -> (device buffer, device desc, host desc)"""
    buf = np.full(n, guard, dtype=np.uint8)
    rows = []
    for m, off in zip(maps, offsets):
        buf[off:off + m.size] = m.reshape(-1)
        rows.append([off, m.shape[0], m.shape[1], 1])
    host = torch.tensor(rows, dtype=torch.int64)
    return torch.from_numpy(buf).cuda(), host.cuda(), host


def _dense(maps):
    offs = np.cumsum([0] + [m.size for m in maps[:-1]]).tolist()
    return _place(maps, offs, sum(m.size for m in maps), 0)


def _check(cons, nodes, batches, triples, q, per_image, what, labels=None, support=None):
    """one call on `triples` against the reference on `batches` (batches[m][b]); -> (labels, support, counts) of the device"""
    from hrseg_amd import ops
    want, wlab, wsup = R.count_batch(batches, nodes, cons.none_val, q, per_image)
    got = ops.consensus_labels(triples, cons.tables, cons.out_val, cons.none_val, q, per_image, None, True, labels, support)
    lab, sup, counts = (t.cpu() for t in got)
    assert torch.equal(counts, torch.from_numpy(want)), (what, "counters")
    for b, (off, H, W, _) in enumerate(triples[0][2].tolist()):
        assert torch.equal(lab[off:off + H * W].view(H, W), torch.from_numpy(wlab[b])), (what, b, "labels")
        assert torch.equal(sup[off:off + H * W].view(H, W), torch.from_numpy(wsup[b])), (what, b, "support")
    return lab, sup, counts


def test_every_alignment_of_every_span_with_guard_bytes():
    """one 1 x 37 image, three members: each member's span starts at every byte of a 16-byte line in turn, the others fixed.
    The outputs are packed as member 0 is, so member 0's turn moves the output span over every byte of a dword and of a
    16-byte line.  The guard bytes in front of and behind every member span hold a valid class the maps do not use: a stray
    read changes the counters.  The guard bytes around the outputs come back untouched."""
    tree, cmap, nodes, cons = _setup("tl")
    rng = np.random.default_rng(3)
    guard = 42                                                   # composite: a leaf the maps never hold
    vals = [v for v in R.palette(nodes) if v != guard]
    maps = [R.blob_map(rng, vals, 1, 37, block=3), rng.choice(vals, size=(1, 37)).astype(np.uint8), R.blob_map(rng, vals, 1, 37, block=6)]
    fixed = (5, 18, 31)
    for m in range(3):
        for start in range(16):
            offs = [start if k == m else fixed[k] for k in range(3)]
            triples = [_place([maps[k]], [offs[k]], 96, guard) for k in range(3)]
            labels = torch.full((96,), 0xAB, dtype=torch.uint8, device="cuda")
            support = torch.full((96,), 0xCD, dtype=torch.uint8, device="cuda")
            lab, sup, _ = _check(cons, nodes, [[a] for a in maps], triples, 2, True, (m, start), labels, support)
            inside = torch.zeros(96, dtype=torch.bool)
            inside[offs[0]:offs[0] + 37] = True
            assert bool((lab[~inside] == 0xAB).all()) and bool((sup[~inside] == 0xCD).all()), (m, start, "guard bytes of the outputs")


@pytest.mark.parametrize("per_image", [True, False])
def test_ragged_batch_around_the_block_step(per_image):
    """1 x 1, 1 x 17, 7 x 9, 64 x 65 and one image of exactly one pixel more than a block's step, with gaps between the maps
    and different gaps per member"""
    from hrseg_amd import ops
    tree, cmap, nodes, cons = _setup("tl")
    rng = np.random.default_rng(7)
    sizes = [(1, 1), (1, 17), (7, 9), (64, 65), (1, ops.CONSENSUS_BLOCK_STEP + 1)]
    guard = 42
    vals = [v for v in R.palette(nodes) if v != guard]
    batches = [[R.blob_map(rng, vals, H, W, block=4 + m) for H, W in sizes] for m in range(3)]
    triples = []
    for m in range(3):
        offs, off = [], 1 + 2 * m
        for H, W in sizes:
            offs.append(off)
            off += H * W + 3 + m
        triples.append(_place(batches[m], offs, off + 32, guard))
    n = triples[0][0].numel()
    labels = torch.full((n,), 0xAB, dtype=torch.uint8, device="cuda")
    lab, _, _ = _check(cons, nodes, batches, triples, 2, per_image, "ragged", labels)
    inside = torch.zeros(n, dtype=torch.bool)
    for off, H, W, _ in triples[0][2].tolist():
        inside[off:off + H * W] = True
    assert bool((lab[~inside] == 0xAB).all())


@pytest.mark.parametrize("regime", R.REGIMES)
@pytest.mark.parametrize("key", ["tl", "chain", "wide"])
def test_members_quorums_trees_and_regimes(key, regime):
    """M in {1, 2, 3, 5, 8} with the quorum at both ends of its range; the maps hold leaves, internal bytes, the none / reject
    byte and a foreign byte.  constant: every lane has the same key; blobs; salt: neighbouring tuples always differ"""
    tree, cmap, nodes, cons = _setup(key)
    rng = np.random.default_rng(len(key) * 31 + len(regime))
    vals = R.palette(nodes)
    sizes = [(5, 9), (33, 41)]
    for M in R.MEMBERS:
        batches = list(zip(*[R.member_maps(rng, regime, vals, H, W, M) for H, W in sizes]))          # [m][b]
        if regime == "salt":
            for b in range(len(sizes)):
                flat = np.stack([batches[m][b].reshape(-1) for m in range(M)], 1)
                assert bool((flat[1:] != flat[:-1]).any(1).all()), "every pixel's tuple differs from its neighbour's"
        triples = [_dense(list(batches[m])) for m in range(M)]
        for q in R.quorums(M):
            _check(cons, nodes, batches, triples, q, True, (key, regime, M, q))


def test_a_member_that_abstains_everywhere():
    tree, cmap, nodes, cons = _setup("tl")
    rng = np.random.default_rng(19)
    vals = R.palette(nodes)
    sizes = [(9, 14), (21, 30)]
    batches = [[R.blob_map(rng, vals, H, W) for H, W in sizes], [np.full((H, W), R.FOREIGN, np.uint8) for H, W in sizes],
               [R.blob_map(rng, vals, H, W, block=3) for H, W in sizes]]
    triples = [_dense(b) for b in batches]
    _, _, counts = _check(cons, nodes, batches, triples, 2, False, "abstainer")
    _, first = R.cells(nodes, 3)
    assert int(counts[0, first["abstain"] + 1]) == sum(H * W for H, W in sizes)
    _, sup, _ = _check(cons, nodes, batches, triples, 3, False, "abstainer, quorum 3")
    assert int(sup.max()) == 0, "with the quorum at M an abstainer vetoes everything"


def test_accumulation_repetition_and_one_launch_per_call():
    from hrseg_amd import _lib
    from hrseg_amd.Data import ConsensusLabels
    from hrseg_amd.Data.decode import RaggedLabels
    tree, cmap, nodes, cons = _setup("tl")
    rng = np.random.default_rng(23)
    vals = R.palette(nodes)
    sizes = [(40, 55), (62, 62)]
    first = []
    for _ in range(3):
        buf, desc, host = _dense([R.blob_map(rng, vals, H, W) for H, W in sizes])
        first.append(RaggedLabels(buf, None, desc, host))
    second = [_dense([R.blob_map(rng, vals, H, W, block=3) for H, W in sizes]) for _ in range(3)]      # triples work as well
    families = ["consensus_labels", "score_labels", None]
    start = [_lib.launch_count(f) for f in families]
    a = cons(first, per_image=True, want_support=True)
    assert [_lib.launch_count(f) - s for f, s in zip(families, start)] == [1, 0, 0], "one launch, its own family"
    assert isinstance(a, ConsensusLabels) and a.confidence is None and a.members == 3 and a.cons is cons
    again = cons(first, per_image=True, want_support=True)
    assert torch.equal(a.labels, again.labels) and torch.equal(a.support, again.support) and torch.equal(a.counts, again.counts)
    b = cons(second, per_image=True)
    assert b.support is None
    acc = cons(first, per_image=True)
    both = cons(second, per_image=True, out=acc)
    assert both.counts is acc.counts and torch.equal(both.counts, a.counts + b.counts) and torch.equal(both.labels, b.labels)
    total = cons(first)
    assert torch.equal(total.counts, a.counts.sum(0, keepdim=True))
    s = a.summary()
    assert s["pixels"] == sum(H * W for H, W in sizes) and s["members"] == 3 and s["quorum"] == 2
    assert [m.shape for m in a.unpack()] == sizes and [m.shape for m in a.unpack_support()] == sizes
    with pytest.raises(ValueError, match="member 1, sample 1: 62x61, member 0 has 62x62"):
        cons([first[0], _dense([np.zeros((40, 55), np.uint8), np.zeros((62, 61), np.uint8)]), first[2]])
    with pytest.raises(ValueError, match="out was counted over 3 members, this call has 2"):
        cons(first[:2], per_image=True, out=acc)
    with pytest.raises(ValueError, match="quorum 2 of 4 members"):
        type(cons)(tree, cmap, quorum=2)(first + first[:1])
    assert _lib.launch_count("consensus_labels") - start[0] == 6, "a refused call launches nothing"


@pytest.mark.parametrize("key", ["tl", "chain", "wide"])
def test_pairwise_cells_are_the_diagonal_of_the_label_scorer(key):
    """for every pair (i, j) and node, `both` is the diagonal cell of hrseg_score_labels(pred = member i, gt = member j) with
    the same path table: (c, c) at level 0, (c + 1, c + 1) below.  With abstentions too: the scorer drops those pixels, and
    `both` cannot count them."""
    from hrseg_amd.Data import DeviceScore
    tree, cmap, nodes, cons = _setup(key)
    rng = np.random.default_rng(29)
    vals = R.palette(nodes)
    sizes = [(17, 23), (40, 31)]
    M = 4
    triples = [_dense([R.blob_map(rng, vals, H, W, block=2 + m) for H, W in sizes]) for m in range(M)]
    out = cons(triples, per_image=False)
    assert out.cons.scorer.tables.path == cons.tables.path
    _, first = R.cells(nodes, M)
    N = len(nodes.names)
    both = out.counts[0, first["both"]:first["abstain"]].view(-1, N)
    scorer = DeviceScore(tree, cmap, internal_values=cons.values)
    assert int(both.sum()) > 0
    for p, (i, j) in enumerate(itertools.combinations(range(M), 2)):
        scores = scorer.score(triples[i], triples[j], per_image=False)
        diag = [scores.confusion(L).diagonal()[(1 if L else 0):] for L in range(len(cons.tables.C))]
        assert torch.equal(both[p], torch.cat(diag)), (key, i, j)


# ------------------------------------------------------------------------------------------------------------ end to end
def test_ensemble_predictor(tmp_path):
    from hrseg_amd import ops
    from hrseg_amd import predictEval as PE
    from hrseg_amd.Data import ConsensusLabels, DeviceConsensus, DeviceScore
    from hrseg_amd.Models import models as PM
    from hrseg_amd.Data.decode import pack_images
    from hrseg_amd.utils import synth
    from hrseg_amd.utils.config import hrnet_w48_config
    from tests.decode_harness import _source
    from tests.helpers import build_model
    tree, cmap = R.tl_tree()
    one = build_model(PM, "hrnet", True, tree, 64).cuda()
    other = synth.fill_state_dict(PM.HighResolutionNet(hrnet_w48_config(), hierarchy=tree, model_type=1), salt=1).cuda()
    args = argparse.Namespace(img_size=64, model_type=1, model_select=1)
    cons = DeviceConsensus(tree, cmap)
    members = [PE.Predictor(one, tree, cmap, args), PE.Predictor(one, tree, cmap, args, tta=PE.TestTimeAugment()),
               PE.Predictor(other, tree, cmap, args)]
    ens = PE.EnsemblePredictor(members, cons)
    rng = np.random.default_rng(41)
    imgs = [_source(rng, 50, 70, 3), _source(rng, 60, 100, 1)]
    out = ens(imgs, per_image=True, want_support=True)
    assert isinstance(out, ConsensusLabels) and [(H, W) for _, H, W, _ in out.desc_host.tolist()] == [m.shape[:2] for m in imgs]
    own = [(m.labels, m.desc, m.desc_host) for m in ens.last_members]
    assert not torch.equal(own[0][0], own[2][0]), "the second seed is another model"
    labels, support, counts = ops.consensus_labels(own, cons.tables, cons.out_val, cons.none_val, 2, True, None, True)
    assert torch.equal(out.labels, labels) and torch.equal(out.support, support) and torch.equal(out.counts, counts)
    gts = [R.blob_map(rng, sorted(R.Nodes(tree, cmap).byte.values()), 33, 47, block=8), R.blob_map(rng, [0, 85, 170], 60, 100, block=8)]
    scores = ens.score(imgs, gts)
    buf, host = pack_images(gts)
    want = DeviceScore(tree, cmap, internal_values=cons.values).score(ens.last_labels, (buf, host, host))
    assert torch.equal(scores.counts, want.counts) and torch.equal(scores.ignored, want.ignored)
    assert [(H, W) for _, H, W, _ in ens.last_labels.desc_host.tolist()] == [(33, 47), (60, 100)]
    s = out.summary()
    path = tmp_path / "metrics_consensus.csv"
    PE.write_consensus_csv(str(path), s)
    with open(path) as f:
        rows = list(csv.DictReader(f))
    nodes = [r for r in rows if r["Row"] == "node"]
    assert [r["Name"] for r in nodes] == cons.node_names and [int(r["Pixels"]) for r in nodes] == [v["ended"] for v in s["nodes"].values()]
    assert [int(r["Pixels"]) for r in rows if r["Row"] == "none"] == [s["none"]]
    pairs = [r for r in rows if r["Row"] == "pair"]
    assert len(pairs) == 3 * len(cons.node_names) and {r["Members"] for r in pairs} == {"0-1", "0-2", "1-2"}
    assert [int(r["Both"]) for r in pairs] == [v["both"] for rows_ in s["pairs"].values() for v in rows_.values()]
    assert [float(r["Abstained"]) for r in rows if r["Row"] == "member"] == s["abstained"] == [0.0, 0.0, 0.0]
    with pytest.raises(ValueError, match="0 members"):
        PE.EnsemblePredictor([], cons)


def test_three_hedged_decodes_come_back_as_targets_with_the_votes_own_counts():
    """the loop closes on the device: three hedged decodes -> consensus -> TargetEncoder(internal_values, ignore_values): per
    node, the pixels with target[n] == 1 and no child of n equal to 1 are ended[n]; the none pixels are -1 at every root"""
    from hrseg_amd.Data import DeviceConsensus, DeviceDecode, Hedge, TargetEncoder
    from tests import decode_ref
    from tests.decode_harness import _tree
    tree, cmap = _tree("ext")
    sizes = [(40, 55), (62, 62)]
    h = Hedge(tree, cmap, [0.55, 0.5, 0.4, 0.35], reject_value=200)
    dec = DeviceDecode(tree, cmap, 1)
    members = [dec.decode_hedged_sizes([z.cuda() for z in decode_ref.smooth_logits(len(sizes), list(h.tables.C), 62, seed)], h, sizes)
               for seed in (17, 18, 19)]
    cons = DeviceConsensus.from_hedge(h)
    assert cons.values == h.values and cons.none_val == h.reject_val
    out = cons(members, per_image=True)
    enc = TargetEncoder(tree, cmap, 1, internal_values=cons.values, ignore_values=[cons.none_val])
    names = cons.node_names
    assert names == enc.names
    kids = {n: [k for k, p in zip(names, enc.parent) if p == c] for c, n in enumerate(names)}
    N = len(names)
    counts = out.counts.cpu()
    for b, (off, H, W, _) in enumerate(out.desc_host.tolist()):
        t = enc(out.labels[off:off + H * W].view(H, W))[0].cpu()
        for c, n in enumerate(names):
            ends = t[c] == 1
            for k in kids[n]:
                ends &= t[names.index(k)] != 1
            assert int(ends.sum()) == int(counts[b, c]), (b, n)
        roots = [c for c, p in enumerate(enc.parent) if p < 0]
        assert int((t[roots] == -1).all(dim=0).sum()) == int(counts[b, N]), b
    total = counts.sum(0)
    assert any(int(total[names.index(n)]) > 0 for n in cons.values), "no vote ended on an internal node: the case does not disagree"
    assert int(total[N]) > 0, "no pixel went without a consensus"
