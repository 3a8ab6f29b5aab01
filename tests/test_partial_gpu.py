"""Partial labels on the device (csrc/targets.hip, csrc/augment.hip, Data/dataset.py, Data/augment.py) against the torch-CPU
restatement tests/partial_ref.py: the partial entry points with an empty unknown table are the old ones bit for bit, encoded
and augmented targets with internal and ignore bytes equal the reference, the loss ignores what the encoder marks, hedged maps
come back as targets with the decode's own counts, and the launch counts stay what they were."""
import csv
import os

import numpy as np
import pytest
import torch

from tests import augment_ref as R
from tests import headloss_ref as HR
from tests import partial_ref as PR
from tests.helpers import DATA, load_tree

pytestmark = pytest.mark.gpu

S = 62
TREES = {"tl": ("class_tree_tl.json", "class_map.csv"), "ext": ("class_tree_tl_extended.json", "class_map_extended.csv")}
INTERNAL = {"tl": {"tooth": 9}, "ext": {"tooth+alveolar": 11, "alveolar": 12, "tooth": 7, "healthy": 9},
            "wide": {f"group{g}": 1 + g for g in range(4)}}
IGNORE = 254
RAGGED = [(50, 70, 3), (80, 64, 1), (62, 62, 3), (30, 100, 1)]
BLOCKS = [7, 11, 7, 11]


def _wide_tree():
    """21 nodes (17 leaves): more target channels than the shipped trees, so the wide coverage kernel runs"""
    tree, cmap, v = {"background": {}}, [{"class_name": "background", "pixel_val": "0"}], 10
    for g in range(4):
        tree[f"group{g}"] = {}
        cmap.append({"class_name": f"group{g}", "pixel_val": "None"})
        for k in range(4):
            tree[f"group{g}"][f"g{g}c{k}"] = {}
            cmap.append({"class_name": f"g{g}c{k}", "pixel_val": str(v)})
            v += 10
    return tree, cmap


def _tree(key):
    if key == "wide":
        return _wide_tree()
    t, m = TREES[key]
    with open(os.path.join(DATA, m)) as f:
        return load_tree(t), list(csv.DictReader(f))


def _source(rng, H, W, ch):
    img = rng.integers(0, 256, size=(H, W, ch)).astype(np.uint8)
    return img[..., 0] if ch == 1 else img


def _bytes(key):
    """the byte mix of the label maps: every leaf byte, every internal byte and the ignore byte"""
    _, cmap = _tree(key)
    leaves = sorted(R.name2pix(cmap).values())
    return np.array(leaves + sorted(INTERNAL[key].values()) + [IGNORE], dtype=np.uint8)


def _label(rng, H, W, key, block):
    coarse = rng.choice(_bytes(key), size=(H // block + 1, W // block + 1))
    return np.ascontiguousarray(np.repeat(np.repeat(coarse, block, 0), block, 1)[:H, :W])


def _ragged(seed, key):
    rng = np.random.default_rng(seed)
    imgs = [_source(rng, h, w, c) for h, w, c in RAGGED]
    labs = [_label(rng, h, w, key, blk) for (h, w, _), blk in zip(RAGGED, BLOCKS)]
    return imgs, labs


# ------------------------------------------------------------------------------------------------ 1. identity
@pytest.mark.parametrize("antialias", [True, False])
def test_empty_unknown_table_is_the_old_entry_points_bit_for_bit(antialias):
    from hrseg_amd import ops
    from hrseg_amd.Data import DeviceAugment, TargetEncoder, ragged_collate
    tree, cmap = _tree("ext")
    enc = TargetEncoder(tree, cmap, 1)
    zero = torch.zeros_like(enc.on_lut)
    rng = np.random.default_rng(31)
    shapes = [(50, 70), (80, 64), (30, 100)]
    labs = [_label(rng, h, w, "ext", 7) for h, w in shapes]
    imgs = [_source(rng, h, w, 1) for h, w in shapes]
    dev = ragged_collate(list(zip(imgs, labs))).to("cuda")
    aug = DeviceAugment(S, tree, cmap, 1, train=True, seed=3, vflip=True)
    from hrseg_amd.Data.augment import pack_params
    table = pack_params(aug.sample(len(shapes)), S).cuda()
    for warp in (False, True):
        want = ops.augment_targets(dev.label, dev.ldesc, dev.ldesc_host, enc.on_lut, enc.parent, table if warp else None, S, warp,
                                   antialias)
        got = ops.augment_targets_partial(dev.label, dev.ldesc, dev.ldesc_host, enc.on_lut, zero, enc.parent,
                                          table if warp else None, S, warp, antialias, False)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (warp, antialias)
    lab = torch.from_numpy(_label(rng, 37, 53, "ext", 3)[None]).cuda()
    assert torch.equal(ops.encode_targets_partial(lab, enc.on_lut, zero, enc.parent).view(torch.int32),
                       ops.encode_targets(lab, enc.on_lut, enc.parent).view(torch.int32))


# ------------------------------------------------------------------------------------------------ 2. encode
_ENCODED = {}


def _encoded(key, model_type):
    """(label [2,37,53] uint8, the reference targets), computed once per case and shared (callers must not change them)"""
    if (key, model_type) not in _ENCODED:
        tree, cmap = _tree(key)
        rng = np.random.default_rng(41)
        lab = rng.choice(np.concatenate([_bytes(key), np.array([3], dtype=np.uint8)]), size=(2, 37, 53))   # 3: an unused byte
        _ENCODED[(key, model_type)] = (lab, PR.encode(lab, tree, cmap, model_type, INTERNAL[key], [IGNORE]))
    return _ENCODED[(key, model_type)]


@pytest.mark.parametrize("model_type", [0, 1])
@pytest.mark.parametrize("key", ["tl", "ext", "wide"])
def test_encoder_with_internal_and_ignore_bytes(key, model_type):
    from hrseg_amd.Data import TargetEncoder
    tree, cmap = _tree(key)
    lab, want = _encoded(key, model_type)
    enc = TargetEncoder(tree, cmap, model_type, internal_values=INTERNAL[key], ignore_values=[IGNORE])
    got = enc(torch.from_numpy(lab).cuda()).cpu()
    assert got.shape == want.shape and torch.equal(got, want), int((got != want).sum())
    assert bool((want[:, :, lab[0] == IGNORE][0] == -1).all()) and bool((want == -1).any()) and bool((want == 1).any())


# ------------------------------------------------------------------------------------------------ 3. augment
@pytest.mark.parametrize("fill", ["reference", "ignore"])
@pytest.mark.parametrize("antialias", [True, False])
@pytest.mark.parametrize("key", ["tl", "ext", "wide"])
def test_device_augment_against_the_reference(key, antialias, fill):
    from hrseg_amd.Data import DeviceAugment
    tree, cmap = _tree(key)
    imgs, labs = _ragged(53, key)
    kw = dict(internal_values=INTERNAL[key], ignore_values=[IGNORE], fill=fill, target_antialias=antialias)
    train = DeviceAugment(S, tree, cmap, 1, train=True, seed=5, vflip=True, **kw)
    assert (len(train.names) > 16) == (key == "wide")
    params = train.sample(len(imgs))
    params["affine"][:] = True
    params["hflip"][0], params["hflip"][1], params["vflip"][1], params["vflip"][2] = True, False, True, False
    for aug, p in ((train, params), (DeviceAugment(S, tree, cmap, 1, train=False, **kw), None)):
        y = aug(imgs, labs, params=p)[1].cpu()
        excluded = near = 0
        for i in range(len(imgs)):
            yr, excl, nr = PR.augment_targets(labs[i], S, tree, cmap, 1, INTERNAL[key], [IGNORE], R.sample_dict(p, i) if p else None,
                                              antialias, fill)
            keep = ~excl[None].expand_as(yr)
            assert torch.equal(y[i][keep], yr[keep]), (key, antialias, fill, p is not None, i, int((y[i] != yr)[keep].sum()))
            excluded += int(excl.sum())
            near += int(nr.sum())
        print(f"{key} antialias={antialias} fill={fill} train={p is not None}: excluded {excluded} (near 0.5: {near}) of {len(imgs) * S * S}")
        assert excluded <= 0.005 * len(imgs) * S * S, (excluded, near)
        if p is not None and fill == "ignore":
            assert bool((y == -1).all(dim=1).any()), "the warp brought unlabelled corners in"


def test_flat_mode_through_the_augment():
    from hrseg_amd.Data import DeviceAugment
    tree, cmap = _tree("ext")
    imgs, labs = _ragged(59, "ext")
    aug = DeviceAugment(S, tree, cmap, 0, train=False, internal_values=INTERNAL["ext"], ignore_values=[IGNORE])
    y = aug(imgs, labs)[1].cpu()
    excluded = 0
    for i in range(len(imgs)):
        yr, excl, _ = PR.augment_targets(labs[i], S, tree, cmap, 0, INTERNAL["ext"], [IGNORE])
        keep = ~excl[None].expand_as(yr)
        assert torch.equal(y[i][keep], yr[keep]), i
        excluded += int(excl.sum())
    assert excluded <= 0.005 * len(imgs) * S * S


# ------------------------------------------------------------------------------------------------ 4. the loss
LEVELS_EXT = [(0, 2), (2, 4), (4, 8), (8, 11)]


@pytest.mark.parametrize("level", range(4))
def test_the_loss_ignores_what_the_encoder_marks(level):
    from hrseg_amd import ops
    from hrseg_amd.Data import TargetEncoder
    tree, cmap = _tree("ext")
    lab, _ = _encoded("ext", 1)
    enc = TargetEncoder(tree, cmap, 1, internal_values=INTERNAL["ext"], ignore_values=[IGNORE])
    lo, hi = LEVELS_EXT[level]
    t = enc(torch.from_numpy(lab).cuda())[:, lo:hi].contiguous()
    B, Cn, H, W = t.shape
    g = torch.Generator().manual_seed(70 + level)
    z = 2.0 * torch.randn(B, Cn, H, W, generator=g)
    w = [float(v) for v in (0.25 + 1.5 * torch.rand(Cn, generator=g))]
    # the fp64 evaluation of the same z and t
    z64 = HR._leaf(z, torch.float64)
    ce, dice, nvalid = HR.ce_dice(z64, t.cpu().double(), w)
    (HR.LOSS_UPSTREAM[0] * ce + HR.LOSS_UPSTREAM[1] * dice).backward()
    out, coef = ops.loss_fwd(z.cuda(), t, torch.tensor(w).cuda())
    out = out.cpu()
    dz = ops.loss_bwd(z.cuda(), t, coef, torch.tensor(HR.LOSS_UPSTREAM).cuda()).cpu()
    d_ce, d_dice, d_dz = HR.absdiff(out[0], ce.detach()), HR.absdiff(out[1], dice.detach()), HR.rel(dz, z64.grad)
    print(f"level {level}: ce {d_ce:.2e} dice {d_dice:.2e} (bar {HR.LOSS_BARS['ce']:.0e}), dz rel {d_dz:.2e} (bar {HR.LOSS_BARS['dz']:.0e})")
    dead = (t == -1).all(dim=1, keepdim=True).expand_as(t).cpu()
    assert bool(dead.any()) and not bool(dead.all())
    assert bool((dz[dead] == 0.0).all()), "a pixel whose channels are all -1 at the level gets no gradient at all"
    assert bool((z64.grad[dead] == 0.0).all())
    assert float(out[2]) == nvalid
    assert d_ce < HR.LOSS_BARS["ce"] and d_dice < HR.LOSS_BARS["dice"] and d_dz < HR.LOSS_BARS["dz"]


# ------------------------------------------------------------------------------------------------ 5. loop closure
def test_hedged_maps_come_back_as_targets_with_the_decodes_own_counts():
    from hrseg_amd.Data import DeviceDecode, Hedge, TargetEncoder
    from tests import decode_ref
    tree, cmap = _tree("ext")
    sizes = [(40, 55), (62, 62)]
    reject = 200
    h = Hedge(tree, cmap, [0.55, 0.5, 0.4, 0.35], reject_value=reject)
    logits = [z.cuda() for z in decode_ref.smooth_logits(len(sizes), list(h.tables.C), S, 17)]
    out = DeviceDecode(tree, cmap, 1).decode_hedged_sizes(logits, h, sizes)
    enc = TargetEncoder(tree, cmap, 1, internal_values=h.values, ignore_values=[h.reject_val])
    names = h.node_names
    assert names == enc.names
    kids = {n: [k for k, p in zip(names, enc.parent) if p == c] for c, n in enumerate(names)}
    nodes = len(names)
    stops = out.stops.cpu()
    for b, (off, H, W, _) in enumerate(out.desc_host.tolist()):
        t = enc(out.labels[off:off + H * W].view(H, W))[0].cpu()
        for c, n in enumerate(names):
            ends = t[c] == 1
            for k in kids[n]:
                ends &= t[names.index(k)] != 1
            assert int(ends.sum()) == int(stops[b, c]), (b, n)
        roots = [c for c, p in enumerate(enc.parent) if p < 0]
        assert int((t[roots] == -1).all(dim=0).sum()) == int(stops[b, nodes]), b
        assert int(stops[b, nodes + 1]) == 0
    total = stops.sum(0)
    for n, v in h.values.items():
        assert int(total[names.index(n)]) > 0, f"no pixel stopped at '{n}': the case does not hedge there"
    assert int(total[nodes]) > 0, "no pixel was rejected"


# ------------------------------------------------------------------------------------------------ 6. launch counts
def test_launch_counts():
    from hrseg_amd import _lib
    from hrseg_amd.Data import DeviceAugment, TargetEncoder
    tree, cmap = _tree("tl")
    rng = np.random.default_rng(67)
    imgs = [_source(rng, 40, 50, 3) for _ in range(2)]
    labs = [_label(rng, 40, 50, "tl", 5) for _ in range(2)]
    kw = dict(internal_values=INTERNAL["tl"], ignore_values=[IGNORE])
    cases = [(dict(train=True), 2), (dict(train=False), 1), (dict(train=True, **kw), 2), (dict(train=False, **kw), 1),
             (dict(train=True, fill="ignore"), 2), (dict(train=False, fill="ignore"), 1)]
    for args, per in cases:
        aug = DeviceAugment(32, tree, cmap, 1, **args)
        assert aug.partial == (len(args) > 1)
        torch.cuda.synchronize()
        _lib.launch_count(reset=True)
        _lib.launch_count("augment_targets", reset=True)
        _lib.launch_count("augment_image", reset=True)
        aug(imgs, labs)
        assert _lib.launch_count("augment_targets") == per and _lib.launch_count("augment_image") == per, args
        assert _lib.launch_count() == 0
    _lib.launch_count("augment_targets", reset=True)
    _lib.launch_count("augment_image", reset=True)
    # the default objects call the entry points they always did: no unknown table is built, no partial kernel is chosen
    enc = TargetEncoder(tree, cmap, 1)
    assert not enc.partial and enc.unk_lut is None
    assert not DeviceAugment(32, tree, cmap, 1).partial
    assert TargetEncoder(tree, cmap, 1, **kw).partial
