"""Device input pipeline (csrc/augment.hip, Data/augment.py, Data/loader.py) against the torch-CPU restatement of the
reference's transforms (tests/augment_ref.py), driven with identical per-sample draws."""
import numpy as np
import pytest
import torch

from tests import augment_ref as R
from tests.helpers import DATA, build_model, level_weights_for, load_tree

pytestmark = pytest.mark.gpu


def _class_map(name):
    import csv
    import os
    with open(os.path.join(DATA, name)) as f:
        return list(csv.DictReader(f))


TREES = {"tl": ("class_tree_tl.json", "class_map.csv"), "ext": ("class_tree_tl_extended.json", "class_map_extended.csv")}


def _tree(key):
    t, m = TREES[key]
    return load_tree(t), _class_map(m)


def _source(rng, H, W, ch):
    yy, xx = np.mgrid[0:H, 0:W]
    base = (96 + 80 * np.sin(xx / (7.0 + W / 40)) * np.cos(yy / (5.0 + H / 50)))[..., None]
    noise = rng.integers(-60, 61, size=(H, W, ch))
    img = np.clip(base + noise + np.array([0, 25, -25][:ch]), 0, 255).astype(np.uint8)
    return img[..., 0] if ch == 1 else img


def _label(rng, H, W, class_map, block):
    vals = np.array(sorted({int(float(r["pixel_val"])) for r in class_map if str(r["pixel_val"]) not in ("None", "")}),
                    dtype=np.uint8)
    coarse = rng.choice(vals, size=(H // block + 1, W // block + 1))
    return np.ascontiguousarray(np.repeat(np.repeat(coarse, block, 0), block, 1)[:H, :W])


def _compare(aug, imgs, labs, tree, cmap, model_type, params, train, antialias=True):
    S = aug.size
    x, y = aug(imgs, labs, params=params)
    x, y = x.cpu(), y.cpu()
    excluded = total = 0
    for i in range(len(imgs)):
        p = R.sample_dict(params, i) if train else None
        xr, yr, tie, excl = R.augment_sample(imgs[i], labs[i], S, tree, cmap, model_type, p, target_antialias=antialias)
        dx = (x[i] - xr).abs().masked_fill(tie[None], 0)
        assert float(dx.max()) <= 2e-5, (i, float(dx.max()))
        keep = ~excl[None].expand_as(yr)
        assert torch.equal(y[i][keep], yr[keep]), (i, int((y[i] != yr)[keep].sum()))
        excluded += int(excl.sum())
        total += S * S
    assert excluded <= 0.005 * total, (excluded, total)
    return x, y


def _augment(S, key, model_type, train, seed=0, **kw):
    from hrseg_amd.Data.augment import DeviceAugment
    tree, cmap = _tree(key)
    return DeviceAugment(S, tree, cmap, model_type, train=train, seed=seed, **kw), tree, cmap


def test_downsampling_620_three_channels_train_and_eval():
    rng = np.random.default_rng(0)
    tree, cmap = _tree("tl")
    imgs = [_source(rng, 1400, 2900, 3) for _ in range(2)]
    labs = [_label(rng, 1400, 2900, cmap, 50) for _ in range(2)]
    aug, tree, cmap = _augment(620, "tl", 1, True, seed=1)
    params = aug.sample(2)
    params["affine"][:] = True
    params["hflip"][0], params["hflip"][1] = True, False
    _compare(aug, imgs, labs, tree, cmap, 1, params, True)
    ev, _, _ = _augment(620, "tl", 1, False)
    _compare(ev, imgs, labs, tree, cmap, 1, None, False)


@pytest.mark.parametrize("model_type", [0, 1])
def test_upsampling_one_channel_both_trees(model_type):
    rng = np.random.default_rng(1 + model_type)
    for key in ("tl", "ext"):
        aug, tree, cmap = _augment(62, key, model_type, True, seed=3)
        imgs = [_source(rng, 50, 70, 1) for _ in range(2)]
        labs = [_label(rng, 50, 70, cmap, 7) for _ in range(2)]
        params = aug.sample(2)
        params["hflip"][0] = True
        _compare(aug, imgs, labs, tree, cmap, model_type, params, True)
        ev, _, _ = _augment(62, key, model_type, False)
        _compare(ev, imgs, labs, tree, cmap, model_type, None, False)


@pytest.mark.parametrize("antialias", [True, False])
def test_ragged_batch_mixing_sizes_and_channels(antialias):
    rng = np.random.default_rng(7)
    aug, tree, cmap = _augment(62, "ext", 1, True, seed=5, target_antialias=antialias, vflip=True)
    shapes = [(50, 70, 3), (80, 64, 1), (62, 62, 3), (30, 100, 1)]
    imgs = [_source(rng, h, w, c) for h, w, c in shapes]
    labs = [_label(rng, h, w, cmap, 11) for h, w, _ in shapes]
    params = aug.sample(len(shapes))
    params["vflip"][1] = True
    _compare(aug, imgs, labs, tree, cmap, 1, params, True, antialias)
    ev, _, _ = _augment(62, "ext", 1, False, target_antialias=antialias)
    _compare(ev, imgs, labs, tree, cmap, 1, None, False, antialias)


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


@pytest.mark.parametrize("model_type", [0, 1])
def test_more_than_16_target_channels(model_type):
    from hrseg_amd.Data.augment import DeviceAugment
    tree, cmap = _wide_tree()
    rng = np.random.default_rng(23 + model_type)
    shapes = [(50, 70, 3), (70, 44, 1)]
    imgs = [_source(rng, h, w, c) for h, w, c in shapes]
    labs = [_label(rng, h, w, cmap, 9) for h, w, _ in shapes]
    aug = DeviceAugment(62, tree, cmap, model_type, train=True, seed=7)
    assert len(aug.names) > 16
    _compare(aug, imgs, labs, tree, cmap, model_type, aug.sample(2), True)
    _compare(DeviceAugment(62, tree, cmap, model_type, train=False), imgs, labs, tree, cmap, model_type, None, False)


@pytest.mark.parametrize("model_type", [0, 1])
def test_identity_geometry_targets_equal_target_encoder(model_type):
    from hrseg_amd.Data import TargetEncoder
    rng = np.random.default_rng(11)
    S = 62
    tree, cmap = _tree("ext")
    labs = [_label(rng, S, S, cmap, 3) for _ in range(3)]
    imgs = [_source(rng, S, S, 3) for _ in range(3)]
    want = TargetEncoder(tree, cmap, model_type)(torch.from_numpy(np.stack(labs)).cuda()).cpu()
    ev, _, _ = _augment(S, "ext", model_type, False)
    assert torch.equal(ev(imgs, labs)[1].cpu(), want)
    tr, _, _ = _augment(S, "ext", model_type, True, hflip=False, affine=False)
    params = tr.sample(3)
    assert not bool(params["hflip"].any()) and not bool(params["affine"].any())
    assert torch.equal(tr(imgs, labs, params=params)[1].cpu(), want)


def test_same_seed_repeats_bitwise_and_seeds_differ():
    rng = np.random.default_rng(13)
    imgs = [_source(rng, 90, 120, 3), _source(rng, 70, 60, 1)]
    tree, cmap = _tree("tl")
    labs = [_label(rng, 90, 120, cmap, 9), _label(rng, 70, 60, cmap, 9)]
    outs = []
    for seed in (4, 4, 5):
        aug, _, _ = _augment(64, "tl", 1, True, seed=seed)
        outs.append([t.cpu() for t in aug(imgs, labs)] + [t.cpu() for t in aug(imgs, labs)])
    assert all(torch.equal(a, b) for a, b in zip(outs[0], outs[1]))
    assert not torch.equal(outs[0][0], outs[2][0])
    assert not torch.equal(outs[0][0], outs[0][2])          # the next batch of one stream draws anew


def test_launch_counts_per_batch():
    from hrseg_amd import _lib
    rng = np.random.default_rng(17)
    tree, cmap = _tree("tl")
    imgs = [_source(rng, 40, 50, 3) for _ in range(2)]
    labs = [_label(rng, 40, 50, cmap, 5) for _ in range(2)]
    for train, per in ((True, 2), (False, 1)):
        aug, _, _ = _augment(32, "tl", 1, train)
        torch.cuda.synchronize()
        _lib.launch_count(reset=True)
        aug(imgs, labs)
        assert _lib.launch_count("augment_image") == per and _lib.launch_count("augment_targets") == per
        assert _lib.launch_count() == 0, "the input pipeline issues no convolution launches"
        _lib.launch_count("augment_image", reset=True)
        _lib.launch_count("augment_targets", reset=True)


def test_train_epoch_through_the_device_loader():
    import argparse
    from hrseg_amd import train as PT
    from hrseg_amd.Data import DeviceAugmentLoader
    from hrseg_amd.Metrics import losses as PL
    from hrseg_amd.Metrics import performance_metrics as PP
    from hrseg_amd.Models import models as PM
    from hrseg_amd.utils.hierarchy import get_classes
    rng = np.random.default_rng(19)
    tree, cmap = _tree("tl")
    data = [(_source(rng, 48 + 8 * i, 40 + 4 * i, 3 if i % 2 else 1), None) for i in range(4)]
    data = [(img, _label(rng, img.shape[0], img.shape[1], cmap, 6)) for img, _ in data]
    aug, _, _ = _augment(32, "tl", 1, True, seed=2)
    loader = DeviceAugmentLoader(data, batch_size=2, shuffle=True, num_workers=0, augment=aug)
    nc = get_classes(tree, full=True)
    args = argparse.Namespace(model_type=1, model_select=0, num_classes=nc,
                              level_weights=level_weights_for("class_tree_tl.json", True), level0_pretrain_epochs=None,
                              batch_size=2)
    model = build_model(PM, "unet", True, tree, 32).cuda()
    opt = PT.FusedAdamW(model, lr=[1e-4])
    fns = [[PL.CrossEntropyLoss(), PL.SoftDiceLoss(num_classes=n)] for n in nc]
    mets = [PP.Accuracy(), PP.Jaccardindex(), PP.DiceScore(), PP.Precision(), PP.Recall()]
    out = PT.train_epoch(model, torch.device("cuda"), loader, opt, 1, fns, args, tree, None, *mets, epoch_num=1)
    assert len(loader) == 2 and np.isfinite(out[0]) and all(np.isfinite(v) for v in out[7])
    for xb, yb in loader:               # leaving an epoch early stops its producer thread
        assert xb.is_cuda and xb.shape == (2, 3, 32, 32) and yb.shape == (2, len(aug.names), 32, 32)
        break
    torch.cuda.synchronize()
