"""Device output pipeline (csrc/decode.hip, Data/decode.py, predictEval.Predictor) against the float64 torch-CPU oracle
(tests/decode_ref.py).  The kernel tests feed the SAME synthetic logits to the device and to the oracle, so they do not
depend on model numerics; the end-to-end tests apply the oracle to the logits the GPU forward itself returned.

Oracle parity is the rule of tests/decode_harness.py: labels equal outside the oracle's near-tie mask (gap of the deciding
group below 2e-4), which may cover at most 0.5 % of a case's pixels; confidence outside the mask within 4x the largest
distance of the fp32 torch-CPU evaluation of the same formula from the fp64 one on the same inputs (floor 1e-6)."""
import argparse
import os

import numpy as np
import pytest
import torch

from tests import decode_ref as R
from tests.decode_harness import RAGGED, STRIDED, _source, _tree, _wide_tree, check
from tests.helpers import build_model

pytestmark = pytest.mark.gpu


def _check(out, logits, tree, cmap, model_type, what):
    """a RaggedLabels against the oracle on the same logits (list of CPU [B,C_L,S,S]): the harness' rule on the fp64 and fp32
    evaluations of tests/decode_ref.py"""
    samples = []
    for b, (_, H, W, _) in enumerate(out.desc_host.tolist()):
        zb = [z[b] for z in logits]
        want, conf, tie, path = R.decode_sample(zb, tree, cmap, model_type, H, W)
        samples.append((want, conf, tie, path, R.decode_sample(zb, tree, cmap, model_type, H, W, dtype=torch.float32)[1]))
    check(out, samples, what)


def _run(tree, cmap, model_type, S, sizes, seed, what):
    from hrseg_amd.Data import DeviceDecode
    dec = DeviceDecode(tree, cmap, model_type)
    logits = R.smooth_logits(len(sizes), dec.tables.C, S, seed)
    out = dec.decode_sizes([z.cuda() for z in logits], sizes, want_confidence=True)
    _check(out, logits, tree, cmap, model_type, what)
    plain = dec.decode_sizes([z.cuda() for z in logits], sizes)                 # the kernel without the confidence
    assert plain.confidence is None and torch.equal(plain.labels, out.labels)
    return dec, logits, out


def test_620_to_two_panoramics_tl_tree():
    tree, cmap = _tree("tl")
    _run(tree, cmap, 1, 620, [(1400, 2900), (1400, 2900)], 0, "620->1400x2900 tl")


@pytest.mark.parametrize("model_type", [1, 0])
@pytest.mark.parametrize("key", ["tl", "ext"])
def test_ragged_up_and_downsampling_both_trees(key, model_type):
    tree, cmap = _tree(key)
    _run(tree, cmap, model_type, 62, RAGGED, 1 + model_type, f"62->ragged {key} model_type {model_type}")


@pytest.mark.parametrize("key", ["tl", "ext"])
def test_a_block_that_takes_a_second_tile(key):
    """one 4100 x 250 map: 1025 tiles for the 1024 blocks of a batch of one, so block 0 runs its tile loop twice (the logits
    of the bit-identity tests of the multi-view and window decodes at this size: seed 40 + model_type)"""
    tree, cmap = _tree(key)
    _run(tree, cmap, 1, 62, STRIDED, 41, f"62->4100x250 {key}")


def test_level_of_16_channels():
    tree, cmap = _wide_tree()
    dec, _, out = _run(tree, cmap, 1, 62, RAGGED, 5, "62->ragged wide tree")
    assert dec.tables.C == [4, 16]
    assert len(np.unique(np.concatenate([m.reshape(-1) for m in out.unpack()]))) > 8


@pytest.mark.parametrize("model_type", [1, 0])
@pytest.mark.parametrize("key", ["tl", "ext"])
def test_identity_geometry_is_exact_and_re_encodes_to_the_path(key, model_type):
    from hrseg_amd.Data import DeviceDecode, TargetEncoder
    tree, cmap = _tree(key)
    S, B = 62, 3
    dec = DeviceDecode(tree, cmap, model_type)
    logits = R.smooth_logits(B, dec.tables.C, S, 9)
    out = dec.decode_sizes([z.cuda() for z in logits], [(S, S)] * B, want_confidence=True)
    maps = out.unpack()
    target = TargetEncoder(tree, cmap, model_type)(torch.from_numpy(np.stack(maps)).cuda()).cpu()
    for b in range(B):
        want, _, tie, path = R.decode_sample([z[b] for z in logits], tree, cmap, model_type, S, S)
        assert not bool(tie.any())
        assert np.array_equal(maps[b], want.numpy())
        s = 0
        for L, n in enumerate(dec.tables.C):
            on = target[b, s:s + n] == 1
            chan = torch.where(on.any(0), on.float().argmax(0), torch.full((S, S), -1))
            assert torch.equal(chan, path[L]), (b, L)
            s += n


def test_repeatable_bitwise():
    from hrseg_amd.Data import DeviceDecode
    tree, cmap = _tree("ext")
    dec = DeviceDecode(tree, cmap, 1)
    z = [a.cuda() for a in R.smooth_logits(4, dec.tables.C, 62, 21)]
    a, b = dec.decode_sizes(z, RAGGED, True), dec.decode_sizes(z, RAGGED, True)
    assert torch.equal(a.labels, b.labels) and torch.equal(a.confidence, b.confidence)
    assert a.labels.numel() == sum(h * w for h, w in RAGGED)


def test_launch_counts():
    from hrseg_amd import _lib
    from hrseg_amd.Data import DeviceDecode
    tree, cmap = _tree("tl")
    dec = DeviceDecode(tree, cmap, 1)
    z = [a.cuda() for a in R.smooth_logits(4, dec.tables.C, 32, 2)]
    torch.cuda.synchronize()
    _lib.launch_count(reset=True)
    _lib.launch_count("decode_labels", reset=True)
    dec.decode_sizes(z, RAGGED)
    assert _lib.launch_count("decode_labels") == 1
    dec.decode_sizes(z, RAGGED, want_confidence=True)
    assert _lib.launch_count("decode_labels", reset=True) == 2
    assert _lib.launch_count() == 0, "the output pipeline issues no convolution launches"
    assert _lib.launch_count("augment_image") == 0 and _lib.launch_count("augment_targets") == 0


def test_argument_checks_raise_without_launching():
    from hrseg_amd import _lib, ops
    from hrseg_amd.Data import DeviceDecode
    from hrseg_amd.Data.decode import DecodeTables, label_desc
    tree, cmap = _tree("tl")
    dec = DeviceDecode(tree, cmap, 1)
    z = [a.cuda() for a in R.smooth_logits(2, dec.tables.C, 32, 2)]
    sizes = [(20, 30), (40, 24)]
    host = label_desc(sizes)
    _lib.launch_count("decode_labels", reset=True)
    past = host.clone()
    past[1, 0] += 1                                                # the last map would end one byte past the buffer
    with pytest.raises(ValueError, match="does not fit"):
        ops.decode_labels(z, dec.tables, past.cuda(), past)
    with pytest.raises(ValueError, match="1 logit levels for a 2-level table"):
        ops.decode_labels(z[:1], dec.tables, host.cuda(), host)
    wide = DecodeTables([17], [[-1] * 17], [[0] * 17], [list(range(17))], True)
    with pytest.raises(ValueError, match="17 channels"):
        ops.decode_labels([torch.zeros(2, 17, 32, 32, device="cuda")], wide, host.cuda(), host)
    assert _lib.launch_count("decode_labels") == 0
    # the C entry point itself refuses the same things
    import ctypes
    t = _lib.DecodeTree()
    rc = _lib._fn["hrseg_decode_labels"](1, _lib.ptr_array(z[:1]), _lib.int_array([17]), ctypes.byref(t), host.cuda().data_ptr(),
                                         z[0].data_ptr(), None, 2, 32, None)
    assert rc == -1 and "not in 1..16" in _lib.last_error()
    assert _lib.launch_count("decode_labels") == 0


# ----------------------------------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("kind,size", [("unet", 62), ("hrnet", 64)])
def test_predictor_matches_the_oracle_on_its_own_logits(kind, size, tmp_path):
    from PIL import Image
    from hrseg_amd import predictEval as PE
    from hrseg_amd.Models import models as PM
    tree, cmap = _tree("tl")
    rng = np.random.default_rng(31)
    shapes = [(50, 70, 3), (80, 64, 1), (size, size, 3)]
    imgs = [_source(rng, h, w, c) for h, w, c in shapes]
    model = build_model(PM, kind, True, tree, size).cuda()
    args = argparse.Namespace(img_size=size, model_type=1, model_select=0 if kind == "unet" else 1)
    predictor = PE.Predictor(model, tree, cmap, args, want_confidence=True, keep_logits=True)
    model.train()
    out = predictor(imgs)
    assert model.training, "the caller's mode comes back after the eval-mode forward"
    assert [(H, W) for _, H, W, _ in out.desc_host.tolist()] == [s[:2] for s in shapes]
    logits = [z.detach().float().cpu() for z in predictor.last_logits]
    _check(out, logits, tree, cmap, 1, f"predictor {kind}")
    maps = out.unpack()
    leaf_values = set(predictor.decoder.leaf_values)
    assert leaf_values == {0, 212, 255, 127, 170, 85, 42}
    assert all(set(np.unique(m).tolist()) <= leaf_values for m in maps)
    names = [f"img{i}.png" for i in range(len(maps))]
    paths = PE.save_label_maps(str(tmp_path / "labels"), names, out)
    for p, m in zip(paths, maps):
        with Image.open(p) as im:
            assert im.mode == "L" and np.array_equal(np.array(im), m)


def test_predict_loop_writes_every_label_map_and_keeps_its_metrics(tmp_path):
    from PIL import Image
    from hrseg_amd import predictEval as PE
    from hrseg_amd.Data import DeviceAugment, DeviceAugmentLoader, DeviceDecode
    from hrseg_amd.Metrics import performance_metrics as PP
    from hrseg_amd.Models import models as PM
    from hrseg_amd.utils.hierarchy import get_classes
    tree, cmap = _tree("tl")
    size = 32
    rng = np.random.default_rng(37)
    vals = np.array(DeviceDecode(tree, cmap, 1).leaf_values, dtype=np.uint8)
    data = []
    for i in range(4):
        img = _source(rng, 40 + 6 * i, 36 + 5 * i, 3 if i % 2 else 1)
        coarse = rng.choice(vals, size=(img.shape[0] // 6 + 1, img.shape[1] // 6 + 1))
        data.append((img, np.ascontiguousarray(np.repeat(np.repeat(coarse, 6, 0), 6, 1)[:img.shape[0], :img.shape[1]])))
    nc = get_classes(tree, full=True)
    args = argparse.Namespace(model_type=1, model_select=0, num_classes=nc, num_classes_full=nc, batch_size=2, img_size=size)
    model = build_model(PM, "unet", True, tree, size).cuda()
    aug = DeviceAugment(size, tree, cmap, 1, train=False)

    def run(**kw):
        loader = DeviceAugmentLoader(data, batch_size=2, augment=aug, with_sources=bool(kw))
        mets = [PP.Accuracy(), PP.Jaccardindex(), PP.DiceScore(), PP.Precision(), PP.Recall()]
        return PE.predict_loop(model, torch.device("cuda"), loader, args, tree, *mets, **kw)

    plain = run()
    label_dir = tmp_path / "maps"
    with_maps = run(label_dir=str(label_dir), class_map=cmap)
    for k in ("accuracy", "iou", "dice", "precision", "recall", "class_metrics", "performance"):
        assert plain[k] == with_maps[k], k
    files = sorted(os.listdir(label_dir))
    assert files == [f"{i:05d}.png" for i in range(4)]
    predictor = PE.Predictor(model, tree, cmap, args)                  # batches of two, as the loader forms them
    want = predictor([img for img, _ in data[:2]]).unpack() + predictor([img for img, _ in data[2:]]).unpack()
    assert predictor.last_logits is None, "logits are kept on request only"
    for f, (img, _), w in zip(files, data, want):
        with Image.open(label_dir / f) as im:
            m = np.array(im)
        assert m.shape == img.shape[:2] and set(np.unique(m).tolist()) <= set(vals.tolist())
        assert np.array_equal(m, w)
