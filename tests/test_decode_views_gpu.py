"""Test-time augmentation on the device (csrc/decode_views.hip, ops.decode_views / ops.flip_views,
Data.DeviceDecode.decode_views, predictEval.Predictor(tta=...)) against the float64 torch-CPU oracle
(tests/decode_views_ref.py) and against the single-view decode.

Oracle parity (tests/decode_harness.py): labels equal outside the oracle's near-tie mask (gap of the deciding group below 2e-4; at most 0.5 % of
a case's pixels, and tests/test_decode_views_cpu.py shows every case far below that); confidence outside the mask
within 4x the largest distance of the fp32 torch-CPU evaluation of the same formula from the fp64 one (floor 1e-6).
Bit identities need no oracle: one unflipped view IS the single-view decode, and so are flipped copies of one logit set
(mirrored taps read the same values, and the fp32 mean of 2 or 4 equal values is exact)."""
import argparse
import ctypes

import numpy as np
import pytest
import torch

from tests import decode_ref as R
from tests import decode_views_ref as V
from tests.decode_harness import EDGE, IDENTITY, STRIDED, _source, _tree, check
from tests.helpers import build_model

pytestmark = pytest.mark.gpu

FLIP_SETS = {"one": [0], "h": [0, 1], "v": [0, 2], "all": [0, 1, 2, 3]}


def _cuda(views):
    return [([z.cuda() for z in logits], f) for logits, f in views]


# -------------------------------------------------------------------------------------------------------- oracle parity
@pytest.mark.parametrize("key,model_type,vs", V.CASES)
def test_views_match_the_oracle(key, model_type, vs):
    from hrseg_amd.Data import DeviceDecode
    tree, cmap, views, samples = V.case_oracle(key, model_type, vs, _tree)
    dec = DeviceDecode(tree, cmap, model_type)
    if key == "wide":
        assert dec.tables.C == [4, 16]
    dev = _cuda(views)
    out = dec.decode_views_sizes(dev, V.RAGGED, want_confidence=True)
    check(out, samples, f"{key} model_type {model_type} views {vs}")
    plain = dec.decode_views_sizes(dev, V.RAGGED)                              # the kernel without the confidence
    assert plain.confidence is None and torch.equal(plain.labels, out.labels)


# ------------------------------------------------------------------------------------------------------- bit identities
@pytest.mark.parametrize("sizes", [V.RAGGED, EDGE, IDENTITY, STRIDED], ids=["ragged", "edge", "identity", "strided"])
@pytest.mark.parametrize("key,model_type", [("tl", 1), ("ext", 1), ("ext", 0)])
def test_one_view_and_flipped_copies_are_the_single_view_decode(key, model_type, sizes):
    from hrseg_amd.Data import DeviceDecode
    tree, cmap = _tree(key)
    dec = DeviceDecode(tree, cmap, model_type)
    z = [a.cuda() for a in R.smooth_logits(len(sizes), dec.tables.C, 62, 40 + model_type)]
    for conf in (True, False):
        ref = dec.decode_sizes(z, sizes, want_confidence=conf)
        for name, flags in FLIP_SETS.items():
            got = dec.decode_views_sizes([([V.flip(a, f).contiguous() for a in z], f) for f in flags], sizes, want_confidence=conf)
            assert torch.equal(got.labels, ref.labels), (name, conf)
            assert (got.confidence is None and ref.confidence is None) if not conf else torch.equal(got.confidence, ref.confidence), name
            assert got.desc_host.tolist() == ref.desc_host.tolist()


def test_batch_slices_of_one_forward_are_read_in_place():
    """views that are the contiguous slices z[v*B:(v+1)*B] of batched tensors decode as separately allocated ones"""
    from hrseg_amd.Data import DeviceDecode
    tree, cmap = _tree("tl")
    dec = DeviceDecode(tree, cmap, 1)
    B = len(V.RAGGED)
    parts = [R.smooth_logits(B, dec.tables.C, 62, 60 + i) for i in range(2)]
    batched = [torch.cat([p[L] for p in parts]).cuda() for L in range(2)]
    a = dec.decode_views_sizes([([z[i * B:(i + 1) * B] for z in batched], f) for i, f in enumerate((0, 3))], V.RAGGED, True)
    b = dec.decode_views_sizes([([z.cuda() for z in p], f) for p, f in zip(parts, (0, 3))], V.RAGGED, True)
    assert torch.equal(a.labels, b.labels) and torch.equal(a.confidence, b.confidence)


def test_repeatable_bitwise():
    from hrseg_amd.Data import DeviceDecode
    tree, cmap, views, _ = V.case_oracle("ext", 1, 2, _tree)
    dec = DeviceDecode(tree, cmap, 1)
    dev = _cuda(views)
    a, b = dec.decode_views_sizes(dev, V.RAGGED, True), dec.decode_views_sizes(dev, V.RAGGED, True)
    assert torch.equal(a.labels, b.labels) and torch.equal(a.confidence, b.confidence)
    assert a.labels.numel() == sum(h * w for h, w in V.RAGGED)


# ----------------------------------------------------------------------------------------------------------- flip_views
@pytest.mark.parametrize("H,W", [(62, 62), (5, 7), (1, 1), (64, 130), (6, 8), (5, 260)])
def test_flip_views_is_torch_flip(H, W):
    """62x62, 5x7, 1x1 and 64x130 rows move float by float, 6x8 and 5x260 as float4 (W % 4 == 0)"""
    from hrseg_amd import _lib, ops
    x = torch.randn(3, 3, H, W, generator=torch.Generator().manual_seed(H * 1000 + W)).cuda()
    _lib.launch_count("flip_views", reset=True)
    for flags in ([0, 1, 2, 3], [3], [2, 0, 1]):
        got = ops.flip_views(x, flags)
        assert got.shape == (len(flags) * 3, 3, H, W)
        assert torch.equal(got, torch.cat([V.flip(x, f) for f in flags]))
    assert _lib.launch_count("flip_views", reset=True) == 3


def test_flip_views_of_a_misaligned_tensor():
    """W % 4 == 0 but the data starts 4 bytes off a 16-byte boundary: no float4 moves, same result"""
    from hrseg_amd import ops
    base = torch.randn(2 * 3 * 4 * 8 + 1, generator=torch.Generator().manual_seed(5)).cuda()
    x = base[1:].view(2, 3, 4, 8)
    assert x.data_ptr() % 16 == 4 and x.is_contiguous()
    assert torch.equal(ops.flip_views(x, [1, 2]), torch.cat([V.flip(x, 1), V.flip(x, 2)]))


# ------------------------------------------------------------------------------------- launch counts, argument checks
def test_launch_counts():
    from hrseg_amd import _lib
    from hrseg_amd.Data import DeviceDecode
    tree, cmap = _tree("tl")
    dec = DeviceDecode(tree, cmap, 1)
    z = [a.cuda() for a in R.smooth_logits(4, dec.tables.C, 32, 2)]
    views = [(z, 0), ([V.flip(a, 1).contiguous() for a in z], 1)]
    torch.cuda.synchronize()
    for fam in (None, "decode_views", "decode_labels", "flip_views"):
        _lib.launch_count(fam, reset=True)
    dec.decode_views_sizes(views, V.RAGGED)
    assert _lib.launch_count("decode_views") == 1
    dec.decode_views_sizes(views, V.RAGGED, want_confidence=True)
    assert _lib.launch_count("decode_views", reset=True) == 2
    assert _lib.launch_count("decode_labels") == 0 and _lib.launch_count("flip_views") == 0
    assert _lib.launch_count() == 0, "the multi-view decode issues no convolution launches"


def test_argument_checks_raise_without_launching():
    from hrseg_amd import _lib, ops
    from hrseg_amd.Data import DeviceDecode
    from hrseg_amd.Data.decode import label_desc
    tree, cmap = _tree("tl")
    dec = DeviceDecode(tree, cmap, 1)
    z = [a.cuda() for a in R.smooth_logits(2, dec.tables.C, 32, 2)]
    host = label_desc([(20, 30), (40, 24)])
    desc = host.cuda()
    _lib.launch_count("decode_views", reset=True)
    _lib.launch_count("flip_views", reset=True)
    with pytest.raises(ValueError, match="0 views"):
        ops.decode_views([], dec.tables, desc, host)
    with pytest.raises(ValueError, match="9 views"):
        ops.decode_views([(z, 0)] * 9, dec.tables, desc, host)
    with pytest.raises(ValueError, match="flags 4"):
        ops.decode_views([(z, 0), (z, 4)], dec.tables, desc, host)
    with pytest.raises(ValueError, match="batch size 1, view 0 has 2"):
        ops.decode_views([(z, 0), ([a[:1] for a in z], 1)], dec.tables, desc, host)
    with pytest.raises(ValueError, match="level 1 logits of shape"):
        ops.decode_views([(z, 0), ([z[0], z[1][:, :, :16, :16].contiguous()], 1)], dec.tables, desc, host)
    with pytest.raises(ValueError, match="level 0 logits of shape"):
        ops.decode_views([([z[0][:, :, :, :16].contiguous(), z[1]], 0)], dec.tables, desc, host)
    with pytest.raises(ValueError, match="1 logit levels for a 2-level table"):
        ops.decode_views([(z[:1], 0)], dec.tables, desc, host)
    past = host.clone()
    past[1, 0] += 1                                                # the last map would end one byte past the buffer
    with pytest.raises(ValueError, match="does not fit"):
        ops.decode_views([(z, 0)], dec.tables, past.cuda(), past)
    with pytest.raises(ValueError, match="flags 7"):
        ops.flip_views(z[0], [0, 7])
    with pytest.raises(ValueError, match="9 views"):
        ops.flip_views(z[0], [0] * 9)
    assert _lib.launch_count("decode_views") == 0 and _lib.launch_count("flip_views") == 0
    # the C entry points themselves refuse the same things (placeholder output pointers, never written)
    dv, fv = _lib._fn["hrseg_decode_views"], _lib._fn["hrseg_flip_views"]
    t = ops._decode_tree_struct(dec.tables)
    Cs, out = _lib.int_array(dec.tables.C), torch.empty(4096, dtype=torch.uint8, device="cuda")

    def raw(nviews, S, flags, ptrs):
        return dv(nviews, _lib.int_array(S), _lib.int_array(flags), 2, _lib.ptr_array(ptrs), Cs, ctypes.byref(t), desc.data_ptr(),
                  out.data_ptr(), None, 2, None)
    assert raw(0, [32], [0], z) == -1 and "nviews=0 not in 1..8" in _lib.last_error()
    assert raw(9, [32] * 9, [0] * 9, z * 9) == -1 and "nviews=9 not in 1..8" in _lib.last_error()
    assert raw(2, [32, 32], [0, 4], z * 2) == -1 and "flags[1]=4 not in 0..3" in _lib.last_error()
    assert raw(1, [0], [0], z) == -1 and "S[0]=0 not in 1..32768" in _lib.last_error()
    assert raw(1, [32769], [0], z) == -1 and "S[0]=32769" in _lib.last_error()
    assert raw(2, [32, 32], [0, 1], z + [z[0], None]) == -1 and "view 1, level 1 has no logits" in _lib.last_error()
    assert dv(1, _lib.int_array([32]), _lib.int_array([0]), 2, _lib.ptr_array(z), Cs, ctypes.byref(t), desc.data_ptr(),
              out.data_ptr() + 1, None, 2, None) == -1 and "aligned" in _lib.last_error()
    assert dv(1, _lib.int_array([32]), _lib.int_array([0]), 1, _lib.ptr_array(z[:1]), _lib.int_array([17]), ctypes.byref(t),
              desc.data_ptr(), out.data_ptr(), None, 2, None) == -1 and "hrseg_decode_views: C[0]=17 not in 1..16" in _lib.last_error()
    assert fv(z[0].data_ptr(), out.data_ptr(), 2, _lib.int_array([0, 5]), 2, 4, 32, 32, None) == -1
    assert "flags[1]=5 not in 0..3" in _lib.last_error()
    assert fv(z[0].data_ptr(), out.data_ptr(), 0, _lib.int_array([0]), 2, 4, 32, 32, None) == -1
    assert "nviews=0 not in 1..8" in _lib.last_error()
    assert fv(z[0].data_ptr(), out.data_ptr(), 8, _lib.int_array([0] * 8), 65535, 16, 620, 620, None) == -1
    assert "at most 2^31 - 1" in _lib.last_error()
    assert _lib.launch_count("decode_views") == 0 and _lib.launch_count("flip_views") == 0


# ----------------------------------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("kind,size", [("unet", 62), ("hrnet", 64)])
def test_predictor_with_tta_end_to_end(kind, size):
    from hrseg_amd import _lib
    from hrseg_amd import predictEval as PE
    from hrseg_amd.Data import DeviceScore
    from hrseg_amd.Models import models as PM
    tree, cmap = _tree("tl")
    rng = np.random.default_rng(43)
    shapes = [(50, 70, 3), (80, 64, 1)]
    imgs = [_source(rng, h, w, c) for h, w, c in shapes]
    model = build_model(PM, kind, True, tree, size).cuda()
    args = argparse.Namespace(img_size=size, model_type=1, model_select=0 if kind == "unet" else 1)
    tta = PE.TestTimeAugment(hflip=True, vflip=True, scales=(1.0, 0.75))
    small = int(round(size * 0.75))
    assert tta.views(size) == [(size, f) for f in range(4)] + [(small, f) for f in range(4)]
    predictor = PE.Predictor(model, tree, cmap, args, want_confidence=True, keep_logits=True, tta=tta)
    seen = []
    hook = model.register_forward_pre_hook(lambda mod, inputs: seen.append(inputs[0].detach().clone()))
    model.train()
    torch.cuda.synchronize()
    for fam in (None, "decode_views", "decode_labels", "flip_views", "augment_image"):
        _lib.launch_count(fam, reset=True)
    try:
        out = predictor(imgs)
    finally:
        hook.remove()
    assert model.training, "the caller's mode comes back after the eval-mode forwards"
    assert _lib.launch_count("decode_views") == 1 and _lib.launch_count("decode_labels") == 0
    assert _lib.launch_count("flip_views") == 2 and _lib.launch_count("augment_image") == 2, "one of each per scale"
    convs = _lib.launch_count()
    assert convs > 0
    # one forward per scale, of all four flip views of the batch; the flipped inputs are torch.flip of the unflipped one
    assert [tuple(x.shape) for x in seen] == [(8, 3, size, size), (8, 3, small, small)]
    for x in seen:
        for i, f in enumerate(range(4)):
            assert torch.equal(x[2 * i:2 * i + 2], V.flip(x[:2], f)), f
    # the oracle on the logits the decode read: independent of convolution arithmetic
    assert predictor.last_logits is None
    kept = predictor.last_view_logits
    assert [f for _, f in kept] == [f for _, f in tta.views(size)]
    assert [z[0].shape[-1] for z, _ in kept] == [S for S, _ in tta.views(size)]
    views = [([z.detach().float().cpu() for z in logits], f) for logits, f in kept]
    sizes = [s[:2] for s in shapes]
    assert [(H, W) for _, H, W, _ in out.desc_host.tolist()] == sizes
    check(out, V.oracle_batch(views, tree, cmap, 1, sizes), f"predictor tta {kind}")
    again = predictor.decoder.decode_views(kept, out.desc_host, None, True)          # the decode adds no convolution launch
    assert _lib.launch_count() == convs and torch.equal(again.labels, out.labels)
    leaf_values = set(predictor.decoder.leaf_values)
    assert all(set(np.unique(m).tolist()) <= leaf_values for m in out.unpack())
    # Predictor.score goes through the same path: its counts are DeviceScore's on the maps _predict returned
    vals = np.array(sorted(leaf_values), dtype=np.uint8)
    gts = [np.ascontiguousarray(np.repeat(np.repeat(rng.choice(vals, size=(h // 6 + 1, w // 6 + 1)), 6, 0), 6, 1)[:h, :w])
           for h, w in [(50, 70), (33, 47)]]                                           # the second at a size of its own
    scores = predictor.score(imgs, gts)
    maps = predictor.last_labels
    assert [(H, W) for _, H, W, _ in maps.desc_host.tolist()] == [(50, 70), (33, 47)]
    from hrseg_amd.Data.decode import pack_images
    buf, host = pack_images(gts)
    want = DeviceScore(tree, cmap).score(maps, (buf, host, host))
    assert torch.equal(scores.counts, want.counts) and torch.equal(scores.ignored, want.ignored)
    assert int(scores.counts.sum()) > 0
    # without tta nothing changes: one decode_labels launch, no decode_views
    plain = PE.Predictor(model, tree, cmap, args)
    for fam in ("decode_views", "decode_labels", "flip_views"):
        _lib.launch_count(fam, reset=True)
    plain(imgs)
    assert _lib.launch_count("decode_labels") == 1 and _lib.launch_count("decode_views") == 0
    assert _lib.launch_count("flip_views") == 0 and plain.last_view_logits is None
