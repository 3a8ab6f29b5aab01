"""Sliding-window inference on the device (csrc/windows.hip, ops.window_crops / ops.decode_windows,
Data.DeviceDecode.decode_windows, predictEval.Predictor(window=...)) against the float64 torch-CPU oracle
(tests/window_ref.py), against the single-window decode and against the eval-mode resize.

Oracle parity is the rule of tests/decode_harness.py: labels equal outside the oracle's near-tie mask (gap of the
deciding group below 2e-4; at most 0.5 % of a call's pixels, and tests/test_decode_windows_cpu.py shows every call far below
that); confidence outside the mask within 4x the largest distance of the fp32 torch-CPU evaluation of the same formula from the
fp64 one (floor 1e-6).  Bit identities need no oracle: one window per image with the all-ones profile IS the single-window
decode, and one window on a canvas of its own size IS the eval-mode resize."""
import argparse
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import decode_ref as R
from tests import window_ref as WR
from tests.decode_harness import EDGE, IDENTITY, RAGGED, STRIDED, _source, _tree, check
from tests.helpers import build_model

pytestmark = pytest.mark.gpu


def _plan(canvases, S, overlap):
    from hrseg_amd.Data.decode import plan_windows
    return plan_windows(canvases, S, WR.stride_of(S, overlap))


# -------------------------------------------------------------------------------------------------------- oracle parity
@pytest.mark.parametrize("key,model_type,overlap,blend", WR.CASES)
def test_windows_match_the_oracle(key, model_type, overlap, blend):
    from hrseg_amd.Data import DeviceDecode
    tree, cmap, calls = WR.case_oracle(key, model_type, overlap, blend, _tree)
    dec = DeviceDecode(tree, cmap, model_type)
    if key == "wide":
        assert dec.tables.C == [4, 16]
    prof = WR.profile(WR.S, blend)
    for batch, ((canvases, sizes), (logits, samples)) in enumerate(zip(WR.BATCHES, calls)):
        plan = _plan(canvases, WR.S, overlap)
        assert plan.nwindows == logits[0].shape[0] and plan.first_window(3) > 3, "four images per call: the n0 offsets matter"
        dev = [z.cuda() for z in logits]
        out = dec.decode_windows_sizes(dev, plan, prof, sizes, want_confidence=True)
        check(out, samples, f"{key} model_type {model_type} overlap {overlap} {blend} call {batch}")
        plain = dec.decode_windows_sizes(dev, plan, prof, sizes)                    # the kernel without the confidence
        assert plain.confidence is None and torch.equal(plain.labels, out.labels)


# ------------------------------------------------------------------------------------------------------- bit identities
@pytest.mark.parametrize("sizes", [RAGGED, EDGE, IDENTITY, STRIDED], ids=["ragged", "edge", "identity", "strided"])
@pytest.mark.parametrize("key,model_type", [("tl", 1), ("ext", 1), ("ext", 0)])
def test_one_window_with_the_uniform_profile_is_the_single_window_decode(key, model_type, sizes):
    from hrseg_amd.Data import DeviceDecode
    tree, cmap = _tree(key)
    dec = DeviceDecode(tree, cmap, model_type)
    z = [a.cuda() for a in R.smooth_logits(len(sizes), dec.tables.C, 62, 40 + model_type)]
    plan = _plan([(62, 62)] * len(sizes), 62, 0.5)
    assert plan.nwindows == len(sizes)
    for conf in (True, False):
        ref = dec.decode_sizes(z, sizes, want_confidence=conf)
        got = dec.decode_windows_sizes(z, plan, torch.ones(62), sizes, want_confidence=conf)
        assert torch.equal(got.labels, ref.labels), conf
        assert (got.confidence is None and ref.confidence is None) if not conf else torch.equal(got.confidence, ref.confidence)
        assert got.desc_host.tolist() == ref.desc_host.tolist()


@pytest.mark.parametrize("blend", WR.BLENDS)
@pytest.mark.parametrize("overlap", WR.OVERLAPS)
def test_windows_cut_from_one_field_decode_as_the_field(overlap, blend):
    """windows cut on the device from one [C, Hc, Wc] logit field per image: outside near ties the labels are those of the
    field itself (the oracle's walk on the resized field), whatever the profile"""
    from hrseg_amd.Data import DeviceDecode
    tree, cmap = _tree("ext")
    dec = DeviceDecode(tree, cmap, 1)
    pairs = [((50, 70), (50, 70)), ((80, 64), (33, 47)), ((64, 64), (90, 100)), ((32, 100), (32, 100))]
    canvases, sizes = [c for c, _ in pairs], [s for _, s in pairs]
    plan = _plan(canvases, WR.S, overlap)
    fields = [[R.smooth_logits(1, [n], max(Hc, Wc), 80 + i, coarse=12)[0][0][:, :Hc, :Wc].contiguous() for n in dec.tables.C]
              for i, (Hc, Wc) in enumerate(canvases)]
    wins = []
    for L in range(len(dec.tables.C)):
        per_image = []
        for m, f in enumerate(fields):
            ys, xs = plan.axes(m)
            g = f[L].cuda()
            per_image.append(torch.stack([g[:, y0:y0 + WR.S, x0:x0 + WR.S] for y0 in ys for x0 in xs]))
        wins.append(torch.cat(per_image).contiguous())
    out = dec.decode_windows_sizes(wins, plan, WR.profile(WR.S, blend), sizes, want_confidence=True)
    maps, confs = out.unpack(), out.unpack_confidence()
    for m, (H, W) in enumerate(sizes):
        want, conf, tie, _ = WR.walk(WR.resize([f.double() for f in fields[m]], H, W), tree, cmap, 1)
        wrong = int(((torch.from_numpy(maps[m]) != want) & ~tie).sum())
        dconf = float((torch.from_numpy(confs[m]).double() - conf).abs()[~tie].max())
        print(f"overlap {overlap} {blend} image {m}: {int(tie.sum())} near ties of {H * W}, {wrong} labels differ outside them, "
              f"confidence within {dconf:.3e}")
        assert wrong == 0 and int(tie.sum()) <= WR.MASK_CAP * H * W


def test_repeatable_bitwise():
    from hrseg_amd.Data import DeviceDecode
    tree, cmap, calls = WR.case_oracle("ext", 1, 0.5, "hann", _tree)
    dec = DeviceDecode(tree, cmap, 1)
    canvases, sizes = WR.BATCHES[0]
    plan, prof = _plan(canvases, WR.S, 0.5), WR.profile(WR.S, "hann")
    dev = [z.cuda() for z in calls[0][0]]
    a, b = dec.decode_windows_sizes(dev, plan, prof, sizes, True), dec.decode_windows_sizes(dev, plan, prof, sizes, True)
    assert torch.equal(a.labels, b.labels) and torch.equal(a.confidence, b.confidence)
    assert a.labels.numel() == sum(h * w for h, w in sizes)


# --------------------------------------------------------------------------------------------------------- window_crops
CROP_SOURCES = [(50, 70, 3), (80, 64, 1), (20, 100, 3)]


def _packed(shapes, seed):
    from hrseg_amd.Data.decode import pack_images
    rng = np.random.default_rng(seed)
    imgs = [_source(rng, h, w, c) for h, w, c in shapes]
    src, host = pack_images(imgs)
    return imgs, src.cuda(), host.cuda(), host


def test_one_window_on_a_canvas_of_its_size_is_the_eval_resize():
    from hrseg_amd import ops
    _, src, desc, host = _packed(CROP_SOURCES, 7)
    for S in (32, 37):
        plan = _plan([(S, S)] * len(CROP_SOURCES), S, 0.5)
        assert torch.equal(ops.window_crops(src, desc, host, plan, S), ops.augment_image(src, desc, host, None, S, False))


@pytest.mark.parametrize("scale", [1.0, 0.5, 1.5])
def test_crops_are_slices_of_the_resized_source(scale):
    """against F.interpolate of src / 255 to the canvas, sliced and normalised, within 2e-5: the bar tests/test_augment_gpu.py
    holds image values to"""
    from hrseg_amd import ops
    from hrseg_amd.predictEval import SlidingWindow
    imgs, src, desc, host = _packed(CROP_SOURCES, 11)
    S = 32
    plan = SlidingWindow(overlap=0.5, scale=scale).plan([s[:2] for s in CROP_SOURCES], S)
    x = ops.window_crops(src, desc, host, plan, S).cpu()
    assert x.shape == (plan.nwindows, 3, S, S)
    worst = 0.0
    for m, img in enumerate(imgs):
        Hc, Wc = plan.canvas(m)
        assert (Hc, Wc) == (max(S, int(round(img.shape[0] * scale))), max(S, int(round(img.shape[1] * scale))))
        t = torch.from_numpy(img).float().div(255.0)
        t = t[None].expand(3, -1, -1) if t.dim() == 2 else t.permute(2, 0, 1)
        canvas = (F.interpolate(t[None], size=(Hc, Wc), mode="bilinear", align_corners=False, antialias=False)[0] - 0.5) / 0.5
        ys, xs = plan.axes(m)
        for a, y0 in enumerate(ys):
            for b, x0 in enumerate(xs):
                got = x[plan.first_window(m) + a * len(xs) + b]
                worst = max(worst, float((got - canvas[:, y0:y0 + S, x0:x0 + S]).abs().max()))
    print(f"scale {scale}: {plan.nwindows} windows, largest distance from the sliced resize {worst:.3e}")
    assert worst <= 2e-5


# ------------------------------------------------------------------------------------- launch counts, argument checks
FAMILIES = (None, "window_crops", "decode_windows", "decode_labels", "decode_views", "augment_image")


def test_launch_counts():
    from hrseg_amd import _lib, ops
    from hrseg_amd.Data import DeviceDecode
    tree, cmap = _tree("tl")
    dec = DeviceDecode(tree, cmap, 1)
    canvases, sizes = WR.BATCHES[0]
    plan, prof = _plan(canvases, WR.S, 0.5), WR.profile(WR.S, "hann")
    z = [a.cuda() for a in R.smooth_logits(plan.nwindows, dec.tables.C, WR.S, 2)]
    _, src, desc, host = _packed([(h, w, 3) for h, w in canvases], 3)
    torch.cuda.synchronize()
    for fam in FAMILIES:
        _lib.launch_count(fam, reset=True)
    dec.decode_windows_sizes(z, plan, prof, sizes)
    assert _lib.launch_count("decode_windows") == 1
    dec.decode_windows_sizes(z, plan, prof, sizes, want_confidence=True)
    assert _lib.launch_count("decode_windows") == 2 and _lib.launch_count("window_crops") == 0
    ops.window_crops(src, desc, host, plan, WR.S)
    assert _lib.launch_count("window_crops") == 1 and _lib.launch_count("decode_windows") == 2
    assert _lib.launch_count("decode_labels") == 0 and _lib.launch_count("decode_views") == 0
    assert _lib.launch_count("augment_image") == 0
    assert _lib.launch_count() == 0, "neither kernel counts as a convolution launch"


def test_argument_checks_raise_without_launching():
    from hrseg_amd import _lib, ops
    from hrseg_amd.Data import DeviceDecode
    from hrseg_amd.Data.decode import WindowPlan, label_desc
    tree, cmap = _tree("tl")
    dec = DeviceDecode(tree, cmap, 1)
    canvases = [(50, 70), (80, 64)]
    plan, prof = _plan(canvases, 32, 0.5), torch.ones(32)
    N = plan.nwindows
    z = [a.cuda() for a in R.smooth_logits(N, dec.tables.C, 32, 2)]
    host = label_desc([(20, 30), (40, 24)])
    desc = host.cuda()
    _, src, sdesc, shost = _packed([(50, 70, 3), (80, 64, 1)], 5)
    for fam in ("window_crops", "decode_windows"):
        _lib.launch_count(fam, reset=True)

    def bad_plan(image, entry, value=None, origins=None, nwindows=None):
        wd = plan.wdesc.clone()
        if value is not None:
            wd[image, entry] = value
        return WindowPlan(wd, plan.origins if origins is None else torch.tensor(origins, dtype=torch.int32),
                          N if nwindows is None else nwindows, 32)
    org = plan.origins.tolist()
    assert org[:3] == [0, 16, 18]
    refused = [(bad_plan(0, 0, origins=[1] + org[1:]), "do not run from 0"),
               (bad_plan(0, 0, origins=[0, 16, 17] + org[3:]), "do not run from 0"),
               (bad_plan(0, 0, origins=[0, 18, 18] + org[3:]), "not increasing"),
               (bad_plan(1, 0, 81), "do not run from 0"),                              # a gap at the canvas' end
               (bad_plan(0, 2, 65), "supported 1..64 per axis"),
               (bad_plan(1, 4, 13), "are not inside"),
               (bad_plan(1, 5, len(org)), "lie outside the table"),
               (bad_plan(0, 0, 31), "smaller than a window"),
               (bad_plan(0, 0, nwindows=1), "1 windows for 2 images")]
    for p, msg in refused:
        with pytest.raises(ValueError, match=msg):
            ops.window_crops(src, sdesc, shost, p, 32)
        if p.nwindows == N:
            with pytest.raises(ValueError, match=msg):
                ops.decode_windows(z, dec.tables, p, prof, desc, host)
    with pytest.raises(ValueError, match="more than 3 windows"):
        ops.check_window_axis("t", [0, 8, 16, 24, 40], 72, 32)
    with pytest.raises(ValueError, match="made for windows of 32, not 31"):
        ops.window_crops(src, sdesc, shost, plan, 31)
    with pytest.raises(ValueError, match="logits of 23 windows for a plan of 24"):
        ops.decode_windows([a[:23] for a in z], dec.tables, plan, prof, desc, host)
    with pytest.raises(ValueError, match="level 1 logits of shape"):
        ops.decode_windows([z[0], z[1][:, :, :16, :16].contiguous()], dec.tables, plan, prof, desc, host)
    with pytest.raises(ValueError, match="1 logit levels for a 2-level table"):
        ops.decode_windows(z[:1], dec.tables, plan, prof, desc, host)
    with pytest.raises(ValueError, match="fp32 device tensors"):
        ops.decode_windows([z[0], z[1].double()], dec.tables, plan, prof, desc, host)
    for p, msg in ((torch.ones(31), "32 entries"), (torch.ones(32, dtype=torch.float64), "fp32 tensor"),
                   (torch.cat([torch.ones(31), torch.zeros(1)]), "strictly positive"),
                   (torch.cat([torch.ones(31), -torch.ones(1)]).cuda(), "strictly positive"),
                   (torch.cat([torch.ones(31), torch.tensor([float("nan")])]), "strictly positive")):
        with pytest.raises(ValueError, match=msg):
            ops.decode_windows(z, dec.tables, plan, p, desc, host)
    past = host.clone()
    past[1, 0] += 1                                                # the last map would end one byte past the buffer
    with pytest.raises(ValueError, match="does not fit"):
        ops.decode_windows(z, dec.tables, plan, prof, past.cuda(), past)
    assert _lib.launch_count("window_crops") == 0 and _lib.launch_count("decode_windows") == 0
    # the C entry points themselves refuse what they can see (placeholder output pointers, never written)
    dw, wc = _lib._fn["hrseg_decode_windows"], _lib._fn["hrseg_window_crops"]
    t = ops._decode_tree_struct(dec.tables)
    Cs, out = _lib.int_array(dec.tables.C), torch.empty(4096, dtype=torch.uint8, device="cuda")
    wdesc, origins, dprof = plan.wdesc.cuda(), plan.origins.cuda(), prof.cuda()

    def raw(nlevels=2, ptrs=z, Cv=Cs, wd=wdesc.data_ptr(), og=origins.data_ptr(), pf=dprof.data_ptr(), ds=desc.data_ptr(),
            lab=out.data_ptr(), cf=None, B=2, S=32, nw=N):
        return dw(nlevels, _lib.ptr_array(ptrs), Cv, ctypes.byref(t), wd, og, pf, ds, lab, cf, B, S, nw, None)
    for kw, msg in ((dict(S=0), "S=0 not in 1..32768"), (dict(S=32769), "S=32769 not in 1..32768"),
                    (dict(nw=1), "1 windows for 2 images"), (dict(B=0), "B=0 not in 1..65535"),
                    (dict(wd=None), "NULL argument"), (dict(og=None), "NULL argument"), (dict(pf=None), "NULL argument"),
                    (dict(ds=None), "NULL argument"), (dict(lab=None), "NULL argument"),
                    (dict(lab=out.data_ptr() + 1), "aligned"), (dict(cf=out.data_ptr() + 4), "aligned"),
                    (dict(nlevels=0), "nlevels=0 not in 1..8"), (dict(nlevels=9), "nlevels=9 not in 1..8"),
                    (dict(ptrs=[z[0], None]), "level 1 has no logits"),
                    (dict(nlevels=1, ptrs=z[:1], Cv=_lib.int_array([17])), "hrseg_decode_windows: C[0]=17 not in 1..16")):
        assert raw(**kw) == -1 and msg in _lib.last_error(), (kw, _lib.last_error())
    x = torch.empty(16, device="cuda")

    def raw_crops(s=src.data_ptr(), ds=sdesc.data_ptr(), wd=wdesc.data_ptr(), og=origins.data_ptr(), xo=x.data_ptr(), B=2, S=32, nw=N):
        return wc(s, ds, wd, og, xo, B, S, nw, None)
    for kw, msg in ((dict(S=0), "S=0 not in 1..32768"), (dict(S=32769), "S=32769"), (dict(nw=1), "1 windows for 2 images"),
                    (dict(B=65536), "B=65536 not in 1..65535"), (dict(s=None), "NULL argument"), (dict(ds=None), "NULL argument"),
                    (dict(wd=None), "NULL argument"), (dict(og=None), "NULL argument"), (dict(xo=None), "NULL argument")):
        assert raw_crops(**kw) == -1 and msg in _lib.last_error(), (kw, _lib.last_error())
    assert _lib.launch_count("window_crops") == 0 and _lib.launch_count("decode_windows") == 0


def test_window_and_tta_together_are_refused():
    from hrseg_amd import predictEval as PE
    tree, cmap = _tree("tl")
    args = argparse.Namespace(img_size=32, model_type=1, model_select=0)
    with pytest.raises(ValueError, match="window together with tta"):
        PE.Predictor(torch.nn.Identity(), tree, cmap, args, tta=PE.TestTimeAugment(), window=PE.SlidingWindow())


# ----------------------------------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("kind,size", [("unet", 62), ("hrnet", 64)])
def test_predictor_with_windows_end_to_end(kind, size):
    from hrseg_amd import _lib, ops
    from hrseg_amd import predictEval as PE
    from hrseg_amd.Data import DeviceScore
    from hrseg_amd.Data.decode import pack_images
    from hrseg_amd.Models import models as PM
    tree, cmap = _tree("tl")
    rng = np.random.default_rng(47)
    shapes = [(100, 150, 3), (70, 62, 1)]
    imgs = [_source(rng, h, w, c) for h, w, c in shapes]
    model = build_model(PM, kind, True, tree, size).cuda()
    args = argparse.Namespace(img_size=size, model_type=1, model_select=0 if kind == "unet" else 1)
    window = PE.SlidingWindow(overlap=0.5, window_batch=8)
    predictor = PE.Predictor(model, tree, cmap, args, want_confidence=True, keep_logits=True, window=window)
    seen = []
    hook = model.register_forward_pre_hook(lambda mod, inputs: seen.append(inputs[0].detach().clone()))
    model.train()
    torch.cuda.synchronize()
    for fam in FAMILIES:
        _lib.launch_count(fam, reset=True)
    try:
        out = predictor(imgs)
    finally:
        hook.remove()
    assert model.training, "the caller's mode comes back after the eval-mode forwards"
    assert _lib.launch_count("window_crops") == 1 and _lib.launch_count("decode_windows") == 1
    assert _lib.launch_count("decode_labels") == 0 and _lib.launch_count("decode_views") == 0
    assert _lib.launch_count("augment_image") == 0
    convs = _lib.launch_count()
    assert convs > 0
    # 3 x 4 windows of the first image and 2 x 1 of the second, in forwards of 8 and 6 that are the crops
    logits, plan = predictor.last_window_logits
    assert plan.wdesc[:, :5].tolist() == [[100, 150, 3, 4, 0], [70, max(size, 62), 2, 1, 12]] and plan.nwindows == 14
    assert [tuple(x.shape) for x in seen] == [(8, 3, size, size), (6, 3, size, size)]
    src, host = pack_images(imgs)
    crops = ops.window_crops(src.cuda(), host.cuda(), host, plan, size)
    assert torch.equal(torch.cat(seen), crops)
    # the oracle on the logits the decode read: independent of convolution arithmetic
    assert predictor.last_logits is None and predictor.last_view_logits is None
    assert [tuple(z.shape) for z in logits] == [(14, n, size, size) for n in predictor.decoder.tables.C]
    cpu = [z.detach().float().cpu() for z in logits]
    sizes = [s[:2] for s in shapes]
    canvases = [plan.canvas(m) for m in range(2)]
    assert [(H, W) for _, H, W, _ in out.desc_host.tolist()] == sizes
    stride, prof = WR.stride_of(size, 0.5), WR.profile(size, "hann")
    check(out, WR.oracle_batch(cpu, canvases, sizes, size, stride, prof, tree, cmap, 1), f"predictor windows {kind}")
    again = predictor.decoder.decode_windows(logits, plan, window.profile(size), out.desc_host, None, True)
    assert _lib.launch_count() == convs and torch.equal(again.labels, out.labels), "the decode adds no convolution launch"
    leaf_values = set(predictor.decoder.leaf_values)
    assert all(set(np.unique(m).tolist()) <= leaf_values for m in out.unpack())
    # Predictor.score goes through the same path, decoding at the ground-truth sizes: its counts are DeviceScore's on the maps
    vals = np.array(sorted(leaf_values), dtype=np.uint8)
    gts = [np.ascontiguousarray(np.repeat(np.repeat(rng.choice(vals, size=(h // 6 + 1, w // 6 + 1)), 6, 0), 6, 1)[:h, :w])
           for h, w in [(100, 150), (33, 47)]]                                         # the second at a size of its own
    scores = predictor.score(imgs, gts)
    maps = predictor.last_labels
    assert [(H, W) for _, H, W, _ in maps.desc_host.tolist()] == [(100, 150), (33, 47)]
    check(maps, WR.oracle_batch([z.detach().float().cpu() for z in predictor.last_window_logits[0]], canvases,
                                 [(100, 150), (33, 47)], size, stride, prof, tree, cmap, 1), f"predictor windows {kind} score")
    buf, ghost = pack_images(gts)
    want = DeviceScore(tree, cmap).score(maps, (buf, ghost, ghost))
    assert torch.equal(scores.counts, want.counts) and torch.equal(scores.ignored, want.ignored)
    assert int(scores.counts.sum()) > 0
    assert model.training
    # without a window nothing changes: one decode_labels launch, none of the window kernels
    plain = PE.Predictor(model, tree, cmap, args)
    for fam in FAMILIES:
        _lib.launch_count(fam, reset=True)
    plain(imgs)
    assert _lib.launch_count("decode_labels") == 1 and _lib.launch_count("augment_image") == 1
    assert _lib.launch_count("decode_windows") == 0 and _lib.launch_count("window_crops") == 0
    assert plain.last_window_logits is None
