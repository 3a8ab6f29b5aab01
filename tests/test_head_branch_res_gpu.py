"""The HRNet head's 1x1 convolution at branch resolution (engine.Recorder.head_conv_bn, HRSEG_HEAD_BRANCH_RES):
conv(cat_j up(x_j)) + b = W_0 x_0 + sum_j up(W_j x_j) + b, then the unchanged BatchNorm + ReLU.

Layer level.  The yardstick is a torch-CPU fp64 evaluation of upsample -> concat -> 1x1 convolution + bias -> training
BatchNorm -> ReLU and its autograd (tests/head_branch_ref.py).  The new path and the path it replaces (upsample_concat +
conv_bn) run on the same inputs; for the output, every input gradient and the weight gradient the new path's maximum and
median error against fp64 (relative to the largest reference value) may be at most 2 x the old path's -- the project's "no
further from fp64 than" factor (tests/test_headline_size_gpu.py) -- plus the summation floor sqrt(N) * 2^-24 with N = B * H * W
pixels: the BatchNorm statistics (forward and backward) and the weight gradient are sums over that many fp32 terms, and another
order of them moves every output by about that much.
  case A: branch widths (16, 32, 48, 64) -> 160 at 9 / 5 / 3 / 2 pixels, batch 2: distinct widths, so a column block in the
          wrong place is a wrong result;
  case B: (48, 48, 48, 96) -> 240 at 256 / 128 / 64 / 32, batch 1: M = 65536 reaches the wide-tile forward and weight-gradient
          kernels (launch counters asserted).
Deterministic mode: two runs of the new path give the same bits.

Model level: hrnet_hier_tl_64 through the golden comparison of tests/test_models_gpu.py with the switch on and off, and the
recorded launch tape of the train step replays with the switch on."""
import numpy as np
import pytest
import torch

from tests.head_branch_ref import head_layer_fp64

pytestmark = pytest.mark.gpu

CASES = {"A": ((16, 32, 48, 64), (9, 5, 3, 2), 2), "B": ((48, 48, 48, 96), (256, 128, 64, 32), 1)}
U = 2.0 ** -24
_REF = {}


def _problem(case, align):
    """seeded inputs, parameters, output gradient and the fp64 results, computed once per (case, align_corners)"""
    key = (case, align)
    if key not in _REF:
        chans, sizes, Bn = CASES[case]
        C = sum(chans)
        gen = torch.Generator().manual_seed(31 * ord(case) + int(align))

        def rnd(*shape):
            return torch.randn(shape, generator=gen)
        xs = [rnd(Bn, s, s, c) for c, s in zip(chans, sizes)]
        w, b = rnd(C, C) * (2.0 / C) ** 0.5, rnd(C) * 0.1
        gamma, beta = 1.0 + 0.2 * rnd(C), 0.3 * rnd(C)
        dz = rnd(Bn, sizes[0], sizes[0], C) * 1e-2
        ref = head_layer_fp64(xs, w, b, gamma, beta, 1e-5, dz, align)
        _REF[key] = dict(xs=xs, w=w, b=b, gamma=gamma, beta=beta, dz=dz, ref=ref)
    return _REF[key]


def _run_layer(p, align, new):
    """one forward + backward of the layer on the GPU through the engine -> (z, [dx_j], dW [Cout, Cin]) and the launch counts"""
    from hrseg_amd import _lib, engine
    from hrseg_amd.Models import models as PM
    C = p["w"].shape[0]

    class Layer(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.conv = PM.Conv2d(C, C, kernel_size=1, stride=1, padding=0, bias=True)
            self.bn = PM.BatchNorm2d(C, momentum=0.1, eps=1e-5)
    layer = Layer()
    with torch.no_grad():
        layer.conv.weight.copy_(p["w"][:, :, None, None])
        layer.conv.bias.copy_(p["b"])
        layer.bn.weight.copy_(p["gamma"])
        layer.bn.bias.copy_(p["beta"])
    layer.cuda().train()
    flat = engine.FlatParams(layer, torch.device("cuda", torch.cuda.current_device()))
    rec = engine.Recorder(True, True, flat, prec=_lib.CONV_PRECISION["auto"])
    xs = [engine.Act(x.cuda()) for x in p["xs"]]
    _lib.launch_count(None, reset=True)
    for fam in ("sp_wide", "wgrad_sp_wide", "sp_im2col", "sp_group", "f32_group"):
        _lib.launch_count(fam, reset=True)
    if new:
        z = rec.head_conv_bn(xs, layer.conv, layer.bn, align, defer=True)
    else:
        z = rec.conv_bn(rec.upsample_concat(xs, align), layer.conv, layer.bn, relu=True, defer=True)
    out = z.data.clone()
    z.grad = p["dz"].cuda()
    rec.backward()
    torch.cuda.synchronize()
    counts = {fam: _lib.launch_count(fam) for fam in ("sp_wide", "wgrad_sp_wide", "sp_im2col", "sp_group", "f32_group")}
    counts["all"] = _lib.launch_count(None)
    return out, [x.grad for x in xs], layer.conv.weight._hr_gview[:, :, 0, 0].clone(), counts


def _errors(got, ref):
    d = (got.double().cpu() - ref).abs() / float(ref.abs().max())
    return float(d.max()), float(d.median())


@pytest.mark.parametrize("align", [True, False], ids=["align", "noalign"])
@pytest.mark.parametrize("case", ["A", "B"])
def test_layer_is_no_further_from_fp64_than_the_concat_path(case, align):
    from hrseg_amd import _lib
    p = _problem(case, align)
    _lib.tune(sp_wide_min_blocks=1)
    try:
        new = _run_layer(p, align, True)
        old = _run_layer(p, align, False)
    finally:
        _lib.tune(sp_wide_min_blocks=256)
    print(f"case {case} align={align}: launches new {new[3]} old {old[3]}")
    if case == "B":
        assert new[3]["sp_wide"] >= 1 and new[3]["wgrad_sp_wide"] >= 1, new[3]
        assert new[3]["sp_group"] + new[3]["f32_group"] >= 1, new[3]           # the branch-resolution convolutions, grouped
        # the path it replaces: the 240 -> 240 layer at full resolution, forward and data gradient on the narrow im2col body
        assert old[3]["sp_wide"] == 0 and old[3]["sp_im2col"] >= 2, old[3]
        assert old[3]["sp_group"] + old[3]["f32_group"] == 0, old[3]
    chans, sizes, Bn = CASES[case]
    floor = (Bn * sizes[0] * sizes[0]) ** 0.5 * U
    z64, dx64, dw64 = p["ref"]
    pairs = [("y", new[0], old[0], z64)] + [(f"dx{j}", new[1][j], old[1][j], dx64[j]) for j in range(len(chans))] + \
        [("dW", new[2], old[2], dw64)]
    bad = []
    for name, a, b, ref in pairs:
        (amax, amed), (bmax, bmed) = _errors(a, ref), _errors(b, ref)
        print(f"  {name}: new max {amax:.3e} median {amed:.3e} | old max {bmax:.3e} median {bmed:.3e} | floor {floor:.3e}")
        if not (amax <= 2 * bmax + floor and amed <= 2 * bmed + floor):
            bad.append(name)
    assert not bad, bad


def test_layer_is_bit_reproducible_in_deterministic_mode():
    from hrseg_amd import _lib
    p = _problem("A", True)
    _lib.set_deterministic(True)
    try:
        r1 = _run_layer(p, True, True)
        r2 = _run_layer(p, True, True)
    finally:
        _lib.set_deterministic(False)
    assert torch.equal(r1[0], r2[0]) and torch.equal(r1[2], r2[2])
    for a, b in zip(r1[1], r2[1]):
        assert torch.equal(a, b)
    # and it is the layer: the deterministic results sit on the fp64 yardstick
    z64, dx64, dw64 = p["ref"]
    assert _errors(r1[0], z64)[0] < 1e-4 and _errors(r1[2], dw64)[0] < 1e-4


@pytest.mark.parametrize("switch", ["1", "0"], ids=["branch_res", "concat"])
def test_golden_model_with_the_switch_on_and_off(switch, monkeypatch):
    from hrseg_amd import engine
    from hrseg_amd.Models import models as PM
    from tests.helpers import CASES as GOLDEN_CASES, build_model, conv_mode, load_tree
    from tests.test_models_gpu import _golden_body
    monkeypatch.setenv("HRSEG_HEAD_BRANCH_RES", switch)
    calls = []
    orig = engine.Recorder.head_conv_bn
    monkeypatch.setattr(engine.Recorder, "head_conv_bn", lambda self, *a, **k: (calls.append(1), orig(self, *a, **k))[1])
    name = "hrnet_hier_tl_64"
    kind, hier, tree_file, size, batch = GOLDEN_CASES[name]
    model = build_model(PM, kind, hier, load_tree(tree_file), size).cuda()
    with conv_mode(model, "auto"):
        _golden_body(name, model, "auto")
    assert (len(calls) > 0) == (switch == "1"), "the switch selects the path in training (inference keeps the concat path)"


def test_recorded_tape_replays_with_the_switch_on(monkeypatch):
    """three batches through the eager step twice and through the launch tape (recording run + two replays): the tape tracks
    the eager step to the eager step's own run-to-run noise (the form of tests/test_tape_gpu.py)"""
    from hrseg_amd import train as PT
    from tests.test_tape_gpu import _batches, _setup
    monkeypatch.setenv("HRSEG_HEAD_BRANCH_RES", "1")
    res = {}
    for mode in ("eager", "eager2", "tape"):
        model, opt, fns, args, tree, g = _setup("hrnet_hier_tl_64", lr=1e-4)
        losses, taped, ll = [], None, []
        for x, t in _batches(g, 3):
            if mode != "tape":
                losses.append(float(PT.train_step(model, opt, x, t, fns, args, tree, ll)[0]))
            elif taped is None:
                taped = PT.TapedTrainStep(model, opt, fns, args, tree, x, t)
                losses.append(taped.unpack(taped.result()[0].tolist())[0])
            else:
                losses.append(taped.unpack(taped(x, t)[0].tolist())[0])
        res[mode] = losses
        if mode == "tape":
            assert taped.replays == 2
    noise = max(abs(a - b) for a, b in zip(res["eager"], res["eager2"]))
    print(res, noise)
    for a, b in zip(res["eager"], res["tape"]):
        assert np.isfinite(b) and abs(a - b) <= max(1e-3 * abs(a), 4 * noise), (res, noise)
