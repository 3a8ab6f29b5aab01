"""Border weights without a GPU: the two references of the weight map agree, the table, the options and their refusals, the
options in the key of a recorded step, and the room fp32 has on the weighted loss at the bars the GPU test uses
(tests/test_loss_pw_gpu.py).  Run with -s for the worst distances."""
import math

import numpy as np
import pytest
import torch

from tests import border_ref as BR
from tests import headloss_ref as R
from tests import loss_options_ref as LR


# ------------------------------------------------------------------------------------------------ weight map references
def _tiny_cases():
    rng = np.random.default_rng(11)
    cases = []
    for i in range(20):
        B, C = int(rng.integers(1, 3)), int(rng.integers(1, 6))
        H, W = int(rng.integers(1, 10)), int(rng.integers(1, 10))
        radius = int(rng.integers(1, 7))
        t = rng.integers(-1, 2, (B, C, H, W)).astype(np.float32)          # -1 / 0 / 1 at random: several on, none on, void
        if i % 4 == 0:
            t = BR.planes(BR.voronoi(B, C, H, W, seed=i, nseeds=3), C, void=rng.random((B, H, W)) < 0.2)
        if i % 5 == 1:
            t[0, 0, 0, 0] = np.nan
        cases.append((t, radius))
    return cases


def test_brute_force_equals_the_double_loop():
    for t, radius in _tiny_cases():
        lut = BR.table(10.0, 2.0, radius)
        a, b = BR.weight_map(t, radius, lut), BR.weight_map_loops(t, radius, lut)
        for x, y, name in zip(a, b, ("labels", "v", "d2")):
            assert x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8)), (name, t.shape, radius)


def test_known_answers():
    # two labels side by side: distance to the other half, capped by the radius
    lab = np.zeros((1, 1, 8), dtype=np.int64)
    lab[..., 4:] = 1
    labels, v, d2 = BR.weight_map(BR.planes(lab, 2), 2, BR.table(1.0, 1.0, 2))
    assert d2.reshape(-1).tolist() == [0, 0, 4, 1, 1, 4, 0, 0]
    assert labels.reshape(-1).tolist() == [0, 0, 0, 0, 1, 1, 1, 1]
    # a void gap: never a source, gets d2 = 0, and the label behind it is found
    t = BR.planes(lab, 2)
    t[..., 3:5] = -1.0
    labels, v, d2 = BR.weight_map(t, 3, BR.table(1.0, 1.0, 3))
    assert labels.reshape(-1).tolist() == [0, 0, 0, 255, 255, 1, 1, 1]
    assert d2.reshape(-1).tolist() == [0, 0, 9, 0, 0, 9, 0, 0]
    assert v.reshape(-1)[3] == np.float32(1.0)


def test_table_values():
    from hrseg_amd.Metrics.border import BorderWeights, border_table
    for w0, sigma, radius in ((10.0, 5.0, 15), (0.0, 1.0, 3), (3.5, 0.7, 32), (10.0, 2.0, 5)):
        lut = BorderWeights(w0, sigma, radius).table()
        assert lut.dtype == np.float32 and lut.shape == (radius * radius + 1,)
        assert lut[0] == np.float32(1.0)
        for k in (1, 2, radius, radius * radius):
            assert lut[k] == np.float32(1.0 + w0 * math.exp(-k / (2.0 * sigma * sigma))), (w0, sigma, k)
        assert np.array_equal(lut, BR.table(w0, sigma, radius)) and np.array_equal(lut, border_table(w0, sigma, radius))
        assert (np.diff(lut[1:]) <= 0).all() and lut.min() >= 1.0
    assert BorderWeights(0.0, 1.0, 3).table().tolist() == [1.0] * 10


def test_options_and_their_refusals():
    from hrseg_amd.Metrics import losses
    from hrseg_amd.Metrics.border import BorderOptions, BorderWeights
    assert losses.BorderWeights is BorderWeights and losses.BorderOptions is BorderOptions
    bw = BorderWeights()
    assert (bw.w0, bw.sigma, bw.radius) == (10.0, 5.0, 15) and bw.options == BorderOptions(10.0, 5.0, 15)
    assert BorderWeights(sigma=20.0).radius == 32 and BorderWeights(sigma=0.1).radius == 1 and BorderWeights(1, 2.0).radius == 6
    assert bw.labels is None and bw.last is None
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="w0"):
            BorderWeights(w0=bad)
    for bad in (0.0, -2.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="sigma"):
            BorderWeights(sigma=bad)
    for bad in (0, 33, -1, 2.5, True, "3"):
        with pytest.raises(ValueError, match="radius"):
            BorderWeights(radius=bad)
    assert BorderOptions.from_ce(None) is None and BorderOptions.from_ce(losses.CrossEntropyLoss()) is None
    assert BorderOptions.from_ce(losses.CrossEntropyLoss(border=BorderWeights(3, 2, 5))) == (3.0, 2.0, 5)
    with pytest.raises(ValueError, match="ohem_thresh.*border"):
        losses.CrossEntropyLoss(ohem_thresh=0.7, border=bw)
    with pytest.raises(ValueError, match="border"):
        losses.CrossEntropyLoss(border=(10.0, 5.0))
    assert losses.CrossEntropyLoss().last_border is None


def test_fused_ce_dice_refuses_a_bad_pixel_weight():
    from hrseg_amd.Metrics import losses
    z, t, w = torch.zeros(2, 3, 4, 5), torch.zeros(2, 3, 4, 5), [1.0, 1.0, 1.0]
    for bad, what in ((torch.ones(2, 4, 4), "pixel_weight must be a"), (torch.ones(2, 3, 4, 5), "pixel_weight must be a"),
                      (torch.ones(40), "pixel_weight must be a"), (np.ones((2, 4, 5), dtype=np.float32), "pixel_weight must be a"),
                      (torch.ones(2, 4, 5, dtype=torch.float64), "float32"), (torch.ones(2, 1, 4, 5, dtype=torch.int32), "float32"),
                      (torch.ones(2, 4, 5, device="meta"), "is on")):
        with pytest.raises(ValueError, match=what):
            losses.fused_ce_dice(z, t, w, pixel_weight=bad)
    with pytest.raises(ValueError, match="pixel_weight and ohem"):
        losses.fused_ce_dice(z, t, w, ohem=(0.7, 0), pixel_weight=torch.ones(2, 4, 5))


def test_border_options_are_part_of_the_tape_key(monkeypatch):
    """taped_step_for keys its recordings on the BorderOptions of every level: the recording is stubbed out, the key is not"""
    import argparse
    from hrseg_amd import train as T
    from hrseg_amd.Metrics import losses

    built = []

    class Step:
        def __init__(self, *a, **k):
            built.append(a[2])

    class Model:
        conv_dtype, training, _grad_hook = "auto", True, None

        def _bn_sync(self):
            return None

        def flatten_parameters(self, device):
            return self

    class Cuda:
        is_cuda, shape, device = True, (2, 3, 8, 8), "cuda:0"

    monkeypatch.setattr(T, "TapedTrainStep", Step)
    monkeypatch.delenv("HRSEG_TAPE", raising=False)
    model, opt = Model(), object()
    args = argparse.Namespace(level_weights=[[1.0, 2.0]], level0_pretrain_epochs=None)

    def fns(border):
        return [[losses.CrossEntropyLoss(border=border), losses.SoftDiceLoss()]]

    def step_for(border):
        return T.taped_step_for(model, opt, fns(border), args, None, Cuda(), Cuda())
    s0, fresh0 = step_for(None)
    s1, fresh1 = step_for(losses.BorderWeights(10, 2, 5))
    s2, fresh2 = step_for(losses.BorderWeights(10, 2, 5))
    s3, fresh3 = step_for(losses.BorderWeights(10, 2, 6))
    assert (fresh0, fresh1, fresh2, fresh3) == (True, True, False, True)
    assert s1 is s2 and len({id(s0), id(s1), id(s3)}) == 3 and len(built) == 3


# ------------------------------------------------------------------------------------------------ room of the weighted loss
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for kind, d in WORST.items():
        print(f"\nfp32 vs fp64, weighted reference, {kind}: " + ", ".join(f"{k} {v:.2e}" for k, v in d.items()))


@pytest.mark.parametrize("kind", BR.WEIGHT_KINDS)
def test_fp32_has_room_at_the_bars(kind):
    """the fp32 evaluation of the weighted reference stays inside LOSS_BARS of the fp64 one on the whole grid of the GPU test"""
    worst = WORST.setdefault(kind, {"ce": 0.0, "dice": 0.0, "dz": 0.0})
    for C in LR.LOSS_C:
        for hw in LR.LOSS_HW:
            for B in LR.LOSS_B:
                for pattern in LR.LOSS_PATTERNS:
                    for opt in BR.PW_OPTION_SETS:
                        a, b = BR.run(C, hw, B, pattern, kind, opt, torch.float32), BR.run(C, hw, B, pattern, kind, opt, torch.float64)
                        assert a["nvalid"] == b["nvalid"]
                        d = {"ce": R.absdiff(a["ce"], b["ce"]), "dice": R.absdiff(a["dice"], b["dice"]), "dz": R.rel(a["dz"], b["dz"])}
                        for k, v in d.items():
                            worst[k] = max(worst[k], v)
                            assert v < LR.LOSS_BARS[k], (kind, C, hw, B, pattern, opt, k, v)


def test_constant_maps_and_the_empty_weighted_mask():
    """a constant map gives the loss of the unweighted reference; a class mask of weighted mass 0 makes the item the constant 1.0
    with a CE gradient of exactly 0"""
    C, hw, B = 5, 257, 3
    for pattern in ("no_ignore", "random_ignore"):
        plain = LR.run(C, hw, B, pattern, LR.DEFAULTS, torch.float64)
        for kind in ("ones", "twos"):
            got = BR.run(C, hw, B, pattern, kind, LR.DEFAULTS, torch.float64)
            assert R.absdiff(got["ce"], plain["ce"]) < 1e-12 and R.rel(got["dz"], plain["dz"]) < 1e-12
        x = LR.inputs(C, hw, B, pattern)
        z = R._leaf(x["z"], torch.float64)
        pw = BR.pixel_weights("plane_zero", C, hw, B, pattern)
        ce, _, _ = BR.ce_dice(z, x["t"].double(), x["w"], pw)
        ce.backward()
        b, _ = BR.plane_zero_at(B, C)
        assert float(z.grad[b].abs().max()) == 0.0 and float(z.grad.abs().max()) > 0.0
        others, _, _ = BR.ce_dice(x["z"].double()[:b], x["t"].double()[:b], x["w"], pw[:b])
        assert abs(float(ce.detach()) - (float(others) * b + 1.0) / B) < 1e-12
