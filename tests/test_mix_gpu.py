"""Mixing augmentation on the device (csrc/mix.hip, Data/mix.py) against the torch-CPU restatement tests/mix_ref.py: counts,
chosen sets, masks and both gathered tensors are equal bit for bit on every named case, the launch budget holds, and a
DeviceAugment without a mix does what it did."""
import numpy as np
import pytest
import torch

from tests import mix_ref as MR

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.contiguous().view(torch.int32)


def _device_case(name):
    """(case, DeviceMix, x, y on the device); y comes from TargetEncoder at S x S and equals the restatement's"""
    from hrseg_amd.Data import DeviceMix, TargetEncoder
    case = MR.resolved(name)
    tree, cmap = MR.tree_of(case["tree"])
    enc = TargetEncoder(tree, cmap, case["model_type"], internal_values=case["internal"], ignore_values=case["ignore"])
    y = enc(torch.from_numpy(case["labels"]).cuda())
    assert torch.equal(y.cpu(), case["y"])
    mix = DeviceMix(tree, cmap, case["model_type"], **case["mix"])
    assert mix.names == enc.names
    return case, mix, case["x"].cuda(), y


def _check(case, mix, x2, y2):
    ref = case["ref"]
    assert torch.equal(mix.last_mask.cpu(), ref["mask"]), int((mix.last_mask.cpu() != ref["mask"]).sum())
    assert torch.equal(mix.last_chosen.cpu(), MR.chosen_bits(ref["chosen"]))
    assert mix.chosen_names() == [[mix.names[c] for c in cs] for cs in ref["chosen"]]
    if mix.last_counts is not None:
        assert torch.equal(mix.last_counts.cpu(), ref["counts"])
    assert torch.equal(_bits(x2).cpu(), _bits(ref["x2"])), int((_bits(x2).cpu() != _bits(ref["x2"])).sum())
    assert torch.equal(_bits(y2).cpu(), _bits(ref["y2"])), int((_bits(y2).cpu() != _bits(ref["y2"])).sum())


@pytest.mark.parametrize("name", sorted(MR.CASES))
def test_mix_equals_the_reference_bit_for_bit(name):
    case, mix, x, y = _device_case(name)
    x0, y0 = x.clone(), y.clone()
    x2, y2 = mix(x, y, params=case["params"])
    _check(case, mix, x2, y2)
    assert torch.equal(_bits(x), _bits(x0)) and torch.equal(_bits(y), _bits(y0)), "the inputs are untouched"
    assert mix.last_params is case["params"]
    boxed = bool(case["params"]["boxed"].all())
    assert (mix.last_counts is None) == boxed
    if not boxed:
        assert torch.equal(mix.last_counts, (y == 1).sum((2, 3)).int())


def test_two_calls_give_the_same_bytes():
    case, mix, x, y = _device_case("A")
    first = mix(x, y, params=case["params"])
    kept = [t.clone() for t in (*first, mix.last_mask, mix.last_chosen, mix.last_counts)]
    second = mix(x, y, params=case["params"])
    for a, b in zip(kept, (*second, mix.last_mask, mix.last_chosen, mix.last_counts)):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def test_gather_reapplies_the_latest_mix():
    case, mix, x, y = _device_case("A")
    with pytest.raises(RuntimeError, match="latest mix"):
        mix.gather(x)
    mix(x, y, params=case["params"])
    B, S = y.shape[0], y.shape[2]
    w = MR.image(B, 1, S, 181)
    want = MR.mix(w, case["y"], case["params"], case["cand"], case["k_of_n"], case["min_pixels"])["x2"]
    got = mix.gather(w.cuda())
    assert got.shape == (B, 1, S, S) and torch.equal(_bits(got).cpu(), _bits(want))
    with pytest.raises(ValueError, match="mask must be"):
        mix.gather(w.cuda()[:, :, :60, :60].contiguous())


def test_out_is_in_is_refused():
    from hrseg_amd import _lib, ops
    case, mix, x, y = _device_case("F")
    mix(x, y, params=case["params"])
    with pytest.raises(ValueError, match="must not alias"):
        ops.mix_gather(x, mix.last_mask, mix._table, out=x)
    fn = _lib._fn["hrseg_mix_gather"]
    assert fn(x.data_ptr(), mix.last_mask.data_ptr(), mix._table.data_ptr(), x.data_ptr(), 1, 3, 30, _lib.stream()) == -1
    assert "hrseg_mix_gather: out must not alias in" in _lib.last_error()


def test_python_validation():
    from hrseg_amd import ops
    case, mix, x, y = _device_case("D")
    with pytest.raises(ValueError, match="channels"):
        mix(x, y[:, :5].contiguous(), params=case["params"])
    with pytest.raises(ValueError, match="one size"):
        mix(x[:, :, :12, :12].contiguous(), y, params=case["params"])
    with pytest.raises(ValueError, match=r"\[B,K,S,S\]"):
        ops.mix_counts(y[:, :, :, :12].contiguous())
    with pytest.raises(AssertionError):
        ops.mix_counts(y.double())
    with pytest.raises(AssertionError):
        ops.mix_counts(y.transpose(2, 3))
    with pytest.raises(ValueError, match="2\\^31"):
        ops.mix_counts(torch.empty(1, 1, 1, 1, device="cuda").expand(1, 2, 32768, 32768))


@pytest.mark.parametrize("name,budget", [("A", 4), ("G", 3)])
def test_launch_budget(name, budget):
    from hrseg_amd import _lib
    case, mix, x, y = _device_case(name)
    torch.cuda.synchronize()
    _lib.launch_count("mix", reset=True)
    _lib.launch_count(reset=True)
    x2, y2 = mix(x, y, params=case["params"])
    n = _lib.launch_count("mix", reset=True)
    assert 0 < n <= budget, n
    assert _lib.launch_count() == 0, "the mix does not count towards the convolution total"
    mix.gather(x)
    assert _lib.launch_count("mix", reset=True) == 1
    _check(case, mix, x2, y2)


# ------------------------------------------------------------------------------------------------ through the augment
RAGGED = [(50, 70, 3), (80, 64, 1), (62, 62, 3), (30, 100, 1)]


def _ragged(seed):
    """the ragged sources of tests/test_partial_gpu.py: uint8 images and blocky label maps of the tl tree's leaf bytes"""
    _, cmap = MR.tree_of("tl")
    values = sorted(MR.R.name2pix(cmap).values())
    rng = np.random.default_rng(seed)
    imgs = []
    for h, w, ch in RAGGED:
        img = rng.integers(0, 256, size=(h, w, ch)).astype(np.uint8)
        imgs.append(img[..., 0] if ch == 1 else img)
    labs = []
    for (h, w, _), block in zip(RAGGED, [7, 11, 7, 11]):
        coarse = rng.choice(np.asarray(values, dtype=np.uint8), size=(h // block + 1, w // block + 1))
        labs.append(np.ascontiguousarray(np.repeat(np.repeat(coarse, block, 0), block, 1)[:h, :w]))
    return imgs, labs


@pytest.mark.parametrize("train", [True, False])
def test_an_augment_without_a_mix_does_what_it_did(train):
    from hrseg_amd import _lib
    from hrseg_amd.Data import DeviceAugment
    tree, cmap = MR.tree_of("tl")
    imgs, labs = _ragged(191)
    plain = DeviceAugment(62, tree, cmap, 1, train=train, seed=5)
    none = DeviceAugment(62, tree, cmap, 1, train=train, seed=5, mix=None)
    assert none.mix is None
    p = plain.sample(len(imgs)) if train else None
    torch.cuda.synchronize()
    for fam in ("mix", "augment_image", "augment_targets"):
        _lib.launch_count(fam, reset=True)
    want = plain(imgs, labs, params=p)
    per = {fam: _lib.launch_count(fam, reset=True) for fam in ("mix", "augment_image", "augment_targets")}
    got = none(imgs, labs, params=p)
    assert {fam: _lib.launch_count(fam, reset=True) for fam in per} == per
    assert per == {"mix": 0, "augment_image": 2 if train else 1, "augment_targets": 2 if train else 1}
    assert torch.equal(_bits(got[0]), _bits(want[0])) and torch.equal(_bits(got[1]), _bits(want[1]))


def test_the_augment_hands_out_the_mixed_pair():
    from hrseg_amd import _lib
    from hrseg_amd.Data import DeviceAugment, DeviceMix
    tree, cmap = MR.tree_of("tl")
    imgs, labs = _ragged(193)
    mix = DeviceMix(tree, cmap, 1, level=0, max_shift=9, seed=11)
    aug = DeviceAugment(62, tree, cmap, 1, train=True, seed=7, mix=mix)
    _lib.launch_count("mix", reset=True)
    x2, y2 = aug(imgs, labs)
    assert _lib.launch_count("mix", reset=True) == 4
    x, y = DeviceAugment(62, tree, cmap, 1, train=True)(imgs, labs, params=aug.last_params)
    p = mix.last_params
    assert bool(p["apply"].all()) and bool((p["dx"] != 0).any())
    ref = MR.mix(x.cpu(), y.cpu(), p, MR.candidates(tree, 1, 0), MR.k_of_n(0.5), 1)
    assert bool(ref["mask"].any()) and not bool(ref["mask"].all())
    assert torch.equal(mix.last_mask.cpu(), ref["mask"])
    assert torch.equal(_bits(x2).cpu(), _bits(ref["x2"])) and torch.equal(_bits(y2).cpu(), _bits(ref["y2"]))
    # evaluation ignores the mix
    ev = DeviceAugment(62, tree, cmap, 1, train=False, mix=mix)
    xe, ye = ev(imgs, labs)
    assert _lib.launch_count("mix") == 0
    want = DeviceAugment(62, tree, cmap, 1, train=False)(imgs, labs)
    assert torch.equal(_bits(xe), _bits(want[0])) and torch.equal(_bits(ye), _bits(want[1]))


def test_a_mix_over_other_channels_is_refused_at_construction():
    from hrseg_amd.Data import DeviceAugment, DeviceMix
    tree, cmap = MR.tree_of("tl")
    ext, emap = MR.tree_of("ext")
    with pytest.raises(ValueError, match="same class tree"):
        DeviceAugment(62, tree, cmap, 1, mix=DeviceMix(ext, emap, 1))
    with pytest.raises(ValueError, match="same class tree"):
        DeviceAugment(62, tree, cmap, 1, mix=DeviceMix(tree, cmap, 0))
    with pytest.raises(ValueError, match="molar"):
        DeviceMix(tree, cmap, 1, nodes=["molar"])
    with pytest.raises(ValueError, match="level 5"):
        DeviceMix(tree, cmap, 1, level=5)
