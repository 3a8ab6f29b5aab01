"""Multi-view decode (test-time augmentation), the parts that need no GPU: the float64 oracle (tests/decode_views_ref.py)
against the single-view oracle and under flipped copies, the near-tie share of every case the GPU test compares with it,
predictEval.TestTimeAugment, and the compile-time resources of the decode_views kernels."""
import os

import pytest
import torch

from tests import decode_ref as R
from tests import decode_views_ref as V
from tests.decode_harness import _tree
from tests.helpers import HIPCC, _resources


def _same(a, b):
    assert torch.equal(a[0], b[0]), "labels"
    assert torch.equal(a[1], b[1]), "confidence"
    assert torch.equal(a[2], b[2]), "near-tie mask"
    assert len(a[3]) == len(b[3]) and all(torch.equal(p, q) for p, q in zip(a[3], b[3])), "path"


@pytest.mark.parametrize("model_type", [1, 0])
@pytest.mark.parametrize("key", ["tl", "ext"])
def test_one_unflipped_view_is_the_single_view_oracle(key, model_type):
    tree, cmap = _tree(key)
    logits = R.smooth_logits(3, V.channels(tree, model_type), 30, 11 + model_type)
    for b, (H, W) in enumerate([(25, 41), (30, 30), (47, 19)]):           # resampled both ways, and identity geometry
        zb = [z[b] for z in logits]
        for dtype in (torch.float64, torch.float32):
            _same(V.decode_views_sample([(zb, 0)], tree, cmap, model_type, H, W, dtype=dtype),
                  R.decode_sample(zb, tree, cmap, model_type, H, W, dtype=dtype))


@pytest.mark.parametrize("flags", [[0, 1], [0, 2], [0, 1, 2, 3], [3, 0]])
@pytest.mark.parametrize("key,model_type", [("tl", 1), ("ext", 1), ("ext", 0)])
def test_flipped_copies_of_a_view_change_nothing(key, model_type, flags):
    """the flipped-back copies are the view itself, and (r + r), ((r + r) + r) + r are exact: every output is equal"""
    tree, cmap = _tree(key)
    logits = R.smooth_logits(2, V.channels(tree, model_type), 30, 17)
    for b, (H, W) in enumerate([(25, 41), (44, 23)]):
        zb = [z[b] for z in logits]
        one = V.decode_views_sample([(zb, 0)], tree, cmap, model_type, H, W)
        many = V.decode_views_sample([([V.flip(z, f) for z in zb], f) for f in flags], tree, cmap, model_type, H, W)
        _same(many, one)


@pytest.mark.parametrize("key,model_type,vs", V.CASES)
def test_near_tie_share_of_the_gpu_cases_stays_under_the_cap(key, model_type, vs):
    """the GPU test excuses label differences on near ties only, up to MASK_CAP of a case's pixels: every case it runs
    stays far below that here, and torch's own fp32 evaluation of the formula differs from fp64 nowhere outside them"""
    _, _, _, samples = V.case_oracle(key, model_type, vs, _tree)
    masked = sum(int(tie.sum()) for _, _, tie, _, _ in samples)
    total = sum(h * w for h, w in V.RAGGED)
    wrong = sum(int(((l32 != l) & ~tie).sum()) for l, _, tie, l32, _ in samples)
    d32 = max(float((c32.double() - c).abs()[~tie].max()) for _, c, tie, _, c32 in samples)
    print(f"{key} model_type {model_type} views {vs}: mask {masked}/{total}, fp32 labels differing outside it {wrong}, "
          f"fp32 confidence within {d32:.3e} of fp64")
    assert total == 15464
    assert masked <= V.MASK_CAP * total, (masked, total)
    assert wrong == 0


def test_identity_geometry_marks_ties_only_with_more_than_one_view():
    tree, cmap = _tree("tl")
    z = [a[0] for a in R.smooth_logits(1, [4, 4], 24, 3)]
    z[0][0, 5, 5] = z[0][1, 5, 5] = 9.0                       # an exact tie of level 0 at one pixel
    assert not bool(V.decode_views_sample([(z, 0)], tree, cmap, 1, 24, 24)[2].any())
    two = V.decode_views_sample([(z, 0), ([V.flip(a, 1) for a in z], 1)], tree, cmap, 1, 24, 24)
    assert bool(two[2][5, 5])


def test_test_time_augment_views_and_errors():
    from hrseg_amd.predictEval import TestTimeAugment
    assert TestTimeAugment().views(620) == [(620, 0), (620, 1)]
    assert TestTimeAugment(hflip=False).views(64) == [(64, 0)]
    assert TestTimeAugment(hflip=False, vflip=True).views(64) == [(64, 0), (64, 2)]
    assert TestTimeAugment(True, True, (1.0, 0.75)).views(62) == [(62, 0), (62, 1), (62, 2), (62, 3), (46, 0), (46, 1), (46, 2), (46, 3)]
    assert TestTimeAugment(True, False, (0.75, 1.25, 1.0)).views(62) == [(46, 0), (46, 1), (78, 0), (78, 1), (62, 0), (62, 1)]
    assert TestTimeAugment(False, False, tuple(0.5 + 0.125 * i for i in range(8))).views(64)[-1] == (88, 0)
    with pytest.raises(ValueError, match="more than 8 views"):
        TestTimeAugment(True, True, (1.0, 0.75, 0.5))
    with pytest.raises(ValueError, match="more than 8 views"):
        TestTimeAugment(False, False, tuple(1.0 + 0.1 * i for i in range(9)))
    with pytest.raises(ValueError, match="positive"):
        TestTimeAugment(scales=(1.0, 0.0))
    with pytest.raises(ValueError, match="positive"):
        TestTimeAugment(scales=(-0.5,))
    with pytest.raises(ValueError, match="duplicate"):
        TestTimeAugment(scales=(1.0, 0.75, 1.0))
    with pytest.raises(ValueError, match="gives 0"):
        TestTimeAugment(scales=(0.001,)).views(62)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_decode_views_kernels_fit_four_waves_per_simd_without_spilling():
    """512 VGPRs per SIMD lane: 4 waves need <= 128 each; no scratch and no spilled vector register in either instantiation"""
    res = {n: r for n, r in _resources("decode_views").items() if "decode_views_kernel" in n}
    print(res)
    assert len(res) == 2, sorted(res)
    for name, r in res.items():
        assert r["scratch"] == 0 and r["spill"] == 0 and r["vgprs"] <= 128, (name, r)
