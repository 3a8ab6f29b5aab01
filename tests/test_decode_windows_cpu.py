"""Sliding-window inference, the parts that need no GPU: the window plan of predictEval.SlidingWindow (coverage, the shifted
last window, the refusals), the blend profile, the float64 oracle (tests/window_ref.py) against the single-window oracle and
on windows cut from one global logit field, the near-tie share of every case the GPU test compares with the oracle, and the
compile-time resources of the kernels."""
import os

import pytest
import torch

from tests import decode_ref as R
from tests import window_ref as WR
from tests.decode_harness import _tree
from tests.helpers import HIPCC, _resources


# ------------------------------------------------------------------------------------------------------------- the plan
def _cover(origins, n, S):
    return [sum(1 for o in origins if o <= r < o + S) for r in range(n)]


@pytest.mark.parametrize("overlap,stride", [(0.5, 16), (0.25, 24), (0.0, 32)])
def test_plan_covers_every_row_and_column_one_to_three_times(overlap, stride):
    from hrseg_amd.predictEval import SlidingWindow
    w = SlidingWindow(overlap=overlap)
    assert w.stride(32) == stride == WR.stride_of(32, overlap)
    lengths = sorted({n for canvases, _ in WR.BATCHES for hw in canvases for n in hw} | set(range(32, 32 + 4 * stride + 2)))
    plan = w.plan([(n, n) for n in lengths], 32)
    n0 = 0
    for m, n in enumerate(lengths):
        ys, xs = plan.axes(m)
        assert ys == xs == WR.origins(n, 32, stride), n
        assert ys[0] == 0 and ys[-1] == n - 32, "the last window ends at the edge"
        assert all(a < b for a, b in zip(ys, ys[1:]))
        cover = _cover(ys, n, 32)
        assert min(cover) >= 1 and max(cover) <= 3, (n, ys)
        assert plan.canvas(m) == (n, n) and plan.first_window(m) == n0
        n0 += len(ys) * len(xs)
    assert plan.nwindows == n0
    if overlap == 0.0:
        assert plan.axes(lengths.index(64)) == ([0, 32], [0, 32]) and max(_cover([0, 32], 64, 32)) == 1, "abutting windows"


def test_plan_canvas_window_order_and_tables():
    from hrseg_amd.predictEval import SlidingWindow
    plan = SlidingWindow().plan([(100, 150), (70, 62), (20, 31)], 62)
    assert plan.wdesc.tolist() == [[100, 150, 3, 4, 0, 0, 0, 0], [70, 62, 2, 1, 12, 7, 0, 0], [62, 62, 1, 1, 14, 10, 0, 0]]
    assert plan.origins.tolist() == [0, 31, 38, 0, 31, 62, 88, 0, 8, 0, 0, 0] and plan.nwindows == 15
    assert plan.wdesc.dtype == torch.int64 and plan.origins.dtype == torch.int32
    assert SlidingWindow(scale=0.5).plan([(1400, 2900), (100, 100)], 620).wdesc[:, :4].tolist() == [[700, 1450, 2, 4], [620, 620, 1, 1]]
    assert SlidingWindow(scale=1.5).canvas(50, 70, 32) == (75, 105)
    assert SlidingWindow().plan([(1400, 2900)] * 2, 620).wdesc[:, 2:5].tolist() == [[4, 9, 0], [4, 9, 36]]


def test_plan_refusals():
    from hrseg_amd import ops
    from hrseg_amd.Data.decode import WindowPlan, plan_windows
    from hrseg_amd.predictEval import SlidingWindow
    for bad in (dict(overlap=0.51), dict(overlap=-0.1), dict(scale=0.0), dict(scale=float("inf")), dict(blend="cosine"),
                dict(window_batch=0)):
        with pytest.raises(ValueError):
            SlidingWindow(**bad)
    with pytest.raises(ValueError, match="window size 0"):
        SlidingWindow().plan([(10, 10)], 0)
    with pytest.raises(ValueError, match="window size 32769"):
        SlidingWindow().plan([(10, 10)], 32769)
    with pytest.raises(ValueError, match="supported 1..64 per axis"):
        SlidingWindow().plan([(40, 16 * 65 + 32)], 32)
    good = plan_windows([(50, 70), (80, 64)], 32, 16)
    ops.check_window_plan("t", good, 2, 32)

    def with_origins(vals):
        """`good` with the row origins of image 0 replaced"""
        org = good.origins.tolist()
        oo, n = int(good.wdesc[0, 5]), int(good.wdesc[0, 2])
        org[oo:oo + n] = vals
        return WindowPlan(good.wdesc, torch.tensor(org, dtype=torch.int32), good.nwindows, 32)
    assert good.axes(0)[0] == [0, 16, 18]
    for vals, msg in (([1, 16, 18], "do not run from 0"), ([0, 16, 17], "do not run from 0"), ([0, 18, 18], "not increasing"),
                      ([0, 18, 16], "do not run from 0")):
        with pytest.raises(ValueError, match=msg):
            ops.check_window_plan("t", with_origins(vals), 2, 32)
    with pytest.raises(ValueError, match="steps of at most 32"):
        ops.check_window_axis("t", [0, 33, 40], 72, 32)
    with pytest.raises(ValueError, match="more than 3 windows"):
        ops.check_window_axis("t", [0, 8, 16, 24, 40], 72, 32)
    ops.check_window_axis("t", [0, 8, 16, 32, 40], 72, 32)                    # origins[k + 3] >= origins[k] + S holds
    wd = good.wdesc.clone()
    wd[1, 4] += 1                                                               # the last window number would be N
    with pytest.raises(ValueError, match="are not inside the 24 windows"):
        ops.check_window_plan("t", WindowPlan(wd, good.origins, good.nwindows, 32), 2, 32)
    wd = good.wdesc.clone()
    wd[0, 0] = 31
    with pytest.raises(ValueError, match="smaller than a window"):
        ops.check_window_plan("t", WindowPlan(wd, good.origins, good.nwindows, 32), 2, 32)
    with pytest.raises(ValueError, match="made for windows of 32, not 31"):
        ops.check_window_plan("t", good, 2, 31)
    with pytest.raises(ValueError, match=r"\[3,8\] int64 host tensor"):
        ops.check_window_plan("t", good, 3, 32)
    with pytest.raises(ValueError, match="1 windows for 2 images"):
        ops.check_window_plan("t", WindowPlan(good.wdesc, good.origins, 1, 32), 2, 32)
    for prof, msg in ((torch.ones(31), "32 entries"), (torch.ones(32, dtype=torch.float64), "fp32"),
                      (torch.cat([torch.ones(31), torch.zeros(1)]), "strictly positive"),
                      (torch.cat([torch.ones(31), torch.tensor([float("nan")])]), "strictly positive"),
                      (torch.cat([torch.ones(31), torch.tensor([float("inf")])]), "finite")):
        with pytest.raises(ValueError, match=msg):
            ops.check_window_profile("t", prof, 32)


@pytest.mark.parametrize("S", [1, 2, 31, 32, 620, 32768])
def test_profile_is_positive_in_fp32(S):
    from hrseg_amd.predictEval import SlidingWindow
    p = SlidingWindow().profile(S)
    assert p.dtype == torch.float32 and p.shape == (S,) and bool((p > 0).all()) and bool(torch.isfinite(p).all())
    assert torch.equal(SlidingWindow(blend="uniform").profile(S), torch.ones(S))
    if S <= 620:
        assert torch.equal(p, WR.profile(S, "hann")), "the product's table is the oracle's formula"


# ----------------------------------------------------------------------------------------------------- oracle identities
def _same(a, b):
    assert torch.equal(a[0], b[0]), "labels"
    assert torch.equal(a[1], b[1]), "confidence"
    assert len(a[3]) == len(b[3]) and all(torch.equal(p, q) for p, q in zip(a[3], b[3])), "path"


@pytest.mark.parametrize("model_type", [1, 0])
@pytest.mark.parametrize("key", ["tl", "ext"])
def test_one_window_with_the_uniform_profile_is_the_single_window_oracle(key, model_type):
    tree, cmap = _tree(key)
    logits = R.smooth_logits(3, WR.channels(tree, model_type), 30, 11 + model_type)
    for b, (H, W) in enumerate([(25, 41), (30, 30), (47, 19)]):
        zb = [z[b] for z in logits]
        for dtype in (torch.float64, torch.float32):
            got = WR.decode_windows_sample([z[None] for z in zb], [0], [0], 30, 30, WR.profile(30, "uniform"), tree, cmap,
                                           model_type, H, W, dtype)
            _same(got, R.decode_sample(zb, tree, cmap, model_type, H, W, dtype=dtype))


@pytest.mark.parametrize("blend", WR.BLENDS)
@pytest.mark.parametrize("overlap", WR.OVERLAPS)
@pytest.mark.parametrize("key,model_type", [("tl", 1), ("ext", 1), ("ext", 0)])
def test_windows_cut_from_one_field_decode_as_the_field(key, model_type, overlap, blend):
    """blending copies of the same value gives the value back (up to rounding): outside near ties the decode of the windows is
    the decode of the field itself, whatever the profile"""
    tree, cmap = _tree(key)
    stride = WR.stride_of(WR.S, overlap)
    for i, ((Hc, Wc), (H, W)) in enumerate([((50, 70), (50, 70)), ((80, 64), (33, 47)), ((64, 64), (90, 100))]):
        field = [R.smooth_logits(1, [n], max(Hc, Wc), 70 + i + model_type, coarse=12)[0][0][:, :Hc, :Wc] for n in
                 WR.channels(tree, model_type)]
        ys, xs = WR.origins(Hc, WR.S, stride), WR.origins(Wc, WR.S, stride)
        wins = [WR.cut_windows(f, ys, xs, WR.S) for f in field]
        got = WR.decode_windows_sample(wins, ys, xs, Hc, Wc, WR.profile(WR.S, blend), tree, cmap, model_type, H, W)
        want = WR.walk(WR.resize([f.double() for f in field], H, W), tree, cmap, model_type)
        keep = ~(got[2] | want[2])
        assert int(((got[0] != want[0]) & keep).sum()) == 0
        assert float((got[1] - want[1]).abs()[keep].max()) < 1e-12
        assert int((~keep).sum()) <= WR.MASK_CAP * H * W


@pytest.mark.parametrize("key,model_type,overlap,blend", WR.CASES)
def test_near_tie_share_of_the_gpu_cases_stays_under_the_cap(key, model_type, overlap, blend):
    """the GPU test excuses label differences on near ties only, up to MASK_CAP of a call's pixels: every call it makes stays
    below that here, and torch's own fp32 evaluation of the formula differs from fp64 nowhere outside them"""
    _, _, calls = WR.case_oracle(key, model_type, overlap, blend, _tree)
    for batch, (_, samples) in enumerate(calls):
        masked = sum(int(tie.sum()) for _, _, tie, _, _ in samples)
        total = sum(h * w for h, w in WR.BATCHES[batch][1])
        wrong = sum(int(((l32 != l) & ~tie).sum()) for l, _, tie, l32, _ in samples)
        d32 = max(float((c32.double() - c).abs()[~tie].max()) for _, c, tie, _, c32 in samples)
        print(f"{key} model_type {model_type} overlap {overlap} {blend} call {batch}: mask {masked}/{total}, fp32 labels differing "
              f"outside it {wrong}, fp32 confidence within {d32:.3e} of fp64")
        assert total == (9107, 8517)[batch]
        assert masked <= WR.MASK_CAP * total, (masked, total)
        assert wrong == 0


# ------------------------------------------------------------------------------------------------------------ resources
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_window_kernels_fit_four_waves_per_simd_without_scratch():
    """512 VGPRs per SIMD lane: 4 waves need <= 128 each; no scratch and no spilled vector register in any kernel"""
    res = _resources("windows")
    print(res)
    dec = {n: r for n, r in res.items() if "decode_windows_kernel" in n}
    crops = {n: r for n, r in res.items() if "window_crops_kernel" in n}
    assert len(dec) == 2 and len(crops) == 1, sorted(res)
    for name, r in res.items():
        assert r["scratch"] == 0 and r["spill"] == 0 and r["vgprs"] <= 128, (name, r)
