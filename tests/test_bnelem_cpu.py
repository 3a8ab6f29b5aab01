"""Pins tests/bnelem_ref.py on the CPU: the float64 references against torch's float64 functional ops, the fp32 index / weight
restatement of the bilinear reference against fp32 F.interpolate, the bounds (finite, and small enough to see one dropped
pixel, a swapped align_corners and a gradient sent to the last maximum), and the case lists against the restated host rules.
No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import bnelem_ref as R

TIGHT = 1e-12


def close(a, b, tol=TIGHT):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    err = np.abs(a - b).max() if a.size else 0.0
    assert err <= tol * max(1.0, np.abs(b).max() if b.size else 0.0), err


def t64(a):
    return torch.from_numpy(np.asarray(a, np.float64).copy())


def check_bound(value, bound):
    value, bound = np.asarray(value, np.float64), np.asarray(bound, np.float64)
    assert np.isfinite(value).all() and np.isfinite(bound).all() and (bound >= 0).all()
    assert (bound[value != 0] > 0).all()


# =========================================================================== references against torch float64
@pytest.mark.parametrize("residual,relu", [(False, False), (True, True), (False, True)])
def test_bn_reference_is_torch_batch_norm(residual, relu):
    npix, C, mom = 333, 12, 0.1
    y = R.bn_input(npix, C, 2.0, 3, 1)
    gamma, beta = R.randn(C, 2) + 1.5, R.randn(C, 3)
    rm, rv = R.randn(C, 4), np.abs(R.randn(C, 5)) + 0.5
    res = R.randn((npix, C), 6) if residual else None
    dz = R.randn((npix, C), 7)
    f = R.bn_forward(y, gamma, beta, rm, rv, 11, mom, R.EPS, 4)
    yt, gt, bt = t64(y).requires_grad_(True), t64(gamma).requires_grad_(True), t64(beta).requires_grad_(True)
    rt = t64(res).requires_grad_(True) if residual else None
    rmt, rvt = t64(rm), t64(rv)
    # (the ABI takes eps and momentum as float: the reference uses their fp32 values)
    z = F.batch_norm(yt, rmt, rvt, gt, bt, True, float(R.f32(mom)), float(R.f32(R.EPS)))
    if residual:
        z = z + rt
    pre = z
    if relu:
        z = torch.relu(z)
    z.backward(t64(dz))
    coef = f["coef"][0]
    close(coef[0], yt.detach().mean(0).numpy())
    close(coef[1], 1.0 / np.sqrt(yt.detach().var(0, unbiased=False).numpy() + R.f32(R.EPS)))
    close(f["running_mean"][0], rmt.numpy())
    close(f["running_var"][0], rvt.numpy())
    assert f["nbt"] == 12
    rows, b_rows = R.bn_rows_from_rows(coef, gamma, beta)
    close(rows, coef[2:])
    check_bound(rows, b_rows)
    wrong = coef.copy()
    wrong[1] *= 1.0 + 4 * R.U                                 # scale and shift that do not follow a moved rstd are seen
    assert (np.abs(R.bn_rows_from_rows(wrong, gamma, beta)[0][0] - coef[2]) > b_rows[0]).all()
    zr, _, prer = R.bn_apply(y, coef, res, relu)
    close(zr, z.detach().numpy())
    close(prer, pre.detach().numpy())
    mask = (prer > 0) if relu else None
    b = R.bn_backward(dz, y, coef, mask, 4, dgamma=np.zeros(C), dbeta=np.zeros(C), dres=np.zeros((npix, C)) if residual else None)
    close(b["dy"][0], yt.grad.numpy())
    close(b["dgamma"][0], gt.grad.numpy())
    close(b["dbeta"][0], bt.grad.numpy())
    if residual:
        close(b["dres"], rt.grad.numpy().astype(np.float32), 1e-7)
    # eval mode: the running statistics are constants
    ce, b_ce = R.bn_eval_coef(gamma, beta, rm, rv, R.EPS)
    check_bound(ce[1:], b_ce[1:])
    assert np.array_equal(ce[0], rm.astype(np.float64)) and not b_ce[0].any()          # (the mean row is the running mean itself)
    close(ce[1], 1.0 / np.sqrt(rv.astype(np.float64) + R.f32(R.EPS)))
    yt2, gt2, bt2 = t64(y).requires_grad_(True), t64(gamma).requires_grad_(True), t64(beta).requires_grad_(True)
    ze = F.batch_norm(yt2, t64(rm), t64(rv), gt2, bt2, False, 0.0, float(R.f32(R.EPS)))
    close(R.bn_apply(y, ce)[0], ze.detach().numpy())
    ze0 = F.batch_norm(t64(y), t64(rm), t64(rv), None, None, False, 0.0, float(R.f32(R.EPS)))          # gamma / beta null
    close(R.bn_apply(y, R.bn_eval_coef(None, None, rm, rv, R.EPS)[0])[0], ze0.numpy())
    ze.backward(t64(dz))
    e = R.bn_backward(dz, y, ce, None, 4, eval_mode=True, dgamma=np.ones(C), dbeta=np.ones(C))
    close(e["dy"][0], yt2.grad.numpy())
    close(e["dgamma"][0], 1.0 + gt2.grad.numpy())
    close(e["dbeta"][0], 1.0 + bt2.grad.numpy())


def test_bn_repeat_and_stat_div():
    """repeat = 3: three sequential running updates of the same statistics; stat_div = 3: the unbiased factor of npix / 3"""
    npix, C, mom = 30, 4, 0.1
    y = np.tile(R.randn((10, C), 1), (3, 1))
    rm, rv = R.randn(C, 2), np.abs(R.randn(C, 3)) + 0.5
    f = R.bn_forward(y, None, None, rm, rv, 5, mom, R.EPS, 1, repeat=3, stat_div=3)
    rmt, rvt = t64(rm), t64(rv)
    for _ in range(3):
        F.batch_norm(t64(y[:10]), rmt, rvt, None, None, True, float(R.f32(mom)), float(R.f32(R.EPS)))
    close(f["running_mean"][0], rmt.numpy())
    close(f["running_var"][0], rvt.numpy())
    assert f["nbt"] == 8
    one = R.bn_forward(y[:1], None, None, rm, rv, None, mom, R.EPS, 1)          # n1 <= 1: the biased variance (0) enters
    close(one["running_var"][0], (1.0 - R.f32(mom)) * rv)
    assert one["nbt"] is None


def test_fold_is_conv_then_bn():
    for (cout, row), nulls in zip(R.FOLD_CASES, R.FOLD_NULLS):
        w, bias, gamma, beta = R.randn((cout, row), 1, row), R.randn(cout, 2), R.randn(cout, 3) + 1.5, R.randn(cout, 4)
        rm, rv = R.randn(cout, 5), np.abs(R.randn(cout, 6)) + 0.1
        args = dict(bias=bias, gamma=gamma, beta=beta)
        for k in nulls:
            args[k] = None
        (wf, bw), (bf, bb) = R.bn_fold(w, args["bias"], args["gamma"], args["beta"], rm, rv, R.EPS)
        check_bound(wf, bw)
        check_bound(bf, bb)
        x = R.randn((17, row), 7).astype(np.float64)
        conv = x @ w.astype(np.float64).T + (0.0 if args["bias"] is None else bias)
        unfolded = F.batch_norm(t64(conv), t64(rm), t64(rv), None if args["gamma"] is None else t64(gamma),
                                None if args["beta"] is None else t64(beta), False, 0.0, float(R.f32(R.EPS))).numpy()
        close(x @ wf.T + bf, unfolded)


@pytest.mark.parametrize("case", R.POOL_CASES[:-1], ids=lambda c: c[0])
def test_maxpool_reference_is_torch(case):
    _, B, H, W, C = case
    x = R.ties((B, H, W, C), 1, H, W, C)
    xt = t64(x).permute(0, 3, 1, 2).requires_grad_(True)
    yt = F.max_pool2d(xt, 2)
    y = R.maxpool2_fwd(x)
    assert np.array_equal(y, yt.detach().permute(0, 2, 3, 1).numpy().astype(np.float32))
    dy = R.randn(y.shape, 2)
    yt.backward(t64(dy).permute(0, 3, 1, 2))
    want = xt.grad.permute(0, 2, 3, 1).numpy().astype(np.float32)
    assert np.array_equal(R.maxpool2_bwd(x, dy), want)
    old = R.randn(x.shape, 3)
    assert np.array_equal(R.maxpool2_bwd(x, dy, dx_old=old), old + want)
    # a gradient sent to the LAST maximum is seen: the inputs hold ties
    assert not np.array_equal(R.maxpool2_bwd(x, dy, last=True), want)


GEOMS = [(g, a) for g in R.RESIZE_GEOMETRIES for a in (1, 0)]


@pytest.mark.parametrize("geom,align", GEOMS, ids=lambda v: v[0] if isinstance(v, tuple) else str(v))
def test_bilinear_reference_is_torch(geom, align):
    name, Hi, Wi, Hr, Wr = geom
    B, C = (1, 4) if name.startswith("trip") or name.endswith("4x") else (2, 8)
    x = R.randn((B, Hi, Wi, C), 1, Hi, Wr)
    xt = t64(x).permute(0, 3, 1, 2).requires_grad_(True)
    up = F.interpolate(xt, size=(Hr, Wr), mode="bilinear", align_corners=bool(align))
    # float64 coordinates: torch's float64 op to 1e-12, with placement = F.pad
    v, _ = R.bilinear_fwd(x, Hr, Wr, align, Hr + 5, Wr + 4, 2, 3, dtype=np.float64)
    close(v, F.pad(up, (3, 1, 2, 3)).detach().permute(0, 2, 3, 1).numpy())
    g = R.randn((B, Hr + 5, Wr + 4, C), 2, Hi)
    F.pad(up, (3, 1, 2, 3)).backward(t64(g).permute(0, 3, 1, 2))
    d, bd = R.bilinear_bwd(g, Hi, Wi, Hr, Wr, align, 2, 3, dtype=np.float64)
    close(d, xt.grad.permute(0, 2, 3, 1).numpy())
    # fp32 index and weights: fp32 F.interpolate within 4 ulp of the bound's scale A = sum |w| |v|
    v32, b32 = R.bilinear_fwd(x, Hr, Wr, align)
    check_bound(v32, b32)
    check_bound(*R.bilinear_bwd(g, Hi, Wi, Hr, Wr, align, 2, 3))
    A = b32 / ((4 + 2) * R.U)
    t32 = F.interpolate(torch.from_numpy(x).permute(0, 3, 1, 2), size=(Hr, Wr), mode="bilinear", align_corners=bool(align))
    err = np.abs(v32 - t32.permute(0, 2, 3, 1).numpy().astype(np.float64))
    assert (err <= 4 * 2.0 ** -23 * A).all(), float((err / np.maximum(A, 1e-300)).max() / 2.0 ** -23)
    # accumulate and ReLU
    old = R.randn(v32.shape, 3)
    va, ba = R.bilinear_fwd(x, Hr, Wr, align, out_old=old, relu=True)
    close(va, np.maximum(v32 + old, 0.0))
    assert (ba >= b32).all()
    da, _ = R.bilinear_bwd(g, Hi, Wi, Hr, Wr, align, 2, 3, din_old=x)
    close(da, R.bilinear_bwd(g, Hi, Wi, Hr, Wr, align, 2, 3)[0] + x)


def test_swapped_align_corners_breaks_the_bound():
    for name, Hi, Wi, Hr, Wr in R.RESIZE_GEOMETRIES:
        if (Hi, Wi) == (Hr, Wr) or Hi * Wi == 1:
            continue          # identity and a one-pixel source do not depend on the mode
        x = R.randn((1, Hi, Wi, 4), 5, Hi)
        v1, b1 = R.bilinear_fwd(x, Hr, Wr, 1)
        v0, _ = R.bilinear_fwd(x, Hr, Wr, 0)
        assert (np.abs(v1 - v0) > b1).any(), name
        g = R.randn((1, Hr, Wr, 4), 6, Hi)
        d1, bd1 = R.bilinear_bwd(g, Hi, Wi, Hr, Wr, 1)
        d0, _ = R.bilinear_bwd(g, Hi, Wi, Hr, Wr, 0)
        assert (np.abs(d1 - d0) > bd1).any(), name


@pytest.mark.parametrize("case", R.FUSE_CASES, ids=lambda c: c[0])
def test_fuse_sum_reference_is_torch(case):
    _, B, H, W, C, n_same, lows, align, relu = case
    C = min(C, 12)
    same = [R.randn((B, H, W, C), 1, i) for i in range(n_same)]
    low = [R.randn((B, h, w, C), 2, j) for j, (h, w) in enumerate(lows)]
    want = sum(t64(t).permute(0, 3, 1, 2) for t in same)
    for t in low:
        want = want + F.interpolate(t64(t).permute(0, 3, 1, 2), size=(H, W), mode="bilinear", align_corners=bool(align))
    if relu:
        want = torch.relu(want)
    v, b = R.fuse_sum(same, low, align, relu, dtype=np.float64)
    close(v, want.permute(0, 2, 3, 1).numpy())
    check_bound(*R.fuse_sum(same, low, align, relu))


def test_glue_references():
    a, b = R.randn((3, 5, 7, 8), 1), R.randn((3, 5, 7, 8), 2)
    assert np.array_equal(R.add(a, b, True), torch.relu(torch.from_numpy(a) + torch.from_numpy(b)).numpy())
    assert np.array_equal(R.copy(a, b), a + b) and np.array_equal(R.copy(a), a)
    z = a.copy()
    z.reshape(-1)[::3] = 0.0
    z.reshape(-1)[1::3] = -0.0
    assert np.array_equal(R.relu_bwd(b, z), np.where(z > 0, b, 0))
    assert R.relu_bwd(b, z).reshape(-1)[:2].tolist() == [0.0, 0.0]          # exact and negative zeros do not pass
    assert R.absmax(a) == np.abs(a).max() and R.absmax(np.zeros((1, 1, 2, 4))) == 0
    n = np.arange(2 * 3 * 4 * 5, dtype=np.float32).reshape(2, 3, 4, 5)
    assert np.array_equal(R.nhwc_to_nchw(R.nchw_to_nhwc(n)), n) and R.nchw_to_nhwc(n)[1, 2, 3, 1] == n[1, 1, 2, 3]
    for _, rows, widths in R.COLS_CASES:
        w = R.randn((rows, sum(widths)), 3, rows)
        blocks = R.weight_cols_gather(w, widths)
        assert blocks.shape == (w.size,)
        off = rows * widths[0]
        if len(widths) > 1:
            assert np.array_equal(blocks[off:off + rows * widths[1]].reshape(rows, widths[1]), w[:, widths[0]:widths[0] + widths[1]])
        dw = R.randn(w.shape, 4)
        assert np.array_equal(R.weight_cols_scatter_add(blocks, rows, widths, dw), dw + w)


# =========================================================================== the bounds see a dropped pixel
@pytest.mark.parametrize("case", R.STATS_CASES, ids=lambda c: c[0])
def test_statistics_bounds_see_one_dropped_pixel(case):
    name, npix, C, nchunks, ratio, const = case
    y = R.bn_input(npix, C, ratio, const, 1, npix, C)
    gamma, beta = R.randn(C, 2) + 1.5, R.randn(C, 3)
    rm, rv = R.randn(C, 4), np.abs(R.randn(C, 5)) + 0.5
    f = R.bn_forward(y, gamma, beta, rm, rv, 0, 0.1, R.EPS, nchunks)
    for k in ("coef", "var", "running_mean", "running_var"):
        check_bound(*f[k])
    (coef, b_coef), (var, b_var) = f["coef"], f["var"]
    drop = np.abs(y).argmax(0)
    g = R.bn_forward(y, gamma, beta, rm, rv, 0, 0.1, R.EPS, nchunks, drop=drop)
    assert (np.abs(g["coef"][0][0] - coef[0]) > b_coef[0]).all(), "a dropped pixel hides inside the bound of the mean"
    if npix > 2:
        seen = np.abs(g["var"][0] - var) > b_var
        assert seen[np.arange(C) != (const if const is not None else -1)].all(), "a dropped pixel hides inside the bound of the variance"
    # rstd and z see it too, in every channel, the ill-conditioned and the constant one included (z: the end-to-end bound in
    # the centred form; the pixel is lost from the statistics only, z is still computed for it)
    if npix > 2:
        lo, hi = f["rstd_interval"]
        check_bound(coef[1], hi - lo)
        assert (lo <= coef[1]).all() and (coef[1] <= hi).all()
        assert ((g["coef"][0][1] < lo) | (g["coef"][0][1] > hi)).all(), "a dropped pixel hides inside the interval of rstd"
    res = R.randn((npix, C), 6, npix)
    for residual, relu in ((None, False), (res, False)):
        z, b_z = R.bn_end_to_end(y, f, residual, relu)
        check_bound(z, b_z)
        close(z, R.bn_apply(y, coef, residual, relu)[0])
        zg = R.bn_apply(y, g["coef"][0], residual, relu)[0]
        assert (np.abs(zg - z) > b_z).any(0).all(), "a dropped pixel hides inside the end-to-end bound of z"
    # a constant channel: the float64 variance is exactly 0 and z is beta exactly; the kernel's E[x^2] - mean^2 may leave up to
    # b_var, so rstd may fall (never rise: the kernel clamps at 0) and z stays within |scale| d_mean plus the roundings of beta
    if const is not None:
        assert var[const] == 0.0 and b_var[const] > 0 and hi[const] == coef[1][const] * (1.0 + R.U)
        z, b_z = R.bn_end_to_end(y, f)
        assert np.array_equal(z[:, const], np.full(npix, np.float64(beta[const])))
        # the statistics move z by up to about 1.5e-4 |gamma| (rstd 316, mean error 5e-7); with the fp32
        # roundings of a shift of magnitude 3.7 * 316 |gamma| on top, the bound stays within 2e-3 (|gamma| + |beta|)
        assert (b_z[:, const] <= 2e-3 * (abs(gamma[const]) + abs(beta[const]))).all(), float(b_z[:, const].max())


@pytest.mark.parametrize("case", R.BWD_CASES, ids=lambda c: c[0])
def test_backward_bounds_see_one_dropped_pixel(case):
    name, npix, C = case
    nch = R.nchunks_rule(npix, C)
    y, dz = R.bn_input(npix, C, 0.25, None, 1, npix, C), R.randn((npix, C), 2, npix)
    coef = R.bn_forward(y, None, None, None, None, None, 0.0, R.EPS, nch)["coef"][0]
    coef[2], coef[3] = coef[1] * 1.5, 0.25
    b = R.bn_backward(dz, y, coef, None, nch, dgamma=np.ones(C), dbeta=np.ones(C), dres=np.zeros((npix, C), np.float32))
    for k in ("dy", "dgamma", "dbeta"):
        check_bound(*b[k])
    drop = np.abs(dz).argmax(0)
    w = R.bn_backward(dz, y, coef, None, nch, dgamma=np.ones(C), dbeta=np.ones(C), drop=drop)
    assert (np.abs(w["dbeta"][0] - b["dbeta"][0]) > b["dbeta"][1]).all()
    if npix > 2:
        assert (np.abs(w["dy"][0] - b["dy"][0]) > b["dy"][1]).any()


# =========================================================================== the case lists reach every path
def test_channel_mappings_and_pixel_counts():
    idle = {C: R.lanes(C)[2] for C in R.CHANNEL_MAPPINGS}
    assert idle == {4: 0, 12: 1, 48: 4, 720: 76, 1024: 0} and R.lanes(720)[1] == 1 and R.lanes(1024)[1] == 1
    for cases, npix_of in ((R.GLUE_CASES, lambda c: c[1]), (R.BWD_CASES, lambda c: c[1]), (R.STATS_CASES, lambda c: c[1]),
                           (R.POOL_CASES, lambda c: c[1] * (c[2] // 2) * (c[3] // 2))):
        for C in R.CHANNEL_MAPPINGS:
            mine = [c for c in cases if c[0] == f"C{C}"]
            assert mine, C
            P = R.lanes(C)[1]
            assert P == 1 or npix_of(mine[0]) % P != 0, (C, mine[0])
    for C in R.CHANNEL_MAPPINGS:
        for a in (1, 0):
            (_, B, _, g, *_), = [c for c in R.RESIZE_CASES if c[0] == f"C{C}_a{a}"]
            Hi, Wi, Hr, Wr = R.GEOMETRY[g]
            P = R.lanes(C)[1]
            assert P == 1 or ((B * Hr * Wr) % P != 0 and (B * Hi * Wi) % P != 0)


def test_second_grid_stride_trip():
    assert R.elem_grid(4096 * 21, 48) == R.GRID_CAP and R.grid_trips(4096 * 21, 48) == 1 and R.grid_trips(4096 * 21 + 1, 48) == 2
    (_, npix, C), = [c for c in R.GLUE_CASES if c[0] == "second_trip"]
    assert R.grid_trips(npix, C) == 2
    (_, npix, C), = [c for c in R.BWD_CASES if c[0] == "second_trip"]
    assert R.grid_trips(npix, C) == 2
    (_, npix, C, *_), = [c for c in R.STATS_CASES if c[0] == "second_trip"]
    assert R.grid_trips(npix, C) == 2
    (_, B, H, W, C), = [c for c in R.POOL_CASES if c[0] == "second_trip"]
    assert R.grid_trips(B * (H // 2) * (W // 2), C) == 2 and R.grid_trips(B * ((H + 1) // 2) * ((W + 1) // 2), C) == 2
    by_name = {c[0]: c for c in R.RESIZE_CASES}
    _, B, C, g, *_ = by_name["fwd_second_trip"]
    Hi, Wi, Hr, Wr = R.GEOMETRY[g]
    assert R.grid_trips(B * Hr * Wr, C) == 2
    _, B, C, g, *_ = by_name["bwd_second_trip"]
    Hi, Wi, Hr, Wr = R.GEOMETRY[g]
    assert R.bilinear_bwd_trips(B, Hi, Wi, C, Hr) == 2
    assert all(R.bilinear_bwd_trips(c[1], *R.GEOMETRY[c[3]][:2], c[2], R.GEOMETRY[c[3]][2]) == 1 for c in R.RESIZE_CASES if c[0] != "bwd_second_trip")
    # no tensor of a case is larger than about 70 MB
    sizes = [c[1] * c[2] * c[3] * c[4] * 4 for c in R.POOL_CASES] + [c[1] * c[2] * 4 for c in R.GLUE_CASES + R.BWD_CASES]
    assert max(sizes) <= 70e6


def test_chunk_counts_and_reduction_paths():
    want = {1, 15, 16, 17, 48, 49, 64, 65, 256}
    assert want <= {c[3] for c in R.STATS_CASES}
    assert want == {R.nchunks_rule(n, 48) for n in R.BWD_NPIX_FOR_CHUNKS.values()}
    assert all(R.nchunks_rule(n, 48) == k for k, n in R.BWD_NPIX_FOR_CHUNKS.items())
    paths = {c[0]: R.stats_paths(c[1], c[2], c[3]) for c in R.STATS_CASES}
    assert "idle_lane" in paths["chunks15"] and "idle_lane" not in paths["chunks16"]
    assert "batched" not in paths["chunks48"] and "batched" in paths["chunks49"] and "tail" in paths["chunks49"]
    assert "tail" not in paths["chunks64"] and {"batched", "tail"} <= paths["chunks65"]
    assert "empty_chunk" in paths["chunks256"] and "empty_chunk" not in paths["chunks48"]
    assert any("ragged_trip" in p for p in paths.values()) and any("full_trip" in p for p in paths.values())
    bwd = [R.stats_paths(n, C, R.nchunks_rule(n, C)) for _, n, C in R.BWD_CASES]
    assert {"idle_lane", "batched", "tail", "ragged_trip", "full_trip"} <= set().union(*bwd)
    assert {c[1] for c in R.STATS_CASES} >= {1, 2} and {c[1] for c in R.BWD_CASES} >= {1, 2}
    assert {c[4] for c in R.STATS_CASES} >= {0.25, 8, 32, 128} and any(c[5] is not None for c in R.STATS_CASES)
    assert set(R.GROUP_SIZES) == {1, 2, R.BN_MAXG} and all(len(v) == k for k, v in R.GROUP_SIZES.items())
    assert len({p for p in R.GROUP_SIZES[8]}) == 8


def test_every_row_split_instance_is_reached():
    rs = {}
    for name, B, C, g, *_ in R.RESIZE_CASES:
        Hi, Wi, Hr, Wr = R.GEOMETRY[g]
        rs.setdefault(R.bilinear_bwd_rs(B, Hi, Wi, C, Hr), []).append(name)
    assert set(rs) == {1, 2, 4, 8}, rs
    assert "rs8_a1" in rs[8] and "rs4_a1" in rs[4] and "up_int_a1" in rs[2] and "down_4x_a0" in rs[1] and "Hr1_a1" in rs[1]
    # scale 0 (the "whole range" branch of the transpose): align_corners with one output row / column, or a one-pixel source
    zero = [n for n, Hi, Wi, Hr, Wr in R.RESIZE_GEOMETRIES if R.resize_scale(Hi, Hr, 1) == 0 or R.resize_scale(Wi, Wr, 1) == 0]
    assert {"one_pixel", "Hr1", "Wr1"} <= set(zero)
    both = {(c[3], c[4]) for c in R.RESIZE_CASES}
    assert all((g[0], a) in both for g in R.RESIZE_GEOMETRIES[:-2] for a in (1, 0))
    flags = {(bool(c[9]), bool(c[10])) for c in R.RESIZE_CASES}
    assert {(True, True), (True, False), (False, True), (False, False)} == flags
    assert any(c[5] and c[7] > 0 and c[8] > 0 and c[7] + R.GEOMETRY[c[3]][2] < c[5] and c[8] + R.GEOMETRY[c[3]][3] < c[6] for c in R.RESIZE_CASES)
    assert {c[7] for c in R.FUSE_CASES} == {0, 1}


def test_batchnorm_flags_are_all_set():
    """every BatchNorm flag of the issue's list is set by a case of BN_FLAG_SPECS (tests/test_bnelem_gpu.py runs each of them,
    forward and backward), and every key a case sets is one the defaults know"""
    specs = {k: dict(R.BN_FLAG_DEFAULTS, **v) for k, v in R.BN_FLAG_SPECS.items()}
    assert all(set(v) <= set(R.BN_FLAG_DEFAULTS) for v in R.BN_FLAG_SPECS.values())

    def some(**want):
        return any(all(s[k] == v for k, v in want.items()) for s in specs.values())
    assert some(null_params=True) and some(null_running=True) and some(null_params=False, null_running=False)
    assert some(repeat=3, stat_div=3) and specs["repeat3_stat_div3"]["_npix"] % 3 == 0
    assert some(_eval=True, relu="none") and some(_eval=True, relu="z", dres="acc") and some(_eval=False)
    assert {s["relu"] for s in specs.values()} == {"none", "z", "recomputed", "mask"}
    assert {s["dres"] for s in specs.values()} == {"none", "write", "acc"} and some(dres="acc", _eval=False)
    assert some(own_dy=True) and some(own_dy=False, relu="mask")          # dy in a buffer of its own, and in place over dz
    assert some(grads=False) and some(grads=True)                         # (dgamma / dbeta are pre-filled with non-zero values)
    assert some(strided=True, own_dy=True, dres="acc", residual=True) and some(strided=True, own_dy=False, relu="mask")
    assert all(s["dres"] == "none" or s["residual"] for s in specs.values())
    # groups: one problem brings mask bytes and another does not
    kinds = {n: [R.group_relu_kind(i, npix) for i, (npix, C) in enumerate(v)] for n, v in R.GROUP_SIZES.items()}
    assert kinds[2] == ["mask", "z"] and {"mask", "z", "recomputed"} <= set(kinds[8])


def test_builders_leave_no_near_zero_pre_activation():
    for npix, C in ((427, 48), (90, 12)):
        gamma, beta = R.randn(C, 2) + 1.5, R.randn(C, 3)
        for res in (None, R.randn((npix, C), 4)):
            y0 = R.bn_input(npix, C, 0.25, None, 1, npix)
            assert R.near_zero_left(y0, gamma, beta, R.EPS, res) > 0          # (the builder has something to do)
            y = R.clear_of_zero(y0, gamma, beta, R.EPS, res)
            assert R.near_zero_left(y, gamma, beta, R.EPS, res) == 0 and y.dtype == np.float32


def test_constants_stay_small():
    # (every derivation has run by now in this module's other tests; run the ones a -k selection might have skipped)
    R.bn_fold(np.ones((1, 1)), None, None, None, np.zeros(1), np.ones(1), R.EPS)
    y = R.randn((8, 4), 1)
    c = R.bn_forward(y, None, None, np.zeros(4), np.ones(4), 0, 0.1, R.EPS, 1)["coef"][0]
    R.bn_apply(y, c)
    R.bn_eval_coef(None, None, np.zeros(4), np.ones(4), R.EPS)
    R.bn_end_to_end(y, R.bn_forward(y, None, None, None, None, None, 0.1, R.EPS, 1))
    R.bn_backward(y, y, c, None, 1, dgamma=np.zeros(4), dbeta=np.zeros(4))
    R.bn_backward(y, y, c, None, 1, eval_mode=True)
    R.bilinear_fwd(y.reshape(1, 2, 4, 4), 3, 5, 1)
    R.bilinear_bwd(y.reshape(1, 2, 4, 4), 1, 2, 2, 4, 1)
    R.fuse_sum([y.reshape(1, 2, 4, 4)], [], 1, True)
    assert len(R.CONSTANTS) >= 17 and all(0 < v <= R.C_MAX for v in R.CONSTANTS.values()), R.CONSTANTS
