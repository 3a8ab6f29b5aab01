"""The kernels downstream of the backbone -- csrc/head.hip, compose.hip, loss.hip and the AdamW kernels of csrc/optim.hip -- against the fp64
references of tests/headloss_ref.py, at the shapes where they take another path: every head template and thread mapping,
both pixel loops striding, both align_corners values and down-sampling in the logits resize, singleton / 16-child / chained
/ saturated composition, the 16-wide loss and metrics instances, several loss blocks, the consistency backward, AdamW's
grid-stride loop and device-scalar state.  Bars are those of tests/test_kernels_gpu.py (headloss_ref.BAR_*); inputs and
case lists are shared with tests/test_headloss_cpu.py, which pins the references and the room fp32 has at these inputs.
Which branch a case takes is derived from the host code next to the case lists in headloss_ref.py (the library counts
launches for the convolution, augment, decode and score families only).  Run with -s for the worst rel per group."""
import numpy as np
import pytest
import torch

from tests import headloss_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = 7.25
WORST = {}


@pytest.fixture(scope="module")
def ops():
    from hrseg_amd import ops as o
    assert torch.cuda.is_available()
    yield o
    for group, d in WORST.items():
        print(f"\nworst vs fp64, {group}: " + ", ".join(f"{k} {v[0]:.2e} (bar {v[1]:.0e})" for k, v in d.items()))


@pytest.fixture
def deterministic():
    from hrseg_amd import _lib
    _lib.set_deterministic(True)
    yield
    _lib.set_deterministic(False)


def check(group, name, got, ref, bar, absolute=False):
    d = R.absdiff(got, ref) if absolute else R.rel(got, ref)
    w = WORST.setdefault(group, {})
    w[name] = (max(w.get(name, (0.0, bar))[0], d), bar)
    assert d < bar, (group, name, d, bar)


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous().cuda()


def nchw(x):
    return x.permute(0, 3, 1, 2).contiguous().cpu()


def in_slice(x_nhwc, pad_lo, pad_hi):
    """the NHWC tensor as a channel slice of a wider sentinel-filled buffer -> (buffer, view)"""
    B, H, W, C = x_nhwc.shape
    buf = torch.full((B, H, W, pad_lo + C + pad_hi), SENTINEL, device="cuda")
    view = buf[..., pad_lo:pad_lo + C]
    view.copy_(x_nhwc)
    return buf, view


def outside_untouched(buf, pad_lo, C):
    return bool((buf[..., :pad_lo] == SENTINEL).all()) and bool((buf[..., pad_lo + C:] == SENTINEL).all())


# ================================================================================================ head
def _head_gpu(ops, case, group="head"):
    from hrseg_amd._lib import call, ptr
    nf, cout, film, has_bias, H, W, sliced, df_acc = case
    B = R.HEAD_B
    x, ref = R.head_inputs(case), R.head_run(case, torch.float64)
    w, bias = x["w"].cuda(), x["bias"].cuda() if has_bias else None
    gb = x["gb"].cuda() if film else None
    f, dz = nhwc(x["f"]), nhwc(x["dz"])
    if sliced:                                  # ldf = F + 12 > F, ldz = Cout + 3, lddf = F + 8, lddz = Cout + 5
        _, f = in_slice(f, 4, 8)
        _, dz = in_slice(dz, 2, 3)
        zbuf = torch.full((B, H, W, cout + 3), SENTINEL, device="cuda")
        z = zbuf[..., 2:2 + cout]
        call("hrseg_head_fwd", ptr(f), ops._ld(f), ptr(gb), ptr(w), ptr(bias), ptr(z), cout + 3, B, H * W, nf, cout)
        assert outside_untouched(zbuf, 2, cout)
    else:
        z = ops.head_fwd(f, gb, w, bias)
    check(group, "z", nchw(z), ref["z"], R.HEAD_BARS["z"])

    g = torch.Generator().manual_seed(nf + cout)
    dw0, db0, dgb0 = torch.randn(cout, nf, generator=g), torch.randn(cout, generator=g), torch.randn(B, 2 * nf, generator=g)
    df0 = torch.randn(B, H, W, nf, generator=g)
    dw, db = dw0.cuda(), db0.cuda() if has_bias else None           # non-zero start: the contract is +=
    dgb = dgb0.cuda() if film else None
    dfbuf = None
    if sliced:
        dfbuf, df = in_slice(df0.cuda() if df_acc else torch.zeros(B, H, W, nf, device="cuda"), 4, 4)
    else:
        df = df0.cuda() if df_acc else None
    df = ops.head_bwd(f, gb, w, dz, dw, db, dgb, df=df, df_accumulate=df_acc)
    if dfbuf is not None:
        assert outside_untouched(dfbuf, 4, nf)
    got_df = nchw(df).double() - (df0.permute(0, 3, 1, 2).double() if df_acc else 0.0)
    check(group, "df", got_df, ref["df"], R.HEAD_BARS["df"])
    check(group, "dw", dw.cpu().double() - dw0.double(), ref["dw"], R.HEAD_BARS["dw"])
    if has_bias:
        check(group, "dbias", db.cpu().double() - db0.double(), ref["dbias"], R.HEAD_BARS["dbias"])
    if film:
        check(group, "dgb", dgb.cpu().double() - dgb0.double(), ref["dgb"], R.HEAD_BARS["dgb"])
    # want_df=False: the reduced gradients alone, from zero
    dw2, db2 = torch.zeros_like(dw), torch.zeros_like(db) if has_bias else None
    dgb2 = torch.zeros_like(dgb) if film else None
    assert ops.head_bwd(f, gb, w, dz, dw2, db2, dgb2, want_df=False) is None
    check(group, "dw", dw2, ref["dw"], R.HEAD_BARS["dw"])
    if has_bias:
        check(group, "dbias", db2, ref["dbias"], R.HEAD_BARS["dbias"])
    if film:
        check(group, "dgb", dgb2, ref["dgb"], R.HEAD_BARS["dgb"])
    return z, df, dw2, db2, dgb2


@pytest.mark.parametrize("case", R.HEAD_CASES, ids=lambda c: f"F{c[0]}-C{c[1]}-{c[4]}x{c[5]}")
def test_head_fwd_bwd(ops, case):
    _head_gpu(ops, case)


@pytest.mark.parametrize("case", [R.HEAD_CASES[3], R.HEAD_CASES[7]], ids=lambda c: f"F{c[0]}-C{c[1]}")
def test_head_deterministic_mode_meets_the_bars_and_repeats_bit_for_bit(ops, deterministic, case):
    a = _head_gpu(ops, case, "head deterministic")
    b = _head_gpu(ops, case, "head deterministic")
    for u, v in zip(a, b):
        assert (u is None and v is None) or torch.equal(u, v)


# ================================================================================================ logits resize
@pytest.mark.parametrize("align", [True, False])
@pytest.mark.parametrize("sizes", R.UP_SIZES, ids=lambda s: f"{s[0]}x{s[1]}to{s[2]}x{s[3]}")
def test_logits_up(ops, sizes, align):
    Hi, Wi, Ho, Wo = sizes
    for C in R.UP_C:
        x, ref = R.up_inputs(sizes, align, C), R.up_run(sizes, align, C, torch.float64)
        check("logits_up", "out", ops.logits_up_fwd(nhwc(x["z"]), Ho, Wo, align), ref["out"], R.UP_BARS["out"])
        check("logits_up", "din", nchw(ops.logits_up_bwd(x["d"].cuda(), Hi, Wi, align)), ref["din"], R.UP_BARS["din"])


@pytest.mark.parametrize("align", [True, False])
def test_logits_up_row_strides(ops, align):
    """ldin > C on the way in, lddin > C on the way out: the padding channels keep their sentinel"""
    from hrseg_amd._lib import call, ptr
    sizes, C = R.UP_SIZES[2], 3
    Hi, Wi, Ho, Wo = sizes
    x, ref = R.up_inputs(sizes, align, C), R.up_run(sizes, align, C, torch.float64)
    _, z = in_slice(nhwc(x["z"]), 2, 3)
    check("logits_up", "out", ops.logits_up_fwd(z, Ho, Wo, align), ref["out"], R.UP_BARS["out"])
    dbuf = torch.full((R.UP_B, Hi, Wi, 2 + C + 3), SENTINEL, device="cuda")
    din = dbuf[..., 2:2 + C]
    call("hrseg_logits_up_bwd", ptr(x["d"].cuda()), R.UP_B, Hi, Wi, C, ptr(din), 2 + C + 3, Ho, Wo, int(align))
    assert outside_untouched(dbuf, 2, C)
    check("logits_up", "din", nchw(din), ref["din"], R.UP_BARS["din"])


# ================================================================================================ sigmoid / composition
def test_sigmoid(ops):
    for scale in R.SIGMOID_SCALES:
        x, ref = R.sigmoid_inputs(scale), R.sigmoid_run(scale, torch.float64)
        z, dp = x["z"].cuda(), x["dp"].cuda()
        check("sigmoid", "p", ops.sigmoid_fwd(z), ref["p"], R.SIGMOID_BARS["p"])
        check("sigmoid", "dz", ops.sigmoid_bwd(dp, z), ref["dz"], R.SIGMOID_BARS["dz"])
        base = torch.randn(z.shape, generator=torch.Generator().manual_seed(1))
        acc = ops.sigmoid_bwd(dp, z, dz=base.cuda(), accumulate=True)
        check("sigmoid", "dz", acc.cpu().double() - base.double(), ref["dz"], R.SIGMOID_BARS["dz"])


@pytest.mark.parametrize("hw", R.COMPOSE_HW, ids=lambda h: f"{h[0]}x{h[1]}")
@pytest.mark.parametrize("tree", R.TREES, ids=lambda t: f"{len(t[0])}groups{sum(t[1])}ch")
def test_compose_fwd_bwd(ops, tree, hw):
    bars = R.COMPOSE_BARS
    for scales in R.COMPOSE_SCALES:
        x, ref = R.compose_inputs(tree, scales, hw), R.compose_run(tree, scales, hw, torch.float64)
        z, pprev, dp = x["z"].cuda(), x["pprev"].cuda(), x["dp"].cuda()
        check("compose", "p", ops.compose_fwd(z, pprev, *tree), ref["p"], bars["p"])
        dz, dpp = ops.compose_bwd(dp, z, pprev, *tree)
        check("compose", "dz", dz, ref["dz"], bars["dz"])
        check("compose", "dpprev", dpp, ref["dpprev"], bars["dpprev"])
        # the [B,C,1,1] gradient of a pooled quantity, expanded without materialising it
        dpb = x["dpb"].cuda()[:, :, None, None].expand(z.shape)
        dzb, dppb = ops.compose_bwd(dpb, z, pprev, *tree)
        check("compose", "dz_b", dzb, ref["dz_b"], bars["dz_b"])
        check("compose", "dpprev_b", dppb, ref["dpprev_b"], bars["dpprev_b"])
        # accumulate flags onto non-zero buffers; dz=None / dpprev=None leave the other output as it was
        g = torch.Generator().manual_seed(2)
        bz, bp = torch.randn(z.shape, generator=g), torch.randn(pprev.shape, generator=g)
        az, ap = ops.compose_bwd(dp, z, pprev, *tree, dz=bz.cuda(), dz_accumulate=True, dpprev=bp.cuda(), dpprev_accumulate=True)
        check("compose", "dz", az.cpu().double() - bz.double(), ref["dz"], bars["dz"])
        check("compose", "dpprev", ap.cpu().double() - bp.double(), ref["dpprev"], bars["dpprev"])
        only_z, none_p = ops.compose_bwd(dp, z, pprev, *tree, want_dpprev=False)
        none_z, only_p = ops.compose_bwd(dp, z, pprev, *tree, want_dz=False)
        assert none_p is None and none_z is None and torch.equal(only_z, dz) and torch.equal(only_p, dpp)


@pytest.mark.parametrize("hw", R.COMPOSE_HW, ids=lambda h: f"{h[0]}x{h[1]}")
def test_compose_three_level_chain(ops, hw):
    """level 2 composed from the COMPOSED level 1; the backward runs through both, level 1's own upstream gradient is the
    buffer the second composition accumulates its parent gradient onto"""
    for scales in R.COMPOSE_SCALES:
        x, ref = R.chain_inputs(scales, hw), R.chain_run(scales, hw, torch.float64)
        p0, z1, z2 = x["p0"].cuda(), x["z1"].cuda(), x["z2"].cuda()
        p1 = ops.compose_fwd(z1, p0, *R.CHAIN[0])
        p2 = ops.compose_fwd(z2, p1, *R.CHAIN[1])
        check("compose chain", "p1", p1, ref["p1"], R.CHAIN_BARS["p1"])
        check("compose chain", "p2", p2, ref["p2"], R.CHAIN_BARS["p2"])
        dz2, dp1 = ops.compose_bwd(x["d2"].cuda(), z2, p1, *R.CHAIN[1], dpprev=x["d1"].cuda(), dpprev_accumulate=True)
        dz1, dp0 = ops.compose_bwd(dp1, z1, p0, *R.CHAIN[0])
        for name, got in (("dz2", dz2), ("dz1", dz1), ("dp0", dp0)):
            check("compose chain", name, got, ref[name], R.CHAIN_BARS[name])


# ================================================================================================ loss / metrics
@pytest.mark.parametrize("C", R.LOSS_C)
def test_loss_fwd_bwd(ops, C):
    for hw in R.LOSS_HW:
        for B in R.LOSS_B:
            for pattern in R.LOSS_PATTERNS:
                x, ref = R.loss_inputs(C, hw, B, pattern), R.loss_run(C, hw, B, pattern, torch.float64)
                z, t = x["z"].cuda(), x["t"].cuda()
                out, coef = ops.loss_fwd(z, t, torch.tensor(x["w"]).cuda())
                out = out.cpu()
                check("loss", "ce", out[0], ref["ce"], R.LOSS_BARS["ce"], absolute=True)
                check("loss", "dice", out[1], ref["dice"], R.LOSS_BARS["dice"], absolute=True)
                assert float(out[2]) == ref["nvalid"], (C, hw, B, pattern)
                up = torch.tensor(R.LOSS_UPSTREAM).cuda()
                dz = ops.loss_bwd(z, t, coef, up)
                check("loss", "dz", dz, ref["dz"], R.LOSS_BARS["dz"])
                # the buffer accumulated onto has the gradient's own magnitude (1e-3 and less at hw >= 255): on an O(1) buffer
                # the fp32 rounding of the SUM alone, 1e-7 absolute, would be 5e-5 of max |dz| and hide the kernel's error
                scale = float(ref["dz"].abs().max()) or 1.0
                base = scale * torch.randn(z.shape, generator=torch.Generator().manual_seed(3))
                acc = ops.loss_bwd(z, t, coef, up, dz=base.cuda(), accumulate=True)
                check("loss", "dz", acc.cpu().double() - base.double(), ref["dz"], R.LOSS_BARS["dz"])


@pytest.mark.parametrize("child", [False, True])
@pytest.mark.parametrize("C", [9, 16])
def test_predict_metrics_16_wide_instance(ops, C, child):
    """the train-loop form (logits + ternary targets, mask_pred=1) at C = 9 and 16 -- the CT=16 instance -- against the
    per-pixel brute force of tests/test_metrics_bruteforce.py; its test()-loop form runs there with the same C"""
    from hrseg_amd import train as PT
    from hrseg_amd.Metrics import performance_metrics as PP
    from tests.test_metrics_bruteforce import brute_force_level_metrics
    g = np.random.Generator(np.random.PCG64(100 + C + int(child)))
    B, H, W = 2, 9, 8
    z = g.standard_normal((B, C, H, W)).astype(np.float32)
    t = np.moveaxis(np.eye(C, dtype=np.float32)[g.integers(0, C, size=(B, H, W))], -1, 1).copy()
    if child:
        t[np.broadcast_to((g.random((B, H, W)) < 0.4)[:, None], t.shape)] = -1.0
    else:
        t[0, C - 1, :3] = -1.0
    oh = np.moveaxis(np.eye(C, dtype=np.float32)[z.argmax(1)], -1, 1)
    p_in, t_in = np.where(t == -1, 0.0, oh).astype(np.float32), np.where(t == -1, 0.0, t).astype(np.float32)
    want = brute_force_level_metrics(p_in, t_in, child)
    onehot, cm = ops.predict_metrics(torch.from_numpy(z).cuda(), torch.from_numpy(t).cuda(), child=child, mask_pred=True)
    assert np.array_equal(onehot.cpu().numpy(), p_in) and int(cm.sum()) == B * H * W
    vec = PT._metric_vectors([cm] if not child else [torch.zeros((C, C), dtype=torch.int64, device="cuda"), cm])
    for k in PP.METRIC_NAMES:
        got = vec[k].cpu().numpy()
        assert np.allclose(got[C:] if child else got, want[k], atol=1e-7), (C, child, k)


# ================================================================================================ consistency
def _cons_expected(ref):
    """the backward is +-(g * scale) per pixel, both factors fp32 as the kernel multiplies them"""
    gs = float(np.float32(R.CONS_G) * np.float32(R.CONS_SCALE))
    return gs * torch.sign(ref["diffs"])                      # [B,G,H,W]


@pytest.mark.parametrize("hw", R.CONS_HW, ids=lambda h: f"{h[0]}x{h[1]}")
@pytest.mark.parametrize("tree", R.TREES, ids=lambda t: f"{len(t[0])}groups{sum(t[1])}ch")
def test_consistency_fwd_bwd(ops, tree, hw):
    parents, sizes = tree
    for maker in (R.cons_inputs, R.cons_onehot_inputs):
        x = maker(tree, hw)
        ref = R.cons_run(x, tree, torch.float64)
        cur, prev = x["cur"].cuda(), x["prev"].cuda()
        n = cur.shape[0] * cur.shape[2] * cur.shape[3]
        check("consistency", "mean", ops.consistency_sums(cur, prev, parents, sizes).cpu() / n, ref["mean"],
              R.CONS_BARS["mean"], absolute=True)
        dcur, dprev = ops.consistency_bwd(cur, prev, torch.tensor([R.CONS_G]).cuda(), R.CONS_SCALE, parents, sizes)
        dcur, dprev = dcur.cpu(), dprev.cpu()
        keep = ~ref["tie"] if maker is R.cons_inputs else torch.ones_like(ref["tie"])     # one-hot ties are exact: compared
        assert float((~keep).any(dim=1).float().mean()) <= R.CONS_MAX_TIE_SHARE
        sg = _cons_expected(ref)
        start = 0
        want_prev = torch.zeros(prev.shape, dtype=torch.float64)
        used = torch.zeros(prev.shape, dtype=torch.bool)
        for gi, (par, sz) in enumerate(zip(parents, sizes)):
            for c in range(start, start + sz):
                assert torch.equal(dcur[:, c].double()[keep[:, gi]], sg[:, gi][keep[:, gi]]), (gi, c)
            want_prev[:, par] = -sg[:, gi]
            used[:, par] = ~keep[:, gi]
            start += sz
        assert torch.equal(dprev.double()[~used], want_prev[~used])       # parents without children get exact zeros
        if maker is R.cons_onehot_inputs:
            assert float((dcur == 0).float().mean()) > 0.3


@pytest.mark.parametrize("reduction", ["mean", "sum"])
def test_consistency_loss_end_to_end(ops, reduction):
    """hierarchical_consistency_loss on leaf tensors that require grad: hrseg_consistency forward, hrseg_consistency_bwd through
    autograd (the training loop feeds it one-hots without gradient, so nothing else runs that kernel)"""
    from hrseg_amd.Metrics import losses as PL
    ref = R.e2e_run(reduction, torch.float64)
    probs = [p.cuda().requires_grad_(True) for p in R.e2e_inputs()]
    loss = PL.hierarchical_consistency_loss(probs, R.E2E_LEVELS, R.E2E_PARENT_OF, reduction)
    (1.3 * loss).backward()
    # 'mean' is O(1): 2e-6 absolute.  'sum' is the same quantity times the 798 pixels and leaves the kernel as ONE fp32
    # number, so the bar is 2e-6 of its magnitude (an fp32 ulp there is 6e-8 of it)
    assert abs(float(loss) - float(ref["loss"])) < R.BAR_LOSS * max(1.0, abs(float(ref["loss"])))
    for got, want in zip(probs, ref["grads"]):
        check("consistency", "e2e grads", got.grad, want, R.BAR_POINT)


# ================================================================================================ AdamW
def _hyper(lr, wd):
    return torch.tensor([lr, R.ADAMW_BETA1, R.ADAMW_BETA2, R.ADAMW_EPS, wd, R.ADAMW_GSCALE], dtype=torch.float32)


@pytest.mark.parametrize("n", R.ADAMW_N)
def test_adamw_both_entry_points(ops, n):
    x = R.adamw_inputs(n)
    p0, grads = x["p"].cuda(), [g.cuda() for g in x["grads"]]
    for wd in R.ADAMW_WDS:
        ref = {k: v.cuda() for k, v in R.adamw_run(x, wd, torch.float64).items()}
        for dev in (False, True):
            p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
            hyper, state = _hyper(R.ADAMW_LRS[0], wd).cuda(), torch.zeros(3, device="cuda")
            for k, lr in enumerate(R.ADAMW_LRS):
                if dev:
                    hyper[0] = lr                                   # a scheduler's new lr: written to the device, no new launch arguments
                    ops.adamw_dev(p, grads[k], m, v, hyper, state)
                    assert np.allclose(state.cpu().numpy(), np.array(R.adamw_state(k + 1), np.float32), rtol=1.2e-7, atol=0)
                else:
                    ops.adamw(p, grads[k], m, v, lr, R.ADAMW_BETA1, R.ADAMW_BETA2, R.ADAMW_EPS, wd, k + 1, R.ADAMW_GSCALE)
            for name, got in (("p", p), ("m", m), ("v", v)):
                d = float((got.double() - ref[name]).abs().max() / ref[name].abs().max())
                w = WORST.setdefault("adamw", {})
                w[name] = (max(w.get(name, (0.0, 0))[0], d), R.ADAMW_BARS[name])
                assert d < R.ADAMW_BARS[name], (n, wd, dev, name, d)


def test_adamw_refuses_unaligned_views(ops):
    p, g, m, v = (torch.randn(64, device="cuda") for _ in range(4))
    before = [t.clone() for t in (p, m, v)]
    hyper, state = _hyper(1e-3, 0.01).cuda(), torch.zeros(3, device="cuda")
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        ops.adamw(p[1:], g[1:], m[1:], v[1:], 1e-3, 0.9, 0.999, 1e-8, 0.01, 1)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        ops.adamw_dev(p[1:], g[1:], m[1:], v[1:], hyper, state)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip((p, m, v), before)) and float(state.abs().max()) == 0.0


# ================================================================================================ GAP / FiLM linear
@pytest.mark.parametrize("hw", R.GAP_HW, ids=lambda h: f"{h[0]}x{h[1]}")
def test_gap_nchw(ops, hw):
    check("gap", "cond", ops.gap_nchw(R.gap_inputs(hw)["p"].cuda()), R.gap_run(hw, torch.float64)["cond"], R.GAP_BARS["cond"])


@pytest.mark.parametrize("case", R.FILM_CASES, ids=lambda c: f"B{c[0]}-Cc{c[1]}-F2_{c[2]}")
def test_film_linear(ops, case):
    x, ref = R.film_inputs(case), R.film_run(case, torch.float64)
    cond, wl, bl, dgb = (x[k].cuda() for k in ("cond", "wl", "bl", "dgb"))
    check("film_linear", "gb", ops.film_linear_fwd(cond, wl, bl), ref["gb"], R.FILM_BARS["gb"])
    g = torch.Generator().manual_seed(4)
    dwl0, dbl0 = torch.randn(wl.shape, generator=g), torch.randn(bl.shape, generator=g)
    dwl, dbl = dwl0.cuda(), dbl0.cuda()                              # non-zero start: the contract is +=
    dcond = ops.film_linear_bwd(cond, wl, dgb, dwl, dbl, R.FILM_DCOND_SCALE)
    check("film_linear", "dcond", dcond, ref["dcond"], R.FILM_BARS["dcond"])
    check("film_linear", "dwl", dwl.cpu().double() - dwl0.double(), ref["dwl"], R.FILM_BARS["dwl"])
    check("film_linear", "dbl", dbl.cpu().double() - dbl0.double(), ref["dbl"], R.FILM_BARS["dbl"])
    dwl2, dbl2 = torch.zeros_like(dwl), torch.zeros_like(dbl)
    assert ops.film_linear_bwd(cond, wl, dgb, dwl2, dbl2, R.FILM_DCOND_SCALE, want_dcond=False) is None
    check("film_linear", "dwl", dwl2, ref["dwl"], R.FILM_BARS["dwl"])
    check("film_linear", "dbl", dbl2, ref["dbl"], R.FILM_BARS["dbl"])
