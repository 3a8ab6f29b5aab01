"""The BatchNorm, pooling, resize and glue kernels (csrc/bn.hip, csrc/elem.hip) against the float64 references of
tests/bnelem_ref.py: every instance, loop and flag the case lists there reach, every comparison under a per-element bound
the reference derives itself (or for equality where fp32 is exact).  Only arguments the kernels are written for are passed:
aligned pointers, ld >= C, ld % 4 == 0, buffers sized by the helpers from the sizes the call is given; the refusals are
tests/test_bnelem_abi.py's.  `pytest -s` prints the largest error / bound per case family."""
import numpy as np
import pytest
import torch

from tests import bnelem_ref as R

pytestmark = pytest.mark.gpu

RATIOS = {}          # family -> largest error / bound seen


@pytest.fixture(scope="module")
def ops():
    from hrseg_amd import ops as o
    assert torch.cuda.is_available()
    return o


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    for k in sorted(RATIOS):
        print(f"\nbnelem ratio {k}: {RATIOS[k]:.4f}", end="")
    print()


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def within(family, got, value, bound, what=""):
    """|got - value| <= bound element by element (bound 0: equality); records the largest ratio of the family"""
    got, value, bound = np.asarray(got, np.float64), np.asarray(value, np.float64), np.asarray(bound, np.float64)
    assert got.shape == value.shape == bound.shape, (family, what, got.shape, value.shape, bound.shape)
    assert np.isfinite(got).all(), (family, what, "non-finite result")
    err = np.abs(got - value)
    ratio = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    RATIOS[family] = max(RATIOS.get(family, 0.0), ratio)
    print(f"{family} {what}: error / bound = {ratio:.4f}")
    bad = err > bound
    assert not bad.any(), (family, what, f"{int(bad.sum())} elements beyond the bound, worst ratio {ratio:.3f}")


class Wide:
    """a channel slice [..., left:left + C] of a wider NHWC buffer pre-filled with random int32 bits: an offset base pointer,
    ld > C, both multiples of 4.  unchanged(): every byte outside the slice is as it was"""

    def __init__(self, shape, key, fill=None, left=8, right=4):
        B, H, W, C = shape
        bits = R.rng(77, key, C).integers(-2 ** 31, 2 ** 31, size=(B, H, W, left + C + right), dtype=np.int64).astype(np.int32)
        self.bits = torch.from_numpy(bits).cuda()
        self.view = self.bits.view(torch.float32)[..., left:left + C]
        if fill is not None:
            self.view.copy_(dev(np.asarray(fill, np.float32).reshape(shape)))
        self.before, self.left, self.C = self.bits.clone(), left, C

    def unchanged(self):
        lo, hi = self.left, self.left + self.C
        return torch.equal(self.bits[..., :lo], self.before[..., :lo]) and torch.equal(self.bits[..., hi:], self.before[..., hi:])


def operand(a, shape, strided, key):
    """-> (device tensor holding a, Wide or None)"""
    if strided:
        w = Wide(shape, key, fill=a)
        return w.view, w
    return dev(np.asarray(a, np.float32).reshape(shape)), None


def output(shape, strided, key, fill=None):
    if strided:
        w = Wide(shape, key, fill=fill)
        return w.view, w
    t = torch.empty(shape, dtype=torch.float32, device="cuda") if fill is None else dev(np.asarray(fill, np.float32).reshape(shape))
    return t, None


# =========================================================================== BatchNorm
def bn_spec(npix, C, **kw):
    s = dict(npix=npix, C=C, relu="none", residual=False, dres="none", own_dy=False, null_params=False, null_running=False, strided=False,
             nchunks=None, ratio=0.25, const=None, repeat=1, stat_div=1, grads=True)
    s.update(kw)
    return s


def run_bn(ops, family, specs, eval_mode=False, backward=True):
    """forward (training statistics, or the running ones with eval_mode) and backward of a group of problems, every output
    of every problem against the reference"""
    n = len(specs)
    P = []
    for i, s in enumerate(specs):
        npix, C = s["npix"], s["C"]
        key = (npix, C, i)
        shape = (1, 1, npix, C)
        p = dict(s=s, shape=shape)
        p["gamma"], p["beta"] = (None, None) if s["null_params"] else (R.randn(C, 2, *key) + 1.5, R.randn(C, 3, *key))
        p["rm"], p["rv"] = (None, None) if s["null_running"] else (R.randn(C, 4, *key), np.abs(R.randn(C, 5, *key)) + 0.5)
        p["res"] = R.randn((npix, C), 6, *key) if s["residual"] else None
        y = R.bn_input(npix, C, s["ratio"], s["const"], 1, *key)
        if s["relu"] == "recomputed":
            y = R.clear_of_zero(y, p["gamma"], p["beta"], R.EPS, p["res"])
        p["y"], p["dz"] = y, R.randn((npix, C), 7, *key)
        p["nch"] = s["nchunks"] or R.nchunks_rule(npix, C)
        p["y_d"], _ = operand(y, shape, s["strided"], 1)
        p["res_d"], _ = operand(p["res"], shape, s["strided"], 2) if s["residual"] else (None, None)
        p["z_d"], p["z_w"] = output(shape, s["strided"], 3)
        for k in ("gamma", "beta", "rm", "rv"):
            p[k + "_d"] = None if p[k] is None else dev(p[k])
        p["nbt_d"] = None if s["null_running"] else torch.full((1,), 41, dtype=torch.int64, device="cuda")
        p["mask_d"] = torch.zeros(npix * (C // 4), dtype=torch.uint8, device="cuda") if s["relu"] == "mask" else None
        p["part_d"] = torch.empty(p["nch"] * 2 * C, dtype=torch.float64, device="cuda")          # sized from the nchunks the call is given
        P.append(p)
    items = [dict(y=p["y_d"], gamma=p["gamma_d"], beta=p["beta_d"], rm=p["rm_d"], rv=p["rv_d"], nbt=p["nbt_d"], momentum=0.1, eps=R.EPS,
                  residual=p["res_d"], relu=p["s"]["relu"] != "none", out=p["z_d"], relu_mask=p["mask_d"], repeat=p["s"]["repeat"],
                  stat_div=p["s"]["stat_div"], **({} if eval_mode else dict(partial=(p["part_d"], p["nch"])))) for p in P]
    outs = ops.bn_fwd_group(items, not eval_mode)
    torch.cuda.synchronize()
    for i, (p, (z_d, coef_d)) in enumerate(zip(P, outs)):
        s, C, npix = p["s"], p["s"]["C"], p["s"]["npix"]
        tag = f"problem {i} of {n} ({npix} x {C})"
        coef = host(coef_d).reshape(4, C).astype(np.float64)
        relu = s["relu"] != "none"
        if eval_mode:
            within(family + "/eval coef", coef, *R.bn_eval_coef(p["gamma"], p["beta"], p["rm"], p["rv"], R.EPS), tag)
            assert np.array_equal(host(p["rm_d"]), p["rm"]) and np.array_equal(host(p["rv_d"]), p["rv"]) and int(p["nbt_d"]) == 41
        else:
            f = R.bn_forward(p["y"], p["gamma"], p["beta"], p["rm"], p["rv"], None if s["null_running"] else 41, 0.1, R.EPS, p["nch"],
                             s["repeat"], s["stat_div"])
            within(family + "/coef", coef, *f["coef"], tag)
            if not s["null_running"]:
                within(family + "/running", host(p["rm_d"]), *f["running_mean"], tag + " running_mean")
                within(family + "/running", host(p["rv_d"]), *f["running_var"], tag + " running_var")
                assert int(p["nbt_d"]) == f["nbt"], tag
            within(family + "/scale, shift from the device's mean, rstd", coef[2:], *R.bn_rows_from_rows(coef, p["gamma"], p["beta"]), tag)
            lo, hi = f["rstd_interval"]
            assert ((lo <= coef[1]) & (coef[1] <= hi)).all(), tag + ": rstd outside the interval its variance bound allows"
            # end to end, in the centred form (a constant channel: z within this of beta)
            within(family + "/z end to end", host(z_d).reshape(npix, C), *R.bn_end_to_end(p["y"], f, p["res"], relu), tag)
        zr, bz, _ = R.bn_apply(p["y"], coef, p["res"], relu)
        z = host(z_d).reshape(npix, C)
        within(family + "/z", z, zr, bz, tag)
        assert p["z_w"] is None or p["z_w"].unchanged(), tag + ": the apply wrote outside its channel slice"
        if s["relu"] == "mask":
            bits = host(p["mask_d"]).reshape(npix, C // 4)
            passed = ((bits[:, :, None] >> np.arange(4)) & 1).reshape(npix, C).astype(bool)
            assert np.array_equal(passed, z > 0) and (bits < 16).all(), tag + ": mask bytes"
            p["mask"] = passed
        elif s["relu"] == "z":
            p["mask"] = z > 0
        elif s["relu"] == "recomputed":
            pre = p["y"].astype(np.float64) * coef[2] + coef[3]
            assert (np.abs(pre) >= R.NEAR_ZERO / 2).all(), tag
            p["mask"] = pre > 0
        else:
            p["mask"] = None
        p["coef"], p["coef_d"], p["z_out"] = coef, coef_d, z_d
    if not backward:
        return
    bitems = []
    for i, p in enumerate(P):
        s, C, npix, shape = p["s"], p["s"]["C"], p["s"]["npix"], p["shape"]
        p["dg0"], p["db0"] = (R.randn(C, 8, i) if s["grads"] else None), (R.randn(C, 9, i) if s["grads"] else None)
        p["dg_d"], p["db_d"] = (dev(p["dg0"]) if s["grads"] else None), (dev(p["db0"]) if s["grads"] else None)
        p["dz_d"], p["dz_w"] = output(shape, s["strided"], 4, fill=p["dz"])                   # (dy is written over it unless own_dy)
        p["dy_d"], p["dy_w"] = output(shape, s["strided"], 5) if s["own_dy"] else (p["dz_d"], p["dz_w"])
        p["dres0"] = R.randn((npix, C), 10, i) if s["dres"] == "acc" else None
        p["dres_d"], p["dres_w"] = output(shape, s["strided"], 6, fill=p["dres0"]) if s["dres"] != "none" else (None, None)
        p["amax_d"] = torch.full((64,), 7.0, dtype=torch.float32, device="cuda")              # (the call resets it)
        it = dict(dz=p["dz_d"], z=p["z_out"] if s["relu"] == "z" else None, relu=s["relu"] != "none", y=p["y_d"], coef=p["coef_d"],
                  dgamma=p["dg_d"], dbeta=p["db_d"], dres=p["dres_d"], dres_accumulate=s["dres"] == "acc", dy_absmax=p["amax_d"],
                  relu_mask=p["mask_d"])
        if s["own_dy"]:
            it["dy"] = p["dy_d"]
        bitems.append(it)
    ops.bn_bwd_group(bitems, eval_mode)
    torch.cuda.synchronize()
    for i, p in enumerate(P):
        s, C, npix = p["s"], p["s"]["C"], p["s"]["npix"]
        tag = f"problem {i} of {n} ({npix} x {C})"
        b = R.bn_backward(p["dz"], p["y"], p["coef"], p["mask"], R.nchunks_rule(npix, C), eval_mode, p["dg0"], p["db0"],
                          None if s["dres"] == "none" else (p["dres0"] if p["dres0"] is not None else np.zeros((npix, C), np.float32)),
                          s["dres"] == "acc")
        dy = host(p["dy_d"]).reshape(npix, C)
        within(family + ("/dy (eval: one product)" if eval_mode else "/dy"), dy, *b["dy"], tag)
        if s["grads"]:
            within(family + "/dgamma dbeta", host(p["dg_d"]), *b["dgamma"], tag + " dgamma")
            within(family + "/dgamma dbeta", host(p["db_d"]), *b["dbeta"], tag + " dbeta")
        if s["dres"] != "none":
            assert np.array_equal(host(p["dres_d"]).reshape(npix, C), b["dres"]), tag + ": dres"
            assert p["dres_w"] is None or p["dres_w"].unchanged(), tag
        assert float(p["amax_d"].max()) == float(np.abs(dy).max()), tag + ": dy_absmax"
        assert p["dy_w"] is None or p["dy_w"].unchanged(), tag + ": the backward wrote outside its channel slice"
        if s["own_dy"]:
            assert np.array_equal(host(p["dz_d"]).reshape(npix, C), p["dz"]), tag + ": dz must stay as it was"


@pytest.mark.parametrize("case", R.STATS_CASES, ids=lambda c: c[0])
def test_bn_statistics(ops, case):
    name, npix, C, nchunks, ratio, const = case
    family = "bn conditioning" if name.startswith("ratio") else "bn statistics"
    run_bn(ops, family, [bn_spec(npix, C, nchunks=nchunks, ratio=ratio, const=const, relu="z")], backward=False)


@pytest.mark.parametrize("case", R.BWD_CASES, ids=lambda c: c[0])
def test_bn_backward_sizes(ops, case):
    name, npix, C = case
    run_bn(ops, "bn backward", [bn_spec(npix, C, relu="z", residual=True, dres="write")])


@pytest.mark.parametrize("flag", sorted(R.BN_FLAG_SPECS))
def test_bn_flags(ops, flag):
    kw = dict(R.BN_FLAG_DEFAULTS, **R.BN_FLAG_SPECS[flag])
    ev, npix = kw.pop("_eval"), kw.pop("_npix")
    run_bn(ops, "bn flags", [bn_spec(npix, 48, **kw)], eval_mode=ev)


@pytest.mark.parametrize("n", sorted(R.GROUP_SIZES))
def test_bn_groups(ops, n):
    """unequal problems in one launch; with more than one, even problems bring mask bytes and odd ones do not (the masked
    instance of the reduce kernel serves both), and one recomputes its mask from y"""
    specs = []
    for i, (npix, C) in enumerate(R.GROUP_SIZES[n]):
        kind = R.group_relu_kind(i, npix)
        res = kind != "recomputed"
        specs.append(bn_spec(npix, C, relu=kind, residual=res, dres=("write" if i % 2 else "acc") if res else "none", own_dy=i % 3 == 0))
    run_bn(ops, "bn groups", specs)


@pytest.mark.parametrize("i", range(len(R.FOLD_CASES)), ids=lambda i: "row%d_null_%s" % (R.FOLD_CASES[i][1], "_".join(R.FOLD_NULLS[i]) or "none"))
def test_bn_fold(ops, i):
    (cout, row), nulls = R.FOLD_CASES[i], R.FOLD_NULLS[i]
    a = dict(w=R.randn((cout, row), 1, row), bias=R.randn(cout, 2), gamma=R.randn(cout, 3) + 1.5, beta=R.randn(cout, 4), rm=R.randn(cout, 5),
             rv=np.abs(R.randn(cout, 6)) + 0.1)
    for k in nulls:
        a[k] = None
    d = {k: (None if v is None else dev(v)) for k, v in a.items()}
    w_f, b_f = ops.bn_fold(d["w"], d["bias"], d["gamma"], d["beta"], d["rm"], d["rv"], R.EPS, cout)
    (wr, bw), (br, bb) = R.bn_fold(a["w"], a["bias"], a["gamma"], a["beta"], a["rm"], a["rv"], R.EPS)
    within("bn_fold", host(w_f), wr, bw, "weight")
    within("bn_fold", host(b_f), br, bb, "bias")


# =========================================================================== max pool
def _with_strided(cases, small):
    """every case dense, and the small ones once more as channel slices of wider buffers"""
    return [pytest.param(c, st, id=c[0] + ("_strided" if st else "")) for c in cases for st in (False, True) if not st or small(c)]


@pytest.mark.parametrize("case,strided", _with_strided(R.POOL_CASES, lambda c: c[0] != "second_trip"))
def test_maxpool(ops, case, strided):
    name, B, H, W, C = case
    x = R.ties((B, H, W, C), 1, H, W, C)
    x_d, _ = operand(x, x.shape, strided, 1)
    if strided:           # (ops.maxpool2_fwd allocates its own dense output: the strided output goes through the ABI)
        from hrseg_amd import _lib
        y_d, y_w = output((B, H // 2, W // 2, C), True, 2)
        _lib.call("hrseg_maxpool2_fwd", x_d.data_ptr(), ops._ld(x_d), y_d.data_ptr(), ops._ld(y_d), B, H, W, C)
        assert y_w.unchanged()
    else:
        y_d = ops.maxpool2_fwd(x_d)
    y = R.maxpool2_fwd(x)
    assert np.array_equal(host(y_d), y)
    dy = R.randn(y.shape, 2, H)
    dy_d, _ = operand(dy, dy.shape, strided, 3)
    dx_d, dx_w = output(x.shape, strided, 4)
    ops.maxpool2_bwd(x_d, dy_d, dx=dx_d, accumulate=False)
    assert np.array_equal(host(dx_d), R.maxpool2_bwd(x, dy)), "first maximum in scan order; zero on the odd leftover"
    old = R.randn(x.shape, 5, H)
    acc_d, acc_w = output(x.shape, strided, 6, fill=old)
    ops.maxpool2_bwd(x_d, dy_d, dx=acc_d, accumulate=True)
    assert np.array_equal(host(acc_d), R.maxpool2_bwd(x, dy, dx_old=old))
    assert all(w is None or w.unchanged() for w in (dx_w, acc_w))


# =========================================================================== bilinear
@pytest.mark.parametrize("case,strided", _with_strided(R.RESIZE_CASES, lambda c: c[2] <= 48 and "4x" not in c[0]))
def test_bilinear(ops, case, strided):
    name, B, C, g, align, Hout, Wout, py, px, acc, relu = case
    Hi, Wi, Hr, Wr = R.GEOMETRY[g]
    Hout, Wout = Hout or Hr, Wout or Wr
    x = R.randn((B, Hi, Wi, C), 1, Hi, Wr, C)
    old = R.randn((B, Hout, Wout, C), 2, Hi, C)
    x_d, _ = operand(x, x.shape, strided, 1)
    out_d, out_w = output(old.shape, strided, 2, fill=old if acc else None)
    ops.bilinear_fwd(x_d, out_d, Hr, Wr, py, px, align_corners=bool(align), accumulate=acc, relu=relu)
    v, b = R.bilinear_fwd(x, Hr, Wr, align, Hout, Wout, py, px, old if acc else None, relu)
    fam = "bilinear" + (" downscale" if Hr < Hi else "")
    within(fam + " forward", host(out_d), v, b, name)
    assert out_w is None or out_w.unchanged()
    # the transpose, written and accumulated (the RS instance: bnelem_ref.bilinear_bwd_rs)
    gr = R.randn((B, Hout, Wout, C), 3, Hi, C)
    g_d, _ = operand(gr, gr.shape, strided, 3)
    din_d, din_w = output(x.shape, strided, 4, fill=x if acc else None)
    ops.bilinear_bwd(g_d, x.shape, Hr, Wr, py, px, align_corners=bool(align), din=din_d, accumulate=acc)
    d, bd = R.bilinear_bwd(gr, Hi, Wi, Hr, Wr, align, py, px, x if acc else None)
    within(fam + f" transpose RS={R.bilinear_bwd_rs(B, Hi, Wi, C, Hr)}", host(din_d), d, bd, name)
    assert din_w is None or din_w.unchanged()


@pytest.mark.parametrize("strided_out", (False, True), ids=("dense_out", "strided_out"))
@pytest.mark.parametrize("case", R.FUSE_CASES, ids=lambda c: c[0])
def test_fuse_sum(ops, case, strided_out):
    name, B, H, W, C, n_same, lows, align, relu = case
    same = [R.randn((B, H, W, C), 1, i, C) for i in range(n_same)]
    low = [R.randn((B, h, w, C), 2, j, C) for j, (h, w) in enumerate(lows)]
    same_d = [operand(t, t.shape, i % 2 == 1, 10 + i)[0] for i, t in enumerate(same)]
    low_d = [operand(t, t.shape, j % 2 == 0, 20 + j)[0] for j, t in enumerate(low)]
    if strided_out:           # (ops.fuse_sum allocates its own dense output: ldo > C goes through the ABI, as ops.fuse_sum calls it)
        from hrseg_amd import _lib
        out_d, out_w = output((B, H, W, C), True, 30)
        _lib.call("hrseg_fuse_sum", len(same_d), _lib.ptr_array(same_d), _lib.int_array([ops._ld(t) for t in same_d]), len(low_d),
                  _lib.ptr_array(low_d) if low_d else None, _lib.int_array([ops._ld(t) for t in low_d]) if low_d else None,
                  _lib.int_array([t.shape[1] for t in low_d]) if low_d else None, _lib.int_array([t.shape[2] for t in low_d]) if low_d else None,
                  out_d.data_ptr(), ops._ld(out_d), B, H, W, C, int(align), int(relu))
        torch.cuda.synchronize()
        assert out_w.unchanged(), "fuse_sum wrote outside its channel slice"
    else:
        out_d = ops.fuse_sum(same_d, low_d, relu=relu, align_corners=bool(align))
    within("fuse_sum", host(out_d), *R.fuse_sum(same, low, align, relu), name)


# =========================================================================== glue
@pytest.mark.parametrize("case,strided", _with_strided(R.GLUE_CASES, lambda c: c[0] != "second_trip"))
def test_glue(ops, case, strided):
    name, npix, C = case
    shape = (1, 7, npix // 7, C) if npix % 7 == 0 else (1, 1, npix, C)
    a, b = R.randn(shape, 1, npix, C), R.randn(shape, 2, npix, C)
    a_d, _ = operand(a, shape, strided, 1)
    b_d, _ = operand(b, shape, strided, 2)
    for relu in (False, True):
        o_d, o_w = output(shape, strided, 3)
        ops.add(a_d, b_d, relu=relu, out=o_d)
        assert np.array_equal(host(o_d), R.add(a, b, relu)) and (o_w is None or o_w.unchanged()), ("add", relu)
    o_d, o_w = output(shape, strided, 4)
    ops.copy(a_d, o_d)
    assert np.array_equal(host(o_d), a) and (o_w is None or o_w.unchanged()), "copy"
    o_d, o_w = output(shape, strided, 5, fill=b)
    ops.copy(a_d, o_d, accumulate=True)
    assert np.array_equal(host(o_d), R.copy(a, b)) and (o_w is None or o_w.unchanged()), "copy-accumulate"
    z = a.copy()
    z.reshape(-1)[::5] = 0.0
    z.reshape(-1)[1::5] = -0.0
    z_d, _ = operand(z, shape, strided, 6)
    o_d, o_w = output(shape, strided, 7)
    ops.relu_bwd(b_d, z_d, out=o_d)
    assert np.array_equal(host(o_d), R.relu_bwd(b, z)) and (o_w is None or o_w.unchanged()), "relu_bwd"
    # absmax: the maximum in the last pixel of the last block; an all-zero tensor
    m = a.copy()
    m.reshape(-1, C)[-1, C - 1] = -1234.5
    m_d, _ = operand(m, shape, strided, 8)
    assert float(ops.absmax(m_d)) == float(R.absmax(m)) == 1234.5
    assert float(ops.absmax(a_d)) == float(R.absmax(a))
    zero_d, _ = operand(np.zeros(shape, np.float32), shape, strided, 9)
    assert float(ops.absmax(zero_d)) == 0.0


@pytest.mark.parametrize("case", R.TRANSPOSE_CASES, ids=lambda c: f"C{c[1]}")
def test_transposes(ops, case):
    B, C, H, W = case
    x = R.randn((B, C, H, W), 1, C)
    assert np.array_equal(host(ops.nchw_to_nhwc(dev(x))), R.nchw_to_nhwc(x))
    assert np.array_equal(host(ops.nhwc_to_nchw(dev(R.nchw_to_nhwc(x)))), x)
    # ld > C and an offset base pointer: the two calls of concat_image_logits, the one of nhwc_slice_to_nchw
    img = R.randn((B, 3, H, W), 2, C)
    cat = ops.concat_image_logits(dev(img), dev(x))
    want = np.concatenate([R.nchw_to_nhwc(img), R.nchw_to_nhwc(x)], axis=3)
    assert np.array_equal(host(cat), want)
    assert np.array_equal(host(ops.nhwc_slice_to_nchw(cat, 3)), x)
    assert np.array_equal(host(ops.nhwc_slice_to_nchw(cat, 0)), R.nhwc_to_nchw(want))
    # a strided NHWC source through _ld (ld > C, offset a multiple of 4 floats)
    src = Wide((B, H, W, C), 3, fill=R.nchw_to_nhwc(x))
    assert np.array_equal(host(ops.nhwc_to_nchw(src.view)), x) and src.unchanged()


@pytest.mark.parametrize("case", R.COLS_CASES, ids=lambda c: c[0])
def test_weight_cols(ops, case):
    name, rows, widths = case
    w = R.randn((rows, sum(widths)), 1, rows)
    blocks = ops.weight_cols_gather(dev(w), rows, widths)
    want = R.weight_cols_gather(w, widths)
    assert len(blocks) == len(widths) and np.array_equal(np.concatenate([host(b) for b in blocks]), want)
    stage = R.randn(want.shape, 2, rows)
    dw = R.randn(w.shape, 3, rows)
    dw_d = dev(dw)
    ops.weight_cols_scatter_add(dev(stage), rows, widths, dw_d)
    assert np.array_equal(host(dw_d), R.weight_cols_scatter_add(stage, rows, widths, dw)), "scatter-add onto a non-zero dw"


@pytest.mark.parametrize("n", R.FILL_LENGTHS)
def test_fill(ops, n):
    buf = dev(R.randn(n + 8, 1, n))
    before = host(buf).copy()
    ops.fill(buf[4:4 + n], 2.5)
    now = host(buf)
    assert (now[4:4 + n] == 2.5).all() and np.array_equal(now[:4], before[:4]) and np.array_equal(now[4 + n:], before[4 + n:])
    z = ops.zeros((n,), torch.float32, buf.device)
    assert z.shape == (n,) and not host(z).any()
