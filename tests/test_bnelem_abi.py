"""Every entry point of csrc/bn.hip and csrc/elem.hip outside the head families refuses what its kernel cannot take -- by return
code and under its own name, before anything is launched (placeholder pointers, never dereferenced).  Without a device a
call that slipped past validation would come back as a launch error instead of -1: the assertion then names the missing
check.  No GPU."""
import ctypes

import pytest

P = ctypes.c_void_p(4096)        # aligned placeholder
ODD = ctypes.c_void_p(4100)      # 4-byte but not 16-byte aligned


@pytest.fixture(scope="module")
def lib():
    from hrseg_amd import _lib
    so = ctypes.CDLL(_lib.LIB_PATH)
    so.hrseg_last_error_string.restype = ctypes.c_char_p
    for name in ("hrseg_bn_fold", "hrseg_bn_fwd_group", "hrseg_bn_bwd_group", "hrseg_bn_fwd_group_phases",
                 "hrseg_bn_bwd_group_phases", "hrseg_maxpool2_fwd", "hrseg_maxpool2_bwd", "hrseg_bilinear_fwd", "hrseg_bilinear_bwd",
                 "hrseg_absmax", "hrseg_fuse_sum", "hrseg_weight_cols_gather", "hrseg_weight_cols_scatter_add", "hrseg_add",
                 "hrseg_copy", "hrseg_relu_bwd", "hrseg_nchw_to_nhwc", "hrseg_nhwc_to_nchw", "hrseg_fill"):
        getattr(so, name).argtypes = _lib.PROTOTYPES[name] if name in _lib.PROTOTYPES else None
        getattr(so, name).restype = ctypes.c_int
    return so


def refused(lib, name, rc):
    """-> the text of the refusal; `name` is the entry point whose name the message must carry"""
    who, _, text = lib.hrseg_last_error_string().decode().partition(": ")
    assert rc == -1 and who == name, (name, rc, who, text)
    return text


BAD_C = (0, 6, 1028)


def _operand_refusals(call, operands, C=8):
    """each (pointer keyword, ld keyword): ld < C, ld not a multiple of 4, a base that is not 16-byte aligned"""
    for pk, lk in operands:
        assert f"leading dimension {C - 4}" in call(**{lk: C - 4}), (pk, "ld < C")
        assert f"leading dimension {C + 2}" in call(**{lk: C + 2}), (pk, "ld % 4")
        assert "16-byte aligned" in call(**{pk: ODD}), (pk, "alignment")


def test_maxpool_refusals(lib):
    def fwd(x=P, ldx=8, y=P, ldy=8, B=2, Hi=6, Wi=5, C=8):
        return refused(lib, "hrseg_maxpool2_fwd", lib.hrseg_maxpool2_fwd(x, ldx, y, ldy, B, Hi, Wi, C, None))

    def bwd(x=P, ldx=8, dy=P, lddy=8, dx=P, lddx=8, acc=0, B=2, Hi=6, Wi=5, C=8):
        return refused(lib, "hrseg_maxpool2_bwd", lib.hrseg_maxpool2_bwd(x, ldx, dy, lddy, dx, lddx, acc, B, Hi, Wi, C, None))
    for fn, ptrs, ops in ((fwd, ("x", "y"), (("x", "ldx"), ("y", "ldy"))),
                          (bwd, ("x", "dy", "dx"), (("x", "ldx"), ("dy", "lddy"), ("dx", "lddx")))):
        for C in BAD_C:
            assert f"C={C} must be a multiple of 4" in fn(C=C, **{lk: max(C, 4) // 4 * 4 + 4 for _, lk in ops})
        for null in ptrs:
            assert "bad arguments" in fn(**{null: None}), null
        for bad in (dict(B=0), dict(B=-1), dict(Hi=1), dict(Wi=1), dict(Hi=0), dict(Wi=-2)):
            assert "bad arguments" in fn(**bad), bad
        _operand_refusals(fn, ops)


def test_bilinear_refusals(lib):
    def fwd(src=P, ldin=8, B=2, Hi=4, Wi=5, C=8, out=P, ldout=8, Hout=12, Wout=11, Hr=8, Wr=9, py=2, px=1, align=1, acc=0, relu=0):
        return refused(lib, "hrseg_bilinear_fwd", lib.hrseg_bilinear_fwd(src, ldin, B, Hi, Wi, C, out, ldout, Hout, Wout, Hr, Wr, py,
                                                                         px, align, acc, relu, None))

    def bwd(dout=P, lddout=8, B=2, Hi=4, Wi=5, C=8, din=P, lddin=8, Hout=12, Wout=11, Hr=8, Wr=9, py=2, px=1, align=1, acc=0):
        return refused(lib, "hrseg_bilinear_bwd", lib.hrseg_bilinear_bwd(dout, lddout, B, Hi, Wi, C, din, lddin, Hout, Wout, Hr, Wr,
                                                                         py, px, align, acc, None))
    for fn, ptrs, ops, geometry in ((fwd, ("src", "out"), (("src", "ldin"), ("out", "ldout")), "does not fit"),
                                    (bwd, ("dout", "din"), (("dout", "lddout"), ("din", "lddin")), "bad geometry")):
        for C in BAD_C:
            assert f"C={C} must be a multiple of 4" in fn(C=C)
        for null in ptrs:
            assert geometry in fn(**{null: None}), null
        for bad in (dict(B=0), dict(Hi=0), dict(Wi=0), dict(Hr=0), dict(Wr=-1), dict(py=-1), dict(px=-1),
                    dict(py=5), dict(px=3), dict(Hr=11), dict(Wr=11), dict(Hout=9), dict(Wout=9)):      # a placed image that does not fit
            assert geometry in fn(**bad), bad
        _operand_refusals(fn, ops)


def _fuse(lib, n_same=2, same=(P, P, P, P), ld_same=(8, 8, 8, 8), n_low=2, low=(P, P, P), ld_low=(8, 8, 8), Hi=(3, 2, 1), Wi=(4, 2, 1),
          out=P, ldo=8, B=2, H=6, W=7, C=8, null=()):
    arr = lambda xs, t: (t * len(xs))(*xs)       # noqa: E731
    vp = lambda xs: (ctypes.c_void_p * len(xs))(*[x.value if isinstance(x, ctypes.c_void_p) else x for x in xs])      # noqa: E731
    args = dict(same=vp(same), ld_same=arr(ld_same, ctypes.c_int), low=vp(low), ld_low=arr(ld_low, ctypes.c_int),
                Hi=arr(Hi, ctypes.c_int), Wi=arr(Wi, ctypes.c_int))
    for k in null:
        args[k] = None
    rc = lib.hrseg_fuse_sum(n_same, args["same"], args["ld_same"], n_low, args["low"], args["ld_low"], args["Hi"], args["Wi"], out, ldo,
                            B, H, W, C, 1, 1, None)
    return refused(lib, "hrseg_fuse_sum", rc)


def test_fuse_sum_refusals(lib):
    for C in BAD_C:
        assert f"C={C} must be a multiple of 4" in _fuse(lib, C=C)
    for bad in (dict(n_same=0), dict(n_same=5), dict(n_low=4), dict(n_low=-1), dict(out=None), dict(B=0), dict(H=0), dict(W=0),
                dict(null=("same",)), dict(null=("ld_same",))):
        assert "1..4 same-resolution terms" in _fuse(lib, **bad), bad
    for k in ("low", "ld_low", "Hi", "Wi"):
        assert "need their geometry" in _fuse(lib, null=(k,)), k
    assert "bad same-resolution term 1" in _fuse(lib, same=(P, None, P, P))
    assert "bad same-resolution term 0" in _fuse(lib, ld_same=(4, 8, 8, 8))
    assert "bad same-resolution term 1" in _fuse(lib, ld_same=(8, 10, 8, 8))
    assert "bad same-resolution term 1" in _fuse(lib, same=(P, ODD, P, P))
    assert "bad low-resolution term 1" in _fuse(lib, low=(P, None, P))
    assert "bad low-resolution term 0" in _fuse(lib, ld_low=(4, 8, 8))
    assert "bad low-resolution term 1" in _fuse(lib, ld_low=(8, 10, 8))
    assert "bad low-resolution term 0" in _fuse(lib, low=(ODD, P, P))
    assert "bad low-resolution term 1" in _fuse(lib, Hi=(3, 0, 1))
    assert "bad low-resolution term 0" in _fuse(lib, Wi=(-1, 2, 1))
    assert "leading dimension 4 of out" in _fuse(lib, ldo=4)
    assert "leading dimension 10 of out" in _fuse(lib, ldo=10)
    assert "out must be 16-byte aligned" in _fuse(lib, out=ODD)


def test_glue_refusals(lib):
    def add(a=P, lda=8, b=P, ldb=8, out=P, ldo=8, relu=0, npix=10, C=8):
        return refused(lib, "hrseg_add", lib.hrseg_add(a, lda, b, ldb, out, ldo, relu, npix, C, None))

    def copy(src=P, ldin=8, out=P, ldout=8, acc=0, npix=10, C=8):
        return refused(lib, "hrseg_copy", lib.hrseg_copy(src, ldin, out, ldout, acc, npix, C, None))

    def relu_bwd(dz=P, lddz=8, z=P, ldz=8, dx=P, lddx=8, npix=10, C=8):
        return refused(lib, "hrseg_relu_bwd", lib.hrseg_relu_bwd(dz, lddz, z, ldz, dx, lddx, npix, C, None))

    def absmax(x=P, ldx=8, npix=10, C=8, out=P):
        return refused(lib, "hrseg_absmax", lib.hrseg_absmax(x, ldx, npix, C, out, None))
    for fn, ptrs, ops in ((add, ("a", "b", "out"), (("a", "lda"), ("b", "ldb"), ("out", "ldo"))),
                          (copy, ("src", "out"), (("src", "ldin"), ("out", "ldout"))),
                          (relu_bwd, ("dz", "z", "dx"), (("dz", "lddz"), ("z", "ldz"), ("dx", "lddx"))),
                          (absmax, ("x", "out"), (("x", "ldx"),))):
        for C in BAD_C:
            assert f"C={C} must be a multiple of 4" in fn(C=C)
        for null in ptrs:
            assert "bad arguments" in fn(**{null: None}), (fn.__name__, null)
        for npix in (0, -5):
            assert "bad arguments" in fn(npix=npix), (fn.__name__, npix)
        _operand_refusals(fn, ops)


def test_transpose_refusals(lib):
    def to_nhwc(src=P, out=P, ldout=7, B=2, C=3, H=4, W=5):
        return refused(lib, "hrseg_nchw_to_nhwc", lib.hrseg_nchw_to_nhwc(src, out, ldout, B, C, H, W, None))

    def to_nchw(src=P, ldin=7, out=P, B=2, C=3, H=4, W=5):
        return refused(lib, "hrseg_nhwc_to_nchw", lib.hrseg_nhwc_to_nchw(src, ldin, out, B, C, H, W, None))
    for fn, ld in ((to_nhwc, "ldout"), (to_nchw, "ldin")):
        for bad in (dict(src=None), dict(out=None), dict(B=0), dict(C=0), dict(C=-1), dict(H=0), dict(H=-4), dict(W=0), dict(W=-5),
                    {ld: 2}):      # ld must be >= C
            assert "bad arguments" in fn(**bad), (fn.__name__, bad)


def test_weight_cols_and_fill_refusals(lib):
    for name in ("hrseg_weight_cols_gather", "hrseg_weight_cols_scatter_add"):
        def call(src=P, rows=5, Cin=16, n=3, widths=(4, 8, 4), dst=P, null_widths=False):
            w = None if null_widths else (ctypes.c_int * len(widths))(*widths)
            return refused(lib, name, getattr(lib, name)(src, rows, Cin, n, w, dst, None))
        for bad in (dict(src=None), dict(dst=None), dict(rows=0), dict(Cin=0), dict(Cin=6, widths=(4, 2)), dict(n=0),
                    dict(n=9, widths=(4,) * 9, Cin=36), dict(null_widths=True), dict(src=ODD), dict(dst=ODD)):      # 9 column blocks
            assert "bad arguments" in call(**bad), (name, bad)
        assert "block width 6 must be a positive multiple of 4" in call(widths=(4, 6, 6))
        assert "block width 0 must be a positive multiple of 4" in call(widths=(4, 0, 12))
        assert "block widths sum to 12" in call(widths=(4, 4, 4))
        assert "block widths sum to 20" in call(widths=(4, 12, 4))
    lib.hrseg_fill.argtypes = [ctypes.c_void_p, ctypes.c_float, ctypes.c_long, ctypes.c_void_p]
    assert "bad arguments" in refused(lib, "hrseg_fill", lib.hrseg_fill(None, 0.0, 4, None))
    assert "bad arguments" in refused(lib, "hrseg_fill", lib.hrseg_fill(P, 0.0, -1, None))


def test_bn_fold_refusals(lib):
    def fold(w=P, bias=P, gamma=P, beta=P, rm=P, rv=P, eps=1e-5, Cout=4, row=27, w_out=P, b_out=P):
        return refused(lib, "hrseg_bn_fold", lib.hrseg_bn_fold(w, bias, gamma, beta, rm, rv, eps, Cout, row, w_out, b_out, None))
    for bad in (dict(w=None), dict(rm=None), dict(rv=None), dict(w_out=None), dict(b_out=None), dict(Cout=0), dict(row=0), dict(row=-3)):
        assert "bad arguments" in fold(**bad), bad


def _fwd_problem(_lib, **kw):
    f = dict(y=P, ldy=8, npix=100, C=8, gamma=P, beta=P, running_mean=P, running_var=P, num_batches_tracked=P, momentum=0.1, eps=1e-5,
             residual=None, ldr=0, relu=1, z=P, ldz=8, coef=P, partial=P, nchunks=4)
    f.update(kw)
    arr = (_lib.BnFwd * 8)()
    for a in arr:
        for k, v in f.items():
            setattr(a, k, v.value if isinstance(v, ctypes.c_void_p) else v)
    return arr


def _bwd_problem(_lib, **kw):
    f = dict(dz=P, lddz=8, z=P, ldz=8, relu=1, y=P, ldy=8, coef=P, dgamma=P, dbeta=P, dy=P, lddy=8, dres=P, lddres=8, dres_accumulate=0,
             npix=100, C=8, partial=P, nchunks=4, nseg=1)
    f.update(kw)
    arr = (_lib.BnBwd * 8)()
    for a in arr:
        for k, v in f.items():
            setattr(a, k, v.value if isinstance(v, ctypes.c_void_p) else v)
    return arr


def test_bn_group_refusals(lib):
    from hrseg_amd import _lib

    def fwd(n=2, training=1, phases=None, **kw):
        arr = _fwd_problem(_lib, **kw)
        rc = lib.hrseg_bn_fwd_group(n, arr, training, None) if phases is None else lib.hrseg_bn_fwd_group_phases(n, arr, training, phases, None)
        who, _, text = lib.hrseg_last_error_string().decode().partition(": ")
        assert rc == -1 and who in ("hrseg_bn_fwd_group", "hrseg_bn_fwd_group_phases"), (rc, who, text)
        return text

    def bwd(n=2, eval_mode=0, phases=None, **kw):
        arr = _bwd_problem(_lib, **kw)
        rc = lib.hrseg_bn_bwd_group(n, arr, eval_mode, None) if phases is None else lib.hrseg_bn_bwd_group_phases(n, arr, eval_mode, phases, None)
        who, _, text = lib.hrseg_last_error_string().decode().partition(": ")
        assert rc == -1 and who in ("hrseg_bn_bwd_group", "hrseg_bn_bwd_group_phases"), (rc, who, text)
        return text
    for fn in (fwd, bwd):
        for n in (0, 9, -1):
            assert "n must be 1..8" in fn(n=n), (fn.__name__, n)
        for phases in (0, 8):
            assert "phases is a mask of bits 0..2" in fn(phases=phases), (fn.__name__, phases)
        for C in BAD_C:
            assert f"C={C} must be a multiple of 4" in fn(C=C), (fn.__name__, C)
    # forward: what each phase needs
    for bad in (dict(coef=None), dict(coef=ODD)):
        assert "(coef)" in fwd(**bad), bad
    for bad in (dict(y=None), dict(ldy=4), dict(ldy=10), dict(y=ODD)):
        assert "(y, ldy)" in fwd(**bad), bad
    assert "(npix)" in fwd(npix=0)
    for bad in (dict(z=None), dict(ldz=4), dict(ldz=10), dict(z=ODD)):
        assert "the apply phase needs z, ldz" in fwd(**bad), bad
    for bad in (dict(partial=None), dict(nchunks=0)):
        assert "training needs partial/nchunks" in fwd(**bad), bad
    for bad in (dict(running_mean=None), dict(running_var=None)):
        assert "eval needs running stats" in fwd(training=0, **bad), bad
    assert "leading dimension 4 of residual" in fwd(residual=P, ldr=4)
    assert "leading dimension 10 of residual" in fwd(residual=P, ldr=10)
    assert "residual must be 16-byte aligned" in fwd(residual=ODD, ldr=8)
    # backward
    for null in ("dz", "y", "coef", "dy", "partial"):
        assert "bad arguments" in bwd(**{null: None}), null
    for bad in (dict(npix=0), dict(nchunks=0)):
        assert "bad arguments" in bwd(**bad), bad
    assert "nseg=3 must divide nchunks=4 and npix" in bwd(nseg=3)               # nchunks does not divide
    assert "nseg=2 must divide nchunks=4 and npix" in bwd(nseg=2, npix=101)     # npix does not divide
    _operand_refusals(bwd, (("dz", "lddz"), ("y", "ldy"), ("dy", "lddy"), ("z", "ldz"), ("dres", "lddres")))
    assert "coef must be 16-byte aligned" in bwd(coef=ODD)
    # (z is read only under relu, dres only when given: their strides are not looked at otherwise -- nothing to refuse)
