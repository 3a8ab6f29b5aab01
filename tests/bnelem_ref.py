"""float64 references, case lists, input builders and error bounds for the BatchNorm, pooling, resize and glue kernels
(csrc/bn.hip, csrc/elem.hip; tests/test_bnelem_cpu.py pins this module, tests/test_bnelem_gpu.py holds the kernels to it).

Every reference restates what include/hrseg.h and the kernel comments promise, on NHWC numpy arrays, in float64.

ERROR MODEL.  u = 2^-24 is the unit roundoff of fp32.  A result that is an n-term fp32 sum of products may differ from the
float64 value by at most (n + c) * u * A, where A = sum |w_k| |v_k| comes from the SAME float64 code run on absolute values,
n is the longest chain of fp32 additions the kernel's documented order allows and c (<= 8) counts the remaining roundings;
each c has its derivation next to it.  An error that enters through an input with a bound of its own (the batch mean inside
`shift`) is propagated to first order and multiplied by SECOND = 1.25 for the second-order terms; where first order does not
hold (a variance bound that is not small against var + eps) the exact interval of rstd is the bound, and z is bounded end to
end in the centred form (bn_end_to_end), in which the errors of scale and shift cancel as they do on the device.  Operations
that are exact in fp32 have an fp32 restatement and are compared for equality.

Imports numpy only."""
import numpy as np

U = 2.0 ** -24
SECOND = 1.25
C_MAX = 8                    # no constant c below exceeds it (asserted by the CPU test through CONSTANTS)
CONSTANTS = {}               # name -> c, filled next to each derivation


def _c(name, value):
    CONSTANTS[name] = value
    return value


# =========================================================================== host rules, restated once
GRID_CAP = 4096              # csrc/elem_common.h elem_grid
BN_MAX_CHUNKS = 256          # ops._BN_MAX_CHUNKS (its default)
BN_MAXG = 8                  # csrc/bn.hip
CHANNEL_MAPPINGS = (4, 12, 48, 720, 1024)


def lanes(C):
    """csrc/elem_common.h make_lanes: -> (Q channel quads, P pixel lanes per block, idle threads of the 256)"""
    Q = C // 4
    P = 1 if Q >= 256 else 256 // Q
    return Q, P, 256 - Q * P


def elem_grid(npix, C):
    _, P, _ = lanes(C)
    return max(1, min(GRID_CAP, (npix + P - 1) // P))


def grid_trips(npix, C):
    """trips of the grid-stride loop of the block that makes the most"""
    _, P, _ = lanes(C)
    per_trip = elem_grid(npix, C) * P
    return (npix + per_trip - 1) // per_trip


def nchunks_rule(npix, C):
    """ops._nchunks"""
    _, P, _ = lanes(C)
    return max(1, min(BN_MAX_CHUNKS, npix // (8 * P)))


def chunk_range(npix, nchunks, chunk):
    """csrc/bn.hip stats_body with nseg = 1: pixels [lo, hi) of a chunk (empty when lo >= hi)"""
    per = (npix + nchunks - 1) // nchunks
    lo = chunk * per
    return lo, max(lo, min(lo + per, npix))


def stats_chain(npix, C, nchunks):
    """pixels one thread of stats_body walks at most: the longest fp32 chain of the statistics; beyond a thread sums are fp64"""
    _, P, _ = lanes(C)
    per = (npix + nchunks - 1) // nchunks
    return max(1, (per + P - 1) // P)


def stats_paths(npix, C, nchunks):
    """which paths of stats_body / reduce_chunks16 a (npix, C, nchunks) reaches"""
    _, P, _ = lanes(C)
    out = set()
    for k in range(nchunks):
        lo, hi = chunk_range(npix, nchunks, k)
        if hi <= lo:
            out.add("empty_chunk")
            continue
        for pl in range(min(P, hi - lo)):
            for pix0 in range(lo + pl, hi, 4 * P):
                out.add("ragged_trip" if pix0 + 3 * P >= hi else "full_trip")
    for lane in range(16):                      # reduce_chunks16: 16 chunk lanes per channel
        k = lane
        if k >= nchunks:
            out.add("idle_lane")
        while k + 48 < nchunks:
            out.add("batched")
            k += 64
        if k < nchunks:
            out.add("tail")
    return out


def bilinear_bwd_rs(B, Hi, Wi, C, Hr):
    """the row-split instance hrseg_bilinear_bwd launches (csrc/elem.hip)"""
    Q, npix = C // 4, B * Hi * Wi
    foot = int(2.0 * (Hr - 1) / (Hi - 1)) + 3 if (Hi > 1 and Hr > 1) else Hr
    rs = 1
    while rs < 8 and Q * rs * 2 <= 256 and rs * 2 <= foot // 2 and npix // max(1, 256 // (Q * rs)) < 1024:
        rs *= 2
    return rs


def bilinear_bwd_trips(B, Hi, Wi, C, Hr):
    Q, npix = C // 4, B * Hi * Wi
    P2 = max(1, 256 // (Q * bilinear_bwd_rs(B, Hi, Wi, C, Hr)))
    blocks = min(GRID_CAP, (npix + P2 - 1) // P2)
    return (npix + blocks * P2 - 1) // (blocks * P2)


# =========================================================================== BatchNorm
def f32(x):
    """the float64 value of x rounded to fp32 (scalars the ABI takes as float: eps, momentum)"""
    return np.float64(np.float32(x))


def bn_forward(y, gamma, beta, rm, rv, nbt, momentum, eps, nchunks, repeat=1, stat_div=1, drop=None):
    """Training statistics of y [npix, C] (fp32 values) -> dict name -> (value, bound) in float64:
    coef [4, C] (mean, rstd, scale, shift), running_mean, running_var [C] or None, nbt (exact), and the intermediate
    `var`.  gamma / beta / rm / rv may be None (gamma 1, beta 0; no running statistics).
    drop (test only): [C] pixel indices, one per channel, that a wrong kernel would lose from both sums."""
    y = np.asarray(y, dtype=np.float64)
    npix, C = y.shape
    ga = np.ones(C) if gamma is None else np.asarray(gamma, np.float64)
    be = np.zeros(C) if beta is None else np.asarray(beta, np.float64)
    m, eps = f32(momentum), f32(eps)
    if drop is None:
        mean = y.mean(0)
        var = ((y - mean) ** 2).mean(0)                      # biased, two-pass: the float64 truth of E[x^2] - mean^2
    else:
        lost = y[drop, np.arange(C)]
        mean = (y.sum(0) - lost) / npix
        var = np.maximum(((y ** 2).sum(0) - lost ** 2) / npix - mean ** 2, 0.0)
    e_abs, e_sq = np.abs(y).mean(0), (y ** 2).mean(0)
    n = stats_chain(npix, C, nchunks)
    # A thread adds n values starting from an exact first one: (n - 1) u E|x| on the mean, and n u E[x^2] on the second moment
    # (one more rounding for x * x).  |d var| <= |d E[x^2]| + 2 |mean| |d mean| <= n u E[x^2] + 2 (n - 1) u |mean| E|x|, and
    # |mean| E|x| <= E[x^2]: together the issue's 3 n u E[x^2].  Lane and chunk sums and the finalize arithmetic are fp64.
    # s_*: what the fp64 statistics of the device may be off by (before any cast); b_*: the bound of an fp32 coef row.
    s_mean = (n - 1) * U * e_abs
    b_mean = s_mean + _c("mean: the cast to fp32", 1) * U * e_abs                      # together n u E|x|
    b_var = 3 * n * U * e_sq
    rstd = 1.0 / np.sqrt(var + eps)
    # rstd of a variance in [max(var - b_var, 0), var + b_var] (the kernel clamps at 0) lies in [rstd_lo, rstd_hi] exactly.
    # First order times SECOND holds while b_var is small against var + eps ((1 - x)^-1/2 - 1 <= 0.625 x up to x = 0.25; used
    # up to 0.1); beyond that (ill-conditioned channels, a constant channel with var = 0) the interval itself is the bound.
    rstd_lo, rstd_hi = 1.0 / np.sqrt(var + eps + b_var), 1.0 / np.sqrt(np.maximum(var - b_var, 0.0) + eps)
    s_rstd = np.where(b_var <= 0.1 * (var + eps), SECOND * 0.5 * rstd ** 3 * b_var, np.maximum(rstd_hi - rstd, rstd - rstd_lo))
    b_rstd = s_rstd + _c("rstd: the cast to fp32", 1) * U * rstd_hi                    # (rstd_hi: the largest magnitude it may have)
    scale = ga * rstd
    b_scale = np.abs(ga) * b_rstd + _c("scale: one product", 1) * U * np.abs(ga) * rstd_hi
    shift = be - mean * ga * rstd
    b_shift = SECOND * (np.abs(ga * rstd) * b_mean + np.abs(mean * ga) * b_rstd) + \
        _c("shift: two products and the subtraction", 3) * U * (np.abs(be) + np.abs(mean * ga) * rstd_hi)
    out = {"coef": (np.stack([mean, rstd, scale, shift]), np.stack([b_mean, b_rstd, b_scale, b_shift])), "var": (var, b_var),
           # the fp32 rstd row, one-sided where the variance can only move one way: (lowest, highest) value it may hold
           "rstd_interval": (rstd_lo * (1.0 - U), rstd_hi * (1.0 + U)),
           "stat": dict(mean=mean, s_mean=s_mean, s_scale=np.abs(ga) * s_rstd, scale_mag=np.abs(ga) * rstd_hi, beta=be)}
    reps = max(1, int(repeat))

    def running(old, new, b_new):
        # reps sequential updates v = (1 - m) v + m new in fp32: per update the rounding of 1 - m, two products and one
        # addition touch each term at most three times (n = 3 reps); c: the cast of `new` to fp32 and a spare for fp64 -> fp32
        # of the unbiased factor
        v, a = np.asarray(old, np.float64).copy(), np.abs(np.asarray(old, np.float64))
        for _ in range(reps):
            v, a = (1.0 - m) * v + m * new, (1.0 - m) * a + m * np.abs(new)
        return v, (1.0 - (1.0 - m) ** reps) * b_new + (3 * reps + _c("running statistics: casts", 2)) * U * a
    out["running_mean"] = None if rm is None else running(rm, mean, b_mean)
    if rv is None:
        out["running_var"] = None
    else:
        n1 = npix // max(1, int(stat_div))
        f = n1 / (n1 - 1.0) if n1 > 1 else 1.0
        out["running_var"] = running(rv, var * f, b_var * f)
    out["nbt"] = None if nbt is None else int(nbt) + reps
    return out


def bn_eval_coef(gamma, beta, rm, rv, eps):
    """coef [4, C] of the running statistics (eval mode, fp32 arithmetic throughout) -> (value, bound)"""
    rm, rv = np.asarray(rm, np.float64), np.asarray(rv, np.float64)
    ga = np.ones(rm.shape) if gamma is None else np.asarray(gamma, np.float64)
    be = np.zeros(rm.shape) if beta is None else np.asarray(beta, np.float64)
    rstd = 1.0 / np.sqrt(rv + f32(eps))
    b_rstd = _c("eval rstd: var + eps, sqrt, division", 3) * U * rstd
    scale, shift = ga * rstd, be - rm * ga * rstd
    b_scale = np.abs(ga) * b_rstd + U * np.abs(scale)
    b_shift = SECOND * np.abs(rm * ga) * b_rstd + 3 * U * (np.abs(be) + np.abs(rm * ga * rstd))      # (c as for the training shift)
    return np.stack([rm, rstd, scale, shift]), np.stack([np.zeros(rm.shape), b_rstd, b_scale, b_shift])


def bn_apply(y, coef, residual=None, relu=False):
    """z = relu?(y * scale + shift (+ residual)) on coef [4, C] as given (the device's, widened) -> (z, bound, pre-activation)"""
    y, coef = np.asarray(y, np.float64), np.asarray(coef, np.float64)
    v, a = y * coef[2] + coef[3], np.abs(y * coef[2]) + np.abs(coef[3])
    n = 2
    if residual is not None:
        r = np.asarray(residual, np.float64)
        v, a, n = v + r, a + np.abs(r), 3
    # n terms; c: the product (one rounding where the compiler does not fuse it).  |relu(a) - relu(b)| <= |a - b|.
    bound = (n + _c("apply: the product", 1)) * U * a
    return (np.maximum(v, 0.0) if relu else v), bound, v


def bn_rows_from_rows(coef, gamma, beta):
    """the scale and shift rows of coef [4, C] (the device's, widened) from ITS mean and rstd rows -> (value, bound) [2, C].
    However far an ill-conditioned variance moves rstd, scale and shift must follow it: scale = gamma * rstd is one product,
    shift = beta - mean * gamma * rstd two products and a subtraction of fp32 values."""
    coef = np.asarray(coef, np.float64)
    ga = np.ones(coef.shape[1]) if gamma is None else np.asarray(gamma, np.float64)
    be = np.zeros(coef.shape[1]) if beta is None else np.asarray(beta, np.float64)
    scale, prod = ga * coef[1], coef[0] * ga * coef[1]
    return np.stack([scale, be - prod]), np.stack([CONSTANTS["scale: one product"] * U * np.abs(scale),
                                                   CONSTANTS["shift: two products and the subtraction"] * U * (np.abs(be) + np.abs(prod))])


def bn_end_to_end(y, f, residual=None, relu=False):
    """z of the device against z of the float64 statistics f = bn_forward(y, ...) -> (z, bound).  The errors of the scale and
    shift rows are not independent: with the device's fp64 statistics m*, r* and s* = gamma r*, t* = beta - m* s*,
        (y s* + t*) - (y s + t) = (y - m)(s* - s) - (m* - m) s*          (an identity, nothing dropped),
    so the statistics enter as |y - mean| d_scale + |s*| d_mean: a constant channel (y = mean) keeps only the second term and
    stays near beta however far its rstd moves.  The roundings on the way to the fp32 z come on top, on the magnitudes."""
    y = np.asarray(y, np.float64)
    st, coef = f["stat"], f["coef"][0]
    z, _, _ = bn_apply(y, coef, residual, relu)
    S, M = st["scale_mag"], np.abs(st["mean"]) + st["s_mean"]
    T = np.abs(st["beta"]) + M * S
    b_stat = np.abs(y - st["mean"]) * st["s_scale"] + S * st["s_mean"]
    n, a = 2, np.abs(y) * S + T
    if residual is not None:
        n, a = 3, a + np.abs(np.asarray(residual, np.float64))
    b_round = _c("z: scale row, the cast of rstd and the product", 2) * U * np.abs(y) * S + \
        _c("z: shift row, the casts of mean and rstd, two products, the subtraction", 5) * U * T + \
        (n + CONSTANTS["apply: the product"]) * U * a
    return z, b_stat + b_round


def bn_backward(dz, y, coef, mask, nchunks, eval_mode=False, dgamma=None, dbeta=None, dres=None, dres_accumulate=False, drop=None):
    """Backward of z = relu?(bn(y) + residual) on [npix, C] arrays, coef [4, C] as the device left it (widened): this bounds
    the backward's arithmetic alone.  mask: [npix, C] bool (who passed the ReLU) or None.
    -> dict: dy, dgamma, dbeta as (value, bound) (dgamma / dbeta: old + sum, None when not given), dres as an fp32 array that
    must be matched exactly (None when not given).  drop (test only): [C] pixel indices, one per channel, lost from the sums."""
    dz, y, coef = np.asarray(dz, np.float64), np.asarray(y, np.float64), np.asarray(coef, np.float64)
    npix, C = y.shape
    mean, rstd, scale = coef[0], coef[1], coef[2]
    g = dz if mask is None else np.where(mask, dz, 0.0)
    xh = (y - mean) * rstd
    s, sx = g.sum(0), (g * xh).sum(0)
    if drop is not None:
        s, sx = s - g[drop, np.arange(C)], sx - (g * xh)[drop, np.arange(C)]
    a_s, a_sx = np.abs(g).sum(0), np.abs(g * xh).sum(0)
    n = stats_chain(npix, C, nchunks)
    # sums: a thread adds n terms in fp32; g * xhat carries three roundings (y - mean, * rstd, * g) before it is added
    b_s = (n - 1) * U * a_s
    b_sx = (n + _c("sum g*xhat: xhat's two roundings and the product", 3) - 1) * U * a_sx
    out = {}
    for name, old, tot, b_tot, a_tot in (("dgamma", dgamma, sx, b_sx, a_sx), ("dbeta", dbeta, s, b_s, a_s)):
        if old is None:
            out[name] = None
            continue
        old = np.asarray(old, np.float64)
        # += (float)total: the cast and the addition
        out[name] = (old + tot, b_tot + _c("dgamma/dbeta: cast and +=", 2) * U * (a_tot + np.abs(old)))
    if eval_mode:
        # inv = 0: dy = scale * (g - 0 - xhat * 0) = scale * g, one product
        out["dy"] = (scale * g, _c("dy (eval): one product", 1) * U * np.abs(scale * g))
    else:
        mg, mgx = s / npix, sx / npix
        # (float)total * (float)(1 / npix): c = 3 for the two casts and the product
        b_mg = b_s / npix + _c("mean of g: two casts and a product", 3) * U * a_s / npix
        b_mgx = b_sx / npix + 3 * U * a_sx / npix
        dy = scale * (g - mg - xh * mgx)
        a_dy = np.abs(g) + np.abs(mg) + np.abs(xh * mgx)
        # xhat * mgx: three roundings (y - mean, * rstd, * mgx); two subtractions; the product with scale
        b_dy = np.abs(scale) * (SECOND * (b_mg + np.abs(xh) * b_mgx) + _c("dy: xhat*mgx 3, subtractions 2, * scale 1", 6) * U * a_dy)
        out["dy"] = (dy, b_dy)
    if dres is None:
        out["dres"] = None
    else:
        g32 = g.astype(np.float32)              # (g is dz or 0: exact)
        out["dres"] = (np.asarray(dres, np.float32) + g32) if dres_accumulate else g32
    return out


def bn_fold(w, bias, gamma, beta, rm, rv, eps):
    """hrseg_bn_fold on w [Cout, row]: -> (w_out, bound), (b_out, bound).  Four fp32 roundings reach a folded weight (var + eps,
    sqrt, the division, the product): 2 ulp; the issue's bound is 4 ulp = 8 u relative, on the magnitudes for the bias."""
    w = np.asarray(w, np.float64)
    Cout = w.shape[0]
    ga = np.ones(Cout) if gamma is None else np.asarray(gamma, np.float64)
    be = np.zeros(Cout) if beta is None else np.asarray(beta, np.float64)
    bi = np.zeros(Cout) if bias is None else np.asarray(bias, np.float64)
    s = ga / np.sqrt(np.asarray(rv, np.float64) + f32(eps))
    ulp4 = _c("fold: 4 ulp", 8) * U
    w_out = w * s[:, None]
    b_out = (bi - np.asarray(rm, np.float64)) * s + be
    return (w_out, ulp4 * np.abs(w_out)), (b_out, ulp4 * ((np.abs(bi) + np.abs(rm)) * np.abs(s) + np.abs(be)))


# =========================================================================== max pool 2x2 (floor)
def maxpool2_fwd(x):
    """x [B, H, W, C] fp32 -> [B, H//2, W//2, C] fp32, exact"""
    x = np.asarray(x, np.float32)
    B, H, W, C = x.shape
    Ho, Wo = H // 2, W // 2
    v = x[:, :2 * Ho, :2 * Wo].reshape(B, Ho, 2, Wo, 2, C)
    return v.max(axis=(2, 4))


def maxpool2_bwd(x, dy, dx_old=None, last=False):
    """the gradient goes to the FIRST maximum in scan order (strict >); the odd leftover row / column gets zero; dx_old: += in
    fp32.  last (test only): a wrong kernel that prefers the last maximum."""
    x, dy = np.asarray(x, np.float32), np.asarray(dy, np.float32)
    B, H, W, C = x.shape
    Ho, Wo = H // 2, W // 2
    v = x[:, :2 * Ho, :2 * Wo].reshape(B, Ho, 2, Wo, 2, C).transpose(0, 1, 3, 5, 2, 4).reshape(B, Ho, Wo, C, 4)      # k = 2*dy + dx
    arg = (3 - np.argmax(v[..., ::-1], axis=-1)) if last else np.argmax(v, axis=-1)      # argmax: first occurrence
    dx = np.zeros((B, H, W, C), np.float32)
    for k in range(4):
        dx[:, (k >> 1):2 * Ho:2, (k & 1):2 * Wo:2] = np.where(arg == k, dy, np.float32(0))
    return dx if dx_old is None else np.asarray(dx_old, np.float32) + dx


# =========================================================================== bilinear
def resize_scale(in_size, out_size, align, dtype=np.float32):
    if align:
        return dtype(in_size - 1) / dtype(out_size - 1) if out_size > 1 else dtype(0)
    return dtype(in_size) / dtype(out_size)


def bilinear_matrix(in_size, out_size, align, dtype=np.float32):
    """[out_size, in_size] interpolation weights of one axis.  dtype float32: source index and the two weights in fp32 exactly
    as torch's upsample_bilinear2d and csrc/elem.hip src_index compute them (a float64 coordinate would differ from the kernel
    by O(size * 2^-24) in the weight); float64: the same formula in float64, which is what torch's float64 op evaluates."""
    f = dtype
    scale = resize_scale(in_size, out_size, align, f)
    o = np.arange(out_size).astype(f)
    if align:
        r = scale * o
    else:
        # scale * (o + 0.5) - 0.5 is ONE fused multiply-add in the compiled kernels (the compiler contracts it, as it does in
        # torch's own kernels): the product is not rounded.  A float64 product of two fp32 values is exact, so rounding the
        # float64 expression once is that instruction.  (An unfused product would move the weight by up to size * u.)
        r = np.maximum((np.float64(scale) * (o + f(0.5)).astype(np.float64) - 0.5).astype(f), f(0))
    assert r.dtype == f
    i0 = np.minimum(r.astype(np.int64), in_size - 1)
    i1 = i0 + (i0 < in_size - 1)
    l1 = r - i0.astype(f)
    l0 = f(1) - l1
    m = np.zeros((out_size, in_size), f)
    np.add.at(m, (np.arange(out_size), i0), l0)
    np.add.at(m, (np.arange(out_size), i1), l1)
    return m


def _resize(x64, my, mx):
    return np.einsum("oi,bijc,xj->boxc", my, x64, mx, optimize=True)


def bilinear_fwd(x, Hr, Wr, align, Hout=None, Wout=None, py=0, px=0, out_old=None, relu=False, dtype=np.float32):
    """resize x [B, Hi, Wi, C] to Hr x Wr and place it at (py, px) of a Hout x Wout image (zero outside; out_old: += on the
    whole image); relu after the add -> (value, bound)"""
    x = np.asarray(x, np.float64)
    B, Hi, Wi, C = x.shape
    Hout, Wout = Hout or Hr, Wout or Wr
    my, mx = bilinear_matrix(Hi, Hr, align, dtype).astype(np.float64), bilinear_matrix(Wi, Wr, align, dtype).astype(np.float64)
    v, a = np.zeros((B, Hout, Wout, C)), np.zeros((B, Hout, Wout, C))
    v[:, py:py + Hr, px:px + Wr] = _resize(x, my, mx)
    a[:, py:py + Hr, px:px + Wr] = _resize(np.abs(x), my, mx)
    n = 4                                                          # four taps
    if out_old is not None:
        old = np.asarray(out_old, np.float64)
        v, a, n = v + old, a + np.abs(old), 5
    # each tap: lx * v, the inner addition, * ly, the outer addition: the additions are the n, c the two products
    bound = (n + _c("bilinear: the two weight products of a tap", 2)) * U * a
    return (np.maximum(v, 0.0) if relu else v), bound


def bilinear_footprint(Hi, Wi, Hr, Wr, align):
    """most output pixels with weight on one input pixel: the longest chain of bilinear_bwd (one thread, RS = 1)"""
    my, mx = bilinear_matrix(Hi, Hr, align), bilinear_matrix(Wi, Wr, align)
    return int((my != 0).sum(0).max()) * int((mx != 0).sum(0).max())


def bilinear_bwd(dout, Hi, Wi, Hr, Wr, align, py=0, px=0, din_old=None, dtype=np.float32):
    """the transpose: din[iy, ix] (+)= sum over the placed Hr x Wr window of dout of (wy * wx) * dout -> (value, bound)"""
    g = np.asarray(dout, np.float64)[:, py:py + Hr, px:px + Wr]
    my, mx = bilinear_matrix(Hi, Hr, align, dtype).astype(np.float64), bilinear_matrix(Wi, Wr, align, dtype).astype(np.float64)
    v = np.einsum("oi,boxc,xj->bijc", my, g, mx, optimize=True)
    a = np.einsum("oi,boxc,xj->bijc", my, np.abs(g), mx, optimize=True)
    n = max(1, bilinear_footprint(Hi, Wi, Hr, Wr, align))
    if din_old is not None:
        old = np.asarray(din_old, np.float64)
        v, a, n = v + old, a + np.abs(old), n + 1
    # c: wy * wx and its product with the gradient; one more where both taps of an output fall on the pixel and are added
    return v, (n + _c("bilinear transpose: wy*wx, * g, merged taps", 3)) * U * a


def fuse_sum(same, lows, align, relu, dtype=np.float32):
    """relu?(sum of same-resolution terms + sum of resized low-resolution terms) -> (value, bound)"""
    v = sum(np.asarray(t, np.float64) for t in same)
    a = sum(np.abs(np.asarray(t, np.float64)) for t in same)
    _, H, W, _ = same[0].shape
    for t in lows:
        r, _ = bilinear_fwd(t, H, W, align, dtype=dtype)
        ra, _ = bilinear_fwd(np.abs(np.asarray(t, np.float64)), H, W, align, dtype=dtype)
        v, a = v + r, a + ra
    # outer chain: one addition per term; inside a resized term 3 additions and 2 products (bilinear_fwd): n = terms + 3, c = 2
    bound = (len(same) + len(lows) + 3 + _c("fuse_sum: the two weight products of a tap", 2)) * U * a
    return (np.maximum(v, 0.0) if relu else v), bound


# =========================================================================== glue: exact fp32 restatements
def add(a, b, relu=False):
    v = np.asarray(a, np.float32) + np.asarray(b, np.float32)
    return np.maximum(v, np.float32(0)) if relu else v


def copy(src, dst_old=None):
    src = np.asarray(src, np.float32)
    return src.copy() if dst_old is None else np.asarray(dst_old, np.float32) + src


def relu_bwd(dz, z):
    return np.where(np.asarray(z, np.float32) > 0, np.asarray(dz, np.float32), np.float32(0))


def absmax(x):
    return np.float32(np.abs(np.asarray(x, np.float32)).max())


def nchw_to_nhwc(x):
    return np.ascontiguousarray(np.asarray(x, np.float32).transpose(0, 2, 3, 1))


def nhwc_to_nchw(x):
    return np.ascontiguousarray(np.asarray(x, np.float32).transpose(0, 3, 1, 2))


def weight_cols_gather(w, widths):
    """w [rows, Cin] -> the blocks [rows, width_j] laid end to end, flat"""
    w = np.asarray(w, np.float32)
    edges = np.cumsum([0] + list(widths))
    return np.concatenate([w[:, edges[j]:edges[j + 1]].reshape(-1) for j in range(len(widths))])


def weight_cols_scatter_add(blocks, rows, widths, dw_old):
    out = np.asarray(dw_old, np.float32).copy()
    edges, off = np.cumsum([0] + list(widths)), 0
    for j, wd in enumerate(widths):
        out[:, edges[j]:edges[j + 1]] += np.asarray(blocks, np.float32)[off:off + rows * wd].reshape(rows, wd)
        off += rows * wd
    return out


# =========================================================================== input builders
def rng(*key):
    return np.random.default_rng([int(k) for k in key])


def randn(shape, *key):
    return rng(*key).standard_normal(shape).astype(np.float32)


def ties(shape, *key):
    """values on a grid of 5: every 2x2 window is likely to hold equal maxima"""
    return rng(*key).integers(-2, 3, size=shape).astype(np.float32)


NEAR_ZERO = 1e-3


def bn_input(npix, C, ratio, const_channel, *key):
    """y [npix, C] fp32 with |mean| / std = ratio in every channel; const_channel: that channel holds 3.7 everywhere"""
    y = (rng(*key).standard_normal((npix, C)) + ratio).astype(np.float32)
    if const_channel is not None:
        y[:, const_channel] = np.float32(3.7)
    return y


def clear_of_zero(y, gamma, beta, eps, residual=None):
    """Moves every element whose pre-activation z = bn_train(y) (+ residual) has |z| < NEAR_ZERO away from zero, so that a ReLU
    mask recomputed in fp32 equals the float64 one: y changes, the statistics with it, so it repeats until nothing is left
    (the CPU test asserts that).  -> y (fp32)"""
    y = np.array(y, np.float32)
    for _ in range(20):
        f = bn_forward(y, gamma, beta, None, None, None, 0.0, eps, 1)["coef"][0]
        _, _, z = bn_apply(y, f, residual)
        bad = np.abs(z) < 2 * NEAR_ZERO
        if not bad.any():
            break
        step = 8 * NEAR_ZERO / np.maximum(np.abs(f[2]), 1e-6)                 # |dz| = 8 NEAR_ZERO
        y = np.where(bad, y + np.where(z >= 0, 1.0, -1.0) * np.sign(f[2] + (f[2] == 0)) * step, y).astype(np.float32)
    return y


def near_zero_left(y, gamma, beta, eps, residual=None):
    f = bn_forward(y, gamma, beta, None, None, None, 0.0, eps, 1)["coef"][0]
    return int((np.abs(bn_apply(y, f, residual)[2]) < NEAR_ZERO).sum())


# =========================================================================== case lists
EPS = 1e-5
# ---- BatchNorm statistics: (name, npix, C, nchunks, |mean|/std, constant channel)
STATS_CASES = [(f"chunks{k}", 1000, 48, k, 0.25, None) for k in (1, 15, 16, 17, 48, 49, 64, 65, 256)] + \
    [(f"C{C}", 427, C, nchunks_rule(427, C), 0.25, None) for C in CHANNEL_MAPPINGS] + \
    [("npix1", 1, 12, 1, 0.25, None), ("npix2", 2, 12, 1, 0.25, None), ("second_trip", 4160, 1024, nchunks_rule(4160, 1024), 0.25, None)] + \
    [(f"ratio{r}", 3000, 12, nchunks_rule(3000, 12), r, 5) for r in (0.25, 8, 32, 128)]
# ---- BatchNorm backward: the chunk count follows from the pixel count through ops._nchunks: (name, npix, C)
BWD_NPIX_FOR_CHUNKS = {1: 100, 15: 2600, 16: 2700, 17: 2860, 48: 8100, 49: 8250, 64: 10800, 65: 10930, 256: 43100}      # at C = 48
BWD_CASES = [(f"chunks{k}", n, 48) for k, n in BWD_NPIX_FOR_CHUNKS.items()] + [(f"C{C}", 427, C) for C in CHANNEL_MAPPINGS] + \
    [("npix1", 1, 12), ("npix2", 2, 12), ("second_trip", 4160, 1024)]
# flags of the backward, one case each (on 427 pixels x 48 channels unless the case is about a size)
# relu: where the backward's mask comes from (none / stored z / recomputed from y / mask bytes); dres: none / write / acc;
# _eval: eval mode both ways; _npix: another pixel count; strided: every operand a channel slice of a wider buffer
BN_FLAG_DEFAULTS = dict(relu="none", residual=False, dres="none", own_dy=False, null_params=False, null_running=False, strided=False,
                        repeat=1, stat_div=1, grads=True, _eval=False, _npix=427)
BN_FLAG_SPECS = {
    "plain": dict(),
    "relu_z": dict(relu="z", residual=True, dres="write"),
    "relu_recomputed": dict(relu="recomputed"),
    "relu_mask": dict(relu="mask", residual=True, dres="write"),
    "eval": dict(_eval=True),
    "eval_relu": dict(_eval=True, relu="z", residual=True, dres="acc"),
    "dres": dict(residual=True, dres="write"),
    "dres_accumulate": dict(relu="z", residual=True, dres="acc"),
    "own_dy": dict(relu="mask", residual=True, dres="write", own_dy=True),
    "no_dgamma_dbeta": dict(grads=False, relu="z"),
    "null_gamma_beta": dict(null_params=True, null_running=True, relu="recomputed"),
    "repeat3_stat_div3": dict(repeat=3, stat_div=3, _npix=429),
    "strided": dict(strided=True, relu="z", residual=True, dres="acc", own_dy=True),
    "strided_in_place": dict(strided=True, relu="mask", residual=True, dres="write"),
}
GROUP_SIZES = {1: [(427, 48)], 2: [(427, 48), (90, 12)],
               8: [(427, 48), (90, 12), (33, 4), (1000, 48), (61, 720), (7, 1024), (2, 12), (350, 96)]}


def group_relu_kind(i, npix):
    """where problem i of a group takes its ReLU mask from: with more than one problem, one brings mask bytes and the next does
    not (the masked instance of the reduce kernel then serves both), and one recomputes its mask from y"""
    return ("mask", "z", "mask", "recomputed")[i % 4] if npix > 8 else "z"


# ---- bn_fold: (Cout, row)
FOLD_CASES = [(5, 9 * 48), (4, 3), (3, 700), (2, 256)]
FOLD_NULLS = [(), ("bias",), ("gamma",), ("beta",)]
# ---- max pool: (name, B, H, W, C)
POOL_CASES = [(f"C{C}", 2, 7, 9, C) for C in CHANNEL_MAPPINGS] + [("even", 1, 6, 8, 12), ("two", 3, 2, 2, 4), ("odd_both", 2, 5, 3, 48),
                                                                  ("second_trip", 1, 130, 128, 1024)]
# ---- bilinear: geometry (name, Hi, Wi, Hr, Wr), each with both values of align_corners
RESIZE_GEOMETRIES = [("up_int", 10, 10, 20, 20), ("up_frac", 7, 9, 18, 14), ("up_4x", 39, 39, 155, 155), ("down_4x", 155, 155, 39, 39),
                     ("down_frac", 20, 20, 7, 7), ("identity", 6, 5, 6, 5), ("one_pixel", 1, 1, 5, 4), ("Hr1", 4, 6, 1, 6),
                     ("Wr1", 6, 4, 5, 1), ("rs8", 5, 5, 33, 33), ("rs4", 5, 5, 17, 17), ("up_odd", 5, 7, 11, 13)]
# (name, B, C, geometry name, align, Hout, Wout, py, px, accumulate, relu)
RESIZE_CASES = [(f"{g[0]}_a{a}", 2, 12, g[0], a, None, None, 0, 0, False, False) for g in RESIZE_GEOMETRIES for a in (1, 0)] + \
    [(f"C{C}_a{a}", 1, C, "up_odd", a, None, None, 0, 0, False, False) for C in CHANNEL_MAPPINGS for a in (1, 0)] + \
    [("placed_a1", 2, 12, "up_frac", 1, 23, 20, 2, 3, False, False), ("placed_a0", 2, 12, "up_frac", 0, 23, 20, 2, 3, False, False),
     ("placed_acc_relu", 2, 12, "up_frac", 1, 23, 20, 2, 3, True, True), ("acc", 2, 48, "up_int", 0, None, None, 0, 0, True, False),
     ("relu", 2, 48, "up_int", 1, None, None, 0, 0, False, True),
     ("fwd_second_trip", 1, 1024, "trip_up", 1, None, None, 0, 0, False, False),
     ("bwd_second_trip", 1, 1024, "trip_down", 0, None, None, 0, 0, False, False)]
RESIZE_GEOMETRIES += [("trip_up", 33, 32, 65, 64), ("trip_down", 65, 64, 33, 32)]
GEOMETRY = {g[0]: g[1:] for g in RESIZE_GEOMETRIES}
# ---- fuse_sum: (name, B, H, W, C, n_same, low sizes, align, relu)
FUSE_CASES = [("a1", 2, 12, 10, 48, 2, [(6, 5), (3, 3), (1, 2)], 1, True), ("a0", 2, 9, 11, 12, 1, [(5, 6), (2, 3)], 0, False),
              ("same_only", 1, 5, 7, 720, 4, [], 1, True)]
# ---- glue: pixel counts per channel mapping (not a multiple of P) and the second trip
GLUE_CASES = [(f"C{C}", 427, C) for C in CHANNEL_MAPPINGS] + [("second_trip", 4160, 1024)]
TRANSPOSE_CASES = [(2, C, 5, 7) for C in (1, 3, 7, 16)]
COLS_CASES = [("one", 5, [12]), ("eight", 103, [4, 8, 12, 4, 16, 8, 4, 20])]          # 103 rows x 19 quads: not a multiple of 256
FILL_LENGTHS = (1, 3, 4, 1025)
