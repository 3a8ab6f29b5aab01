"""The non-finite contract of the activation path in one place (include/hrseg.h, 'non-finite values on the activation path'):
what a kernel must do with a NaN, a +Inf or a -Inf among its inputs.  Plain torch references, the case lists and the input
builders that tests/test_nonfinite_cpu.py and tests/test_nonfinite_gpu.py share (the pattern of tests/headloss_ref.py).

Pointwise and reducing operations (ReLU, max pooling, BatchNorm, add, copy, the ReLU backward, clamp, the softmax maxima,
absmax): the CLASS of every output element -- finite, +Inf, -Inf or NaN -- equals the class of the float64 torch reference on
the same float32 inputs, and the elements that are finite in both meet the bar the operation already has in
tests/test_kernels_gpu.py / tests/headloss_ref.py.  Inputs are O(1) random float32 values plus ONE special value at a named
position, so float32 and float64 arithmetic agree on every class (nothing is near an overflow or a cancellation to Inf - Inf
that only one precision sees).

Resize kernels: a tap whose interpolation weight is exactly 0 gives NaN in one evaluation order (0 * NaN) and is skipped in
another (the gather backward skips zero weights, autograd multiplies by them), so the contract is a pair of sets:
    must = outputs whose weight on the poisoned element is robustly non-zero,
    may  = outputs whose 2 x 2 support touches the poisoned element,
and  must <= nonfinite(output) <= may.  `must` takes the float64 weight above RESIZE_W_MIN = 1e-5 rather than "non-zero": the
source coordinate carries float32 rounding of a few 1e-7 relative (scale * index, index <= 18 here), which can turn a float64
weight of 1e-16 at an exactly-integer coordinate into a true 0 but cannot remove a weight of 1e-5; `may` is the union of the
supports computed with float32 and with float64 coordinates for the same reason.  At the shapes below may \\ must is at most
RESIZE_MAY_CAP = 5 % of the outputs of the poisoned plane (asserted by the CPU test for every case).
"""
import torch
import torch.nn.functional as F

from tests.headloss_ref import BAR_POINT, BAR_REDUCED, EPS_GATE, _gen  # noqa: F401  (the bars are taken, not invented)

FINITE, POS_INF, NEG_INF, NAN = 0, 1, 2, 3
SPECIALS = {"nan": float("nan"), "+inf": float("inf"), "-inf": float("-inf")}
BAR_BN = 1e-5            # tests/test_kernels_gpu.py::test_batchnorm_train_fwd_bwd, z / running statistics
BAR_CONV = {"f32": 2e-5, "small_cin": 1e-5, "fp16x2": 2e-5}      # test_conv_fwd_dgrad_wgrad / first-layer test / test_ws_gpu.TOL


def classes(t):
    """int8 tensor of the shape of t: FINITE, POS_INF, NEG_INF or NAN per element"""
    t = t.detach().cpu()
    c = torch.full(t.shape, FINITE, dtype=torch.int8)
    c[t == float("inf")] = POS_INF
    c[t == float("-inf")] = NEG_INF
    c[torch.isnan(t)] = NAN
    return c


def check_classes(got, ref, bar, what, absolute=False):
    """the pointwise / reducing contract: equal class maps; where both are finite, max |got - ref| <= bar * max |ref| over the
    finite elements of ref (absolute=True: bar itself).  -> the measured figure"""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    cg, cr = classes(got), classes(ref)
    if not torch.equal(cg, cr):
        bad = (cg != cr).nonzero()
        i = tuple(int(v) for v in bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {cg.numel()} elements differ in class from the float64 reference; first at "
                             f"{i}: got {float(got[i])!r}, reference {float(ref[i])!r}")
    fin = cr == FINITE
    if not bool(fin.any()):
        return 0.0
    scale = 1.0 if absolute else max(float(ref[fin].abs().max()), 1e-12)
    d = float((got[fin] - ref[fin]).abs().max()) / scale
    assert d <= bar, f"{what}: finite elements {d:.3e} from the reference, bar {bar:.1e}"
    return d


# ------------------------------------------------------------------------------------------------ inputs (NHWC, float32)
def base(shape, *key, scale=1.0, shift=0.0):
    return torch.randn(shape, generator=_gen(*key, *shape)) * scale + shift


def positions(shape):
    """named positions of an NHWC tensor: one interior element, and the last channel of the last pixel (the tail lanes)"""
    B, H, W, C = shape
    return {"interior": (B // 2, H // 2, W // 2, min(5, C - 1)), "tail": (B - 1, H - 1, W - 1, C - 1)}


def grad_positions(shape):
    """named positions of the OUTPUT-side (upstream gradient) tensor of a resize, NHWC: the interior pixel is one step off the
    centre, (Ho//2 + 1, Wo//2 + 1) -- at RESIZE_CASES the centre pixel of 5x7 -> 13x11 has an exactly-integer source coordinate
    on both axes in both align modes (one tap of weight 1, three of weight 0: may \\ must = 3 of 35), this one has a fractional
    coordinate on both axes in every case and mode (four taps of non-zero weight); the tail is the last pixel's last channel,
    whose source is the clamped last input pixel (one tap)"""
    B, H, W, C = shape
    return {"interior": (B // 2, H // 2 + 1, W // 2 + 1, min(5, C - 1)), "tail": (B - 1, H - 1, W - 1, C - 1)}


def poisoned(x, pos, special):
    x = x.clone()
    x[pos] = SPECIALS[special]
    return x


def nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


# ------------------------------------------------------------------------------------------------ references (float64)
def bn_ref(y, gamma, beta, rm, rv, training, residual=None, relu=True, momentum=0.1, eps=1e-5):
    """NHWC float32 inputs -> dict(z NHWC, pre = z in front of the ReLU, rm, rv, mask [npix][C/4] or None) in float64
    (mask: bit j = channel 4q+j of `pre` > 0, so 0 for NaN)"""
    rm64, rv64 = rm.double().clone(), rv.double().clone()
    z = F.batch_norm(nchw(y.double()), rm64, rv64, gamma.double(), beta.double(), training, momentum, eps)
    if residual is not None:
        z = z + nchw(residual.double())
    C = y.shape[-1]
    pre = nhwc(z)
    mask = ((pre.reshape(-1, C // 4, 4) > 0).to(torch.int32) * torch.tensor([1, 2, 4, 8], dtype=torch.int32)).sum(-1).to(torch.uint8)
    if relu:
        z = F.relu(z)
    return dict(z=nhwc(z), pre=pre, rm=rm64, rv=rv64, mask=mask if relu else None)


def maxpool_ref(x):
    return nhwc(F.max_pool2d(nchw(x.double()), 2))


def resize_ref(x, Ho, Wo, align):
    return nhwc(F.interpolate(nchw(x.double()), size=(Ho, Wo), mode="bilinear", align_corners=align))


def conv_ref(x, w_store, bias, k, s, residual=None, relu=True):
    """x NHWC, w_store [Cout][k*k][Cin] -> NHWC float64"""
    cout, cin = w_store.shape[0], w_store.shape[-1]
    w = w_store.double().reshape(cout, k, k, cin).permute(0, 3, 1, 2)
    y = F.conv2d(nchw(x.double()), w, None if bias is None else bias.double(), stride=s, padding=(k - 1) // 2)
    if residual is not None:
        y = y + nchw(residual.double())
    return nhwc(F.relu(y) if relu else y)


def group_kl_ref(z, pprev, parents, sizes):
    """[G] sums over batch, pixels and children of Q (log Q + log size), Q = softmax(z + log(P_parent + 1e-6)).clamp_min(1e-8),
    and d(sum of all groups' sums * per-group 1/size)/dz as hrseg_group_kl_bwd scales it (scale = 1, upstream 1)"""
    z = z.double().clone().requires_grad_(True)
    sums, start, total = [], 0, 0.0
    for par, n in zip(parents, sizes):
        q = torch.softmax(z[:, start:start + n] + torch.log(pprev[:, par:par + 1].double() + 1e-6), dim=1).clamp(min=1e-8)
        s = (q * (q.log() + torch.log(torch.tensor(float(n), dtype=torch.float64)))).sum()
        sums.append(s)
        total = total + s / n
        start += n
    total.backward()
    return torch.stack(sums).detach(), z.grad


# ------------------------------------------------------------------------------------------------ resize: must / may
RESIZE_CASES = [(7, 9, 14, 18), (5, 7, 13, 11)]        # Hi, Wi, Ho, Wo: non-integer scales in at least one mode and axis
RESIZE_W_MIN = 1e-5
RESIZE_MAY_CAP = 0.05


def _taps(n_in, n_out, align, dtype):
    """torch's upsample_bilinear2d source index, in `dtype`: (i0, i1, l0, l1) per output index"""
    o = torch.arange(n_out, dtype=dtype)
    num, den = (n_in - 1, max(n_out - 1, 1)) if align else (n_in, n_out)
    scale = torch.tensor(float(num), dtype=dtype) / torch.tensor(float(den), dtype=dtype)        # (the division in `dtype`)
    r = scale * o if align else (scale * (o + 0.5) - 0.5).clamp(min=0.0)
    i0 = r.floor().long().clamp(max=n_in - 1)
    i1 = (i0 + 1).clamp(max=n_in - 1)
    l1 = r - i0.to(dtype)
    return i0, i1, 1.0 - l1, l1


def _axis(n_in, n_out, align, p):
    """per output index: (float64 weight on input index p, whether p is in the support under float32 or float64 coordinates)"""
    i0, i1, l0, l1 = _taps(n_in, n_out, align, torch.float64)
    w = l0 * (i0 == p) + l1 * (i1 == p)
    j0, j1, _, _ = _taps(n_in, n_out, align, torch.float32)
    return w, (i0 == p) | (i1 == p) | (j0 == p) | (j1 == p)


def resize_sets(Hi, Wi, Ho, Wo, align, py, px):
    """forward resize with input pixel (py, px) poisoned -> (must, may) bool [Ho, Wo]"""
    wy, sy = _axis(Hi, Ho, align, py)
    wx, sx = _axis(Wi, Wo, align, px)
    return (wy[:, None] * wx[None, :]) > RESIZE_W_MIN, sy[:, None] & sx[None, :]


def resize_bwd_sets(Hi, Wi, Ho, Wo, align, oy, ox):
    """transpose (gradient of the resize) with OUTPUT-side pixel (oy, ox) of the upstream gradient poisoned -> (must, may)
    bool [Hi, Wi]: the inputs that pixel interpolates from"""
    must, may = torch.zeros(Hi, Wi, dtype=torch.bool), torch.zeros(Hi, Wi, dtype=torch.bool)
    for py in range(Hi):
        wy, sy = _axis(Hi, Ho, align, py)
        for px in range(Wi):
            wx, sx = _axis(Wi, Wo, align, px)
            must[py, px] = bool(wy[oy] * wx[ox] > RESIZE_W_MIN)
            may[py, px] = bool(sy[oy] & sx[ox])
    return must, may


def check_sets(got_plane, must, may, what, relu_neg_inf=False):
    """must <= nonfinite(got) <= may on one [H, W] plane.  relu_neg_inf: the special is -Inf and a ReLU follows -- a non-zero
    weight gives -Inf, which the ReLU maps to 0 as torch's does: the must elements are exactly 0 and only zero-weight taps
    (0 * Inf = NaN) may stay non-finite"""
    got_plane = got_plane.detach().cpu()
    bad = ~torch.isfinite(got_plane)
    if relu_neg_inf:
        # (a must element may ALSO tap the poisoned element with weight 0 -- at the clamped last row / column both taps are
        # the same element -- and is then NaN in either evaluation order: 0 or NaN, never another finite value or an infinity)
        m = got_plane[must]
        assert bool(((m == 0) | torch.isnan(m)).all()), f"{what}: relu(-Inf * positive weight) must be 0 (NaN beside a zero-weight tap)"
        assert not bool((bad & ~may).any()), f"{what}: non-finite outputs outside the poisoned element's support"
        return
    assert not bool((must & ~bad).any()), f"{what}: {int((must & ~bad).sum())} outputs that interpolate from the poisoned element are finite"
    assert not bool((bad & ~may).any()), f"{what}: {int((bad & ~may).sum())} non-finite outputs outside the poisoned element's support"
