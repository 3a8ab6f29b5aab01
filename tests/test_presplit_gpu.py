"""Pre-split activations at the kernel level (include/hrseg.h: hrseg_bn_fwd_t.z_split / residual_split,
hrseg_conv_shape_t.x_split), through the C ABI.

The format has one writer and three readers, and writer and readers use the same split (csrc/sp_arith.h: hrseg_split_f16x2 ==
sp_split<4, .> with scale 1, side by side), so the strongest statements available are cheap and are the ones asserted here:

  writer    BatchNorm apply with z_split writes, byte for byte, split_ref.pack(z) of the fp32 tensor the same launch writes
            without the flag (tests/split_ref.py is a torch-CPU model that shares nothing with the library; it is pinned by
            tests/test_presplit_cpu.py) -- and nothing else of the launch changes;
  readers   the wave-specialised forward kernels, the nine-tap weight gradient and BatchNorm's residual_split give, BIT FOR
            BIT, what the same kernel gives on the fp32 tensor (resp. on hi + lo for the residual); the launch counters prove
            that both calls took the route the case is about; fp32 torch on the CPU pins each case within the fp16x2 tolerance;
  refusals  every other route refuses an x_split operand (RuntimeError naming x_split), launches nothing and leaves the output
            untouched -- never a misread tensor.

A staging path that dropped or swapped a `lo` dword on one tile kind would move the conv output by ~1e-4 relative: inside
the 1e-3 bar of the model-level tests, outside equality."""
import contextlib

import pytest
import torch
import torch.nn.functional as F

from tests import split_ref as S
from tests.test_ws_gpu import TOL, X_SPLIT_SETS, _rel

pytestmark = pytest.mark.gpu

DEFAULTS = dict(sp_ws=1, sp_ws_n48=1, sp_ws_canvas=5, sp_ws_waste=200, sp_ws_min_tiles=0, wgrad9=1)
FAMILIES = ("ws", "ws_group", "ws_canvas", "wgrad9")


@contextlib.contextmanager
def _tuned(**kv):
    """hrseg_tune knobs for the duration of a block; every knob this file touches goes back to its default afterwards"""
    from hrseg_amd import _lib
    try:
        _lib.tune(**kv)
        yield
    finally:
        _lib.tune(**DEFAULTS)


@pytest.fixture(autouse=True)
def _restore_switches():
    from hrseg_amd import _lib
    yield
    _lib.tune(**DEFAULTS)
    _lib.set_deterministic(False)


def _routes(n48=1, canvas=5):
    """the routing of the existing kernel tests: thresholds down to one tile, any padding accepted"""
    return _tuned(sp_ws_min_tiles=1, sp_ws_waste=1000, sp_ws_n48=n48, sp_ws_canvas=canvas)


def _counted(fn):
    """fn() -> (result, {family: launches}, all convolution launches)"""
    from hrseg_amd import _lib
    _lib.launch_count(None, reset=True)
    out = fn()
    return out, {f: _lib.launch_count(f) for f in FAMILIES}, _lib.launch_count(None)


def _packed(x):
    """fp32 NHWC (host) -> the device tensor holding its pre-split bytes (typed fp32, as the C ABI takes it)"""
    return S.as_f32_bytes(S.pack(x)).cuda()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _activation(shape, g):
    """unit normal, half of the elements through ReLU: many exact zeros, as after BatchNorm + ReLU, next to negative values"""
    x = torch.randn(shape, generator=g)
    return torch.where(torch.rand(shape, generator=g) < 0.5, x.clamp_min(0.0), x)


# ====================================================================================================================
# 2. the writer: BatchNorm z_split, and the residual reader
# ====================================================================================================================
def _assert_bytes_are_the_model(z_bytes, z32, what):
    """the device's pre-split bytes against split_ref on the fp32 tensor: every fp16 piece bit for bit (where the model's
    piece is NaN: NaN-ness instead of the payload)"""
    dev = _bits(z_bytes).cpu()
    ref = z32.detach().cpu()
    mh, ml = S.split(ref)
    dh, dl = S.unpack(dev)
    for name, m, d in (("hi", mh, dh), ("lo", ml, dl)):
        nan = torch.isnan(m)
        assert torch.equal(torch.isnan(d), nan), f"{what}: NaN pieces of `{name}` differ"
        mb, db = m.view(torch.int16), d.view(torch.int16)
        bad = (mb != db) & ~nan
        if bool(bad.any()):
            sub = S.subnormal(m) & bad
            i = int(bad.reshape(-1).nonzero()[0])
            raise AssertionError(
                f"{what}: {int(bad.sum())} of {bad.numel()} `{name}` pieces differ from the model ({int(sub.sum())} of them where "
                f"the model's piece is a nonzero fp16 subnormal); first: x = {float(ref.reshape(-1)[i])!r}, device "
                f"0x{int(db.reshape(-1)[i]) & 0xffff:04x}, model 0x{int(mb.reshape(-1)[i]) & 0xffff:04x}")
    if not bool(torch.isnan(mh).any() | torch.isnan(ml).any()):
        assert torch.equal(dev, S.pack(ref)), f"{what}: granule layout"


class _BnProblem:
    """one BatchNorm problem with host-side state: every run gets fresh device copies (the launch updates running statistics)"""

    def __init__(self, shape, g, relu, residual=None, mask=False, gamma_scale=1.0, **extra):
        C = shape[-1]
        self.shape, self.relu, self.mask, self.extra = shape, relu, mask, extra
        self.y = torch.randn(shape, generator=g) * 1.5 + 0.3
        self.gamma = (torch.rand(C, generator=g) + 0.5) * gamma_scale
        self.beta = torch.randn(C, generator=g) * 0.3
        self.rm = torch.randn(C, generator=g) * 0.2
        self.rv = torch.rand(C, generator=g) + 0.5
        self.residual = residual                  # None | fp32 host tensor | ("split", host tensor): stored pre-split

    def item(self, z_split, residual_as=None):
        """residual_as: None = as constructed, "joined" = a ("split", r) residual given as the fp32 tensor hi + lo"""
        res, res_split = self.residual, False
        if isinstance(res, tuple):
            if residual_as == "joined":
                res = S.join(S.pack(res[1])).cuda()
            else:
                res, res_split = _packed(res[1]), True
        elif res is not None:
            res = res.cuda()
        npix = self.shape[0] * self.shape[1] * self.shape[2]
        it = dict(y=self.y.cuda(), gamma=self.gamma.cuda(), beta=self.beta.cuda(), rm=self.rm.cuda(), rv=self.rv.cuda(),
                  nbt=torch.full((), 3, dtype=torch.int64, device="cuda"), momentum=0.1, eps=1e-5, residual=res, relu=self.relu,
                  z_split=z_split, residual_split=res_split, **self.extra)
        if self.mask:
            it["relu_mask"] = torch.full((npix, self.shape[-1] // 4), 0xA5, dtype=torch.uint8, device="cuda")
        return it


def _bn_run(problems, training, z_splits, residual_as=None):
    from hrseg_amd import ops
    items = [p.item(s, residual_as) for p, s in zip(problems, z_splits)]
    out = ops.bn_fwd_group(items, training)
    torch.cuda.synchronize()
    return [dict(z=z, coef=coef, rm=it["rm"], rv=it["rv"], nbt=it["nbt"], mask=it.get("relu_mask")) for (z, coef), it in zip(out, items)]


def _assert_only_the_format_changed(plain, split, what):
    for k in ("coef", "rm", "rv"):
        assert _same_bits(plain[k], split[k]), f"{what}: `{k}` depends on z_split"
    assert torch.equal(plain["nbt"], split["nbt"]), what
    if plain["mask"] is not None:
        assert torch.equal(plain["mask"], split["mask"]), f"{what}: relu_mask depends on z_split"


def _check_writer(problems, training, what, flags=None):
    flags = flags if flags is not None else [True] * len(problems)
    plain = _bn_run(problems, training, [False] * len(problems))
    split = _bn_run(problems, training, flags)
    for i, (a, b, f) in enumerate(zip(plain, split, flags)):
        w = f"{what}, problem {i}"
        _assert_only_the_format_changed(a, b, w)
        if f:
            _assert_bytes_are_the_model(b["z"], a["z"], w)
        else:
            assert _same_bits(a["z"], b["z"]), f"{w}: an fp32 output changed because ANOTHER problem of the launch is split"
    return plain


# one C per thread layout of csrc/elem_common.h make_lanes (Q = C / 4 channel quads, P = 256 / Q pixel lanes, threads beyond
# P * Q idle): 16 / 64: Q divides 256, every thread works; 48 (P = 21), 96 (P = 10), 192 (P = 5), 384 (P = 2): 4, 16, 16
# and 64 idle threads; 1024: Q = 256, P = 1 (one pixel per block pass)
BN_CHANNELS = [16, 48, 64, 96, 192, 384, 1024]


@pytest.mark.parametrize("C", BN_CHANNELS)
def test_bn_z_split_writes_the_model_bytes(C):
    """3 x 7 x 9 = 189 pixels (no multiple of any lane count): ReLU on / off (off: negative values, and -0.0 pieces), without
    residual, with an fp32 residual, with a residual and relu_mask bytes; training and eval.

    Every piece is compared, the many fp16-subnormal `lo` pieces of |z| ~ 1 included (|z| in [1, 2): one element in 16; a
    quarter of a unit normal): the library is built with fp16 denormals on, so a piece flushed to zero is a defect here, and the
    failure message says how many of the differing pieces are subnormal in the model."""
    g = torch.Generator().manual_seed(100 + C)
    shape = (3, 7, 9, C)
    res = torch.randn(shape, generator=g)
    n_sub = 0
    for relu in (True, False):
        for residual, mask in ((None, False), (res, False), (res, True)):
            for training in (True, False):
                p = _BnProblem(shape, g, relu, residual=residual, mask=mask)
                plain = _check_writer([p], training, f"C={C} relu={relu} residual={residual is not None} mask={mask} training={training}")
                z = plain[0]["z"].cpu()
                n_sub += int(S.subnormal(S.split(z)[1]).sum())
                assert bool((z < 0).any()) != relu and (not relu or bool((z == 0).any()))
                if mask and relu:
                    want = (z.reshape(-1, C // 4, 4) > 0).to(torch.int32)
                    want = (want * torch.tensor([1, 2, 4, 8], dtype=torch.int32)).sum(-1).to(torch.uint8)
                    assert torch.equal(plain[0]["mask"].cpu(), want)
    assert n_sub > 0, "the case never produced a subnormal piece: it cannot see a flush to zero"


def test_bn_z_split_ragged_image_and_batched_pass_bookkeeping():
    """2 x 20 x 23 pixels; the batched-pass bookkeeping (two identical copies of a pass in one tensor: stat_div = 2, statistics
    entering the running averages twice: repeat = 2) is untouched by the flag"""
    g = torch.Generator().manual_seed(7)
    p = _BnProblem((2, 20, 23, 96), g, True)
    for training in (True, False):
        _check_writer([p], training, f"20 x 23, training={training}")
    q = _BnProblem((4, 7, 9, 48), g, True, repeat=2, stat_div=2)
    q.y = torch.cat([q.y[:2], q.y[:2]])
    plain = _check_writer([q], True, "repeat / stat_div = 2")
    once = _BnProblem((4, 7, 9, 48), g, True)
    once.y, once.gamma, once.beta, once.rm, once.rv = q.y, q.gamma, q.beta, q.rm, q.rv
    ref = _bn_run([once], True, [False])
    assert int(plain[0]["nbt"]) == 5 and int(ref[0]["nbt"]) == 4            # (the bookkeeping is really on in this case)
    assert not torch.equal(plain[0]["rv"], ref[0]["rv"])


def test_bn_z_split_is_per_problem_in_a_grouped_launch():
    """two problems of different C in ONE launch, one of them split: each follows its own flag"""
    g = torch.Generator().manual_seed(8)
    a = _BnProblem((3, 7, 9, 48), g, True)
    b = _BnProblem((2, 5, 11, 64), g, False, residual=torch.randn((2, 5, 11, 64), generator=g))
    for flags in ([True, False], [False, True]):
        for training in (True, False):
            _check_writer([a, b], training, f"group, z_split={flags}, training={training}", flags)


@pytest.mark.parametrize("relu", [False, True])
def test_bn_z_split_out_of_range_values_follow_the_model(relu):
    """eval mode, gamma ~ 4e4: a fifth of z lies in (65504, 1.3e5), where hi saturates at +-65504 and lo stays finite; a few
    elements lie beyond (lo overflows to Inf: the loud behaviour of hrseg.h); channel 3 of y is +-Inf and channel 5 NaN"""
    g = torch.Generator().manual_seed(9)
    p = _BnProblem((3, 7, 9, 16), g, relu, gamma_scale=4.0e4)
    p.y[..., 3] = torch.where(p.y[..., 3] > 0, float("inf"), float("-inf"))
    p.y[..., 5] = float("nan")
    p.y[0, 0, :4, 0] = torch.tensor([3.0, -3.0, 6.0, -6.0])                  # |z| ~ 1e5 and beyond 1.3e5, whatever the seed
    p.gamma[0], p.rv[0], p.rm[0], p.beta[0] = 4.0e4, 1.0, 0.0, 0.0
    plain = _check_writer([p], False, f"out of range, relu={relu}")
    z = plain[0]["z"].cpu()
    fin = torch.isfinite(z)
    assert bool(((z.abs() > 65504) & (z.abs() < 1.3e5) & fin).float().mean() > 0.05)
    assert bool((z[fin].abs() > 1.4e5).any()) and bool(torch.isinf(z).any())
    # the ReLU keeps NaN (include/hrseg.h, non-finite values stay loud): the NaN channel stays NaN with it and without it; of the
    # infinite channel it removes -Inf only, as torch's does
    assert bool(torch.isnan(z[..., 5]).all()) and bool((z[..., 3] == float("inf")).any())
    assert bool((z[..., 3] == float("-inf")).any()) != relu and bool((z[..., 3] == 0).any()) == relu


@pytest.mark.parametrize("C", [48, 64])
@pytest.mark.parametrize("relu", [False, True])
def test_bn_residual_split_adds_hi_plus_lo(C, relu):
    """the residual stored pre-split gives, bit for bit, what its fp32 value hi + lo gives: z, relu_mask, and the pre-split
    output when the launch also writes z_split (the engine's block chain does both)"""
    g = torch.Generator().manual_seed(30 + C)
    shape = (3, 7, 9, C)
    r = _activation(shape, g) * 3.0
    p = _BnProblem(shape, g, relu, residual=("split", r), mask=True)
    for training in (True, False):
        joined = _bn_run([p], training, [False], residual_as="joined")[0]
        split = _bn_run([p], training, [False])[0]
        what = f"C={C} relu={relu} training={training}"
        assert _same_bits(joined["z"], split["z"]), f"{what}: residual_split changed z"
        assert torch.equal(joined["mask"], split["mask"]), f"{what}: residual_split changed relu_mask"
        assert _same_bits(joined["coef"], split["coef"]) and _same_bits(joined["rv"], split["rv"])
        both = _bn_run([p], training, [True])[0]
        _assert_bytes_are_the_model(both["z"], joined["z"], what + ", z_split too")
        # ... and the value is the 22-bit one, not the fp32 residual's
        exact = _BnProblem(shape, g, relu, residual=r)
        exact.y, exact.gamma, exact.beta, exact.rm, exact.rv = p.y, p.gamma, p.beta, p.rm, p.rv
        z_exact = _bn_run([exact], training, [False])[0]["z"]
        assert not torch.equal(z_exact, split["z"]) and float((z_exact - split["z"]).abs().max()) < 1e-5


# ====================================================================================================================
# 3. the readers: x_split gives the bits of the fp32 input
# ====================================================================================================================
def _conv_case(cin, cout, H, W, B, seed):
    g = torch.Generator().manual_seed(seed)
    xf = _activation((B, H, W, cin), g)
    w = torch.randn(cout, 9, cin, generator=g) / (9 * cin) ** 0.5           # storage layout [Cout][tap][Cin]
    bias = torch.randn(cout, generator=g)
    return xf, w, bias


def _torch_conv(xf, w, bias):
    """fp32 torch-CPU convolution of NHWC x with the storage-layout weight -> NHWC"""
    cout, _, cin = w.shape
    y = F.conv2d(xf.permute(0, 3, 1, 2), w.view(cout, 3, 3, cin).permute(0, 3, 1, 2), bias, stride=1, padding=1)
    return y.permute(0, 2, 3, 1)


def _check_forward_single(xf, xs, w, bias, canvas, what, stat_rows=None):
    """precision auto and fp16x2, with and without bias: the pre-split call equals the fp32 call bit for bit, one `ws` launch
    each (canvas-tiled or not, as the case says); fp32 torch within TOL; stat_rows: the number of persistent blocks the launch
    reports for its epilogue statistics (= ceil(tiles / ceil(tiles / 256)): it tells 8- from 16-row tiles)"""
    from hrseg_amd import _lib, ops
    xd, wd, bd = xf.cuda(), w.cuda(), bias.cuda()
    want = {"ws": 1, "ws_group": 0, "ws_canvas": int(canvas), "wgrad9": 0}
    y_first = None
    for prec in ("auto", "fp16x2"):
        pr = _lib.CONV_PRECISION[prec]
        for b in (None, bd):
            y32, c32, n32 = _counted(lambda: ops.conv_fwd(xd, wd, b, 3, 1, prec=pr))
            ysp, csp, nsp = _counted(lambda: ops.conv_fwd(xs, wd, b, 3, 1, prec=pr, x_split=True))
            w_ = f"{what}, {prec}, bias={b is not None}"
            assert c32 == want and n32 == 1, (w_, "fp32 input", c32, n32)
            assert csp == want and nsp == 1, (w_, "pre-split input", csp, nsp)
            assert torch.equal(y32, ysp), f"{w_}: the pre-split input gives other bits than the fp32 input " \
                                          f"(max |diff| {float((y32 - ysp).abs().max()):.3e}, {int((y32 != ysp).sum())} elements)"
            if b is not None and y_first is None:
                y_first = ysp
    ref = _torch_conv(xf, w, bias)
    assert _rel(y_first, ref) < TOL, (what, _rel(y_first, ref))
    if stat_rows is not None:
        auto = _lib.CONV_PRECISION["auto"]
        (y1, st1), c1, _ = _counted(lambda: ops.conv_fwd(xd, wd, None, 3, 1, prec=auto, stats=True))
        (y2, st2), c2, _ = _counted(lambda: ops.conv_fwd(xs, wd, None, 3, 1, prec=auto, stats=True, x_split=True))
        assert c1 == want and c2 == want
        assert st1 is not None and st2 is not None and st1[1] == stat_rows and st2[1] == stat_rows, (what, st1 and st1[1], st2 and st2[1])
        assert torch.equal(y1, y2)


# Cin, Cout, H, W, B, n48, canvas, rows of epilogue statistics (None: not asked).  Shapes moved from the ones first listed for
# this test, each to the nearest that takes the intended route (csrc/conv.hip ws_kind / ws_canvas):
#   96-channel tiles want >= 160 of them (B ceil(H/8) ceil(W/16) at 96 channels): 35 x 52 at B = 8 (5 x 4 tiles per image);
#     at B = 2 the layer runs 48-channel tiles instead;
#   192 channels at 20 x 20, B = 3 are 36 96-channel tiles: the case runs 48-channel tiles (n48 = 1) -- still four K stages on a
#     canvas of pitch 21;
#   the canvas must cut the padded area by 5 %: at pitch 14 (33 x 13 images) from B = 8 on (7 tile columns instead of 8).
FWD_CASES = [
    # 48-channel tiles, one K stage, per-image tiling: tiles y0 = 8 .. 32, x0 = 16, 32 are interior ("fast": y0 >= 1,
    # y0 + 9 <= 41, x0 >= 1, x0 + 17 <= 53), the rest ragged border tiles; 2 * 6 * 4 = 48 tiles of 8 rows (16 rows: 24)
    (48, 48, 41, 53, 2, 1, False, 48),
    (96, 96, 35, 52, 8, 0, False, None),      # 96-channel tiles (n48 = 0: no 48-channel tiling to fall to), two K stages
    (96, 96, 35, 52, 2, 1, False, None),      # the same layer on 48-channel tiles: two channel tiles x two K stages
    (64, 128, 29, 37, 3, 0, False, None),     # the 64-channel tilings
    (128, 64, 30, 38, 2, 0, False, None),
    (192, 192, 20, 20, 3, 1, True, None),     # four K stages, canvas of pitch 21
    (128, 64, 33, 13, 8, 0, True, None),      # canvas of pitch 14 < 18: the exact per-granule address path (cv_narrow)
    (96, 48, 17, 9, 5, 1, True, None),        # pitch 10, 48-channel tiles, two K stages
    # 16-row tiles: 48-channel tiles of a layer that has no 96-channel tiling, >= 256 tiles of 16 x 16 with <= 10 % padding:
    # 2 * 7 * 7 pixel tiles x 3 channel tiles = 294 -> 147 blocks (8-row tiles: 588 -> 196); interior and ragged tiles
    (48, 144, 109, 111, 2, 1, False, 147),
]


@pytest.mark.parametrize("case", FWD_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_forward_on_presplit_input_equals_fp32_input_bit_for_bit(case):
    cin, cout, H, W, B, n48, canvas, rows = case
    xf, w, bias = _conv_case(cin, cout, H, W, B, seed=sum(case[:5]))
    xs = _packed(xf)
    with _routes(n48=n48, canvas=5 if canvas else 0):
        _check_forward_single(xf, xs, w, bias, canvas, str(case), stat_rows=rows)


def test_forward_reads_what_batchnorm_wrote():
    """writer and reader chained: the input of the convolution is the z_split output of a BatchNorm + ReLU launch, the fp32
    twin the output of the same launch without the flag"""
    g = torch.Generator().manual_seed(12)
    cin, cout, shape = 48, 48, (2, 41, 53, 48)
    p = _BnProblem(shape, g, True)
    z32 = _bn_run([p], True, [False])[0]["z"]
    zsp = _bn_run([p], True, [True])[0]["z"]
    assert not torch.equal(z32, zsp) and bool((z32 == 0).float().mean() > 0.2)
    _, w, bias = _conv_case(cin, cout, 41, 53, 2, seed=13)
    with _routes(n48=1, canvas=0):
        _check_forward_single(z32.cpu(), zsp, w, bias, False, "BatchNorm -> conv")


def _branches(g, B=4):
    chans, sizes = [48, 96, 192, 384], [(33, 41), (17, 21), (9, 11), (5, 6)]
    xf = [_activation((B, h, w, c), g) for c, (h, w) in zip(chans, sizes)]
    ws = [torch.randn(c, 9, c, generator=g) / (9 * c) ** 0.5 for c in chans]
    return chans, xf, ws


def test_grouped_forward_on_presplit_inputs():
    """the four parallel branches as ONE grouped launch (auto arithmetic): all inputs pre-split, and mixed (problems 0 and 2
    only): every output equals the all-fp32 grouped call bit for bit.  With epilogue statistics the outputs are still equal and
    the statistics rows add up to the sums of the output (the rows themselves are not bit-stable: LDS atomics)."""
    from hrseg_amd import _lib, ops
    auto = _lib.CONV_PRECISION["auto"]
    chans, xf, ws = _branches(torch.Generator().manual_seed(14))
    xd, xs, wd = [x.cuda() for x in xf], [_packed(x) for x in xf], [w.cuda() for w in ws]
    mixes = {"all": [True] * 4, "mixed": [True, False, True, False]}
    with _routes(n48=1, canvas=5):
        y32, c32, n32 = _counted(lambda: ops.conv_fwd_group(xd, wd, [None] * 4, 3, 1, chans, prec=auto))
        assert c32["ws_group"] == 1 and c32["ws"] == 0 and n32 == 1, (c32, n32)
        for i in range(4):
            assert _rel(y32[i], _torch_conv(xf[i], ws[i], None)) < TOL, i
        for name, flags in mixes.items():
            xin = [s if f else d for s, d, f in zip(xs, xd, flags)]
            ysp, csp, nsp = _counted(lambda: ops.conv_fwd_group(xin, wd, [None] * 4, 3, 1, chans, prec=auto, x_splits=flags))
            assert csp == c32 and nsp == 1, (name, csp, nsp)
            for i in range(4):
                assert torch.equal(ysp[i], y32[i]), f"{name}: branch {i} differs from the all-fp32 grouped call"
            (yst, stats), cst, nst = _counted(lambda: ops.conv_fwd_group(xin, wd, [None] * 4, 3, 1, chans, prec=auto, stats=True,
                                                                         x_splits=flags))
            assert cst == c32 and nst == 1, (name, cst, nst)
            for i, (y, st, co) in enumerate(zip(yst, stats, chans)):
                assert torch.equal(y, y32[i]), f"{name}, statistics on: branch {i} differs"
                assert st is not None, "the wave-specialised launch reported no statistics rows"
                part, rows = st
                assert 0 < rows <= 256
                tot = part[:rows * 2 * co].view(rows, 2, co).sum(0).cpu()
                y64 = y.double().reshape(-1, co).cpu()
                s1, s2 = y64.sum(0), (y64 * y64).sum(0)
                assert float((tot[0] - s1).abs().max()) < 1e-5 * float(s2.sqrt().max()) * 30, (name, i)
                assert float(((tot[1] - s2) / s2).abs().max()) < 2e-6, (name, i)


WGRAD_SETS = {
    "branches": [(48, 48, 29, 37, 3), (96, 96, 15, 19, 3), (192, 192, 8, 10, 3)],
    "tiles64": [(64, 128, 21, 27, 2), (128, 64, 11, 14, 2)],
}


def _wgrad_inputs(shapes, g):
    xf = [_activation((b, h, w, ci), g) for ci, co, h, w, b in shapes]
    dys = [(torch.randn(b, h, w, co, generator=g) * 1e-3).cuda() for ci, co, h, w, b in shapes]
    gms = [d.abs().max().reshape(1).repeat(64) for d in dys]
    base = [torch.randn(co, 9, ci, generator=g).cuda() for ci, co, h, w, b in shapes]
    return xf, dys, gms, base


@pytest.mark.parametrize("name", list(WGRAD_SETS))
def test_nine_tap_weight_gradient_on_presplit_inputs(name):
    """conv_wgrad_group on the nine-tap kernel (no atomics), accumulating into an existing dw: all inputs pre-split, and mixed:
    the bits of the fp32-input call; fp16x2 and auto; values against fp64 torch on the CPU"""
    from hrseg_amd import _lib, ops
    shapes = WGRAD_SETS[name]
    xf, dys, gms, base = _wgrad_inputs(shapes, torch.Generator().manual_seed(40 + len(name)))
    xd, xs = [x.cuda() for x in xf], [_packed(x) for x in xf]
    n = len(shapes)
    want = {"ws": 0, "ws_group": 0, "ws_canvas": 0, "wgrad9": 1}

    def run(xin, flags, pr):
        dws = [b.clone() for b in base]
        _, c, total = _counted(lambda: ops.conv_wgrad_group(xin, dys, dws, 3, 1, prec=pr, gmaxs=gms, x_splits=flags))
        assert c == want and total == 1, (name, flags, c, total)
        return dws

    for prec in ("fp16x2", "auto"):
        pr = _lib.CONV_PRECISION[prec]
        d32 = run(xd, None, pr)
        for flags in ([True] * n, [i % 2 == 0 for i in range(n)]):
            dsp = run([s if f else d for s, d, f in zip(xs, xd, flags)], flags, pr)
            for i in range(n):
                assert torch.equal(dsp[i], d32[i]), f"{name}, {prec}, x_splits={flags}: dw of problem {i} differs from the fp32-input call"
        if prec == "fp16x2":
            for a, b0, x, dy, (ci, co, h, w, b) in zip(d32, base, xf, dys, shapes):
                wr = torch.zeros(co, ci, 3, 3, dtype=torch.float64, requires_grad=True)
                F.conv2d(x.double().permute(0, 3, 1, 2), wr, padding=1).backward(dy.double().permute(0, 3, 1, 2).cpu())
                assert _rel((a - b0).view(co, 3, 3, ci).permute(0, 3, 1, 2), wr.grad) < TOL, (name, ci, co)
    # a single problem through conv_wgrad
    pr = _lib.CONV_PRECISION["fp16x2"]
    d1, d2 = base[0].clone(), base[0].clone()
    _, c1, _ = _counted(lambda: ops.conv_wgrad(xd[0], dys[0], d1, 3, 1, prec=pr, gmax=gms[0]))
    _, c2, t2 = _counted(lambda: ops.conv_wgrad(xs[0], dys[0], d2, 3, 1, prec=pr, gmax=gms[0], x_split=True))
    assert c1 == want and c2 == want and t2 == 1
    assert torch.equal(d1, d2)


@pytest.mark.parametrize("name,probs,want", X_SPLIT_SETS, ids=[s[0] for s in X_SPLIT_SETS])
def test_where_x_split_ok_says_yes_the_presplit_calls_work(name, probs, want):
    """the promise of hrseg_conv_x_split_ok kept with the flag SET: where it answers 1, the forward and weight-gradient calls
    of those problems succeed on packed inputs and give the bits of the fp32 calls"""
    from hrseg_amd import _lib, ops
    auto = _lib.CONV_PRECISION["auto"]
    B, H = 2, 32
    _lib.ensure_scratch(torch.device("cuda:0"))
    g = torch.Generator().manual_seed(11)
    xf = [_activation((B, H, H, ci), g) for ci, co, k, s, relu in probs]
    with _tuned(sp_ws_min_tiles=1):
        shapes = [ops._shape(tuple(x.shape), ci, co, co, k, s, auto, relu=relu) for x, (ci, co, k, s, relu) in zip(xf, probs)]
        got = int(_lib.conv_x_split_ok(ops._shape_array(shapes), len(shapes)))
        assert got == want
        if not got:
            return
        n = len(probs)
        couts = [p[1] for p in probs]
        xd, xs = [x.cuda() for x in xf], [_packed(x) for x in xf]
        ws = [(torch.randn(co, 9, ci, generator=g) / (9 * ci) ** 0.5).cuda() for ci, co, *_ in probs]
        if n == 1:
            y32 = [ops.conv_fwd(xd[0], ws[0], None, 3, 1, prec=auto)]
            ysp, c, total = _counted(lambda: [ops.conv_fwd(xs[0], ws[0], None, 3, 1, prec=auto, x_split=True)])
        else:
            y32 = ops.conv_fwd_group(xd, ws, [None] * n, 3, 1, couts, prec=auto)
            ysp, c, total = _counted(lambda: ops.conv_fwd_group(xs, ws, [None] * n, 3, 1, couts, prec=auto, x_splits=[True] * n))
        assert c["ws"] + c["ws_group"] == 1 and total == 1, (name, c, total)
        for a, b in zip(y32, ysp):
            assert torch.equal(a, b), f"{name}: forward"
        dys = [torch.randn(y.shape, generator=g).cuda() * 1e-3 for y in y32]
        gms = [d.abs().max().reshape(1).repeat(64) for d in dys]
        d32, dsp = [torch.zeros_like(w) for w in ws], [torch.zeros_like(w) for w in ws]
        ops.conv_wgrad_group(xd, dys, d32, 3, 1, prec=auto, gmaxs=gms)
        _, c, total = _counted(lambda: ops.conv_wgrad_group(xs, dys, dsp, 3, 1, prec=auto, gmaxs=gms, x_splits=[True] * n))
        assert c["wgrad9"] == 1 and total == 1, (name, c, total)
        for a, b in zip(d32, dsp):
            assert torch.equal(a, b), f"{name}: weight gradient"
            assert bool(a.abs().max() > 0)


# ====================================================================================================================
# 4. refusals: every other route fails loudly, launches nothing, writes nothing
# ====================================================================================================================
SENTINEL = 777.0


def _fwd_group_into(xs, ws, outs, k, s, prec, x_splits):
    """ops.conv_fwd_group with caller-owned outputs (the refusal tests look at them afterwards)"""
    from hrseg_amd import _lib, ops
    _lib.ensure_scratch(xs[0].device)
    shapes = [ops._shape(x.shape, ops._ld(x), y.shape[3], ops._ld(y), k, s, prec, x_split=q) for x, y, q in zip(xs, outs, x_splits)]
    _lib.call("hrseg_conv_fwd_group", len(xs), _lib.ptr_array(xs), _lib.ptr_array(ws), None, _lib.ptr_array(outs),
              ops._shape_array(shapes))


def _refusal_cases():
    from hrseg_amd import _lib, ops
    P = _lib.CONV_PRECISION
    g = torch.Generator().manual_seed(50)
    B, H = 2, 32
    x48, x64 = _activation((B, H, H, 48), g), _activation((B, H, H, 64), g)       # finite values: a route that misread the bytes
    s48, s64 = _packed(x48), _packed(x64)                                         # as fp32 would compute wrong numbers, no more
    w3 = (torch.randn(48, 9, 48, generator=g) / 21).cuda()
    w3_64 = (torch.randn(64, 9, 64, generator=g) / 24).cuda()
    w1 = (torch.randn(48, 1, 48, generator=g) / 7).cuda()
    dy = (torch.randn(B, H, H, 48, generator=g) * 1e-3).cuda()
    dy64 = (torch.randn(B, H, H, 64, generator=g) * 1e-3).cuda()
    gm, gm64 = dy.abs().max().reshape(1).repeat(64), dy64.abs().max().reshape(1).repeat(64)

    def out(c=48, h=H):
        return torch.full((B, h, h, c), SENTINEL, device="cuda")

    def dw(co=48, taps=9, ci=48):
        return torch.full((co, taps, ci), SENTINEL, device="cuda")

    cases = {}

    def case(name, make, **knobs):
        cases[name] = (make, knobs)

    def fwd(k, s, prec, h=H):
        def make():
            o = out(h=h)
            return [o], lambda: ops.conv_fwd(s48, w1 if k == 1 else w3, None, k, s, out=o, prec=P[prec], x_split=True)
        return make

    case("k1", fwd(1, 1, "auto"))
    case("stride2", fwd(3, 2, "auto", h=H // 2))
    case("f32", fwd(3, 1, "f32"))
    case("bf16", fwd(3, 1, "bf16"))
    case("bf16x3", fwd(3, 1, "bf16x3"))
    case("sp_ws_off", fwd(3, 1, "auto"), sp_ws=0)

    def group_fp16x2():
        o = [out(), out()]
        return o, lambda: _fwd_group_into([s48, s48], [w3, w3], o, 3, 1, P["fp16x2"], [True, True])
    case("explicit_fp16x2_group", group_fp16x2)

    def wgrad_k1():
        d = dw(taps=1)
        return [d], lambda: ops.conv_wgrad(s48, dy, d, 1, 1, prec=P["fp16x2"], gmax=gm, x_split=True)
    case("wgrad_k1", wgrad_k1)

    def wgrad_no_workspace():
        d = [dw(), dw()]
        return d, lambda: ops.conv_wgrad_group([s48, s48], [dy, dy], d, 3, 1, prec=P["auto"], gmaxs=[gm, gm], x_splits=[True, True])
    case("wgrad_group_without_nine_tap", wgrad_no_workspace, wgrad9=0)

    # a 48- with a 64-channel problem: the nine-tap weight gradient wants ONE tile size per call, so hrseg_conv_x_split_ok says
    # no and the weight-gradient call refuses (the forward group is looked at in the test itself)
    def wgrad_48_64():
        d = [dw(), dw(64, 9, 64)]
        return d, lambda: ops.conv_wgrad_group([s48, s64], [dy, dy64], d, 3, 1, prec=P["auto"], gmaxs=[gm, gm64], x_splits=[True, True])
    case("wgrad_group_48_with_64", wgrad_48_64)
    return cases, dict(x48=x48, x64=x64, s48=s48, s64=s64, w3=w3, w3_64=w3_64)


REFUSALS = ["k1", "stride2", "f32", "bf16", "bf16x3", "sp_ws_off", "explicit_fp16x2_group", "wgrad_k1",
            "wgrad_group_without_nine_tap", "wgrad_group_48_with_64"]


def _assert_refused(call, outputs):
    from hrseg_amd import _lib
    torch.cuda.synchronize()
    before = _lib.launch_count(None)
    with pytest.raises(RuntimeError, match="x_split") as e:
        call()
    assert "(-3)" in str(e.value), str(e.value)                 # HRSEG_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert _lib.launch_count(None) == before, "a refused call launched a convolution kernel"
    for o in outputs:
        assert bool((o == SENTINEL).all()), "a refused call wrote to its output"


@pytest.mark.parametrize("name", REFUSALS)
def test_routes_that_cannot_read_the_form_refuse_it(name):
    from hrseg_amd import _lib, ops
    auto = _lib.CONV_PRECISION["auto"]
    cases, t = _refusal_cases()
    assert sorted(cases) == sorted(REFUSALS)
    make, knobs = cases[name]
    with _tuned(sp_ws_min_tiles=1):
        legal32 = ops.conv_fwd(t["x48"].cuda(), t["w3"], None, 3, 1, prec=auto)
        try:
            _lib.tune(**knobs)
            outputs, call = make()
            _assert_refused(call, outputs)
        finally:
            _lib.tune(**{k: DEFAULTS[k] for k in knobs})
        again, c, total = _counted(lambda: ops.conv_fwd(t["s48"], t["w3"], None, 3, 1, prec=auto, x_split=True))
        assert c["ws"] == 1 and total == 1
        assert torch.equal(again, legal32), "the legal pre-split call after a refusal"


def test_forward_group_of_48_and_64_channels_is_never_misread():
    """hrseg_conv_x_split_ok answers 0 for a 48- with a 64-channel problem because of the weight gradient (refused above).  The
    forward group of the pair may take the wave-specialised group launch, which reads the form -- then it must give the fp32
    call's bits -- or refuse; it must never compute on misread bytes"""
    from hrseg_amd import _lib, ops
    auto = _lib.CONV_PRECISION["auto"]
    _, t = _refusal_cases()
    with _tuned(sp_ws_min_tiles=1):
        xd = [t["x48"].cuda(), t["x64"].cuda()]
        ws = [t["w3"], t["w3_64"]]
        shapes = [ops._shape(tuple(x.shape), c, c, c, 3, 1, auto) for x, c in zip(xd, (48, 64))]
        assert int(_lib.conv_x_split_ok(ops._shape_array(shapes), 2)) == 0
        y32 = [torch.empty_like(xd[0]), torch.empty_like(xd[1])]
        _fwd_group_into(xd, ws, y32, 3, 1, auto, [False, False])
        outs = [torch.full_like(y32[0], SENTINEL), torch.full_like(y32[1], SENTINEL)]
        torch.cuda.synchronize()
        before, group_before = _lib.launch_count(None), _lib.launch_count("ws_group")
        try:
            _fwd_group_into([t["s48"], t["s64"]], ws, outs, 3, 1, auto, [True, True])
        except RuntimeError as e:
            assert "x_split" in str(e)
            torch.cuda.synchronize()
            assert _lib.launch_count(None) == before and all(bool((o == SENTINEL).all()) for o in outs)
        else:
            assert _lib.launch_count("ws_group") == group_before + 1 and _lib.launch_count(None) == before + 1
            for a, b in zip(outs, y32):
                assert torch.equal(a, b)
