"""The streaming body of hrseg_bilinear_bwd_multi (csrc/elem.hip bilinear_bwd_stream_kernel): dy is staged on chip row by row
and every target element is wy * (sum wx * g) summed over ascending dy rows, by one block, whatever the band count and the slab
width (hrseg_tune bwd_multi_bands / bwd_multi_slab).

Each target against hrseg_bilinear_bwd on the same dy, with the bound of tests/test_bilinear_bwd_multi_gpu.py: the two kernels
add the same n products in another order and with the weights multiplied in another order, within 2 * n * 2^-24 * A,
A = hrseg_bilinear_bwd(|dy|), n = the target's largest footprint count (tests/head_branch_ref.py).  max|dt| equals
dt.abs().max() exactly and two runs give the same bits.

Knob independence: every (bands, slab) pair gives the bits of (1 band, automatic slab) -- a wrong halo, a row stored twice or a
row missed at a band's edge shows here.

A knob that is set sends every shape the streaming body can hold to it; left to itself the library routes tensors this small
to the gather body (csrc/elem.hip hrseg_bilinear_bwd_multi), so every run here sets at least the band count.

The shapes are the smallest at which the kernel can go wrong: 23 x 19 (odd, no multiple of anything) onto 12 x 10 / 6 x 5 /
3 x 3, 40 channels inside a 48-channel buffer (row stride != C; 8-channel slabs: five of them, 16-channel slabs: a ragged
third one), 1 / 2 / 4 bands and 99 (clamped to the coarsest target's 3 rows)."""
import contextlib

import pytest
import torch

from tests import nonfinite_ref as N
from tests.head_branch_ref import bilinear_matrix, footprint_count

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
B, H, W, C = 2, 23, 19, 40
TARGETS = [(12, 10), (6, 5), (3, 3)]
BANDS = [1, 2, 4, 99]
SLABS = [0, 8, 16]


@contextlib.contextmanager
def knobs(bands=0, slab=0):
    from hrseg_amd import _lib
    _lib.tune(bwd_multi_bands=bands, bwd_multi_slab=slab)
    try:
        yield
    finally:
        _lib.tune(bwd_multi_bands=0, bwd_multi_slab=0)


def run(dy, targets, align, bands=0, slab=0):
    from hrseg_amd import ops
    with knobs(bands, slab):
        dts, amax = ops.bilinear_bwd_multi(dy, targets, align, want_absmax=True)
    torch.cuda.synchronize()
    return dts, amax


def reference(dy, targets, align):
    """per target: hrseg_bilinear_bwd(dy), the bound 2 * n * 2^-24 * hrseg_bilinear_bwd(|dy|)"""
    from hrseg_amd import ops
    Bn, Hn, Wn, Cn = dy.shape
    out = []
    for h, w in targets:
        want = ops.bilinear_bwd(dy, (Bn, h, w, Cn), Hn, Wn, 0, 0, align)
        A = ops.bilinear_bwd(dy.abs(), (Bn, h, w, Cn), Hn, Wn, 0, 0, align)
        out.append((want.double(), 2 * footprint_count(h, w, Hn, Wn, align) * U * A.double()))
    return out


def check(dy, targets, align, got, ref, what):
    dts, amax = got
    for j, (h, w) in enumerate(targets):
        want, bound = ref[j]
        delta = (dts[j].double() - want).abs()
        print(f"{what} target {h}x{w}: max |delta| {float(delta.max()):.3e}, "
              f"max delta/bound {float((delta / bound.clamp_min(1e-300)).max()):.3f}")
        assert bool((delta <= bound).all()), f"{what}: target {h}x{w} outside the bound"
        assert float(amax[j].max()) == float(dts[j].abs().max()), f"{what}: absmax of target {h}x{w}"


_case = {}


def main_case(align):
    """dy, the references and the (1 band, automatic slab) outputs of the main case, computed once per align setting"""
    if align not in _case:
        gen = torch.Generator(device="cuda").manual_seed(31 + int(align))
        dy = torch.randn((B, H, W, C + 8), generator=gen, device="cuda")[..., 4:4 + C]
        _case[align] = (dy, reference(dy, TARGETS, align), run(dy, TARGETS, align, bands=1, slab=0))
    return _case[align]


@pytest.mark.parametrize("slab", SLABS)
@pytest.mark.parametrize("bands", BANDS)
@pytest.mark.parametrize("align", [True, False], ids=["align", "noalign"])
def test_every_band_count_and_slab_width(align, bands, slab):
    dy, ref, base = main_case(align)
    got = run(dy, TARGETS, align, bands, slab)
    check(dy, TARGETS, align, got, ref, f"align={align} bands={bands} slab={slab}")
    again = run(dy, TARGETS, align, bands, slab)
    for j in range(len(TARGETS)):
        assert torch.equal(again[0][j], got[0][j]), "two runs differ"
        assert torch.equal(got[0][j], base[0][j]), f"target {TARGETS[j]}: the bits depend on bands={bands} / slab={slab}"
    assert torch.equal(again[1], got[1])
    assert torch.equal(got[1].max(dim=1).values, base[1].max(dim=1).values)


EDGES = {
    "scale-1": ((2, 23, 19, 8), [(23, 19), (6, 5)], (True, False)),                # a target of dy's own size: footprint 1
    "one-row-align": ((2, 23, 19, 8), [(12, 10), (1, 2)], (True,)),                # scale 0: every dy row feeds the one row
    "H1": ((2, 1, 19, 8), [(1, 10), (1, 3)], (True, False)),
    "W1": ((2, 23, 1, 8), [(12, 1), (3, 1)], (True, False)),
    "B1": ((1, 23, 19, 8), [(12, 10), (6, 5), (3, 3)], (True, False)),
    "one-target": ((2, 23, 19, 8), [(6, 5)], (True, False)),
    "up-sizing": ((2, 23, 19, 8), [(26, 19), (6, 5)], (True, False)),              # Hi = H + 3 (no model issues one)
    "head-layout": ((2, 9, 11, 720), [(5, 6), (3, 3), (1, 2)], (True, False)),     # 720 channels: the thread layout of the head
    "wide-block": ((1, 5, 40, 240), [(3, 20), (2, 7)], (False,)),                  # slab forced to 240 channels: 1024 threads
}
FORCED = {"wide-block": dict(bands=2, slab=240)}                                   # every other edge: 3 bands, 8-channel slabs


@pytest.mark.parametrize("name", list(EDGES))
def test_edges(name):
    shape, targets, aligns = EDGES[name]
    kn = FORCED.get(name, dict(bands=3, slab=8))
    for align in aligns:
        gen = torch.Generator(device="cuda").manual_seed(len(name) + int(align))
        dy = torch.randn(shape, generator=gen, device="cuda")
        ref = reference(dy, targets, align)
        one = run(dy, targets, align, bands=1)
        check(dy, targets, align, one, ref, f"{name} align={align}")
        forced = run(dy, targets, align, **kn)
        again = run(dy, targets, align, **kn)
        for j in range(len(targets)):
            assert torch.equal(forced[0][j], one[0][j]), f"{name}: the bits depend on the knobs"
            assert torch.equal(again[0][j], forced[0][j]), f"{name}: two runs differ"
        assert torch.equal(again[1], forced[1])


@pytest.mark.parametrize("align", [True, False], ids=["align", "noalign"])
def test_non_finite_gradients_stay_inside_their_support(align):
    """bands forced to 4 (clamped to 3 by the coarsest target): a NaN on the first and a +Inf on the last dy row that feeds the
    inner band of the finest target, each in a plane of its own"""
    shape = (B, H, W, 8)
    h0 = TARGETS[0][0]
    nb = min(4, min(h for h, _ in TARGETS))
    r0, r1 = -(-1 * h0 // nb), -(-2 * h0 // nb)                        # band 1: rows [ceil(Hi / nb), ceil(2 Hi / nb))
    feeds = (bilinear_matrix(h0, H, align)[:, r0:r1] != 0).any(axis=1).nonzero()[0]
    poison = {"nan": (0, int(feeds[0]), 5, 1), "+inf": (1, int(feeds[-1]), 12, 6)}
    d = N.base(shape, 91)
    for special, pos in poison.items():
        d = N.poisoned(d, pos, special)
    dts, amax = run(d.cuda(), TARGETS, align, bands=4)
    for j, (h, w) in enumerate(TARGETS):
        got = dts[j].cpu()
        rest = torch.ones(got.shape, dtype=torch.bool)
        for special, pos in poison.items():
            must, may = N.resize_bwd_sets(h, w, H, W, align, pos[1], pos[2])
            N.check_sets(got[pos[0], :, :, pos[3]], must, may, f"target {h}x{w}: {special} at {pos}")
            rest[pos[0], :, :, pos[3]] = False
        assert bool(torch.isfinite(got[rest]).all()), f"target {h}x{w}: another plane went non-finite"
        assert float(amax[j].max()) == float("inf"), "absmax: a non-finite gradient reads +Inf"


def _fuse_backward(same, lows, dz, multi, pre=None):
    """Recorder.fuse_sum forward + backward on fresh Acts -> (gradients of the same-resolution terms, of the low ones)"""
    from hrseg_amd import _lib
    from hrseg_amd.engine import Act, Recorder
    rec = Recorder(training=True, record=True)
    sa, la = [Act(t.clone()) for t in same], [Act(t.clone()) for t in lows]
    if pre is not None:
        la[-1].grad = pre.clone()
    _lib.tune(fuse_bwd_multi=int(multi))
    try:
        y = rec.fuse_sum([(a, False) for a in sa] + [(a, True) for a in la])
        y.grad = dz.clone()
        rec.backward()
    finally:
        _lib.tune(fuse_bwd_multi=1)
    torch.cuda.synchronize()
    return [a.grad for a in sa], [a.grad for a in la]


@pytest.mark.parametrize("branch", [0, 1])
def test_fuse_layer_backward_routes_agree(branch):
    """B = 2, branches 16 x 16 x 8 / 8 x 8 x 16 / 4 x 4 x 32: the fuse layer of branch 0 (two low-resolution terms) and of
    branch 1 (two same-resolution terms, one low one), fuse_bwd_multi off and on; then with the last low term already holding a
    gradient (it keeps the accumulating launch on either route)"""
    from hrseg_amd import ops
    gen = torch.Generator(device="cuda").manual_seed(5 + branch)
    rnd = lambda *s: torch.randn(s, generator=gen, device="cuda")
    (h, c), lowhw = [((16, 8), (8, 4)), ((8, 16), (4,))][branch]
    same = [rnd(2, h, h, c) for _ in range(1 + branch)]
    lows = [rnd(2, s, s, c) for s in lowhw]
    dz = rnd(2, h, h, c)
    for pre in (None, rnd(*lows[-1].shape)):
        s_off, l_off = _fuse_backward(same, lows, dz, False, pre)
        s_on, l_on = _fuse_backward(same, lows, dz, True, pre)
        for x, y in zip(s_off, s_on):
            assert torch.equal(x, y), "a same-resolution term's gradient changed"
        g = s_off[-1]                                                 # relu_bwd(dz): the gradient both routes transpose
        for j, (x, y) in enumerate(zip(l_off, l_on)):
            s = lowhw[j]
            A = ops.bilinear_bwd(g.abs(), (2, s, s, c), h, h, 0, 0, True)
            bound = 2 * footprint_count(s, s, h, h, True) * U * A.double()
            delta = (x.double() - y.double()).abs()
            print(f"branch {branch} low {s}x{s} pre={pre is not None}: max delta/bound "
                  f"{float((delta / bound.clamp_min(1e-300)).max()):.3f}")
            assert bool((delta <= bound).all())
        if pre is not None:
            assert torch.equal(l_off[-1], l_on[-1]), "a term that already held a gradient keeps the accumulating launch"
