"""The clipping kernels of csrc/optim.hip -- the fp64 sum of squares, the finalize + step-count launch and AdamW with a verdict -- against
tests/gradclip_ref.py at the smallest sizes where they can go wrong.  With CH = the library's chunk length and MB = the most
blocks a launch uses (both read from the library): n = 1, 3 run the scalar tail alone, 4 exactly one 16-byte piece, 5 and
1023 pieces plus tail; CH-1 / CH / CH+1 sit around the unguarded full-chunk path; 2*CH+5 is two full chunks and a one-element
tail; (MB+2)*CH+7 has more chunks than the launch has blocks (blocks 0 and 1 take a second chunk, block 2 the partial
one); 8192*1024+5 is the size at which AdamW's own grid-stride loop takes a second trip (headloss_ref.ADAMW_N).

Bars: norm and coef are fp64 results stored once as fp32; the fp64 sum's own error is below 1e-12 at these sizes, so 2 ulp
(rtol 2.4e-7) holds them.  p, m, v: headloss_ref.ADAMW_BARS.  "Bitwise" means torch.equal."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import gradclip_ref as G
from tests import headloss_ref as R

pytestmark = pytest.mark.gpu

RTOL = 2.4e-7
GSCALE = R.ADAMW_GSCALE
INF = math.inf


@pytest.fixture(scope="module")
def ops():
    from hrseg_amd import ops as o
    assert torch.cuda.is_available()
    return o


@pytest.fixture(scope="module")
def geom():
    from hrseg_amd import _lib
    return _lib.grad_sumsq_chunk_len(), _lib.grad_sumsq_max_blocks()


def _sizes(CH, MB):
    return [1, 3, 4, 5, 1023, CH - 1, CH, CH + 1, 2 * CH + 5, (MB + 2) * CH + 7, 8192 * 1024 + 5]


N_IDS = ["1", "3", "4", "5", "1023", "CH-1", "CH", "CH+1", "2CH+5", "more_chunks_than_blocks", "adamw_large"]
SMALL = [3, 4, 6, 7, 8]                   # indices into _sizes: 5, 1023, CH, CH+1, 2CH+5
LARGE = 10


def _hyper(lr, wd, gscale=GSCALE):
    return torch.tensor([lr, R.ADAMW_BETA1, R.ADAMW_BETA2, R.ADAMW_EPS, wd, gscale], dtype=torch.float32, device="cuda")


def _cfg(max_norm, skip):
    return torch.tensor([max_norm, float(skip)], dtype=torch.float32, device="cuda")


def _reduce(ops, g, hyper, cfg, state=None, clip=None):
    state = torch.zeros(3, device="cuda") if state is None else state
    clip = torch.zeros(4, device="cuda") if clip is None else clip
    partial = ops.grad_sumsq(g)
    ops.grad_clip_finalize(partial, hyper, cfg, state, clip)
    return partial, state, clip


def _close(got, want):
    return abs(float(got) - want) <= RTOL * abs(want)


def _grad(n, seed=0):
    return 4.0 * torch.randn(n, generator=torch.Generator().manual_seed(1000 + seed + n % 100003))


# ================================================================================================ norm, coef, reproducibility
@pytest.mark.parametrize("i", range(len(N_IDS)), ids=N_IDS)
def test_norm_coef_and_reproducibility(ops, geom, i):
    from hrseg_amd import _lib
    n = _sizes(*geom)[i]
    g = _grad(n)
    ref = G.verdict(g, GSCALE)
    gd, hyper = g.cuda(), _hyper(1e-3, 0.01)
    assert _lib.grad_sumsq_chunks(n) == -(-n // geom[0])
    for factor in (0.5, 2.0, INF):
        max_norm = G.f32(factor * ref["norm32"])
        want = G.verdict(g, GSCALE, max_norm)
        partial, state, clip = _reduce(ops, gd, hyper, _cfg(max_norm, True))
        partial2, _, clip2 = _reduce(ops, gd, hyper, _cfg(max_norm, True))
        got = clip.tolist()
        print(f"n={n} max_norm={max_norm}: norm {got[0]!r} (ref {want['norm32']!r}) coef {got[1]!r} (ref {want['coef32']!r})")
        assert partial.numel() == _lib.grad_sumsq_chunks(n)
        assert abs(float(partial.sum()) - want["S"]) <= 1e-12 * want["S"]
        assert _close(got[0], want["norm32"]) and _close(got[1], want["coef32"]) and got[2] == 1.0 and got[3] == 0.0
        assert (got[1] == 1.0) == (factor >= 2.0) and (factor == 0.5) == (0.49 < got[1] < 0.51)
        assert np.allclose(state.cpu().numpy(), np.array(R.adamw_state(1), np.float32), rtol=1.2e-7, atol=0)
        assert torch.equal(partial, partial2) and torch.equal(clip, clip2)          # the same buffer reduced twice


@pytest.mark.parametrize("mag,max_norm", [(1e20, 1e18), (1e-30, 1e-7)], ids=["1e20", "1e-30"])
def test_range_beyond_fp32_squares(ops, geom, mag, max_norm):
    """|g| ~ 1e20: fp32 squares overflow; ~ 1e-30: they vanish.  An fp32 square or accumulator fails here."""
    for n in (5, 2 * geom[0] + 5):
        gen = torch.Generator().manual_seed(n)
        g = (torch.rand(n, generator=gen) * 0.5 + 0.5) * mag * (torch.randint(0, 2, (n,), generator=gen) * 2 - 1)
        assert not (0.0 < float((g * g).sum()) < INF)
        want = G.verdict(g, GSCALE, max_norm)
        _, _, clip = _reduce(ops, g.cuda(), _hyper(1e-3, 0.01), _cfg(max_norm, True))
        got = clip.tolist()
        print(f"n={n} mag={mag}: norm {got[0]!r} (ref {want['norm32']!r}) coef {got[1]!r} (ref {want['coef32']!r})")
        assert want["finite"] and want["coef32"] < 1.0
        assert _close(got[0], want["norm32"]) and _close(got[1], want["coef32"]) and got[2] == 1.0


# ================================================================================================ verdict and the void step
def _poison(g, kind, CH):
    g = g.clone()
    if kind == "nan_last_tail":
        g[-1] = math.nan
    elif kind == "inf_mid_chunk":
        g[CH + CH // 2] = INF
    else:
        g[CH // 3], g[CH + 17] = INF, -INF
    return g


@pytest.mark.parametrize("kind", ["nan_last_tail", "inf_mid_chunk", "inf_pair"])
def test_nonfinite_verdict_and_void_step(ops, geom, kind):
    CH = geom[0]
    n = 2 * CH + 5                                    # n % 4 == 1: the last element is the scalar tail
    x = R.adamw_inputs(n)
    g0, g1, g2 = x["grads"][:3]
    bad = _poison(g1, kind, CH)
    wd, max_norm = 0.01, 3.0
    hyper, cfg = _hyper(1e-3, wd), _cfg(max_norm, True)
    p, m, v = x["p"].cuda(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    state, clip = torch.zeros(3, device="cuda"), torch.zeros(4, device="cuda")

    def step(g):
        _reduce(ops, g, hyper, cfg, state, clip)
        ops.adamw_dev_clip(p, g, m, v, hyper, state, cfg, clip)

    step(g0.cuda())
    before = [t.clone() for t in (p, m, v, state)]
    step(bad.cuda())
    assert clip[2].item() == 0.0 and clip[3].item() == 1.0
    assert all(torch.equal(a, b) for a, b in zip((p, m, v, state), before))       # bitwise untouched
    hyper[0] = 5e-4
    step(g2.cuda())
    ref = G.run(x["p"], [g0, g2], [1e-3, 5e-4], wd, torch.float64, max_norms=[max_norm] * 2, skip=True)   # never saw `bad`
    assert clip[2].item() == 1.0 and clip[3].item() == 1.0
    assert np.allclose(state.cpu().numpy(), np.array(R.adamw_state(2), np.float32), rtol=1.2e-7, atol=0)
    for name, got in (("p", p), ("m", m), ("v", v)):
        assert R.rel(got, ref.tensors()[name]) < R.ADAMW_BARS[name], (kind, name, R.rel(got, ref.tensors()[name]))
    # skip clear: same verdict, but no special case -- the step counts
    _, state2, clip2 = _reduce(ops, bad.cuda(), hyper, _cfg(max_norm, False))
    assert clip2[2].item() == 0.0 and clip2[3].item() == 0.0 and state2[0].item() == 1.0


# ================================================================================================ off means off
@pytest.mark.parametrize("i", SMALL + [LARGE], ids=[N_IDS[i] for i in SMALL + [LARGE]])
def test_max_norm_inf_is_adamw_dev_bitwise(ops, geom, i):
    n = _sizes(*geom)[i]
    x = R.adamw_inputs(n)
    p0, grads = x["p"].cuda(), [g.cuda() for g in x["grads"]]
    for wd, gscale in ((0.0, GSCALE), (0.01, 1.0 / 3.0)):
        pa, ma, va, sa = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0), torch.zeros(3, device="cuda")
        pb, mb, vb, sb = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0), torch.zeros(3, device="cuda")
        hyper, cfg, clip = _hyper(R.ADAMW_LRS[0], wd, gscale), _cfg(INF, True), torch.zeros(4, device="cuda")
        for k, lr in enumerate(R.ADAMW_LRS):
            hyper[0] = lr
            ops.adamw_dev(pa, grads[k], ma, va, hyper, sa)
            _reduce(ops, grads[k], hyper, cfg, sb, clip)
            ops.adamw_dev_clip(pb, grads[k], mb, vb, hyper, sb, cfg, clip)
            assert clip[1].item() == 1.0
            for name, a, b in (("p", pa, pb), ("m", ma, mb), ("v", va, vb), ("state", sa, sb)):
                assert torch.equal(a, b), (n, wd, gscale, k, name)


# ================================================================================================ clipping
@pytest.mark.parametrize("factor", [0.5, 2.0])
@pytest.mark.parametrize("i", SMALL + [LARGE], ids=[N_IDS[i] for i in SMALL + [LARGE]])
def test_clipped_update_matches_reference(ops, geom, i, factor):
    n = _sizes(*geom)[i]
    x = R.adamw_inputs(n)
    steps = 2 if i == LARGE else len(R.ADAMW_LRS)          # the fp64 reference of 8M elements runs on the host
    grads = [g.cuda() for g in x["grads"][:steps]]
    for wd in R.ADAMW_WDS:
        p, m, v = x["p"].cuda(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
        hyper, cfg = _hyper(R.ADAMW_LRS[0], wd), _cfg(INF, False)
        state, clip = torch.zeros(3, device="cuda"), torch.zeros(4, device="cuda")
        ref = G.Run(x["p"], wd, torch.float64)
        for k in range(steps):
            hyper[0] = R.ADAMW_LRS[k]
            _, _, probe = _reduce(ops, grads[k], hyper, cfg)                      # the measured norm of this gradient
            max_norm = G.f32(factor * probe[0].item())
            cfg[0] = max_norm                                                     # a new threshold: written to the device
            _reduce(ops, grads[k], hyper, cfg, state, clip)
            ops.adamw_dev_clip(p, grads[k], m, v, hyper, state, cfg, clip)
            want = ref.step(x["grads"][k], R.ADAMW_LRS[k], max_norm)
            assert _close(clip[0].item(), want["norm32"]) and _close(clip[1].item(), want["coef32"])
            assert (clip[1].item() < 1.0) == (factor < 1.0)
        for name, got in (("p", p), ("m", m), ("v", v)):
            d = R.rel(got, ref.tensors()[name])
            print(f"n={n} wd={wd} factor={factor} {name}: rel {d:.2e} (bar {R.ADAMW_BARS[name]:.0e})")
            assert d < R.ADAMW_BARS[name], (n, wd, factor, name, d)


# ================================================================================================ argument checks
def test_bad_arguments_are_refused_before_any_launch(geom):
    """placeholder pointers, never dereferenced: every call below must return -1 from the host-side checks"""
    from hrseg_amd import _lib
    CH = geom[0]
    P, ODD4, ODD8 = ctypes.c_void_p(4096), ctypes.c_void_p(4100), ctypes.c_void_p(4104)
    sumsq, fin, upd = (_lib._fn[k] for k in ("hrseg_grad_sumsq", "hrseg_grad_clip_finalize", "hrseg_adamw_dev_clip"))
    n, k = 2 * CH + 5, 3
    bad = [sumsq(None, n, P, k, None), sumsq(P, n, None, k, None), sumsq(P, 0, P, 0, None), sumsq(P, -4, P, 1, None),
           sumsq(ODD4, n, P, k, None), sumsq(ODD8, n, P, k, None), sumsq(P, n, ODD4, k, None),
           sumsq(P, n, P, k - 1, None), sumsq(P, n, P, k + 1, None), sumsq(P, 2 * CH, P, 3, None),
           fin(None, k, P, P, P, P, None), fin(P, k, None, P, P, P, None), fin(P, k, P, None, P, P, None),
           fin(P, k, P, P, None, P, None), fin(P, k, P, P, P, None, None), fin(P, 0, P, P, P, P, None),
           fin(ODD4, k, P, P, P, P, None),
           upd(None, P, P, P, n, P, P, P, P, None), upd(P, None, P, P, n, P, P, P, P, None),
           upd(P, P, None, P, n, P, P, P, P, None), upd(P, P, P, None, n, P, P, P, P, None),
           upd(P, P, P, P, n, None, P, P, P, None), upd(P, P, P, P, n, P, None, P, P, None),
           upd(P, P, P, P, n, P, P, None, P, None), upd(P, P, P, P, n, P, P, P, None, None),
           upd(P, P, P, P, 0, P, P, P, P, None), upd(ODD4, P, P, P, n, P, P, P, P, None),
           upd(P, ODD8, P, P, n, P, P, P, P, None), upd(P, P, P, ODD4, n, P, P, P, P, None)]
    assert bad == [-1] * len(bad), bad
    assert _lib.raw["hrseg_grad_sumsq_chunks"](0) == -1 and _lib.raw["hrseg_grad_sumsq_chunks"](-1) == -1
    assert sumsq(P, n, P, k - 1, None) == -1 and "does not match" in _lib.last_error()
    with pytest.raises(RuntimeError):
        _lib.grad_sumsq_chunks(0)
