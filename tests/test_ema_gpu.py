"""The weight-average kernels of csrc/optim.hip -- hrseg_adamw_dev_ema, hrseg_adamw_dev_clip_ema, hrseg_ema_update,
hrseg_swap -- against the entry points they extend (bitwise) and tests/ema_ref.py (the derived bar), at the sizes of
ema_ref.SIZES: the scalar tail alone, one 16-byte group, groups plus tail, and the size at which the cap on blocks sends threads
round the grid-stride loop a second time.  "Bitwise" means torch.equal.  The fp64 reference is evaluated on the device that
holds the kernel's own p' and previous e."""
import ctypes
import math

import pytest
import torch

from tests import ema_ref as E
from tests import headloss_ref as R

pytestmark = pytest.mark.gpu

INF = math.inf
SIZES = pytest.mark.parametrize("n", E.SIZES, ids=E.SIZE_IDS)


@pytest.fixture(scope="module")
def ops():
    from hrseg_amd import ops as o
    assert torch.cuda.is_available()
    return o


def _hyper(lr=1e-3, wd=0.01, gscale=R.ADAMW_GSCALE):
    return torch.tensor([lr, R.ADAMW_BETA1, R.ADAMW_BETA2, R.ADAMW_EPS, wd, gscale], dtype=torch.float32, device="cuda")


def _clipcfg(max_norm, skip):
    return torch.tensor([max_norm, float(skip)], dtype=torch.float32, device="cuda")


def _state(k):
    """AdamW's device state after k steps"""
    return torch.tensor(R.adamw_state(k) if k else [0.0, 0.0, 0.0], dtype=torch.float32, device="cuda")


def _dev(x):
    return {k: v.cuda() for k, v in x.items()}


def _verdict(ops, g, hyper, cfg, state, clip):
    ops.grad_clip_finalize(ops.grad_sumsq(g), hyper, cfg, state, clip)


def _check_e(got, e_prev, p_new, d, warmup, s, s0, what):
    use = E.bar_use(got, e_prev, p_new, d, warmup, s, s0)
    print(f"{what}: e uses {use:.3f} of the bar")
    assert use <= 1.0, (what, use)
    assert not torch.equal(got, e_prev)


# ================================================================================================ fused with adamw_dev
@SIZES
def test_adamw_dev_ema_is_adamw_dev_bitwise_and_e_within_the_bar(ops, n):
    x = _dev(E.inputs(n))
    hyper = _hyper()
    for d, warmup, s0, k in ((0.9, False, 0, 0), (0.999, True, 2, 6)):
        cfg = E.emacfg(d, warmup, s0, "cuda")
        a, b = {q: x[q].clone() for q in "pmv"}, {q: x[q].clone() for q in "pmve"}
        sa, sb = _state(k), _state(k)
        ops.adamw_dev(a["p"], x["g"], a["m"], a["v"], hyper, sa)
        ops.adamw_dev_ema(b["p"], x["g"], b["m"], b["v"], b["e"], hyper, sb, cfg)
        for q in "pmv":
            assert torch.equal(a[q], b[q]), (n, d, q)
        assert torch.equal(sa, sb) and sb[0].item() == k + 1
        assert not torch.equal(b["p"], x["p"])
        _check_e(b["e"], x["e"], b["p"], d, warmup, k + 1, s0, f"n={n} d={d} warmup={warmup}")


# ================================================================================================ fused with adamw_dev_clip
@pytest.mark.parametrize("factor", [INF, 0.5], ids=["coef1", "coef_half"])
@SIZES
def test_adamw_dev_clip_ema_is_adamw_dev_clip_bitwise_and_e_within_the_bar(ops, n, factor):
    x = _dev(E.inputs(n))
    hyper = _hyper()
    d, warmup, s0, k = 0.99, True, 1, 4
    cfg = E.emacfg(d, warmup, s0, "cuda")
    probe = torch.zeros(4, device="cuda")
    _verdict(ops, x["g"], hyper, _clipcfg(INF, True), _state(k), probe)
    ccfg = _clipcfg(INF if factor == INF else R.f32(factor * probe[0].item()), True)
    a, b = {q: x[q].clone() for q in "pmv"}, {q: x[q].clone() for q in "pmve"}
    sa, sb, ca, cb = _state(k), _state(k), torch.zeros(4, device="cuda"), torch.zeros(4, device="cuda")
    _verdict(ops, x["g"], hyper, ccfg, sa, ca)
    ops.adamw_dev_clip(a["p"], x["g"], a["m"], a["v"], hyper, sa, ccfg, ca)
    _verdict(ops, x["g"], hyper, ccfg, sb, cb)
    ops.adamw_dev_clip_ema(b["p"], x["g"], b["m"], b["v"], b["e"], hyper, sb, ccfg, cb, cfg)
    coef = cb[1].item()
    assert (coef == 1.0) if factor == INF else (0.49 < coef < 0.51), coef
    for q in "pmv":
        assert torch.equal(a[q], b[q]), (n, factor, q)
    assert torch.equal(sa, sb) and torch.equal(ca, cb) and sb[0].item() == k + 1
    _check_e(b["e"], x["e"], b["p"], d, warmup, k + 1, s0, f"n={n} coef={coef:.3f}")


# ================================================================================================ fused == unfused
@SIZES
def test_fused_e_is_adamw_dev_then_ema_update_bitwise(ops, n):
    x = _dev(E.inputs(n))
    hyper = _hyper()
    for d, warmup, s0, k in ((0.9, False, 0, 0), (0.5, True, 5, 9), (0.9999, True, 0, 3)):
        cfg = E.emacfg(d, warmup, s0, "cuda")
        a, b, c = ({q: x[q].clone() for q in "pmve"} for _ in range(3))
        sa, sb, sc, clip = _state(k), _state(k), _state(k), torch.zeros(4, device="cuda")
        ops.adamw_dev_ema(a["p"], x["g"], a["m"], a["v"], a["e"], hyper, sa, cfg)
        ops.adamw_dev(b["p"], x["g"], b["m"], b["v"], hyper, sb)
        ops.ema_update(b["e"], b["p"], sb, cfg)
        _verdict(ops, x["g"], hyper, _clipcfg(INF, True), sc, clip)
        ops.adamw_dev_clip_ema(c["p"], x["g"], c["m"], c["v"], c["e"], hyper, sc, _clipcfg(INF, True), clip, cfg)
        assert torch.equal(a["p"], b["p"]) and torch.equal(a["p"], c["p"])
        assert torch.equal(a["e"], b["e"]), (n, d, "fused vs adamw_dev + ema_update")
        assert torch.equal(a["e"], c["e"]), (n, d, "the two fused kernels")
        assert not torch.equal(a["e"], x["e"])


# ================================================================================================ void step
@SIZES
def test_void_step_leaves_everything_alone_and_the_warmup_count_too(ops, n):
    x = E.inputs(n)
    g0 = x["g"]
    g1 = 4.0 * torch.randn(n, generator=torch.Generator().manual_seed(n))
    bad = g1.clone()
    bad[n // 2] = math.nan
    d, s0 = 0.5, 0
    hyper, ccfg, cfg = _hyper(), _clipcfg(INF, True), E.emacfg(d, True, s0, "cuda")

    def run(grads):
        t = _dev({q: x[q] for q in "pmve"})
        state, clip, trace = _state(0), torch.zeros(4, device="cuda"), []
        for g in grads:
            before = [v.clone() for v in (t["p"], t["m"], t["v"], t["e"], state)]
            _verdict(ops, g.cuda(), hyper, ccfg, state, clip)
            ops.adamw_dev_clip_ema(t["p"], g.cuda(), t["m"], t["v"], t["e"], hyper, state, ccfg, clip, cfg)
            trace.append((before, [v.clone() for v in (t["p"], t["m"], t["v"], t["e"], state)], clip.clone()))
        return trace

    with_void, without = run([g0, bad, g1]), run([g0, g1])
    before, after, clip = with_void[1]
    assert clip[2].item() == 0.0 and clip[3].item() == 1.0
    assert all(torch.equal(a, b) for a, b in zip(before, after))                  # p, m, v, e, state: bitwise untouched
    # the step after it is the step it would have been: t = 1, eff = min(0.5, 2/11), not t = 2
    assert all(torch.equal(a, b) for a, b in zip(with_void[2][1], without[1][1]))
    e_prev, (p_new, _, _, e_new, state) = with_void[2][0][3], with_void[2][1]
    assert state[0].item() == 2.0
    _check_e(e_new, e_prev, p_new, d, True, 2, s0, f"n={n} after the void step")
    assert E.bar_use(e_new, e_prev, p_new, d, True, 3, s0) > 1.0                  # (the bar tells t = 1 from t = 2)


# ================================================================================================ warm-up
@SIZES
def test_warmup_sequence_matches_the_reference_step_by_step(ops, n):
    c = E.WARMUP_CASE
    x = _dev(E.inputs(n))
    hyper, cfg = _hyper(), E.emacfg(c["d"], True, c["s0"], "cuda")
    t = {q: x[q].clone() for q in "pmve"}
    state = _state(c["s0"])
    gen = torch.Generator(device="cuda").manual_seed(1)
    for k in range(c["steps"]):
        g = 4.0 * torch.randn(n, generator=gen, device="cuda")
        e_prev = t["e"].clone()
        ops.adamw_dev_ema(t["p"], g, t["m"], t["v"], t["e"], hyper, state, cfg)
        s = c["s0"] + 1 + k
        assert state[0].item() == s
        assert E.eff(c["d"], True, s, c["s0"]) == pytest.approx(E.WARMUP_EFF[k], rel=1e-15)
        _check_e(t["e"], e_prev, t["p"], c["d"], True, s, c["s0"], f"update {k}: eff {E.WARMUP_EFF[k]:.4f}")
        if n >= 1023 and k + 1 < c["steps"] and E.WARMUP_EFF[k + 1] != E.WARMUP_EFF[k]:     # a count off by one does not pass
            assert E.bar_use(t["e"], e_prev, t["p"], c["d"], True, s + 1, c["s0"]) > 1.0
    # warm-up off: the decay from the first update on
    cfg[1] = 0.0
    e_prev = t["e"].clone()
    ops.ema_update(t["e"], t["p"], state, cfg)
    _check_e(t["e"], e_prev, t["p"], c["d"], False, 0, 0, "warm-up off")


# ================================================================================================ swap
@SIZES
def test_swap_exchanges_and_restores_bitwise(ops, n):
    gen = torch.Generator(device="cuda").manual_seed(n % 1000)
    # room on both sides of either buffer: the kernel writes n elements and not one more
    store = torch.randn(2 * n + 24, generator=gen, device="cuda")
    keep = store.clone()
    a, b = store[4:4 + n], store[n + 12 - n % 4:2 * n + 12 - n % 4]
    assert a.data_ptr() % 16 == 0 and b.data_ptr() % 16 == 0 and a.data_ptr() + 4 * n <= b.data_ptr()
    a0, b0 = a.clone(), b.clone()
    assert not torch.equal(a0, b0)
    ops.swap(a, b)
    assert torch.equal(a, b0) and torch.equal(b, a0)
    ops.swap(a, b)
    assert torch.equal(store, keep)


# ================================================================================================ argument checks
def test_bad_arguments_are_refused_before_any_launch():
    """placeholder pointers, never dereferenced: every call below must return -1 from the host-side checks (no GPU needed)"""
    from hrseg_amd import _lib
    P, G, M, V, Ee, H, S, C = (ctypes.c_void_p(4096 * (i + 1)) for i in range(8))
    ODD4, ODD8 = ctypes.c_void_p(65536 + 4), ctypes.c_void_p(65536 + 8)
    ema, cema, upd, swap = (_lib._fn[k] for k in ("hrseg_adamw_dev_ema", "hrseg_adamw_dev_clip_ema", "hrseg_ema_update",
                                                  "hrseg_swap"))
    n = 1029
    good_ema, good_cema = [P, G, M, V, Ee, n, H, S, C], [P, G, M, V, Ee, n, H, S, C, C, C]
    bad = []
    for fn, good in ((ema, good_ema), (cema, good_cema), (upd, [Ee, P, n, S, C]), (swap, [P, G, n])):
        for i, arg in enumerate(good):
            broken = list(good)
            broken[i] = 0 if isinstance(arg, int) else None                        # n = 0 / a null pointer
            bad.append(fn(*broken, None))
    for fn, good, e_at in ((ema, good_ema, 4), (cema, good_cema, 4), (upd, [Ee, P, n, S, C], 0)):
        for odd in (ODD4, ODD8):
            broken = list(good)
            broken[e_at] = odd                                                     # a misaligned shadow
            bad.append(fn(*broken, None))
            assert "16-byte aligned" in _lib.last_error()
        broken = list(good)
        broken[e_at] = P                                                           # the shadow is the parameter buffer
        bad.append(fn(*broken, None))
    bad += [ema(ODD4, G, M, V, Ee, n, H, S, C, None), cema(P, G, M, ODD8, Ee, n, H, S, C, C, C, None), upd(Ee, ODD4, n, S, C, None),
            ema(P, G, M, V, Ee, -3, H, S, C, None), swap(ODD4, G, n, None), swap(P, ODD8, n, None), swap(P, P, n, None),
            swap(P, ctypes.c_void_p(4096 + 16), n, None), swap(P, G, -1, None)]
    assert bad == [-1] * len(bad), bad
