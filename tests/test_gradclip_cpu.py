"""tests/gradclip_ref.py against the real thing on the CPU in fp64: torch.nn.utils.clip_grad_norm_ followed by
torch.optim.AdamW.step() over several tensors that the reference treats as one flat buffer; the skip rule; and
max_norm = inf reproducing the unclipped reference exactly.  No GPU."""
import math

import torch

from tests import gradclip_ref as G
from tests import headloss_ref as R

SHAPES = [(7, 3, 3, 3), (7,), (5, 7), (1,), (13, 2)]
LRS = R.ADAMW_LRS
GSCALE = 0.25


def _flat(ts):
    return torch.cat([t.reshape(-1) for t in ts])


def test_reference_is_clip_grad_norm_then_torch_adamw():
    gen = torch.Generator().manual_seed(11)
    p0 = [torch.randn(s, generator=gen) for s in SHAPES]                       # fp32 values, evaluated in fp64
    grads = [[4.0 * torch.randn(s, generator=gen) for s in SHAPES] for _ in LRS]
    norms = [G.verdict(_flat(g), GSCALE)["norm"] for g in grads]
    # thresholds around the norms: clip hard, far above, just below, just above, clip
    max_norms = [0.3 * norms[0], 50.0 * norms[1], 0.99 * norms[2], 1.01 * norms[3], 0.5 * norms[4]]
    for wd in R.ADAMW_WDS:
        params = [torch.nn.Parameter(p.double().clone()) for p in p0]
        opt = torch.optim.AdamW(params, lr=LRS[0], betas=(R.ADAMW_BETA1, R.ADAMW_BETA2), eps=R.ADAMW_EPS,
                                weight_decay=G.f32(wd))
        ref = G.Run(_flat(p0), wd, torch.float64, GSCALE)
        clipped = []
        for k, lr in enumerate(LRS):
            opt.param_groups[0]["lr"] = G.f32(lr)
            for p, g in zip(params, grads[k]):
                p.grad = G.f32(GSCALE) * g.double()
            total = torch.nn.utils.clip_grad_norm_(params, G.f32(max_norms[k]))
            opt.step()
            vd = ref.step(_flat(grads[k]), lr, max_norms[k])
            clipped.append(vd["coef"] < 1.0)
            assert abs(float(total) - vd["norm"]) <= 1e-12 * vd["norm"]
            want_coef = min(1.0, G.f32(max_norms[k]) / (float(total) + 1e-6))
            assert abs(vd["coef"] - want_coef) <= 1e-12 and abs(vd["coef32"] - want_coef) <= 6e-8 * want_coef
            got = {"p": _flat([p.data for p in params]), "m": _flat([opt.state[p]["exp_avg"] for p in params]),
                   "v": _flat([opt.state[p]["exp_avg_sq"] for p in params])}
            for name, t in ref.tensors().items():
                assert R.rel(t, got[name]) < R.BAR_ADAMW, (wd, k, name, R.rel(t, got[name]))
        assert clipped == [True, False, True, False, True]      # both kinds occur
        assert ref.steps == len(LRS) and ref.skipped == 0


def test_max_norm_inf_is_the_unclipped_reference_exactly():
    for n in (1, 5, 1023):
        x = R.adamw_inputs(n)
        for wd in R.ADAMW_WDS:
            for dtype in (torch.float64, torch.float32):
                want = R.adamw_run(x, wd, dtype)
                got = G.run(x["p"], x["grads"], R.ADAMW_LRS, wd, dtype, max_norms=None, skip=True)
                assert all(vd["coef32"] == 1.0 and vd["finite"] for vd in got.log)
                for name, t in got.tensors().items():
                    assert torch.equal(t, want[name]), (n, wd, dtype, name)


def _poisoned(g, kind):
    g = g.clone()
    if kind == "nan":
        g[-1] = math.nan
    elif kind == "inf":
        g[len(g) // 2] = math.inf
    else:
        g[1], g[len(g) - 2] = math.inf, -math.inf
    return g


def test_skip_rule_and_resumed_bias_correction():
    x = R.adamw_inputs(1023)
    g0, g1, g2 = x["grads"][:3]
    for kind in ("nan", "inf", "inf_pair"):
        bad = _poisoned(g1, kind)
        vd = G.verdict(bad, 0.25, 1.0)
        assert not vd["finite"] and (math.isnan(vd["norm"]) or math.isinf(vd["norm"]))
        assert G.verdict(bad, 0.25)["finite"] is False and G.verdict(g1, math.inf)["finite"] is False
        r = G.Run(x["p"], 0.01, torch.float64)
        r.step(g0, 1e-3, 3.0, skip=True)
        before = {k: t.clone() for k, t in r.tensors().items()}
        r.step(bad, 1e-3, 3.0, skip=True)
        assert r.steps == 1 and r.skipped == 1 and r.state() == R.adamw_state(1)
        assert all(torch.equal(t, before[k]) for k, t in r.tensors().items())          # the void step touched nothing
        r.step(g2, 5e-4, 3.0, skip=True)
        clean = G.run(x["p"], [g0, g2], [1e-3, 5e-4], 0.01, torch.float64, max_norms=[3.0, 3.0], skip=True)
        assert r.steps == clean.steps == 2 and r.state() == R.adamw_state(2)          # bias correction resumed at step 2
        assert all(torch.equal(t, clean.tensors()[k]) for k, t in r.tensors().items())
        # skip clear: the formula is applied with no special case and the poison reaches the state
        loud = G.Run(x["p"], 0.01, torch.float64)
        loud.step(bad, 1e-3, 3.0, skip=False)
        assert loud.steps == 1 and loud.skipped == 0 and not bool(torch.isfinite(loud.m).all())


def test_fp64_sum_has_the_range_fp32_lacks():
    for mag in (1e20, 1e-30):
        g = torch.full((1000,), mag, dtype=torch.float32)
        assert not (0.0 < float((g * g).sum()) < math.inf)                 # fp32 squares overflow / vanish
        vd = G.verdict(g)
        assert vd["finite"] and abs(vd["norm"] - float(g[0]) * math.sqrt(1000.0)) <= 1e-12 * vd["norm"]
