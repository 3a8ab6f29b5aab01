"""Online hard example mining on the GPU (csrc/loss_ohem.hip, the OHEM instances of csrc/loss.hip), in three kernel-level layers so
that a failure names its kernel, then end to end:

  1. hrseg_ohem_scores against the fp64 reference of tests/ohem_ref.py at the pointwise bar, -1 exactly at the pixels without a
     valid channel, NaN where a logit is NaN;
  2. hrseg_ohem_select is EXACT: for score buffers built on the host, lam_k (bit for bit; a NaN lam_k as NaN), n_candidates and
     n_kept are what torch.sort of the same fp32 values gives on the CPU, twice in a row on one workspace;
  3. hrseg_loss_partials_ohem / hrseg_loss_bwd_ohem against the fp64 reference evaluated WITH THE KEEP MASK THE GPU PRODUCED (its
     scores and record copied back), at the bars of tests/loss_options_ref.py -- on `saturated` by the rule of
     tests/test_loss_options_gpu.py::test_saturated_logits (CE relative to max(1, |ref|), dz within SATURATED_SLACK times the
     fp32 CPU evaluation's own distance, never asked below the bar): tests/test_ohem_cpu.py shows fp32 cannot hold the absolute
     bar where the CE reaches 60; the Dice term and the Dice part of dz carry the bits of the calls without OHEM.

End to end the GPU's keep mask is compared with the fp64 reference's own under the band and cap of ohem_ref.flips; with
ohem=None ops.loss_fwd / loss_bwd issue exactly today's calls and return their bits.  Run with -s for the worst distances."""
import math

import pytest
import torch

from tests import headloss_ref as R
from tests import loss_options_ref as LR
from tests import ohem_ref as OR

pytestmark = pytest.mark.gpu

WORST = {}
TIES = [0]


@pytest.fixture(scope="module")
def ops():
    from hrseg_amd import ops as o
    assert torch.cuda.is_available()
    yield o
    for group, d in WORST.items():
        print(f"\nworst vs fp64, {group}: " + ", ".join(f"{k} {v[0]:.2e} (bar {v[1]:.0e})" for k, v in d.items()))
    print(f"most exact-tie pixels kept by the GPU alone in one case: {TIES[0]}")


@pytest.fixture
def deterministic():
    from hrseg_amd import _lib
    _lib.set_deterministic(True)
    yield
    _lib.set_deterministic(False)


def check(group, name, d, bar):
    w = WORST.setdefault(group, {})
    w[name] = (max(w.get(name, (0.0, bar))[0], d), bar)
    assert d < bar, (group, name, d, bar)


def device_case(C, hw, B, pattern):
    x = LR.inputs(C, hw, B, pattern)
    return x["z"].cuda(), x["t"].cuda(), torch.tensor(x["w"]).cuda(), torch.tensor(LR.LOSS_UPSTREAM).cuda()


def record_of(rec):
    """device record -> (lam_k as a 0-dim fp32 CPU tensor, n_candidates, n_kept)"""
    r = rec.cpu()
    return r[:1].view(torch.float32)[0], int(r[1]), int(r[2])


def keep_of(q, lam, thresh):
    """the keep mask the kernels apply, from the scores and lam_k they stored (fp32, on the host)"""
    return (q != -1) & (torch.isnan(q) | (q < torch.tensor(OR.f32(thresh))) | (q <= lam))


# ------------------------------------------------------------------------------------------------ 1. scores
@pytest.mark.parametrize("C", OR.LOSS_C)
def test_scores_against_fp64(ops, C):
    for hw in OR.OHEM_HW:
        for B in OR.LOSS_B:
            for pattern in OR.OHEM_PATTERNS:
                x = LR.inputs(C, hw, B, pattern)
                ref = OR.scores(x["z"].double(), x["t"])
                q = ops.ohem_scores(x["z"].cuda(), x["t"].cuda()).cpu().reshape(B, hw)
                assert torch.equal(q == -1, ref == -1), (C, hw, B, pattern, "-1 exactly at the pixels without a valid channel")
                check("scores", "q", R.rel(q, ref), OR.BAR_POINT)


def test_scores_are_nan_where_a_logit_is_nan(ops):
    x = LR.inputs(5, 257, 3, "random_ignore")
    t = x["t"].clone()
    t[1, :, 0, 100] = torch.tensor([1.0, 0.0, 0.0, -1.0, 0.0])
    clean = ops.ohem_scores(x["z"].cuda(), t.cuda()).cpu().reshape(3, 257)
    for ch in (0, 1, 3):                # a target-1 channel, a target-0 channel, an ignored channel of that pixel
        z = x["z"].clone()
        z[1, ch, 0, 100] = float("nan")
        q = ops.ohem_scores(z.cuda(), t.cuda()).cpu().reshape(3, 257)
        assert math.isnan(float(q[1, 100])), ch
        q[1, 100] = clean[1, 100]
        assert torch.equal(q, clean), "and nowhere else"


# ------------------------------------------------------------------------------------------------ 2. selection
# 257: one element more than a block takes in one trip; 700: three blocks; 262145: one element more than the 1024-block grid takes
# in one trip (the grid-stride loop runs twice in one block); 1537600: batch 4 at 620 x 620
SELECT_SIZES = (1, 63, 64, 65, 255, 256, 257, 700, 262145, 1537600)
NEG_NAN = torch.tensor([-4194304], dtype=torch.int32).view(torch.float32)[0]          # 0xFFC00000: a NaN with the sign bit set


def _contents(n):
    """name -> fp32 score buffer of n elements: values in [0, 1], -1 for non-candidates, NaN"""
    g = torch.Generator().manual_seed(1000 + n % 9973)
    perm = torch.randperm(n, generator=g)
    out = {"uniform": torch.rand(n, generator=g), "all_equal": torch.full((n,), 0.37),
           "two_values": torch.where(torch.rand(n, generator=g) < 0.4, torch.tensor(0.25), torch.tensor(0.75))}
    lows, run = n // 4, n // 2          # a run of exact ties over the middle half of the ranks: it straddles rank N // 2
    tie = torch.cat([0.3 * torch.rand(lows, generator=g), torch.full((run,), 0.5), 0.6 + 0.4 * torch.rand(n - lows - run, generator=g)])
    out["tie_run"] = tie[perm]
    out["low_bits"] = (0.5 + (torch.arange(n) % 1024).float() * 2.0 ** -24)[perm]          # differ in the low 10 bits only
    out["high_bits"] = torch.pow(2.0, -torch.randint(0, 120, (n,), generator=g).float())      # differ in the exponent only
    special = torch.rand(n, generator=g)
    for i, v in enumerate((0.0, 1e-40, 1.0)):                                                 # 1e-40: a denormal
        if i < n:
            special[perm[i]] = v
    out["zero_denormal_one"] = special
    half = torch.rand(n, generator=g)
    half[torch.rand(n, generator=g) < 0.5] = -1.0
    out["half_ignored"] = half
    out["all_ignored"] = torch.full((n,), -1.0)
    nans = torch.rand(n, generator=g)
    nans[torch.rand(n, generator=g) < 0.2] = -1.0
    for i, v in enumerate((float("nan"), NEG_NAN, float("nan"))):
        if i < n:
            nans[perm[i]] = v
    out["nan_both_signs"] = nans
    return out


@pytest.mark.parametrize("n", SELECT_SIZES)
def test_selection_is_exact(ops, n):
    from hrseg_amd import _lib
    ws = torch.empty(_lib.ohem_workspace_bytes() // 4, dtype=torch.int32).cuda()
    for name, q in _contents(n).items():
        assert q.dtype == torch.float32 and q.numel() == n
        dq = q.cuda()
        ranked = torch.sort(q[q != -1]).values
        N = ranked.numel()
        for min_kept in sorted({0, 1, max(N - 1, 0), N, N + 1, N // 2, 10 ** 9}):
            for thresh in (0.0, 0.5):
                lam, n_cand, keep = OR.select(q, thresh, min_kept, ranked)
                first = ops.ohem_select(dq, thresh, min_kept, workspace=ws).cpu()
                again = ops.ohem_select(dq, thresh, min_kept, workspace=ws).cpu()          # (the workspace is dirty now)
                assert torch.equal(first, again), (n, name, min_kept, thresh)
                got, got_n, got_kept = record_of(first)
                assert int(first[3]) == 0
                assert got_n == n_cand == N, (n, name, min_kept, thresh)
                if math.isnan(float(lam)):
                    assert math.isnan(float(got)), (n, name, min_kept, thresh)
                else:
                    assert got.view(torch.int32).item() == lam.view(torch.int32).item(), (n, name, min_kept, thresh, float(got), float(lam))
                assert got_kept == int(keep.sum()), (n, name, min_kept, thresh)
                if not bool(torch.isnan(q).any()):
                    assert got_kept >= min(min_kept, N)


# ------------------------------------------------------------------------------------------------ 3. masked loss
@pytest.mark.parametrize("C", OR.LOSS_C)
def test_masked_loss_against_fp64_with_the_gpu_mask(ops, C):
    for hw in OR.OHEM_HW:
        for B in OR.LOSS_B:
            for pattern in OR.OHEM_PATTERNS:
                z, t, w, up = device_case(C, hw, B, pattern)
                x = LR.inputs(C, hw, B, pattern)
                q64 = OR.scores(x["z"].double(), x["t"])
                sat = pattern == LR.SATURATED
                group = "masked loss, saturated" if sat else "masked loss"
                for pair in OR.ohem_pairs(hw):
                    lam64, _, keep64 = OR.select(q64, *pair)
                    for gamma in OR.OHEM_GAMMAS:
                        case = (C, hw, B, pattern, pair, gamma)
                        opt = LR.options_f32(OR.options(gamma))
                        out, coef, state = ops.loss_fwd(z, t, w, None if gamma == 0.0 else opt, ohem=pair)
                        dz = ops.loss_bwd(z, t, coef, up, options=None if gamma == 0.0 else opt, ohem=state)
                        q, (lam, n_cand, n_kept) = state.q.cpu().reshape(B, hw), record_of(state.record)
                        keep = keep_of(q, lam, pair[0])
                        assert n_cand == int((q != -1).sum()) and n_kept == int(keep.sum()), case
                        assert n_kept >= min(pair[1], n_cand), case
                        # end to end: the GPU's mask against the fp64 reference's own selection
                        outside, plain, tie = OR.flips(keep, q, lam, keep64, q64, lam64, pair[0])
                        assert OR.flips_ok(outside, plain, tie), (case, outside, plain, tie)
                        TIES[0] = max(TIES[0], tie)
                        # the loss kernels against fp64 under the GPU's mask
                        ref = OR.run(*case, torch.float64, keep=keep)
                        out = out.cpu()
                        assert float(out[2]) == ref["nvalid"], case
                        check(group, "dice", R.absdiff(out[1], ref["dice"]), OR.LOSS_BARS["dice"])
                        scale = float(ref["dz"].abs().max()) or 1.0
                        base = scale * torch.randn(z.shape, generator=torch.Generator().manual_seed(3))
                        acc = ops.loss_bwd(z, t, coef, up, dz=base.cuda(), accumulate=True, options=None if gamma == 0.0 else opt, ohem=state)
                        acc = acc.cpu().double() - base.double()
                        if not sat:
                            check(group, "ce", R.absdiff(out[0], ref["ce"]), OR.LOSS_BARS["ce"])
                            check(group, "dz", R.rel(dz, ref["dz"]), OR.LOSS_BARS["dz"])
                            check(group, "dz", R.rel(acc, ref["dz"]), OR.LOSS_BARS["dz"])
                        else:
                            assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(dz).all()), case
                            check(group, "ce", R.absdiff(out[0], ref["ce"]) / max(1.0, abs(float(ref["ce"]))), OR.LOSS_BARS["ce"])
                            yard = R.rel(OR.run(*case, torch.float32, keep=keep)["dz"], ref["dz"])
                            bar = max(LR.SATURATED_SLACK * yard, OR.LOSS_BARS["dz"])
                            assert R.rel(dz, ref["dz"]) <= bar and R.rel(acc, ref["dz"]) <= bar, (case, R.rel(dz, ref["dz"]), yard, bar)


@pytest.mark.parametrize("C", (4, 9))
def test_dice_term_carries_the_bits_of_the_calls_without_ohem(ops, deterministic, C):
    """(deterministic mode: one adder per image, so that two runs of ONE entry point agree bit for bit to begin with)"""
    dice_only = torch.tensor([0.0, LR.LOSS_UPSTREAM[1], 0.0]).cuda()
    for hw in (257, 5000):
        for pattern in ("random_ignore", "item_ignored", LR.SATURATED):
            z, t, w, _ = device_case(C, hw, 3, pattern)
            for gamma in OR.OHEM_GAMMAS:
                opt = None if gamma == 0.0 else LR.options_f32(OR.options(gamma))
                out0, coef0 = ops.loss_fwd(z, t, w, opt)
                for pair in OR.ohem_pairs(hw):
                    out1, coef1, state = ops.loss_fwd(z, t, w, opt, ohem=pair)
                    assert torch.equal(out0[1:], out1[1:]), (C, hw, pattern, gamma, pair)
                    assert torch.equal(coef0.reshape(-1, 4)[:, 1:], coef1.reshape(-1, 4)[:, 1:])
                    assert torch.equal(ops.loss_bwd(z, t, coef0, dice_only, options=opt),
                                       ops.loss_bwd(z, t, coef1, dice_only, options=opt, ohem=state)), (C, hw, pattern, gamma, pair)


@pytest.mark.parametrize("gamma", OR.OHEM_GAMMAS)
def test_min_kept_beyond_the_candidates_is_the_plain_loss(ops, gamma):
    for C, hw, B, pattern in ((5, 257, 3, "random_ignore"), (4, 5000, 1, "no_ignore"), (9, 256, 3, "plane_ignored"), (16, 255, 3, "zero_weight")):
        z, t, w, up = device_case(C, hw, B, pattern)
        opt = None if gamma == 0.0 else LR.options_f32(OR.options(gamma))
        ref = LR.run(C, hw, B, pattern, OR.options(gamma), torch.float64)
        out, coef, state = ops.loss_fwd(z, t, w, opt, ohem=(0.0, 10 ** 9))
        _, n_cand, n_kept = record_of(state.record)
        assert n_kept == n_cand
        assert R.absdiff(out[0], ref["ce"]) < OR.LOSS_BARS["ce"] and R.absdiff(out[1], ref["dice"]) < OR.LOSS_BARS["dice"]
        assert R.rel(ops.loss_bwd(z, t, coef, up, options=opt, ohem=state), ref["dz"]) < OR.LOSS_BARS["dz"]


@pytest.mark.parametrize("gamma", OR.OHEM_GAMMAS)
def test_nothing_kept_is_the_constant_one_without_ce_gradient(ops, gamma):
    ce_only = torch.tensor([LR.LOSS_UPSTREAM[0], 0.0, 0.0]).cuda()
    for C, hw, B, pattern in ((5, 257, 3, "random_ignore"), (4, 5000, 1, "no_ignore"), (16, 256, 3, "item_ignored")):
        z, t, w, _ = device_case(C, hw, B, pattern)
        opt = None if gamma == 0.0 else LR.options_f32(OR.options(gamma))
        out, coef, state = ops.loss_fwd(z, t, w, opt, ohem=(0.0, 0))
        lam, n_cand, n_kept = record_of(state.record)
        assert float(lam) == -1.0 and n_kept == 0 and n_cand > 0
        assert float(out[0]) == 1.0
        assert not bool(ops.loss_bwd(z, t, coef, ce_only, options=opt, ohem=state).any())


@pytest.mark.parametrize("gamma", OR.OHEM_GAMMAS)
def test_a_nan_logit_is_kept_and_stays_loud(ops, gamma):
    z, t, w, up = device_case(5, 257, 3, "random_ignore")
    t[1, :, 0, 100] = torch.tensor([1.0, 0.0, 0.0, -1.0, 0.0]).cuda()
    opt = None if gamma == 0.0 else LR.options_f32(OR.options(gamma))
    for ch in (0, 1, 3):                # a target-1 channel, a target-0 channel, an ignored channel of that pixel
        zn = z.clone()
        zn[1, ch, 0, 100] = float("nan")
        out, coef, state = ops.loss_fwd(zn, t, w, opt, ohem=(0.0, 1))
        q = state.q.cpu()
        lam, _, n_kept = record_of(state.record)
        assert math.isnan(float(q[257 + 100])) and n_kept == int((q == lam).sum()) + 1, ch
        assert bool(torch.isnan(out[0])), (ch, out)
        dz = ops.loss_bwd(zn, t, coef, up, options=opt, ohem=state)
        assert bool(torch.isnan(dz[1, :, 0, 100]).all()), ch


# ------------------------------------------------------------------------------------------------ OHEM off
def test_without_ohem_the_calls_and_the_bits_are_todays(ops, deterministic):
    from hrseg_amd import _lib
    from hrseg_amd._lib import call, ptr
    z, t, w, up = device_case(5, 5000, 3, "random_ignore")
    B, C, hw = 3, 5, 5000
    _lib.launch_count("ohem", reset=True)
    for opt, names in ((None, ("hrseg_loss_partials", "hrseg_loss_finalize", "hrseg_loss_bwd")),
                       ((2.0, 1.0, 0.3, 0.7), ("hrseg_loss_partials_opt", "hrseg_loss_finalize_opt", "hrseg_loss_bwd_opt"))):
        with _lib.Tape() as tape:
            out, coef = ops.loss_fwd(z, t, w, opt, ohem=None)
            dz = ops.loss_bwd(z, t, coef, up, options=opt, ohem=None)
        assert tuple(e[1].__name__ for e in tape.entries) == names and tape.calls == 3
        part = torch.empty(B * C * 5, dtype=torch.float64).cuda()
        out0, coef0, dz0 = torch.empty(3).cuda(), torch.empty(B * C * 4).cuda(), torch.empty_like(z)
        if opt is None:
            call(names[0], ptr(z), ptr(t), ptr(part), B, C, hw)
            call(names[1], ptr(part), ptr(w), B, C, ptr(out0), ptr(coef0))
            call(names[2], ptr(z), ptr(t), ptr(coef0), ptr(up), ptr(dz0), 0, B, C, hw)
        else:
            call(names[0], ptr(z), ptr(t), ptr(part), B, C, hw, opt[0])
            call(names[1], ptr(part), ptr(w), B, C, opt[1], opt[2], opt[3], ptr(out0), ptr(coef0))
            call(names[2], ptr(z), ptr(t), ptr(coef0), ptr(up), ptr(dz0), 0, B, C, hw, opt[0])
        assert torch.equal(out, out0) and torch.equal(coef, coef0) and torch.equal(dz, dz0)
    assert _lib.launch_count("ohem") == 0, "no OHEM launch without OHEM"
    with _lib.Tape() as tape:
        out, coef, state = ops.loss_fwd(z, t, w, None, ohem=(0.7, 100))
        ops.loss_bwd(z, t, coef, up, ohem=state)
    assert tuple(e[1].__name__ for e in tape.entries) == ("hrseg_ohem_scores", "hrseg_ohem_select", "hrseg_loss_partials_ohem",
                                                          "hrseg_loss_finalize", "hrseg_loss_bwd_ohem")
    assert _lib.launch_count("ohem") == 1 + 7 + 1 + 1


def test_loss_objects_with_ohem(ops):
    """the public surface: CrossEntropyLoss(ohem_thresh, ohem_min_kept) through autograd, last_ohem without a sync"""
    from hrseg_amd.Metrics import losses as PL
    x = LR.inputs(5, 5000, 3, "random_ignore")
    pair = (0.7, 2000)
    ce_fn = PL.CrossEntropyLoss(ohem_thresh=pair[0], ohem_min_kept=pair[1])
    z = x["z"].cuda().requires_grad_(True)
    ce = ce_fn(z, x["t"].cuda(), logits_input=True, class_weight=x["w"])
    (LR.LOSS_UPSTREAM[0] * ce).backward()
    lam, n_cand, n_kept = record_of(ce_fn.last_ohem)
    assert n_kept >= min(pair[1], n_cand) and ce_fn.kept_fraction() == n_kept / n_cand
    q = ops.ohem_scores(x["z"].cuda(), x["t"].cuda()).cpu().reshape(3, 5000)
    ref = OR.run_parts(5, 5000, 3, "random_ignore", pair, 0.0, torch.float64, keep=keep_of(q, lam, pair[0]))
    assert R.rel(z.grad, ref["ce"]) < OR.LOSS_BARS["dz"]
    plain = PL.CrossEntropyLoss()(x["z"].cuda(), x["t"].cuda(), logits_input=True, class_weight=x["w"])
    assert abs(float(ce.detach()) - float(plain)) > 1e-3, "the selection changes the CE"
    res = PL.fused_ce_dice(x["z"].cuda(), x["t"].cuda(), x["w"], ohem=pair)
    assert abs(float(res[0]) - float(ce.detach())) < OR.LOSS_BARS["ce"]
