"""The tree distillation kernels (csrc/distill.hip) against the float64 reference of tests/distill_ref.py within its derived
bounds, the exact facts the header states (include/hrseg.h, "tree distillation"), non-finite values, the deterministic knob, and
the module and train-step layers above them."""
import argparse
import os
import re

import pytest
import torch

from tests import distill_ref as R
from tests.helpers import CSRC, load_tree

pytestmark = pytest.mark.gpu


def _run(c, z=None, u=None, wprev="case", pw="case", T=None, thresh=None, dz0=None):
    """both entry points on a case's tensors (or replacements) -> (out [G,3] float64, dz, accumulated dz or None), on the host"""
    from hrseg_amd import ops
    B, H, W = c["B"], c["H"], c["W"]

    def dev(t, ch=None):
        return None if t is None else t.reshape((B, H, W) if ch is None else (B, ch, H, W)).contiguous().cuda()
    z = dev(c["z"] if z is None else z, c["C"])
    u = dev(c["u"] if u is None else u, c["C"])
    wprev = c["wprev"] if isinstance(wprev, str) else wprev
    wprev = None if wprev is None else dev(wprev, wprev.shape[1])
    pw = dev(c["pw"] if isinstance(pw, str) else pw)
    beta = c["beta"] if T is None else 1.0 / T
    thresh = c["thresh"] if thresh is None else thresh
    g = torch.tensor([c["g"]], dtype=torch.float32, device="cuda")
    out = ops.tree_kl_fwd(z, u, wprev, pw, beta, thresh, c["gp"], c["gs"])
    dz = ops.tree_kl_bwd(z, u, wprev, pw, beta, thresh, g, c["scale"], c["gp"], c["gs"])
    acc = None
    if dz0 is not None:
        acc = dev(dz0, c["C"]).clone()
        ops.tree_kl_bwd(z, u, wprev, pw, beta, thresh, g, c["scale"], c["gp"], c["gs"], dz=acc, accumulate=True)
        acc = acc.cpu().reshape(B, c["C"], -1)
    return out.cpu(), dz.cpu().reshape(B, c["C"], -1), acc


@pytest.fixture
def deterministic():
    from hrseg_amd import _lib
    _lib.set_deterministic(True)
    yield
    _lib.set_deterministic(False)


@pytest.mark.parametrize("name", list(R.CASES))
def test_case_against_the_reference(name):
    from hrseg_amd import _lib
    c, r = R.reference(name)
    _lib.launch_count("tree_kl", reset=True)
    out, dz, acc = _run(c, dz0=c["dz0"] if c["accumulate"] else None)
    assert _lib.launch_count("tree_kl") == (3 if c["accumulate"] else 2), "one launch per call"
    print(name, "out", out.tolist(), "ref", r["out"].tolist(), "value bound", r["value_bound"].tolist(),
          "max dz err", float((dz.double() - r["dz"]).abs().max()), "max dz bound", float(r["dz_bound"].max()))
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(dz).all())
    assert R.check_against(name, out, dz, acc) == []


def _dropped_mask(c, r):
    """[B,C,hw] bool: channels of the (pixel, group) pairs the reference drops"""
    m = torch.zeros(c["B"], c["C"], c["hw"], dtype=torch.bool)
    for gi, sl in enumerate(R.group_slices(c["gs"])):
        m[:, sl] = ~r["keep"][:, gi][:, None]
    return m


@pytest.mark.parametrize("name", ["c8_215_gated_T2_acc", "c4_22_big_gated_acc"])
def test_dropped_groups_write_zero_and_leave_an_accumulated_dz_bit_identical(name):
    c, r = R.reference(name)
    _, dz, acc = _run(c, dz0=c["dz0"])
    drop = _dropped_mask(c, r)
    assert 0.2 < float(drop.double().mean()) < 0.8
    assert bool((dz[drop] == 0).all()) and not bool(torch.signbit(dz[drop]).any())
    assert torch.equal(acc[drop].view(torch.int32), c["dz0"][drop].view(torch.int32))
    assert not torch.equal(acc[~drop], c["dz0"][~drop])


@pytest.mark.parametrize("name,T", [("c8_215_gated_T2_acc", 0.7), ("c16_flat", 0.7), ("c5_one_parent_T2", 1.0)])
def test_teacher_equal_to_student_gives_exactly_zero(name, T):
    """u == z: both sides run the same operations on the same bits, whatever the temperature (0.7: beta is no power of two)"""
    c, _ = R.reference(name)
    out, dz, _ = _run(c, u=c["z"], T=T, thresh=0.0)
    assert bool((out[:, 0] == 0).all()), out
    assert bool((dz == 0).all())
    assert bool((out[:, 2] == c["B"] * c["hw"]).all())


def test_groups_of_one_give_exactly_zero():
    c, _ = R.reference("c16_ones_gated_T2")
    for T in (0.7, 2.0):
        out, dz, _ = _run(c, T=T, thresh=0.0)
        assert bool((out[:, 0] == 0).all()) and bool((dz == 0).all())
        assert bool((out[:, 1] > 0).all())
    c, _ = R.reference("c6_123_gated_pwzeros")
    out, dz, _ = _run(c, T=0.7)
    assert float(out[0, 0]) == 0.0 and bool((dz[:, 0] == 0).all()) and float(out[1, 0]) > 0.0


@pytest.mark.parametrize("name", ["c8_215_gated_T2_acc", "c6_123_gated_pwzeros", "c9_gated_pw_T05"])
def test_thresh_zero_gives_the_bits_of_the_gated_instance_that_keeps_everything(deterministic, name):
    """thresh = 0 runs the instance without the gate; 1e-30 runs the gated one, and every conf of these cases is far above it"""
    c, _ = R.reference(name)
    a = _run(c, thresh=0.0, dz0=c["dz0"])
    b = _run(c, thresh=1e-30, dz0=c["dz0"])
    assert bool((a[0][:, 2] == c["B"] * c["hw"]).all())
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int64 if x.dtype == torch.float64 else torch.int32),
                           y.view(torch.int64 if y.dtype == torch.float64 else torch.int32))


def test_two_deterministic_runs_give_the_same_bytes(deterministic):
    c, _ = R.reference("c4_22_big_gated_acc")
    a, b = _run(c), _run(c)
    assert torch.equal(a[0].view(torch.int64), b[0].view(torch.int64))
    assert torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    assert R.check_against("c4_22_big_gated_acc", a[0], a[1]) == []


def _poisoned(name, side, value, thresh, zero_weight=True):
    """one logit of `side` replaced by `value` in group 2 (five channels) at (image 0, pixel 5), and a zero pixel weight there
    -> the case, the group's slice, what _run gives and what it gives on the clean tensors"""
    c, _ = R.reference(name)
    sl = R.group_slices(c["gs"])[2]
    t = c[side].clone()
    t[0, sl.start + 1, 5] = value
    pw = torch.ones(c["B"], c["hw"]) if c["pw"] is None else c["pw"].clone()
    if zero_weight:
        pw[0, 5] = 0.0
    return c, sl, _run(c, pw=pw, thresh=thresh, **{side: t}), _run(c, pw=pw, thresh=thresh)


@pytest.mark.parametrize("side", ["u", "z"])
@pytest.mark.parametrize("value", [float("nan"), float("inf")])
def test_a_nan_or_plus_inf_logit_shows_in_its_group_and_nowhere_else(side, value):
    """whatever m is (0 there): the group's first slot is NaN, dz is NaN on the group's channels at that pixel; the other groups'
    sums stay finite and every other dz element has the bits of the clean run.  A teacher NaN is kept by the gate as well."""
    for thresh in ((0.0, 0.6) if side == "u" else (0.0,)):
        c, sl, (out, dz, _), (_, dz0, _) = _poisoned("c8_215_gated_T2_acc", side, value, thresh)
        assert bool(torch.isnan(out[2, 0])), out
        assert bool(torch.isfinite(out[[0, 1]]).all()) and bool(torch.isfinite(out[2, 1:]).all())
        hit = torch.zeros_like(dz, dtype=torch.bool)
        hit[0, sl, 5] = True
        assert bool(torch.isnan(dz[hit]).all())
        assert torch.equal(dz[~hit].view(torch.int32), dz0[~hit].view(torch.int32))


def test_a_minus_inf_logit_gives_what_the_header_states():
    # teacher: q_c = 0 and lq_c = -Inf make the first slot NaN (0 * -Inf); dz stays finite
    c, sl, (out, dz, _), _ = _poisoned("c8_215_gated_T2_acc", "u", float("-inf"), 0.0, zero_weight=False)
    assert bool(torch.isnan(out[2, 0])) and bool(torch.isfinite(out[[0, 1]]).all()) and bool(torch.isfinite(dz).all())
    assert float(dz[0, sl.start + 1, 5]) >= 0.0          # q_j = 0 there: the element is w p_j
    # student: lp_c = -Inf against q_c > 0 is +Inf; dz stays finite
    c, sl, (out, dz, _), _ = _poisoned("c8_215_gated_T2_acc", "z", float("-inf"), 0.0, zero_weight=False)
    assert float(out[2, 0]) == float("inf") and bool(torch.isfinite(out[[0, 1]]).all()) and bool(torch.isfinite(dz).all())
    assert float(dz[0, sl.start + 1, 5]) <= 0.0          # p_j = 0 there: the element is -w q_j


# ----------------------------------------------------------------------------- the module and the train step
SIZE, BATCH = 32, 2


def _setup(ema=False):
    from hrseg_amd import train as PT
    from hrseg_amd.Metrics import losses as PL
    from hrseg_amd.Models import models as PM
    from hrseg_amd.utils import synth
    from hrseg_amd.utils.hierarchy import get_classes
    tree = load_tree("class_tree_tl.json")
    nc = get_classes(tree, full=True)
    args = argparse.Namespace(model_type=1, model_select=0, num_classes=nc, level_weights=synth.README_LEVEL_WEIGHTS_TL,
                              level0_pretrain_epochs=None, batch_size=BATCH)
    model = synth.fill_state_dict(PM.UNet(size=SIZE, n_channels=3, hierarchy=tree, model_type=1)).cuda()
    model.train()
    opt = PT.FusedAdamW(model, lr=[1e-3], **(dict(ema_decay=0.9) if ema else {}))
    fns = [[PL.CrossEntropyLoss(), PL.SoftDiceLoss(num_classes=n)] for n in nc]
    x, t = synth.synthetic_batch(tree, BATCH, SIZE, seed=3, hierarchical=True, blob=4)
    return model, opt, fns, args, tree, torch.from_numpy(x).cuda(), torch.from_numpy(t).cuda()


def _families():
    with open(os.path.join(CSRC, "runtime.h")) as f:
        return re.findall(r'^\s*X\([A-Z0-9_]+, "(\w+)", [01]\)', f.read(), re.M)


def test_module_on_a_models_logits_equals_the_reference_forward_and_backward():
    from hrseg_amd.Metrics import losses as PL
    model, _, _, args, tree, x, _ = _setup()
    with torch.no_grad():
        model.eval()
        tprobs, tlogits = model(x, type=1, hierarchy=tree)
        model.train()
        _, slogits = model(x, type=1, hierarchy=tree)
    slogits = [z.detach().clone().requires_grad_(True) for z in slogits]
    pw = (torch.rand(BATCH, SIZE, SIZE, generator=torch.Generator().manual_seed(2)) + 0.5).cuda()
    T, lw = [1.0, 2.0, 0.5, 1.0][:len(slogits)], [1.0, 0.5, 2.0, 1.5][:len(slogits)]
    d = PL.TreeDistillation.for_model(model, temperature=T, level_weights=lw)
    assert len(d.groups) == len(model.levels) and d.groups[0] is None
    loss = d(slogits, tlogits, tprobs, pw)
    assert loss.dim() == 0 and loss.dtype == torch.float32
    grads = torch.autograd.grad(loss, slogits)
    n = BATCH * SIZE * SIZE
    flat = lambda t: t.detach().cpu().reshape(t.shape[0], t.shape[1], -1)      # noqa: E731

    def ref(L, thresh):
        gp, gs = ([0], [slogits[L].shape[1]]) if d.groups[L] is None else d.groups[L]
        return R.tree_kl_ref(flat(slogits[L]), flat(tlogits[L]), None if L == 0 else flat(tprobs[L - 1]), pw.cpu().reshape(BATCH, -1),
                             gp, gs, 1.0 / T[L], thresh, 1.0, lw[L] * T[L] * T[L] / n)
    want, bound = 0.0, 0.0
    for L in range(len(slogits)):
        scale = lw[L] * T[L] * T[L] / n
        r = ref(L, 0.0)
        want += scale * float(r["out"][:, 0].sum())
        bound += scale * float(r["value_bound"].sum())
        err = (flat(grads[L]).double() - r["dz"]).abs()
        assert bool((err <= r["dz_bound"]).all()), (L, float((err - r["dz_bound"]).max()))
        assert torch.equal(d.last_records[L].cpu()[:, 2], r["out"][:, 2])
    loss = loss.detach()
    print("loss", float(loss), "ref", want, "bound", bound)
    # the fp64 sums are rounded to fp32 once per level, and the levels are added in fp32
    assert want > 0 and abs(float(loss) - want) <= bound + 2 * len(slogits) * R.U * abs(want)
    assert d.kept_fraction() == [1.0] * len(slogits)
    # the gate: the kept share is the reference's (a conf within an ulp of the threshold may fall either way: 1 % of room)
    dg = PL.TreeDistillation.for_model(model, temperature=T, thresh=0.3, level_weights=lw)
    lg = dg(slogits, tlogits, tprobs, pw)
    kept = [float(ref(L, 0.3)["keep"].double().mean()) for L in range(len(slogits))]
    got = dg.kept_fraction()
    assert all(abs(a - b) < 0.01 for a, b in zip(got, kept)), (got, kept)
    assert min(got) < 1.0 and 0.0 <= float(lg) < float(loss)
    # restrictive=False passes no parents: the deeper levels weigh every pixel alike
    d2 = PL.TreeDistillation.for_model(model, temperature=T, level_weights=lw, restrictive=False)
    assert float(d2(slogits, tlogits)) > float(loss)
    with pytest.raises(ValueError, match="teacher_probs"):
        d(slogits, tlogits)
    with pytest.raises(ValueError, match="float32"):
        d(slogits, [t.double() for t in tlogits], tprobs)
    with pytest.raises(ValueError, match="pixel_weight"):
        d(slogits, tlogits, tprobs, pw[:, :5])


def test_train_step_without_distillation_launches_what_it_always_did():
    from hrseg_amd import _lib
    from hrseg_amd import train as PT
    counts = []
    for kwargs in ({}, dict(distill=None, teacher=None)):
        model, opt, fns, args, tree, x, t = _setup()
        for fam in _families():
            _lib.launch_count(fam, reset=True)
        loss, _ = PT.train_step(model, opt, x, t, fns, args, tree, [], **kwargs)
        torch.cuda.synchronize()
        counts.append(({fam: _lib.launch_count(fam, reset=True) for fam in _families()}, float(loss)))
    assert counts[0] == counts[1]
    assert counts[0][0]["tree_kl"] == 0 and sum(counts[0][0].values()) > 0


def test_one_distilled_train_step_from_the_ema_teacher():
    from hrseg_amd import _lib
    from hrseg_amd import train as PT
    from hrseg_amd.Metrics import losses as PL
    model, opt, fns, args, tree, x, t = _setup(ema=True)
    PT.train_step(model, opt, x, t, fns, args, tree, [])
    teacher = PT.ema_teacher(model, opt, x, args, tree)
    assert model.training, "the training flag is put back"
    assert teacher.pixel_weight is None and len(teacher.logits) == len(teacher.probs) == len(model.levels)
    assert not any(z.requires_grad for z in teacher.logits)
    d = PL.TreeDistillation.for_model(model, temperature=2.0, thresh=0.2)
    levels_with_groups = sum(1 for g in d.groups if g is None or g[1])
    assert levels_with_groups >= 2
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    _lib.launch_count("tree_kl", reset=True)
    loss, _ = PT.train_step(model, opt, x, t, fns, args, tree, [], distill=d, teacher=teacher)
    torch.cuda.synchronize()
    assert _lib.launch_count("tree_kl", reset=True) == 2 * levels_with_groups
    assert bool(torch.isfinite(loss))
    after = model.state_dict()
    assert all(bool(torch.isfinite(v).all()) for v in after.values() if v.is_floating_point())
    assert any(not torch.equal(before[k], after[k]) for k in before)
    with pytest.raises(ValueError, match="needs a teacher"):
        PT.train_step(model, opt, x, t, fns, args, tree, [], distill=d)
