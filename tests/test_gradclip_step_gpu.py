"""FusedAdamW's max_grad_norm / skip_nonfinite through the train step (eager, recorded tape, train_epoch) on the smallest UNet
of tests/test_tape_gpu.py, in deterministic mode: the taped step is the eager step bit for bit with clipping on; the clipped
update is the fp64 reference's applied to the recorded gradient; a changed threshold reaches a replay without a new recording;
a NaN in the flat gradient voids the step; with both options off the step is today's step."""
import argparse

import pytest
import torch

from tests import gradclip_ref as G
from tests import headloss_ref as R
from tests.helpers import CASES, build_model, level_weights_for, load_golden, load_tree

pytestmark = pytest.mark.gpu

NAME = "unet_hier_tl_62"
LR = 1e-3


@pytest.fixture(autouse=True)
def deterministic():
    from hrseg_amd import _lib
    _lib.set_deterministic(True)
    yield
    _lib.set_deterministic(False)


def _setup(**opt_kw):
    from hrseg_amd.Models import models as PM
    from hrseg_amd.Metrics import losses as PL
    from hrseg_amd import train as PT
    kind, hier, tree_file, size, batch = CASES[NAME]
    g = load_golden(NAME)
    tree = load_tree(tree_file)
    nc = [int(v) for v in g["num_classes"]]
    args = argparse.Namespace(model_type=1, model_select=0, num_classes=nc, level_weights=level_weights_for(tree_file, hier),
                              level0_pretrain_epochs=None, batch_size=batch)
    model = build_model(PM, kind, hier, tree, size).cuda()
    model.train()
    opt = PT.FusedAdamW(model, lr=[LR], **opt_kw)
    fns = [[PL.CrossEntropyLoss(), PL.SoftDiceLoss(num_classes=n)] for n in nc]
    return model, opt, fns, args, tree, g


def _batches(g, n):
    x0, t0 = torch.from_numpy(g["x"]).cuda(), torch.from_numpy(g["target"]).cuda()
    out = [(x0, t0)]
    gen = torch.Generator(device="cuda").manual_seed(5)
    for i in range(1, n):
        out.append((x0 + 0.1 * torch.randn(x0.shape, generator=gen, device="cuda"), t0.roll(i, dims=-1).contiguous()))
    return out


_NORM0 = []


def norm0():
    """global gradient norm of the first step on the golden batch (one eager step, nothing clipped), measured once"""
    if not _NORM0:
        from hrseg_amd import train as PT
        model, opt, fns, args, tree, g = _setup(skip_nonfinite=True)
        x, t = _batches(g, 1)[0]
        PT.train_step(model, opt, x, t, fns, args, tree, [])
        norm, coef, finite, skipped = opt.grad_stats.tolist()
        assert finite == 1.0 and coef == 1.0 and skipped == 0.0 and norm > 0.0
        _NORM0.append(norm)
    return _NORM0[0]


def test_taped_step_is_the_eager_step_bitwise_with_clipping_on():
    from hrseg_amd import train as PT
    max_norm = norm0() / 2
    res = {}
    for mode in ("eager", "tape"):
        model, opt, fns, args, tree, g = _setup(max_grad_norm=max_norm, skip_nonfinite=True)
        losses, stats, taped = [], [], None
        for x, t in _batches(g, 3):
            if mode == "eager":
                losses.append(float(PT.train_step(model, opt, x, t, fns, args, tree, [])[0]))
            else:
                if taped is None:
                    taped = PT.TapedTrainStep(model, opt, fns, args, tree, x, t)
                    packed = taped.result()[0]
                else:
                    packed = taped(x, t)[0]
                host = packed.tolist()
                losses.append(taped.unpack(host)[0])
                gs = taped.grad_stats(host)
                assert gs == {"norm": opt.grad_stats[0].item(), "finite": True, "skipped_total": 0}
            stats.append(opt.grad_stats.cpu().clone())
        torch.cuda.synchronize()
        if mode == "tape":
            names = [e[1].__name__ for e in taped.tape.entries if e[0] == 0]
            assert taped.replays == 2 and names.count("hrseg_grad_sumsq") == 1 and names.count("hrseg_adamw_dev_clip") == 1
            assert "hrseg_adamw_dev" not in names
        res[mode] = (losses, stats, {k: v.detach().cpu().clone() for k, v in model.state_dict().items()},
                     opt._m.cpu().clone(), opt._v.cpu().clone(), opt._state.cpu().clone())
    (le, ge, se, me, ve, ne), (lt, gt, st, mt, vt, nt) = res["eager"], res["tape"]
    assert le == lt, (le, lt)
    print("norm, coef, finite, skipped per step:", [a.tolist() for a in ge])
    assert all(torch.equal(a, b) for a, b in zip(ge, gt)) and 0.49 < ge[0][1].item() < 0.51    # the first step is clipped by half
    assert all(torch.equal(se[k], st[k]) for k in se)
    assert torch.equal(me, mt) and torch.equal(ve, vt) and torch.equal(ne, nt) and ne[0].item() == 3.0


def test_clipped_update_is_the_reference_applied_to_the_recorded_gradient():
    from hrseg_amd import train as PT
    max_norm = norm0() / 2
    model, opt, fns, args, tree, g = _setup(max_grad_norm=max_norm)
    x, t = _batches(g, 1)[0]
    flat = model.flatten_parameters(x.device)
    p0 = flat.data.cpu().clone()
    PT.train_step(model, opt, x, t, fns, args, tree, [])
    grad = flat.grad.cpu().clone()                       # the step leaves its gradient in place until the next zero_grad
    norm, coef, finite, skipped = opt.grad_stats.tolist()
    assert norm == norm0() and finite == 1.0 and skipped == 0.0           # same seed, deterministic mode: the same bits
    ref = G.Run(p0, opt.param_groups[0]["weight_decay"], torch.float64, gscale=1.0)
    want = ref.step(grad, LR, max_norm)
    assert abs(norm - want["norm32"]) <= 2.4e-7 * want["norm32"] and abs(coef - want["coef32"]) <= 2.4e-7 * want["coef32"]
    assert 0.49 < coef < 0.51
    for name, got in (("p", flat.data), ("m", opt._m), ("v", opt._v)):
        d = R.rel(got, ref.tensors()[name])
        print(f"{name}: rel {d:.2e}")
        assert d < R.ADAMW_BARS[name], (name, d)
    # and the update it replaces was twice as long: m is linear in the gradient on the first step
    assert R.rel(opt._m, 0.1 * want["coef32"] * grad.double()) < 1e-5


def test_changed_threshold_reaches_the_next_replay_without_a_new_recording():
    from hrseg_amd import train as PT
    model, opt, fns, args, tree, g = _setup(max_grad_norm=norm0() / 1000)     # far below any of the three steps' norms
    bs = _batches(g, 3)
    step, fresh = PT.taped_step_for(model, opt, fns, args, tree, *bs[0])
    assert fresh and opt.grad_stats[1].item() < 1.0
    step2, fresh2 = PT.taped_step_for(model, opt, fns, args, tree, *bs[1])
    assert step2 is step and not fresh2
    step(*bs[1])
    coef_a = opt.grad_stats[1].item()
    opt.max_grad_norm = 1e30                              # far above: the same recording must now leave the gradient alone
    step3, fresh3 = PT.taped_step_for(model, opt, fns, args, tree, *bs[2])
    assert step3 is step and not fresh3 and len(model._hr_tapes) == 1
    step(*bs[2])
    coef_b = opt.grad_stats[1].item()
    assert coef_a < 1.0 and coef_b == 1.0 and step.replays == 2
    assert int(opt._state[0].item()) == 3


def test_nan_in_the_flat_gradient_voids_the_step():
    model, opt, _, _, _, _ = _setup(skip_nonfinite=True)
    flat = model.flatten_parameters()
    gen = torch.Generator(device="cuda").manual_seed(9)
    flat.grad.copy_(1e-2 * torch.randn(flat.numel, generator=gen, device="cuda"))
    opt.step()                                           # a finite step first: the step count is 1
    assert opt.skipped_steps == 0 and opt.state_dict()["state"][0]["step"].item() == 1.0
    before = [t.clone() for t in (flat.data, opt._m, opt._v, opt._state)]
    flat.grad[flat.numel // 2] = float("nan")
    opt.step()
    assert opt.grad_stats[2].item() == 0.0 and opt.skipped_steps == 1
    assert all(torch.equal(a, b) for a, b in zip((flat.data, opt._m, opt._v, opt._state), before))
    sd = opt.state_dict()
    assert sd["state"][0]["step"].item() == 1.0
    # a checkpoint round trip rebuilds the device scalars: the count continues from the device's 1, not from the two step() calls
    opt.load_state_dict(sd)
    flat.grad.copy_(1e-2 * torch.randn(flat.numel, generator=gen, device="cuda"))
    opt.step()
    assert opt.state_dict()["state"][0]["step"].item() == 2.0 and opt.skipped_steps == 1
    assert not torch.equal(flat.data, before[0])


def test_both_options_off_is_todays_step():
    from hrseg_amd import train as PT
    from hrseg_amd.Metrics.performance_metrics import METRIC_NAMES
    model, opt, fns, args, tree, g = _setup()
    x, t = _batches(g, 1)[0]
    step, fresh = PT.taped_step_for(model, opt, fns, args, tree, x, t)
    host = step.result()[0].tolist()
    L = len(args.num_classes)
    today = 3 * L + sum(n for _, n, _ in step.out["cons"]) + L + len(METRIC_NAMES) * sum(args.num_classes)
    assert fresh and len(host) == today and step.grad_stats(host) is None
    assert not opt.clip_path and opt.grad_stats is None and opt._partial is None and opt.skipped_steps == 0
    names = [e[1].__name__ for e in step.tape.entries if e[0] == 0]
    assert names.count("hrseg_adamw_dev") == 1 and not {"hrseg_grad_sumsq", "hrseg_grad_clip_finalize", "hrseg_adamw_dev_clip"} & set(names)
    model2, opt2, fns2, args2, tree2, _ = _setup(skip_nonfinite=True)
    step2, _ = PT.taped_step_for(model2, opt2, fns2, args2, tree2, x, t)
    host2 = step2.result()[0].tolist()
    assert len(host2) == today + 3 and step2.unpack(host2)[0] == step.unpack(host)[0]
    assert host2[:today] == host


def test_train_epoch_reports_norm_and_skips_from_its_one_readback(monkeypatch, capsys):
    from hrseg_amd import train as PT
    from hrseg_amd.Metrics import performance_metrics as PP
    out = {}
    for tape in ("1", "0"):
        monkeypatch.setenv("HRSEG_TAPE", tape)
        model, opt, fns, args, tree, g = _setup(max_grad_norm=norm0() / 2, skip_nonfinite=True)
        loader = PT.synthetic_loader(tree, 4, 62, 2, hierarchical=True, seed=3)
        mets = [PP.Accuracy(), PP.Jaccardindex(), PP.DiceScore(), PP.Precision(), PP.Recall()]
        r = PT.train_epoch(model, torch.device("cuda"), loader, opt, 1, fns, args, tree, None, *mets, 1)
        assert len(r) == 8 and opt.last_step_skipped is False and opt.last_grad_norm == opt.grad_stats[0].item() > 0.0
        out[tape] = (r[0], opt.last_grad_norm, model.flatten_parameters().data.cpu().clone())
    assert out["1"][:2] == out["0"][:2] and torch.equal(out["1"][2], out["0"][2])
    assert "step skipped" not in capsys.readouterr().out
