"""FusedAdamW's weight average (ema_decay) through the train step -- eager, recorded tape, ema_parameters(), checkpoints -- on the
smallest UNet of tests/test_gradclip_step_gpu.py, in deterministic mode: the taped step is the eager step bit for bit, shadow
included; averaging off is today's step and averaging on adds no launch; a changed decay reaches a replay without a new
recording; inside ema_parameters() the model computes what a fresh model loaded from ema_state_dict() computes (BatchNorm
folded or not) and afterwards training continues as if nothing had happened; a checkpoint resumes bit for bit."""
import pytest
import torch

from tests import ema_ref as E
from tests.test_gradclip_step_gpu import NAME, _batches, _setup

pytestmark = pytest.mark.gpu

EMA_NAMES = {"hrseg_adamw_dev_ema", "hrseg_adamw_dev_clip_ema", "hrseg_ema_update", "hrseg_swap"}


@pytest.fixture(autouse=True)
def deterministic():
    from hrseg_amd import _lib
    _lib.set_deterministic(True)
    yield
    _lib.set_deterministic(False)


_NORM0 = []


def norm0():
    """global gradient norm of the first step on the golden batch (one eager step, nothing clipped), measured once"""
    if not _NORM0:
        from hrseg_amd import train as PT
        model, opt, fns, args, tree, g = _setup(skip_nonfinite=True)
        PT.train_step(model, opt, *_batches(g, 1)[0], fns, args, tree, [])
        _NORM0.append(opt.grad_stats[0].item())
        assert _NORM0[0] > 0.0
    return _NORM0[0]


def _names(step):
    return [e[1].__name__ for e in step.tape.entries if e[0] == 0]


def _snapshot(model, opt):
    torch.cuda.synchronize()
    out = {"sd::" + k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    out.update(m=opt._m.cpu().clone(), v=opt._v.cpu().clone(), state=opt._state.cpu().clone())
    if opt._ema is not None:
        out["ema"] = opt._ema.cpu().clone()
    return out


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k


def _run(mode, n_steps, **opt_kw):
    """n_steps train steps on the batches of _batches -> (model, optimizer, TapedTrainStep or None, the rest of _setup)"""
    from hrseg_amd import train as PT
    model, opt, fns, args, tree, g = _setup(**opt_kw)
    taped = None
    for x, t in _batches(g, n_steps):
        if mode == "eager":
            PT.train_step(model, opt, x, t, fns, args, tree, [])
        elif taped is None:
            taped = PT.TapedTrainStep(model, opt, fns, args, tree, x, t)
        else:
            taped(x, t)
    return model, opt, taped, (fns, args, tree, g)


def _forward(model, x, args, tree):
    with torch.no_grad():
        probs, logits = model(x, type=args.model_type, hierarchy=tree)
    return list(probs) + list(logits)


# ================================================================================================ tape == eager
@pytest.mark.parametrize("clip", [False, True], ids=["clip_off", "clip_on"])
def test_taped_step_is_the_eager_step_bitwise_shadow_included(clip):
    kw = dict(ema_decay=0.9)
    if clip:
        kw.update(max_grad_norm=norm0() / 2, skip_nonfinite=True)
    res = {}
    for mode in ("eager", "tape"):
        model, opt, taped, _ = _run(mode, 3, **kw)
        res[mode] = _snapshot(model, opt)
        assert opt.ema_path and opt._state[0].item() == 3.0 and opt._ema_s0 == 0
        assert opt._emacfg.tolist() == [E.f32(0.9), 1.0, 0.0]
        if mode == "tape":
            names = _names(taped)
            fused = "hrseg_adamw_dev_clip_ema" if clip else "hrseg_adamw_dev_ema"
            assert taped.replays == 2 and names.count(fused) == 1 and EMA_NAMES & set(names) == {fused}
            assert "hrseg_adamw_dev" not in names and "hrseg_adamw_dev_clip" not in names
    _same(res["eager"], res["tape"])
    flat = model.flatten_parameters()
    assert not torch.equal(res["tape"]["ema"], flat.data.cpu())           # an average, not a copy


# ================================================================================================ off is today's step
@pytest.mark.parametrize("clip", [False, True], ids=["clip_off", "clip_on"])
def test_ema_off_is_todays_step_and_ema_on_adds_no_launch(clip):
    kw = dict(max_grad_norm=norm0() / 2, skip_nonfinite=True) if clip else {}
    model0, opt0, tape0, _ = _run("tape", 2, **kw)
    model1, opt1, tape1, _ = _run("tape", 2, ema_decay=0.9, **kw)
    n0, n1 = _names(tape0), _names(tape1)
    plain, fused = ("hrseg_adamw_dev_clip", "hrseg_adamw_dev_clip_ema") if clip else ("hrseg_adamw_dev", "hrseg_adamw_dev_ema")
    assert n0.count(plain) == 1 and not EMA_NAMES & set(n0)
    assert not opt0.ema_path and opt0._ema is None and opt0._emacfg is None
    # the same recorded calls in the same order, but for the one entry point that also carries the average
    assert len(tape0.tape.entries) == len(tape1.tape.entries) and tape0.tape.calls == tape1.tape.calls
    assert [fused if k == plain else k for k in n0] == n1
    a, b = _snapshot(model0, opt0), _snapshot(model1, opt1)
    b.pop("ema")
    _same(a, b)                                                            # parameters, moments, statistics: bitwise
    # and the eager step with averaging off is that step too
    model2, opt2, _, _ = _run("eager", 2, **kw)
    _same(a, _snapshot(model2, opt2))


# ================================================================================================ decay lives on the device
def test_changed_decay_reaches_the_next_replay_without_a_new_recording():
    from hrseg_amd import train as PT
    model, opt, fns, args, tree, g = _setup(ema_decay=0.9, ema_warmup=False)
    bs = _batches(g, 3)
    step, fresh = PT.taped_step_for(model, opt, fns, args, tree, *bs[0])
    assert fresh
    flat, cfg, shadow = model.flatten_parameters(), opt._emacfg, opt._ema
    e_prev = shadow.clone()
    step(*bs[1])
    assert E.bar_use(shadow, e_prev, flat.data, 0.9, False, 2, 0) <= 1.0
    opt.ema_decay = 0.5
    step3, fresh3 = PT.taped_step_for(model, opt, fns, args, tree, *bs[2])
    assert step3 is step and not fresh3 and len(model._hr_tapes) == 1
    e_prev = shadow.clone()
    step(*bs[2])
    assert opt._emacfg is cfg and opt._ema is shadow and cfg.tolist() == [0.5, 0.0, 0.0] and step.replays == 2
    use_new, use_old = (E.bar_use(shadow, e_prev, flat.data, d, False, 3, 0) for d in (0.5, 0.9))
    print(f"replay after ema_decay = 0.5: {use_new:.3f} of the bar (as 0.9: {use_old:.3g})")
    assert use_new <= 1.0 < use_old
    # None <-> a number is another path: a new recording
    opt.ema_decay = None
    with pytest.raises(RuntimeError):
        step(*bs[0])
    step4, fresh4 = PT.taped_step_for(model, opt, fns, args, tree, *bs[0])
    assert fresh4 and step4 is not step and "hrseg_adamw_dev" in _names(step4)


# ================================================================================================ ema_parameters()
def test_ema_parameters_runs_the_average_and_leaves_training_undisturbed():
    from hrseg_amd.Models import models as PM
    from tests.helpers import CASES, build_model, load_tree
    ref_model, ref_opt, _, _ = _run("tape", 3, ema_decay=0.9)              # the uninterrupted run
    want = _snapshot(ref_model, ref_opt)
    model, opt, taped, (fns, args, tree, g) = _run("tape", 2, ema_decay=0.9)
    bs = _batches(g, 3)
    x = bs[0][0]
    flat = model.flatten_parameters()
    before = _snapshot(model, opt)
    p_before, e_before = flat.data.clone(), opt._ema.clone()
    sd = opt.ema_state_dict()
    kind, hier, tree_file, size, _ = CASES[NAME]
    model.eval()
    for fold in (True, False):
        model.fold_bn = fold
        y_raw = _forward(model, x, args, tree)                            # caches built for the raw weights
        # a freshly built model that was given the averaged weights (built first: the model under test runs last and so
        # holds the library's weight-image registration again when training goes on)
        fresh = build_model(PM, kind, hier, load_tree(tree_file), size).cuda()
        fresh.load_state_dict(sd)
        fresh.eval()
        fresh.fold_bn = fold
        y_fresh = _forward(fresh, x, args, tree)
        with opt.ema_parameters():
            assert torch.equal(flat.data, e_before) and torch.equal(opt._ema, p_before)
            y_ema = _forward(model, x, args, tree)
            inner = opt.ema_state_dict()                                   # still the average
            assert all(torch.equal(inner[k], sd[k]) for k in sd)
        assert torch.equal(flat.data, p_before) and torch.equal(opt._ema, e_before)
        y_back = _forward(model, x, args, tree)
        assert len(y_ema) == len(y_fresh) == 2 * len(args.num_classes)
        for a, b, c, d in zip(y_ema, y_fresh, y_raw, y_back):
            assert torch.equal(a, b), f"fold_bn={fold}: the model inside ema_parameters() is not the model with the averaged weights"
            assert torch.equal(c, d), f"fold_bn={fold}: the model after ema_parameters() is not the model before it"
        assert any(not torch.equal(a, c) for a, c in zip(y_ema, y_raw))
    model.fold_bn = True
    model.train()
    _same(before, _snapshot(model, opt))
    taped(*bs[2])
    _same(want, _snapshot(model, opt))


def test_step_replay_and_checkpoint_are_refused_inside_ema_parameters(tmp_path):
    from hrseg_amd import train as PT
    model, opt, taped, (fns, args, tree, g) = _run("tape", 1, ema_decay=0.9)
    x, t = _batches(g, 1)[0]
    before = _snapshot(model, opt)
    with opt.ema_parameters():
        for refused in (opt.step, lambda: taped(x, t), lambda: PT.save_checkpoint(str(tmp_path / "last.pt"), model, opt, 0, 0.0),
                        lambda: opt.ema_parameters().__enter__(), lambda: opt.load_ema_state_dict({})):
            with pytest.raises(RuntimeError):
                refused()
    assert not (tmp_path / "last.pt").exists() and not (tmp_path / "new_last.pt").exists() and taped.replays == 0
    _same(before, _snapshot(model, opt))                                    # nothing moved, and the block put everything back
    taped(x, t)                                                             # outside the block the step runs again
    assert taped.replays == 1
    opt2 = _setup()[1]
    with pytest.raises(RuntimeError):
        opt2.ema_parameters().__enter__()                                   # averaging off


# ================================================================================================ checkpoints
def test_checkpoint_resumes_bitwise_and_a_file_without_average_reseeds(tmp_path):
    from hrseg_amd import train as PT
    kw = dict(ema_decay=0.9)
    model, opt, _, (fns, args, tree, g) = _run("eager", 2, **kw)
    bs = _batches(g, 3)
    path = str(tmp_path / "last.pt")
    PT.save_checkpoint(path, model, opt, 1, 0.0)
    PT.train_step(model, opt, *bs[2], fns, args, tree, [])
    want = _snapshot(model, opt)

    model2, opt2, fns2, args2, tree2, _ = _setup(ema_decay=0.5, ema_warmup=False)       # the file's schedule wins
    opt2._moments()
    shadow, cfg = opt2._ema, opt2._emacfg
    ck = PT.load_checkpoint(path, model2, opt2)
    assert set(ck) >= {"ema_state_dict", "ema_meta"} and ck["ema_meta"] == {"decay": 0.9, "warmup": True, "start_step": 0}
    assert opt2._ema is shadow and opt2._emacfg is cfg and cfg.tolist() == [E.f32(0.9), 1.0, 0.0]      # updated in place
    PT.train_step(model2, opt2, *bs[2], fns2, args2, tree2, [])
    _same(want, _snapshot(model2, opt2))

    # a checkpoint without the two keys (the reference's, or one written with averaging off)
    model3, opt3, _, _ = _run("eager", 2)
    PT.save_checkpoint(path, model3, opt3, 1, 0.0)
    model4, opt4, fns4, args4, tree4, _ = _setup(**kw)
    opt4._moments()
    shadow, cfg = opt4._ema, opt4._emacfg
    ck = PT.load_checkpoint(path, model4, opt4)
    flat = model4.flatten_parameters()
    assert "ema_state_dict" not in ck and "ema_meta" not in ck
    assert opt4._ema is shadow and opt4._emacfg is cfg and cfg.tolist() == [E.f32(0.9), 1.0, 2.0] and opt4._ema_s0 == 2
    assert torch.equal(shadow, flat.data) and torch.equal(flat.data, model3.flatten_parameters().data)
    e_prev = shadow.clone()
    PT.train_step(model4, opt4, *bs[2], fns4, args4, tree4, [])
    assert opt4._state[0].item() == 3.0
    use = E.bar_use(shadow, e_prev, flat.data, 0.9, True, 3, 2)             # warm-up restarted: t = 0, eff = 1/10
    print(f"first update after the re-seed: {use:.3f} of the bar")
    assert use <= 1.0 < E.bar_use(shadow, e_prev, flat.data, 0.9, True, 3, 0)
