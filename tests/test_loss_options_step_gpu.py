"""The loss options through the train step: a small hierarchical UNet (tl tree, 32x32, batch 2) whose loss objects carry a focal
exponent with Dice smoothing, or Tversky weights.  get_loss hands them to the fused loss, TapedTrainStep records the _opt calls
with them by value: in deterministic mode the taped step and the eager train_step agree bitwise on loss and parameters after
two steps; the options do change the loss; taped_step_for keeps one recording per option set; and SoftDiceLoss(smooth > 0)
counts every item, the fully ignored ones too."""
import argparse

import pytest
import torch

from tests.helpers import load_tree

pytestmark = pytest.mark.gpu

SIZE, BATCH = 32, 2
FOCAL_SMOOTH = dict(focal_gamma=2.0, smooth=1.0)
TVERSKY = dict(alpha=0.3, beta=0.7)


def _loss_fns(nc, focal_gamma=0.0, smooth=0.0, alpha=0.5, beta=0.5):
    from hrseg_amd.Metrics import losses as PL
    return [[PL.CrossEntropyLoss(focal_gamma=focal_gamma), PL.SoftDiceLoss(smooth=smooth, num_classes=n, alpha=alpha, beta=beta)]
            for n in nc]


def _setup(**options):
    from hrseg_amd import train as PT
    from hrseg_amd.Models import models as PM
    from hrseg_amd.utils import synth
    from hrseg_amd.utils.hierarchy import get_classes
    tree = load_tree("class_tree_tl.json")
    nc = get_classes(tree, full=True)
    args = argparse.Namespace(model_type=1, model_select=0, num_classes=nc, level_weights=synth.README_LEVEL_WEIGHTS_TL,
                              level0_pretrain_epochs=None, batch_size=BATCH)
    model = synth.fill_state_dict(PM.UNet(size=SIZE, n_channels=3, hierarchy=tree, model_type=1)).cuda()
    model.train()
    opt = PT.FusedAdamW(model, lr=[1e-3])
    batches = []
    for seed in (3, 4):
        x, t = synth.synthetic_batch(tree, BATCH, SIZE, seed=seed, hierarchical=True, blob=4)
        batches.append((torch.from_numpy(x).cuda(), torch.from_numpy(t).cuda()))
    return model, opt, _loss_fns(nc, **options), args, tree, batches


@pytest.fixture
def deterministic():
    from hrseg_amd import _lib
    _lib.set_deterministic(True)
    yield
    _lib.set_deterministic(False)


def _eager(options, steps=2):
    from hrseg_amd import train as PT
    model, opt, fns, args, tree, batches = _setup(**options)
    losses = [float(PT.train_step(model, opt, x, t, fns, args, tree, [])[0]) for x, t in batches[:steps]]
    torch.cuda.synchronize()
    return losses, {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}


def _taped(options, steps=2):
    from hrseg_amd import train as PT
    model, opt, fns, args, tree, batches = _setup(**options)
    step = PT.TapedTrainStep(model, opt, fns, args, tree, *batches[0])
    losses = [step.unpack(step.result()[0].tolist())[0]]
    for x, t in batches[1:steps]:
        losses.append(step.unpack(step(x, t)[0].tolist())[0])
    torch.cuda.synchronize()
    return losses, {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}, step


@pytest.mark.parametrize("options", [FOCAL_SMOOTH, TVERSKY], ids=["focal_smooth", "tversky"])
def test_taped_and_eager_steps_agree_bitwise_with_loss_options(deterministic, options):
    from hrseg_amd.Metrics import losses as PL
    le, se = _eager(options)
    lt, st, step = _taped(options)
    assert step.replays == 1
    assert all(o == PL.LossOptions(options.get("focal_gamma", 0.0), options.get("smooth", 0.0), options.get("alpha", 0.5),
                                   options.get("beta", 0.5)) for o in step.opts)
    assert le == lt, (le, lt)
    for k in se:
        assert torch.equal(se[k], st[k]), k


def test_loss_options_change_the_step(deterministic):
    base = _eager({}, steps=1)[0][0]
    for options in (FOCAL_SMOOTH, TVERSKY):
        got = _eager(options, steps=1)[0][0]
        assert abs(got - base) > 1e-3 * abs(base), (options, got, base)
    assert all(o is None for o in _taped({}, steps=1)[2].opts), "default options record the calls without options"


def test_taped_step_for_keys_its_recordings_by_the_loss_options():
    from hrseg_amd import train as PT
    model, opt, fns, args, tree, batches = _setup(**FOCAL_SMOOTH)
    x, t = batches[0]
    nc = args.num_classes
    first, fresh = PT.taped_step_for(model, opt, fns, args, tree, x, t)
    assert first is not None and fresh
    again, fresh = PT.taped_step_for(model, opt, _loss_fns(nc, **FOCAL_SMOOTH), args, tree, x, t)
    assert again is first and not fresh, "equal options on other loss objects: the same recording"
    other, fresh = PT.taped_step_for(model, opt, _loss_fns(nc, **TVERSKY), args, tree, x, t)
    assert other is not None and other is not first and fresh
    plain, fresh = PT.taped_step_for(model, opt, _loss_fns(nc), args, tree, x, t)
    assert plain is not None and plain is not first and plain is not other and fresh
    assert len(model._hr_tapes) == 3


def test_smooth_dice_counts_fully_ignored_items():
    from hrseg_amd import ops
    from hrseg_amd.Metrics import losses as PL
    B, C = 3, 4
    z = torch.randn(B, C, 8, 8, generator=torch.Generator().manual_seed(1)).cuda()
    t = torch.full((B, C, 8, 8), -1.0).cuda()
    w = [0.5, 1.5, 1.0, 2.0]
    assert PL.SoftDiceLoss()(z, t, logits_input=True, class_weight=w) is None
    dice = PL.SoftDiceLoss(smooth=1.0)(z, t, logits_input=True, class_weight=w)
    assert dice is not None and float(dice) == 0.0
    out, _ = ops.loss_fwd(z, t, torch.tensor(w).cuda(), (0.0, 1.0, 0.5, 0.5))
    assert float(out[2]) == B
