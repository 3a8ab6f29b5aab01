"""Online hard example mining through the train step: a small hierarchical UNet (tl tree, 32x32, batch 2) whose CrossEntropyLoss
objects carry ohem_thresh / ohem_min_kept.  get_loss hands them to the fused loss, TapedTrainStep records the OHEM calls with
them by value and keeps the scores, records and workspaces in its pool: in deterministic mode the taped step and the eager
train_step agree bitwise on loss and parameters after two steps; OHEM does change the step; taped_step_for keeps one recording
per (thresh, min_kept); step.ohem[L] reports n_kept >= min(min_kept, n_candidates); and a recording made with OHEM off issues the
calls it always did."""
import argparse

import pytest
import torch

from tests.helpers import load_tree

pytestmark = pytest.mark.gpu

SIZE, BATCH = 32, 2
# (low thresholds: an untrained model gives few pixels a true-class probability above 0.7, and a selection that keeps everything
# would leave the step what it was)
OHEM = dict(ohem_thresh=0.0, ohem_min_kept=300)
OHEM_FOCAL = dict(ohem_thresh=0.2, ohem_min_kept=200, focal_gamma=2.0)
OHEM_CALLS_PER_LEVEL = 2                      # hrseg_ohem_scores + hrseg_ohem_select; the masked partials / bwd replace the plain ones
OHEM_LAUNCHES_PER_LEVEL = 1 + 7 + 1 + 1       # scores, the selection's seven, masked partials, masked backward


def _loss_fns(nc, **ce_options):
    from hrseg_amd.Metrics import losses as PL
    return [[PL.CrossEntropyLoss(**ce_options), PL.SoftDiceLoss(num_classes=n)] for n in nc]


def _setup(**ce_options):
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
    return model, opt, _loss_fns(nc, **ce_options), args, tree, batches


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
    return losses, {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}, fns


def _taped(options, steps=2):
    from hrseg_amd import train as PT
    model, opt, fns, args, tree, batches = _setup(**options)
    step = PT.TapedTrainStep(model, opt, fns, args, tree, *batches[0])
    losses = [step.unpack(step.result()[0].tolist())[0]]
    for x, t in batches[1:steps]:
        losses.append(step.unpack(step(x, t)[0].tolist())[0])
    torch.cuda.synchronize()
    return losses, {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}, step


def _record(rec):
    r = rec.cpu()
    return float(r[:1].view(torch.float32)[0]), int(r[1]), int(r[2])


@pytest.mark.parametrize("options", [OHEM, OHEM_FOCAL], ids=["ohem", "ohem_focal"])
def test_taped_and_eager_steps_agree_bitwise_with_ohem(deterministic, options):
    from hrseg_amd.Metrics import losses as PL
    le, se, fns = _eager(options)
    lt, st, step = _taped(options)
    assert step.replays == 1
    assert all(o == PL.OhemOptions(options["ohem_thresh"], options["ohem_min_kept"]) for o in step.ohem_opts)
    assert le == lt, (le, lt)
    for k in se:
        assert torch.equal(se[k], st[k]), k
    for L, rec in enumerate(step.ohem):
        lam, n_cand, n_kept = _record(rec)
        assert n_cand <= BATCH * SIZE * SIZE and n_kept >= min(options["ohem_min_kept"], n_cand), (L, lam, n_cand, n_kept)
        if L == 0:
            assert 0 < n_kept < n_cand, (lam, n_cand, n_kept, "the selection drops pixels of the root level at these options")
        # the eager step's loss objects saw the same second batch: the same record
        assert _record(fns[L][0].last_ohem) == (lam, n_cand, n_kept), L


def test_ohem_changes_the_step(deterministic):
    base = _eager({}, steps=1)[0][0]
    for options in (OHEM, OHEM_FOCAL):
        got = _eager(options, steps=1)[0][0]
        assert abs(got - base) > 1e-3 * abs(base), (options, got, base)


def test_a_recording_without_ohem_issues_the_calls_it_always_did():
    from hrseg_amd import _lib
    _lib.launch_count("ohem", reset=True)
    plain = _taped({}, steps=2)[2]
    assert all(o is None for o in plain.ohem_opts) and all(r is None for r in plain.ohem)
    assert _lib.launch_count("ohem") == 0, "recording run and replay: no OHEM launch"
    names = [e[1].__name__ for e in plain.tape.entries if e[0] == 0]
    assert not [n for n in names if "ohem" in n]
    with_ohem = _taped(OHEM, steps=2)[2]
    n_levels = with_ohem.n_levels
    assert with_ohem.tape.calls == plain.tape.calls + OHEM_CALLS_PER_LEVEL * n_levels
    assert _lib.launch_count("ohem") == 2 * OHEM_LAUNCHES_PER_LEVEL * n_levels, "recording run + one replay"
    others = [e[1].__name__ for e in with_ohem.tape.entries if e[0] == 0 and "ohem" not in e[1].__name__]
    assert others == [n for n in names if n not in ("hrseg_loss_partials", "hrseg_loss_bwd")]


def test_taped_step_for_keys_its_recordings_by_the_ohem_options():
    from hrseg_amd import train as PT
    model, opt, fns, args, tree, batches = _setup(**OHEM)
    x, t = batches[0]
    nc = args.num_classes
    first, fresh = PT.taped_step_for(model, opt, fns, args, tree, x, t)
    assert first is not None and fresh
    again, fresh = PT.taped_step_for(model, opt, _loss_fns(nc, **OHEM), args, tree, x, t)
    assert again is first and not fresh, "equal options on other loss objects: the same recording"
    other, fresh = PT.taped_step_for(model, opt, _loss_fns(nc, **dict(OHEM, ohem_min_kept=500)), args, tree, x, t)
    assert other is not None and other is not first and fresh, "a changed ohem_min_kept must not replay the stale tape"
    assert [o.min_kept for o in other.ohem_opts] == [500] * len(nc)
    plain, fresh = PT.taped_step_for(model, opt, _loss_fns(nc), args, tree, x, t)
    assert plain is not None and plain is not first and plain is not other and fresh
    assert len(model._hr_tapes) == 3


def test_graphed_step_refuses_ohem():
    from hrseg_amd import train as PT
    model, opt, fns, args, tree, batches = _setup(**OHEM)
    with pytest.raises(NotImplementedError):
        PT.GraphedTrainStep(model, opt, fns, args, tree, *batches[0])
