"""Border weights inside the train step: the recorded launch tape (train.TapedTrainStep) with CrossEntropyLoss(border=...) on
every level against the eager step, bit for bit in deterministic mode; no ATen launch in the recorded body; the options in the
key of a recording; the family counter stays 0 with the option off; the captured-graph step refuses the option."""
import pytest
import torch

from tests.test_tape_gpu import _batches, _setup

pytestmark = pytest.mark.gpu

CASES = ["hrnet_hier_tl_64", "unet_hier_tl_62"]


def _border_setup(name, lr=1e-3, options=(10.0, 2.0, 5)):
    """tests/test_tape_gpu._setup with border weights on both levels (options = None: off)"""
    from hrseg_amd.Metrics import losses as PL
    model, opt, fns, args, tree, g = _setup(name, lr)
    if options is not None:
        fns = [[PL.CrossEntropyLoss(border=PL.BorderWeights(*options)), dice] for _, dice in fns]
    return model, opt, fns, args, tree, g


@pytest.mark.parametrize("name", CASES)
def test_taped_step_with_border_weights_is_bit_identical_to_the_eager_step(name):
    from hrseg_amd import _lib, train as PT
    _lib.set_deterministic(True)
    try:
        results, batches = {}, None
        for mode in ("eager", "tape"):
            model, opt, fns, args, tree, g = _border_setup(name)
            batches = batches or _batches(g, 3)
            losses, cms_all, maps, taped = [], [], [], None
            _lib.launch_count("border_weights", reset=True)
            for x, t in batches:
                if mode == "eager":
                    loss, cms = PT.train_step(model, opt, x, t, fns, args, tree, [])
                    losses.append(float(loss))
                else:
                    if taped is None:
                        taped = PT.TapedTrainStep(model, opt, fns, args, tree, x, t)
                        packed, cms = taped.result()
                    else:
                        packed, cms = taped(x, t)
                    losses.append(taped.unpack(packed.tolist())[0])
                cms_all.append([c.cpu().clone() for c in cms])
                maps.append([fn[0].last_border.cpu().clone() for fn in fns])
            torch.cuda.synchronize()
            # two launches per level and step, replays included (the tape re-issues the library's own calls)
            assert _lib.launch_count("border_weights", reset=True) == 2 * len(fns) * len(batches)
            results[mode] = (losses, cms_all, maps, {k: v.detach().cpu().clone() for k, v in model.state_dict().items()},
                             opt._m.cpu().clone(), opt._v.cpu().clone())
        (le, ce, be, se, me, ve), (lt, ct, bt, st, mt, vt) = results["eager"], results["tape"]
        assert le == lt, (le, lt)
        for a, b in zip(ce + be, ct + bt):
            for u, v in zip(a, b):
                assert torch.equal(u, v)
        assert all(float(m.max()) > 1.0 for step in be for m in step), "the maps do weigh something"
        assert not torch.equal(be[0][0], be[1][0]), "and follow the batch"
        for k in se:
            assert torch.equal(se[k], st[k]), k
        assert torch.equal(me, mt) and torch.equal(ve, vt)
        # and the option is not a no-op: the same steps without it end elsewhere
        model, opt, fns, args, tree, g = _border_setup(name, options=None)
        plain = [float(PT.train_step(model, opt, x, t, fns, args, tree, [])[0]) for x, t in batches]
        assert plain != le
    finally:
        _lib.set_deterministic(False)


@pytest.mark.parametrize("name", CASES)
def test_recorded_body_with_border_weights_launches_no_aten_kernel(name):
    """as tests/test_tape_gpu.py checks it: one more pass of the body under the profiler, every device activity is one of the
    library's kernels -- the border kernels among them"""
    from torch.profiler import ProfilerActivity, profile
    from hrseg_amd import train as PT
    model, opt, fns, args, tree, g = _border_setup(name)
    x, t = _batches(g, 1)[0]
    taped = PT.TapedTrainStep(model, opt, fns, args, tree, x, t)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        with torch.no_grad():
            taped._body()
        torch.cuda.synchronize()
    names = [ev.name for ev in prof.events() if ev.device_type == torch.autograd.DeviceType.CUDA]
    assert len(names) > 100
    foreign = [n for n in names if "at::" in n or "Memcpy" in n or "Memset" in n or "elementwise_kernel" in n]
    assert not foreign, sorted(set(foreign))
    assert sum("bw_search_kernel" in n for n in names) == len(fns) and sum("bw_labels_kernel" in n for n in names) == len(fns)
    assert sum("loss_partials_kernel" in n for n in names) == len(fns)


def test_two_border_options_get_two_recordings():
    from hrseg_amd import train as PT
    from hrseg_amd.Metrics import losses as PL
    model, opt, fns, args, tree, g = _border_setup("unet_hier_tl_62")
    x, t = _batches(g, 1)[0]
    a, fresh_a = PT.taped_step_for(model, opt, fns, args, tree, x, t)
    again, fresh_again = PT.taped_step_for(model, opt, fns, args, tree, x, t)
    other = [[PL.CrossEntropyLoss(border=PL.BorderWeights(10.0, 2.0, 6)), dice] for _, dice in fns]
    b, fresh_b = PT.taped_step_for(model, opt, other, args, tree, x, t)
    assert fresh_a and not fresh_again and fresh_b and again is a and b is not a
    assert [bw.options for bw in a.border] != [bw.options for bw in b.border]


def test_the_family_counter_stays_zero_with_the_option_off():
    from hrseg_amd import _lib, train as PT
    model, opt, fns, args, tree, g = _border_setup("unet_hier_tl_62", options=None)
    x, t = _batches(g, 1)[0]
    _lib.launch_count("border_weights", reset=True)
    PT.train_step(model, opt, x, t, fns, args, tree, [])
    step = PT.TapedTrainStep(model, opt, fns, args, tree, x, t)
    step(x, t)
    torch.cuda.synchronize()
    assert _lib.launch_count("border_weights") == 0 and step.border == [None] * len(fns)
    assert all(fn[0].last_border is None for fn in fns)


def test_the_graphed_step_refuses_border_weights():
    from hrseg_amd import train as PT
    model, opt, fns, args, tree, g = _border_setup("unet_hier_tl_62")
    x, t = _batches(g, 1)[0]
    with pytest.raises(NotImplementedError, match="border weights"):
        PT.GraphedTrainStep(model, opt, fns, args, tree, x, t)
