"""tests/ema_ref.py pinned against torch's own EMA helper and against hand-worked numbers, and the host-side pieces of
FusedAdamW's weight average that need no GPU: argument validation, ema_state_dict / load_ema_state_dict on a CPU model (torch
copies only, no launch), and the key set save_checkpoint writes with averaging off and on."""
import math

import pytest
import torch

from tests import ema_ref as E
from tests.helpers import CASES, build_model, load_tree

NAME = "unet_hier_tl_62"
TODAY_KEYS = {"epoch", "model_state_dict", "optimizer_state_dict", "loss", "test_measure_mean", "test_measure_std"}


def test_reference_is_torchs_ema_within_the_bar():
    """AveragedModel(multi_avg_fn=get_ema_multi_avg_fn(d)) copies on its first update and then runs e.lerp_(p, 1 - d) in
    fp32: about one ulp from the plain expression, so every update is compared on its own inputs within the bar"""
    from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn
    d = 0.9
    gen = torch.Generator().manual_seed(3)
    net = torch.nn.Linear(37, 11)
    avg = AveragedModel(net, multi_avg_fn=get_ema_multi_avg_fn(d))
    avg.update_parameters(net)                          # the copy
    assert all(torch.equal(a, b) for a, b in zip(avg.module.parameters(), net.parameters()))
    worst = 0.0
    for k in range(6):
        with torch.no_grad():
            for p in net.parameters():
                p.add_(0.3 * torch.randn(p.shape, generator=gen))
        before = [a.detach().clone() for a in avg.module.parameters()]
        avg.update_parameters(net)
        for e0, e1, p in zip(before, avg.module.parameters(), net.parameters()):
            assert not torch.equal(e0, e1)
            worst = max(worst, E.bar_use(e1, e0, p, d, False, k + 1, 0))
    print(f"torch's lerp form uses {worst:.3f} of the bar")
    assert worst <= 1.0


def test_warmup_sequence_takes_both_arms_of_the_min():
    c = E.WARMUP_CASE
    got = [E.eff(c["d"], True, c["s0"] + 1 + k, c["s0"]) for k in range(c["steps"])]
    assert len(E.WARMUP_EFF) == c["steps"] and got == pytest.approx(E.WARMUP_EFF, rel=1e-15, abs=0)
    assert got[7] < 0.5 and got[8] == 0.5 and got[9] == 0.5 and (1 + 9) / (10 + 9) > 0.5       # the crossing is at t = 8
    assert [E.eff(c["d"], False, c["s0"] + 1 + k, c["s0"]) for k in range(3)] == [0.5] * 3
    # d is the fp32 number: 0.999 is not representable
    assert E.eff(0.999, False, 100, 0) == E.f32(0.999) != 0.999
    # twelve updates of a scalar by hand
    e, p = 2.0, 1.0
    for k in range(c["steps"]):
        p = p - 0.125
        e = e + (p - e) * (1.0 - E.WARMUP_EFF[k])
    r = torch.tensor([2.0], dtype=torch.float64)
    pp = 1.0
    for k in range(c["steps"]):
        pp -= 0.125
        r = E.update(r, torch.tensor([pp], dtype=torch.float64), c["d"], True, c["s0"] + 1 + k, c["s0"])
    assert abs(float(r) - e) <= 1e-15 * abs(e)


def test_fp32_evaluation_of_the_expression_sits_inside_the_bar():
    """how much of the bar plain fp32 arithmetic (torch on the host, no fused multiply-add) uses: a record, and a check that
    the bar is not so tight that a correct fp32 evaluation could miss it"""
    worst = 0.0
    for n in (5, 1023, 100003):
        x = E.inputs(n)
        for d, warmup, s, s0 in ((0.9, False, 1, 0), (0.999, True, 3, 0), (0.5, True, 14, 5), (0.9999, True, 5000, 17)):
            t = torch.tensor(float(s)) - torch.tensor(float(s0)) - 1.0
            dd = torch.tensor(d, dtype=torch.float32)
            eff = torch.minimum(dd, (1.0 + t) / (10.0 + t)) if warmup else dd
            alpha = 1.0 - eff
            assert alpha.dtype == torch.float32
            got = x["e"] + (x["p"] - x["e"]) * alpha
            worst = max(worst, E.bar_use(got, x["e"], x["p"], d, warmup, s, s0))
    print(f"fp32 torch evaluation uses {worst:.3f} of the bar")
    assert worst <= 1.0
    # and the bar does catch an update that used the wrong warm-up count
    x = E.inputs(1023)
    wrong = E.update(x["e"], x["p"], 0.5, True, 8, 5).float()
    assert E.bar_use(wrong, x["e"], x["p"], 0.5, True, 9, 5) > 1.0
    # an exact zero must be reproduced exactly
    z = torch.zeros(4)
    assert E.bar_use(z, z, z, 0.9, False, 1, 0) == 0.0 and math.isinf(E.bar_use(z + 1e-30, z, z, 0.9, False, 1, 0))


def _cpu_model_and_optimizer(**kw):
    from hrseg_amd import train as PT
    from hrseg_amd.Models import models as PM
    kind, hier, tree_file, size, _ = CASES[NAME]
    model = build_model(PM, kind, hier, load_tree(tree_file), size)
    return model, PT.FusedAdamW(model, lr=[1e-3], **kw), PT


def test_ema_arguments_are_validated():
    model, opt, PT = _cpu_model_and_optimizer()
    assert opt.ema_decay is None and not opt.ema_path and opt._ema is None and opt._emacfg is None
    for bad in (0.0, 1.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            PT.FusedAdamW(model, lr=[1e-3], ema_decay=bad)
        with pytest.raises(ValueError):
            opt.ema_decay = bad
    assert opt.ema_decay is None
    for off in (opt.ema_state_dict, lambda: opt.load_ema_state_dict({}), lambda: opt.ema_parameters().__enter__()):
        with pytest.raises(RuntimeError):
            off()
    opt.ema_decay = 0.99
    assert opt.ema_path and opt.ema_decay == 0.99 and opt.ema_warmup is True


def test_checkpoint_keys_and_ema_state_dict_round_trip_on_the_host(tmp_path):
    model, opt, PT = _cpu_model_and_optimizer()
    path = str(tmp_path / "last.pt")
    PT.save_checkpoint(path, model, opt, 3, 0.5)
    ck = torch.load(path, map_location="cpu")
    assert set(ck) == TODAY_KEYS                                     # averaging off: exactly today's dict
    assert set(ck["optimizer_state_dict"]) == {"state", "param_groups"}

    model, opt, PT = _cpu_model_and_optimizer(ema_decay=0.75, ema_warmup=False)
    sd = opt.ema_state_dict()                                        # allocates the shadow: a bit copy of the parameters
    msd = model.state_dict()
    names = {n for n, _ in model.named_parameters()}
    assert list(sd) == list(msd) and opt._ema.numel() == model._flat.numel and opt._ema_s0 == 0
    assert opt._emacfg.tolist() == [0.75, 0.0, 0.0]
    for k in msd:
        assert sd[k].shape == msd[k].shape and torch.equal(sd[k], msd[k]), k
        assert (sd[k].data_ptr() != msd[k].data_ptr()) == (k in names), k          # parameters are copies, buffers the live ones
    # load_ema_state_dict is the inverse, into the buffer the optimizer already has
    shadow, cfg = opt._ema, opt._emacfg
    new = {k: (v + 1.0 if k in names else v) for k, v in sd.items()}
    opt.load_ema_state_dict(new)
    assert opt._ema is shadow and opt._emacfg is cfg
    back = opt.ema_state_dict()
    assert all(torch.equal(back[k], new[k]) for k in new)
    assert all(torch.equal(model.state_dict()[k], msd[k]) for k in msd)             # the model itself did not move
    opt.ema_decay = 0.5                                              # a new decay: the same device buffer, updated in place
    opt._sync_hyper(torch.device("cpu"))
    assert opt._emacfg is cfg and cfg.tolist() == [0.5, 0.0, 0.0]
    PT.save_checkpoint(path, model, opt, 4, 0.25)
    ck = torch.load(path, map_location="cpu")
    assert set(ck) == TODAY_KEYS | {"ema_state_dict", "ema_meta"}
    assert ck["ema_meta"] == {"decay": 0.5, "warmup": False, "start_step": 0}
    assert list(ck["ema_state_dict"]) == list(msd) and all(torch.equal(ck["ema_state_dict"][k], new[k]) for k in new)
    assert set(ck["optimizer_state_dict"]) == {"state", "param_groups"}            # still torch.optim.AdamW's format
    # what the prediction script does with such a file
    fresh, _, _ = _cpu_model_and_optimizer()
    fresh.load_state_dict(ck["ema_state_dict"])
    assert all(torch.equal(fresh.state_dict()[k], new[k]) for k in new)
    # no step, checkpoint or second block while the model holds the average (the flag alone: the exchange is a kernel)
    opt._ema_swapped = True
    for refused in (opt.step, lambda: PT.save_checkpoint(path, model, opt, 5, 0.1), lambda: opt.ema_parameters().__enter__(),
                    lambda: opt.load_ema_state_dict(new)):
        with pytest.raises(RuntimeError):
            refused()
