"""Gradient clipping and the non-finite step skip under data parallelism, in the manner of tests/test_ddp_gpu.py: two ranks
(two processes sharing the one card, gloo as the transport).  The norm is taken inside optimizer.step(), after GradSync's
last bucket has arrived, on the all-reduced buffer: both ranks must report bitwise the same norm -- the norm of the AVERAGED
gradient -- with no collective of their own, and a NaN in ONE rank's local gradient must void the step on BOTH."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import gradclip_ref as G

pytestmark = pytest.mark.gpu

NAME = "unet_hier_tl_62"
MAX_NORM = 1e-8         # below the 1e-6 of the formula's denominator: every finite step is clipped, whatever its norm


def _local(rank, n, poisoned=False):
    """rank-local flat gradient of the hand-fed steps (seeded, so the parent can rebuild it)"""
    g = torch.randn(n, generator=torch.Generator().manual_seed(77 + rank)) * (1.0 + rank)
    if poisoned and rank == 1:
        g[n // 3] = float("nan")
    return g


def _worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      HRSEG_WGRAD_STREAM="0", HRSEG_DETERMINISTIC="1")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from hrseg_amd import train as PT
    from hrseg_amd.parallel import GradSync
    from tests.test_ddp_gpu import PER_RANK, _setup
    model, args, tree, fns, x, t = _setup(NAME)
    sync = GradSync(model)
    opt = PT.FusedAdamW(model, lr=[1e-3], max_grad_norm=MAX_NORM, skip_nonfinite=True)
    opt.grad_scale = 1.0 / world
    out = {}
    # (1) a real two-rank train step: the reverse pass issues the buckets, optimizer.step() takes the norm behind them
    sl = slice(rank * PER_RANK, (rank + 1) * PER_RANK)
    PT.train_step(model, opt, x[sl], t[sl], fns, args, tree, [])
    torch.cuda.synchronize()
    flat = model._flat
    assert len(sync.launched) >= 2
    out["step_stats"], out["step_grad"] = opt.grad_stats.cpu().numpy(), flat.grad.cpu().numpy()
    # (2) a hand-fed local gradient through the same exchange ("end" = one bucket over the whole buffer), then the optimizer
    flat.grad.copy_(_local(rank, flat.numel).cuda())
    sync("end")
    opt.step()
    torch.cuda.synchronize()
    out["fed_stats"], out["fed_data"] = opt.grad_stats.cpu().numpy(), flat.data.cpu().numpy()
    # (3) the same with a NaN in rank 1's local gradient only
    before = [v.clone() for v in (flat.data, opt._m, opt._v, opt._state)]
    flat.grad.copy_(_local(rank, flat.numel, poisoned=True).cuda())
    sync("end")
    opt.step()
    torch.cuda.synchronize()
    out["nan_stats"], out["nan_data"] = opt.grad_stats.cpu().numpy(), flat.data.cpu().numpy()
    out["nan_untouched"] = np.array([all(torch.equal(a, b) for a, b in zip((flat.data, opt._m, opt._v, opt._state), before))])
    out["skipped"], out["steps"] = np.array([opt.skipped_steps]), np.array([opt.state_dict()["state"][0]["step"].item()])
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), **out)
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_agree_bitwise_on_norm_and_on_skipping(tmp_path):
    port = 30300 + (os.getpid() % 200)
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    r0, r1 = (np.load(tmp_path / f"rank{r}.npz") for r in range(2))
    for key in ("step_stats", "step_grad", "fed_stats", "fed_data", "nan_data", "skipped", "steps"):
        assert np.array_equal(r0[key], r1[key], equal_nan=True), key            # bitwise the same on both ranks
    # (1) the norm of the real step is the norm of the averaged gradient: grad_scale = 1/2 times the all-reduced sum
    want = G.verdict(torch.from_numpy(r0["step_grad"]), 0.5, MAX_NORM)
    norm, coef, finite, skipped = r0["step_stats"].tolist()
    assert abs(norm - want["norm32"]) <= 2.4e-7 * want["norm32"] and abs(coef - want["coef32"]) <= 2.4e-7 * want["coef32"]
    assert finite == 1.0 and skipped == 0.0 and coef < 1.0
    # (2) hand-fed: the all-reduced buffer is the fp32 sum of the two local gradients
    n = r0["fed_data"].size
    want = G.verdict(_local(0, n) + _local(1, n), 0.5, MAX_NORM)
    norm, coef, finite, skipped = r0["fed_stats"].tolist()
    assert abs(norm - want["norm32"]) <= 2.4e-7 * want["norm32"] and finite == 1.0 and skipped == 0.0
    # (3) rank 1's NaN reached both ranks through the sum: both skipped, nothing moved
    for r in (r0, r1):
        assert r["nan_stats"][2] == 0.0 and r["nan_stats"][3] == 1.0 and np.isnan(r["nan_stats"][0])
        assert bool(r["nan_untouched"][0]) and int(r["skipped"][0]) == 1 and float(r["steps"][0]) == 2.0
        assert np.array_equal(r["nan_data"], r["fed_data"])
