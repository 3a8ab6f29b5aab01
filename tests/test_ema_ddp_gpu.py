"""The weight average under data parallelism, in the manner of tests/test_gradclip_ddp_gpu.py: two ranks (two processes sharing
the one card, gloo as the transport) run three recorded train steps with ema_decay set.  The average is advanced by the update
kernel from the parameters both ranks hold alike, with no collective of its own: after the three steps the shadow must be
bitwise the same on both ranks, and it must be the reference's update of the previous shadow on the step's parameters."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import ema_ref as E

pytestmark = pytest.mark.gpu

NAME = "unet_hier_tl_62"
DECAY = 0.9


def _worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      HRSEG_WGRAD_STREAM="0", HRSEG_DETERMINISTIC="1")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from hrseg_amd import train as PT
    from hrseg_amd.parallel import GradSync
    from tests.test_ddp_gpu import PER_RANK, _setup
    model, args, tree, fns, x, t = _setup(NAME)
    sync = GradSync(model)
    opt = PT.FusedAdamW(model, lr=[1e-3], ema_decay=DECAY)
    opt.grad_scale = 1.0 / world
    sl = slice(rank * PER_RANK, (rank + 1) * PER_RANK)
    xs = [x[sl], (x[sl] * 0.9).contiguous(), x[sl].flip(-1).contiguous()]
    step, prev = None, None
    for xi in xs:
        if step is None:
            step = PT.TapedTrainStep(model, opt, fns, args, tree, xi, t[sl])
        else:
            prev = opt._ema.clone()
            step(xi, t[sl])
    torch.cuda.synchronize()
    names = [e[1].__name__ for e in step.tape.entries if e[0] == 0]
    assert step.replays == 2 and step.synced and len(sync.launched) >= 2 and names.count("hrseg_adamw_dev_ema") == 1
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), ema=opt._ema.cpu().numpy(), prev=prev.cpu().numpy(),
             data=model._flat.data.cpu().numpy(), cfg=opt._emacfg.cpu().numpy(), state=opt._state.cpu().numpy())
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_hold_bitwise_the_same_shadow_after_three_taped_steps(tmp_path):
    port = 30600 + (os.getpid() % 200)
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    r0, r1 = (np.load(tmp_path / f"rank{r}.npz") for r in range(2))
    for key in ("ema", "prev", "data", "cfg", "state"):
        assert np.array_equal(r0[key], r1[key]), key                              # bitwise the same on both ranks
    assert r0["cfg"].tolist() == [E.f32(DECAY), 1.0, 0.0] and r0["state"][0] == 3.0
    assert not np.array_equal(r0["ema"], r0["data"]) and not np.array_equal(r0["ema"], r0["prev"])
    use = E.bar_use(torch.from_numpy(r0["ema"]), torch.from_numpy(r0["prev"]), torch.from_numpy(r0["data"]), DECAY, True, 3, 0)
    print(f"third update (t = 2, eff = 1/4): {use:.3f} of the bar")
    assert use <= 1.0
