"""Generate tests/golden/loss_smooth.npz from the REFERENCE itself (run in the build container only).

    python tests/golden/gen_loss_options_golden.py

The reference's SoftDiceLoss(smooth=1.0) and SoftDiceLoss(smooth=0.25) (Metrics/losses.py:40: (2I + smooth) / (U + smooth))
on the inputs of loss_cases.npz -- B=3, C=4, 16x16, item 1 fully ignored: with smooth > 0 that item is no longer 0/0 and
counts -- value and gradient w.r.t. the logits.  The reference is imported through gen_golden.import_reference(), never
copied; the fixture holds inputs and outputs only.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from gen_golden import import_reference  # noqa: E402

SMOOTHS = (1.0, 0.25)


def main():
    _, ref_losses = import_reference()
    g = np.load(os.path.join(HERE, "loss_cases.npz"), allow_pickle=False)
    z, t, w = g["z"], g["t"], [float(v) for v in g["w"]]
    out = dict(z=z, t=t, w=np.array(w, np.float32), smooth=np.array(SMOOTHS, np.float32))
    for i, s in enumerate(SMOOTHS):
        zt = torch.from_numpy(z).clone().requires_grad_(True)
        dice = ref_losses.SoftDiceLoss(smooth=s)(zt, torch.from_numpy(t), class_weight=w, logits_input=True)
        dice.backward()
        out[f"dice{i}"] = np.float32(dice.item())
        out[f"dz{i}"] = zt.grad.numpy()
        print(f"smooth={s}: dice={dice.item():.8f} |dz|max={float(zt.grad.abs().max()):.3e}")
    np.savez_compressed(os.path.join(HERE, "loss_smooth.npz"), **out)


if __name__ == "__main__":
    main()
