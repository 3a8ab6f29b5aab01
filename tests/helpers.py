"""Shared test helpers: golden-case table, oracle model construction."""
import json
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
DATA = os.path.join(ROOT, "restrictive-hierarchical-semantic-segmentation_amd", "data")

from hrseg_amd.utils import synth  # noqa: E402
from hrseg_amd.utils.config import hrnet_w48_config  # noqa: E402

EXT_WEIGHTS = [[0.3, 1.2], [0.8, 1.1], [1.5, 1.4, 2.0, 0.6], [1.6, 0.4, 1.0]]

# name -> (model kind, hierarchical, tree file, size, batch)
CASES = {
    "unet_flat_tl_32": ("unet", False, "class_tree_tl.json", 32, 2),
    "unet_hier_tl_62": ("unet", True, "class_tree_tl.json", 62, 2),
    "unet_hier_ext_32": ("unet", True, "class_tree_tl_extended.json", 32, 2),
    "hrnet_flat_tl_64": ("hrnet", False, "class_tree_tl.json", 64, 2),
    "hrnet_hier_tl_64": ("hrnet", True, "class_tree_tl.json", 64, 2),
    "hrnet_hier_ext_62": ("hrnet", True, "class_tree_tl_extended.json", 62, 2),
}


CSRC = os.path.join(ROOT, "restrictive-hierarchical-semantic-segmentation_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def _resources(unit):
    """{mangled kernel name: (vgprs, scratch bytes per lane, spilled vgprs)} of one translation unit, compiled with the flags the
    Makefile gives that unit: -fno-slp-vectorize for the units of its CONV_SRCS only"""
    with open(os.path.join(CSRC, "Makefile")) as f:
        conv = re.search(r"^CONV_SRCS = (.*)$", f.read().replace("\\\n", " "), re.M).group(1).split()
    assert "conv_ws.hip" in conv, conv
    cmd = [HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-w"] + \
        (["-fno-slp-vectorize"] if unit + ".hip" in conv else []) + \
        ["-Rpass-analysis=kernel-resource-usage", "-c", unit + ".hip", "-o", os.devnull]
    err = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True, check=True).stderr
    out, name = {}, None
    for line in err.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
            continue
        for key, pat in (("vgprs", r" VGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("spill", r"VGPRs Spill: (\d+)")):
            m = re.search(pat, line)
            if m and name:
                out[name][key] = int(m.group(1))
    return out


def load_tree(tree_file):
    with open(os.path.join(DATA, tree_file)) as f:
        return json.load(f)


def level_weights_for(tree_file, hierarchical):
    if not hierarchical:
        return synth.README_LEVEL_WEIGHTS_FLAT
    return synth.README_LEVEL_WEIGHTS_TL if tree_file == "class_tree_tl.json" else EXT_WEIGHTS


def load_golden(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)


def build_model(models_mod, kind, hier, tree, size):
    """Same constructor calls for the oracle and the product (same API)."""
    if kind == "unet":
        m = models_mod.UNet(size=size, n_channels=3, hierarchy=tree, model_type=1 if hier else 0)
    else:
        m = models_mod.HighResolutionNet(hrnet_w48_config(), hierarchy=tree, model_type=1 if hier else 0)
    return synth.fill_state_dict(m)


def rel_err(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-12))


# ---- convolution arithmetic modes of the parity tests -------------------------------------------------------------
# "auto"    the default policy with the default routing thresholds (small cases: mostly the exact-fp32 kernels)
# "f32"     exact-fp32 MFMA kernels everywhere
# "fp16x2"  the split-precision kernels everywhere, routing thresholds lowered to 1 tile: wave-specialised single launches,
#           block-synchronous halo-patch / pgroup launches, im2col kernels, nine-tap + tap-per-block weight gradients
# "auto_ws" the default policy with the thresholds lowered: what the 620x620 headline runs (wave-specialised GROUP
#           launches of the parallel branches, fp16x2 im2col kernels for 1x1 / stride-2 layers), at golden sizes
CONV_MODES = ["auto", "f32", "fp16x2", "auto_ws"]


class conv_mode:
    """context manager: sets model.conv_dtype and the library's routing thresholds for `mode`, counts launches per
    kernel family while active (self.counts after exit)"""

    def __init__(self, model, mode):
        self.model, self.mode, self.counts = model, mode, {}

    def __enter__(self):
        from hrseg_amd import _lib
        self.model.conv_dtype = {"auto_ws": "auto"}.get(self.mode, self.mode)
        if self.mode in ("fp16x2", "auto_ws"):
            _lib.tune(sp_ws_min_tiles=1, sp_patch_min_tiles=1, auto_min_pixels=1)
        # The 64-pixel HRNet ends in a 2 x 2-pixel branch whose BatchNorm normalises over 8 samples: with EVERY contraction forced
        # onto 22-bit operands its backward is chaotic, and with atomics on the summation order moves the gradients between two
        # basins ~1e-2 apart from run to run (tests/test_grad_noise_gpu.py; round 4 measured it on five library builds: the same
        # four cases 4/4, 3/4 or 1/4 green depending on nothing but kernel timing, 4/4 in deterministic mode on every build).
        # These cases compare KERNEL arithmetic with the reference, so they evaluate in deterministic mode; the default mode
        # (atomics, statistics in the conv epilogue) is what the UNet cases of the same modes, `auto`, the 256- and 620-pixel
        # tests and tests/test_tape_gpu.py run.
        self.det = (self.mode in ("fp16x2", "auto_ws") and type(self.model).__name__ == "HighResolutionNet"
                    and not _lib.deterministic())
        if self.det:
            _lib.set_deterministic(True)
        _lib.launch_count(None, reset=True)
        return self

    def __exit__(self, *exc):
        from hrseg_amd import _lib
        for fam in ("ws", "ws_group", "patch_sp", "sp_im2col", "sp_pgroup", "sp_group", "f32", "f32_group", "wgrad_sp",
                    "wgrad_f32", "wgrad_f32_group", "wgrad9", "wgrad_sp_group"):
            self.counts[fam] = _lib.launch_count(fam, reset=True)
        _lib.tune(sp_ws_min_tiles=0, sp_patch_min_tiles=0, auto_min_pixels=0)      # 0 = defaults
        if self.det:
            _lib.set_deterministic(False)
        return False

    def check_families(self, kind):
        """the case really ran the kernels its mode names"""
        c = self.counts
        if self.mode == "f32":
            assert c["ws"] + c["ws_group"] + c["patch_sp"] + c["sp_im2col"] + c["sp_pgroup"] + c["sp_group"] == 0, c
            assert c["f32"] + c["f32_group"] > 0 and c["wgrad9"] + c["wgrad_sp"] == 0, c
        elif self.mode == "fp16x2":
            assert c["f32"] + c["f32_group"] + c["wgrad_f32"] + c["wgrad_f32_group"] == 0, c
            assert c["ws"] > 0 and c["wgrad9"] > 0, c
            if kind == "hrnet":
                assert c["sp_im2col"] > 0 and c["wgrad_sp"] > 0 and c["wgrad_sp_group"] > 0, c
        elif self.mode == "auto_ws":
            assert c["ws"] + c["ws_group"] > 0 and c["wgrad9"] > 0, c
            if kind == "hrnet":
                assert c["ws_group"] > 0 and c["sp_im2col"] + c["sp_group"] > 0, c


# ---- opt-in extension `concat_prev_logits`: oracle side of tests/test_models_gpu.py::test_concat_prev_logits_...
def concat_model(models_mod, kind, size, tree):
    if kind == "unet":
        m = models_mod.UNet(size=size, n_channels=3, hierarchy=tree, model_type=1, concat_prev_logits=True)
    else:
        m = models_mod.HighResolutionNet(hrnet_w48_config(), hierarchy=tree, model_type=1, concat_prev_logits=True)
    return synth.fill_state_dict(m)


def concat_inputs(tree, size):
    import torch
    xn, tn = synth.synthetic_batch(tree, 2, size, seed=31, hierarchical=True, blob=4)
    return torch.from_numpy(xn), torch.from_numpy(tn)


def concat_oracle_results(kind, size):
    """the CPU oracle twin of the logit-concatenated model: train-mode logits and loss (fp32), the gradients of cond_stems
    in fp32 and fp64, level 0's head gradient in fp64 and with level 1's input DETACHED from level 0's logits, eval logits"""
    import torch
    from oracle import losses as OL
    from oracle import models as OM
    tree = load_tree("class_tree_tl.json")
    weights = level_weights_for("class_tree_tl.json", True)
    x, target = concat_inputs(tree, size)
    head0 = "heads.0.conv.weight" if kind == "unet" else "classifiers.0.weight"

    def run(model, xin, dtype):
        model.train()
        _, z = model(xin, type=1) if kind == "unet" else model(xin)
        loss = 0.0
        for L, a in enumerate(z):
            t = target[:, 4 * L:4 * L + 4].to(dtype)
            loss = loss + OL.cross_entropy_loss(a, t, logits_input=True, class_weight=weights[L]) + \
                OL.soft_dice_loss(a, t, logits_input=True, class_weight=weights[L])
        loss.backward()
        return z, loss

    out = {}
    om = concat_model(OM, kind, size, tree)
    out["param_names"] = np.array([n for n, _ in om.named_parameters()])
    z, loss = run(om, x, torch.float32)
    for L, a in enumerate(z):
        out[f"train_logits{L}"] = a.detach().numpy().copy()
    out["loss"] = np.float32(loss.item())
    for n, p in om.named_parameters():
        if n.startswith("cond_stems."):
            out["g32::" + n] = p.grad.numpy().copy()
    om.eval()
    with torch.no_grad():
        _, ze = om(x, type=1) if kind == "unet" else om(x)
    for L, a in enumerate(ze):
        out[f"eval_logits{L}"] = a.numpy().copy()
    o64 = concat_model(OM, kind, size, tree).double()
    run(o64, x.double(), torch.float64)
    for n, p in o64.named_parameters():
        if n.startswith("cond_stems.") or n == head0:
            out["g64::" + n] = p.grad.numpy().copy()

    class _Detach(torch.nn.Module):
        def __init__(self, conv):
            super().__init__()
            self.conv = conv

        def forward(self, xin):
            return self.conv(torch.cat([xin[:, :3], xin[:, 3:].detach()], dim=1))
    om2 = concat_model(OM, kind, size, tree)
    om2.cond_stems = torch.nn.ModuleList([_Detach(c) for c in om2.cond_stems])
    run(om2, x, torch.float32)
    out["gdet::" + head0] = dict(om2.named_parameters())[head0].grad.numpy().copy()
    return out


def load_concat_fixture(kind, size):
    path = os.path.join(GOLDEN, f"concat_oracle_{kind}_{size}.npz")
    return np.load(path, allow_pickle=False) if os.path.exists(path) else None
