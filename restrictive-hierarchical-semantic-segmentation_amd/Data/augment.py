"""Device input pipeline: the reference's training and evaluation transforms for a whole batch, in HIP.

Mirror of `transform_input4train` / `transform_input4test` / `transform_target` (Data/dataloaders.py:49-70) and the
flips, affine warp and threshold of `SegDataset.__getitem__` (Data/dataset.py:418-470), torchvision >= 0.17 tensor
semantics, for ragged uint8 sources: `x` [B,3,S,S] fp32 in [-1,1] and `y` [B,C,S,S] fp32 targets (ternary for
model_type 1, one-hot over the leaves for model_type 0), both on the device.  Kernels: csrc/augment.hip.

The random parameters are drawn on the host from a seeded torch.Generator with the reference's distributions (not its
Python `random` / global torch streams) into one small per-sample table; `last_params` reads it back and `params=`
injects one, so a test can drive the device path and a CPU restatement with identical draws.
"""
from __future__ import annotations

import math

import torch

from .. import ops
from .._lib import require_gpu
from .dataset import TargetEncoder
from .loader import RaggedBatch, ragged_collate

# per-sample parameter table, laid out as HRSEG_AUG_* in include/hrseg.h
PARAMS = 48
P_FLAGS, P_ORDER, P_BRIGHT, P_CONTRAST, P_SAT, P_HUE, P_THETA, P_TAPS = 0, 1, 5, 6, 8, 10, 12, 18
HFLIP, VFLIP, WARP = 1, 2, 4

# the reference's ranges (dataloaders.py:53-54 GaussianBlur / ColorJitter, dataset.py:457-461 affine)
SIGMA = (0.001, 2.0)
BRIGHTNESS, CONTRAST, SATURATION, HUE = (0.6, 1.4), (0.5, 1.5), (0.75, 1.25), (-0.01, 0.01)
ANGLE, TRANSLATE, SCALE, SHEAR = (-50.0, 50.0), (-20.0, 20.0), (0.85, 1.15), (-5.0, 5.0)
BLUR_SIZE = 25


def blur_taps(sigma: float) -> torch.Tensor:
    """normalised 1-D Gaussian taps of torchvision's 25x25 blur (the 2-D kernel is their outer product), fp32"""
    half = (BLUR_SIZE - 1) * 0.5
    t = torch.linspace(-half, half, steps=BLUR_SIZE)
    pdf = torch.exp(-0.5 * (t / sigma).pow(2))
    return pdf / pdf.sum()


def inverse_affine_matrix(angle, tx, ty, scale, shear):
    """torchvision _get_inverse_affine_matrix, centre (0, 0) = the image centre, shear [shear, 0]; Python doubles"""
    rot = math.radians(angle)
    sx, sy = math.radians(shear), 0.0
    a = math.cos(rot - sy) / math.cos(sy)
    b = -math.cos(rot - sy) * math.tan(sx) / math.cos(sy) - math.sin(rot)
    c = math.sin(rot - sy) / math.cos(sy)
    d = -math.sin(rot - sy) * math.tan(sx) / math.cos(sy) + math.cos(rot)
    m = [d, -b, 0.0, -c, a, 0.0]
    m = [v / scale for v in m]
    m[2] += m[0] * (-tx) + m[1] * (-ty)
    m[5] += m[3] * (-tx) + m[4] * (-ty)
    return m


def affine_theta(matrix, S):
    """the fp32 theta of torchvision's affine, transposed and divided by (S/2, S/2) as _gen_affine_grid does: [6]"""
    theta = torch.tensor(matrix, dtype=torch.float32).reshape(1, 2, 3)
    return (theta.transpose(1, 2) / torch.tensor([0.5 * S, 0.5 * S], dtype=torch.float32)).reshape(6)


def sample_params(B, generator, hflip=True, vflip=False, affine=True):
    """one batch of train-mode draws: dict of [B] tensors (float64 unless noted)"""
    def u(lo_hi):
        lo, hi = lo_hi
        return torch.rand(B, generator=generator, dtype=torch.float64) * (hi - lo) + lo
    p = {"sigma": u(SIGMA),
         "order": torch.stack([torch.randperm(4, generator=generator) for _ in range(B)]) if B else torch.zeros(0, 4, dtype=torch.int64),
         "brightness": u(BRIGHTNESS), "contrast": u(CONTRAST), "saturation": u(SATURATION), "hue": u(HUE)}
    flips = torch.rand(B, 2, generator=generator, dtype=torch.float64) > 0.5
    p["hflip"] = flips[:, 0] & bool(hflip)
    p["vflip"] = flips[:, 1] & bool(vflip)
    p["angle"], p["tx"], p["ty"], p["scale"], p["shear"] = u(ANGLE), u(TRANSLATE), u(TRANSLATE), u(SCALE), u(SHEAR)
    p["affine"] = torch.full((B,), bool(affine))
    return p


def pack_params(p, S):
    """params dict -> [B, PARAMS] fp32 table of csrc/augment.hip"""
    B = p["sigma"].shape[0]
    t = torch.zeros(B, PARAMS, dtype=torch.float32)
    for i in range(B):
        flags = (HFLIP if bool(p["hflip"][i]) else 0) | (VFLIP if bool(p["vflip"][i]) else 0) | \
                (WARP if bool(p["affine"][i]) else 0)
        t[i, P_FLAGS] = flags
        order = [int(v) for v in p["order"][i]]
        if sorted(order) != [0, 1, 2, 3]:
            raise ValueError(f"order {order} is not a permutation of 0..3")
        t[i, P_ORDER:P_ORDER + 4] = torch.tensor(order, dtype=torch.float32)
        c, s = float(p["contrast"][i]), float(p["saturation"][i])
        t[i, P_BRIGHT] = float(p["brightness"][i])
        t[i, P_CONTRAST], t[i, P_CONTRAST + 1] = c, 1.0 - c
        t[i, P_SAT], t[i, P_SAT + 1] = s, 1.0 - s
        t[i, P_HUE] = float(p["hue"][i])
        m = inverse_affine_matrix(float(p["angle"][i]), float(p["tx"][i]), float(p["ty"][i]), float(p["scale"][i]),
                                  float(p["shear"][i]))
        t[i, P_THETA:P_THETA + 6] = affine_theta(m, S)
        t[i, P_TAPS:P_TAPS + BLUR_SIZE] = blur_taps(float(p["sigma"][i]))
    return t


class DeviceAugment:
    """`aug = DeviceAugment(img_size, class_tree, class_map, model_type); x, y = aug(images, labels)` (lists of uint8
    HxW / HxWx3 arrays and HxW label maps) or `aug(batch)` (a RaggedBatch, host or device).

    train=True: the reference's transform_input4train + hflip / vflip / affine of the train SegDataset; train=False:
    transform_input4test (resize + normalise), targets resized and encoded, no randomness.  target_antialias=False
    selects torchvision < 0.17's plain bilinear resize of the masks.

    Partial labels (include/hrseg.h): internal_values / ignore_values as for TargetEncoder (`internal_values=h.values,
    ignore_values=[h.reject_val]` trains on the hedged maps of a `Hedge` h); fill="ignore" marks what the affine warp brings in
    from outside the source frame as unlabelled (-1 in every channel) instead of the reference's fill.  With none of the three
    the object launches `hrseg_augment_targets` as before.

    mix: a `DeviceMix` (Data/mix.py) over the same channels; with train=True the pair that comes back is the mixed one
    (ClassMix / CutMix across the batch; `mix.last_params` holds its draws).  None, or train=False: nothing changes."""

    def __init__(self, img_size, class_tree, class_map, model_type=1, train=True, hflip=True, vflip=False, affine=True,
                 target_antialias=True, seed=0, device="cuda", internal_values=None, ignore_values=(), fill="reference", mix=None):
        require_gpu()
        if fill not in ("reference", "ignore"):
            raise ValueError(f"fill '{fill}' is neither 'reference' nor 'ignore'")
        self.fill = fill
        self.size, self.train = int(img_size), bool(train)
        self.hflip, self.vflip, self.affine, self.target_antialias = bool(hflip), bool(vflip), bool(affine), bool(target_antialias)
        if self.train and self.size <= 12:
            raise ValueError("train mode needs img_size > 12 (the 25x25 blur pads by reflection)")
        self.encoder = TargetEncoder(class_tree, class_map, model_type, device=device, internal_values=internal_values,
                                     ignore_values=ignore_values)
        # the partial kernels run wherever the targets can hold an unknown: a table of them, or unlabelled corners
        self.partial = self.encoder.partial or fill == "ignore"
        if self.partial and self.encoder.unk_lut is None:
            self.encoder.unk_lut = torch.zeros_like(self.encoder.on_lut)
        self.device = self.encoder.on_lut.device
        self.names = self.encoder.names
        if mix is not None and list(mix.names) != list(self.names):
            raise ValueError(f"mix speaks of the channels {list(mix.names)}, the augment's encoder of {list(self.names)}: "
                             "build both from the same class tree, class map and model type")
        self.mix = mix
        self.generator = torch.Generator().manual_seed(int(seed))
        self.last_params = None

    def sample(self, B):
        return sample_params(B, self.generator, self.hflip, self.vflip, self.affine)

    def __call__(self, images, labels=None, params=None):
        if isinstance(images, RaggedBatch):
            batch = images
        else:
            if labels is None or len(labels) != len(images):
                raise ValueError("one label map per image")
            batch = ragged_collate(list(zip(images, labels)))
        B = len(batch)
        table = None
        if self.train:
            p = params if params is not None else self.sample(B)
            table = pack_params(p, self.size).to(self.device, non_blocking=True)
            self.last_params = p
        dev = batch.to(self.device, non_blocking=True)
        x = ops.augment_image(dev.src, dev.desc, dev.desc_host, table, self.size, self.train)
        enc = self.encoder
        if self.partial:
            y = ops.augment_targets_partial(dev.label, dev.ldesc, dev.ldesc_host, enc.on_lut, enc.unk_lut, enc.parent, table,
                                            self.size, self.train, self.target_antialias, self.fill == "ignore")
        else:
            y = ops.augment_targets(dev.label, dev.ldesc, dev.ldesc_host, enc.on_lut, enc.parent, table, self.size, self.train,
                                    self.target_antialias)
        if self.mix is not None and self.train:
            return self.mix(x, y)
        return x, y
