"""Device mixing augmentation: ClassMix, CutMix and paste by tree node on the `(x, y)` a `DeviceAugment` hands out.

ClassMix / DACS cuts the pixels of a share of the classes out of one sample and lays them, labels included, over another;
CutMix does the same with a box.  Here the classes are nodes of the class tree ("all of a tooth" at level 0, "only enamel"
one level down), a pasted pixel takes the donor's whole ternary target column, and `max_shift > 0` lets the cut-out land
somewhere else (object paste).  The semantics are stated once, in include/hrseg.h ("mixing"); kernels: csrc/mix.hip.

The random draws are made on the host from a seeded torch.Generator into one small per-sample table; `last_params` reads it
back and `params=` injects one, as for `DeviceAugment`.  A whole `mix(x, y)` is at most 4 launches (3 for boxes), with no
synchronisation and no device-to-host copy.
"""
from __future__ import annotations

import math

import torch

from .. import ops
from .._lib import require_gpu
from .dataset import build_target_luts

# per-sample parameter table, laid out as HRSEG_MIX_* in include/hrseg.h
PARAMS = ops.MIX_PARAMS
P_FLAGS, P_DONOR, P_DX, P_DY, P_BOX = 0, 1, 2, 3, 4
APPLY, BOX = 1, 2
MODES = ("classmix", "cutmix")
_I32 = (-(1 << 31), (1 << 31) - 1)


def k_of_n_table(share):
    """[65] ints: how many of n present candidates are cut out; 0 for n = 0, else min(n, max(1, ceil(share * n)))"""
    share = float(share)
    if not 0.0 < share <= 1.0:
        raise ValueError(f"share {share} is not in (0, 1]")
    return [0] + [min(n, max(1, math.ceil(share * n))) for n in range(1, 65)]


def candidates(names, parent, model_type, level=0, nodes=None):
    """0/1 per emitted channel (names / parent of build_target_luts): the nodes at depth `level` of the tree, every leaf channel in
    flat mode (level must be 0), or exactly the channels named in `nodes`, at any level"""
    if nodes is not None:
        unknown = [n for n in nodes if n not in names]
        if unknown:
            raise ValueError(f"nodes {unknown} are no target channels (channels: {names})")
        if not nodes:
            raise ValueError("nodes is empty: nothing could ever be pasted")
        return [int(n in nodes) for n in names]
    level = int(level)
    if int(model_type) == 0:
        if level != 0:
            raise ValueError(f"level {level}: a flat model has its leaves at level 0 only")
        return [1] * len(names)
    depth = []
    for c, p in enumerate(parent):
        depth.append(0 if p < 0 else depth[p] + 1)          # (breadth first: a parent comes before its children)
    if level < 0 or level not in depth:
        raise ValueError(f"level {level}: the class tree has levels 0..{max(depth)}")
    return [int(d == level) for d in depth]


def rand_bbox(S, lam, cx, cy):
    """the CutMix paper's rand_bbox for an S x S image: (r0, c0, r1, c1), half-open"""
    cut = int(S * math.sqrt(1.0 - lam))
    c0, c1 = min(max(cx - cut // 2, 0), S), min(max(cx + cut // 2, 0), S)
    r0, r1 = min(max(cy - cut // 2, 0), S), min(max(cy + cut // 2, 0), S)
    return r0, c0, r1, c1


def sample_params(B, C, generator, mode="classmix", p=1.0, max_shift=0, donors=None, recipients=None, S=None):
    """one batch of draws: dict of tensors `apply` [B] bool, `donor` [B], `prio` [B,C], `dx` / `dy` [B], `boxed` [B] bool,
    `box` [B,4] (r0, c0, r1, c1).  apply is Bernoulli(p) on the samples in `recipients` (default all); donor is uniform over
    `donors` (default all) without the sample itself, and where that set is empty the sample is not applied."""
    if mode not in MODES:
        raise ValueError(f"mode '{mode}' is neither 'classmix' nor 'cutmix'")
    if mode == "cutmix" and S is None:
        raise ValueError("cutmix boxes need the image size S")
    donors = list(range(B)) if donors is None else [int(d) for d in donors]
    recipients = list(range(B)) if recipients is None else [int(r) for r in recipients]
    for what, idx in (("donors", donors), ("recipients", recipients)):
        bad = [i for i in idx if not 0 <= i < B]
        if bad:
            raise ValueError(f"{what} {bad} are no samples of a batch of {B}")
    g = generator
    apply = torch.rand(B, generator=g, dtype=torch.float64) < float(p)
    pick = torch.rand(B, generator=g, dtype=torch.float64)
    donor = torch.arange(B, dtype=torch.int64)
    for i in range(B):
        pool = [d for d in donors if d != i]
        if i not in recipients or not pool:
            apply[i] = False
        else:
            donor[i] = pool[min(int(float(pick[i]) * len(pool)), len(pool) - 1)]
    prio = torch.stack([torch.randperm(C, generator=g) for _ in range(B)]) if B else torch.zeros(0, C, dtype=torch.int64)
    m = int(max_shift)
    shift = torch.randint(-m, m + 1, (B, 2), generator=g, dtype=torch.int64)
    lam = torch.rand(B, generator=g, dtype=torch.float64)
    centre = torch.rand(B, 2, generator=g, dtype=torch.float64)
    box = torch.zeros(B, 4, dtype=torch.int64)
    if mode == "cutmix":
        for i in range(B):
            cx, cy = (min(int(float(v) * S), S - 1) for v in centre[i])
            box[i] = torch.tensor(rand_bbox(S, float(lam[i]), cx, cy))
    return {"apply": apply, "donor": donor, "prio": prio, "dx": shift[:, 0].clone(), "dy": shift[:, 1].clone(),
            "boxed": torch.full((B,), mode == "cutmix"), "box": box}


def pack_params(p, S, C):
    """params dict -> (params [B,16] int32, prio [B,C] int32), host tensors laid out as csrc/mix.hip reads them.  ValueError for
    a donor outside the batch, a prio row that is no permutation of 0..C-1, a box that is not ordered inside [0,S] and a shift
    that is no int32."""
    B = p["apply"].shape[0]
    prio = torch.as_tensor(p["prio"]).to(torch.int64)
    if tuple(prio.shape) != (B, C):
        raise ValueError(f"prio must be [{B},{C}], got {list(prio.shape)}")
    wrong = (prio.sort(dim=1).values != torch.arange(C)).any(dim=1).tolist()
    apply, boxed, donor, dxs, dys, boxes = (torch.as_tensor(p[k]).tolist() for k in ("apply", "boxed", "donor", "dx", "dy", "box"))
    rows = []
    for i in range(B):
        d, dx, dy = int(donor[i]), int(dxs[i]), int(dys[i])
        if not 0 <= d < B:
            raise ValueError(f"sample {i}: donor {d} is no sample of a batch of {B}")
        if wrong[i]:
            raise ValueError(f"sample {i}: prio {prio[i].tolist()} is not a permutation of 0..{C - 1}")
        for what, v in (("dx", dx), ("dy", dy)):
            if not _I32[0] <= v <= _I32[1]:
                raise ValueError(f"sample {i}: {what} {v} is no int32")
        r0, c0, r1, c1 = (int(v) for v in boxes[i])
        if boxed[i] and not (0 <= r0 <= r1 <= S and 0 <= c0 <= c1 <= S):
            raise ValueError(f"sample {i}: box rows {r0}..{r1}, columns {c0}..{c1} is not ordered inside [0,{S}]")
        rows.append([(APPLY if apply[i] else 0) | (BOX if boxed[i] else 0), d, dx, dy] + ([r0, c0, r1, c1] if boxed[i] else [0] * 4) +
                    [0] * (PARAMS - 8))
    return torch.tensor(rows, dtype=torch.int32).reshape(B, PARAMS), prio.to(torch.int32)


class DeviceMix:
    """`mix = DeviceMix(class_tree, class_map, model_type, mode="classmix", level=0); x2, y2 = mix(x, y)`: new tensors, x and y
    untouched.

    mode "classmix": of the candidate nodes present in the donor (at least min_pixels pixels), a `share` is cut out, chosen
    by a random priority; candidates are the nodes at depth `level` (every leaf in flat mode), or exactly `nodes=[names]`.
    mode "cutmix": a box after the CutMix paper's rand_bbox, lam ~ U(0,1).  p: the probability that a sample is mixed at all;
    max_shift > 0 moves the donor's content by up to that many pixels each way.  Channel order and names are
    `build_target_luts`', so `DeviceAugment(..., mix=mix)` can check that both speak of the same channels.

    After a call: last_params, last_mask [B,S,S] uint8, last_chosen [B] int64 bit sets, last_counts [B,C] int32 (None when
    every applied sample had a box), all but the first on the device; chosen_names() reads the sets back for logging;
    gather(t) re-applies the latest mix to any other [B,K,S,S] fp32 tensor (per-pixel weights) in one launch."""

    def __init__(self, class_tree, class_map, model_type=1, mode="classmix", level=0, nodes=None, share=0.5, min_pixels=1,
                 p=1.0, max_shift=0, seed=0, device="cuda"):
        require_gpu()
        if mode not in MODES:
            raise ValueError(f"mode '{mode}' is neither 'classmix' nor 'cutmix'")
        if int(min_pixels) < 1:
            raise ValueError(f"min_pixels {min_pixels} below 1")
        if not 0.0 <= float(p) <= 1.0:
            raise ValueError(f"p {p} is no probability")
        if int(max_shift) < 0:
            raise ValueError(f"max_shift {max_shift} is negative")
        self.mode, self.model_type, self.min_pixels, self.p, self.max_shift = mode, int(model_type), int(min_pixels), float(p), int(max_shift)
        self.names, self.parent, _, _ = build_target_luts(class_tree, class_map, model_type)
        self.cand = candidates(self.names, self.parent, model_type, level, nodes)
        self.k_of_n_host = k_of_n_table(share)
        self.device = torch.device(device)
        self.k_of_n = torch.tensor(self.k_of_n_host, dtype=torch.int32, device=self.device)
        self.generator = torch.Generator().manual_seed(int(seed))
        self.last_params = self.last_mask = self.last_chosen = self.last_counts = self._table = None

    def sample(self, B, donors=None, recipients=None, S=None):
        return sample_params(B, len(self.names), self.generator, self.mode, self.p, self.max_shift, donors, recipients, S)

    def pack_params(self, p, S):
        return pack_params(p, S, len(self.names))

    def __call__(self, x, y, params=None):
        if x.dim() != 4 or y.dim() != 4 or x.shape[0] != y.shape[0] or x.shape[2:] != y.shape[2:]:
            raise ValueError(f"x {tuple(x.shape)} and y {tuple(y.shape)} are no batch of images and targets of one size")
        if y.shape[1] != len(self.names):
            raise ValueError(f"y has {y.shape[1]} channels, the class tree gives {len(self.names)}")
        B, S = y.shape[0], y.shape[2]
        p = params if params is not None else self.sample(B, S=S)
        host, prio = self.pack_params(p, S)
        table, prio = host.to(y.device, non_blocking=True), prio.to(y.device, non_blocking=True)
        picks = bool(((host[:, P_FLAGS] & (APPLY | BOX)) == APPLY).any())           # (the host table: no device read)
        counts = ops.mix_counts(y) if picks else None
        mask, chosen = ops.mix_masks(y, counts, table, prio, self.k_of_n, self.cand, self.min_pixels)
        self.last_params, self.last_mask, self.last_chosen, self.last_counts, self._table = p, mask, chosen, counts, table
        return ops.mix_gather(x, mask, table), ops.mix_gather(y, mask, table)

    def gather(self, t):
        if self.last_mask is None:
            raise RuntimeError("gather() re-applies the latest mix: call the object first")
        return ops.mix_gather(t, self.last_mask, self._table)

    def chosen_names(self):
        """per sample, the names of the nodes that were cut out of its donor (a host read: for logging)"""
        if self.last_chosen is None:
            return []
        return [[n for c, n in enumerate(self.names) if (bits >> c) & 1] for bits in self.last_chosen.tolist()]
