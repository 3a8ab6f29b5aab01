"""Host side of the device input pipeline: decode + ragged uint8 collate in DataLoader workers, the host->device copy of
the next batch on a side stream, augmentation on the device (Data/augment.py).

The reference's SegDataset decodes, resizes and augments every sample on the CPU inside its DataLoader workers; here the
workers only decode, and a batch travels as two packed uint8 buffers (images, label maps) plus one int64 descriptor row
per sample (byte offset, H, W, channels), so the samples may all have their own size."""
from __future__ import annotations

import numpy as np
import torch


class RaggedBatch:
    """images: packed uint8 (HWC for 3 channels), desc [B,4] int64 (offset, H, W, channels 1|3); labels: packed uint8,
    ldesc [B,4] (offset, H, W, 1).  desc_host / ldesc_host always stay on the host (bounds checks, sizes)."""

    def __init__(self, src, desc, label, ldesc, desc_host=None, ldesc_host=None):
        self.src, self.desc, self.label, self.ldesc = src, desc, label, ldesc
        self.desc_host = desc if desc_host is None else desc_host
        self.ldesc_host = ldesc if ldesc_host is None else ldesc_host

    def __len__(self):
        return self.desc_host.shape[0]

    def pin_memory(self):
        return RaggedBatch(self.src.pin_memory(), self.desc.pin_memory(), self.label.pin_memory(), self.ldesc.pin_memory(),
                           self.desc_host, self.ldesc_host)

    def to(self, device, non_blocking=False):
        device = torch.device(device)
        if self.src.device.type == device.type and device.index in (None, self.src.device.index):
            return self
        return RaggedBatch(self.src.to(device, non_blocking=non_blocking), self.desc.to(device, non_blocking=non_blocking),
                           self.label.to(device, non_blocking=non_blocking), self.ldesc.to(device, non_blocking=non_blocking),
                           self.desc_host, self.ldesc_host)

    def record_stream(self, stream):
        for t in (self.src, self.desc, self.label, self.ldesc):
            t.record_stream(stream)


def _as_u8(a):
    a = torch.as_tensor(np.ascontiguousarray(a))
    if a.dtype != torch.uint8:
        raise TypeError("sources and label maps must be uint8")
    return a


def ragged_collate(samples):
    """[(image HxW or HxWx3 uint8, label HxW uint8), ...] -> RaggedBatch on the host"""
    imgs, labs = [], []
    desc, ldesc = [], []
    off = loff = 0
    for img, lab in samples:
        img, lab = _as_u8(img), _as_u8(lab)
        if img.dim() == 3 and img.shape[2] == 1:
            img = img[:, :, 0]
        if not (img.dim() == 2 or (img.dim() == 3 and img.shape[2] == 3)):
            raise ValueError(f"image of shape {tuple(img.shape)}: expected HxW or HxWx3")
        if lab.dim() != 2:
            raise ValueError(f"label map of shape {tuple(lab.shape)}: expected HxW")
        ch = 1 if img.dim() == 2 else 3
        desc.append([off, img.shape[0], img.shape[1], ch])
        ldesc.append([loff, lab.shape[0], lab.shape[1], 1])
        imgs.append(img.reshape(-1))
        labs.append(lab.reshape(-1))
        off += imgs[-1].numel()
        loff += labs[-1].numel()
    return RaggedBatch(torch.cat(imgs), torch.tensor(desc, dtype=torch.int64), torch.cat(labs),
                       torch.tensor(ldesc, dtype=torch.int64))


class PngPairDataset(torch.utils.data.Dataset):
    """(image, label map) file pairs decoded with PIL to uint8 arrays: images HxW or HxWx3 (other modes -> RGB), label
    maps HxW (other modes -> L)"""

    def __init__(self, input_paths, target_paths):
        if len(input_paths) != len(target_paths):
            raise ValueError("input_paths and target_paths differ in length")
        self.input_paths, self.target_paths = list(input_paths), list(target_paths)

    def __len__(self):
        return len(self.input_paths)

    def __getitem__(self, index):
        from PIL import Image
        with Image.open(self.input_paths[index]) as im:
            img = np.array(im if im.mode in ("L", "RGB") else im.convert("RGB"))
        with Image.open(self.target_paths[index]) as im:
            lab = np.array(im if im.mode in ("L", "P") else im.convert("L"))
        return img, lab


class DeviceAugmentLoader:
    """`for x, y in DeviceAugmentLoader(dataset, batch_size, shuffle, num_workers, augment)`: x [B,3,S,S] and y [B,C,S,S]
    device tensors from `augment` (a DeviceAugment).  The workers decode and collate uint8 only; batch k+1's host->device
    copy is issued on a side stream before batch k is handed out, so it overlaps the step that consumes batch k.
    with_sources=True yields (x, y, sources): the batch's device RaggedBatch rides along, for consumers that need every
    sample's own size (predictEval.predict_loop writing source-size label maps)."""

    def __init__(self, dataset, batch_size, shuffle=False, num_workers=0, augment=None, drop_last=False, with_sources=False):
        if augment is None:
            raise ValueError("DeviceAugmentLoader needs a DeviceAugment")
        self.dataset, self.augment = dataset, augment
        self.loader = torch.utils.data.DataLoader(dataset, batch_size=batch_size, shuffle=shuffle, num_workers=num_workers,
                                                  collate_fn=ragged_collate, pin_memory=torch.cuda.is_available(),
                                                  drop_last=drop_last)
        self.batch_size = batch_size
        self.with_sources = bool(with_sources)

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        device = self.augment.device
        side = torch.cuda.Stream(device=device)

        def upload(host):
            with torch.cuda.stream(side):
                dev = host.to(device, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(side)
            return dev, ev

        it = iter(self.loader)
        nxt = next(it, None)
        pending = upload(nxt) if nxt is not None else None
        while pending is not None:
            dev, ev = pending
            torch.cuda.current_stream(device).wait_event(ev)
            dev.record_stream(torch.cuda.current_stream(device))
            nxt = next(it, None)
            pending = upload(nxt) if nxt is not None else None       # overlaps the augmentation and the step below
            yield (*self.augment(dev), dev) if self.with_sources else self.augment(dev)
