"""Torch-CPU restatement of the reference's training / evaluation transforms (test infrastructure, not product).

Steps 1-8 of the device input pipeline (Data/augment.py) written the way torchvision >= 0.17 computes them on tensors
(`ToTensor`, `Resize`, `GaussianBlur`, `ColorJitter`, `Normalize`, `hflip` / `vflip`, `affine` with NEAREST and a fill)
and the way SegDataset (Data/dataset.py:41-124, 418-470) composes them, with torch's own primitives where they exist:
`F.interpolate`, a dense 25x25 depthwise `conv2d` after reflect padding, `grid_sample`.  torchvision itself is not
available, so parity against it is not pinned; this module restates its documented formulas.

Per-sample parameters come from the same dict that Data.augment.sample_params draws (floats of one sample)."""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle.targets import is_leaf, level_order_names, node_masks, parent_map


def to_tensor(img_u8) -> torch.Tensor:
    """HxW or HxWx3 uint8 -> [3,H,W] fp32 in [0,1] (a 2-D source stacked to 3 channels, dataset.py:416-417)"""
    a = torch.as_tensor(np.ascontiguousarray(img_u8))
    if a.dim() == 2:
        a = torch.stack([a] * 3, dim=-1)
    return a.permute(2, 0, 1).contiguous().to(torch.float32).div(255)


def resize(x, S, antialias=False):
    return F.interpolate(x[None], size=(S, S), mode="bilinear", align_corners=False, antialias=antialias)[0]


def gaussian_kernel1d(sigma, ksize=25):
    half = (ksize - 1) * 0.5
    t = torch.linspace(-half, half, steps=ksize)
    pdf = torch.exp(-0.5 * (t / sigma).pow(2))
    return pdf / pdf.sum()


def gaussian_blur(x, sigma, ksize=25):
    """torchvision gaussian_blur: dense 2-D kernel = outer(k, k), reflect padding, depthwise conv2d"""
    k = gaussian_kernel1d(sigma, ksize)
    k2 = torch.mm(k[:, None], k[None, :])
    C = x.shape[0]
    pad = ksize // 2
    xp = F.pad(x[None], [pad, pad, pad, pad], mode="reflect")
    return F.conv2d(xp, k2.expand(C, 1, ksize, ksize), groups=C)[0]


def rgb_to_grayscale(x):
    r, g, b = x.unbind(dim=-3)
    return (0.2989 * r + 0.587 * g + 0.114 * b).to(x.dtype).unsqueeze(dim=-3)


def blend(a, m, ratio):
    ratio = float(ratio)
    return (ratio * a + (1.0 - ratio) * m).clamp(0, 1.0).to(a.dtype)


def adjust_brightness(x, f):
    return blend(x, torch.zeros_like(x), f)


def adjust_contrast(x, f):
    mean = torch.mean(rgb_to_grayscale(x), dim=(-3, -2, -1), keepdim=True)
    return blend(x, mean, f)


def adjust_saturation(x, f):
    return blend(x, rgb_to_grayscale(x), f)


def rgb2hsv(img):
    r, g, b = img.unbind(dim=-3)
    maxc = torch.max(img, dim=-3).values
    minc = torch.min(img, dim=-3).values
    eqc = maxc == minc
    cr = maxc - minc
    ones = torch.ones_like(maxc)
    s = cr / torch.where(eqc, ones, maxc)
    cr_divisor = torch.where(eqc, ones, cr)
    rc = (maxc - r) / cr_divisor
    gc = (maxc - g) / cr_divisor
    bc = (maxc - b) / cr_divisor
    hr = (maxc == r) * (bc - gc)
    hg = ((maxc == g) & (maxc != r)) * (2.0 + rc - bc)
    hb = ((maxc != g) & (maxc != r)) * (4.0 + gc - rc)
    h = hr + hg + hb
    h = torch.fmod((h / 6.0 + 1.0), 1.0)
    return torch.stack((h, s, maxc), dim=-3)


def hsv2rgb(img):
    h, s, v = img.unbind(dim=-3)
    i = torch.floor(h * 6.0)
    f = (h * 6.0) - i
    i = i.to(dtype=torch.int32)
    p = torch.clamp((v * (1.0 - s)), 0.0, 1.0)
    q = torch.clamp((v * (1.0 - s * f)), 0.0, 1.0)
    t = torch.clamp((v * (1.0 - s * (1.0 - f))), 0.0, 1.0)
    i = i % 6
    mask = i.unsqueeze(dim=-3) == torch.arange(6, device=i.device).view(-1, 1, 1)
    a1 = torch.stack((v, q, p, p, t, v), dim=-3)
    a2 = torch.stack((t, v, v, q, p, p), dim=-3)
    a3 = torch.stack((p, p, t, v, v, q), dim=-3)
    a4 = torch.stack((a1, a2, a3), dim=-4)
    return torch.einsum("...ijk, ...xijk -> ...xjk", mask.to(dtype=img.dtype), a4)


def adjust_hue(x, hue):
    hsv = rgb2hsv(x)
    h, s, v = hsv.unbind(dim=-3)
    h = (h + hue) % 1.0
    return hsv2rgb(torch.stack((h, s, v), dim=-3))


def color_jitter(x, order, b, c, s, h):
    for op in order:
        op = int(op)
        if op == 0:
            x = adjust_brightness(x, b)
        elif op == 1:
            x = adjust_contrast(x, c)
        elif op == 2:
            x = adjust_saturation(x, s)
        else:
            x = adjust_hue(x, h)
    return x


def inverse_affine_matrix(angle, translate, scale, shear):
    """torchvision _get_inverse_affine_matrix with center (0, 0) relative to the image centre, shear [shear, 0]"""
    rot = math.radians(angle)
    sx, sy = math.radians(shear), 0.0
    tx, ty = translate
    a = math.cos(rot - sy) / math.cos(sy)
    b = -math.cos(rot - sy) * math.tan(sx) / math.cos(sy) - math.sin(rot)
    c = math.sin(rot - sy) / math.cos(sy)
    d = -math.sin(rot - sy) * math.tan(sx) / math.cos(sy) + math.cos(rot)
    matrix = [d, -b, 0.0, -c, a, 0.0]
    matrix = [v / scale for v in matrix]
    matrix[2] += matrix[0] * (-tx) + matrix[1] * (-ty)
    matrix[5] += matrix[3] * (-tx) + matrix[4] * (-ty)
    return matrix


def affine_grid(matrix, S):
    """torchvision _gen_affine_grid for an S x S image: [1,S,S,2] normalised sampling grid"""
    theta = torch.tensor(matrix, dtype=torch.float32).reshape(1, 2, 3)
    d = 0.5
    base = torch.empty(1, S, S, 3, dtype=theta.dtype)
    base[..., 0].copy_(torch.linspace(-S * 0.5 + d, S * 0.5 + d - 1, steps=S))
    base[..., 1].copy_(torch.linspace(-S * 0.5 + d, S * 0.5 + d - 1, steps=S).unsqueeze_(-1))
    base[..., 2].fill_(1)
    rescaled = theta.transpose(1, 2) / torch.tensor([0.5 * S, 0.5 * S], dtype=theta.dtype)
    return base.view(1, S * S, 3).bmm(rescaled).view(1, S, S, 2)


def source_coords(grid, S):
    """grid_sample's unnormalised source coordinates (align_corners=False): (ix, iy) [S,S]"""
    g = grid[0]
    return (g[..., 0] + 1) * (S / 2) - 0.5, (g[..., 1] + 1) * (S / 2) - 0.5


def affine_nearest(img, matrix, fills):
    """torchvision affine(NEAREST) of [C,S,S] with one fill per channel (_apply_grid_transform)"""
    C, S, _ = img.shape
    grid = affine_grid(matrix, S)
    x = torch.cat([img[None], torch.ones(1, 1, S, S, dtype=img.dtype)], dim=1)
    out = F.grid_sample(x, grid, mode="nearest", padding_mode="zeros", align_corners=False)
    mask = out[:, -1:].expand(1, C, S, S) < 0.5
    out = out[:, :-1]
    fill = torch.tensor(fills, dtype=img.dtype).view(1, C, 1, 1).expand_as(out)
    out = torch.where(mask, fill, out)
    return out[0], grid


def name2pix(class_map):
    out = {}
    for row in class_map:
        v = row["pixel_val"]
        if v is None or str(v).strip().lower() in ("none", "nan", ""):
            continue
        out[row["class_name"]] = int(float(v))
    return out


def augment_sample(img_u8, label_u8, S, tree, class_map, model_type, p=None, target_antialias=True):
    """one sample through steps 1-8.  p: None = eval transforms, else a dict of this sample's draws (floats, order list,
    bools).  Returns x [3,S,S], y [C,S,S] and the exclusion masks (x_tie, y_excl) [S,S] of the comparison bars."""
    x = resize(to_tensor(img_u8), S)
    names = level_order_names(tree)
    masks = node_masks(tree, np.asarray(label_u8), name2pix(class_map))
    emit = names if model_type == 1 else [n for n in names if is_leaf(tree, n)]
    m = torch.stack([torch.from_numpy(masks[n].astype(np.float32)) for n in emit])
    cov = resize(m, S, antialias=target_antialias)
    near = ((cov - 0.5).abs() < 1e-5).any(dim=0)
    tie = torch.zeros(S, S, dtype=torch.bool)
    y = cov
    if p is not None:
        x = gaussian_blur(x, p["sigma"])
        x = color_jitter(x, p["order"], p["brightness"], p["contrast"], p["saturation"], p["hue"])
    x = (x - 0.5) / 0.5
    if p is not None:
        if p["hflip"]:
            x, y, near = x.flip(-1), y.flip(-1), near.flip(-1)
        if p["vflip"]:
            x, y, near = x.flip(-2), y.flip(-2), near.flip(-2)
        if p["affine"]:
            mat = inverse_affine_matrix(p["angle"], (p["tx"], p["ty"]), p["scale"], p["shear"])
            x, grid = affine_nearest(x, mat, [-1.0] * 3)
            fill0 = float(y[0].max())
            y, _ = affine_nearest(y, mat, [fill0] + [-1.0] * (y.shape[0] - 1))
            ix, iy = source_coords(grid, S)
            tie = (((ix - ix.floor()) - 0.5).abs() < 1e-4) | (((iy - iy.floor()) - 0.5).abs() < 1e-4)
            nw, _ = affine_nearest(near[None].float(), mat, [1.0 if abs(fill0 - 0.5) < 1e-5 else 0.0])
            near = nw[0] > 0.5
    y = torch.where(y < 0.5, 0.0, 1.0)
    if model_type == 1:
        par = parent_map(tree)
        idx = {n: i for i, n in enumerate(emit)}
        out = y.clone()
        for n, i in idx.items():
            if par[n] is not None:
                out[i] = torch.where(y[i] > 0, 1.0, torch.where(y[idx[par[n]]] > 0, 0.0, -1.0))
        y = out
    return x, y, tie, near | tie


def sample_dict(params, i):
    """sample i of a Data.augment.sample_params batch as plain Python values"""
    return {"sigma": float(params["sigma"][i]), "order": [int(v) for v in params["order"][i]],
            "brightness": float(params["brightness"][i]), "contrast": float(params["contrast"][i]),
            "saturation": float(params["saturation"][i]), "hue": float(params["hue"][i]),
            "hflip": bool(params["hflip"][i]), "vflip": bool(params["vflip"][i]), "affine": bool(params["affine"][i]),
            "angle": float(params["angle"][i]), "tx": float(params["tx"][i]), "ty": float(params["ty"][i]),
            "scale": float(params["scale"][i]), "shear": float(params["shear"][i])}
