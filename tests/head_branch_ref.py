"""CPU yardsticks of the HRNet head at branch resolution (tests/test_bilinear_bwd_multi_gpu.py,
tests/test_head_branch_res_gpu.py): the library's bilinear weights as matrices, footprint counts, and the fp64 evaluation
of upsample -> concat -> 1x1 convolution + bias -> training BatchNorm -> ReLU with its autograd."""
import numpy as np
import torch


def resize_scale(in_size, out_size, align):
    """csrc/elem.hip resize_scale, in fp32"""
    if align:
        return np.float32(in_size - 1) / np.float32(out_size - 1) if out_size > 1 else np.float32(0.0)
    return np.float32(in_size) / np.float32(out_size)


def bilinear_matrix(in_size, out_size, align):
    """[out_size, in_size] fp32 weights of one axis exactly as csrc/elem.hip src_index produces them (fp32 arithmetic; the
    two taps of an output add up where they fall on the same input, as the backward kernels add them)"""
    scale = resize_scale(in_size, out_size, align)
    m = np.zeros((out_size, in_size), dtype=np.float32)
    for o in range(out_size):
        if align:
            r = np.float32(scale * np.float32(o))
        else:
            r = np.float32(np.float32(scale * np.float32(np.float32(o) + np.float32(0.5))) - np.float32(0.5))
            if r < 0:
                r = np.float32(0.0)
        i0 = min(int(r), in_size - 1)
        i1 = i0 + (1 if i0 < in_size - 1 else 0)
        l1 = np.float32(r - np.float32(i0))
        l0 = np.float32(np.float32(1.0) - l1)
        m[o, i0] = np.float32(m[o, i0] + l0)
        m[o, i1] = np.float32(m[o, i1] + l1)
    return m


def bilinear_weights_2d(Hi, Wi, Hr, Wr, align):
    """[Hr, Wr, Hi, Wi] fp64 array of the fp32 products wy * wx the backward kernels multiply the gradient with"""
    my, mx = bilinear_matrix(Hi, Hr, align), bilinear_matrix(Wi, Wr, align)
    w = (my[:, None, :, None] * mx[None, :, None, :]).astype(np.float32)      # the fp32 product (wy * wx)
    return w.astype(np.float64)


def footprint_count(Hi, Wi, Hr, Wr, align):
    """largest number of output pixels with a non-zero weight on one input pixel"""
    w = bilinear_weights_2d(Hi, Wi, Hr, Wr, align)
    return int((w != 0).sum(axis=(0, 1)).max())


def upsample_fp64(t, Hr, Wr, align):
    """t [B, Hi, Wi, C] (any float dtype) -> [B, Hr, Wr, C] fp64 through the fp32 weights above"""
    B, Hi, Wi, C = t.shape
    w = torch.from_numpy(bilinear_weights_2d(Hi, Wi, Hr, Wr, align))
    return torch.einsum("oxiy,biyc->boxc", w, t.double().cpu())


def head_layer_fp64(xs, w, b, gamma, beta, eps, dz, align):
    """xs: NHWC tensors of the branches (the first at full resolution); w [Cout, Cin], b / gamma / beta [Cout], dz NHWC.
    torch-CPU fp64: z = relu(batchnorm_train(conv1x1(cat_j up(x_j)) + b)); -> z, [dz/dx_j], dz/dw given dz (all fp64, NHWC)"""
    import torch.nn.functional as F
    xs64 = [x.detach().double().cpu().permute(0, 3, 1, 2).contiguous().requires_grad_(True) for x in xs]
    w64 = w.detach().double().cpu().clone().requires_grad_(True)
    H, W = xs64[0].shape[2:]
    ups = [xs64[0]] + [F.interpolate(x, size=(H, W), mode="bilinear", align_corners=align) for x in xs64[1:]]
    y = F.conv2d(torch.cat(ups, 1), w64[:, :, None, None], b.detach().double().cpu())
    z = torch.relu(F.batch_norm(y, None, None, gamma.detach().double().cpu(), beta.detach().double().cpu(), True, 0.0, eps))
    z.backward(dz.detach().double().cpu().permute(0, 3, 1, 2))
    return (z.detach().permute(0, 2, 3, 1), [x.grad.permute(0, 2, 3, 1) for x in xs64], w64.grad)
