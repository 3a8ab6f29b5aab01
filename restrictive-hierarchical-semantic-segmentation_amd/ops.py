"""Functional layer over the C ABI: torch tensors in, torch tensors out.

Activations are NHWC fp32 tensors ``[B,H,W,C]`` whose last dim is contiguous;
a channel slice ``t[..., a:b]`` of a wider NHWC tensor is accepted wherever a
row stride ("ld") exists in the ABI.  Every function launches on torch's
current stream and never synchronises.  torch is used for allocation only.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from typing import NamedTuple

import torch

from . import _lib
from ._lib import ConvShape, call, ptr


def _ld(t):
    assert t.dim() == 4 and (t.stride(3) == 1 or t.shape[3] == 1), "NHWC tensor with contiguous channels expected"
    B, H, W, Cn = t.shape
    # strides of size-1 dims are arbitrary: take ld from the first dim that has extent
    if W > 1:
        ld = t.stride(2)
    elif H > 1:
        ld = t.stride(1)
    elif B > 1:
        ld = t.stride(0)
    else:
        ld = Cn
    assert (H == 1 or t.stride(1) == W * ld) and (B == 1 or t.stride(0) == H * W * ld) and ld >= Cn, \
        "only channel-sliced NHWC views are supported"
    return ld


def _npix(t):
    return t.shape[0] * t.shape[1] * t.shape[2]


def zeros(shape, dtype, device):
    """zero-filled tensor through the library's fill KERNEL (torch.zeros issues a memset, which a
    captured hipGraph replays out of order on this stack -- see tools/graph_bisect.py)"""
    t = torch.empty(shape, dtype=dtype, device=device)
    flat = t.view(-1).view(torch.float32)      # int64/float64 zeros are all-zero bits too
    call("hrseg_fill", ptr(flat), 0.0, flat.numel())
    return t


def clone(t):
    """device copy through the library's copy KERNEL (clone() of a contiguous tensor is a D2D memcpy
    node under graph capture; kept out of captured graphs like the memsets)"""
    t = t.contiguous()
    out = torch.empty_like(t)
    n = t.numel()
    if t.dtype == torch.float32 and n % 4 == 0 and n > 0:
        call("hrseg_copy", ptr(t), 4, ptr(out), 4, 0, n // 4, 4)
    else:
        out.copy_(t)
    return out


def empty_nhwc(B, H, W, Cn, like):
    return torch.empty((B, H, W, Cn), dtype=torch.float32, device=like.device)


def conv_out_size(h, k, s):
    pad = (k - 1) // 2
    return (h + 2 * pad - k) // s + 1


def _shape(x_shape, ldx, Cout, ldy, k, s, prec=0, gmax=None, residual=None, relu=False, stat=None, wpersist=False,
           x_split=False):
    """gmax: device scalar max|dy| of the gradient operand (fp16x2 data / weight gradients), see hrseg.h;
    residual / relu: the forward's fused epilogue y = relu?(conv + bias + residual) (inference with folded BatchNorm);
    stat: (device buffer of 256*2*Cout doubles, ctypes int) -- BatchNorm partial sums of the output from the epilogue"""
    B, Hi, Wi, Cin = x_shape
    sh = ConvShape(B=B, Hi=Hi, Wi=Wi, Cin=Cin, ldx=ldx, Ho=conv_out_size(Hi, k, s), Wo=conv_out_size(Wi, k, s),
                   Cout=Cout, ldy=ldy, ksize=k, stride=s, precision=prec, grad_absmax=ptr(gmax),
                   residual=ptr(residual), ldr=_ld(residual) if residual is not None else 0, relu=int(bool(relu)))
    if stat is not None:
        sh.stat_partial = ptr(stat[0])
        sh.stat_rows = C.pointer(stat[1])
    sh.w_persistent = int(bool(wpersist))
    sh.x_split = int(bool(x_split))        # x is stored pre-split (bn_fwd_group item "z_split"): hrseg.h
    return sh


def conv_x_split_ok(x_shapes, couts, k, s, prec):
    """may the producer of these convolutions' inputs (NHWC shapes, contiguous) store them pre-split?  (hrseg_conv_x_split_ok:
    every problem on the wave-specialised forward kernels and the nine-tap weight gradient)"""
    shapes = _shape_array([_shape(tuple(xs), xs[3], co, co, k, s, prec) for xs, co in zip(x_shapes, couts)])
    return _lib.conv_x_split_ok(shapes, len(x_shapes))


STAT_ROWS_MAX = 256          # include/hrseg.h hrseg_conv_shape_t.stat_partial: rows the caller provides


def _stat_buffer(cout, device):
    """(partial-sum buffer for the epilogue statistics of one convolution output, host int that receives the row count)"""
    return torch.empty(STAT_ROWS_MAX * 2 * cout, dtype=torch.float64, device=device), C.c_int(0)


# ------------------------------------------------------------------ convolution
_F16_CODES = (_lib.CONV_PRECISION["auto"], _lib.CONV_PRECISION["fp16x2"])
FP16X2_ACT_LIMIT = 65504.0


def absmax(x):
    """max|x| of an NHWC tensor as a 0-dim device tensor (NaN counts as +Inf): hrseg_absmax"""
    slots = zeros((64,), torch.float32, x.device)
    call("hrseg_absmax", ptr(x), _ld(x), _npix(x), x.shape[3], ptr(slots))
    return slots.max()


def _guard_prec(x, prec):
    """fp16x2 convolutions take their activation operand unscaled (include/hrseg.h): exact up to |x| = 65504, Inf / NaN
    results far beyond.  In deterministic mode (the verification mode: it may synchronise) the operand is range-checked
    and an out-of-range or non-finite tensor runs the exact-fp32 kernels instead; counted in `range_fallbacks`."""
    global range_fallbacks
    if not _lib.deterministic() or prec not in _F16_CODES or x.shape[3] % 4 or torch.cuda.is_current_stream_capturing() \
            or _lib.taping():
        return prec            # (a captured graph cannot read a value back: the guard is an eager-mode check)
    if float(absmax(x)) <= FP16X2_ACT_LIMIT:
        return prec
    range_fallbacks += 1
    return _lib.CONV_PRECISION["f32"]


range_fallbacks = 0


def _shape_array(shapes):
    return (ConvShape * len(shapes))(*shapes)


def conv_fwd_group(xs, ws, biases, k, s, couts, prec=0, residuals=None, relus=None, stats=False, wpersist=False, x_splits=None,
                   outs=None):
    """n independent convolutions (same k, s) in one launch when the library can group them.  xs NHWC, ws storage
    [Cout][k*k][Cin] (a channels_last [Cout,Cin,k,k] parameter, or its flat 1-D slot: hence `couts`).  `prec`:
    _lib.CONV_PRECISION code (all conv functions).  residuals / relus: the fused epilogue per problem (inference with folded
    BatchNorm); outs: per problem a buffer to write (a channel slice of a wider NHWC tensor is fine) or None = allocated.
    stats=True: -> (outs, [(partial, rows) or None per problem]): the BatchNorm partial sums of an output where the kernel
    that ran produces them in its epilogue (hrseg_conv_shape_t.stat_partial), else None"""
    _lib.ensure_scratch(xs[0].device)
    if _lib.deterministic() and any(_guard_prec(x, prec) != prec for i, x in enumerate(xs) if not (x_splits and x_splits[i])):
        prec = _lib.CONV_PRECISION["f32"]        # (one precision per grouped call)
    outs, shapes, sts = list(outs) if outs is not None else [None] * len(xs), [], []
    for i, (x, co) in enumerate(zip(xs, couts)):
        B, Hi, Wi, Cin = x.shape
        if outs[i] is None:
            outs[i] = empty_nhwc(B, conv_out_size(Hi, k, s), conv_out_size(Wi, k, s), co, x)
        y = outs[i]
        sts.append(_stat_buffer(co, x.device) if stats else None)
        shapes.append(_shape(x.shape, _ld(x), co, _ld(y), k, s, prec, residual=residuals[i] if residuals is not None else None,
                             relu=relus[i] if relus is not None else False, stat=sts[i], wpersist=wpersist,
                             x_split=bool(x_splits[i]) if x_splits else False))
    has_bias = any(b is not None for b in biases)
    call("hrseg_conv_fwd_group", len(xs), _lib.ptr_array(xs), _lib.ptr_array(ws),
         _lib.ptr_array(biases) if has_bias else None, _lib.ptr_array(outs), _shape_array(shapes))
    if stats:
        return outs, [(st[0], st[1].value) if st[1].value > 0 else None for st in sts]
    return outs


def conv_dgrad_group(dys, wts, x_shapes, k, s, outs, accumulate, prec=0, gmaxs=None, wpersist=False):
    """wts[i] = weight_transpose(w): [Cin][k*k][Cout]; outs[i] None -> allocated (accumulate ignored)"""
    _lib.ensure_scratch(dys[0].device)
    outs, acc, shapes = list(outs), list(accumulate), []
    for i, (dy, xs) in enumerate(zip(dys, x_shapes)):
        if outs[i] is None:
            outs[i] = empty_nhwc(xs[0], xs[1], xs[2], xs[3], dy)
            acc[i] = False
        shapes.append(_shape(xs, _ld(outs[i]), dy.shape[3], _ld(dy), k, s, prec, gmaxs[i] if gmaxs is not None else None,
                             wpersist=wpersist))
    call("hrseg_conv_dgrad_group", len(dys), _lib.ptr_array(dys), _lib.ptr_array(wts), _lib.ptr_array(outs),
         _lib.int_array([int(a) for a in acc]), _shape_array(shapes))
    return outs


def conv_wgrad_group(xs, dys, dws, k, s, prec=0, gmaxs=None, x_splits=None):
    """dws[i] (+)= ; dws[i] is the running gradient buffer [Cout][k*k][Cin]."""
    if _lib.deterministic() and any(_guard_prec(x, prec) != prec for i, x in enumerate(xs) if not (x_splits and x_splits[i])):
        prec = _lib.CONV_PRECISION["f32"]
    gm = gmaxs if gmaxs is not None else [None] * len(xs)
    sp = x_splits if x_splits else [False] * len(xs)
    shapes = _shape_array([_shape(x.shape, _ld(x), dy.shape[3], _ld(dy), k, s, prec, g, x_split=bool(q))
                           for x, dy, g, q in zip(xs, dys, gm, sp)])
    nbytes = _lib.conv_wgrad_workspace_bytes(shapes, len(xs)) if (prec and k == 3 and s == 1) else 0
    if nbytes:
        # split-precision 3x3 stride-1 problems: per-block partial sums in a workspace + ordered reduce (no atomics)
        ws = torch.empty(nbytes // 4, dtype=torch.float32, device=xs[0].device)
        call("hrseg_conv_wgrad_group_ws", len(xs), _lib.ptr_array(xs), _lib.ptr_array(dys), _lib.ptr_array(dws), shapes,
             ptr(ws), nbytes)
        return
    call("hrseg_conv_wgrad_group", len(xs), _lib.ptr_array(xs), _lib.ptr_array(dys), _lib.ptr_array(dws), shapes)


# The single-problem forms: a group of one through the grouped wrappers (there is no second implementation).
def conv_fwd(x, w, bias, k, s, out=None, cout=None, prec=0, residual=None, relu=False, stats=False, wpersist=False,
             x_split=False):
    """-> out, or with stats=True (out, (partial, rows) or None); pass `cout` when w is the flat 1-D parameter slot"""
    got = conv_fwd_group([x], [w], [bias], k, s, [cout if cout is not None else w.shape[0]], prec, [residual], [relu], stats,
                         wpersist, [x_split], [out])
    return (got[0][0], got[1][0]) if stats else got[0]


def conv_dgrad(dy, wt, x_shape, k, s, out=None, accumulate=False, prec=0, gmax=None, wpersist=False):
    return conv_dgrad_group([dy], [wt], [x_shape], k, s, [out], [accumulate], prec, [gmax], wpersist)[0]


def conv_wgrad(x, dy, dw, k, s, prec=0, gmax=None, x_split=False):
    conv_wgrad_group([x], [dy], [dw], k, s, prec, [gmax], [x_split])


def weight_transpose(w_store, Cout, taps, Cin, out=None):
    if out is None:
        out = torch.empty(Cin * taps * Cout, dtype=torch.float32, device=w_store.device)
    call("hrseg_weight_transpose", ptr(w_store), ptr(out), Cout, taps, Cin)
    return out


# ------------------------------------------------------------------ batch norm
_BN_MAX_CHUNKS = int(os.environ.get("HRSEG_BN_MAX_CHUNKS", "256"))     # pixel chunks (= blocks) per BatchNorm reduction


def _nchunks(npix, Cn):
    q = Cn // 4
    p = 1 if q >= 256 else 256 // q
    return max(1, min(_BN_MAX_CHUNKS, npix // (8 * p)))


# The single-problem forms: one item through the grouped launches (there is no second implementation).
def _bn_one(y=None, gamma=None, beta=None, rm=None, rv=None, nbt=None, momentum=0.0, eps=0.0, residual=None, relu=False, **kw):
    return [dict(y=y, gamma=gamma, beta=beta, rm=rm, rv=rv, nbt=nbt, momentum=momentum, eps=eps, residual=residual, relu=relu, **kw)]


def bn_train_coef(y, gamma, beta, running_mean, running_var, nbt, momentum, eps):
    """batch statistics of y -> coef [4][C] (mean, rstd, scale, shift); updates running stats."""
    return bn_fwd_group(_bn_one(y, gamma, beta, running_mean, running_var, nbt, momentum, eps), True, phases=3)[0][1]


def bn_fold(w, bias, gamma, beta, running_mean, running_var, eps, cout):
    """BatchNorm (running statistics) folded into the convolution in front of it -> (folded weight [same storage layout],
    folded bias [Cout]); hrseg_bn_fold"""
    w_f = torch.empty_like(w)
    b_f = torch.empty(cout, dtype=torch.float32, device=w.device)
    call("hrseg_bn_fold", ptr(w), ptr(bias), ptr(gamma), ptr(beta), ptr(running_mean), ptr(running_var), float(eps), cout,
         w.numel() // cout, ptr(w_f), ptr(b_f))
    return w_f, b_f


def bn_eval_coef(gamma, beta, running_mean, running_var, eps):
    return bn_fwd_group(_bn_one(None, gamma, beta, running_mean, running_var, eps=eps), False, phases=2)[0][1]


def bn_apply(y, coef, residual=None, relu=False, out=None):
    return bn_fwd_group(_bn_one(y, residual=residual, relu=relu, out=out, coef=coef), False, phases=4)[0][0]


def bn_bwd(dz, z, relu, y, coef, dgamma, dbeta, dres=None, dres_accumulate=False, eval_mode=False, dy_out=None):
    """-> dy (gradient w.r.t. the conv output), in a buffer of its own: dz stays as it was; dgamma/dbeta accumulate; dres (+)= g."""
    dy = dy_out if dy_out is not None else torch.empty(y.shape, dtype=torch.float32, device=y.device)
    return bn_bwd_group([dict(dz=dz, z=z if relu else None, relu=relu, y=y, coef=coef, dgamma=dgamma, dbeta=dbeta, dres=dres,
                              dres_accumulate=dres_accumulate, dy=dy)], eval_mode)[0]


def _sync_world(sync):
    import torch.distributed as dist
    return dist.get_world_size(sync)


_SYNC_BN_CHECKED = set()


def _check_sync_bn_shapes(sync, items, device):
    """synchronised BatchNorm all-reduces per-chunk partial sums and divides by stat_ranks * npix: every rank must bring the
    same pixel counts (same per-rank batch: `drop_last=True` in the loader).  Checked ONCE per distinct shape signature (one
    tiny all-reduce + readback), then cached: a ragged last batch raises here instead of hanging in a mismatched collective
    or weighting the statistics wrongly."""
    import torch.distributed as dist
    sig = (id(sync), tuple(_npix(it["y"]) for it in items))
    if sig in _SYNC_BN_CHECKED:
        return
    v = torch.tensor([len(items)] + [n for n in sig[1]], dtype=torch.int64, device=device)
    v = torch.cat([v, -v])
    dist.all_reduce(v, op=dist.ReduceOp.MAX, group=sync)
    h = v.tolist()
    k = len(h) // 2
    if any(h[i] != -h[k + i] for i in range(k)):
        raise RuntimeError("hrseg_amd sync_bn: the ranks bring different batch / image sizes to a synchronised BatchNorm "
                           f"(max over ranks {h[1:k]}, min {[-x for x in h[k + 1:]]}); use equal per-rank batches (drop_last=True)")
    _SYNC_BN_CHECKED.add(sig)


def bn_fwd_group(items, training, sync=None, phases=7):
    """items: list of dict(y, gamma, beta, rm, rv, nbt, momentum, eps, residual, relu[, out]);
    -> [(z, coef)] with three launches for the whole list (statistics, finalize, apply).
    phases (bit 0 statistics, bit 1 finalize / eval coefficients, bit 2 apply): z is allocated only for the apply phase, and
    the eval coefficients alone (training False, phases 2) need no y.
    sync (a process group, training only): cross-rank batch statistics -- the partial sums of all problems live in one
    buffer that is all-reduced between the statistics and the finalize phase (opt-in synchronised BN)."""
    n = len(items)
    arr = (_lib.BnFwd * n)()
    outs = []
    sync = sync if training else None
    ranks = _sync_world(sync) if sync is not None else 1
    pool, pool_off = None, 0
    if sync is not None:
        _check_sync_bn_shapes(sync, items, items[0]["y"].device)
        total = sum(_nchunks(_npix(it["y"]), it["y"].shape[3]) * 2 * it["y"].shape[3] for it in items)
        pool = torch.empty(total, dtype=torch.float64, device=items[0]["y"].device)
    for i, (a, it) in enumerate(zip(arr, items)):
        y = it["y"]
        Cn, npix = (y.shape[3], _npix(y)) if y is not None else (it["rm"].numel(), 0)
        dev = y.device if y is not None else it["rm"].device
        z = it.get("out")
        if z is None and phases & 4:
            z = torch.empty(y.shape, dtype=torch.float32, device=dev)
        coef = it.get("coef")                       # given: the apply phase alone, on coefficients an earlier call finalized
        if coef is None:
            coef = torch.empty(4 * Cn, dtype=torch.float32, device=dev)
        res = it.get("residual")
        a.y, a.ldy, a.npix, a.C = ptr(y), (_ld(y) if y is not None else 0), npix, Cn
        a.gamma, a.beta = ptr(it["gamma"]), ptr(it["beta"])
        a.running_mean, a.running_var = ptr(it["rm"]), ptr(it["rv"])
        a.num_batches_tracked = ptr(it["nbt"]) if training else None
        a.momentum, a.eps = float(it["momentum"]), float(it["eps"])
        a.stat_updates = int(it.get("repeat", 1))
        a.stat_div = int(it.get("stat_div", 1))
        a.residual, a.ldr, a.relu = ptr(res), (_ld(res) if res is not None else 0), int(it["relu"])
        a.z, a.ldz, a.coef = ptr(z), (_ld(z) if z is not None else 0), ptr(coef)
        a.relu_mask = ptr(it.get("relu_mask"))
        a.z_split = int(bool(it.get("z_split", False)))
        a.residual_split = int(bool(it.get("residual_split", False)))
        a.stat_ranks = ranks
        if training and it.get("partial") is not None:
            part, nch = it["partial"]                   # partial sums left by the convolution's epilogue (phases 6)
            a.partial, a.nchunks = ptr(part), int(nch)
            outs.append((z, coef, part))
        elif training:
            nch = _nchunks(npix, Cn)
            if pool is not None:
                part = pool[pool_off:pool_off + nch * 2 * Cn]
                pool_off += nch * 2 * Cn
            else:
                part = torch.empty(nch * 2 * Cn, dtype=torch.float64, device=y.device)
            a.partial, a.nchunks = ptr(part), nch
            outs.append((z, coef, part))
        else:
            a.partial, a.nchunks = None, 0
            outs.append((z, coef, None))
    if sync is not None:
        import torch.distributed as dist
        call("hrseg_bn_fwd_group_phases", n, arr, 1, 1)
        dist.all_reduce(pool, op=dist.ReduceOp.SUM, group=sync)
        call("hrseg_bn_fwd_group_phases", n, arr, 1, 6)
    elif phases != 7:           # (measurement switches of engine.py only)
        call("hrseg_bn_fwd_group_phases", n, arr, int(training), int(phases))
    else:
        call("hrseg_bn_fwd_group", n, arr, int(training))
    return [(z, coef) for z, coef, _ in outs]


def bn_bwd_group(items, eval_mode, sync=None):
    """items: list of dict(dz, z, relu, y, coef, dgamma, dbeta, dres, dres_accumulate[, dy]); dy is written
    in place over dz unless the item brings a buffer `dy` for it.  Three launches for the whole list.  sync: see bn_fwd_group (the backward's batch means become
    global; dgamma / dbeta receive this rank's share, so the gradient all-reduce sums them to the global value)."""
    n = len(items)
    arr = (_lib.BnBwd * n)()
    keep = []
    sync = None if eval_mode else sync
    ranks = _sync_world(sync) if sync is not None else 1
    pool, pool_off = None, 0
    if sync is not None:
        total = 0
        for it in items:
            Cn, npix, nseg = it["y"].shape[3], _npix(it["y"]), int(it.get("nseg", 1))
            nch = _nchunks(npix, Cn)
            nch = max(nseg, nch // nseg * nseg) if nseg > 1 else nch
            total += (nch + nseg) * 2 * Cn
        pool = zeros((total,), torch.float64, items[0]["y"].device)
    for i, (a, it) in enumerate(zip(arr, items)):
        y, dz, z = it["y"], it["dz"], it["z"]
        Cn, npix = y.shape[3], _npix(y)
        nseg = int(it.get("nseg", 1))
        nch = _nchunks(npix, Cn)
        if nseg > 1:                                  # chunks never straddle two segments
            nch = max(nseg, nch // nseg * nseg)
        if pool is not None:
            part = pool[pool_off:pool_off + (nch + nseg) * 2 * Cn]
            pool_off += (nch + nseg) * 2 * Cn
        else:
            part = torch.empty((nch + nseg) * 2 * Cn, dtype=torch.float64, device=y.device)
        keep.append(part)
        a.nseg = nseg
        a.sum_ranks = ranks
        dres = it.get("dres")
        a.dz, a.lddz = ptr(dz), _ld(dz)
        use_z = it["relu"] and z is not None      # z None: mask recomputed from y (forward without residual)
        a.z, a.ldz, a.relu = (ptr(z) if use_z else None), (_ld(z) if use_z else 0), int(it["relu"])
        a.y, a.ldy, a.coef = ptr(y), _ld(y), ptr(it["coef"])
        a.dgamma, a.dbeta = ptr(it["dgamma"]), ptr(it["dbeta"])
        dy = it.get("dy", dz)
        a.dy, a.lddy = ptr(dy), _ld(dy)
        a.dres, a.lddres = ptr(dres), (_ld(dres) if dres is not None else 0)
        a.dres_accumulate = int(bool(it.get("dres_accumulate", False)))
        a.npix, a.C, a.partial, a.nchunks = npix, Cn, ptr(part), nch
        a.dy_absmax = ptr(it.get("dy_absmax"))
        a.relu_mask = ptr(it.get("relu_mask"))
    if sync is not None:
        import torch.distributed as dist
        call("hrseg_bn_bwd_group_phases", n, arr, 0, 1)
        dist.all_reduce(pool, op=dist.ReduceOp.SUM, group=sync)
        call("hrseg_bn_bwd_group_phases", n, arr, 0, 6)
    else:
        call("hrseg_bn_bwd_group", n, arr, int(eval_mode))
    return [it.get("dy", it["dz"]) for it in items]


# ------------------------------------------------------------------ pooling / resize / glue
def maxpool2_fwd(x):
    B, H, W, Cn = x.shape
    y = empty_nhwc(B, H // 2, W // 2, Cn, x)
    call("hrseg_maxpool2_fwd", ptr(x), _ld(x), ptr(y), _ld(y), B, H, W, Cn)
    return y


def maxpool2_bwd(x, dy, dx=None, accumulate=False):
    B, H, W, Cn = x.shape
    if dx is None:
        dx = torch.empty(x.shape, dtype=torch.float32, device=x.device)
        accumulate = False
    call("hrseg_maxpool2_bwd", ptr(x), _ld(x), ptr(dy), _ld(dy), ptr(dx), _ld(dx), int(accumulate), B, H, W, Cn)
    return dx


def bilinear_fwd(x, out, Hr, Wr, py=0, px=0, align_corners=True, accumulate=False, relu=False):
    """resize x to Hr x Wr and place it at (py,px) of `out` (NHWC view, may be a channel slice)."""
    B, Hi, Wi, Cn = x.shape
    call("hrseg_bilinear_fwd", ptr(x), _ld(x), B, Hi, Wi, Cn, ptr(out), _ld(out), out.shape[1], out.shape[2], Hr, Wr,
         py, px, int(align_corners), int(accumulate), int(relu))
    return out


def bilinear_bwd(dout, x_shape, Hr, Wr, py=0, px=0, align_corners=True, din=None, accumulate=False):
    B, Hi, Wi, Cn = x_shape
    if din is None:
        din = empty_nhwc(B, Hi, Wi, Cn, dout)
        accumulate = False
    call("hrseg_bilinear_bwd", ptr(dout), _ld(dout), B, Hi, Wi, Cn, ptr(din), _ld(din), dout.shape[1], dout.shape[2],
         Hr, Wr, py, px, int(align_corners), int(accumulate))
    return din


def fuse_sum(same, lows, relu=True, align_corners=True):
    """relu?(sum of same-resolution NHWC tensors + sum of bilinearly up-sampled low-resolution ones) in one pass"""
    ref = same[0]
    B, H, W, Cn = ref.shape
    out = torch.empty(ref.shape, dtype=torch.float32, device=ref.device)
    call("hrseg_fuse_sum", len(same), _lib.ptr_array(same), _lib.int_array([_ld(t) for t in same]), len(lows),
         _lib.ptr_array(lows) if lows else None, _lib.int_array([_ld(t) for t in lows]) if lows else None,
         _lib.int_array([t.shape[1] for t in lows]) if lows else None, _lib.int_array([t.shape[2] for t in lows]) if lows else None,
         ptr(out), _ld(out), B, H, W, Cn, int(align_corners), int(relu))
    return out


HEAD_MIX_MAX_CHUNKS = 1024       # pixel chunks (= blocks = partial-sum rows) of hrseg_head_mix


def head_mix(y, lows, bias=None, align_corners=True, stats=True):
    """y += sum of the bilinearly up-sampled lows + bias, in place (hrseg_head_mix: the HRNet head at branch resolution).
    stats=True: -> (partial, rows), the BatchNorm partial sums of the result for bn_fwd_group's item "partial"; else None"""
    B, H, W, Cn = y.shape
    npix, q = B * H * W, Cn // 4
    nch = max(1, min(HEAD_MIX_MAX_CHUNKS, npix // (4 * min(16, 1024 // q))))       # at least 4 pixels per pixel lane (csrc/elem.hip head_mix_lanes)
    part = torch.empty(nch * 2 * Cn, dtype=torch.float64, device=y.device) if stats else None
    call("hrseg_head_mix", ptr(y), _ld(y), ptr(bias), len(lows), _lib.ptr_array(lows) if lows else None,
         _lib.int_array([_ld(t) for t in lows]) if lows else None, _lib.int_array([t.shape[1] for t in lows]) if lows else None,
         _lib.int_array([t.shape[2] for t in lows]) if lows else None, B, H, W, Cn, int(align_corners), ptr(part), nch)
    return (part, nch) if stats else None


def bilinear_bwd_multi(dout, sizes, align_corners=True, want_absmax=False):
    """the transpose of the bilinear resize of dout onto every (Hi, Wi) of `sizes` (1..3) in one launch, all channels each:
    -> (dins, absmax [n][64] or None: max|din| per target as hrseg_absmax leaves it)"""
    B, H, W, Cn = dout.shape
    dins = [empty_nhwc(B, h, w, Cn, dout) for h, w in sizes]
    amax = zeros((len(sizes), 64), torch.float32, dout.device) if want_absmax else None
    call("hrseg_bilinear_bwd_multi", ptr(dout), _ld(dout), B, H, W, Cn, len(sizes), _lib.ptr_array(dins),
         _lib.int_array([_ld(t) for t in dins]), _lib.int_array([h for h, _ in sizes]), _lib.int_array([w for _, w in sizes]),
         int(align_corners), ptr(amax))
    return dins, amax


def _col_blocks(buf, rows, widths):
    out, off = [], 0
    for w in widths:
        out.append(buf[off:off + rows * w])
        off += rows * w
    return out


def weight_cols_gather(w_store, rows, widths):
    """column blocks of a weight [rows][sum(widths)] as contiguous [rows][width] matrices -> list of flat tensors (views of
    one buffer): the operands of a layer that is computed per input-channel block"""
    buf = torch.empty(rows * sum(widths), dtype=torch.float32, device=w_store.device)
    call("hrseg_weight_cols_gather", ptr(w_store), rows, sum(widths), len(widths), _lib.int_array(widths), ptr(buf))
    return _col_blocks(buf, rows, widths)


def weight_cols_scatter_add(blocks_buf, rows, widths, dw):
    """dw[rows][sum(widths)] += the column blocks laid end to end in blocks_buf (the reverse of weight_cols_gather)"""
    call("hrseg_weight_cols_scatter_add", ptr(blocks_buf), rows, sum(widths), len(widths), _lib.int_array(widths), ptr(dw))


def add(a, b, relu=False, out=None):
    if out is None:
        out = torch.empty(a.shape, dtype=torch.float32, device=a.device)
    call("hrseg_add", ptr(a), _ld(a), ptr(b), _ld(b), ptr(out), _ld(out), int(relu), _npix(a), a.shape[3])
    return out


def copy(src, dst, accumulate=False):
    call("hrseg_copy", ptr(src), _ld(src), ptr(dst), _ld(dst), int(accumulate), _npix(src), src.shape[3])
    return dst


def relu_bwd(dz, z, out=None):
    if out is None:
        out = torch.empty(z.shape, dtype=torch.float32, device=z.device)
    call("hrseg_relu_bwd", ptr(dz), _ld(dz), ptr(z), _ld(z), ptr(out), _ld(out), _npix(z), z.shape[3])
    return out


def nchw_to_nhwc(x, out=None):
    B, Cn, H, W = x.shape
    if out is None:
        out = empty_nhwc(B, H, W, Cn, x)
    call("hrseg_nchw_to_nhwc", ptr(x), ptr(out), Cn, B, Cn, H, W)
    return out


def nhwc_to_nchw(x):
    B, H, W, Cn = x.shape
    out = torch.empty((B, Cn, H, W), dtype=torch.float32, device=x.device)
    call("hrseg_nhwc_to_nchw", ptr(x), _ld(x), ptr(out), B, Cn, H, W)
    return out


def concat_image_logits(x, z):
    """NCHW image [B,Ci,H,W] + NCHW logits [B,C,H,W] -> NHWC [B,H,W,Ci+C] (the input of a logit-concatenated level pass)"""
    x, z = _c(x.float()), _c(z.float())
    B, Ci, H, W = x.shape
    Cz = z.shape[1]
    out = torch.empty((B, H, W, Ci + Cz), dtype=torch.float32, device=x.device)
    call("hrseg_nchw_to_nhwc", ptr(x), ptr(out), Ci + Cz, B, Ci, H, W)
    call("hrseg_nchw_to_nhwc", ptr(z), out.data_ptr() + 4 * Ci, Ci + Cz, B, Cz, H, W)
    return out


def nhwc_slice_to_nchw(g, c0):
    """channels [c0:] of an NHWC tensor as a contiguous NCHW tensor"""
    B, H, W, Cn = g.shape
    assert g.is_contiguous()
    out = torch.empty((B, Cn - c0, H, W), dtype=torch.float32, device=g.device)
    call("hrseg_nhwc_to_nchw", g.data_ptr() + 4 * c0, Cn, ptr(out), B, Cn - c0, H, W)
    return out


def accumulate_flat(dst, src):
    """dst += src for two contiguous fp32 tensors of the same size (the copy kernel's accumulate form)"""
    n = dst.numel()
    assert src.numel() == n and dst.is_contiguous() and src.is_contiguous()
    if n % 4 == 0 and n > 0:
        call("hrseg_copy", ptr(src), 4, ptr(dst), 4, 1, n // 4, 4)
    else:
        dst.add_(src)
    return dst


def encode_targets(label, on_lut, parent):
    """label [B,H,W] uint8 (device), on_lut [256] int64 bit table (device), parent list[int] -> [B,C,H,W] fp32"""
    assert label.dtype == torch.uint8 and label.is_cuda and label.dim() == 3
    assert on_lut.dtype == torch.int64 and on_lut.numel() == 256 and on_lut.is_cuda
    label = label.contiguous()
    B, H, W = label.shape
    Cn = len(parent)
    out = torch.empty((B, Cn, H, W), dtype=torch.float32, device=label.device)
    call("hrseg_encode_targets", ptr(label), ptr(on_lut), _lib.int_array(list(parent)), ptr(out), B, Cn, H * W)
    return out


def augment_workspace(B, S):
    """bytes of device workspace (image, targets) that the train-mode augment entry points need"""
    img, tgt = C.c_size_t(0), C.c_size_t(0)
    _lib.call_raw("hrseg_augment_workspace", int(B), int(S), C.byref(img), C.byref(tgt))
    return int(img.value), int(tgt.value)


def _check_ragged(buf, desc, desc_host, channels):
    """a packed uint8 buffer and its [B,4] int64 descriptor table (device) are consistent with the host copy"""
    assert buf.dtype == torch.uint8 and buf.is_cuda and buf.dim() == 1 and buf.is_contiguous()
    assert desc.dtype == torch.int64 and desc.is_cuda and desc.shape == desc_host.shape and desc.dim() == 2 and desc.shape[1] == 4
    n = buf.numel()
    for off, H, W, ch in desc_host.tolist():
        if ch not in channels or H < 1 or W < 1 or off < 0 or off + H * W * ch > n:
            raise ValueError(f"ragged descriptor (offset {off}, {H}x{W}, {ch} channels) does not fit a {n}-byte buffer")


def augment_image(src, desc, desc_host, params, S, train):
    """packed uint8 sources + [B,4] descriptors (device, and their host copy for the bounds check), [B,48] fp32 params
    (device; None in eval mode) -> x [B,3,S,S] fp32"""
    _check_ragged(src, desc, desc_host, (1, 3))
    B = desc.shape[0]
    x = torch.empty((B, 3, S, S), dtype=torch.float32, device=src.device)
    work, nbytes = None, 0
    if train:
        assert params is not None and params.is_cuda and params.dtype == torch.float32 and params.shape == (B, 48)
        nbytes = augment_workspace(B, S)[0]
        work = torch.empty(nbytes, dtype=torch.uint8, device=src.device)
    call("hrseg_augment_image", ptr(src), ptr(desc), ptr(params) if train else None, ptr(x), B, S, int(bool(train)),
         ptr(work), nbytes)
    return x


def augment_targets(label, desc, desc_host, on_lut, parent, params, S, warp, antialias=True):
    """packed uint8 label maps + [B,4] descriptors -> y [B,C,S,S] fp32 (resized per-node masks, thresholded, encoded as
    encode_targets; warp: flips + affine from params)"""
    _check_ragged(label, desc, desc_host, (1,))
    assert on_lut.dtype == torch.int64 and on_lut.numel() == 256 and on_lut.is_cuda
    B, Cn = desc.shape[0], len(parent)
    y = torch.empty((B, Cn, S, S), dtype=torch.float32, device=label.device)
    work, nbytes = None, 0
    if warp:
        assert params is not None and params.is_cuda and params.dtype == torch.float32 and params.shape == (B, 48)
        nbytes = augment_workspace(B, S)[1]
        work = torch.empty(nbytes, dtype=torch.uint8, device=label.device)
    call("hrseg_augment_targets", ptr(label), ptr(desc), ptr(on_lut), _lib.int_array(list(parent)),
         ptr(params) if warp else None, ptr(y), B, Cn, S, int(bool(warp)), int(bool(antialias)), ptr(work), nbytes)
    return y


def _check_lut(lut, what):
    assert lut.dtype == torch.int64 and lut.numel() == 256 and lut.is_cuda and lut.is_contiguous(), what


def encode_targets_partial(label, on_lut, unk_lut, parent):
    """encode_targets for partial labels (include/hrseg.h, "partial labels"): unk_lut [256] int64 bit table (device) of the
    channels a pixel value says nothing about"""
    assert label.dtype == torch.uint8 and label.is_cuda and label.dim() == 3
    _check_lut(on_lut, "on_lut")
    _check_lut(unk_lut, "unk_lut")
    label = label.contiguous()
    B, H, W = label.shape
    Cn = len(parent)
    out = torch.empty((B, Cn, H, W), dtype=torch.float32, device=label.device)
    call("hrseg_encode_targets_partial", ptr(label), ptr(on_lut), ptr(unk_lut), _lib.int_array(list(parent)), ptr(out), B, Cn,
         H * W)
    return out


def augment_workspace_partial(B, S):
    """bytes of device workspace the warp of augment_targets_partial needs"""
    tgt = C.c_size_t(0)
    _lib.call_raw("hrseg_augment_workspace_partial", int(B), int(S), C.byref(tgt))
    return int(tgt.value)


def augment_targets_partial(label, desc, desc_host, on_lut, unk_lut, parent, params, S, warp, antialias=True, fill_unknown=False):
    """augment_targets for partial labels: two coverages per channel, both thresholded sets warped; fill_unknown: out of
    frame every channel is unknown (-1) instead of the reference's fill"""
    _check_ragged(label, desc, desc_host, (1,))
    _check_lut(on_lut, "on_lut")
    _check_lut(unk_lut, "unk_lut")
    B, Cn = desc.shape[0], len(parent)
    y = torch.empty((B, Cn, S, S), dtype=torch.float32, device=label.device)
    work, nbytes = None, 0
    if warp:
        assert params is not None and params.is_cuda and params.dtype == torch.float32 and params.shape == (B, 48)
        nbytes = augment_workspace_partial(B, S)
        work = torch.empty(nbytes, dtype=torch.uint8, device=label.device)
    call("hrseg_augment_targets_partial", ptr(label), ptr(desc), ptr(on_lut), ptr(unk_lut), _lib.int_array(list(parent)),
         ptr(params) if warp else None, ptr(y), B, Cn, S, int(bool(warp)), int(bool(antialias)), int(bool(fill_unknown)),
         ptr(work), nbytes)
    return y


MIX_PARAMS = 16                     # HRSEG_MIX_PARAMS


def _check_mix_planes(who, t, what):
    """a [B,K,S,S] fp32 device tensor, contiguous, below 2^31 elements -> (B, K, S)"""
    if t.dim() != 4 or t.shape[2] != t.shape[3] or min(t.shape) < 1:
        raise ValueError(f"{who}: {what} must be [B,K,S,S], got {tuple(t.shape)}")
    if t.numel() >= 1 << 31:
        raise ValueError(f"{who}: {what} {tuple(t.shape)} has 2^31 elements or more")
    assert t.dtype == torch.float32 and t.is_cuda and t.is_contiguous(), f"{who}: {what} must be contiguous fp32 on the device"
    return t.shape[0], t.shape[1], t.shape[2]


def _check_mix_table(who, t, what, shape):
    assert t.dtype == torch.int32 and t.is_cuda and t.is_contiguous(), f"{who}: {what} must be contiguous int32 on the device"
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{who}: {what} must be {tuple(shape)}, got {tuple(t.shape)}")


def mix_counts(y):
    """y [B,C,S,S] fp32 targets -> counts [B,C] int32: pixels with y == 1 (include/hrseg.h, "mixing")"""
    B, Cn, S = _check_mix_planes("mix_counts", y, "y")
    if Cn > 64:
        raise ValueError(f"mix_counts: {Cn} channels, at most 64")
    counts = torch.empty((B, Cn), dtype=torch.int32, device=y.device)
    call("hrseg_mix_counts", ptr(y), ptr(counts), B, Cn, S * S)
    return counts


def mix_masks(y, counts, params, prio, k_of_n, cand, min_pixels=1):
    """y [B,C,S,S], counts [B,C] int32 or None (no applied sample without a box), params [B,16] / prio [B,C] / k_of_n [65]
    int32 (device), cand list of C 0/1 (host) -> (mask [B,S,S] uint8, chosen [B] int64 bit sets)"""
    B, Cn, S = _check_mix_planes("mix_masks", y, "y")
    if Cn > 64:
        raise ValueError(f"mix_masks: {Cn} channels, at most 64")
    if counts is not None:
        _check_mix_table("mix_masks", counts, "counts", (B, Cn))
    _check_mix_table("mix_masks", params, "params", (B, MIX_PARAMS))
    _check_mix_table("mix_masks", prio, "prio", (B, Cn))
    _check_mix_table("mix_masks", k_of_n, "k_of_n", (65,))
    if len(cand) != Cn:
        raise ValueError(f"mix_masks: {len(cand)} candidate flags for {Cn} channels")
    if int(min_pixels) < 1:
        raise ValueError(f"mix_masks: min_pixels {min_pixels} below 1")
    mask = torch.empty((B, S, S), dtype=torch.uint8, device=y.device)
    chosen = torch.empty((B,), dtype=torch.int64, device=y.device)
    call("hrseg_mix_masks", ptr(y), ptr(counts), ptr(params), ptr(prio), ptr(k_of_n), _lib.int_array([int(bool(v)) for v in cand]),
         int(min_pixels), ptr(mask), ptr(chosen), B, Cn, S)
    return mask, chosen


def mix_gather(t, mask, params, out=None):
    """out[b] = mask[b] ? t[donor(b)] moved by (dx, dy) : t[b], as bits; t [B,K,S,S] fp32, mask [B,S,S] uint8, params [B,16] int32"""
    B, K, S = _check_mix_planes("mix_gather", t, "the input")
    assert mask.dtype == torch.uint8 and mask.is_cuda and mask.is_contiguous(), "mix_gather: mask must be contiguous uint8 on the device"
    if tuple(mask.shape) != (B, S, S):
        raise ValueError(f"mix_gather: mask must be {(B, S, S)}, got {tuple(mask.shape)}")
    _check_mix_table("mix_gather", params, "params", (B, MIX_PARAMS))
    if out is None:
        out = torch.empty_like(t)
    else:
        assert out.dtype == torch.float32 and out.is_cuda and out.is_contiguous() and out.shape == t.shape
        if out is t or out.data_ptr() == t.data_ptr():
            raise ValueError("mix_gather: out must not alias the input (a donor can itself be a recipient)")
    call("hrseg_mix_gather", ptr(t), ptr(mask), ptr(params), ptr(out), B, K, S)
    return out


DECODE_MAX_LEVELS, DECODE_MAX_CHANNELS, DECODE_MAX_TOTAL = 8, 16, 64


def check_decode_tables(tables):
    """the limits of hrseg_decode_labels on a Data.decode.DecodeTables: <= 8 levels, <= 16 channels per level, <= 64 in
    all, child groups inside the next level, leaf pixel values in uint8 (ValueError otherwise; needs no GPU)"""
    Cs = list(tables.C)
    if not 1 <= len(Cs) <= DECODE_MAX_LEVELS:
        raise ValueError(f"decode_labels: {len(Cs)} levels, supported 1..{DECODE_MAX_LEVELS}")
    for L, n in enumerate(Cs):
        if not 1 <= n <= DECODE_MAX_CHANNELS:
            raise ValueError(f"decode_labels: level {L} has {n} channels, supported 1..{DECODE_MAX_CHANNELS}")
        if not (len(tables.first_child[L]) == len(tables.n_children[L]) == len(tables.pixel_val[L]) == n):
            raise ValueError(f"decode_labels: the tables of level {L} do not have {n} entries")
    if sum(Cs) > DECODE_MAX_TOTAL:
        raise ValueError(f"decode_labels: {sum(Cs)} channels over all levels, at most {DECODE_MAX_TOTAL}")
    for L, n in enumerate(Cs):
        for c in range(n):
            first, kids, pv = tables.first_child[L][c], tables.n_children[L][c], tables.pixel_val[L][c]
            if kids == 0:
                if not 0 <= pv <= 255:
                    raise ValueError(f"decode_labels: leaf (level {L}, channel {c}) has pixel value {pv}")
            elif L + 1 >= len(Cs) or kids < 0 or first < 0 or first + kids > Cs[L + 1]:
                raise ValueError(f"decode_labels: children [{first}, {first + kids}) of (level {L}, channel {c}) are not "
                                 "channels of the next level")


def _decode_tree_struct(tables):
    t = _lib.DecodeTree()
    for L, n in enumerate(tables.C):
        for c in range(n):
            t.first_child[L][c] = int(tables.first_child[L][c])
            t.n_children[L][c] = int(tables.n_children[L][c])
            t.pixel_val[L][c] = int(tables.pixel_val[L][c])
    t.root_softmax = int(bool(tables.root_softmax))
    return t


def _decode_logits(who, logits, tables, view=None):
    """one set of per-level logits of `who` (a list of [N,C_L,S,S] fp32 device tensors, or one tensor; `view`: its number
    in an ensemble, for the messages) against the tables -> (the tensors, contiguous; N; S)"""
    has, at = (f"view {view} has ", f"view {view}, ") if view is not None else ("", "")
    logits = [logits] if torch.is_tensor(logits) else list(logits)
    if len(logits) != len(tables.C):
        raise ValueError(f"{who}: {has}{len(logits)} logit levels for a {len(tables.C)}-level table")
    if logits[0].dim() != 4:
        raise ValueError(f"{who}: {at}level 0 logits of shape {tuple(logits[0].shape)}, expected 4 dimensions")
    N, S = logits[0].shape[0], logits[0].shape[2]
    for L, z in enumerate(logits):
        if z.dim() != 4 or tuple(z.shape) != (N, tables.C[L], S, S):
            raise ValueError(f"{who}: {at}level {L} logits of shape {tuple(z.shape)}, expected {(N, tables.C[L], S, S)}")
        if not z.is_cuda or z.dtype != torch.float32:
            raise ValueError(f"{who}: {at}level {L}: logits must be fp32 device tensors")
    return [_c(z) for z in logits], N, S


def _decode_desc(who, desc, desc_host, B=None):
    """the [B,4] int64 label descriptors (byte offset, H, W, 1) of `who`, on the device and their host copy (B: from the host
    copy where None), and the ragged rows against the densely packed buffer they describe -> its bytes"""
    if not torch.is_tensor(desc_host) or desc_host.dim() != 2 or desc_host.shape[1] != 4:
        raise ValueError(f"{who}: the host descriptor table must be [B,4] int64")
    B = desc_host.shape[0] if B is None else B
    if desc.dtype != torch.int64 or not desc.is_cuda or not tuple(desc.shape) == tuple(desc_host.shape) == (B, 4):
        raise ValueError(f"{who}: the descriptor tables must be [{B},4] int64, one on the device and its host copy")
    rows = desc_host.tolist()
    n = sum(H * W for _, H, W, _ in rows)
    for off, H, W, ch in rows:
        if ch != 1 or H < 1 or W < 1 or off < 0 or off + H * W > n:
            raise ValueError(f"ragged descriptor (offset {off}, {H}x{W}, {ch} channels) does not fit a {n}-byte label buffer")
    return n


def _decode_outputs(n, device, want_confidence):
    """the packed uint8 labels and, when asked for, the packed fp32 confidence (else None) of n pixels"""
    return (torch.empty(n, dtype=torch.uint8, device=device),
            torch.empty(n, dtype=torch.float32, device=device) if want_confidence else None)


def decode_labels(logits, tables, desc, desc_host, want_confidence=False):
    """per-level logits (list of [B,C_L,S,S] fp32 device tensors, or one tensor) + a Data.decode.DecodeTables + [B,4] int64
    label descriptors (byte offset, H, W, 1; device, and their host copy for the bounds check) -> the packed uint8
    label maps (sum of H*W bytes: a densely packed batch), each at its own H x W, plus the packed fp32 path confidence
    when asked for (else None).  The tables are read afresh on every call.  One launch, no synchronisation."""
    check_decode_tables(tables)
    logits, B, S = _decode_logits("decode_labels", logits, tables)
    n = _decode_desc("decode_labels", desc, desc_host, B)
    labels, conf = _decode_outputs(n, logits[0].device, want_confidence)
    call("hrseg_decode_labels", len(logits), _lib.ptr_array(logits), _lib.int_array(list(tables.C)),
         C.byref(_decode_tree_struct(tables)),
         ptr(desc), ptr(labels), ptr(conf), B, S)
    return labels, conf


HEDGE_MAX_PIXELS = 1 << 31


def check_hedge(hedge):
    """the rules of hrseg_decode_hedged on a Data.hedge.Hedge (or anything with its host tables `tables` -- a
    Data.decode.DecodeTables --, `tau` and `stop_val` per level and channel, `reject_val`): the limits of decode_labels, a
    tree model, thresholds in [0, 1], internal stop values and the reject value in uint8, no rejection (-1) only with all-zero
    level-0 thresholds, and no byte written by two of {leaves, internal nodes, rejection}.  The messages name the nodes
    (ValueError otherwise; needs no GPU)."""
    tables = hedge.tables
    check_decode_tables(tables)
    if tables.root_softmax:
        raise ValueError("decode_hedged: model_type 0 (a flat model) has no path to shorten")
    name = lambda L, c: f"'{tables.names[L][c]}'" if tables.names else f"(level {L}, channel {c})"      # noqa: E731
    reject = int(hedge.reject_val)
    if not -1 <= reject <= 255:
        raise ValueError(f"decode_hedged: reject value {reject} not in -1..255")
    owner = {} if reject < 0 else {reject: "the reject value"}
    for L, n in enumerate(tables.C):
        if len(hedge.tau[L]) != n or len(hedge.stop_val[L]) != n:
            raise ValueError(f"decode_hedged: the hedge tables of level {L} do not have {n} entries")
        for c in range(n):
            t = float(hedge.tau[L][c])
            if not 0.0 <= t <= 1.0:                                            # (a NaN fails both comparisons)
                raise ValueError(f"decode_hedged: threshold {t} of {name(L, c)} is not in 0..1")
            if L == 0 and t != 0.0 and reject < 0:
                raise ValueError(f"decode_hedged: {name(L, c)} has the level-0 threshold {t}, but there is no reject value")
            v = int(tables.pixel_val[L][c])
            if tables.n_children[L][c]:
                v = int(hedge.stop_val[L][c])
                if not 0 <= v <= 255:
                    raise ValueError(f"decode_hedged: internal node {name(L, c)} has the stop value {v}, not in 0..255")
            if v in owner:
                raise ValueError(f"decode_hedged: {owner[v]} and {name(L, c)} share the byte {v}")
            owner[v] = name(L, c)


def _hedge_struct(hedge):
    h = _lib.Hedge()
    for L, n in enumerate(hedge.tables.C):
        for c in range(n):
            h.tau[L][c] = float(hedge.tau[L][c])
            h.stop_val[L][c] = int(hedge.stop_val[L][c])
    h.reject_val = int(hedge.reject_val)
    return h


def decode_hedged(logits, hedge, desc, desc_host, want_confidence=False, stops=None):
    """decode_labels that stops at the parent where the child is unsure (hrseg_decode_hedged): per-level logits + a
    Data.hedge.Hedge + [B,4] int64 label descriptors (device, and their host copy) -> (packed uint8 labels, packed fp32
    confidence or None, stops [B, sum C + 2] int64: pixels ended per tree node in breadth-first order, then "rejected", then
    "nonfinite").  stops = the counters of an earlier call with the same batch size: they are added to.  The tables are
    read afresh on every call.  One launch, no synchronisation."""
    check_hedge(hedge)
    tables = hedge.tables
    logits, B, S = _decode_logits("decode_hedged", logits, tables)
    n = _decode_desc("decode_hedged", desc, desc_host, B)
    for b, (_, H, W, _) in enumerate(desc_host.tolist()):
        if H * W > HEDGE_MAX_PIXELS:
            raise ValueError(f"decode_hedged: sample {b}: {H}x{W} has more than 2^31 pixels")
    device = logits[0].device
    shape = (B, sum(tables.C) + 2)
    if stops is None:
        stops = zeros(shape, torch.int64, device)
    elif stops.dtype != torch.int64 or not stops.is_cuda or tuple(stops.shape) != shape or not stops.is_contiguous():
        raise ValueError(f"decode_hedged: stops must be a contiguous int64 device tensor of shape {shape}")
    labels, conf = _decode_outputs(n, device, want_confidence)
    call("hrseg_decode_hedged", len(logits), _lib.ptr_array(logits), _lib.int_array(list(tables.C)),
         C.byref(_decode_tree_struct(tables)), C.byref(_hedge_struct(hedge)), ptr(desc), ptr(labels), ptr(conf), ptr(stops), B, S)
    return labels, conf, stops


DECODE_MAX_VIEWS, DECODE_MAX_SIZE = 8, 32768
VIEW_HFLIP, VIEW_VFLIP = 1, 2


def _check_view_flags(what, flags):
    flags = [int(f) for f in flags]
    if not 1 <= len(flags) <= DECODE_MAX_VIEWS:
        raise ValueError(f"{what}: {len(flags)} views, supported 1..{DECODE_MAX_VIEWS}")
    for v, f in enumerate(flags):
        if not 0 <= f <= 3:
            raise ValueError(f"{what}: view {v} has flags {f}, supported 0..3 (HFLIP = 1, VFLIP = 2)")
    return flags


def flip_views(x, flags):
    """x [B,C,H,W] fp32 (device) + one flag word per view (0, VIEW_HFLIP, VIEW_VFLIP or both) -> [len(flags)*B,C,H,W]:
    block v is x mirrored as flags[v] says, bit for bit (the network inputs of the flip views of one scale, for ONE
    eval-mode forward).  One launch, no synchronisation."""
    flags = _check_view_flags("flip_views", flags)
    if x.dim() != 4 or x.dtype != torch.float32 or not x.is_cuda:
        raise ValueError(f"flip_views: x must be a [B,C,H,W] fp32 device tensor, got {tuple(x.shape)} {x.dtype} on {x.device}")
    B, Cn, H, W = x.shape
    if min(B, Cn, H, W) < 1 or len(flags) * x.numel() >= 1 << 31:
        raise ValueError(f"flip_views: {len(flags)} views of {tuple(x.shape)}: empty, or 2^31 output elements or more")
    x = _c(x)
    out = torch.empty((len(flags) * B, Cn, H, W), dtype=torch.float32, device=x.device)
    call("hrseg_flip_views", ptr(x), ptr(out), len(flags), _lib.int_array(flags), B, Cn, H, W)
    return out


def decode_views(views, tables, desc, desc_host, want_confidence=False):
    """decode_labels on the mean logit of an ensemble: views = [(per-level logits [B,C_L,S_v,S_v] fp32 device tensors, or one
    tensor; flags), ...] with flags 0, VIEW_HFLIP, VIEW_VFLIP or both (the network saw the image mirrored), the sizes
    S_v free per view -> (packed uint8 labels, packed fp32 confidence or None) exactly as decode_labels returns them.
    Contiguous batch slices z[v*B:(v+1)*B] of one batched forward are read in place.  One launch, no synchronisation."""
    flags = _check_view_flags("decode_views", [f for _, f in views])
    check_decode_tables(tables)
    flat, sizes, B = [], [], None
    for v, (logits, _) in enumerate(views):
        logits, N, S = _decode_logits("decode_views", logits, tables, v)
        B = N if B is None else B
        if N != B:
            raise ValueError(f"decode_views: view {v} has batch size {N}, view 0 has {B}")
        if not 1 <= S <= DECODE_MAX_SIZE:
            raise ValueError(f"decode_views: view {v} has size {S}, supported 1..{DECODE_MAX_SIZE}")
        flat += logits
        sizes.append(S)
    n = _decode_desc("decode_views", desc, desc_host, B)
    labels, conf = _decode_outputs(n, flat[0].device, want_confidence)
    call("hrseg_decode_views", len(views), _lib.int_array(sizes), _lib.int_array(flags), len(tables.C), _lib.ptr_array(flat),
         _lib.int_array(list(tables.C)), C.byref(_decode_tree_struct(tables)), ptr(desc), ptr(labels), ptr(conf), B)
    return labels, conf


WINDOW_MAX_ORIGINS, WINDOW_MAX_COVER = 64, 3


def check_window_axis(what, origins, n, S):
    """the rules of include/hrseg.h on the window origins along one canvas axis of length n (ValueError otherwise)"""
    o = [int(v) for v in origins]
    if not 1 <= len(o) <= WINDOW_MAX_ORIGINS:
        raise ValueError(f"{what}: {len(o)} window origins, supported 1..{WINDOW_MAX_ORIGINS}")
    if o[0] != 0 or o[-1] != n - S:
        raise ValueError(f"{what}: window origins {o[0]}..{o[-1]} do not run from 0 to {n} - {S}")
    for k in range(1, len(o)):
        if not o[k - 1] < o[k] <= o[k - 1] + S:
            raise ValueError(f"{what}: window origins {o[k - 1]}, {o[k]} are not increasing in steps of at most {S}")
    for k in range(len(o) - WINDOW_MAX_COVER):
        if o[k + WINDOW_MAX_COVER] < o[k] + S:
            raise ValueError(f"{what}: more than {WINDOW_MAX_COVER} windows cover coordinate {o[k + WINDOW_MAX_COVER]}")


def check_window_plan(what, plan, B, S):
    """a Data.decode.WindowPlan (or anything with its host tables `wdesc` [B,8] int64, `origins` int32, `nwindows`, `S`)
    against the rules of include/hrseg.h for B images and windows of S x S (ValueError otherwise; needs no GPU)"""
    if not 1 <= int(S) <= DECODE_MAX_SIZE:
        raise ValueError(f"{what}: window size {S}, supported 1..{DECODE_MAX_SIZE}")
    if int(plan.S) != int(S):
        raise ValueError(f"{what}: the plan was made for windows of {plan.S}, not {S}")
    wdesc, origins, N = plan.wdesc, plan.origins, int(plan.nwindows)
    if not (torch.is_tensor(wdesc) and wdesc.dtype == torch.int64 and not wdesc.is_cuda and tuple(wdesc.shape) == (B, 8)):
        raise ValueError(f"{what}: the window table must be a [{B},8] int64 host tensor")
    if not (torch.is_tensor(origins) and origins.dtype == torch.int32 and not origins.is_cuda and origins.dim() == 1):
        raise ValueError(f"{what}: the window origins must be a 1-D int32 host tensor")
    if N < B:
        raise ValueError(f"{what}: {N} windows for {B} images")
    org = origins.tolist()
    for m, (Hc, Wc, ny, nx, n0, oo, _, _) in enumerate(wdesc.tolist()):
        if Hc < S or Wc < S:
            raise ValueError(f"{what}: image {m} has a {Hc}x{Wc} canvas, smaller than a window of {S}")
        if not (1 <= ny <= WINDOW_MAX_ORIGINS and 1 <= nx <= WINDOW_MAX_ORIGINS):
            raise ValueError(f"{what}: image {m} has {ny}x{nx} windows, supported 1..{WINDOW_MAX_ORIGINS} per axis")
        if oo < 0 or oo + ny + nx > len(org):
            raise ValueError(f"{what}: the origins of image {m} ([{oo}, {oo + ny + nx})) lie outside the table of {len(org)}")
        if n0 < 0 or n0 + ny * nx > N:
            raise ValueError(f"{what}: windows [{n0}, {n0 + ny * nx}) of image {m} are not inside the {N} windows")
        check_window_axis(f"{what}: image {m} rows", org[oo:oo + ny], Hc, S)
        check_window_axis(f"{what}: image {m} columns", org[oo + ny:oo + ny + nx], Wc, S)


def _window_tables(plan, device):
    """the plan's two tables on the device (copied on every call, as the decode tables are read afresh on every call)"""
    return plan.wdesc.to(device), plan.origins.to(device)


def window_crops(src, desc, desc_host, plan, S):
    """packed uint8 sources + [B,4] descriptors (device, and their host copy) + a window plan -> x [N,3,S,S] fp32: window n
    is the eval-mode resize of its image to the plan's canvas, cut at the window's origin (what augment_image(..., False)
    gives where the canvas is one window).  One launch, no synchronisation."""
    _check_ragged(src, desc, desc_host, (1, 3))
    B = desc.shape[0]
    check_window_plan("window_crops", plan, B, S)
    wdesc, origins = _window_tables(plan, src.device)
    x = torch.empty((int(plan.nwindows), 3, S, S), dtype=torch.float32, device=src.device)
    call("hrseg_window_crops", ptr(src), ptr(desc), ptr(wdesc), ptr(origins), ptr(x), B, int(S), int(plan.nwindows))
    return x


def check_window_profile(what, profile, S):
    """the blend profile: S finite, strictly positive fp32 weights (validated on the host: a device tensor is copied back)"""
    if not (torch.is_tensor(profile) and profile.dtype == torch.float32 and tuple(profile.shape) == (S,)):
        raise ValueError(f"{what}: the blend profile must be a fp32 tensor of {S} entries")
    host = profile.detach().cpu()
    if not bool((torch.isfinite(host) & (host > 0)).all()):
        raise ValueError(f"{what}: the blend profile must be finite and strictly positive")


def decode_windows(logits, tables, plan, profile, desc, desc_host, want_confidence=False):
    """decode_labels on the blend of overlapping windows: per-level logits [N,C_L,S,S] of the plan's N windows (fp32 device
    tensors, or one tensor), a Data.decode.WindowPlan, the blend profile (S positive fp32 weights) and [B,4] label
    descriptors of the wanted sizes -> (packed uint8 labels, packed fp32 confidence or None) as decode_labels returns
    them.  No canvas-size tensor is built.  One launch, no synchronisation."""
    check_decode_tables(tables)
    logits, N, S = _decode_logits("decode_windows", logits, tables)
    n = _decode_desc("decode_windows", desc, desc_host)
    B = desc_host.shape[0]
    check_window_plan("decode_windows", plan, B, S)
    if int(plan.nwindows) != N:
        raise ValueError(f"decode_windows: logits of {N} windows for a plan of {plan.nwindows}")
    check_window_profile("decode_windows", profile, S)
    device = logits[0].device
    wdesc, origins = _window_tables(plan, device)
    profile = _c(profile.to(device))
    labels, conf = _decode_outputs(n, device, want_confidence)
    call("hrseg_decode_windows", len(logits), _lib.ptr_array(logits), _lib.int_array(list(tables.C)),
         C.byref(_decode_tree_struct(tables)), ptr(wdesc), ptr(origins), ptr(profile), ptr(desc), ptr(labels), ptr(conf), B, S, N)
    return labels, conf


SCORE_MAX_LEVELS, SCORE_MAX_CHANNELS, SCORE_MAX_TOTAL = 8, 16, 64
# pixels a lane / a wave / a block of hrseg_score_labels takes per step (HRSEG_SCORE_*_STEP of include/hrseg.h): the sizes
# around which the kernel changes path
SCORE_LANE_STEP, SCORE_WAVE_STEP, SCORE_BLOCK_STEP = 16, 1024, 4096
SCORE_MAX_PIXELS = 1 << 31


def check_score_tables(tables):
    """the limits of hrseg_score_labels on a Data.score.ScoreTables: <= 8 levels, <= 16 channels per level, <= 64 in all,
    and a path table whose bytes name channels of their levels (ValueError otherwise; needs no GPU).  The path rule is
    the one the kernels apply entry by entry: LM_PATH_ENTRY in csrc/labelmap_common.h is its device-side statement."""
    Cs = list(tables.C)
    if not 1 <= len(Cs) <= SCORE_MAX_LEVELS:
        raise ValueError(f"score_labels: {len(Cs)} levels, supported 1..{SCORE_MAX_LEVELS}")
    for L, n in enumerate(Cs):
        if not 1 <= n <= SCORE_MAX_CHANNELS:
            raise ValueError(f"score_labels: level {L} has {n} channels, supported 1..{SCORE_MAX_CHANNELS}")
    if sum(Cs) > SCORE_MAX_TOTAL:
        raise ValueError(f"score_labels: {sum(Cs)} channels over all levels, at most {SCORE_MAX_TOTAL}")
    K = [n + (1 if L else 0) for L, n in enumerate(Cs)]
    if list(tables.K) != K or list(tables.offsets) != [sum(k * k for k in K[:L]) for L in range(len(K))] or \
            tables.total != sum(k * k for k in K):
        raise ValueError("score_labels: K / offsets / total do not follow from C")
    path = list(tables.path)
    if len(path) != 256:
        raise ValueError(f"score_labels: the path table has {len(path)} entries, not 256")
    for v, e in enumerate(path):
        if e == 0:
            continue
        for L in range(8):
            c = (e >> (8 * L)) & 0xFF
            if (c != 0 if L >= len(Cs) else (c > Cs[L] or (L == 0 and c == 0))):
                raise ValueError(f"score_labels: path of pixel value {v} names channel {c - 1} at level {L}")


def score_labels(pred, pdesc, pdesc_host, gt, gdesc, gdesc_host, tables, out=None, per_image=True):
    """predicted against ground-truth label maps, both packed uint8 device buffers with [B,4] int64 descriptors (byte
    offset, H, W, 1; device, and their host copies for the bounds checks) of equal (H, W) per sample, + a
    Data.score.ScoreTables -> (counts [R, tables.total] int64, ignored [R, 2] int64), R = B (per_image) or 1: the level
    matrices (target, predicted) side by side, as hrseg_score_labels states them.  out = (counts, ignored) of an earlier
    call: both are added to.  One launch, no synchronisation."""
    check_score_tables(tables)
    _check_ragged(pred, pdesc, pdesc_host, (1,))
    _check_ragged(gt, gdesc, gdesc_host, (1,))
    prow, grow = pdesc_host.tolist(), gdesc_host.tolist()
    if len(prow) != len(grow) or not prow:
        raise ValueError(f"score_labels: {len(prow)} predicted maps against {len(grow)} ground-truth maps")
    for b, ((_, H, W, _), (_, gH, gW, _)) in enumerate(zip(prow, grow)):
        if (H, W) != (gH, gW):
            raise ValueError(f"score_labels: sample {b}: predicted map {H}x{W}, ground truth {gH}x{gW}")
        if H * W > SCORE_MAX_PIXELS:
            raise ValueError(f"score_labels: sample {b}: {H}x{W} has more than 2^31 pixels")
    B, R = len(prow), len(prow) if per_image else 1
    if gt.device != pred.device:
        raise ValueError("score_labels: the two buffers live on different devices")
    if out is None:
        counts, ignored = zeros((R, tables.total), torch.int64, pred.device), zeros((R, 2), torch.int64, pred.device)
    else:
        counts, ignored = out
        for t, shape in ((counts, (R, tables.total)), (ignored, (R, 2))):
            if t.dtype != torch.int64 or not t.is_cuda or tuple(t.shape) != shape or not t.is_contiguous():
                raise ValueError(f"score_labels: out must hold contiguous int64 device tensors of shapes {(R, tables.total)} and "
                                 f"{(R, 2)}")
    call("hrseg_score_labels", ptr(pred), ptr(pdesc), ptr(gt), ptr(gdesc), ptr(tables.device_lut(pred.device)), len(tables.C),
         _lib.int_array(list(tables.C)), ptr(counts), ptr(ignored), B, int(bool(per_image)))
    return counts, ignored


CONSENSUS_MAX_MEMBERS = 8           # HRSEG_CONSENSUS_MAX_MEMBERS
# pixels a lane / a block of hrseg_consensus_labels takes per step (HRSEG_CONSENSUS_*_STEP of include/hrseg.h)
CONSENSUS_LANE_STEP, CONSENSUS_BLOCK_STEP = 16, 4096
CONSENSUS_MAX_PIXELS = 1 << 31


def consensus_cells(nodes, M):
    """cells of a row of hrseg_consensus_labels counters, and the first cell of each block:
    (total, dict(ended, votes, area, both, abstain))"""
    P = M * (M - 1) // 2
    first = dict(ended=0, votes=nodes + 1, area=nodes + 1 + nodes * M, both=nodes + 1 + 2 * nodes * M,
                 abstain=nodes + 1 + 2 * nodes * M + P * nodes)
    return first["abstain"] + M, first


def check_consensus(tables, out_val, none_val, quorum, M):
    """the rules of hrseg_consensus_labels on its host tables: a Data.score.ScoreTables (check_score_tables), out_val per
    level and channel and none_val in uint8 and all different, 1 <= M <= 8, 2 * quorum > M and quorum <= M (ValueError
    otherwise; needs no GPU)"""
    check_score_tables(tables)
    if not 1 <= M <= CONSENSUS_MAX_MEMBERS:
        raise ValueError(f"consensus_labels: {M} members, supported 1..{CONSENSUS_MAX_MEMBERS}")
    if not (2 * quorum > M and quorum <= M):
        raise ValueError(f"consensus_labels: quorum {quorum} of {M} members: need 2 * quorum > M and quorum <= M")
    name = lambda L, c: f"'{tables.names[L][c]}'" if tables.names else f"(level {L}, channel {c})"      # noqa: E731
    if not 0 <= int(none_val) <= 255:
        raise ValueError(f"consensus_labels: none value {none_val} not in 0..255")
    owner = {int(none_val): "the none value"}
    if len(out_val) != len(tables.C):
        raise ValueError(f"consensus_labels: out_val has {len(out_val)} levels, the tree {len(tables.C)}")
    for L, n in enumerate(tables.C):
        if len(out_val[L]) != n:
            raise ValueError(f"consensus_labels: out_val of level {L} does not have {n} entries")
        for c in range(n):
            v = int(out_val[L][c])
            if not 0 <= v <= 255:
                raise ValueError(f"consensus_labels: {name(L, c)} has the output value {v}, not in 0..255")
            if v in owner:
                raise ValueError(f"consensus_labels: {owner[v]} and {name(L, c)} share the byte {v}")
            owner[v] = name(L, c)


def _consensus_struct(tables, out_val, none_val, quorum):
    s = _lib.Consensus()
    s.nlevels = len(tables.C)
    for L, n in enumerate(tables.C):
        s.C[L] = int(n)
        for c in range(n):
            s.out_val[L][c] = int(out_val[L][c])
    s.none_val, s.quorum = int(none_val), int(quorum)
    return s


def consensus_labels(members, tables, out_val, none_val, quorum, per_image=False, counts=None, want_support=False, labels=None,
                     support=None):
    """vote M label maps of the same images down the class tree (hrseg_consensus_labels; the semantics are stated in
    include/hrseg.h under "consensus").  members: list of (buffer, desc, desc_host) triples, packed uint8 device buffers with
    [B,4] int64 descriptors (device, and their host copies for the checks) of equal (H, W) per sample; tables: a
    Data.score.ScoreTables whose path table knows the internal nodes' bytes; out_val per level and channel, none_val, quorum
    -> (labels, support or None, counts [R, cells] int64), R = B (per_image) or 1, the outputs packed as member 0 is (a
    buffer of member 0's size; bytes outside the spans are not written).  counts = the counters of an earlier call with the
    same M, batch size and per_image: they are added to.  labels / support: buffers to write into (else allocated).
    One launch, no synchronisation."""
    members = list(members)
    M = len(members)
    check_consensus(tables, out_val, none_val, quorum, M)
    rows0 = None
    for m, (buf, desc, host) in enumerate(members):
        _check_ragged(buf, desc, host, (1,))
        if buf.device != members[0][0].device:
            raise ValueError(f"consensus_labels: member {m} lives on another device than member 0")
        rows = host.tolist()
        if m == 0:
            rows0 = rows
            if not rows:
                raise ValueError("consensus_labels: an empty batch")
        if len(rows) != len(rows0):
            raise ValueError(f"consensus_labels: member {m} has {len(rows)} maps, member 0 has {len(rows0)}")
        for b, ((_, H, W, _), (_, H0, W0, _)) in enumerate(zip(rows, rows0)):
            if (H, W) != (H0, W0):
                raise ValueError(f"consensus_labels: member {m}, sample {b}: {H}x{W}, member 0 has {H0}x{W0}")
            if H * W >= CONSENSUS_MAX_PIXELS:
                raise ValueError(f"consensus_labels: member {m}, sample {b}: {H}x{W} has 2^31 pixels or more")
    device, n = members[0][0].device, members[0][0].numel()
    B, R = len(rows0), len(rows0) if per_image else 1
    total, _ = consensus_cells(sum(tables.C), M)
    if counts is None:
        counts = zeros((R, total), torch.int64, device)
    elif counts.dtype != torch.int64 or not counts.is_cuda or tuple(counts.shape) != (R, total) or not counts.is_contiguous():
        raise ValueError(f"consensus_labels: counts must be a contiguous int64 device tensor of shape {(R, total)}")
    outs = []
    for what, t, wanted in (("labels", labels, True), ("support", support, want_support or support is not None)):
        if t is None:
            t = torch.empty(n, dtype=torch.uint8, device=device) if wanted else None
        elif t.dtype != torch.uint8 or not t.is_cuda or t.dim() != 1 or t.numel() < n or not t.is_contiguous():
            raise ValueError(f"consensus_labels: {what} must be a contiguous uint8 device buffer of at least {n} bytes")
        outs.append(t)
    labels, support = outs
    host = torch.stack([h.to(torch.int64) for _, _, h in members]).contiguous()          # [M,B,4]
    desc = host.to(device, non_blocking=True)
    call("hrseg_consensus_labels", M, _lib.ptr_array([buf for buf, _, _ in members]), ptr(desc), host.data_ptr(),
         ptr(tables.device_lut(device)), C.byref(_consensus_struct(tables, out_val, none_val, quorum)), ptr(labels), ptr(support),
         ptr(counts), B, int(bool(per_image)))
    return labels, support, counts


CALIBRATION_MAX_BINS = 32


def check_calibration_tables(tables, score_tables):
    """the limits of hrseg_score_calibration on a Data.decode.DecodeTables and the Data.score.ScoreTables of the same levels:
    those of decode_labels and score_labels, the same channel counts in both, and every channel of a child level in exactly
    one child group (ValueError otherwise; needs no GPU)"""
    check_decode_tables(tables)
    check_score_tables(score_tables)
    if list(tables.C) != list(score_tables.C):
        raise ValueError(f"score_calibration: the decode tables have {list(tables.C)} channels per level, the path table "
                         f"{list(score_tables.C)}")
    for L in range(len(tables.C) - 1):
        owner = [None] * tables.C[L + 1]
        for p, (first, kids) in enumerate(zip(tables.first_child[L], tables.n_children[L])):
            for c in range(first, first + kids):
                if owner[c] is not None:
                    raise ValueError(f"score_calibration: channel {c} of level {L + 1} is in the child groups of channels "
                                     f"{owner[c]} and {p}")
                owner[c] = p
        for c, p in enumerate(owner):
            if p is None:
                raise ValueError(f"score_calibration: channel {c} of level {L + 1} is in no child group")


def score_calibration(logits, tables, gt, score_tables, inv_temp=None, n_bins=15, out=None, per_image=False):
    """per-level logits (list of [B,C_L,S,S] fp32 device tensors, or one tensor) + a Data.decode.DecodeTables against the
    ground-truth maps gt = (packed uint8 device buffer, [B,4] int64 descriptors on the device, their host copy) + the
    Data.score.ScoreTables of the same levels -> (hist [R, rows, n_bins + 1, 4] int64, ignored [R] int64), R = B (per_image)
    or 1, rows = sum C_L + levels: the reliability records (n, pos, sum_q, sum_e2) as hrseg_score_calibration states them.
    inv_temp: one fp32 value per level (None: all 1).  out = (hist, ignored) of an earlier call: both are added to.  One
    launch, no synchronisation."""
    check_calibration_tables(tables, score_tables)
    logits, B, S = _decode_logits("score_calibration", logits, tables)
    if S > DECODE_MAX_SIZE:
        raise ValueError(f"score_calibration: logits of side {S}, at most {DECODE_MAX_SIZE}")
    n_bins = int(n_bins)
    if not 1 <= n_bins <= CALIBRATION_MAX_BINS:
        raise ValueError(f"score_calibration: n_bins={n_bins}, supported 1..{CALIBRATION_MAX_BINS}")
    inv = [1.0] * len(logits) if inv_temp is None else [float(v) for v in inv_temp]
    if len(inv) != len(logits) or not all(0.0 < v < float("inf") for v in inv):
        raise ValueError(f"score_calibration: inv_temp {inv} must hold one finite positive value per level ({len(logits)})")
    gbuf, gdesc, ghost = gt
    _check_ragged(gbuf, gdesc, ghost, (1,))
    rows = ghost.tolist()
    if len(rows) != B:
        raise ValueError(f"score_calibration: logits of {B} samples against {len(rows)} ground-truth maps")
    for b, (_, H, W, _) in enumerate(rows):
        if H * W > SCORE_MAX_PIXELS:
            raise ValueError(f"score_calibration: sample {b}: {H}x{W} has more than 2^31 pixels")
    device = logits[0].device
    if gbuf.device != device or gdesc.device != device:
        raise ValueError("score_calibration: the logits and the ground truth live on different devices")
    R, nrows = (B if per_image else 1), sum(tables.C) + len(tables.C)
    shape = (R, nrows, n_bins + 1, 4)
    if out is None:
        hist, ignored = zeros(shape, torch.int64, device), zeros((R,), torch.int64, device)
    else:
        hist, ignored = out
        for t, want in ((hist, shape), (ignored, (R,))):
            if t.dtype != torch.int64 or not t.is_cuda or tuple(t.shape) != want or not t.is_contiguous():
                raise ValueError(f"score_calibration: out must hold contiguous int64 device tensors of shapes {shape} and {(R,)}")
    call("hrseg_score_calibration", len(logits), _lib.ptr_array(logits), _lib.int_array(list(tables.C)),
         C.byref(_decode_tree_struct(tables)), (C.c_float * len(inv))(*inv), ptr(gbuf), ptr(gdesc),
         ptr(score_tables.device_lut(device)), n_bins, ptr(hist), ptr(ignored), B, S, int(bool(per_image)))
    return hist, ignored


COMPONENTS_MAX_PIXELS = (1 << 31) - 1
LABEL_COMPONENTS_LAUNCHES, FILTER_COMPONENTS_LAUNCHES = 3, 3


def components_tile():
    """(width, height) of the tile one block of label_components labels in LDS"""
    return _lib.components_tile()


def _check_components(who, labels, desc, desc_host, group, connectivity=8):
    _check_ragged(labels, desc, desc_host, (1,))
    if desc_host.is_cuda or desc_host.dtype != torch.int64 or not desc_host.is_contiguous() or desc_host.shape[0] < 1:
        raise ValueError(f"{who}: desc_host must be a contiguous int64 host table with at least one row")
    for b, (_, H, W, _) in enumerate(desc_host.tolist()):
        if H * W > COMPONENTS_MAX_PIXELS:
            raise ValueError(f"{who}: image {b}: {H}x{W} has 2^31 pixels or more")
    if connectivity not in (4, 8):
        raise ValueError(f"{who}: connectivity {connectivity}, supported 4 and 8")
    if group.dtype != torch.uint8 or group.numel() != 256 or group.device != labels.device or not group.is_contiguous():
        raise ValueError(f"{who}: group must be a contiguous uint8 table of 256 entries on the labels' device")


def label_components(labels, desc, desc_host, group, connectivity=8, out=None):
    """packed uint8 label maps + [B,4] int64 descriptors (device, and the host copy) + group [256] uint8 (device) ->
    (roots, area), int32 tensors with the labels buffer's own indexing, as hrseg_label_components states them; elements
    outside the image spans are left as they are (out = (roots, area)) or uninitialised.  3 launches, no synchronisation."""
    _check_components("label_components", labels, desc, desc_host, group, connectivity)
    if out is None:
        roots = torch.empty(labels.numel(), dtype=torch.int32, device=labels.device)
        area = torch.empty(labels.numel(), dtype=torch.int32, device=labels.device)
    else:
        roots, area = out
        for t in (roots, area):
            if t.dtype != torch.int32 or t.device != labels.device or t.numel() != labels.numel() or not t.is_contiguous():
                raise ValueError("label_components: out must hold contiguous int32 device tensors of the labels' length")
    call("hrseg_label_components", ptr(labels), ptr(desc), desc_host.data_ptr(), desc_host.shape[0], ptr(group), int(connectivity),
         ptr(roots), ptr(area))
    return roots, area


def filter_components(labels, desc, desc_host, group, rules, roots, area, out=None, stats=None):
    """the filter of hrseg_filter_components on what label_components returned for the same maps: rules [256,3] int32
    (device; min_area, keep_largest, fill or -1) -> (out, stats): the cleaned maps in the layout of labels (bytes outside
    the spans: as they were in `out`, else uninitialised) and int64 [B,256,3] (found, removed, pixels), added to when given.
    3 launches (+ one fill launch when stats is allocated here), no synchronisation."""
    _check_components("filter_components", labels, desc, desc_host, group)
    B, dev = desc_host.shape[0], labels.device
    if rules.dtype != torch.int32 or tuple(rules.shape) != (256, 3) or rules.device != dev or not rules.is_contiguous():
        raise ValueError("filter_components: rules must be a contiguous int32 [256,3] table on the labels' device")
    for t in (roots, area):
        if t.dtype != torch.int32 or t.device != dev or t.numel() != labels.numel() or not t.is_contiguous():
            raise ValueError("filter_components: roots and area must be contiguous int32 device tensors of the labels' length")
    if out is None:
        out = torch.empty(labels.numel(), dtype=torch.uint8, device=dev)
    elif out.dtype != torch.uint8 or out.device != dev or out.numel() != labels.numel() or not out.is_contiguous():
        raise ValueError("filter_components: out must be a contiguous uint8 device tensor of the labels' length")
    if stats is None:
        stats = zeros((B, 256, 3), torch.int64, dev)
    elif stats.dtype != torch.int64 or stats.device != dev or tuple(stats.shape) != (B, 256, 3) or not stats.is_contiguous():
        raise ValueError(f"filter_components: stats must be a contiguous int64 device tensor of shape {(B, 256, 3)}")
    work = torch.empty(_lib.filter_components_workspace_bytes(B) // 8, dtype=torch.int64, device=dev)
    call("hrseg_filter_components", ptr(labels), ptr(desc), desc_host.data_ptr(), B, ptr(group), ptr(rules), ptr(roots), ptr(area),
         ptr(out), ptr(stats), ptr(work))
    return out, stats


SCORE_BOUNDARIES_LAUNCHES = 11
BOUNDARY_MAX_SIDE = 32768
BOUNDARY_FIELDS = ("n", "sum_q16", "max_d2", "within", "pk_d2")


def _pair_host_table(who, pred, pdesc, pdesc_host, gt, gdesc, gdesc_host, max_side=BOUNDARY_MAX_SIDE):
    """the checks of score_labels on the two descriptor tables + the limit of hrseg_score_boundaries on a side (max_side=None:
    that of hrseg_label_components on the pixels) -> the [2B,4] host table"""
    _check_ragged(pred, pdesc, pdesc_host, (1,))
    _check_ragged(gt, gdesc, gdesc_host, (1,))
    prow, grow = pdesc_host.tolist(), gdesc_host.tolist()
    if len(prow) != len(grow) or not prow:
        raise ValueError(f"{who}: {len(prow)} predicted maps against {len(grow)} ground-truth maps")
    for b, ((_, H, W, _), (_, gH, gW, _)) in enumerate(zip(prow, grow)):
        if (H, W) != (gH, gW):
            raise ValueError(f"{who}: sample {b}: predicted map {H}x{W}, ground truth {gH}x{gW}")
        if max_side is not None and (H > max_side or W > max_side):
            raise ValueError(f"{who}: sample {b}: {H}x{W}, a side above {max_side}")
        if max_side is None and H * W > COMPONENTS_MAX_PIXELS:
            raise ValueError(f"{who}: sample {b}: {H}x{W} has 2^31 pixels or more")
    if gt.device != pred.device:
        raise ValueError(f"{who}: the two buffers live on different devices")
    return torch.cat([pdesc_host.to(torch.int64), gdesc_host.to(torch.int64)]).contiguous()


def boundary_workspace_bytes(desc_host, tables):
    """bytes of the workspace score_boundaries needs for the images of a [B,4] int64 host descriptor table (needs no GPU)"""
    check_score_tables(tables)
    if desc_host.is_cuda or desc_host.dtype != torch.int64 or desc_host.dim() != 2 or desc_host.shape[1] != 4 or desc_host.shape[0] < 1:
        raise ValueError("boundary_workspace_bytes: desc_host must be an int64 host table [B,4] with at least one row")
    desc_host = desc_host.contiguous()
    return _lib.boundary_workspace_bytes(desc_host.data_ptr(), desc_host.shape[0], list(tables.C))


def score_boundaries(pred, pdesc, pdesc_host, gt, gdesc, gdesc_host, tables, tau2, percentile=95, out=None, workspace=None):
    """boundary records of predicted against ground-truth label maps (arguments as score_labels) -> int64 [B, N, 2, 5]
    device tensor as hrseg_score_boundaries states it: per image, tree node (breadth first) and direction (0: prediction ->
    truth) the fields BOUNDARY_FIELDS.  tau2 = floor(tolerance^2), percentile in 1..100.  The records are written, not
    added to (out: a tensor to write into); workspace: an int64 device tensor of at least boundary_workspace_bytes bytes
    (dirty is fine), else allocated here.  SCORE_BOUNDARIES_LAUNCHES launches, no synchronisation."""
    check_score_tables(tables)
    host = _pair_host_table("score_boundaries", pred, pdesc, pdesc_host, gt, gdesc, gdesc_host)
    tau2, percentile = int(tau2), int(percentile)
    if not 1 <= percentile <= 100:
        raise ValueError(f"score_boundaries: percentile {percentile} not in 1..100")
    if tau2 < 0:
        raise ValueError(f"score_boundaries: tau2 {tau2} is negative")
    B, N, dev = host.shape[0] // 2, sum(tables.C), pred.device
    shape = (B, N, 2, len(BOUNDARY_FIELDS))
    if out is None:
        out = torch.empty(shape, dtype=torch.int64, device=dev)
    elif out.dtype != torch.int64 or out.device != dev or tuple(out.shape) != shape or not out.is_contiguous():
        raise ValueError(f"score_boundaries: out must be a contiguous int64 device tensor of shape {shape}")
    need = _lib.boundary_workspace_bytes(host.data_ptr(), B, list(tables.C))
    if workspace is None:
        workspace = torch.empty((need + 7) // 8, dtype=torch.int64, device=dev)
    elif workspace.dtype != torch.int64 or workspace.device != dev or not workspace.is_contiguous() or workspace.numel() * 8 < need:
        raise ValueError(f"score_boundaries: workspace must be a contiguous int64 device tensor of at least {need} bytes")
    call("hrseg_score_boundaries", ptr(pred), ptr(pdesc), ptr(gt), ptr(gdesc), host.data_ptr(), ptr(tables.device_lut(dev)),
         len(tables.C), _lib.int_array(list(tables.C)), tau2, percentile, ptr(out), ptr(workspace), B)
    return out


# launches counted under the family "score_instances": the masked copy's one and hrseg_score_instances' four.
# SCORE_INSTANCES_LAUNCHES is what one DeviceInstanceScore.score adds to the family (the labellings count under their own)
MASK_VOID_LABELS_LAUNCHES, SCORE_INSTANCES_CALL_LAUNCHES = 1, 4
SCORE_INSTANCES_LAUNCHES = MASK_VOID_LABELS_LAUNCHES + SCORE_INSTANCES_CALL_LAUNCHES
INSTANCE_FIELDS = ("n_gt", "n_pred", "tp", "sum_iou_q30", "sum_inter", "sum_union", "tp_at0", "tp_at1", "tp_at2", "tp_at3")
INSTANCE_MAX_THRESHOLDS = 4


def _check_byte_table(who, what, t, device):
    if t.dtype != torch.uint8 or t.numel() != 256 or t.device != device or not t.is_contiguous():
        raise ValueError(f"{who}: {what} must be a contiguous uint8 table of 256 entries on the maps' device")


def void_value(group):
    """the byte the masked copy writes at void pixels: the largest pixel value of group 255 in a host group table (256
    ints), or -1 when every value has a group (then nothing can be void)"""
    free = [v for v, g in enumerate(group) if int(g) == 255]
    return free[-1] if free else -1


def instances_workspace_bytes(pdesc_host, gdesc_host):
    """bytes of the workspace score_instances needs for the images of two [B,4] int64 host descriptor tables: 12 bytes per
    byte of the ground-truth buffer's extent, rounded up to 8 (needs no GPU)"""
    for t in (pdesc_host, gdesc_host):
        if t.is_cuda or t.dtype != torch.int64 or t.dim() != 2 or t.shape[1] != 4 or t.shape[0] < 1:
            raise ValueError("instances_workspace_bytes: the descriptor tables must be int64 host tables [B,4] with at least one row")
    if pdesc_host.shape != gdesc_host.shape:
        raise ValueError(f"instances_workspace_bytes: {pdesc_host.shape[0]} predicted maps against {gdesc_host.shape[0]} ground-truth maps")
    host = torch.cat([pdesc_host, gdesc_host]).contiguous()
    return _lib.instances_workspace_bytes(host.data_ptr(), pdesc_host.shape[0])


def mask_void_labels(pred, pdesc, pdesc_host, gt, gdesc, gdesc_host, group, group_host, void=None, out=None):
    """the masked copy of hrseg_mask_void_labels: the predicted maps with the byte `void` wherever the ground truth's value
    has group 255 (void=None: void_value(group_host); -1: a plain copy).  group: the [256] uint8 device table, group_host:
    the 256 ints it was built from -- group[void] == 255 is checked HERE, on the host table, the library checks the range.
    out: a uint8 device tensor of pred's length to write into (bytes outside the spans stay), else allocated here.
    One launch, no synchronisation."""
    who = "mask_void_labels"
    if len(group_host) != 256:
        raise ValueError(f"{who}: the host group table has {len(group_host)} entries, not 256")
    v = void_value(group_host) if void is None else int(void)
    if not -1 <= v <= 255 or (v >= 0 and int(group_host[v]) != 255):
        raise ValueError(f"{who}: void value {v}: a byte whose group is 255, or -1 for none")
    if v < 0 and any(int(g) == 255 for g in group_host):
        raise ValueError(f"{who}: void value -1, but the group table has bytes of group 255")
    host = _pair_host_table(who, pred, pdesc, pdesc_host, gt, gdesc, gdesc_host, None)
    _check_byte_table(who, "group", group, pred.device)
    if out is None:
        out = torch.empty(pred.numel(), dtype=torch.uint8, device=pred.device)
    elif out.dtype != torch.uint8 or out.device != pred.device or out.numel() != pred.numel() or not out.is_contiguous():
        raise ValueError(f"{who}: out must be a contiguous uint8 device tensor of pred's length")
    call("hrseg_mask_void_labels", ptr(pred), ptr(pdesc), ptr(gt), ptr(gdesc), host.data_ptr(), ptr(group), v, ptr(out),
         host.shape[0] // 2)
    return out


def score_instances(pm, pdesc, pdesc_host, proots, parea, gt, gdesc, gdesc_host, groots, garea, group, things, thresholds=(),
                    per_image=True, out=None, workspace=None):
    """hrseg_score_instances on the masked prediction `pm` and the ground truth with what label_components returned for
    each; group / things: [256] uint8 device tables; thresholds: up to 4 per-mille values, 0 or 501..1000.
    -> (records, pmatch, gmatch, ginter): int64 [R, 256, 10] (R = B or 1; fields INSTANCE_FIELDS) and the int32 match maps
    indexed like the prediction (pmatch) and the ground-truth buffer (gmatch, ginter).  out = that tuple of an earlier
    call: records are added to, the maps written inside the spans and returned as given; else records are zeroed and the
    maps uninitialised outside the spans.  workspace: an int64 device tensor of at least instances_workspace_bytes bytes
    (dirty is fine), else allocated here.  SCORE_INSTANCES_CALL_LAUNCHES launches, no synchronisation."""
    who = "score_instances"
    host = _pair_host_table(who, pm, pdesc, pdesc_host, gt, gdesc, gdesc_host, None)
    dev, B = pm.device, host.shape[0] // 2
    _check_byte_table(who, "group", group, dev)
    _check_byte_table(who, "things", things, dev)
    thr = [int(t) for t in thresholds]
    if len(thr) > INSTANCE_MAX_THRESHOLDS or any(t != 0 and not 501 <= t <= 1000 for t in thr):
        raise ValueError(f"{who}: thresholds {thr}: at most {INSTANCE_MAX_THRESHOLDS} per-mille values, each 0 or in 501..1000")
    thr += [0] * (INSTANCE_MAX_THRESHOLDS - len(thr))
    for t, like in ((proots, pm), (parea, pm), (groots, gt), (garea, gt)):
        if t.dtype != torch.int32 or t.device != dev or t.numel() != like.numel() or not t.is_contiguous():
            raise ValueError(f"{who}: roots and areas must be contiguous int32 device tensors of their label buffer's length")
    R = B if per_image else 1
    shape = (R, 256, len(INSTANCE_FIELDS))
    if out is None:
        records = zeros(shape, torch.int64, dev)
        pmatch = torch.empty(pm.numel(), dtype=torch.int32, device=dev)
        gmatch = torch.empty(gt.numel(), dtype=torch.int32, device=dev)
        ginter = torch.empty(gt.numel(), dtype=torch.int32, device=dev)
    else:
        records, pmatch, gmatch, ginter = out
        if records.dtype != torch.int64 or records.device != dev or tuple(records.shape) != shape or not records.is_contiguous():
            raise ValueError(f"{who}: out's records must be a contiguous int64 device tensor of shape {shape}")
        for t, like in ((pmatch, pm), (gmatch, gt), (ginter, gt)):
            if t.dtype != torch.int32 or t.device != dev or t.numel() != like.numel() or not t.is_contiguous():
                raise ValueError(f"{who}: out's match maps must be contiguous int32 device tensors of their label buffer's length")
    need = _lib.instances_workspace_bytes(host.data_ptr(), B)
    if workspace is None:
        workspace = torch.empty((need + 7) // 8, dtype=torch.int64, device=dev)
    elif workspace.dtype != torch.int64 or workspace.device != dev or not workspace.is_contiguous() or workspace.numel() * 8 < need:
        raise ValueError(f"{who}: workspace must be a contiguous int64 device tensor of at least {need} bytes")
    call("hrseg_score_instances", ptr(pm), ptr(pdesc), ptr(proots), ptr(parea), ptr(gt), ptr(gdesc), ptr(groots), ptr(garea),
         host.data_ptr(), ptr(group), ptr(things), _lib.int_array(thr), ptr(records), ptr(pmatch), ptr(gmatch), ptr(ginter),
         ptr(workspace), B, int(bool(per_image)))
    return records, pmatch, gmatch, ginter


def combine_levels(x0, x1, masks, is_union):
    """x0 [B,C0,H,W] (+ x1 [B,C1,H,W] or None), per output channel a bit mask over the C0+C1 input channels and a
    union flag -> [B,len(masks),H,W]: copy of the selected channel, or 1.0 where any selected channel is > 0"""
    x0 = _c(x0.float())
    B, C0, H, W = x0.shape
    C1 = 0
    if x1 is not None:
        x1 = _c(x1.float())
        C1 = x1.shape[1]
    out = torch.empty((B, len(masks), H, W), dtype=torch.float32, device=x0.device)
    call("hrseg_combine_levels", ptr(x0), C0, ptr(x1), C1, (C.c_ulonglong * len(masks))(*[int(m) for m in masks]),
         _lib.int_array([int(u) for u in is_union]), ptr(out), B, len(masks), H * W)
    return out


def fill(t, v):
    call("hrseg_fill", ptr(t), float(v), t.numel())
    return t


# ------------------------------------------------------------------ FiLM / head / composition
def gap_nchw(p):
    B, Cn, H, W = p.shape
    cond = torch.empty((B, Cn), dtype=torch.float32, device=p.device)
    scratch = torch.empty(B * Cn * 64, dtype=torch.float64, device=p.device)
    call("hrseg_gap_nchw", ptr(p), ptr(cond), ptr(scratch), B * Cn, H * W)
    return cond


def film_linear_fwd(cond, wl, bl):
    B, Cc = cond.shape
    F2 = bl.numel()
    gb = torch.empty((B, F2), dtype=torch.float32, device=cond.device)
    call("hrseg_film_linear_fwd", ptr(cond), ptr(wl), ptr(bl), ptr(gb), B, Cc, F2)
    return gb


def film_linear_bwd(cond, wl, dgb, dwl, dbl, dcond_scale, want_dcond=True):
    B, Cc = cond.shape
    dcond = torch.empty((B, Cc), dtype=torch.float32, device=cond.device) if want_dcond else None
    call("hrseg_film_linear_bwd", ptr(cond), ptr(wl), ptr(dgb), ptr(dcond), ptr(dwl), ptr(dbl), B, Cc, dgb.shape[1],
         float(dcond_scale))
    return dcond


def head_fwd(f, gb, w, bias, cout=None):
    """f NHWC [B,H,W,F]; w [Cout,F] storage; -> z NHWC [B,H,W,Cout]"""
    B, H, W, F = f.shape
    Cout = cout if cout is not None else w.shape[0]
    z = empty_nhwc(B, H, W, Cout, f)
    call("hrseg_head_fwd", ptr(f), _ld(f), ptr(gb), ptr(w), ptr(bias), ptr(z), Cout, B, H * W, F, Cout)
    return z


def head_bwd(f, gb, w, dz, dw, dbias, dgb, want_df=True, df=None, df_accumulate=False, cout=None):
    B, H, W, F = f.shape
    Cout = cout if cout is not None else w.shape[0]
    if want_df and df is None:
        df = torch.empty(f.shape, dtype=torch.float32, device=f.device)
        df_accumulate = False
    call("hrseg_head_bwd", ptr(f), _ld(f), ptr(gb), ptr(w), ptr(dz), _ld(dz), ptr(df), _ld(df) if df is not None else 0,
         int(df_accumulate), ptr(dw), ptr(dbias), ptr(dgb), B, H * W, F, Cout)
    return df


def head_bn_fwd(y, coef, gb, w, bias, cout=None):
    """head_fwd on the un-normalised conv output y of the BatchNorm + ReLU layer in front of the heads (coef: that BatchNorm's
    [4][F]); the same logits as bn_fwd_group's apply phase + head_fwd, without the normalised tensor (hrseg_head_bn_fwd)"""
    B, H, W, F = y.shape
    Cout = cout if cout is not None else w.shape[0]
    z = empty_nhwc(B, H, W, Cout, y)
    call("hrseg_head_bn_fwd", ptr(y), _ld(y), ptr(coef), ptr(gb), ptr(w), ptr(bias), ptr(z), Cout, B, H * W, F, Cout)
    return z


def head_bn_chunks(npix, F, nseg):
    """pixel chunks of the fused head + BatchNorm backward: bn_bwd_group's, so that the partial sums are the same ones"""
    nch = _nchunks(npix, F)
    return max(nseg, nch // nseg * nseg) if nseg > 1 else nch


def _head_bn_struct(y, coef, nseg, partial, nchunks, heads, dy=None, dy_absmax=None):
    """heads: per segment dict(gb, w, dzl, cout, dw, dbias, dgb) or None (a segment this call does not touch)"""
    NB, H, W, F = y.shape
    assert NB % nseg == 0 and len(heads) == nseg and partial.numel() >= (nchunks + nseg) * 2 * F
    a = _lib.HeadBn()
    a.y, a.ldy, a.coef = ptr(y), _ld(y), ptr(coef)
    a.F, a.nseg, a.B, a.hw = F, nseg, NB // nseg, H * W
    a.partial, a.nchunks, a.dy_absmax = ptr(partial), int(nchunks), ptr(dy_absmax)
    a.dy, a.lddy = ptr(dy), (_ld(dy) if dy is not None else 0)
    for s, h in enumerate(heads):
        if h is None:
            continue
        dzl = h["dzl"]
        assert dzl.shape[0] * dzl.shape[1] * dzl.shape[2] == a.B * a.hw
        a.gb[s], a.w[s], a.dzl[s], a.lddzl[s], a.Cout[s] = ptr(h.get("gb")), ptr(h["w"]), ptr(dzl), _ld(dzl), int(h["cout"])
        a.dw[s], a.dbias[s], a.dgb[s] = ptr(h.get("dw")), ptr(h.get("dbias")), ptr(h.get("dgb"))
    return a


def head_bn_bwd_reduce(y, coef, nseg, partial, nchunks, heads, seg0=0, nsegs=None, dy_absmax=None):
    """first pass of the fused backward for segments [seg0, seg0 + nsegs) (hrseg_head_bn_bwd_reduce): dw / dbias / dgb of their
    heads accumulate, the BatchNorm partial sums of their chunks are written"""
    nsegs = nseg - seg0 if nsegs is None else nsegs
    hs = [h if seg0 <= s < seg0 + nsegs else None for s, h in enumerate(heads)]
    a = _head_bn_struct(y, coef, nseg, partial, nchunks, hs, dy_absmax=dy_absmax)
    call("hrseg_head_bn_bwd_reduce", C.byref(a), int(seg0), int(nsegs))


def bn_bwd_finalize(y, coef, nseg, partial, nchunks, dgamma, dbeta):
    """the unchanged finalize phase of bn_bwd_group alone (totals per segment behind the partials, dgamma / dbeta +=)"""
    arr = (_lib.BnBwd * 1)()
    a = arr[0]
    F = y.shape[3]
    # hrseg_bn_bwd_group_phases checks dz / y / dy of every problem whatever the phases; phase 2 (finalize) reads `partial` and
    # writes the totals, dgamma and dbeta only.  A finalize-only call relies on that: y stands in for dz and dy, untouched
    a.dz, a.lddz, a.y, a.ldy, a.coef = ptr(y), _ld(y), ptr(y), _ld(y), ptr(coef)     # (dz / dy: unused by this phase, non-NULL)
    a.dy, a.lddy = ptr(y), _ld(y)
    a.dgamma, a.dbeta = ptr(dgamma), ptr(dbeta)
    a.npix, a.C, a.partial, a.nchunks, a.nseg, a.sum_ranks = _npix(y), F, ptr(partial), int(nchunks), nseg, 1
    call("hrseg_bn_bwd_group_phases", 1, arr, 0, 2)


def head_bn_bwd_apply(y, coef, nseg, partial, nchunks, heads, dy=None, dy_absmax=None):
    """second pass (hrseg_head_bn_bwd_apply): -> dy of the layer's convolution output"""
    if dy is None:
        dy = torch.empty(y.shape, dtype=torch.float32, device=y.device)
    a = _head_bn_struct(y, coef, nseg, partial, nchunks, heads, dy=dy, dy_absmax=dy_absmax)
    call("hrseg_head_bn_bwd_apply", C.byref(a))
    return dy


def logits_up_fwd(z, Ho, Wo, align_corners=True):
    B, Hi, Wi, Cn = z.shape
    out = torch.empty((B, Cn, Ho, Wo), dtype=torch.float32, device=z.device)
    call("hrseg_logits_up_fwd", ptr(z), _ld(z), B, Hi, Wi, Cn, ptr(out), Ho, Wo, int(align_corners))
    return out


def logits_up_bwd(dout, Hi, Wi, align_corners=True):
    B, Cn, Ho, Wo = dout.shape
    din = empty_nhwc(B, Hi, Wi, Cn, dout)
    call("hrseg_logits_up_bwd", ptr(dout), B, Hi, Wi, Cn, ptr(din), Cn, Ho, Wo, int(align_corners))
    return din


def sigmoid_fwd(z):
    p = torch.empty_like(z)
    call("hrseg_sigmoid_fwd", ptr(z), ptr(p), z.numel())
    return p


def _strides3(dp, B, Cn, hw):
    """(sb, sc, si) element strides of a [B,C,H,W]-shaped (possibly expanded) gradient."""
    if dp.dim() == 4:
        assert dp.stride(3) in (0, 1) and (dp.stride(2) == dp.shape[3] * dp.stride(3) or dp.shape[2] == 1)
        return dp.stride(0), dp.stride(1), dp.stride(3)
    assert dp.dim() == 2
    return dp.stride(0), dp.stride(1), 0


def sigmoid_bwd(dp, z, dz=None, accumulate=False):
    B, Cn, H, W = z.shape
    if dz is None:
        dz = torch.empty_like(z)
        accumulate = False
    sb, sc, si = _strides3(dp, B, Cn, H * W)
    call("hrseg_sigmoid_bwd", ptr(dp), sb, sc, si, ptr(z), ptr(dz), int(accumulate), B, Cn, H * W)
    return dz


def _group_args(group_parent, group_size):
    """the (ngroups, group_parent, group_size) argument triple of the entry points that take a level's group table"""
    return len(group_parent), _lib.int_array(group_parent), _lib.int_array(group_size)


def compose_fwd(z, pprev, group_parent, group_size):
    B, Cn, H, W = z.shape
    p = torch.empty_like(z)
    call("hrseg_compose_fwd", ptr(z), ptr(pprev), ptr(p), B, Cn, pprev.shape[1], H * W, *_group_args(group_parent, group_size))
    return p


def compose_bwd(dp, z, pprev, group_parent, group_size, dz=None, dz_accumulate=False, dpprev=None,
                dpprev_accumulate=False, want_dz=True, want_dpprev=True):
    B, Cn, H, W = z.shape
    if want_dz and dz is None:
        dz, dz_accumulate = torch.empty_like(z), False
    if want_dpprev and dpprev is None:
        dpprev, dpprev_accumulate = torch.empty_like(pprev), False
    sb, sc, si = _strides3(dp, B, Cn, H * W)
    call("hrseg_compose_bwd", ptr(dp), sb, sc, si, ptr(z), ptr(pprev), ptr(dz), int(dz_accumulate), ptr(dpprev),
         int(dpprev_accumulate), B, Cn, pprev.shape[1], H * W, *_group_args(group_parent, group_size))
    return dz, dpprev


# ------------------------------------------------------------------ loss / metrics / optimizer
def _c(t):
    """NCHW planes are addressed as b*C*hw + c*hw + i: insist on contiguous storage"""
    return t if t.is_contiguous() else t.contiguous()


class OhemState(NamedTuple):
    """what loss_fwd leaves for loss_bwd when online hard example mining is on: the options it ran with, the stored scores
    q[B*hw] and the selection's record (int32[4] on the device: lam_k as fp32 bits, n_candidates, n_kept, reserved)"""
    thresh: float
    min_kept: int
    q: torch.Tensor
    record: torch.Tensor

    @property
    def lam_k(self):
        """0-dim device tensor (no sync)"""
        return self.record[:1].view(torch.float32)[0]


def ohem_scores(z, t, q=None):
    """-> q[B*hw] fp32: per pixel the softmax probability mass on the valid channels' targets, sum_{t_c != -1} t_c p_c; -1 where
    every channel is ignored (hrseg_ohem_scores)"""
    z, t = _c(z), _c(t)
    B, Cn, H, W = z.shape
    if q is None:
        q = torch.empty(B * H * W, dtype=torch.float32, device=z.device)
    call("hrseg_ohem_scores", ptr(z), ptr(t), ptr(q), B, Cn, H * W)
    return q


def ohem_select(q, thresh, min_kept, record=None, workspace=None):
    """-> record (int32[4], device): the exact min(min_kept, N)-th smallest candidate score of q and the counts that go with
    it (hrseg_ohem_select; no sync, no sort).  `workspace`: _lib.ohem_workspace_bytes() bytes the call zeroes itself."""
    if record is None:
        record = torch.empty(4, dtype=torch.int32, device=q.device)
    if workspace is None:
        workspace = torch.empty(_lib.ohem_workspace_bytes() // 4, dtype=torch.int32, device=q.device)
    call("hrseg_ohem_select", ptr(q), q.numel(), float(thresh), int(min_kept), ptr(workspace), ptr(record))
    return record


BORDER_MAX_RADIUS = 32              # HRSEG_BORDER_MAX_RADIUS
BORDER_MAX_PIXELS = 1 << 31


def border_weights(t, radius, lut, want_d2=False):
    """t [B,C,H,W] fp32 target planes (-1 / 0 / 1), lut [radius^2 + 1] fp32 on t's device -> (labels [B,H,W] uint8,
    v [B,H,W] fp32[, d2 [B,H,W] int32]): the label map, lut[d2] and the squared distance to the nearest other label within
    `radius` (include/hrseg.h, "border weights"; hrseg_border_weights)"""
    if t.dim() != 4 or min(t.shape) < 1:
        raise ValueError(f"border_weights: t must be [B,C,H,W], got {tuple(t.shape)}")
    B, Cn, H, W = t.shape
    if Cn > 16:
        raise ValueError(f"border_weights: {Cn} channels, at most 16")
    if H * W >= BORDER_MAX_PIXELS:
        raise ValueError(f"border_weights: {H} x {W} has 2^31 pixels or more")
    radius = int(radius)
    if not 1 <= radius <= BORDER_MAX_RADIUS:
        raise ValueError(f"border_weights: radius {radius} outside 1..{BORDER_MAX_RADIUS}")
    assert t.dtype == torch.float32 and t.is_cuda and t.is_contiguous(), "border_weights: t must be contiguous fp32 on the device"
    assert lut.dtype == torch.float32 and lut.device == t.device and lut.is_contiguous(), \
        "border_weights: lut must be contiguous fp32 on t's device"
    if lut.numel() != radius * radius + 1:
        raise ValueError(f"border_weights: lut has {lut.numel()} entries, radius {radius} needs {radius * radius + 1}")
    labels = torch.empty((B, H, W), dtype=torch.uint8, device=t.device)
    v = torch.empty((B, H, W), dtype=torch.float32, device=t.device)
    d2 = torch.empty((B, H, W), dtype=torch.int32, device=t.device) if want_d2 else None
    call("hrseg_border_weights", ptr(t), B, Cn, H, W, radius, ptr(lut), ptr(labels), ptr(v), ptr(d2))
    return (labels, v, d2) if want_d2 else (labels, v)


def _pixel_weight(who, pw, z):
    """a [B,H,W] / [B,1,H,W] / [B*H*W] fp32 tensor on z's device, contiguous -> itself"""
    B, _, H, W = z.shape
    assert pw.dtype == torch.float32 and pw.device == z.device and pw.is_contiguous() and pw.numel() == B * H * W, \
        f"{who}: pixel_weight must be contiguous fp32 [B,H,W] on the logits' device"
    return pw


def loss_fwd(z, t, w, options=None, ohem=None, pixel_weight=None):
    """-> (out[3] = ce, dice, n_valid_dice ; coef for the backward).  options = (focal gamma, Dice smooth, Tversky alpha,
    beta) selects the hrseg_loss_*_opt entry points; None = the calls without options (gamma 0, smooth 0, alpha = beta = 0.5).
    ohem = (thresh, min_kept): online hard example mining on the CE term -- scores, selection, then the masked partials; the
    return value gains a third entry, the OhemState loss_bwd needs.  None = exactly the calls above.
    pixel_weight [B,H,W] fp32: one weight per pixel on the CE term (hrseg_loss_partials_pw; include/hrseg.h, "border
    weights"); not together with ohem.  None = exactly the calls above."""
    z, t = _c(z), _c(t)
    B, Cn, H, W = z.shape
    if pixel_weight is not None and ohem is not None:
        raise ValueError("loss_fwd: pixel_weight and ohem are not combined")
    part = torch.empty(B * Cn * 5, dtype=torch.float64, device=z.device)
    out = torch.empty(3, dtype=torch.float32, device=z.device)
    coef = torch.empty(B * Cn * 4, dtype=torch.float32, device=z.device)
    state = None
    own = ohem is not None or pixel_weight is not None          # the partials come from an entry point of the option's own
    if ohem is not None:
        thresh, min_kept = float(ohem[0]), int(ohem[1])
        q = ohem_scores(z, t)
        state = OhemState(thresh, min_kept, q, ohem_select(q, thresh, min_kept))
        gamma = 0.0 if options is None else float(options[0])
        call("hrseg_loss_partials_ohem", ptr(z), ptr(t), ptr(q), ptr(state.record), thresh, ptr(part), B, Cn, H * W, gamma)
    elif pixel_weight is not None:
        pw = _pixel_weight("loss_fwd", pixel_weight, z)
        call("hrseg_loss_partials_pw", ptr(z), ptr(t), ptr(pw), ptr(part), B, Cn, H * W, 0.0 if options is None else float(options[0]))
    if options is None:
        if not own:
            call("hrseg_loss_partials", ptr(z), ptr(t), ptr(part), B, Cn, H * W)
        call("hrseg_loss_finalize", ptr(part), ptr(w), B, Cn, ptr(out), ptr(coef))
    else:
        gamma, smooth, alpha, beta = (float(v) for v in options)
        if not own:
            call("hrseg_loss_partials_opt", ptr(z), ptr(t), ptr(part), B, Cn, H * W, gamma)
        call("hrseg_loss_finalize_opt", ptr(part), ptr(w), B, Cn, smooth, alpha, beta, ptr(out), ptr(coef))
    return (out, coef) if ohem is None else (out, coef, state)


def loss_bwd(z, t, coef, g, dz=None, accumulate=False, options=None, ohem=None, pixel_weight=None):
    """`options`: the ones loss_fwd produced `coef` with (the backward itself reads the focal gamma only); `ohem`: the
    OhemState that loss_fwd returned (the keep decision is read from its stored scores and record, never recomputed);
    `pixel_weight`: the map loss_fwd was given (hrseg_loss_bwd_pw)"""
    z, t = _c(z), _c(t)
    B, Cn, H, W = z.shape
    if dz is None:
        dz, accumulate = torch.empty_like(z), False
    if pixel_weight is not None:
        if ohem is not None:
            raise ValueError("loss_bwd: pixel_weight and ohem are not combined")
        pw = _pixel_weight("loss_bwd", pixel_weight, z)
        call("hrseg_loss_bwd_pw", ptr(z), ptr(t), ptr(pw), ptr(coef), ptr(g), ptr(dz), int(accumulate), B, Cn, H * W,
             0.0 if options is None else float(options[0]))
    elif ohem is not None:
        call("hrseg_loss_bwd_ohem", ptr(z), ptr(t), ptr(ohem.q), ptr(ohem.record), float(ohem.thresh), ptr(coef), ptr(g), ptr(dz),
             int(accumulate), B, Cn, H * W, 0.0 if options is None else float(options[0]))
    elif options is None:
        call("hrseg_loss_bwd", ptr(z), ptr(t), ptr(coef), ptr(g), ptr(dz), int(accumulate), B, Cn, H * W)
    else:
        call("hrseg_loss_bwd_opt", ptr(z), ptr(t), ptr(coef), ptr(g), ptr(dz), int(accumulate), B, Cn, H * W, float(options[0]))
    return dz


def consistency_sums(p, pprev, group_parent, group_size):
    """-> [ngroups] float64 sums of |sum_children P - P_parent| over batch and pixels"""
    p, pprev = _c(p), _c(pprev)
    B, Cn, H, W = p.shape
    out = zeros((len(group_parent),), torch.float64, p.device)
    call("hrseg_consistency", ptr(p), ptr(pprev), ptr(out), B, Cn, pprev.shape[1], H * W, *_group_args(group_parent, group_size))
    return out


def consistency_bwd(p, pprev, g, scale, group_parent, group_size):
    """-> (dp, dpprev) for  scale * g * sum |sum_children P - P_parent|"""
    p, pprev = _c(p), _c(pprev)
    B, Cn, H, W = p.shape
    dp, dpprev = torch.empty_like(p), torch.empty_like(pprev)
    call("hrseg_consistency_bwd", ptr(p), ptr(pprev), ptr(g), float(scale), ptr(dp), ptr(dpprev), B, Cn, pprev.shape[1],
         H * W, *_group_args(group_parent, group_size))
    return dp, dpprev


def group_kl_sums(z, pprev, group_parent, group_size):
    """-> [ngroups] float64: sum over b, pixels and the group's children of Q (log Q + log size) (hrseg_group_kl)"""
    z, pprev = _c(z), _c(pprev)
    B, Cn, H, W = z.shape
    out = zeros((len(group_parent),), torch.float64, z.device)
    call("hrseg_group_kl", ptr(z), ptr(pprev), ptr(out), B, Cn, pprev.shape[1], H * W, *_group_args(group_parent, group_size))
    return out


def group_kl_bwd(z, pprev, g, scale, group_parent, group_size):
    z, pprev = _c(z), _c(pprev)
    B, Cn, H, W = z.shape
    dz = torch.empty_like(z)
    call("hrseg_group_kl_bwd", ptr(z), ptr(pprev), ptr(g), float(scale), ptr(dz), B, Cn, pprev.shape[1], H * W,
         *_group_args(group_parent, group_size))
    return dz


def _tree_kl_args(who, z, u, wprev, pw, inv_temp, thresh, group_parent, group_size):
    """shape / dtype / device checks shared by tree_kl_fwd and tree_kl_bwd -> (B, C, Cprev, hw)"""
    if z.dim() != 4 or u.shape != z.shape:
        raise ValueError(f"{who}: student and teacher logits must both be [B,C,H,W], got {tuple(z.shape)} and {tuple(u.shape)}")
    B, Cn, H, W = z.shape
    for name, t in (("student logits", z), ("teacher logits", u), ("teacher parent probabilities", wprev), ("pixel_weight", pw)):
        if t is not None and (t.dtype != torch.float32 or t.device != z.device or not t.is_cuda or not t.is_contiguous()):
            raise ValueError(f"{who}: {name} must be contiguous float32 on the student logits' device (a GPU)")
    if wprev is not None and (wprev.dim() != 4 or wprev.shape[0] != B or tuple(wprev.shape[2:]) != (H, W)):
        raise ValueError(f"{who}: teacher parent probabilities must be [{B},Cprev,{H},{W}], got {tuple(wprev.shape)}")
    if pw is not None and pw.numel() != B * H * W:
        raise ValueError(f"{who}: pixel_weight must hold {B} x {H} x {W} values, got {tuple(pw.shape)}")
    if len(group_parent) != len(group_size) or sum(group_size) != Cn:
        raise ValueError(f"{who}: group sizes {list(group_size)} do not add up to the level's {Cn} channels")
    if not (math.isfinite(inv_temp) and inv_temp > 0.0):
        raise ValueError(f"{who}: inv_temp must be finite and > 0, got {inv_temp!r}")
    if not 0.0 <= thresh <= 1.0:
        raise ValueError(f"{who}: thresh must be in [0, 1], got {thresh!r}")
    return B, Cn, (1 if wprev is None else wprev.shape[1]), H * W


def tree_kl_fwd(z, u, wprev, pw, inv_temp, thresh, group_parent, group_size, out=None):
    """-> [ngroups,3] float64: per group the sums over the kept (pixel, group) pairs of m omega kl and of m omega, and their
    number (hrseg_tree_kl; include/hrseg.h, "tree distillation").  wprev / pw may be None; `out` is added to when given."""
    inv_temp, thresh = float(inv_temp), float(thresh)
    B, Cn, Cprev, hw = _tree_kl_args("tree_kl_fwd", z, u, wprev, pw, inv_temp, thresh, group_parent, group_size)
    if out is None:
        out = zeros((len(group_size), 3), torch.float64, z.device)
    call("hrseg_tree_kl", ptr(z), ptr(u), ptr(wprev), ptr(pw), inv_temp, thresh, ptr(out), B, Cn, Cprev, hw,
         *_group_args(group_parent, group_size))
    return out


def tree_kl_bwd(z, u, wprev, pw, inv_temp, thresh, g, scale, group_parent, group_size, dz=None, accumulate=False):
    """-> dz (=|+=) g[0] * scale * m omega beta (p - q) on the kept groups (hrseg_tree_kl_bwd); g: a 1-element fp32 device
    tensor; the same inv_temp and thresh as the forward call"""
    inv_temp, thresh = float(inv_temp), float(thresh)
    B, Cn, Cprev, hw = _tree_kl_args("tree_kl_bwd", z, u, wprev, pw, inv_temp, thresh, group_parent, group_size)
    if dz is None:
        dz, accumulate = torch.empty_like(z), False
    elif dz.shape != z.shape or dz.dtype != torch.float32 or dz.device != z.device or not dz.is_contiguous():
        raise ValueError("tree_kl_bwd: dz must be a contiguous float32 tensor of the logits' shape on their device")
    if g.dtype != torch.float32 or g.device != z.device or g.numel() < 1:
        raise ValueError("tree_kl_bwd: g must be a float32 tensor on the logits' device")
    call("hrseg_tree_kl_bwd", ptr(z), ptr(u), ptr(wprev), ptr(pw), inv_temp, thresh, ptr(g), float(scale), ptr(dz), int(accumulate),
         B, Cn, Cprev, hw, *_group_args(group_parent, group_size))
    return dz


def predict_metrics(z, t, child, mask_pred=True, want_onehot=True):
    """-> (onehot or None, confusion matrix [K,K] int64 with K = C + child)"""
    z, t = _c(z), _c(t)
    B, Cn, H, W = z.shape
    K = Cn + (1 if child else 0)
    onehot = torch.empty_like(z) if (want_onehot and mask_pred) else None
    cm = zeros((K, K), torch.int64, z.device)
    call("hrseg_predict_metrics", ptr(z), ptr(t), ptr(onehot), ptr(cm), B, Cn, H * W, int(child), int(mask_pred))
    return onehot, cm


def metric_vectors(cms, child):
    """per-level confusion matrices [K,K] int64 (predict_metrics) -> [5][sum C_L] fp32: accuracy, iou, dice, precision,
    recall of every class, the levels side by side; one launch (hrseg_metric_vectors)"""
    cms = [_c(cm) for cm in cms]
    K = [cm.shape[0] for cm in cms]
    total = sum(k - (1 if ch else 0) for k, ch in zip(K, child))
    out = torch.empty((5, total), dtype=torch.float32, device=cms[0].device)
    call("hrseg_metric_vectors", len(cms), _lib.ptr_array(cms), _lib.int_array(K), _lib.int_array([int(bool(c)) for c in child]),
         ptr(out))
    return out


def adamw(p, g, m, v, lr, beta1, beta2, eps, wd, step, gscale=1.0):
    bc1 = 1.0 - beta1 ** step
    bc2 = 1.0 - beta2 ** step
    call("hrseg_adamw", ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), float(lr), float(beta1), float(beta2), float(eps),
         float(wd), float(bc1), float(bc2), float(gscale))


def adamw_dev(p, g, m, v, hyper, state):
    """graph-replayable AdamW step: hyper/state are device tensors (see hrseg.h)"""
    call("hrseg_adamw_dev", ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), ptr(hyper), ptr(state))


def grad_sumsq(g, partial=None):
    """fp64 partial sums of squares of the flat fp32 buffer g, one per chunk of _lib.grad_sumsq_chunk_len() elements
    (hrseg_grad_sumsq: chunking a function of g.numel() alone, no atomics) -> partial [nchunks] float64"""
    n = g.numel()
    nchunks = _lib.grad_sumsq_chunks(n)
    if partial is None:
        partial = torch.empty(nchunks, dtype=torch.float64, device=g.device)
    call("hrseg_grad_sumsq", ptr(g), n, ptr(partial), partial.numel())
    return partial


def grad_clip_finalize(partial, hyper, clipcfg, state, clip):
    """partials -> clip = {norm, coef, finite, skipped_total}; advances AdamW's device `state` unless the step is void
    (clipcfg = {max_norm, skip_nonfinite}; see hrseg.h)"""
    call("hrseg_grad_clip_finalize", ptr(partial), partial.numel(), ptr(hyper), ptr(clipcfg), ptr(state), ptr(clip))


def adamw_dev_clip(p, g, m, v, hyper, state, clipcfg, clip):
    """adamw_dev with the gradient scaled by clip's coefficient, or nothing at all on a void step; `state` was advanced
    by grad_clip_finalize"""
    call("hrseg_adamw_dev_clip", ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), ptr(hyper), ptr(state), ptr(clipcfg), ptr(clip))


def adamw_dev_ema(p, g, m, v, e, hyper, state, emacfg):
    """adamw_dev that also advances the weight average e (emacfg = {decay, warmup, s0}; see hrseg.h): p, m, v bitwise as
    from adamw_dev, no extra launch"""
    call("hrseg_adamw_dev_ema", ptr(p), ptr(g), ptr(m), ptr(v), ptr(e), p.numel(), ptr(hyper), ptr(state), ptr(emacfg))


def adamw_dev_clip_ema(p, g, m, v, e, hyper, state, clipcfg, clip, emacfg):
    """adamw_dev_clip that also advances the weight average e; a void step leaves e alone too"""
    call("hrseg_adamw_dev_clip_ema", ptr(p), ptr(g), ptr(m), ptr(v), ptr(e), p.numel(), ptr(hyper), ptr(state), ptr(clipcfg),
         ptr(clip), ptr(emacfg))


def ema_update(e, p, state, emacfg):
    """the weight average's update alone, for parameters p whose step is done (`state` already advanced): bitwise the e
    of the fused kernels"""
    call("hrseg_ema_update", ptr(e), ptr(p), p.numel(), ptr(state), ptr(emacfg))


def swap(a, b):
    """exchange the contents of two flat fp32 buffers in place (hrseg_swap)"""
    if a.numel() != b.numel():
        raise ValueError(f"ops.swap: {a.numel()} vs {b.numel()} elements")
    call("hrseg_swap", ptr(a), ptr(b), a.numel())
