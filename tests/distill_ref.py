"""float64 reference, leaf enumeration, case list and error bounds of the tree distillation kernels (csrc/distill.hip;
include/hrseg.h, "tree distillation").  tests/test_distill_cpu.py pins this module, tests/test_distill_gpu.py holds the kernels
to it.

The reference follows the header's formulas literally, on torch CPU tensors [B,C,hw]; run in float64 it is the reference, run in
float32 it is "the same formulas in fp32" that the bound must admit, and `variant` switches in the three mistakes the bound must
catch.

ERROR MODEL.  u = 2^-24 is the unit roundoff of fp32; expf and logf are taken as 1 ulp = 2u, the division as correctly rounded.
Per pixel and group, with A = max_c |beta u_c|, Z = max_c |beta z_c|, La = |log sum_c exp(xa_c)|, Lz likewise, every absolute
error in units of u:
    a_c = beta*u_c                 A          (one rounding)
    ma                             A          (the same rounding at the arg-max)
    xa_c = a_c - ma                2A + |xa_c| <= 4A
    ea_c = exp(xa_c)               relative 4A + 2
    sa = sum ea_c                  relative 4A + 2 + 15          (at most 15 additions)
    la = log(sa)                   4A + 17 + 2 La
    lq_c = xa_c - la               4A + (4A + 17 + 2 La) + |lq_c| <= 10A + 3La + 17          (|lq_c| <= 2A + La)
    q_c = ea_c * (1 / sa)          relative (4A + 2) + (4A + 17 + 1) + 1 = 8A + 21
    d_c = lq_c - lp_c              10(A + Z) + 3(La + Lz) + 34 + |d_c|
    q_c * d_c                      q_c [10(A + Z) + 3(La + Lz) + 34] + q_c |d_c| (1 + 8A + 21 + 1)
    kl = sum_c                     + 15 q_c |d_c| per term
    (m * omega) * kl               + 2 |value|
so  |value - ref| <= SECOND u m omega [ K_LOG (A + Z) + K_LSE (La + Lz) + K_ONE + sum_c q_c |d_c| (K_Q A + K_QONE) ]      (sum_c q_c = 1)
with K_LOG = 10, K_LSE = 3, K_ONE = 34, K_Q = 8, K_QONE = 40, and SECOND = 1.25 for the second-order terms.  The sums over pixels
are fp64 on the device: nothing is added for them.  An exponential that lands below the normal range may be flushed: each q_c
then carries an absolute error of at most 2^-126, i.e. FLUSH |d_c| m omega per channel with FLUSH = 2^-125.
Slot 1 (sum of m * omega) is one rounding per term: 2 u sum |m omega| with room for the fp64 sum.  Slot 2 is an integer: exact,
provided no conf lies within GATE_MARGIN of the threshold (the case builder moves such pixels away; conf itself is good to
(4 max|u| + 20) u relative, far inside the margin).
Gradient element:  dz_j = w (p_j - q_j),  w = ((g scale) (m omega)) beta: four roundings, the difference one, the product one:
    |dz_j - ref| <= SECOND u |w| [ p_j (K_Q Z + K_P) + q_j (K_Q A + K_P) + K_W |p_j - q_j| ] + FLUSH |w|,   K_P = 21, K_W = 6
and one more rounding of the result when the call accumulates.

Imports numpy and torch (CPU)."""
import numpy as np
import torch

U = 2.0 ** -24
SECOND = 1.25
FLUSH = 2.0 ** -125
K_LOG, K_LSE, K_ONE, K_Q, K_QONE = 10, 3, 34, 8, 40
K_P, K_W = 21, 6
GATE_MARGIN = 2e-3


def group_slices(gs):
    out, s = [], 0
    for n in gs:
        out.append(slice(s, s + n))
        s += n
    return out


def _side(v, beta):
    """one side's group softmax in the log domain, in the header's operation order -> (log-softmax, softmax, |beta v| max, |log sum|)"""
    a = beta * v
    ma = a.max(dim=1, keepdim=True).values      # (torch's max hands a NaN on; the kernel's drops it and meets it again in a - ma)
    x = a - ma
    e = torch.exp(x)
    s = e.sum(dim=1, keepdim=True)
    ls = torch.log(s)
    return x - ls, e * (1.0 / s), a.abs().max(dim=1).values, ls.abs()[:, 0]


def gate_conf(u, omega):
    """conf_g = omega / sum_c exp(u_c - max_c u_c): temperature 1 whatever beta"""
    mu = u.max(dim=1, keepdim=True).values
    return omega / torch.exp(u - mu).sum(dim=1)


def tree_kl_ref(z, u, wprev, pw, gp, gs, beta, thresh, g=1.0, scale=1.0, dtype=torch.float64, variant=None):
    """-> dict: out [G,3], dz [B,C,hw] (as written with accumulate = 0), keep [B,G,hw], value_bound [G], weight_bound [G],
    dz_bound [B,C,hw], value [G] (= out[:,0]) as a tensor that autograd can follow when z requires grad.
    variant: None | "swapped" (teacher and student exchanged) | "no_beta_in_grad" | "gate_at_T" (the gate's sum at temperature T)"""
    z, u = z.to(dtype), u.to(dtype)
    B, C, hw = z.shape
    m = torch.ones(B, hw, dtype=dtype) if pw is None else pw.to(dtype).reshape(B, hw)
    G = len(gs)
    out = torch.zeros(G, 3, dtype=torch.float64)
    values = []
    dz = torch.zeros(B, C, hw, dtype=dtype)
    keep_all = torch.zeros(B, G, hw, dtype=torch.bool)
    vb, wb = torch.zeros(G, dtype=torch.float64), torch.zeros(G, dtype=torch.float64)
    dzb = torch.zeros(B, C, hw, dtype=torch.float64)
    th = torch.tensor(thresh, dtype=torch.float32)
    for gi, sl in enumerate(group_slices(gs)):
        zg, ug = z[:, sl], u[:, sl]
        if variant == "swapped":
            lq, q, A, La = _side(zg, beta)
            lp, p, Z, Lz = _side(ug, beta)
        else:
            lq, q, A, La = _side(ug, beta)
            lp, p, Z, Lz = _side(zg, beta)
        d = lq - lp
        kl = (q * d).sum(dim=1)
        omega = torch.ones(B, hw, dtype=dtype) if wprev is None else wprev.to(dtype)[:, gp[gi]]
        conf = gate_conf(beta * ug if variant == "gate_at_T" else ug, omega)
        keep = ~(conf.to(torch.float32) < th)            # fp32, <: a NaN is never dropped, thresh = 0 keeps everything
        keep_all[:, gi] = keep
        mo = m * omega
        val = torch.where(keep, mo * kl, torch.zeros_like(kl)).sum()
        values.append(val)
        out[gi, 0] = float(val.detach())
        out[gi, 1] = float(torch.where(keep, mo, torch.zeros_like(mo)).sum())
        out[gi, 2] = float(keep.sum())
        w = (g * scale) * mo * (1.0 if variant == "no_beta_in_grad" else beta)
        dz[:, sl] = torch.where(keep[:, None], w[:, None] * (p - q), torch.zeros_like(p))
        # ---- bounds (float64, from the quantities above; see the module docstring)
        f = lambda t: t.detach().to(torch.float64)      # noqa: E731
        qd = (f(q) * f(d).abs()).sum(dim=1)
        per = f(mo).abs() * (K_LOG * (f(A) + f(Z)) + K_LSE * (f(La) + f(Lz)) + K_ONE + qd * (K_Q * f(A) + K_QONE))
        per = SECOND * U * per + FLUSH * f(mo).abs() * f(d).abs().sum(dim=1)
        k64 = keep.to(torch.float64)
        vb[gi] = torch.nan_to_num(per * k64, nan=0.0, posinf=0.0).sum()
        wb[gi] = 2 * U * (f(mo).abs() * k64).sum()
        e = f(p) * (K_Q * f(Z)[:, None] + K_P) + f(q) * (K_Q * f(A)[:, None] + K_P) + K_W * (f(p) - f(q)).abs()
        dzb[:, sl] = (SECOND * U * e + FLUSH) * f(w).abs()[:, None] * k64[:, None]
    return dict(out=out, value=torch.stack(values), dz=dz, keep=keep_all, value_bound=vb, weight_bound=wb, dz_bound=dzb)


# ----------------------------------------------------------------------------- leaf enumeration (chain rule of KL)
def leaf_distributions(levels, beta):
    """levels: [(logits [B,C_L,hw], gp, gs)] with level 0 one group (softmax root).  -> [B,n_leaves,hw] composed leaf
    distribution: a node's probability is its parent's times its conditional; a node without children is a leaf."""
    probs, leaves = [], []
    for L, (v, gp, gs) in enumerate(levels):
        p = torch.zeros_like(v)
        for gi, sl in enumerate(group_slices(gs)):
            cond = torch.softmax(beta * v[:, sl], dim=1)
            p[:, sl] = cond if L == 0 else cond * probs[L - 1][:, gp[gi]:gp[gi] + 1]
        probs.append(p)
    for L, (v, gp, gs) in enumerate(levels):
        parents = set(levels[L + 1][1]) if L + 1 < len(levels) else set()
        for c in range(v.shape[1]):
            if c not in parents:
                leaves.append(probs[L][:, c])
    return torch.stack(leaves, dim=1), probs


def leaf_kl(teacher_levels, student_levels, beta):
    """sum over pixels of KL(teacher leaves || student leaves), and the teacher's composed probabilities per level"""
    qt, tprobs = leaf_distributions(teacher_levels, beta)
    ps, _ = leaf_distributions(student_levels, beta)
    return (qt * (torch.log(qt) - torch.log(ps))).sum(), tprobs


# ----------------------------------------------------------------------------- cases
# name: B, (H, W), group sizes, group parents (None: no wprev), Cprev, pw ("none" | "rand" | "zeros"), T, thresh, accumulate, gap
CASES = {
    "c1_single_pixel": (1, (1, 1), [1], None, 0, "none", 1.0, 0.0, 0, None),
    "c3_flat_pw_T05": (3, (7, 37), [3], None, 0, "rand", 0.5, 0.0, 0, None),
    "c4_flat_gated": (1, (33, 31), [4], None, 0, "none", 1.0, 0.6, 0, None),
    "c5_one_parent_T2": (3, (7, 37), [5], [1], 2, "none", 2.0, 0.0, 1, None),
    "c6_123_gated_pwzeros": (1, (41, 100), [1, 2, 3], [0, 1, 2], 3, "zeros", 1.0, 0.6, 0, None),
    "c8_215_gated_T2_acc": (3, (33, 31), [2, 1, 5], [2, 0, 2], 3, "none", 2.0, 0.6, 1, None),
    "c8_flat_acc": (1, (7, 37), [8], None, 0, "none", 1.0, 0.0, 1, None),
    "c9_gated_pw_T05": (3, (7, 37), [9], [0], 1, "rand", 0.5, 0.6, 0, None),
    "c16_flat": (1, (33, 31), [16], None, 0, "none", 1.0, 0.0, 0, None),
    "c16_ones_gated_T2": (3, (7, 37), [1] * 16, list(range(16)), 16, "rand", 2.0, 0.6, 0, None),
    "c4_22_big_gated_acc": (3, (41, 100), [2, 2], [1, 0], 2, "zeros", 1.0, 0.6, 1, None),
    "c4_teacher_gap": (1, (7, 37), [4], None, 0, "none", 1.0, 0.0, 0, "teacher"),
    "c8_215_student_gap": (3, (7, 37), [2, 1, 5], [1, 1, 0], 2, "rand", 2.0, 0.0, 0, "student"),
    "c3_12_both_gap_T05": (1, (33, 31), [1, 2], [0, 0], 1, "none", 0.5, 0.0, 1, "both"),
}
GATED = [k for k, v in CASES.items() if v[7] > 0]


def make_case(name):
    """-> dict of float32 torch tensors z, u [B,C,hw], wprev [B,Cprev,hw] or None, pw [B,hw] or None, dz0 [B,C,hw] (what an
    accumulating call adds to), g (float), scale (float) and the case's scalars"""
    B, (H, W), gs, gp, Cprev, pwmode, T, thresh, acc, gap = CASES[name]
    rng = np.random.RandomState(sum(ord(ch) * (i + 1) for i, ch in enumerate(name)))
    C, hw = sum(gs), H * W
    # (a gated case must keep a fair share of its pairs -- tests/test_distill_cpu.py asks for 20 % .. 80 % --, so its teacher is
    # surer of itself and its parents are likelier than a composed distribution over many parents would make them)
    u = ((3.0 if thresh > 0 else 1.5) * rng.randn(B, C, hw)).astype(np.float32)
    z = (u + 0.8 * rng.randn(B, C, hw)).astype(np.float32)
    wprev = None
    if gp is not None:
        raw = 3.0 * rng.randn(B, Cprev, hw)
        if thresh > 0:
            wprev = rng.uniform(0.45, 1.0, size=(B, Cprev, hw))
        elif Cprev == 1:
            wprev = 1.0 / (1.0 + np.exp(-(raw + 2.0)))
        else:
            e = np.exp(raw - raw.max(axis=1, keepdims=True))
            wprev = e / e.sum(axis=1, keepdims=True)
        wprev = wprev.astype(np.float32)
    pw = None
    if pwmode != "none":
        pw = rng.uniform(0.25, 2.0, size=(B, hw)).astype(np.float32)
        if pwmode == "zeros":
            pw[rng.rand(B, hw) < 0.3] = 0.0
    if gap is not None:
        sign = np.where(rng.rand(B, 1, hw) < 0.5, -100.0, 100.0).astype(np.float32)
        for sl in group_slices(gs):
            if gap in ("teacher", "both"):
                u[:, sl.start:sl.start + 1] += sign
            if gap == "student":
                z[:, sl.stop - 1:sl.stop] -= sign
            if gap == "both":           # the student is as sure of the opposite
                z[:, sl.start:sl.start + 1] -= sign
    beta = 1.0 / T
    if thresh > 0:          # move every conf away from the threshold, so that the fp32 comparison cannot depend on an ulp
        for _ in range(50):
            moved = False
            ut = torch.from_numpy(u).double()
            for gi, sl in enumerate(group_slices(gs)):
                omega = torch.ones(B, hw, dtype=torch.float64) if wprev is None else torch.from_numpy(wprev).double()[:, gp[gi]]
                near = ((gate_conf(ut[:, sl], omega) - thresh).abs() < GATE_MARGIN).numpy()
                if not near.any():
                    continue
                moved = True
                if wprev is not None:       # (conf <= omega: where the top child is certain only the parent can move it)
                    wprev[:, gp[gi]][near] *= np.float32(0.97)
                if sl.stop - sl.start > 1:
                    top = u[:, sl].argmax(axis=1)
                    bi, pi = np.nonzero(near)
                    u[bi, sl.start + top[bi, pi], pi] += np.float32(0.37)
            if not moved:
                break
        else:
            raise AssertionError(f"{name}: could not move every conf away from the threshold")
    dz0 = rng.randn(B, C, hw).astype(np.float32)
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a))      # noqa: E731
    return dict(name=name, B=B, H=H, W=W, C=C, hw=hw, gs=gs, gp=gp if gp is not None else [0] * len(gs), has_wprev=gp is not None,
                Cprev=Cprev, T=T, beta=beta, thresh=thresh, accumulate=acc, z=t(z), u=t(u), wprev=t(wprev), pw=t(pw), dz0=t(dz0),
                g=0.75, scale=1.0 / (B * hw))


_REF = {}


def reference(name):
    """the float64 reference of a case, computed once and shared (treat as read-only)"""
    if name not in _REF:
        c = make_case(name)
        _REF[name] = (c, tree_kl_ref(c["z"], c["u"], c["wprev"], c["pw"], c["gp"], c["gs"], c["beta"], c["thresh"], c["g"], c["scale"]))
    return _REF[name]


def check_against(name, out, dz, dz_accumulated=None):
    """the assertions both the fp32 CPU evaluation and the kernels must pass; -> list of violations (empty = inside the bounds)"""
    c, r = reference(name)
    bad = []
    out = torch.as_tensor(out, dtype=torch.float64)
    err = (out[:, 0] - r["out"][:, 0]).abs()
    if not bool((err <= r["value_bound"]).all()):
        bad.append(("value", err.tolist(), r["value_bound"].tolist()))
    err = (out[:, 1] - r["out"][:, 1]).abs()
    if not bool((err <= r["weight_bound"]).all()):
        bad.append(("weight", err.tolist(), r["weight_bound"].tolist()))
    if not torch.equal(out[:, 2], r["out"][:, 2]):
        bad.append(("count", out[:, 2].tolist(), r["out"][:, 2].tolist()))
    err = (torch.as_tensor(dz, dtype=torch.float64) - r["dz"]).abs()
    if not bool((err <= r["dz_bound"]).all()):
        bad.append(("dz", float((err - r["dz_bound"]).max())))
    if dz_accumulated is not None:
        want = c["dz0"].double() + r["dz"]
        err = (torch.as_tensor(dz_accumulated, dtype=torch.float64) - want).abs()
        if not bool((err <= r["dz_bound"] + U * want.abs()).all()):
            bad.append(("dz accumulated", float((err - r["dz_bound"] - U * want.abs()).max())))
    return bad
