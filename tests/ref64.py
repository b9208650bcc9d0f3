"""fp64 references with an error model for the bf16 hot-path kernels (tests/test_gpu_bf16_kernels.py, tests/test_ref64_host.py) and for the
text gate and CPAM kernels in fp32 and bf16 (tests/test_gpu_gates_ref64.py), and for the LayerNorm, cross-merge and depthwise SS2D kernels
(tests/test_gpu_ss2d_ref64.py), and for the MFMA linear and x_proj kernels (tests/test_gpu_gemm_ref64.py), and for the BatchNorm kernels of
csrc/bn.hip in both layouts, the pair, the segmented form and the statistics alone (tests/test_gpu_bn_ref64.py), and for the loss-term,
matcher-cost and box-refinement kernels of csrc/detrloss.hip and the clip / AdamW / EMA kernels of csrc/optim.hip (tests/test_gpu_loss_ref64.py).

Every reference takes the operands exactly as the kernel sees them (bf16 tensors, fp32 side inputs), promotes them to float64 and
computes on the CPU.  Next to each value it returns a magnitude: the same computation on absolute values.  check() then asserts,
elementwise,

    |got - ref| <= a * 2^-8 * |ref| + b * mag

`a` covers the kernel's final rounding to bf16 (0 where the kernel writes fp32); `b` covers fp32 accumulation (a small multiple of
2^-24 n) plus any intermediate bf16 rounding the kernel does on purpose.  There is no free absolute term: where the true value and its
magnitude are 0 the kernel must write an exact 0.  check() returns the worst err / bound ratio; with TAMTR_REF64_REPORT=<file> set it
also appends one JSON line per assertion to that file.
"""
import json
import math
import os

import torch

U8 = 2.0 ** -8     # bf16 unit roundoff: 8 significant bits, round to nearest
U24 = 2.0 ** -24   # fp32 unit roundoff


def fp32_b(n):
    """b for an fp32 result of a serial chain of n roundings (accumulation, products, exp / rsqrt)."""
    return n * U24


def _d(t):
    return t.detach().cpu().double()


def check(what, got, ref, mag, a, b, log=True, envelope=None, tiny=0.0):
    """Elementwise |got - ref| <= a 2^-8 |ref| + b mag.  NaN in ref must be NaN in got (and only there).  Returns the worst ratio.
    log=False: one piece of a larger tensor (see report()).
    envelope = (lo, hi), lo <= ref <= hi elementwise: the reference is an interval (an operand that the operation rounds on purpose may
    fall on either neighbour); the error is the distance of got from [lo, hi], 0 inside it, and the bound is unchanged.
    tiny: the one absolute term a caller may ask for, and only as fp32's underflow threshold (FLT_MIN times the factors that follow the
    underflow): a product below 2^-126 may be flushed to 0 or lose bits as a denormal.  Both default to the plain rule."""
    got, ref, mag = _d(got), _d(ref), _d(mag)
    assert got.shape == ref.shape == mag.shape, f'{what}: shapes {tuple(got.shape)} {tuple(ref.shape)} {tuple(mag.shape)}'
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(got), nan), f'{what}: NaN pattern differs ({int(torch.isnan(got).sum())} vs {int(nan.sum())})'
    live = ~nan
    assert bool(torch.isfinite(got[live]).all()), f'{what}: non-finite output'
    if envelope is None:
        err = (got - ref).abs()[live]
    else:
        lo, hi = _d(envelope[0]), _d(envelope[1])
        assert lo.shape == hi.shape == ref.shape and bool(((lo <= ref) & (ref <= hi))[live].all()), f'{what}: the envelope does not hold the reference'
        err = torch.maximum(lo - got, got - hi).clamp_min(0)[live]
    bound = (a * U8 * ref.abs() + b * mag + tiny)[live]
    zero = bound == 0
    assert bool((err[zero] == 0).all()), f'{what}: {int((err[zero] != 0).sum())} elements must be exactly 0 and are not'
    ratio = torch.zeros_like(err)
    ratio[~zero] = err[~zero] / bound[~zero]
    worst = float(ratio.max()) if ratio.numel() else 0.0
    if log:
        report(what, worst, a, b, err.numel())
    if worst > 1:
        i = int(ratio.argmax())
        r, g, bd = ref[live][i], got[live][i], bound[i]
        raise AssertionError(f'{what}: err / bound = {worst:.3g} at flat {i}: got {float(g):.9g} ref {float(r):.9g} bound {float(bd):.3g} '
                             f'({int((ratio > 1).sum())} of {ratio.numel()} over)')
    return worst


def report(what, worst, a, b, n):
    """With TAMTR_REF64_REPORT=<file> set, append the worst err / bound ratio of one assertion to that file as a JSON line."""
    path = os.environ.get('TAMTR_REF64_REPORT')
    if path:
        with open(path, 'a') as f:
            f.write(json.dumps({'check': what, 'worst': worst, 'a': a, 'b': b, 'n': int(n)}) + '\n')


def note(text):
    """With TAMTR_REF64_REPORT=<file> set, append a line of text (a fact about the run, not an assertion) to that file."""
    path = os.environ.get('TAMTR_REF64_REPORT')
    if path:
        with open(path, 'a') as f:
            f.write(json.dumps({'note': text}) + '\n')


def old_close(got, ref, rtol, atol):
    """The tolerance rule the suite used before these references: |got - ref| <= atol + rtol |ref| (tests/conftest.py assert_close)."""
    got, ref = _d(got), _d(ref)
    return bool(((got - ref).abs() <= atol + rtol * ref.abs()).all())


# ------------------------------------------------------------------------------------------------ contrastive head
def contrastive(x, w, logit_scale, bias, g):
    """csrc/contrastive.hip: logits = <x/|x|, w/|w|> exp(logit_scale) + bias, and its backward for the cotangent g (fp32 [B,Q,K]).

    x [B,Q,C] as the kernel reads it (bf16 or fp32), w fp32 [B,K,C].  Rounding points: none on purpose.  The logits, d(what) and
    therefore dw are fp32 (a = 0); dx is stored in x's dtype (a = 1 for bf16).  Returns {name: (value, magnitude)} for
    logits, dx, dw."""
    from oracle import tamtr_oracle as O
    xr, wr = _d(x).requires_grad_(), _d(w).requires_grad_()
    ls, bi = _d(logit_scale).reshape(()), _d(bias).reshape(1)
    out = O.contrastive_head(xr, wr, {'logit_scale': ls, 'bias': bi})
    gd = _d(g)
    (out * gd).sum().backward()
    sc = math.exp(float(ls))
    with torch.no_grad():
        xi = 1 / xr.norm(dim=-1, keepdim=True).clamp_min(1e-12)
        wi = 1 / wr.norm(dim=-1, keepdim=True).clamp_min(1e-12)
        xh, wh = (xr * xi).abs(), (wr * wi).abs()
        m_log = sc * torch.einsum('bqc,bkc->bqk', xh, wh) + bi.abs()
        dh = sc * torch.einsum('bqk,bkc->bqc', gd.abs(), wh)                   # d xhat = s sum_k g what
        m_dx = xi * (dh + xh * (dh * xh).sum(-1, keepdim=True))
        dw_ = sc * torch.einsum('bqk,bqc->bkc', gd.abs(), xh)                  # d what = s sum_q g xhat
        m_dw = wi * (dw_ + wh * (dw_ * wh).sum(-1, keepdim=True))
    return {'logits': (out.detach(), m_log), 'dx': (xr.grad, m_dx), 'dw': (wr.grad, m_dw)}


# ------------------------------------------------------------------------------------------------ self-attention
def attention(q, k, v, nh, mask, go):
    """csrc/selfattn.hip: o = softmax(q k^T / sqrt(dh), blocked = -inf) v per head, and dq, dk, dv for the cotangent go.

    q, k, v, go [B,Q,C] bf16 (strided views are fine), mask bool [Q,Q] (True = blocked) or None.  A fully blocked row gives NaN (0/0), in
    its output row, its dq row, and - through delta_i = <dO_i, O_i> - in every dk; dv treats that row's P as 0, as the kernel does.
    Rounding points of the MFMA kernels (dh = 64, 16-byte aligned operands): P is packed to bf16 before PV and before dV = P^T dO; dS is
    packed to bf16 before dQ = dS K and dK = dS^T Q; delta_i is formed from the stored (bf16) O.  The scalar kernels round only their
    stores.  Magnitudes: o: sum_j p_j |v_j|;  dv: sum_i p_ij |dO_i|;  dq / dk: scale sum p_ij (|dP_ij| + sum_c |dO_ic O_ic|) |k_j| / |q_i|
    (the second term carries delta's error from the rounded O).  Returns {name: (value, magnitude)} for o, dq, dk, dv, each [B,Q,C]."""
    B, Q, C = q.shape
    dh = C // nh
    sc = dh ** -0.5

    def heads(t):
        return _d(t).reshape(B, Q, nh, dh).transpose(1, 2)
    qh, kh, vh, gh = heads(q), heads(k), heads(v), heads(go)
    s = qh @ kh.transpose(-1, -2) * sc
    if mask is not None:
        s = s.masked_fill(mask.cpu()[None, None], float('-inf'))
    p = torch.softmax(s, -1)                                # NaN rows where everything is blocked
    o = p @ vh
    dead = torch.isnan(p[..., :1])                          # [B,nh,Q,1]
    p0 = torch.where(dead, torch.zeros_like(p), p)
    dv = p0.transpose(-1, -2) @ gh
    dp = gh @ vh.transpose(-1, -2)
    dl = (gh * o).sum(-1, keepdim=True)
    ds = p * (dp - dl) * sc
    dq, dk = ds @ kh, ds.transpose(-1, -2) @ qh
    dl_m = (gh.abs() * o.abs()).sum(-1, keepdim=True)
    dsm = p0 * (dp.abs() + dl_m) * sc
    m_o = p.abs() @ vh.abs()
    m_dv = p0.transpose(-1, -2) @ gh.abs()
    m_dq = dsm @ kh.abs()
    m_dk = dsm.transpose(-1, -2) @ qh.abs()

    def back(t):
        return t.transpose(1, 2).reshape(B, Q, C)
    return {n: (back(a), back(m)) for n, a, m in (('o', o, m_o), ('dq', dq, m_dq), ('dk', dk, m_dk), ('dv', dv, m_dv))}


# ------------------------------------------------------------------------------------------------ deformable core
def pixel_coords(loc, W, H):
    """The kernel's x = loc_x W - 0.5, y = loc_y H - 0.5 in fp32 (one rounding: the compiler contracts it to an FMA; the fp64 product of an
    fp32 by a level size is exact, so rounding it once to fp32 gives the FMA's result), then floor and the fractions, exactly as fp32."""
    x = (_d(loc[..., 0]) * W - 0.5).float().double()
    y = (_d(loc[..., 1]) * H - 0.5).float().double()
    return x, y


def msda(value, shapes, loc, aw, gout):
    """csrc/msdeform.hip: out[b,q,m] = sum_{l,p,corner on the map} a w_corner value[b, row, m], and d(value), d(loc), d(aw), colw (the
    on-map weight of every (b, q, m)) for the cotangent gout [B,Q,M*D] (bf16, as the kernel reads it).

    value [B,L,M,D] bf16, loc [B,Q,M,nl,P,2] fp32, aw [B,Q,M,nl,P] fp32.  The pixel coordinate is formed in fp32 as the kernel forms it
    (pixel_coords), so floor() picks the same corners; d(loc) = W * d/d(fx).  No intermediate rounding: out and d(value) are stored in bf16
    (a = 1), d(loc), d(aw), colw in fp32 (a = 0).  Magnitudes: the same sums over |a|, |w|, |value|, |gout|, with the corner differences
    of d(loc) taken as sums.  Returns {name: (value, magnitude)} for out [B,Q,M*D], gvalue [B,L,M,D], gloc, gaw, colw, and 'runs': the
longest list of corners summed into one row of d(value)."""
    B, L, M, D = value.shape
    _, Q, _, nl, P, _ = loc.shape
    v, a, g = _d(value), _d(aw), _d(gout).view(B, Q, M, D)
    out, m_out = torch.zeros(B, Q, M, D, dtype=torch.float64), torch.zeros(B, Q, M, D, dtype=torch.float64)
    gval, m_gval = torch.zeros(B * L * M, D, dtype=torch.float64), torch.zeros(B * L * M, D, dtype=torch.float64)
    gloc, m_gloc = torch.zeros(B, Q, M, nl, P, 2, dtype=torch.float64), torch.zeros(B, Q, M, nl, P, 2, dtype=torch.float64)
    gaw, m_gaw = torch.zeros(B, Q, M, nl, P, dtype=torch.float64), torch.zeros(B, Q, M, nl, P, dtype=torch.float64)
    colw, m_colw = torch.zeros(B, Q, M, dtype=torch.float64), torch.zeros(B, Q, M, dtype=torch.float64)
    runs = torch.zeros(B * L * M, dtype=torch.float64)
    bi = torch.arange(B).view(B, 1, 1, 1)
    mi = torch.arange(M).view(1, 1, M, 1)
    start = 0
    for l, (H, W) in enumerate(shapes):
        H, W = int(H), int(W)
        x, y = pixel_coords(loc[:, :, :, l], W, H)          # [B,Q,M,P]
        xf, yf = torch.floor(x), torch.floor(y)
        fx, fy = x - xf, y - yf
        al = a[:, :, :, l]
        s_aw, s_x, s_y = (torch.zeros_like(x) for _ in range(3))
        m_s, m_x, m_y = (torch.zeros_like(x) for _ in range(3))
        for dy in (0, 1):
            for dx in (0, 1):
                wx, wy = (fx if dx else 1 - fx), (fy if dy else 1 - fy)
                sx, sy = (1.0 if dx else -1.0), (1.0 if dy else -1.0)
                xi, yi = (xf + dx).long(), (yf + dy).long()
                ok = ((xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)).double()
                row = start + yi.clamp(0, H - 1) * W + xi.clamp(0, W - 1)
                samp = v[bi, row, mi]                        # [B,Q,M,P,D]
                wgt = wx * wy * ok * al
                out += (samp * wgt.unsqueeze(-1)).sum(3)
                m_out += (samp.abs() * wgt.abs().unsqueeze(-1)).sum(3)
                flat = ((bi * L + row) * M + mi).reshape(-1)
                contrib = (wgt.unsqueeze(-1) * g.unsqueeze(3)).reshape(-1, D)
                gval.index_add_(0, flat, contrib)
                m_gval.index_add_(0, flat, contrib.abs())
                runs.index_add_(0, flat, ok.reshape(-1))
                dc = (samp * g.unsqueeze(3)).sum(-1) * ok
                dm = (samp.abs() * g.abs().unsqueeze(3)).sum(-1) * ok
                s_aw += wx * wy * dc
                m_s += wx * wy * dm
                s_x += sx * wy * dc
                m_x += wy * dm
                s_y += sy * wx * dc
                m_y += wx * dm
                colw += (wx * wy * ok * al).sum(-1)
                m_colw += (wx * wy * ok * al.abs()).sum(-1)
        gaw[:, :, :, l], m_gaw[:, :, :, l] = s_aw, m_s
        gloc[:, :, :, l, :, 0], m_gloc[:, :, :, l, :, 0] = s_x * al * W, m_x * al.abs() * W
        gloc[:, :, :, l, :, 1], m_gloc[:, :, :, l, :, 1] = s_y * al * H, m_y * al.abs() * H
        start += H * W
    return {'out': (out.reshape(B, Q, M * D), m_out.reshape(B, Q, M * D)),
            'gvalue': (gval.view(B, L, M, D), m_gval.view(B, L, M, D)),
            'gloc': (gloc, m_gloc), 'gaw': (gaw, m_gaw), 'colw': (colw, m_colw), 'runs': int(runs.max())}


# ------------------------------------------------------------------------------------------------ ln_gate
def ln_gate(x, xz, gamma, beta, gout, eps=1e-5):
    """csrc/ss2d_out.hip ln_gate: out = LayerNorm(x; gamma, beta) * SiLU(z), z = xz[..., D:], and dx, d(xz), dgamma, dbeta for gout.

    x fp32 [N, D], xz bf16 [N, >= 2D] (only z is read), gout bf16 [N, D].  No intermediate rounding: out and d(z) are stored in bf16
    (a = 1), dx, dgamma, dbeta in fp32 (a = 0).  The magnitude of xhat is |xhat| + rstd mean|x| (the fp32 mean is subtracted before the
    scaling, so its error is absolute); SiLU' is taken as sg (1 + |z| (1 - sg)) (it has a zero near z = -1.28).
    Returns {name: (value, magnitude)} for out, dx, dz, dgamma, dbeta."""
    import torch.nn.functional as F
    N, D = x.shape
    xr, zr = _d(x).requires_grad_(), _d(xz)[:, D:2 * D].clone().requires_grad_()
    gr, br = _d(gamma).requires_grad_(), _d(beta).requires_grad_()
    out = F.layer_norm(xr, (D,), gr, br, eps) * F.silu(zr)
    gd = _d(gout)
    (out * gd).sum().backward()
    with torch.no_grad():
        xd = xr.detach()
        mu = xd.mean(-1, keepdim=True)
        rstd = (((xd - mu) ** 2).mean(-1, keepdim=True) + eps).rsqrt()
        X = ((xd - mu) * rstd).abs() + rstd * xd.abs().mean(-1, keepdim=True)
        z = zr.detach()
        sg = torch.sigmoid(z)
        silu = (z * sg).abs()
        my = gr.detach().abs() * X + br.detach().abs()
        m_out = my * silu
        gxh = gd.abs() * silu * gr.detach().abs()
        m_dx = rstd * (gxh + gxh.mean(-1, keepdim=True) + X * (gxh * X).mean(-1, keepdim=True))
        m_dz = gd.abs() * my * sg * (1 + z.abs() * (1 - sg))
        m_dg = (gd.abs() * silu * X).sum(0)
        m_db = (gd.abs() * silu).sum(0)
    return {'out': (out.detach(), m_out), 'dx': (xr.grad, m_dx), 'dz': (zr.grad, m_dz), 'dgamma': (gr.grad, m_dg), 'dbeta': (br.grad, m_db)}


# ------------------------------------------------------------------------------------------------ __expf inside the sigmoids
# Worst |__expf(x) - exp(x)| / exp(x) on gfx950 in units of 2^-24, for |x| below each key: measured by tools/micro/expf_error.hip over
# 2^24 evenly spaced arguments per range and sign (profiles/r08_gates_ref64.txt keeps the run's output).  The ROCm headers state no bound for
# __expf (it is the native v_exp_f32 of x log2(e) rounded to fp32, so the error grows with |x|).  expf_b() doubles the measured figure:
# the measurement samples the range and does not prove a maximum.
# Measured on an MI355X; the larger of the two signs per range.  (The counted part agrees: the fp32 rounding of x log2(e) moves exp by
# up to |x| 2^-24, and v_exp_f32 adds about one ulp.)
EXPF_ULPS = {1: 2.180, 2: 3.032, 4: 4.868, 8: 8.477, 16: 15.911, 32: 30.376, 64: 59.708}
EXPF_MARGIN = 2.0


def expf_b(zmax):
    """b for one __expf whose argument stays within |x| <= zmax: EXPF_MARGIN times the measured worst relative error of that range."""
    for hi in sorted(EXPF_ULPS):
        if zmax < hi:
            return EXPF_MARGIN * EXPF_ULPS[hi] * U24
    raise ValueError(f'__expf was not measured for |x| up to {zmax}')


def sig_mag(s, m_arg):
    """Magnitude of s = sigmoid(z), given the magnitude m_arg of z: s (1 + (1 - s) m_arg).  The sigmoid's own roundings are relative to
    s; an error e in z moves s by s (1 - s) e."""
    return s * (1 + (1 - s) * m_arg)


def ambiguous(gap, mag, b):
    """Number of argmax decisions that fp32 could legitimately take the other way: the fp64 gap between the two largest values is below
    twice their forward bound b * mag.  The gradients routed by such an argmax are discontinuous there; test inputs must have none."""
    return int((gap < 2 * b * mag).sum())


# ------------------------------------------------------------------------------------------------ max-sigmoid text gate
def maxsigmoid_gate(x, gk, bias, v, nh, scale, gout, v_affine=None):
    """csrc/gate.hip: out = v sigmoid(max_t <x, gk_t> / sqrt(hc) + bias) scale per (image, head, pixel), and dv, dx, dlogit (the
    derivative by the winning dot product), dgk, dbias for the cotangent gout (None: forward only).

    x, v, gout [B,C,H,W] as the kernel reads them (bf16 or fp32, any layout), gk fp32 [B,T,C], bias fp32 [nh].  With v_affine =
    (mean_rstd [C,2], gamma [C], beta [C]) it is the forward of gate_cl_fwd_kernel: v is the raw convolution output and the kernel applies
    v (rstd gamma) + (beta - mean rstd gamma) in its load.  The first maximum over the text rows wins (torch.argmax: first occurrence).
    Rounding points: none on purpose.  The dot products, the gate a and dlogit are fp32; the backward reads the stored fp32 a and forms
    1 - a from it.  out, dv, dx are stored in x's dtype (a = 1 for bf16, 0 for fp32); dlogit, dgk, dbias are fp32 (a = 0), dgk and dbias
    being fp32 reductions over the pixels (b grows by fp32_b of their length).
    Magnitudes: the same computation on absolute values, with the logit's |dot| / sqrt(hc) + |bias|, the gate's sig_mag(a, that), and
    1 + (magnitude of a) for 1 - a: the kernel subtracts a rounded a from 1, so a saturated gate keeps no relative accuracy there.
    Returns {name: (value, magnitude)} for out [B,C,H,W], dv, dx, dlogit [B,nh,HW], dgk [B,T,C], dbias [nh], and 'arg' (the fp64 argmax,
    [B,nh,HW]), 'gap' (largest minus second largest dot product, inf at T = 1), 'gap_mag' (the larger magnitude of those two dot
    products), 'zmax' (the largest |logit|: the range of the sigmoid's __expf)."""
    B, C, H, W = x.shape
    T, hc, HW = gk.shape[1], C // nh, H * W
    sc = abs(float(scale))
    xd = _d(x).reshape(B, nh, hc, HW)
    g = _d(gk).reshape(B, T, nh, hc)
    bi = _d(bias).reshape(1, nh, 1)
    vd = _d(v).reshape(B, nh, hc, HW)
    m_v = vd.abs()
    if v_affine is not None:
        mr, ga, be = (_d(t) for t in v_affine)
        mean, k, be = mr[:, 0].reshape(1, nh, hc, 1), (mr[:, 1] * ga).reshape(1, nh, hc, 1), be.reshape(1, nh, hc, 1)
        m_v = vd.abs() * k.abs() + be.abs() + (mean * k).abs()
        vd = vd * k + (be - mean * k)
    dots = torch.einsum('bmcp,bnmc->bmpn', xd, g)                 # [B,nh,HW,T]
    m_dots = torch.einsum('bmcp,bnmc->bmpn', xd.abs(), g.abs())
    arg = dots.argmax(-1)
    best, m_best = dots.gather(-1, arg[..., None])[..., 0], m_dots.gather(-1, arg[..., None])[..., 0]
    if T > 1:
        top = dots.topk(2, -1)
        gap, gap_mag = top.values[..., 0] - top.values[..., 1], m_dots.gather(-1, top.indices).amax(-1)
    else:
        gap, gap_mag = torch.full_like(best, float('inf')), m_best
    rs = math.sqrt(hc)
    z, m_z = best / rs + bi, m_best / rs + bi.abs()
    a = torch.sigmoid(z)
    m_a = sig_mag(a, m_z)
    res = {'out': ((vd * a.unsqueeze(2) * scale).reshape(B, C, H, W), (m_v * m_a.unsqueeze(2) * sc).reshape(B, C, H, W)),
           'arg': arg, 'gap': gap, 'gap_mag': gap_mag, 'zmax': float(z.abs().max())}
    if gout is None:
        return res
    go = _d(gout).reshape(B, nh, hc, HW)
    res['dv'] = ((go * a.unsqueeze(2) * scale).reshape(B, C, H, W), (go.abs() * m_a.unsqueeze(2) * sc).reshape(B, C, H, W))
    daw, m_daw = (go * vd).sum(2), (go.abs() * m_v).sum(2)        # [B,nh,HW]
    dl, m_dl = daw * scale * a * (1 - a) / rs, m_daw * sc * m_a * (1 + m_a) / rs
    res['dlogit'] = (dl, m_dl)
    gsel = g.permute(0, 2, 1, 3).gather(2, arg[..., None].expand(B, nh, HW, hc))      # the winning text row, [B,nh,HW,hc]
    res['dx'] = ((dl[..., None] * gsel).transpose(2, 3).reshape(B, C, H, W), (m_dl[..., None] * gsel.abs()).transpose(2, 3).reshape(B, C, H, W))
    hot = torch.nn.functional.one_hot(arg, T).double()            # [B,nh,HW,T]
    res['dgk'] = (torch.einsum('bmpn,bmp,bmcp->bnmc', hot, dl, xd).reshape(B, T, C),
                  torch.einsum('bmpn,bmp,bmcp->bnmc', hot, m_dl, xd.abs()).reshape(B, T, C))
    res['dbias'] = (dl.sum((0, 2)) * rs, m_dl.sum((0, 2)) * rs)
    return res


# ------------------------------------------------------------------------------------------------ CPAM
def _up2_taps(n):
    """upsample_bilinear2d(scale 2, align_corners=False) along one axis of n pooled cells: for each of the 2n pixels the two cells and
    the second one's weight: src = max((o + 0.5) / 2 - 0.5, 0), i0 = floor(src), i1 = min(i0 + 1, n - 1), lam = src - i0."""
    o = torch.arange(2 * n, dtype=torch.float64)
    src = ((o + 0.5) / 2 - 0.5).clamp_min(0)
    i0 = src.floor().long()
    return i0, (i0 + 1).clamp_max(n - 1), src - i0


def _up2(p):
    """Bilinear x2 of p [..., Hp, Wp].  Pixel row / column 0 sits on cell 0 (lam = 0).  The kernels (make_taps in csrc/cpam.hip) form it as
    0 * p[0] + 1 * p[0]: their zero-weight tap is the clamped cell 0 itself, where torch's is cell 1.  For finite p all three agree; a
    non-finite p[0] gives NaN there (0 * inf), and a non-finite p[1] does not reach pixel 0.  This reference does as the kernels do."""
    Hp, Wp = p.shape[-2:]
    y0, y1, ly = _up2_taps(Hp)
    x0, x1, lx = _up2_taps(Wp)

    def mix(a, b, lam):
        return torch.where(lam == 0, 0 * a + a, (1 - lam) * a + lam * b)
    rows0, rows1 = p[..., y0, :], p[..., y1, :]
    top, bot = mix(rows0[..., x0], rows0[..., x1], lx), mix(rows1[..., x0], rows1[..., x1], lx)
    return mix(top, bot, ly[:, None])


def _up2_adjoint(du):
    """The adjoint of _up2's weights applied to du [..., H, W]: dp[k, l] = sum over the pixels that tap cell (k, l) of wy wx du."""
    H, W = du.shape[-2:]
    Hp, Wp = H // 2, W // 2
    y0, y1, ly = _up2_taps(Hp)
    x0, x1, lx = _up2_taps(Wp)
    t = torch.zeros(du.shape[:-2] + (Hp, W), dtype=du.dtype)
    t.index_add_(-2, y0, du * (1 - ly)[:, None])
    t.index_add_(-2, y1, du * ly[:, None])
    dp = torch.zeros(du.shape[:-2] + (Hp, Wp), dtype=du.dtype)
    dp.index_add_(-1, x0, t * (1 - lx))
    dp.index_add_(-1, x1, t * lx)
    return dp


def _first_max(t, dim):
    """max and argmax along dim: the first maximum wins, a NaN wins over everything and the first NaN stays (torch.max's values; the
    index rule is written out because the kernels depend on it)."""
    nan = torch.isnan(t)
    idx = torch.where(nan.any(dim), nan.double().argmax(dim), torch.where(nan, torch.full_like(t, float('-inf')), t).argmax(dim))
    return t.gather(dim, idx.unsqueeze(dim)).squeeze(dim), idx


def cpam(x, gout):
    """csrc/cpam.hip (both layouts) with its max-pool (csrc/pool.hip, pool3s2_cl_*): p = maxpool 3x3 / stride 2 / padding 1 of x,
    c = sigmoid(bilinear_x2(p)) x, out = sigmoid(max over the chunk's channels of c) c for each of the 8 channel chunks, and dx for the
    cotangent gout (None: forward only).

    x, gout [B,C,H,W] as the kernel reads them (bf16 or fp32, any layout), H and W even.  The pool is written out: padding is -inf, the
    first maximum in row-major window order wins (bf16 maps have many exact ties inside a window, and the backward routes dp to the
    winner); NaN wins.  The chunk maximum: the first maximum wins, NaN wins.  The bilinear x2 is written out with align_corners=False
    clamping (_up2).
    Rounding points for bf16 (cpam_bwd_kernel / cpam_dp_kernel / tamtr_maxpool_bwd and their _cl_ forms): p is exact (a maximum of bf16
    values is one of them); out is rounded once (a = 1); s2 is kept in fp32 (a = 0).  The backward stores dxd (the direct part of dx), du
    and dp each in the map's dtype, and dx is the rounded sum of dxd and the up to four dp values routed to the pixel (a = 1).  So for
    bf16 b of dx is 2^-8 on the stored intermediates plus the fp32 chain, and the magnitude of dx counts the pooled path twice (du and dp
    are two roundings of it): mag = |dxd| + 2 sum |dp|.  For fp32 b is the fp32 chain alone.
    This bound of dx is the worst case of its honest roundings (dxd, du, dp, the sum), which one more rounding on the pooled path seldom
    exceeds: a du rounded twice passes it.  That mistake is caught on the stored du, which is held to a single rounding.
    Magnitudes: the same computation on absolute values, with sig_mag for both sigmoids and 1 + (magnitude of s) for 1 - s.
    The stored intermediates are returned too (the C entry points hand them out): dxd and du are rounded once (a = 1), dp is a rounded
    sum of rounded du (a = 1, b with 2^-8 on its magnitude).
    Returns {name: (value, magnitude)} for out, dx, dxd, du [B,C,H,W], dp [B,C,H/2,W/2], s2 [B,8,H,W], and 'p' (exact), 'arg' (the fp64 argmax channel inside its
    chunk, [B,8,H,W]), 'gap' (largest minus second largest c of the chunk, inf for one channel per chunk), 'gap_mag' (the larger magnitude
    of those two), 'zmax' (the largest argument of either sigmoid)."""
    import torch.nn.functional as F
    xd = _d(x)
    B, C, H, W = xd.shape
    Hp, Wp, Cg = H // 2, W // 2, C // 8
    win = F.pad(xd, (1, 1, 1, 1), value=float('-inf')).unfold(2, 3, 2).unfold(3, 3, 2).reshape(B, C, Hp, Wp, 9)
    p, widx = _first_max(win, -1)                                  # widx = dh * 3 + dw inside the unclipped window
    u, m_u = _up2(p), _up2(p.abs())
    s1 = torch.sigmoid(u)
    m_s1 = sig_mag(s1, torch.where(torch.isfinite(m_u), m_u, torch.zeros_like(m_u)))
    c, m_c = s1 * xd, m_s1 * xd.abs()
    cg, m_cg = c.view(B, 8, Cg, H, W), m_c.view(B, 8, Cg, H, W)
    m, am = _first_max(cg, 2)                                      # [B,8,H,W]
    m_m = m_cg.gather(2, am.unsqueeze(2)).squeeze(2)
    if Cg > 1:
        top = torch.where(torch.isnan(cg), torch.full_like(cg, float('-inf')), cg).topk(2, 2)
        gap, gap_mag = top.values[:, :, 0] - top.values[:, :, 1], m_cg.gather(2, top.indices).amax(2)
    else:
        gap, gap_mag = torch.full_like(m, float('inf')), m_m
    s2 = torch.sigmoid(m)
    m_s2 = sig_mag(s2, torch.where(torch.isfinite(m_m), m_m, torch.zeros_like(m_m)))
    out, m_out = (s2.unsqueeze(2) * cg).reshape(B, C, H, W), (m_s2.unsqueeze(2) * m_cg).reshape(B, C, H, W)
    fin = torch.cat([u[torch.isfinite(u)].abs().flatten(), m[torch.isfinite(m)].abs().flatten()])
    res = {'out': (out, m_out), 's2': (s2, m_s2), 'p': p, 'arg': am, 'gap': gap, 'gap_mag': gap_mag, 'zmax': float(fin.max()) if fin.numel() else 0.0}
    if gout is None:
        return res
    go = _d(gout).view(B, 8, Cg, H, W)
    S, m_S = (go * cg).sum(2), (go.abs() * m_cg).sum(2)
    dm, m_dm = s2 * (1 - s2) * S, m_s2 * (1 + m_s2) * m_S
    hot = F.one_hot(am, Cg).permute(0, 1, 4, 2, 3).double()        # [B,8,Cg,H,W]
    dc = (go * s2.unsqueeze(2) + hot * dm.unsqueeze(2)).reshape(B, C, H, W)
    m_dc = (go.abs() * m_s2.unsqueeze(2) + hot * m_dm.unsqueeze(2)).reshape(B, C, H, W)
    dxd, m_dxd = dc * s1, m_dc * m_s1
    du, m_du = dc * xd * s1 * (1 - s1), m_dc * xd.abs() * m_s1 * (1 + m_s1)
    dp, m_dp = _up2_adjoint(du), _up2_adjoint(m_du)                # [B,C,Hp,Wp]
    # the pool's backward: cell (k, l) sends dp to pixel (2k - 1 + dh, 2l - 1 + dw) of its winner
    k, l = torch.arange(Hp).view(1, 1, Hp, 1), torch.arange(Wp).view(1, 1, 1, Wp)
    pix = ((2 * k - 1 + widx // 3) * W + (2 * l - 1 + widx % 3)).reshape(B, C, Hp * Wp)
    pooled, m_pooled = torch.zeros(B, C, H * W, dtype=torch.float64), torch.zeros(B, C, H * W, dtype=torch.float64)
    pooled.scatter_add_(2, pix, dp.reshape(B, C, Hp * Wp))
    m_pooled.scatter_add_(2, pix, m_dp.reshape(B, C, Hp * Wp))
    res.update({'dxd': (dxd, m_dxd), 'du': (du, m_du), 'dp': (dp, m_dp)})
    res['dx'] = (dxd + pooled.view(B, C, H, W), m_dxd + 2 * m_pooled.view(B, C, H, W))
    return res


# ------------------------------------------------------------------------------------------------ a and b of the gate and CPAM checks
def gate_bounds(hc, HW, B, zmax, bf16):
    """{name: (a, b)} for maxsigmoid_gate's outputs; every figure is a count of fp32 roundings along the kernel's chain.
    The gate a: hc FMAs, / sqrt(hc), + bias (hc + 2), negate-free __expf (expf_b), 1 + e and 1 / (.) (2): hc + 4 and one __expf.
    out: the gate, a * scale and * v (2); the channels-last kernel adds rsqrtf and the three roundings of the folded affine (4) and sums
    its dot product in fewer steps: hc + 12 covers both.  dv: the same chain.  dlogit: hc FMAs of gout v, the gate twice (a and 1 - a),
    the subtraction, three products and the division (6): 3 hc + 18 and two __expf.  dx: one more product.  dgk: dlogit times x summed
    over the HW pixels; dbias: dlogit summed over B HW pixels, times sqrt(hc)."""
    e = expf_b(zmax)
    a = 1 if bf16 else 0
    b_out, b_dl = fp32_b(hc + 12) + e, fp32_b(3 * hc + 18) + 2 * e
    return {'out': (a, b_out), 'dv': (a, b_out), 'dlogit': (0, b_dl), 'dx': (a, b_dl + fp32_b(1)),
            'dgk': (0, b_dl + fp32_b(HW + 1)), 'dbias': (0, b_dl + fp32_b(B * HW + 1))}


CPAM_C_N = 10   # roundings of c = sigmoid(u) x besides its __expf: the bilinear taps (2 products + 1 sum, twice: 6), 1 + e, 1 / (.), * x; +1 spare


def cpam_bounds(Cg, zmax, bf16):
    """{name: (a, b)} for cpam's outputs, and 'c': (0, b) of the gated value that the chunk argmax compares.
    c: CPAM_C_N and one __expf.  s2 = sigmoid(max c): c's chain, 1 + e, 1 / (.), one spare (3) and a second __expf.  out = s2 c: both
    chains and the product: 24 and three __expf; rounded once to the map's dtype.  dx: S = sum of gout c over the chunk (Cg + c's
    chain), dm = s2 (1 - s2) S (s2's chain twice + 3), dc (2), dxd = dc s1 (c's chain), du = dc x s1 (1 - s1) (c's chain twice + 4),
    dp (four weighted taps per row, four rows: 12), the pool's sum of up to four dp (4): Cg + 80 covers it, with eight __expf; in
    bf16 the stored dxd, du and dp add 2^-8 of the magnitude (ref64.cpam counts the pooled path twice for du and dp).  The stored dxd, du
    and dp are held to the same chain (dp with 2^-8 for the rounded du it sums)."""
    e = expf_b(zmax)
    a = 1 if bf16 else 0
    chain = fp32_b(Cg + 80) + 8 * e
    return {'c': (0, fp32_b(CPAM_C_N) + e), 's2': (0, fp32_b(CPAM_C_N + 3) + 2 * e), 'out': (a, fp32_b(24) + 3 * e),
            'dxd': (a, chain), 'du': (a, chain), 'dp': (a, (U8 if bf16 else 0) + chain), 'dx': (a, (U8 if bf16 else 0) + chain)}


# ------------------------------------------------------------------------------------------------ LayerNorm (csrc/ss2d_out.hip)
def layer_norm(x, gamma, beta, gout, eps=1e-5):
    """csrc/ss2d_out.hip ln_fwd / ln_bwd (and their narrow forms): out = LayerNorm(x; gamma, beta) over the last axis, and dx, dgamma, dbeta
    for the cotangent gout.

    x, gout [N, D] in the activation dtype (fp32 or bf16), gamma, beta fp32.  No intermediate rounding: out and dx are stored in x's
    dtype (a = 1 for bf16, 0 for fp32), dgamma and dbeta in fp32 (a = 0).  Magnitudes as in ln_gate() with the SiLU factor 1: xhat is
    |xhat| + rstd mean|x| (the fp32 mean is subtracted before the scaling, so its error is absolute).
    Returns {name: (value, magnitude)} for out, dx, dgamma, dbeta."""
    import torch.nn.functional as F
    N, D = x.shape
    xr, gr, br = _d(x).requires_grad_(), _d(gamma).requires_grad_(), _d(beta).requires_grad_()
    out = F.layer_norm(xr, (D,), gr, br, eps)
    gd = _d(gout)
    (out * gd).sum().backward()
    with torch.no_grad():
        xd = xr.detach()
        mu = xd.mean(-1, keepdim=True)
        rstd = (((xd - mu) ** 2).mean(-1, keepdim=True) + eps).rsqrt()
        X = ((xd - mu) * rstd).abs() + rstd * xd.abs().mean(-1, keepdim=True)
        m_out = gr.detach().abs() * X + br.detach().abs()
        gxh = gd.abs() * gr.detach().abs()
        m_dx = rstd * (gxh + gxh.mean(-1, keepdim=True) + X * (gxh * X).mean(-1, keepdim=True))
        m_dg = (gd.abs() * X).sum(0)
        m_db = gd.abs().sum(0)
    return {'out': (out.detach(), m_out), 'dx': (xr.grad, m_dx), 'dgamma': (gr.grad, m_dg), 'dbeta': (br.grad, m_db)}


# Roundings of xhat = (x - mean) rstd as every LayerNorm kernel of csrc/ss2d_out.hip forms it (the wave-per-token kernels at D = 1024 are
# the longest; the narrow kernels sum 8 + log2(D / 8) terms).  D is a power of two, so the products by 1 / D are exact.
#   mean: a lane's first float4 as (a + b) + (c + d) (2), its three other pieces added on (3), the 64-lane butterfly (6)           = 11
#   x - mean                                                                                                                    =  1
#   var = sum c^2 / D + eps: c's rounding counts twice (2), 16 FMAs, the butterfly (6), + eps (1) = 25; the rsqrt halves it        = 13
#   (a shift of the mean moves var only in second order: sum c = 0); rsqrtf (2); * rstd (1)                                       =  3
LN_XHAT_N = 28
LN_OUT_N = LN_XHAT_N + 1                 # the FMA with gamma and beta
# dx = rstd (gxh - c1 - xhat c2), gxh = g gamma (1): c2 = sum gxh xhat / D is 16 FMAs, the butterfly (6), * (1 / D) (1) on summands that
# carry gxh (1) and xhat; then xhat c2 (xhat again, 1), the two subtractions (2), * rstd (rstd's 14 + 2 are inside LN_XHAT_N; 1)
LN_DX_N = 2 * LN_XHAT_N + 23 + 1 + 1 + 2 + 1
LN_TOK_PER_BLOCK = 64                    # LG_WAVES * LG_TOK_BWD: the tokens of one backward workgroup (one row of the partial sums)


def layer_norm_bounds(ntok, bf16):
    """{name: (a, b)} for layer_norm's outputs.  dgamma: xhat, then 16 tokens per wave as FMAs in registers (16), 4 waves through LDS (4),
    the ordered slab_sum over ceil(ntok / 64) blocks; dbeta: the same chain of plain sums, without xhat."""
    a = 1 if bf16 else 0
    nblk = (ntok + LN_TOK_PER_BLOCK - 1) // LN_TOK_PER_BLOCK
    return {'out': (a, fp32_b(LN_OUT_N)), 'dx': (a, fp32_b(LN_DX_N)),
            'dgamma': (0, fp32_b(LN_XHAT_N + 16 + 4 + nblk)), 'dbeta': (0, fp32_b(16 + 4 + nblk))}


def ln_gate_f32_bounds(ntok):
    """{name: (a, b)} for ln_gate() where xz, out and gout are fp32 (ln_gate_fwd / bwd_kernel<float>): the figures
    tests/test_gpu_bf16_kernels.py uses for the bf16 form, with a = 0 everywhere."""
    nblk = (ntok + LN_TOK_PER_BLOCK - 1) // LN_TOK_PER_BLOCK
    return {'out': (0, fp32_b(48)), 'dx': (0, fp32_b(48)), 'dz': (0, fp32_b(48)), 'dgamma': (0, fp32_b(nblk + 80)), 'dbeta': (0, fp32_b(nblk + 80))}


# ------------------------------------------------------------------------------------------------ cross-merge (csrc/ss2d_out.hip)
def cross_merge(y4, H, W):
    """cross_merge_fwd*: y4 [B, 4, D, L] (directions 0, 2 row-major, 1, 3 column-major flattenings of an H x W map) -> [B, L, D] =
    y0 + y2 + T(y1 + y3), T the transposition of the column-major planes into row-major order.  Magnitude sum |y_k|.  The kernels add
    (y0 + y2) + (y1 + y3): three fp32 roundings, the output is fp32 (a = 0, b = fp32_b(3))."""
    y = _d(y4)
    B, _, D, L = y.shape

    def T(t):
        return t.view(B, D, W, H).transpose(2, 3).reshape(B, D, L)
    val = y[:, 0] + y[:, 2] + T(y[:, 1] + y[:, 3])
    mag = y[:, 0].abs() + y[:, 2].abs() + T(y[:, 1].abs() + y[:, 3].abs())
    return val.transpose(1, 2).contiguous(), mag.transpose(1, 2).contiguous()


def cross_merge_adjoint(g, H, W):
    """cross_merge_bwd*: g [B, L, D] -> [B, 2, D, L]: plane 0 the row-major map, plane 1 the column-major map.  Pure data movement: no
    magnitude; fp32 planes equal it, bf16 planes equal it rounded to nearest-even.  Keeps g's dtype."""
    B, L, D = g.shape
    gm = g.detach().cpu().transpose(1, 2)
    return torch.stack([gm.contiguous(), gm.reshape(B, D, H, W).transpose(2, 3).reshape(B, D, L)], 1)


# ------------------------------------------------------------------------------------------------ depthwise front end (csrc/dwconv.hip)
def dwconv_silu_cross(xz, D, weight, bias, gout2):
    """csrc/dwconv.hip: u2 [B, 2, D, L] = SiLU(conv3x3_depthwise(xi) + bias) in the row-major (plane 0) and column-major (plane 1)
    flattening, xi = the first D channels of each pixel's row of xz [B, H, W, >= D]; and d(xi) [B, H, W, D], d(weight) [D, 9],
    d(bias) [D] for the cotangent pair gout2 [B, 2, D, L] (None: forward only).

    xz and gout2 as the kernel reads them (fp32 or bf16), weight [D, 9] (or [D, 1, 3, 3]) and bias [D] (or None) fp32.  Zero padding.  A
    non-finite input gives what conv2d + SiLU give (the forward value is computed with torch's own conv2d).  No intermediate rounding.
    Magnitudes: the conv z is sum |w| |x| + |bias| (m_z); SiLU(z) = z sigmoid(z) is m_z sig_mag(s, m_z); the backward's SiLU'(z) is
    sig_mag(s, m_z) (1 + |z| (1 - s)) (SiLU' has a zero near z = -1.28; this form has none); the gradients are the same computation on
    absolute values.  Returns {name: (value, magnitude)} for out, dx, dw, db, and 'zmax' (the largest finite |z|: the range of __expf)."""
    import torch.nn.functional as F
    B, H, W = xz.shape[:3]
    L = H * W
    xi = _d(xz)[..., :D].permute(0, 3, 1, 2).contiguous()
    w = _d(weight).reshape(D, 1, 3, 3)
    bi = _d(bias) if bias is not None else torch.zeros(D, dtype=torch.float64)

    def conv(t, k, b_):
        return F.conv2d(t, k, b_, padding=1, groups=D)

    def both(t):                                                   # [B, D, H, W] -> [B, 2, D, L]
        return torch.stack([t.flatten(2), t.transpose(2, 3).flatten(2)], 1)
    z = conv(xi, w, bi)
    fin = torch.isfinite(z)
    m_z = conv(torch.nan_to_num(xi, nan=0.0, posinf=0.0, neginf=0.0).abs(), w.abs(), bi.abs())
    s = torch.sigmoid(z)
    m_s = sig_mag(s, m_z)
    res = {'out': (both(z * s), both(m_z * m_s)), 'zmax': float(z[fin].abs().max()) if bool(fin.any()) else 0.0}
    if gout2 is None:
        return res
    g2 = _d(gout2)
    g = g2[:, 0].view(B, D, H, W) + g2[:, 1].view(B, D, W, H).transpose(2, 3)
    m_g = g2[:, 0].view(B, D, H, W).abs() + g2[:, 1].view(B, D, W, H).transpose(2, 3).abs()
    gz = g * s * (1 + z * (1 - s))
    m_gz = m_g * m_s * (1 + z.abs() * (1 - s))
    flip = w.flip(2, 3)                                            # d(input) = the transposed 3 x 3 of d(conv)
    dx, m_dx = conv(gz, flip, None), conv(m_gz, flip.abs(), None)
    xp, axp = F.pad(xi, (1, 1, 1, 1)), F.pad(xi.abs(), (1, 1, 1, 1))
    dw, m_dw = torch.zeros(D, 9, dtype=torch.float64), torch.zeros(D, 9, dtype=torch.float64)
    for ky in range(3):
        for kx in range(3):
            dw[:, ky * 3 + kx] = (gz * xp[:, :, ky:ky + H, kx:kx + W]).sum((0, 2, 3))
            m_dw[:, ky * 3 + kx] = (m_gz * axp[:, :, ky:ky + H, kx:kx + W]).sum((0, 2, 3))
    res.update({'dx': (dx.permute(0, 2, 3, 1).contiguous(), m_dx.permute(0, 2, 3, 1).contiguous()), 'dw': (dw, m_dw),
                'db': (gz.sum((0, 2, 3)), m_gz.sum((0, 2, 3)))})
    return res


DW_TILE = 16          # csrc/dwconv.hip TS: a workgroup owns a 16 x 16 pixel tile; one row of the d(weight) / d(bias) partials per (image, tile)


def dwconv_tiles(H, W):
    return ((H + DW_TILE - 1) // DW_TILE) * ((W + DW_TILE - 1) // DW_TILE)


def dwconv_bounds(zmax, B, H, W, bf16_act, bf16_planes):
    """{name: (a, b)} for dwconv_silu_cross's outputs; every figure is a count of fp32 roundings along the kernel's chain.
    z: nine FMAs onto the bias (9).  s = 1 / (1 + __expf(-z)): 1 + e and the division (2) and one __expf.  out = z / (1 + e): z's and
    s's chains and one spare for the product form (12 and one __expf); stored in the plane's dtype.
    d(conv) gz = (g0 + g1) s (1 + z (1 - s)): the plane sum (1), z (9), s (2 and __expf), 1 - s, z (.), 1 + (.), s (.), g (.) (5); the
    factor z (1 - s) carries s's absolute error |z| times, so s's chain counts 1 + zmax times.
    dx: nine FMAs over gz (9); stored in the activation dtype.  dw, db: an FMA per pixel (1), up to 21 of the 18 x 18 halo pixels per thread
    in sequence (21), the 16-lane group sum (4), the ordered slab_sum over B * tiles partial rows."""
    e = expf_b(zmax)
    b_s = fp32_b(2) + e
    b_gz = fp32_b(1 + 9 + 5) + (1 + math.ceil(zmax)) * b_s
    b_sum = fp32_b(1 + 21 + 4 + B * dwconv_tiles(H, W))
    return {'out': (1 if bf16_planes else 0, fp32_b(9 + 1) + b_s), 'dx': (1 if bf16_act else 0, b_gz + fp32_b(9)),
            'dw': (0, b_gz + b_sum), 'db': (0, b_gz + b_sum)}


# ------------------------------------------------------------------------------------------------ MFMA linear (csrc/gemm_bf16.hip)
def linear(x, w, bias, gy=None):
    """csrc/gemm_bf16.hip tamtr_linear_bf16 and the backward of ops.linear_bf16: y = x w^T + bias, and dx = gy w, dw = gy^T x, db = the
    column sums of gy for the cotangent gy (None: forward only).

    Operands as the kernel reads them: x bf16 [M, K], w bf16 [N, K], bias fp32 [N] or None, gy bf16 [M, N].  Rounding points: none on
    purpose except the W-stationary kernel's bias split (linear_bounds).  Magnitudes: the same products on absolute values; y's includes
    |bias|.  A NaN in a row of x makes the row of y NaN (every product of the row's sum is NaN or the sum holds one).
    Returns {name: (value, magnitude)} for y, dx, dw, db, and 'bias': |bias| broadcast to y's shape (the term that carries the
    W-stationary kernel's split residual)."""
    X, W = _d(x), _d(w)
    M, N = X.shape[0], W.shape[0]
    b = _d(bias) if bias is not None else torch.zeros(N, dtype=torch.float64)
    aX, aW = X.abs(), W.abs()
    res = {'y': (X @ W.t() + b, aX @ aW.t() + b.abs()), 'bias': b.abs().expand(M, N)}
    if gy is not None:
        G = _d(gy)
        aG = G.abs()
        res.update({'dx': (G @ W, aG @ aW), 'dw': (G.t() @ X, aG.t() @ aX), 'db': (G.sum(0), aG.sum(0))})
    return res


BIAS_SPLIT = 2.0 ** -16   # see linear_bounds: what bf16(b) + bf16(b - bf16(b)) loses of an fp32 b, relative to |b|


def linear_bounds(kernel, M, N, K):
    """(a, b, c) of y for one of tamtr_linear_bf16's kernels ('wstat' | 'n512_k64' | 'tile'): |y - ref| <= a 2^-8 |ref| + b mag + c |bias|.

    Every kernel forms K products of two bf16 values - each exact in fp32: 8 + 8 significant bits - and adds them into an fp32
    accumulator with v_mfma_f32_32x32x16_bf16, 16 products per instruction.  Whether the instruction rounds each of its internal adds or
    fewer is not documented where this project can read it; the count takes the worst case, one fp32 rounding per added product, whatever
    the order: K roundings, each relative to a partial sum that the magnitude bounds.  y is stored in bf16: a = 1.
      tile      the bias is added to the finished accumulator in fp32: K + 1.
      n512_k64  the accumulator starts at the bias, which is then one more summand of the same chain: K.
      wstat     the bias enters by one more MFMA as hi + lo, hi = bf16(b), lo = bf16(b - hi), against two ones: two more products in the
                chain (the instruction's other 14 are exact zeros): K + 2.  The split itself: |b - hi| <= 2^-8 |b| (round to nearest, 8
                significant bits), b - hi is exact in fp32 (it is the part of b's significand below hi's last bit), and
                |(b - hi) - lo| <= 2^-8 |b - hi| <= 2^-16 |b|.  That residual is relative to |bias| alone, not to the products: c = 2^-16.
    dx on the same kernels (N and K exchanged, no bias) takes the same figures."""
    n = {'tile': K + 1, 'n512_k64': K, 'wstat': K + 2}[kernel]
    return 1, fp32_b(n), (BIAS_SPLIT if kernel == 'wstat' else 0.0)


def linear_check(what, got, ref, kernel, K):
    """y (or dx: bias None) of one MFMA kernel against linear()'s result: check() on the combined tensor b mag + c |bias| with b = 1."""
    a, b, c = linear_bounds(kernel, got.shape[0], got.shape[1], K)
    return check(what, got, ref['y'][0], b * ref['y'][1] + c * ref['bias'], a, 1.0)


def slab_sum_chain(R, C):
    """The longest chain of fp32 additions behind one output of csrc/fold.hip tamtr_slab_sum_rows over R rows of C columns.  R <= 32: a
    thread adds its R rows in sequence.  Else 1024 threads = CG column groups x RG row groups (CG = 64, halved while CG / 2 still covers
    the C / 4 column quads): a thread adds its ceil(R / RG) rows, then the row groups that hold any are added in index order."""
    if R <= 32:
        return R
    CG = 64
    while CG > 1 and CG // 2 >= C // 4:
        CG //= 2
    RG = 1024 // CG
    return -(-R // RG) + min(RG, R)


def colsum_chain(M, N, streams):
    """The chain behind one element of ops.colsum of a bf16 [M, N] matrix.  Direct (streams False): slab_sum over the M rows.  Streaming
    (csrc/fold.hip colsum_bf16_kernel): min(ceil(M / 64), 2048) workgroups of ceil(M / workgroups) rows each; 256 / (N / 8) row lanes per
    column group, a lane adds its ceil(rows / lanes) rows in sequence, the lanes are added in order, slab_sum adds the workgroups' rows."""
    if not streams:
        return slab_sum_chain(M, N)
    nblk = min((M + 63) // 64, 2048)
    rows = -(-M // nblk)
    lanes = 256 // (N // 8)
    return -(-rows // lanes) + lanes + slab_sum_chain(nblk, N)


def linear_grad_bounds(M, N, K, S, bmm_f32_out=True, streams=False):
    """{name: (a, b)} for what ops.linear_bf16's backward leaves to the library and to the ordered sums.
    dx (library GEMM, where the MFMA kernel does not take the shape): N products in fp32, stored in bf16: (1, N).
    db: exact bf16 values added in fp32 along the chain that the kernels form, counted in colsum_chain (41 at 8193 x 256 streaming, 79 at
    1000 x 512 direct): (0, chain).  At these counts one dropped row of gy (an element of about 1 against a magnitude of M) misses the bound.
    dw, S = 1 slice: one library GEMM with a bf16 result, widened afterwards: (1, M).  S > 1: S batched library products of M / S rows with
    fp32 results, added in order by slab_sum over S rows of N K columns: (0, M / S + slab_sum_chain(S, N K)); where the build's bmm has no
    fp32 output the partials are bf16 and each carries 2^-8 of its magnitude.  The order inside the library's product is not this
    project's to read, so its M / S products count as M / S roundings, the bound of any order; with the worst-case magnitude that is too
    wide to see ONE dropped row of dw at M / S = 2050 (it sees a dropped slice: tests/test_ref64_host.py) - single rows of dw are held
    by the S = 1 cases (a = 1 on |ref|) and by test_linear_bf16_kernel."""
    dw = (1, fp32_b(M)) if S == 1 else (0, fp32_b(M // S + slab_sum_chain(S, N * K)) + (0 if bmm_f32_out else U8))
    return {'dx': (1, fp32_b(N)), 'db': (0, fp32_b(colsum_chain(M, N, streams))), 'dw': dw}


# ------------------------------------------------------------------------------------------------ x_proj of SS2D (csrc/xproj.hip)
XP_N = 16            # d_state
XP_SLICE = 1024      # pixels per partial tile of the weight gradient


def xproj_wcat(wx):
    """x_proj_weight [4, C, D] -> [2, 2C, D] fp64: the rows [W_i ; W_(i+2)] of stored copy i, rounded to bf16 as ops.xproj_pack_weight does."""
    w = wx.detach().cpu()
    return torch.stack([torch.cat([w[0], w[2]], 0), torch.cat([w[1], w[3]], 0)]).bfloat16().double()


def xproj_rows(dtr, Bs, Cs):
    """[B, 4, R | 16 | 16, L] x 3 -> [B, 2, 2C, L]: copy i's rows [dtr_i ; B_i ; C_i ; dtr_(i+2) ; B_(i+2) ; C_(i+2)] (xp_row's order)."""
    return torch.stack([torch.cat([dtr[:, i], Bs[:, i], Cs[:, i], dtr[:, i + 2], Bs[:, i + 2], Cs[:, i + 2]], 1) for i in range(2)], 1)


def xproj(u2, wx, R, gdtr, gB, gC, gu, plane_bf16=None):
    """csrc/xproj.hip: per image and stored copy i, OUT_i [2C, L] = Wcat_i [2C, D] U_i [D, L] split into dtr / Bs / Cs of directions i and
    i + 2; d/d(u2)[b, i] = gu[b, i] + gu[b, i + 2] + Wcat_i^T G_i; dWcat_i = sum over images and pixels of G_i U_i^T.

    u2 [B, 2, D, L] and gu [B, 4, D, L] in the plane dtype (fp32 or bf16), wx fp32 [4, C, D], gdtr [B, 4, R, L], gB, gC [B, 4, 16, L] fp32.
    Rounding points, from the source, each applied here exactly (round to nearest even, what v_cvt_pk_bf16_f32 does), so that they cost
    no term of the bound: W is bf16 (the packed weight); u is rounded to bf16 in registers (exact for bf16 planes); G is rounded to bf16
    in registers.  What remains:
      forward   D exact products in an fp32 chain, the result rounded to bf16 and stored as fp32: a = 1, b = fp32_b(D + 1); every stored
                value is a bf16 value.
      d/d(u2)   2C products in an fp32 chain (fp32_b(2C) on the product's magnitude m), the product p rounded to bf16 (2^-8 of the fp32
                product, which is within fp32_b(2C) m of |p|: 2^-8 |p| and one more count on m), then gu_i + gu_(i+2) + p in fp32: two
                roundings on |gu_i| + |gu_(i+2)| + m.  The returned magnitude is that whole sum,
                2^-8 |p| + fp32_b(2C + 1) m + fp32_b(2) (|gu_i| + |gu_(i+2)| + m), to be used with b = 1; bf16 planes round the sum once
                more: a = 1, fp32 planes a = 0.
      dWcat     fp32 partial tiles per (image, 1 024-pixel slice): min(L, 1024) products in a chain; the ordered slab_sum over
                B * ceil(L / 1024) rows: a = 0, b = fp32_b(min(L, 1024) + B * slices), as dwconv_bounds counts its partials.
    Returns {name: (value, magnitude)} for dtr, Bs, Cs ([B, 4, R | 16 | 16, L]), gu2 [B, 2, D, L], dw [2, 2C, D]."""
    assert plane_bf16 is None or (u2.dtype == gu.dtype == (torch.bfloat16 if plane_bf16 else torch.float32)), 'u2 and gu are in the plane dtype'
    B, _, D, L = u2.shape
    C = R + 2 * XP_N
    Wc = xproj_wcat(wx)                                             # [2, 2C, D]
    U = u2.detach().cpu().bfloat16().double()                       # the register rounding (exact for bf16 planes)
    out, m_out = torch.einsum('imd,bidl->biml', Wc, U), torch.einsum('imd,bidl->biml', Wc.abs(), U.abs())

    def split(t):                                                   # [B, 2, 2C, L] -> dtr, Bs, Cs
        h = t.view(B, 2, 2, C, L)                                   # [b, i, half (direction i | i + 2), c, l]
        d4 = h.permute(0, 2, 1, 3, 4).reshape(B, 4, C, L)           # direction = 2 half + i
        return d4[:, :, :R], d4[:, :, R:R + XP_N], d4[:, :, R + XP_N:]
    res = {n: (v.contiguous(), m.contiguous()) for n, v, m in zip(('dtr', 'Bs', 'Cs'), split(out), split(m_out))}
    G = xproj_rows(gdtr.detach().cpu(), gB.detach().cpu(), gC.detach().cpu()).bfloat16().double()      # [B, 2, 2C, L]
    g = _d(gu)
    prod, m_prod = torch.einsum('imd,biml->bidl', Wc, G), torch.einsum('imd,biml->bidl', Wc.abs(), G.abs())
    val = g[:, :2] + g[:, 2:] + prod
    m_sum = g[:, :2].abs() + g[:, 2:].abs() + m_prod
    res['gu2'] = (val, U8 * prod.abs() + fp32_b(2 * C + 1) * m_prod + fp32_b(2) * m_sum)
    res['prod'] = prod
    res['dw'] = (torch.einsum('biml,bidl->imd', G, U), torch.einsum('biml,bidl->imd', G.abs(), U.abs()))
    return res


def xproj_slices(L):
    return (L + XP_SLICE - 1) // XP_SLICE


def xproj_bounds(B, D, L, plane_bf16):
    """{name: (a, b)} for xproj()'s outputs; the counts are written out in xproj()'s docstring."""
    fwd = (1, fp32_b(D + 1))
    return {'dtr': fwd, 'Bs': fwd, 'Cs': fwd, 'gu2': (1 if plane_bf16 else 0, 1.0), 'dw': (0, fp32_b(min(L, XP_SLICE) + B * xproj_slices(L)))}


# ------------------------------------------------------------------------------------------------ BatchNorm (csrc/bn.hip)
def _rows(t):
    """[N, C] as it is, an NCHW map given as [B, C, HW] permuted to [B * HW, C]; fp64."""
    t = _d(t)
    return t if t.dim() == 2 else t.permute(0, 2, 1).reshape(-1, t.shape[1])


def _bn_parts(x, chunk_rows, parts):
    """The rows of each partial triple, as a partial index per row: an NCHW map [B, C, HW]: image by image, slices of BN_SLICE pixels;
    channels-last rows with chunk_rows: chunks of that many rows; parts: a list of row counts (hand-made partials); else one partial."""
    if x.dim() == 3:
        B, _, HW = x.shape
        sh = -(-HW // BN_SLICE)
        return (torch.arange(B).view(B, 1) * sh + torch.arange(HW).view(1, HW) // BN_SLICE).reshape(-1)
    if chunk_rows is not None:
        return torch.arange(x.shape[0]) // chunk_rows
    if parts is not None:
        return torch.repeat_interleave(torch.arange(len(parts)), torch.tensor(parts))
    return torch.zeros(x.shape[0], dtype=torch.long)


def _bn_stats(x, eps, pid, shifted):
    """Batch statistics of the rows x [N, C] (fp64) and their magnitudes; pid: the partial (slice | chunk) of each row.  A channel that
    holds a NaN or an Inf has NaN statistics: the kernels' Chan combine forms inf - inf, or inf * 0 against an empty lane, for it
    (nn.BatchNorm2d would report a mean of inf; check() could not hold an inf anyway).

    Magnitudes.  mean: the NCHW kernels sum x itself, M = mean|x|.  The channels-last kernels (shifted) sum d = x - k, k the first row of
    the row's chunk, and add k back: M = mean(|k| + |d|).  var: a sum of squares, relative to itself, where the squares are those the
    kernel forms: (x - slice mean)^2 and the Chan terms for NCHW (they add up to N var), d^2 for channels-last, whose
    M2 = s2 - s1 s1 / n inherits the roundings of s2 = sum d^2 (spread = mean d^2 >= var).  Besides, a Chan combine adds
    n_A n_B / (n_A + n_B) (mean_B - mean_A)^2 from rounded means: an error e in either moves it by at most 2 e times
    sum over the partials s of A and B of n_s |mean_s - mean|, in first order; over one level of combines that is 2 e N D, D the weighted
    mean of |mean_s - mean| (0 for one partial): m_var = spread + 2 D M, and bn_stat_counts() counts the levels.  rstd = (var + eps)^-1/2
    moves by rstd / 2 per relative change of var + eps: m_rstd = rstd (1 + rho), rho = m_var / (2 (var + eps)).  xhat = (x - mean) rstd:
    X = |xhat| (1 + rho) + rstd M, as layer_norm() has it with rho = 0 (its variance is one exact two-pass)."""
    N = x.shape[0]
    bad = ~torch.isfinite(x).all(0)
    nan = torch.full_like(x[0], float('nan'))
    mean = torch.where(bad, nan, x.mean(0))
    var = ((x - mean) ** 2).mean(0)
    S = int(pid.max()) + 1
    n_s = torch.bincount(pid, minlength=S).double().view(S, 1)
    mean_s = torch.zeros(S, x.shape[1], dtype=torch.float64).index_add_(0, pid, x) / n_s
    D = (n_s * (mean_s - mean).abs()).sum(0) / N
    if shifted:
        first = torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(n_s.view(-1).long(), 0)[:-1]])
        k = x[first[pid]]
        M, spread = (k.abs() + (x - k).abs()).mean(0), ((x - k) ** 2).mean(0)
    else:
        M, spread = x.abs().mean(0), var
    m_var = spread + 2 * D * M
    rstd = (var + eps).rsqrt()
    rho = m_var / (2 * (var + eps))
    xh = (x - mean) * rstd
    return {'mean': mean, 'var': var, 'rstd': rstd, 'M': M, 'm_var': m_var, 'rho': rho, 'xh': xh, 'X': xh.abs() * (1 + rho) + rstd * M}


def _bn_act(z, m_z, act):
    """act(z), its magnitude, act'(z), its magnitude (identity: act' is an exact 1).  SiLU as dwconv_silu_cross() has it, with the
    derivative's magnitude sig_mag(s, m_z) (1 + |z|): s' = s (1 + z (1 - s)) carries s's error 1 + |z| times and z's twice."""
    if not act:
        one = torch.ones_like(z)
        return z, m_z, one, one
    s = torch.sigmoid(z)
    m_s = sig_mag(s, m_z)
    return z * s, m_z * m_s, s * (1 + z * (1 - s)), m_s * (1 + z.abs())


def _bn_running(st, N, momentum, rm, rv):
    unb = N / (N - 1) if N > 1 else 1.0           # one value per channel: the biased variance (bn_finalize_kernel, n > 1.f ?)
    rm, rv = _d(rm), _d(rv)
    return {'running_mean': ((1 - momentum) * rm + momentum * st['mean'], (1 - momentum) * rm.abs() + momentum * st['M']),
            'running_var': ((1 - momentum) * rv + momentum * st['var'] * unb, (1 - momentum) * rv.abs() + momentum * st['m_var'] * unb)}


def _bn_core(xs, gammas, betas, gout, eps, momentum, rms, rvs, act, residual, chunk_rows, parts=None):
    """act(sum_i bn_i(x_i)) [+ residual] and its backward for one or two BatchNorms over the same [N, C] shape."""
    pid = _bn_parts(xs[0], chunk_rows, parts)
    xs = [_rows(x) for x in xs]
    N = xs[0].shape[0]
    g = _rows(gout)
    sts = [_bn_stats(x, eps, pid, chunk_rows is not None) for x in xs]
    ga, be = [_d(t) for t in gammas], [_d(t) for t in betas]
    z = sum(a * st['xh'] for a, st in zip(ga, sts)) + sum(be)
    m_z = sum(a.abs() * st['X'] for a, st in zip(ga, sts)) + sum(b.abs() for b in be)
    y, m_y, d, m_d = _bn_act(z, m_z, act)
    fin = torch.isfinite(z)
    res = {'zmax': float(z[fin].abs().max()) if bool(fin.any()) else 0.0}
    if residual is not None:
        r = _rows(residual)
        y, m_y = y + r, m_y + r.abs()
        res['dres'] = (g, g.abs())
    res['out'] = (y, m_y)
    dz, m_dz = g * d, g.abs() * m_d
    db, m_db = dz.sum(0), m_dz.sum(0)
    for i, (a, st) in enumerate(zip(ga, sts)):
        s = '' if len(xs) == 1 else str(i + 1)
        dg, m_dg = (dz * st['xh']).sum(0), (m_dz * st['X']).sum(0)
        res['dgamma' + s], res['dbeta' + s] = (dg, m_dg), (db, m_db)
        res['dx' + s] = (a * st['rstd'] * (dz - db / N - st['xh'] * dg / N),
                         a.abs() * st['rstd'] * (1 + st['rho']) * (m_dz + m_db / N + st['X'] * m_dg / N))
        res['mean' + s], res['rstd' + s] = (st['mean'], st['M']), (st['rstd'], st['rstd'] * (1 + st['rho']))
        if rms[i] is not None:
            for n, v in _bn_running(st, N, momentum, rms[i], rvs[i]).items():
                res[n + s] = v
    return res


def batch_norm(x, gamma, beta, gout, eps, momentum, running_mean, running_var, act, residual=None, chunk_rows=None, parts=None):
    """csrc/bn.hip: out = act(BatchNorm(x; gamma, beta)) [+ residual] with batch statistics (nn.BatchNorm2d in training mode), act =
    identity (0) | SiLU (1), the running statistics after the call, and dx, dgamma, dbeta [, dres] for the cotangent gout.

    x, gout [, residual] [N, C], or an NCHW map as [B, C, HW] (results come back as [N, C] rows, image-major); operands as the kernel
    reads them.  rstd from the biased variance, the running variance from the unbiased one (the biased one where a channel has one
    value).  running_mean = None: no running statistics.  chunk_rows: the rows of one workgroup's chunk of the channels-last kernels
    (bn_cases.cl_plan); it changes no value, only the magnitudes of the statistics (_bn_stats).  No intermediate rounding: out and dx
    are stored in x's dtype, everything else in fp32; the residual is added in fp32 before the one rounding.
    Returns {name: (value, magnitude)} for out, dx, dgamma, dbeta, mean, rstd, running_mean,
    running_var, dres, and 'zmax' (the largest finite |gamma xhat + beta|: the range of __expf)."""
    return _bn_core([x], [gamma], [beta], gout, eps, momentum, [running_mean], [running_var], act, residual, chunk_rows, parts)


def batch_norm_pair(x1, x2, gamma1, beta1, gamma2, beta2, gout, eps, momentum, running_mean1, running_var1, running_mean2, running_var2, act,
                    chunk_rows=None):
    """csrc/bn.hip tamtr_bncl2_act_*: out = act(bn1(x1) + bn2(x2)), both in training mode over the same [N, C] shape.  As batch_norm();
    the names carry the BatchNorm's number: dx1, dx2, dgamma1, ..., running_var2 (dbeta1 == dbeta2)."""
    return _bn_core([x1, x2], [gamma1, gamma2], [beta1, beta2], gout, eps, momentum, [running_mean1, running_mean2], [running_var1, running_var2],
                    act, None, chunk_rows)


BN_SLICE = 4096       # csrc/bn.hip BN_SLICE: the elements of one (image, channel) plane that one workgroup of the NCHW kernels holds


def bn_combine_steps(S):
    """Chan combines behind one channel in combine_slices: a thread's strided loop over ceil(S / 256) triples, the 64-lane butterfly (6),
    the 4 waves in order (4).  A combine with an empty triple changes nothing, so this is an upper bound at small S."""
    return -(-S // 256) + 6 + 4


def bn_stat_counts(layout, plan):
    """(roundings behind the batch mean, roundings behind var + eps) for a plan of tests/bn_cases.py, counted from csrc/bn.hip.

    One Chan combine: d = mb - mean (1), nb / nt (1), d * (.) (1), mean += (1): 4 on the mean; n * nb (1), / nt (1), d * d (1, and d's
    own rounding twice: 2), * (1), + m2b (1), m2 += (1): 8 on M2, less the one that d shares with the mean's count: 7.
    NCHW (bn_stats_kernel, exact two-pass inside a slice): mean_s = 16 elements per thread in sequence (16), butterfly (6), 4 waves
    (4), / n (1) = 27; M2_s = d = v - mean_s counts twice in d^2 (2), 16 FMAs (16), butterfly (6), waves (4) = 28.
    Channels-last (bncl_stats_kernel, sums of d = x - k and d^2): d (1), iters additions per thread, 256 / cg in fold_row_lanes, s1 / n
    (1), k + m (1): iters + 256 / cg + 3 on the mean; s2 the same chain with d twice and without the last two: iters + 256 / cg + 2;
    M2 = s2 - s1 m: the product and the difference (2), and s1 m carries s1's chain twice (s1 and m = s1 / n; (sum |d|)^2 / n <= sum d^2):
    3 (iters + 256 / cg) + 8.
    var + eps: M2's count, / n (1).  The first-order term of _bn_stats (2 D M) carries the mean's count twice (d = mb - mean has the errors
    of both) once per level of combines that a partial can pass: min(S - 1, bn_combine_steps(S)).  The two terms of m_var are separate,
    so the larger count holds for both."""
    if layout == 'nchw':
        S = plan[2]
        c_mean, c_m2 = 27, 28
    else:
        V, cg, iters, _, S = plan
        c_mean, c_m2 = iters + 256 // cg + 3, 3 * (iters + 256 // cg) + 8
    T = bn_combine_steps(S)
    n_mean = c_mean + 4 * T
    return n_mean, max(c_m2 + 7 * T + 1, 2 * n_mean * min(S - 1, T))


def bn_sum_chain(layout, plan):
    """Additions behind one backward sum (sum dz, sum dz xhat): NCHW: 16 FMAs per thread, block_sum (6 + 4) per slice, then every apply
    workgroup's strided loop over ceil(S / 256) partials and block_sum (10).  Channels-last: iters per thread, 256 / cg in fold_row_lanes,
    then bncl_sum_kernel: ceil(S / 256) and block_sum (10)."""
    if layout == 'nchw':
        return 16 + 10 + -(-plan[2] // 256) + 10
    V, cg, iters, _, S = plan
    return iters + 256 // cg + -(-S // 256) + 10


def bn_bounds(layout, plan, bf16, act, zmax=None, residual=False):
    """{name: (a, b)} for batch_norm()'s outputs (layout 'nchw' | 'cl') and batch_norm_pair()'s ('cl2'); plan = bn_cases.nchw_plan() or
    cl_plan().  zmax: ref['zmax'], needed for SiLU.  Every figure is a count of fp32 roundings along the kernel's chain:
      mean          bn_stat_counts()[0]; running_mean: 1 - momentum, two products, the sum (4) more
      rstd          n_var = bn_stat_counts()[1], then eps as an fp32 constant (1), + eps (1), rsqrtf (2): n_var + 4
      running_var   n_var, n - 1 is exact, / (1), 1 - momentum, two products, the sum (4): n_var + 5
      xhat          rstd (n_var + 4), x - mean (1; the mean's count is below n_var and multiplies a separate term of X), * rstd (1): n_var + 6
      z             a = rstd gamma (1), the FMA (1): n_var + 8; the backward forms (x - mean) rstd, then the FMA with gamma and beta: the same;
                    the pair adds beta1 + beta2 (1) and the second FMA (1)
      out           identity: z.  SiLU: z, 1 + e, the division, the product form (3) and one __expf.  A residual: the sum (1).
      dz            identity: exact (gout times 1).  SiLU: z twice (_bn_act), s = 1 / (1 + e) (2 and __expf), 1 - s, z (.), 1 + (.), s (.),
                    gout (.) (5)
      dbeta         dz and bn_sum_chain(); dgamma: dz, xhat, the product (1), bn_sum_chain()
      dx            gamma rstd (n_var + 4 and 1), dz, k1 = sum dz / N: 1 / N as an fp32 constant and the product (2) on dbeta's chain, xhat k2:
                    xhat, the product (1), the same 2 on dgamma's chain (which holds dz and xhat again); two differences, the last product (3)
    a = 1 where the kernel stores bf16 (out, dx; a residual is added in fp32 and the sum rounded once); everything else is fp32.  dres is
    gout itself: (0, 0), an exact copy."""
    lay = 'cl' if layout == 'cl2' else layout
    n_mean, n_var = bn_stat_counts(lay, plan)
    chain = bn_sum_chain(lay, plan)
    a = 1 if bf16 else 0
    e = expf_b(zmax) if act else 0.0
    n_xhat = n_var + 6
    n_z = n_var + 8 + (2 if layout == 'cl2' else 0)
    b_out = fp32_b(n_z + (3 if act else 0) + (1 if residual else 0)) + e
    b_dz = fp32_b(2 * n_z + 2 + 5) + e if act else 0.0
    b_db = b_dz + fp32_b(chain)
    b_dg = b_dz + fp32_b(n_xhat + 1 + chain)
    b_dx = fp32_b(n_var + 5) + b_dz + fp32_b(2 + n_xhat + 1) + b_dg + fp32_b(3)
    one = {'out': (a, b_out), 'dx': (a, b_dx), 'dgamma': (0, b_dg), 'dbeta': (0, b_db), 'mean': (0, fp32_b(n_mean)), 'rstd': (0, fp32_b(n_var + 4)),
           'running_mean': (0, fp32_b(n_mean + 4)), 'running_var': (0, fp32_b(n_var + 5)), 'dres': (0, 0.0)}
    if layout != 'cl2':
        return one
    two = {'out': one['out']}
    for n in ('dx', 'dgamma', 'dbeta', 'mean', 'rstd', 'running_mean', 'running_var'):
        two[n + '1'] = two[n + '2'] = one[n]
    return two


# ------------------------------------------------------------------------------------------------ loss terms, matcher cost, box refinement (csrc/detrloss.hip)
def f32(x):
    """A Python number as the fp32 value a `float` parameter of the C ABI (or an `f` literal of the source) holds, as a Python float."""
    return float(torch.tensor(float(x), dtype=torch.float32))


DL_EPS = f32(1e-7)                    # DL_EPS of csrc/detrloss.hip
DL_ONE_EPS = f32(1.0 + 1e-7)          # its 1.f + DL_EPS, formed in fp32: 1 + 2^-23
FOCAL_EPS = f32(1e-8)                 # the matcher's 1e-8f
REF_EPS = f32(1e-5)                   # inverse_sigmoid's eps
FLT_MIN = 2.0 ** -126                 # fp32's smallest normal number: what check()'s `tiny` is a small multiple of


def riou_parts(a, b, eps=DL_EPS, one_eps=DL_ONE_EPS, mut=()):
    """1 - RIOU (ultralytics/utils/metrics.py:91-130) of predictions a against boxes b (xywh, fp64, broadcastable [..., 4]) and its
    gradient by a, written out as plain formulas; csrc/detrloss.hip riou_xywh / riou_loss_grad state the same ones in fp32.

    The rules: the IoU's intersection clamp passes its gradient where its argument is >= 0; a tie of min / max / maximum gives each side
    half; RIOU's alpha is a constant; coincident centres give d sqrt(rho2) = inf * 0 = NaN in all four components.
    Magnitudes: the same formulas on absolute values with the cancelling terms added: the union a + b - inter as a + b + inter (its
    relative conditioning `ku` multiplies everything that divides by it), the aspect term atan(.) - atan(.) as the sum of the two, the
    denominator of alpha as v + iou + 1, and the three contributions of the gradient (d iou, the distance term, alpha dv) as a sum.
    mut: deliberate mistakes for the host tests ('tie0' | 'tie1': a tie's half as 0 | 1; 'cx_gt': the clamp gate of x as > 0; 'dm1_swap').
    Returns a dict: iou, ku, loss, m_loss, l1, grad [..., 4], m_grad [..., 4]."""
    a, b = torch.broadcast_tensors(a, b)
    ax, ay, aw, ah = a.unbind(-1)
    bx, by, bw, bh = b.unbind(-1)
    ax1, ax2, ay1, ay2 = ax - aw / 2, ax + aw / 2, ay - ah / 2, ay + ah / 2
    bx1, bx2, by1, by2 = bx - bw / 2, bx + bw / 2, by - bh / 2, by + bh / 2
    one, z = torch.ones_like(ax), torch.zeros_like(ax)
    half = 0.0 if 'tie0' in mut else 1.0 if 'tie1' in mut else 0.5

    def step(gt, eq):
        return torch.where(gt, one, torch.where(eq, half * one, z))
    ixr, iyr = torch.minimum(ax2, bx2) - torch.maximum(ax1, bx1), torch.minimum(ay2, by2) - torch.maximum(ay1, by1)
    iw, ih = ixr.clamp(min=0), iyr.clamp(min=0)
    cx, cy = ((ixr > 0) if 'cx_gt' in mut else (ixr >= 0)).double(), (iyr >= 0).double()
    d_ax2, d_ax1 = step(ax2 < bx2, ax2 == bx2) * cx, -step(ax1 > bx1, ax1 == bx1) * cx
    d_ay2, d_ay1 = step(ay2 < by2, ay2 == by2) * cy, -step(ay1 > by1, ay1 == by1) * cy
    diw = [d_ax1 + d_ax2, z, 0.5 * (d_ax2 - d_ax1), z]
    dih = [z, d_ay1 + d_ay2, z, 0.5 * (d_ay2 - d_ay1)]
    inter, areas = iw * ih, aw * ah + bw * bh
    uni = areas - inter + eps
    iou, ku = inter / uni, (areas + inter + eps) / uni
    sx, sy = bx1 + bx2 - ax1 - ax2, by1 + by2 - ay1 - ay2
    rho2 = (sx * sx + sy * sy) / 4
    s = rho2.sqrt()
    cs = torch.maximum(aw, ah) + torch.maximum(bw, bh) + s + eps
    c2 = cs * cs
    r1 = aw / ah
    tb, ta = torch.atan(bw / bh), torch.atan(r1)
    da, m_da = tb - ta, tb + ta
    kv = 4 / math.pi ** 2
    v, m_v = kv * da * da, 2 * kv * da.abs() * m_da
    den = v - iou + one_eps
    alpha = v / den
    m_alpha = m_v / den + alpha * (m_v + iou * ku + one_eps) / den
    loss = 1 - (iou - (rho2 / c2 + v * alpha))
    m_loss = 1 + iou * ku + rho2 / c2 + m_v * m_alpha
    drho2 = [-sx, -sy, z, z]
    wide, tall = step(aw > ah, aw == ah), step(ah > aw, aw == ah)
    dm1 = [z, z, tall, wide] if 'dm1_swap' in mut else [z, z, wide, tall]
    inv = 1 / (ah * (1 + r1 * r1))
    dat = [z, z, inv, -r1 * inv]
    dwh = [z, z, ah, aw]
    g, m_g = [], []
    for k in range(4):
        dinter, m_dinter = diw[k] * ih + iw * dih[k], diw[k].abs() * ih + iw * dih[k].abs()
        diou = (dinter * uni - inter * (dwh[k] - dinter)) / (uni * uni)
        m_diou = ku * (m_dinter * uni + inter * (dwh[k] + m_dinter)) / (uni * uni)
        ds = 0.5 / s * drho2[k]                                  # inf * 0 = NaN where the centres coincide
        dcs = dm1[k] + ds
        dterm = (drho2[k] * c2 - rho2 * 2 * cs * dcs) / (c2 * c2)
        m_dterm = (drho2[k].abs() * c2 + rho2 * 2 * cs * (dm1[k] + ds.abs())) / (c2 * c2)
        dv, m_dv = 2 * kv * da * (-dat[k]), 2 * kv * m_da * dat[k].abs()
        g.append(-(diou - dterm - alpha * dv))
        m_g.append(m_diou + m_dterm + m_alpha * m_dv)
    return {'iou': iou, 'ku': ku, 'loss': loss, 'm_loss': m_loss, 'l1': (a - b).abs().sum(-1), 'grad': torch.stack(g, -1), 'm_grad': torch.stack(m_g, -1)}


def detr_terms(pb, ps, gtb, gtc, li, bi, si, gi, n, gains, up, mut=()):
    """csrc/detrloss.hip tamtr_detr_layers_fwd / _bwd (ops.detr_layer_losses): the (class, bbox, giou) terms [Lr] of the stacked decoder
    layers and d/d(pb), d/d(ps) for the upstream gradient up [3, Lr].

    pb [Lr,B,nq,4], ps [Lr,B,nq,nc] fp32; gtb [G,4], gtc [G]; the matched pairs (li, bi, si) <-> gi as flat lists, n per layer,
    layer-major; gains = (class, bbox, giou).  class = gains[0] / max(n, 1) * sum over every logit of BCE(x, t) w with, on the matched
    class of a matched row, t = w = IoU(pred, box) (a constant: detached), elsewhere t = 0 and w = 0.75 sigmoid(x)^2; bbox = gains[1] / n
    * sum |pred - box|; giou = gains[2] / n * sum (1 - RIOU).  Rounding points: none on purpose.
    Magnitudes.  The three terms: the sum of their absolute summands, BCE as |x| (1 + t) + log1p(exp(-|x|)), the IoU with its
    conditioning ku (riou_parts).  (BCE: the kernel adds max(x, 0) - x t, the torch form of tam-tr_amd/loss.py (1 - t) x + max(-x, 0), which
    cancels for x < 0; |x| (1 + t) covers the summands of both, so both are held to one bound.)  d/d(ps) = u (w (p - t) + BCE dw), dw = 1.5 p^2 (1 - p): |u| (w (p + t) + BCE dw) with 1 - p taken as
    1 + p (the kernel subtracts a rounded p from 1).  A row of d/d(pb): |u_bbox| |sign| + |u_giou| times riou_parts' magnitude.
    mut: riou_parts' mistakes, and 'dw075' (the factor of dw halved).
    Returns {name: (value, magnitude)} for class, bbox, giou [Lr], dpb [Lr,B,nq,4], dps [Lr,B,nq,nc]."""
    pbd, x, gb_, upd = _d(pb), _d(ps), _d(gtb), _d(up)
    Lr, B, nq, nc = x.shape
    gc, gbx, gg = (f32(v) for v in gains)
    li, bi, si, gi, cls = (t.detach().cpu().long() for t in (li, bi, si, gi, gtc))
    a, b = pbd[li, bi, si], gb_[gi]
    rp = riou_parts(a, b, mut=mut)
    tgt = torch.full((Lr, B, nq), nc, dtype=torch.long)
    score, kk = torch.zeros(Lr, B, nq, dtype=torch.float64), torch.ones(Lr, B, nq, dtype=torch.float64)
    tgt[li, bi, si], score[li, bi, si], kk[li, bi, si] = cls[gi], rp['iou'], rp['ku']
    pos = torch.nn.functional.one_hot(tgt, nc + 1)[..., :nc].bool()
    sc, k = score.unsqueeze(-1), kk.unsqueeze(-1)
    p = torch.sigmoid(x)
    t, m_t = torch.where(pos, sc, torch.zeros_like(x)), torch.where(pos, sc * k, torch.zeros_like(x))
    w = torch.where(pos, sc.expand_as(x), 0.75 * p * p)
    m_w = torch.where(pos, (sc * k).expand_as(x), w)
    soft = torch.log1p(torch.exp(-x.abs()))
    bce, m_bce = x.clamp(min=0) - x * t + soft, x.abs() * (1 + m_t) + soft
    dn = float(max(n, 1))
    res = {'class': ((bce * w).sum((1, 2, 3)) / dn * gc, (m_bce * m_w).sum((1, 2, 3)) / dn * gc),
           'bbox': (rp['l1'].view(Lr, n).sum(1) / n * gbx,) * 2,
           'giou': (rp['loss'].view(Lr, n).sum(1) / n * gg, rp['m_loss'].view(Lr, n).sum(1) / n * gg)}
    u = (upd[0] * (gc / n)).view(Lr, 1, 1, 1)
    f = 0.75 if 'dw075' in mut else 1.5
    dw, m_dw = torch.where(pos, torch.zeros_like(x), f * p * p * (1 - p)), torch.where(pos, torch.zeros_like(x), 1.5 * p * p * (1 + p))
    res['dps'] = (u * (w * (p - t) + bce * dw), u.abs() * (m_w * (p + m_t) + m_bce * m_dw))
    ub, ui = (upd[1] * (gbx / n))[li].unsqueeze(-1), (upd[2] * (gg / n))[li].unsqueeze(-1)
    sgn = torch.sign(a - b)
    dpb, m_dpb = torch.zeros_like(pbd), torch.zeros_like(pbd)
    dpb[li, bi, si], m_dpb[li, bi, si] = ub * sgn + ui * rp['grad'], ub.abs() * sgn.abs() + ui.abs() * rp['m_grad']
    res['dpb'] = (dpb, m_dpb)
    return res


# Roundings along the kernels' chains; a math function counts its documented error in ulp: expf 1, logf 1, log1pf 2, atanf 2, powf 1 (ROCm's
# OCML device library; doubled here, since the figures are stated and not proven), the division and sqrtf are correctly rounded (1).
DL_IOU_N = 8          # a.w a.h, b.w b.h, their sum, - inter, + eps (4 + inter's product 1), the division (1), the two edge differences (2)
DL_P_N = 4            # p = 1 / (1 + expf(-x)): expf (2), the sum, the division
DL_BCE_N = 8          # x t (1), max - . (1), expf (2), log1pf (4: 2 ulp, doubled) -> 7, the last sum (1)
DL_RIOU_N = 44        # iou (8), rho2 (3), sqrtf (1), cs (3), c2 (1), rho2 / c2 with c2's error twice (3), two atanf of a quotient (10), da (1),
#                       v (2), alpha's denominator (2) and division (1) with v twice (4), v alpha (1), the three outer differences (3), +1 spare
DL_RIOU_GRAD_N = 72   # the forward chain's intermediates (44 - 4) and, per component: dinter (3), d iou (6), ds (2), dcs (1), the distance
#                       term (7), inv and dat (5), dv (3), alpha dv (1), the two differences and the sign (3) = 31, +1 spare


def detr_bounds(B, nq, nc, n):
    """{name: b} (a = 0: everything is fp32) for detr_terms' outputs.
    class: per logit p (DL_P_N) twice in w = 0.75 p p (+2), or the IoU (DL_IOU_N); BCE (DL_BCE_N, with the IoU inside t: counted by ku in
    the magnitude, DL_IOU_N); the product (1).  Then a thread adds its nc logits in sequence (nc), block_sum256 (6 + 4), the reduce
    kernel's strided loop over the row blocks (ceil(nblk / 256)), block_sum256 again (10), / n and * gain (2).
    bbox: four differences and absolute values summed (7), ceil(n / 256) + 10, the gain, the division (2).  giou: DL_RIOU_N and the same sum.
    dps: p (4), w (10), t and p - t (DL_IOU_N + 1), the product (1), BCE (DL_BCE_N + DL_IOU_N), dw = 1.5 p p (1 - p) with p three
    times (12 + 4), the product and the sum (2), u = up * scale with scale = gain / n, and the last product (3).
    dpb: DL_RIOU_GRAD_N, the two upstream scalings (4), the product and the sum (2)."""
    nblk = -(-B * nq // 256)
    cls_elem = 2 * DL_P_N + 2 + DL_BCE_N + DL_IOU_N + 1
    return {'class': fp32_b(cls_elem + nc + 10 + -(-nblk // 256) + 10 + 2), 'bbox': fp32_b(7 + -(-n // 256) + 10 + 2),
            'giou': fp32_b(DL_RIOU_N + -(-n // 256) + 10 + 2),
            'dps': fp32_b(DL_P_N + 10 + DL_IOU_N + 2 + DL_BCE_N + DL_IOU_N + 16 + 2 + 3), 'dpb': fp32_b(DL_RIOU_GRAD_N + 6)}


def detr_match_cost(ps, pb, gtb, gtc, gains, alpha, gamma):
    """csrc/detrloss.hip tamtr_detr_match_cost (ops.detr_match_cost): C [Lr,B,nq,G] = g_class (pos - neg) + g_bbox |pred - box|_1 +
    g_giou (1 - RIOU), pos = alpha (1 - p)^gamma (-log(p + 1e-8)), neg = (1 - alpha) p^gamma (-log(1 - p + 1e-8)), p = sigmoid of the
    logit of the box's class; a non-finite entry is 0 (models/utils/ops.py:84-112).

    The rounding the operation has on purpose: p is an fp32 number.  Past logit 16.6 the quantised 1 - p decides neg (up to 1.4 in
    absolute cost between fp32 and fp64), so p = sigmoid(x) is formed in fp64 and rounded to fp32, and the focal part is evaluated at that
    p and at its two fp32 neighbours (inside [0, 1]): the device's expf may put p on either.  The envelope (lo, hi) of the three is what
    check(envelope=) takes; the value is the middle one.  1 - p is then exact (p >= 1/2) or one rounding, like p + 1e-8: the argument of
    each logarithm carries a relative 2^-24, the logarithm an absolute one: its magnitude is |log| + 1.
    An entry that is not finite (a NaN or a 0 / 0 aspect in a diverged prediction) has value, envelope and magnitude 0: check() then
    demands an exact 0 there.  Returns (value, magnitude, lo, hi)."""
    x = _d(ps)[..., gtc.detach().cpu().long()]                       # [Lr,B,nq,G]
    gc, gbx, gg, al, ga = (f32(v) for v in (*gains, alpha, gamma))
    p32 = torch.sigmoid(x).float()
    cand = [p32, torch.nextafter(p32, torch.zeros_like(p32)), torch.nextafter(p32, torch.ones_like(p32))]

    def focal(p):
        qp, qn = p + FOCAL_EPS, 1 - p + FOCAL_EPS
        pos, neg = al * (1 - p) ** ga * (-torch.log(qp)), (1 - al) * p ** ga * (-torch.log(qn))
        m = al * (1 - p) ** ga * (torch.log(qp).abs() + 1) + (1 - al) * p ** ga * (torch.log(qn).abs() + 1)
        return gc * (pos - neg), gc * m
    fs = [focal(p.double()) for p in cand]
    vals = torch.stack([f[0] for f in fs])
    rp = riou_parts(_d(pb).unsqueeze(-2), _d(gtb))
    rest = gbx * rp['l1'] + gg * rp['loss']
    val, lo, hi = fs[0][0] + rest, vals.amin(0) + rest, vals.amax(0) + rest
    mag = torch.stack([f[1] for f in fs]).amax(0) + gbx * rp['l1'] + gg * rp['m_loss']
    bad = ~torch.isfinite(val)
    zero = torch.zeros_like(val)
    return tuple(torch.where(bad, zero, t) for t in (val, mag, lo, hi))


# the focal part: p (DL_P_N), 1 - p and + 1e-8 twice (3), two logf (4), two powf of arguments that carry p's error gamma = 2 times (4 + 2 DL_P_N),
# four products per side (8), the difference and the gain (2); L1 (7) and its gain (1); RIOU (DL_RIOU_N), its gain (1); the two sums (2)
DL_COST_N = DL_P_N + 3 + 4 + 4 + 2 * DL_P_N + 8 + 2 + 8 + DL_RIOU_N + 1 + 2


def box_refine(delta, ref, cot):
    """csrc/detrloss.hip tamtr_box_refine_fwd / _bwd (ops.box_refine): y = sigmoid(delta + log(max(x, eps) / max(1 - x, eps))),
    x = clamp(ref, 0, 1), eps = 1e-5f, and d/d(delta), d/d(ref) for the cotangent cot, with torch's clamp gradients: each clamp passes
    where its bound holds, the bound included.

    delta as the kernel reads it (fp32, or bf16 widened), ref fp32.  Magnitudes: the logit is |delta| + |log| + 1 (the logarithm's
    argument carries relative roundings), the sigmoid sig_mag of that; 1 - y in the backward is taken as 1 + (magnitude of y), the kernel
    forms it from the stored y.  Returns {name: (value, magnitude)} for y, gd, gr."""
    d, r, g = _d(delta), _d(ref), _d(cot)
    x = r.clamp(0, 1)
    om = 1 - x
    lg = torch.log(x.clamp(min=REF_EPS) / om.clamp(min=REF_EPS))
    z, m_z = d + lg, d.abs() + lg.abs() + 1
    y = torch.sigmoid(z)
    m_y = sig_mag(y, m_z)
    gd, m_gd = g * y * (1 - y), g.abs() * m_y * (1 + m_y)
    di = torch.where(x >= REF_EPS, 1 / x, torch.zeros_like(x)) + torch.where(om.float().double() >= REF_EPS, 1 / om, torch.zeros_like(x))
    inside = ((r >= 0) & (r <= 1)).double()
    return {'y': (y, m_y), 'gd': (gd, m_gd), 'gr': (gd * di * inside, m_gd * di * inside)}


# y: two clamps exact, 1 - x (1), the division (1), logf (2), the sum (1), expf (2), 1 + e and the division (2) = 9, +1 spare.
# gd: y's chain twice (y and 1 - y) and three roundings; gr: the two reciprocals, their sum and the product (4) more.
BOX_REFINE_B = {'y': fp32_b(10), 'gd': fp32_b(2 * 10 + 3), 'gr': fp32_b(2 * 10 + 7)}


# ------------------------------------------------------------------------------------------------ clip + AdamW + EMA (csrc/optim.hip)
OPT_CHUNK = 8192       # elements per workgroup of csrc/optim.hip (tamtr_optim_chunk)
OPT_NORM_N = OPT_CHUNK // 256 + 6 + 4 + 2     # a thread's 32 squares added in sequence, block_sum (6 + 4); the chunks are added in double;
#                                               sqrt in double and its rounding to fp32 (1), one spare


def optim_step(p, g, m, v, e, step, lr, wd, beta1, beta2, eps, max_norm, ema_decay, mut=()):
    """csrc/optim.hip tamtr_optim_step (engine.FusedOptimStep.step): clip_grad_norm_(max_norm), AdamW, the EMA of the new value; one step
    from a given state.

    p, g, m, v, e, step, lr, wd: one entry per tensor (lr / wd: those of the tensor's parameter group).  g[i] None: no gradient this
    step (no Adam step, the count stays; the EMA still moves); m[i] None: an EMA-only entry; e[i] None: no EMA.  beta1, beta2, eps,
    lr wd and the EMA decay are the fp32 values the C ABI receives (lr wd: the fp32 product of the two fp32 values, as the kernel
    forms it); the bias corrections 1 - beta^t and everything after them are fp64.
    norm = sqrt(sum g^2) over every gradient; coef = min(1, max_norm / (norm + 1e-6)), 1 where max_norm <= 0; gc = coef g;
    m' = m + (1 - beta1)(gc - m); v' = beta2 v + (1 - beta2) gc^2; update = -(lr / (1 - beta1^t)) m' / (sqrt(v') / sqrt(1 - beta2^t) +
    eps); p' = (1 - lr wd) p + update; e' = d e + (1 - d) p'.
    Magnitudes: the same sums on absolute values; p' is |p| + |update|, so a parameter at 0 is held to the accuracy of its update, and
    `update` (what a test forms as p' - (1 - lr wd) p from the stored p') has the same one: the store of p' rounds relative to |p'|.
    mut: 'no_wd' (the decay dropped).
    Returns {'norm', 'coef': (value, magnitude)} and per tensor lists 'gc', 'm', 'v', 'update', 'p', 'e' of (value, magnitude) or None, and
    'step' (the new counts)."""
    b1, b2, ep, d = f32(beta1), f32(beta2), f32(eps), f32(ema_decay)
    sq = sum(float((_d(t) ** 2).sum()) for t in g if t is not None)
    norm = math.sqrt(sq)
    coef = min(1.0, f32(max_norm) / (norm + f32(1e-6))) if max_norm > 0 else 1.0
    res = {'norm': (torch.tensor(norm, dtype=torch.float64),) * 2, 'coef': (torch.tensor(coef, dtype=torch.float64),) * 2,
           'gc': [], 'm': [], 'v': [], 'update': [], 'p': [], 'e': [], 'step': []}
    for i, pt in enumerate(p):
        pd = _d(pt)
        new_p, m_p = pd, pd.abs()
        if m[i] is not None and g[i] is not None:
            lw = 0.0 if 'no_wd' in mut else f32(f32(lr[i]) * f32(wd[i]))
            t = float(step[i]) + 1
            gc = _d(g[i]) * coef
            md, vd = _d(m[i]), _d(v[i])
            mn, m_mn = md + (1 - b1) * (gc - md), md.abs() + (1 - b1) * (gc.abs() + md.abs())
            vn = b2 * vd + (1 - b2) * gc * gc
            step_size, bc2_sqrt = f32(lr[i]) / (1 - b1 ** t), math.sqrt(1 - b2 ** t)
            den = vn.sqrt() / bc2_sqrt + ep
            upd, m_upd = -step_size * mn / den, step_size * m_mn / den
            new_p, m_p = pd - lw * pd + upd, pd.abs() + m_upd
            res['gc'].append((gc, gc.abs())); res['m'].append((mn, m_mn)); res['v'].append((vn, vn))
            res['update'].append((upd, m_p)); res['p'].append((new_p, m_p)); res['step'].append(t)
        else:
            for k in ('gc', 'm', 'v', 'update'):
                res[k].append(None)
            res['p'].append((pd, torch.zeros_like(pd)))          # untouched: bit for bit
            res['step'].append(float(step[i]))
        if e[i] is not None:
            ed = _d(e[i])
            res['e'].append((d * ed + (1 - d) * new_p, d * ed.abs() + (1 - d) * m_p))
        else:
            res['e'].append(None)
    return res


def optim_bounds(clipped):
    """{name: b} (a = 0) for optim_step's outputs.  norm: OPT_NORM_N on the sum of squares, halved by the root: counted whole.  coef:
    the norm, + 1e-6, the division (2).  A gradient that is not clipped is left bit for bit (coef is an exact 1): the norm drops out of
    everything below.  gc: coef and the product (1).  m': gc, the difference, the product, the sum (3), one spare.  v': gc twice, the square,
    two products, the sum (4), one spare.  update: m', half of v' and sqrtf (1), bc2_sqrt rounded to fp32 and the division (2), + eps (1), step_size
    rounded (1), the product and the division (2).  p': the update, lr wd (1), its product with p (1), the two differences (2).
    e': p', 1 - d (1), two products, the sum (3)."""
    n_gc = OPT_NORM_N + 3 if clipped else 0
    n_m, n_v = n_gc + 4, 2 * n_gc + 5
    n_u = n_m + (n_v + 1) // 2 + 7
    return {'norm': fp32_b(OPT_NORM_N), 'coef': fp32_b(OPT_NORM_N + 2), 'gc': fp32_b(n_gc), 'm': fp32_b(n_m), 'v': fp32_b(n_v),
            'update': fp32_b(n_u + 4), 'p': fp32_b(n_u + 4), 'e': fp32_b(n_u + 8)}
