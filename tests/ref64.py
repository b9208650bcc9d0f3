"""fp64 references with an error model for the bf16 hot-path kernels (tests/test_gpu_bf16_kernels.py, tests/test_ref64_host.py).

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


def check(what, got, ref, mag, a, b, log=True):
    """Elementwise |got - ref| <= a 2^-8 |ref| + b mag.  NaN in ref must be NaN in got (and only there).  Returns the worst ratio.
    log=False: one piece of a larger tensor (see report())."""
    got, ref, mag = _d(got), _d(ref), _d(mag)
    assert got.shape == ref.shape == mag.shape, f'{what}: shapes {tuple(got.shape)} {tuple(ref.shape)} {tuple(mag.shape)}'
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(got), nan), f'{what}: NaN pattern differs ({int(torch.isnan(got).sum())} vs {int(nan.sum())})'
    live = ~nan
    assert bool(torch.isfinite(got[live]).all()), f'{what}: non-finite output'
    err = (got - ref).abs()[live]
    bound = (a * U8 * ref.abs() + b * mag)[live]
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
