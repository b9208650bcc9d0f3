"""The fp64 error model of tests/ref64.py is tight enough to matter (CPU only).

For each kernel family: a CPU emulation of the kernel - fp32 arithmetic on the same bf16 operands, rounded where the kernel rounds -
passes the family's assertion, and mutants that the suite's earlier tolerances (1e-2 .. 3e-2 relative plus as much absolute) accept
are rejected by it."""
import math

import pytest
import torch

import ref64 as R
from weights import rnd, urnd


def bf(t):
    return t.bfloat16().float()


def rejected(what, got, ref, mag, a, b):
    with pytest.raises(AssertionError):
        R.check(what, got, ref, mag, a, b)


# ------------------------------------------------------------------------------------------------ contrastive head
def emu_contrastive(x, w, ls, bi, g, xinv_bf16=False, drop_last_row=False):
    """contrastive_fwd/bwd_kernel: fp32 on bf16 x; the logits and d(what) stay fp32, dx is rounded to bf16."""
    x, sc = x.float(), math.exp(float(ls))
    xi = 1 / (x * x).sum(-1, keepdim=True).sqrt().clamp_min(1e-12)
    if xinv_bf16:
        xi = bf(xi)
    wi = 1 / (w * w).sum(-1, keepdim=True).sqrt().clamp_min(1e-12)
    logits = torch.einsum('bqc,bkc->bqk', x, w) * xi * wi.transpose(1, 2) * sc + float(bi)
    xh, what = x * xi, w * wi
    gs = g * sc
    dh = torch.einsum('bqk,bkc->bqc', gs, what)
    dx = bf(xi * (dh - (dh * xh).sum(-1, keepdim=True) * xh))
    if drop_last_row:
        gs = gs.clone()
        gs[:, -1] = 0          # the partial last backward workgroup loses its last row
    dwhat = torch.einsum('bqk,bqc->bkc', gs, xh)
    dw = wi * (dwhat - (dwhat * what).sum(-1, keepdim=True) * what)
    return logits, dx, dw


def test_contrastive_emulation_passes_and_mutants_fail():
    B, Q, K, C = 2, 81, 10, 512
    x, w = rnd((B, Q, C), 1, 2.0).bfloat16(), rnd((B, K, C), 2)
    ls, bi = torch.tensor(math.log(1 / 0.07)), torch.tensor([-10.0])
    g = rnd((B, Q, K), 3, 0.05)
    ref = R.contrastive(x, w, ls, bi, g)
    n = C // 64 + 16
    lg, dx, dw = emu_contrastive(x, w, ls, bi, g)
    R.check('emu logits', lg, *ref['logits'], 0, R.fp32_b(n))
    R.check('emu dx', dx, *ref['dx'], 1, R.fp32_b(K + n))
    R.check('emu dw', dw, *ref['dw'], 0, R.fp32_b(Q // 4 + 2 * n + 16))
    # xinv rounded to bf16: 2^-9 relative on every logit
    lg_m, _, _ = emu_contrastive(x, w, ls, bi, g, xinv_bf16=True)
    assert R.old_close(lg_m, ref['logits'][0], 2e-2, 2e-2)
    rejected('xinv bf16', lg_m, *ref['logits'], 0, R.fp32_b(n))
    # one row of the partial last backward tile dropped from d(what)
    _, _, dw_m = emu_contrastive(x, w, ls, bi, g, drop_last_row=True)
    assert R.old_close(dw_m, ref['dw'][0], 2e-2, 2e-2)
    rejected('dropped row', dw_m, *ref['dw'], 0, R.fp32_b(Q // 4 + 2 * n + 16))


# ------------------------------------------------------------------------------------------------ self-attention
def emu_attention(q, k, v, nh, mask, go, mfma=True, p_bf16=False, lse_bf16=False):
    """selfattn kernels: fp32 scores and softmax; MFMA packs P and dS to bf16; delta from the stored bf16 O; stores rounded to bf16."""
    B, Q, C = q.shape
    dh = C // nh
    sc = dh ** -0.5

    def heads(t):
        return t.float().reshape(B, Q, nh, dh).transpose(1, 2)
    qh, kh, vh, gh = heads(q), heads(k), heads(v), heads(go)
    s = qh @ kh.transpose(-1, -2) * sc
    if mask is not None:
        s = s.masked_fill(mask[None, None], float('-inf'))
    m = s.amax(-1, keepdim=True)
    p = torch.exp(s - m)
    lsum = p.sum(-1, keepdim=True)
    pr = bf(p) if (mfma or p_bf16) else p
    o = bf(pr @ vh / lsum)
    lse = m + torch.log(lsum)
    if lse_bf16:
        lse = bf(lse)
    p = torch.exp(s - lse)
    dl = (gh * o).sum(-1, keepdim=True)
    dp = gh @ vh.transpose(-1, -2)
    ds = p * (dp - dl) * sc
    if mfma:
        ds = bf(ds)
    dq, dk = bf(ds @ kh), bf(ds.transpose(-1, -2) @ qh)
    dv = bf((bf(p) if mfma else p).transpose(-1, -2) @ gh)

    def back(t):
        return t.transpose(1, 2).reshape(B, Q, C)
    return back(o), back(dq), back(dk), back(dv)


def _attn_bounds(q, k, nh, Q, mfma):
    B, _, C = q.shape
    dh = C // nh
    qd, kd = q.double().view(B, Q, nh, dh), k.double().view(B, Q, nh, dh)
    S = float(torch.einsum('bihc,bjhc->bhij', qd.abs(), kd.abs()).max()) * dh ** -0.5
    fp = R.fp32_b(2 * 64 * S + 2 * Q + 64)
    r = R.U8 if mfma else 0
    return {'o': r + fp, 'dq': r + R.U8 + fp, 'dk': r + R.U8 + fp, 'dv': r + fp}


def test_attention_emulation_passes_and_mutants_fail():
    from tamtr_amd.loss import _dn_attn_mask
    B, Q, nh, dh = 2, 100, 2, 64
    C = nh * dh
    p = rnd((B, Q, 3 * C), 1).bfloat16()
    q, k, v = p[..., :C], p[..., C:2 * C], p[..., 2 * C:]
    go = rnd((B, Q, C), 2).bfloat16()
    mask = _dn_attn_mask(40, 60, 5, 4, 'cpu')
    ref = R.attention(q, k, v, nh, mask, go)
    names = ('o', 'dq', 'dk', 'dv')
    for mfma in (True, False):
        bd = _attn_bounds(q, k, nh, Q, mfma)
        for n, t in zip(names, emu_attention(q, k, v, nh, mask, go, mfma=mfma)):
            R.check(f'emu {n} mfma={mfma}', t, *ref[n], 1, bd[n])
    # the scalar kernel rounding P to bf16 (as only the MFMA kernel may)
    o_m = emu_attention(q, k, v, nh, mask, go, mfma=False, p_bf16=True)[0]
    assert R.old_close(o_m, ref['o'][0], 2e-2, 2e-2)
    rejected('scalar P bf16', o_m, *ref['o'], 1, _attn_bounds(q, k, nh, Q, False)['o'])
    # the log-sum-exp kept in bf16: every recomputed P off by up to 2^-9 |lse|
    bd = _attn_bounds(q, k, nh, Q, True)
    mut = emu_attention(q, k, v, nh, mask, go, lse_bf16=True)
    for n, t in zip(names[1:], mut[1:]):
        assert R.old_close(t, ref[n][0], 0, 3e-2 * float(ref[n][0].abs().max()))
    rejected('lse bf16 dv', mut[3], *ref['dv'], 1, bd['dv'])


# ------------------------------------------------------------------------------------------------ deformable core
def emu_msda(value, shapes, loc, aw, gout, drop_last=False, dc_bf16=False):
    """msda_fwd / locaw / gvalue kernels: fp32 corner weights from the fp32 pixel coordinate, fp32 sums; out and d(value) rounded to bf16."""
    B, L, M, D = value.shape
    _, Q, _, nl, P, _ = loc.shape
    v, g = value.float(), gout.float().view(B, Q, M, D)
    out = torch.zeros(B, Q, M, D)
    gval = torch.zeros(B * L * M, D)
    gloc, gaw = torch.zeros(B, Q, M, nl, P, 2), torch.zeros(B, Q, M, nl, P)
    bi, mi = torch.arange(B).view(B, 1, 1, 1), torch.arange(M).view(1, 1, M, 1)
    start = 0
    for l, (H, W) in enumerate(shapes):
        x, y = (t.float() for t in R.pixel_coords(loc[:, :, :, l], W, H))
        xf, yf = torch.floor(x), torch.floor(y)
        fx, fy = x - xf, y - yf
        a = aw[:, :, :, l].clone()
        if drop_last and l == nl - 1:
            a[:, -1, :, -1] = 0
        dcs = []
        for dy in (0, 1):
            for dx in (0, 1):
                xi, yi = (xf + dx).long(), (yf + dy).long()
                ok = ((xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)).float()
                row = start + yi.clamp(0, H - 1) * W + xi.clamp(0, W - 1)
                samp = v[bi, row, mi]
                wgt = (fx if dx else 1 - fx) * (fy if dy else 1 - fy) * a * ok
                out += (samp * wgt.unsqueeze(-1)).sum(3)
                gval.index_add_(0, ((bi * L + row) * M + mi).reshape(-1), (wgt.unsqueeze(-1) * g.unsqueeze(3)).reshape(-1, D))
                dc = (samp * g.unsqueeze(3)).sum(-1) * ok
                dcs.append(bf(dc) if dc_bf16 else dc)
        d00, d01, d10, d11 = dcs
        gaw[:, :, :, l] = (1 - fy) * ((1 - fx) * d00 + fx * d01) + fy * ((1 - fx) * d10 + fx * d11)
        gloc[:, :, :, l, :, 0] = ((1 - fy) * (d01 - d00) + fy * (d11 - d10)) * a * W
        gloc[:, :, :, l, :, 1] = ((1 - fx) * (d10 - d00) + fx * (d11 - d01)) * a * H
        start += H * W
    return bf(out.reshape(B, Q, M * D)), bf(gval.view(B, L, M, D)), gloc, gaw


def test_msda_emulation_passes_and_mutants_fail():
    shapes = [(101, 129), (5, 1), (1, 7)]      # a level of two row slices, W = 1, H = 1
    B, Q, M, D, P = 1, 24, 2, 16, 4
    L, nl = sum(h * w for h, w in shapes), len(shapes)
    value = rnd((B, L, M, D), 1, 0.02).bfloat16()
    loc = urnd((B, Q, M, nl, P, 2), 2, -0.1, 1.1)
    loc[0, :8, :, 0, :, 0] = (64.5 + urnd((8, M, P), 3, 0.01, 0.99)) / 129     # corners on both sides of the slice boundary
    loc[0, :8, :, 0, :, 1] = (49.5 + urnd((8, M, P), 4, 0.01, 1.99)) / 101
    aw = torch.softmax(rnd((B, Q, M, nl * P), 5), -1).view(B, Q, M, nl, P)
    gout = rnd((B, Q, M * D), 6, 0.05).bfloat16()
    ref = R.msda(value, shapes, loc, aw, gout)
    bo, bv, bl = R.fp32_b(4 * nl * P + 8), R.fp32_b(ref['runs'] + 8), R.fp32_b(D // 8 + 24)
    out, gv, gl, ga = emu_msda(value, shapes, loc, aw, gout)
    R.check('emu out', out, *ref['out'], 1, bo)
    R.check('emu gvalue', gv, *ref['gvalue'], 1, bv)
    R.check('emu gloc', gl, *ref['gloc'], 0, bl)
    R.check('emu gaw', ga, *ref['gaw'], 0, bl)
    # the last sample of the last query dropped (a partial last tile)
    out_m = emu_msda(value, shapes, loc, aw, gout, drop_last=True)[0]
    assert R.old_close(out_m, ref['out'][0], 2e-2, 2e-2)
    rejected('dropped sample', out_m, *ref['out'], 1, bo)
    # d(loc) from corner dot products rounded to bf16
    gl_m = emu_msda(value, shapes, loc, aw, gout, dc_bf16=True)[2]
    assert R.old_close(gl_m, ref['gloc'][0], 2e-2, 2e-2)
    rejected('bf16 corner dots', gl_m, *ref['gloc'], 0, bl)


# ------------------------------------------------------------------------------------------------ ln_gate
def emu_ln_gate(x, xz, gamma, beta, gout, eps=1e-5, stats_bf16=False, drop_last_token=False):
    """ln_gate_fwd/bwd_kernel: fp32 statistics of fp32 x, out and d(z) rounded to bf16, dx / dgamma / dbeta fp32."""
    N, D = x.shape
    xs = bf(x) if stats_bf16 else x
    mean = xs.mean(-1, keepdim=True)
    rstd = ((xs - mean) ** 2).mean(-1, keepdim=True).add(eps).rsqrt()
    z, g = xz[:, D:2 * D].float(), gout.float()
    xh = (x - mean) * rstd
    y = xh * gamma + beta
    sg = torch.sigmoid(z)
    out = bf(y * z * sg)
    gy = g * z * sg
    dz = bf(g * y * sg * (1 + z * (1 - sg)))
    gxh = gy * gamma
    dx = rstd * (gxh - gxh.mean(-1, keepdim=True) - xh * (gxh * xh).mean(-1, keepdim=True))
    keep = torch.ones(N, 1)
    if drop_last_token:
        keep[-1] = 0
    return out, dx, dz, (gy * xh * keep).sum(0), (gy * keep).sum(0)


def test_ln_gate_emulation_passes_and_mutants_fail():
    N, D = 77, 256
    x = rnd((N, D), 1) * 1.5 + 0.3
    xz = rnd((N, 2 * D), 2).bfloat16()
    gamma, beta = 1 + 0.2 * rnd((D,), 3), 0.1 * rnd((D,), 4)
    gout = rnd((N, D), 5, 0.01).bfloat16()
    ref = R.ln_gate(x, xz, gamma, beta, gout)
    nblk = (N + 63) // 64
    bounds = {'out': (1, R.fp32_b(48)), 'dx': (0, R.fp32_b(48)), 'dz': (1, R.fp32_b(48)),
              'dgamma': (0, R.fp32_b(nblk + 80)), 'dbeta': (0, R.fp32_b(nblk + 80))}
    for n, t in zip(bounds, emu_ln_gate(x, xz, gamma, beta, gout)):
        R.check(f'emu {n}', t, *ref[n], *bounds[n])
    # statistics from bf16-rounded x (the fp32 x is exact: nothing may round it)
    dx_m = emu_ln_gate(x, xz, gamma, beta, gout, stats_bf16=True)[1]
    assert R.old_close(dx_m, ref['dx'][0], 1e-1, 1e-1)             # test_ln_gate: 5 * 2e-2
    rejected('bf16 stats', dx_m, *ref['dx'], *bounds['dx'])
    # the last token of the partial last backward block missing from the d(gamma) partials
    dg_m = emu_ln_gate(x, xz, gamma, beta, gout, drop_last_token=True)[3]
    assert R.old_close(dg_m, ref['dgamma'][0], 1e-1, 1e-1 * N ** 0.5)
    rejected('dropped token', dg_m, *ref['dgamma'], *bounds['dgamma'])
