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


# ------------------------------------------------------------------------------------------------ max-sigmoid text gate
import gate_cases as G

BF16 = torch.bfloat16


def emu_gate(x, gk, bias, v, nh, scale, gout, drop_row=None, no_rs_head=None, round_before_scale=False, aw_bf16=False):
    """gate_fwd / gate_bwd_kernel: the T dot products as hc serial fp32 multiply-adds per pixel, the first maximum, 1 / (1 + exp(-z)),
    v * (a * scale); the backward from the stored fp32 a; out, dv, dx rounded to the maps' dtype; dgk, dbias by fp32 torch reductions."""
    st = bf if x.dtype == BF16 else (lambda t: t)
    B, C, H, W = x.shape
    T, hc, HW = gk.shape[1], C // nh, H * W
    xf, vf, go = (t.float().reshape(B, nh, hc, HW) for t in (x, v, gout))
    g = gk.view(B, T, nh, hc).permute(0, 2, 1, 3)                  # [B,nh,T,hc]
    acc = torch.zeros(B, nh, T, HW)
    for c in range(hc):
        acc = acc + g[..., c, None] * xf[:, :, c, None, :]
    if drop_row is not None:
        acc[:, :, drop_row] = float('-inf')
    arg = acc.argmax(2)
    best = acc.gather(2, arg.unsqueeze(2)).squeeze(2)
    rs = torch.tensor(float(hc)).sqrt()
    a = 1 / (1 + torch.exp(-(best / rs + bias.view(1, nh, 1))))
    if aw_bf16:
        a = bf(a)
    s = torch.tensor(scale, dtype=torch.float32)
    out = st(st(vf * a.unsqueeze(2)) * s) if round_before_scale else st(vf * (a * s).unsqueeze(2))
    daw = torch.zeros(B, nh, HW)
    for c in range(hc):
        daw = daw + go[:, :, c] * vf[:, :, c]
    dv = st(go * (a * s).unsqueeze(2))
    dl = daw * s * a * (1 - a) / rs
    if no_rs_head is not None:
        dl[:, no_rs_head] = dl[:, no_rs_head] * rs
    gsel = g.gather(2, arg[..., None].expand(B, nh, HW, hc))       # [B,nh,HW,hc]
    dx = st(dl[..., None] * gsel).transpose(2, 3)
    sel = torch.zeros(B, nh, T, HW).scatter_(2, arg.unsqueeze(2), dl.unsqueeze(2))
    dgk = torch.matmul(sel, xf.transpose(2, 3)).permute(0, 2, 1, 3).reshape(B, T, C)
    dbias = dl.sum((0, 2)) * math.sqrt(hc)
    shp = (B, C, H, W)
    return {'out': out.reshape(shp), 'dv': dv.reshape(shp), 'dx': dx.reshape(shp), 'dlogit': dl, 'dgk': dgk, 'dbias': dbias}


def _old_gate_ok(name, got, ref):
    """The rules these checks replace: out, dv 1e-2 / 1e-2 (test_gate_kernel_bf16, test_gate_bf16_full_size_vs_oracle); the gradients
    2e-2 relative plus 2e-2 of the largest gradient."""
    if name in ('out', 'dv'):
        return R.old_close(got, ref, 1e-2, 1e-2)
    return R.old_close(got, ref, 2e-2, 2e-2 * float(ref.abs().max()))


@pytest.mark.parametrize('dt', [torch.float32, BF16])
def test_gate_emulation_passes(dt):
    for case, scale in (('t17', 0.37), ('vec_one_pass', 1.0), ('px1_t37_hc64', 1.0)):
        B, C, nh, H, W, T = G.GATE_NCHW[case]
        x, gk, bias, v, gout = G.gate_inputs(G.GATE_NCHW[case], dt)
        ref = R.maxsigmoid_gate(x, gk, bias, v, nh, scale, gout)
        ab = R.gate_bounds(C // nh, H * W, B, ref['zmax'], dt == BF16)
        for n, t in emu_gate(x, gk, bias, v, nh, scale, gout).items():
            R.check(f'emu gate {case} {n}', t, *ref[n], *ab[n])


def test_gate_mutants_fail():
    shape = G.GATE_NCHW['t17']
    B, C, nh, H, W, T = shape
    x, gk, bias, v, gout = G.gate_inputs(shape, BF16)
    scale = 0.37
    ref = R.maxsigmoid_gate(x, gk, bias, v, nh, scale, gout)
    ab = R.gate_bounds(C // nh, H * W, B, ref['zmax'], True)
    assert int((ref['arg'] == 15).sum()) > 0
    # the last row of the first TC = 16 chunk dropped from the max: the pixels it wins take the runner-up.  (The old rule sees this one
    # too at this size: a plain rejection.)
    m = emu_gate(x, gk, bias, v, nh, scale, gout, drop_row=15)
    rejected('dropped text row', m['out'], *ref['out'], *ab['out'])
    rejected('dropped text row', m['dgk'], *ref['dgk'], *ab['dgk'])
    # dlogit without the 1 / sqrt(hc) on head 1 (the old rule sees it in dx and dgk: a plain rejection)
    m = emu_gate(x, gk, bias, v, nh, scale, gout, no_rs_head=1)
    rejected('no 1/sqrt(hc)', m['dlogit'], *ref['dlogit'], *ab['dlogit'])
    rejected('no 1/sqrt(hc)', m['dx'], *ref['dx'], *ab['dx'])
    # out rounded to bf16 before the multiply by scale: two roundings
    m = emu_gate(x, gk, bias, v, nh, scale, gout, round_before_scale=True)
    assert _old_gate_ok('out', m['out'], ref['out'][0])
    rejected('rounded before scale', m['out'], *ref['out'], *ab['out'])
    # the saved gate kept in bf16: 2^-9 relative on out, dv and, through a (1 - a), on every gradient
    m = emu_gate(x, gk, bias, v, nh, scale, gout, aw_bf16=True)
    for n in ('out', 'dv', 'dx', 'dgk'):
        assert _old_gate_ok(n, m[n], ref[n][0]), n
        rejected('gate in bf16 ' + n, m[n], *ref[n], *ab[n])
    # the text tile staged in bf16: every dot product off by up to 2^-9 of its magnitude
    m = emu_gate(x, bf(gk), bias, v, nh, scale, gout)
    for n in ('dv', 'dx', 'dgk'):
        assert _old_gate_ok(n, m[n], ref[n][0]), n
        rejected('text tile in bf16 ' + n, m[n], *ref[n], *ab[n])


# ------------------------------------------------------------------------------------------------ CPAM
def emu_cpam(x, gout, border_075=False, du_twice=False, argmax_x_chunk=None, s2_bf16=False):
    """cpam_fwd / bwd / dp kernels and the pool: fp32 arithmetic on the map's values; out, dxd, du, dp and dx stored in the map's dtype."""
    import torch.nn.functional as F
    st = bf if x.dtype == BF16 else (lambda t: t)
    B, C, H, W = x.shape
    Hp, Wp, Cg = H // 2, W // 2, C // 8
    xf, go = x.float(), gout.float().view(B, 8, Cg, H, W)
    p, idx = F.max_pool2d(xf, 3, 2, 1, return_indices=True)

    def up(t):
        return F.interpolate(t, scale_factor=2, mode='bilinear', align_corners=False)
    s1 = 1 / (1 + torch.exp(-up(p)))
    c = (s1 * xf).view(B, 8, Cg, H, W)
    am = c.argmax(2)
    if argmax_x_chunk is not None:
        am[:, argmax_x_chunk] = xf.view(B, 8, Cg, H, W)[:, argmax_x_chunk].argmax(1)
    m = c.gather(2, am.unsqueeze(2)).squeeze(2)
    s2 = 1 / (1 + torch.exp(-m))
    if s2_bf16:
        s2 = bf(s2)
    out = st(s2.unsqueeze(2) * c).view(B, C, H, W)
    S = torch.zeros(B, 8, H, W)
    for ch in range(Cg):
        S = S + go[:, :, ch] * c[:, :, ch]
    dm = s2 * (1 - s2) * S
    hot = F.one_hot(am, Cg).permute(0, 1, 4, 2, 3).float()
    dc = (go * s2.unsqueeze(2) + hot * dm.unsqueeze(2)).view(B, C, H, W)
    dxd = st(dc * s1)
    du = st(st(dc * xf * s1) * (1 - s1)) if du_twice else st(dc * xf * s1 * (1 - s1))

    def adjoint(d):
        q = torch.zeros(B, C, Hp, Wp, requires_grad=True)
        return torch.autograd.grad(up(q), q, d)[0]
    dp = adjoint(du)
    if border_075:                                                  # the last pixel column into the last pooled column: 0.75, not 1
        last = torch.zeros_like(du)
        last[..., W - 1] = du[..., W - 1]
        dp = dp - 0.25 * adjoint(last)
    dp = st(dp)
    pooled = torch.zeros(B, C, H * W).scatter_add_(2, idx.view(B, C, -1), dp.view(B, C, -1)).view(B, C, H, W)
    return {'out': out, 's2': s2, 'dxd': dxd, 'du': du, 'dp': dp, 'dx': st(dxd + pooled)}


def _old_cpam_ok(name, got, ref):
    """test_cpam_bf16_and_argument_checks / test_cpam_channels_last_kernels: out 1e-2 / 1e-2, dx 3e-2 / 3e-2."""
    tol = 1e-2 if name == 'out' else 3e-2
    return R.old_close(got, ref, tol, tol)


@pytest.mark.parametrize('dt', [torch.float32, BF16])
def test_cpam_emulation_passes(dt):
    for shape in ((2, 64, 12, 16), (1, 128, 2, 2), (1, 256, 6, 6), (2, 64, 4, 6)):
        x, gout = G.cpam_inputs(shape, dt, G.CPAM_SEED.get((shape, dt), 5))
        ref = R.cpam(x, gout)
        ab = R.cpam_bounds(shape[1] // 8, ref['zmax'], dt == BF16)
        for n, t in emu_cpam(x, gout).items():
            R.check(f'emu cpam {shape} {n}', t, *ref[n], *ab[n])


def test_cpam_mutants_fail():
    shape = (2, 64, 12, 16)
    x, gout = G.cpam_inputs(shape, BF16, G.CPAM_SEED.get((shape, BF16), 5))
    ref = R.cpam(x, gout)
    ab = R.cpam_bounds(shape[1] // 8, ref['zmax'], True)
    # the dp gather's last column weighted 0.75 where the clamped tap makes it 1
    # (at 12 x 16 the old rule sees this one too: a plain rejection)
    m = emu_cpam(x, gout, border_075=True)
    rejected('border weight 0.75', m['dx'], *ref['dx'], *ab['dx'])
    # du rounded twice (once before its last factor)
    # The bound of dx allows the worst case of its three honest roundings, which a fourth seldom exceeds: the stored du itself shows it.
    m = emu_cpam(x, gout, du_twice=True)
    assert _old_cpam_ok('dx', m['dx'], ref['dx'][0])
    rejected('du rounded twice', m['du'], *ref['du'], *ab['du'])
    # chunk 3's argmax taken over x, not over sigmoid(u) x
    m = emu_cpam(x, gout, argmax_x_chunk=3)
    assert _old_cpam_ok('out', m['out'], ref['out'][0])
    rejected('argmax over x', m['out'], *ref['out'], *ab['out'])
    rejected('argmax over x', m['dx'], *ref['dx'], *ab['dx'])
    # s2 kept in bf16
    m = emu_cpam(x, gout, s2_bf16=True)
    assert _old_cpam_ok('out', m['out'], ref['out'][0]) and _old_cpam_ok('dx', m['dx'], ref['dx'][0])
    rejected('s2 in bf16', m['out'], *ref['out'], *ab['out'])
    rejected('s2 in bf16', m['s2'], *ref['s2'], *ab['s2'])


# ------------------------------------------------------------------------------------------------ inputs of the GPU tests
def test_gate_and_cpam_gpu_inputs_have_no_ambiguous_argmax():
    """The argmax-routed gradients (dx, dgk of the gate; dx of CPAM) are discontinuous where the two largest candidates are closer than
    twice their fp32 bound.  Every seeded input of tests/test_gpu_gates_ref64.py must have none of these, judged from the fp64 reference
    alone (the GPU tests repeat the assertion before they look at a kernel's output)."""
    for case, shape in G.GATE_NCHW.items():
        for dt in (torch.float32, BF16):
            x, gk, bias, v, gout = G.gate_inputs(shape, dt, G.GATE_SEED.get((case, dt), 1))
            ref = R.maxsigmoid_gate(x, gk, bias, v, shape[2], 1.0, None)
            assert R.ambiguous(ref['gap'], ref['gap_mag'], R.fp32_b(shape[1] // shape[2])) == 0, (case, dt)
    cases = [(s, BF16) for s in G.CPAM_CL_BF16] + [(s, torch.float32) for s in G.CPAM_CL_F32]
    cases += [(s, dt) for s in G.CPAM_NCHW for dt in (torch.float32, BF16)] + [(G.CPAM_NCHW_GRID_LIMIT, torch.float32)]
    for shape, dt in cases:
        x, _ = G.cpam_inputs(shape, dt, G.CPAM_SEED.get((shape, dt), 5))
        ref = R.cpam(x, None)
        b = R.cpam_bounds(shape[1] // 8, ref['zmax'], dt == BF16)['c'][1]
        assert R.ambiguous(ref['gap'], ref['gap_mag'], b) == 0, (shape, dt)


# ------------------------------------------------------------------------------------------------ the channels-last gate's LDS limit
class _ChannelsLastMap:
    """What ops.gate_cl_ok looks at, for a bf16 channels-last CUDA map [2, C, 12, 12] (no GPU here)."""
    is_cuda, dtype = True, BF16

    def __init__(self, C):
        self.shape = (2, C, 12, 12)

    def dim(self):
        return 4

    def stride(self):
        B, C, H, W = self.shape
        return (H * W * C, 1, W * C, C)

    def element_size(self):
        return 2

    def data_ptr(self):
        return 0


def test_gate_cl_ok_counts_the_text_rows():
    """tamtr_maxsigmoid_gate_cl_fwd keeps the fp32 text tile [T, C] in 60 KiB of LDS: 80 rows fit at C = 64 and do not at C = 256."""
    import tamtr_amd.ops as ops
    assert ops.gate_cl_ok(_ChannelsLastMap(256), 256, 8) and ops.gate_cl_ok(_ChannelsLastMap(256), 256, 8, T=10)
    assert ops.gate_cl_ok(_ChannelsLastMap(256), 256, 8, T=60) and not ops.gate_cl_ok(_ChannelsLastMap(256), 256, 8, T=61)
    assert not ops.gate_cl_ok(_ChannelsLastMap(256), 256, 8, T=80)
    assert ops.gate_cl_ok(_ChannelsLastMap(64), 64, 8, T=80)
    assert ops.gate_cl_ok(_ChannelsLastMap(512), 512, 8, T=30) and not ops.gate_cl_ok(_ChannelsLastMap(512), 512, 8, T=31)


# ------------------------------------------------------------------------------------------------ LayerNorm, cross-merge, depthwise front end
import ss2d_cases as S


def emu_layer_norm(x, gamma, beta, gout, eps=1e-5, drop_last_token=False, stats_bf16=False, next_stats=False, c2_no_div=False):
    """ln_fwd / ln_bwd_kernel and their narrow forms: fp32 on the activation's values, the two-pass mean, mean and rstd stored in fp32 and
    read back by the backward; d(gamma) / d(beta) as 16 tokens per wave in sequence, 4 waves per workgroup, the workgroups in order; out
    and dx rounded to the activation dtype.  Mutants: the backward's stats rounded to bf16 / taken from the next token, c2 without its
    1 / D, the last token missing from d(gamma) / d(beta)."""
    st = bf if x.dtype == BF16 else (lambda t: t)
    N, D = x.shape
    xf, g, inv = x.float(), gout.float(), torch.tensor(1.0 / D)
    mean = xf.sum(-1, keepdim=True) * inv
    c = xf - mean
    rstd = torch.rsqrt((c * c).sum(-1, keepdim=True) * inv + eps)
    if stats_bf16:
        mean, rstd = bf(mean), bf(rstd)
    out = st((xf - mean) * rstd * gamma + beta)
    if next_stats:
        mean, rstd = torch.cat([mean[1:], mean[-1:]]), torch.cat([rstd[1:], rstd[-1:]])
    xh = (xf - mean) * rstd
    gxh = g * gamma
    c1 = gxh.sum(-1, keepdim=True) * inv
    c2 = (gxh * xh).sum(-1, keepdim=True) * (1.0 if c2_no_div else inv)
    dx = st(rstd * (gxh - c1 - xh * c2))
    gt = g.clone()
    if drop_last_token:
        gt[-1] = 0

    def ordered(t):
        t = torch.cat([t, torch.zeros(-N % 64, D)]).view(-1, 4, 16, D)
        wave = torch.zeros(t.shape[0], 4, D)
        for i in range(16):
            wave = wave + t[:, :, i]
        blk = wave[:, 0] + wave[:, 1] + wave[:, 2] + wave[:, 3]
        tot = blk[0]
        for r in range(1, blk.shape[0]):
            tot = tot + blk[r]
        return tot
    return out, dx, ordered(gt * xh), ordered(gt)


def emu_ln_gate_f32(x, xz, gamma, beta, gout, eps=1e-5):
    """ln_gate_fwd / bwd_kernel<float>: emu_ln_gate without the roundings to bf16."""
    N, D = x.shape
    mean = x.mean(-1, keepdim=True)
    rstd = ((x - mean) ** 2).mean(-1, keepdim=True).add(eps).rsqrt()
    z = xz[:, D:2 * D]
    xh = (x - mean) * rstd
    y = xh * gamma + beta
    sg = 1 / (1 + torch.exp(-z))
    gy = gout * (z * sg)
    gxh = gy * gamma
    dx = rstd * (gxh - gxh.mean(-1, keepdim=True) - xh * (gxh * xh).mean(-1, keepdim=True))
    return y * (z * sg), dx, gout * y * (sg * (1 + z * (1 - sg))), (gy * xh).sum(0), gy.sum(0)


def _old_ln_ok(got, ref, n):
    """test_layer_norm_kernel in bf16: out 2e-2 / 2e-2, dx 0.1 / 0.1, dgamma and dbeta 0.1 relative + 0.1 sqrt(n) absolute.  Per output,
    the fraction of elements that rule accepts."""
    tol = {'out': (2e-2, 2e-2), 'dx': (0.1, 0.1), 'dgamma': (0.1, 0.1 * n ** 0.5), 'dbeta': (0.1, 0.1 * n ** 0.5)}
    return {k: float(((t.double() - ref[k][0]).abs() <= tol[k][1] + tol[k][0] * ref[k][0].abs()).double().mean()) for k, t in zip(tol, got)}


@pytest.mark.parametrize('dt', list(S.LN_D))
def test_layer_norm_emulation_passes_every_case(dt):
    for D in S.LN_D[dt]:
        for ntok in S.LN_NTOK:
            for kind in S.LN_KINDS:
                ins = S.ln_inputs(D, ntok, S.DT[dt], kind)
                S.ln_assert(f'emu ln[{dt},{D},{ntok},{kind}]', emu_layer_norm(*ins), *ins)
            for flat in (True, False):
                ins = S.ln_constant_inputs(D, ntok, S.DT[dt], flat)
                S.ln_constant_assert(f'emu ln[{dt},{D},{ntok},constant]', emu_layer_norm(*ins), *ins, flat)
    for D, ntok in (S.LN_GATE_F32 if dt == 'fp32' else []):
        ins = S.ln_gate_inputs(D, ntok)
        S.ln_gate_assert(f'emu ln_gate[fp32,{D},{ntok}]', emu_ln_gate_f32(*ins), *ins)


def test_layer_norm_mutants_fail():
    """On the old test's own rows (bf16, 211 tokens, 2 randn + 0.5).  Its tolerances accept bf16 statistics outright, the next token's
    statistics in dx at D = 1024, and a dropped token in most channels; every mutant misses a counted bound."""
    D, ntok = 256, 211
    ins = S.ln_inputs(D, ntok, BF16, 'ordinary')
    ref = R.layer_norm(*ins)
    ab = R.layer_norm_bounds(ntok, True)
    assert set(_old_ln_ok(emu_layer_norm(*ins), ref, ntok).values()) == {1.0}
    # the last token of the partial last workgroup missing from the partial sums: the old absolute term (1.45) hides it in most channels
    m = emu_layer_norm(*ins, drop_last_token=True)
    old = _old_ln_ok(m, ref, ntok)
    assert old['out'] == old['dx'] == 1 and old['dgamma'] > 0.5 and old['dbeta'] > 0.5
    rejected('dropped token', m[2], *ref['dgamma'], *ab['dgamma'])
    rejected('dropped token', m[3], *ref['dbeta'], *ab['dbeta'])
    # mean and rstd kept in bf16: accepted outright
    m = emu_layer_norm(*ins, stats_bf16=True)
    assert set(_old_ln_ok(m, ref, ntok).values()) == {1.0}
    rejected('bf16 stats', m[1], *ref['dx'], *ab['dx'])
    rejected('bf16 stats', m[2], *ref['dgamma'], *ab['dgamma'])
    insf = S.ln_inputs(D, ntok, torch.float32, 'offset')
    reff = R.layer_norm(*insf)
    rejected('bf16 stats', emu_layer_norm(*insf, stats_bf16=True)[0], *reff['out'], *R.layer_norm_bounds(ntok, False)['out'])
    # the backward normalises token t with the statistics of token t + 1: dx passes the old rule at D = 1024
    ins4 = S.ln_inputs(1024, ntok, BF16, 'ordinary')
    ref4 = R.layer_norm(*ins4)
    m = emu_layer_norm(*ins4, next_stats=True)
    old = _old_ln_ok(m, ref4, ntok)
    assert old['out'] == old['dx'] == old['dbeta'] == 1 and old['dgamma'] > 0.5
    rejected('next token\'s stats', m[1], *ref4['dx'], *ab['dx'])
    rejected('next token\'s stats', m[2], *ref4['dgamma'], *ab['dgamma'])
    # c2 = sum(gxh xhat) without its 1 / D: the old tolerance sees this one too (a plain rejection)
    m = emu_layer_norm(*ins, c2_no_div=True)
    assert _old_ln_ok(m, ref, ntok)['dx'] < 1
    rejected('c2 without 1 / D', m[1], *ref['dx'], *ab['dx'])


# ---- cross-merge
def emu_cross_merge(y4, g, H, W, pdt, swap_hw=False, drop_dir3_block=False, truncate=False):
    """cross_merge_fwd* / bwd*: (y0 + y2) + T(y1 + y3) in fp32; the backward copies g into both flattenings, rounded to nearest-even for
    bf16 planes.  Mutants: the transposed planes read with H and W exchanged, direction 3 left out of the second 16-channel block, the
    backward planes truncated."""
    ymT = g2 = None
    if y4 is not None:
        y = y4.float()
        B, _, D, L = y.shape
        y3 = y[:, 3].clone()
        if drop_dir3_block:
            y3[:, 16:32] = 0
        t = y[:, 1] + y3
        t = t.view(B, D, H, W).transpose(2, 3).reshape(B, D, L) if swap_hw else t.view(B, D, W, H).transpose(2, 3).reshape(B, D, L)
        ymT = ((y[:, 0] + y[:, 2]) + t).transpose(1, 2).contiguous()
    if g is not None:
        B, L, D = g.shape
        gm = g.transpose(1, 2)
        g2 = torch.stack([gm.contiguous(), gm.reshape(B, D, H, W).transpose(2, 3).reshape(B, D, L)], 1)
        if pdt == BF16:
            g2 = (g2.view(torch.int32) & -65536).view(torch.float32).bfloat16() if truncate else g2.bfloat16()
    return ymT, g2


def _cm_cases():
    for dt, shapes in ((torch.float32, S.CM_GENERIC), (BF16, S.CM_FWD_BF16_GENERIC + S.CM_FWD16 + S.CM_BWD16 + S.CM_BWD_BF16_GENERIC)):
        for H, W in dict.fromkeys(shapes):
            for D in S.CM_D:
                yield dt, D, H, W
    yield BF16, 32, *S.CM_BWD16_D32_ONLY[0]


def test_cross_merge_emulation_passes_every_case():
    for dt, D, H, W in _cm_cases():
        y4, g = S.cm_inputs(D, H, W, dt)
        S.cm_assert(f'emu cross_merge[{S.dtn(dt)},{D},{H}x{W}]', *emu_cross_merge(y4, g, H, W, dt), y4, g, H, W)


def test_cross_merge_mutants_fail():
    D = 32
    # H and W exchanged where the column-major planes are read: the same kernel on a square map, wrong on any other
    y4, g = S.cm_inputs(D, 16, 16, torch.float32)
    S.cm_assert('swap at 16 x 16', emu_cross_merge(y4, None, 16, 16, torch.float32, swap_hw=True)[0], None, y4, None, 16, 16)
    for H, W in ((17, 16), (13, 21), (5, 40)):
        y4, g = S.cm_inputs(D, H, W, torch.float32)
        with pytest.raises(AssertionError):
            S.cm_assert('H and W exchanged', emu_cross_merge(y4, None, H, W, torch.float32, swap_hw=True)[0], None, y4, None, H, W)
    # direction 3 left out of the second channel block
    y4, g = S.cm_inputs(D, 34, 30, BF16)
    with pytest.raises(AssertionError):
        S.cm_assert('direction 3 dropped', emu_cross_merge(y4, None, 34, 30, BF16, drop_dir3_block=True)[0], None, y4, None, 34, 30)
    # the backward planes truncated to bf16
    with pytest.raises(AssertionError):
        S.cm_assert('truncated', None, emu_cross_merge(None, g, 34, 30, BF16, truncate=True)[1], None, g, 34, 30)
    S.cm_assert('rounded', None, emu_cross_merge(None, g, 34, 30, BF16)[1], None, g, 34, 30)


def test_cross_merge_cases_reach_the_kernels_they_are_listed_for():
    """The dispatch of tamtr_cross_merge_fwd / _bwd as restated in tests/ss2d_cases.py, on every listed shape."""
    assert all(S.cm_fwd_kernel(H, W, True) == 'cross_merge_fwd_kernel<bf16_t>' for H, W in S.CM_FWD_BF16_GENERIC)
    assert all(S.cm_fwd_kernel(H, W, True) == 'cross_merge_fwd16_kernel' for H, W in S.CM_FWD16)
    assert all(S.cm_bwd_kernel(H, W, True) == 'cross_merge_bwd16_kernel' for H, W in S.CM_BWD16)
    assert all(S.cm_bwd_kernel(H, W, True) == 'cross_merge_bwd_kernel<bf16_t>' for H, W in S.CM_BWD_BF16_GENERIC + S.CM_BWD16_D32_ONLY)
    assert S.cm_bwd_kernel(160, 160, True) == 'cross_merge_bwd16_kernel'          # the bench's first level
    # none of the shapes of test_ss2d_bf16_planes_are_the_f32_kernels_rounded_once reaches the 32 x 32 backward
    assert all(S.cm_bwd_kernel(H, W, True) == 'cross_merge_bwd_kernel<bf16_t>' for H, W in ((24, 40), (16, 24), (8, 16), (36, 28)))
    assert S.cm_fwd_kernel(*S.CM_MISALIGNED_FWD, True, aligned=False) == 'cross_merge_fwd_kernel<bf16_t>'
    assert S.cm_bwd_kernel(*S.CM_MISALIGNED_BWD, True, aligned=False) == 'cross_merge_bwd_kernel<bf16_t>'
    assert S.ln_kernels(64, True) == ('ln_fwd_narrow_kernel<64>', 'ln_bwd_narrow_kernel<64>') and S.ln_kernels(128, True, aligned=False)[1] == 'ln_bwd_kernel<bf16_t, 128>'
    vec = [s for s in S.DW_SHAPES if S.dw_vector_path(*s)]
    assert vec == [(4, 4), (16, 16), (20, 12), (32, 16), (36, 20)] and not any(S.dw_vector_path(*s) for s in S.DW_ROUNDED_ONCE)


# ---- depthwise front end
def emu_dwconv(xz, D, w, bias, gout2, pdt, pad_replicate=False, col_taps_transposed=False, seam_double=False, no_z_term=False, bwd_no_bias=False):
    """dwconv_cross_fwd / bwd_kernel: nine fp32 multiply-adds onto the bias, v / (1 + exp(-v)), both flattenings stored in the plane's
    dtype; backward: the sum of the two planes times s (1 + z (1 - s)) with the conv recomputed, the transposed 3 x 3 for d(xi) (stored in
    the activation dtype), d(weight) / d(bias) as one partial per (image, 16 x 16 tile) added in order.  Mutants: see the arguments."""
    import torch.nn.functional as F
    B, H, W = xz.shape[:3]
    st_a = bf if xz.dtype == BF16 else (lambda t: t)
    st_p = bf if pdt == BF16 else (lambda t: t)
    xi = xz[..., :D].float().permute(0, 3, 1, 2)
    xp = F.pad(xi, (1, 1, 1, 1), mode='replicate') if pad_replicate else F.pad(xi, (1, 1, 1, 1))
    xp0 = F.pad(xi, (1, 1, 1, 1))
    wf = w.view(D, 3, 3)
    bc = bias if bias is not None else torch.zeros(D)

    def conv(src, wk, b_):
        acc = b_.view(1, D, 1, 1).expand(B, D, H, W).clone()
        for ky in range(3):
            for kx in range(3):
                acc = acc + wk[:, ky, kx].view(1, D, 1, 1) * src[:, :, ky:ky + H, kx:kx + W]
        return acc
    z = conv(xp, wf, bc)
    zc = conv(xp, wf.transpose(1, 2), bc) if col_taps_transposed else z
    out = torch.stack([st_p(z / (1 + torch.exp(-z))).flatten(2), st_p(zc / (1 + torch.exp(-zc))).transpose(2, 3).flatten(2)], 1)
    g2 = gout2.float()
    g = g2[:, 0].view(B, D, H, W) + g2[:, 1].view(B, D, W, H).transpose(2, 3)
    zb = conv(xp0, wf, torch.zeros(D) if bwd_no_bias else bc)
    sg = 1 / (1 + torch.exp(-zb))
    gz = g * (sg * (1 + (0 if no_z_term else zb * (1 - sg))))
    gp = F.pad(gz, (1, 1, 1, 1))
    dx = conv(gp, wf.flip(1, 2), torch.zeros(D))
    part = []
    for b in range(B):
        for h0 in range(0, H, 16):
            for w0 in range(0, W, 16):
                e = 1 if seam_double else 0
                hs, ws = slice(max(h0 - e, 0), min(h0 + 16 + e, H)), slice(max(w0 - e, 0), min(w0 + 16 + e, W))
                gt = gz[b, :, hs, ws]
                row = [(gt * xp0[b, :, hs.start + ky:hs.stop + ky, ws.start + kx:ws.stop + kx]).sum((1, 2)) for ky in range(3) for kx in range(3)]
                part.append(torch.stack(row + [gt.sum((1, 2))], 1))
    tot = part[0]
    for p in part[1:]:
        tot = tot + p
    return out, st_a(dx.permute(0, 2, 3, 1)), tot[:, :9], (tot[:, 9] if bias is not None else None)


def _dw_cases():
    for H, W in S.DW_SHAPES:
        for form in S.dw_forms(H, W):
            for D in S.DW_D:
                for bias in (True, False):
                    yield H, W, form, D, bias, 0
    (H, W), D, extra = S.DW_STRIDE_CASE
    for form in S.DW_FORMS:
        yield H, W, form, D, True, extra


def test_dwconv_emulation_passes_every_case():
    for H, W, form, D, bias, extra in _dw_cases():
        xz, w, b, gout2 = S.dw_inputs(D, H, W, form, bias, extra)
        S.dw_assert(f'emu dwconv[{form},{D},{H}x{W},{bias},{extra}]', emu_dwconv(xz, D, w, b, gout2, S.dw_dtypes(form)[1]), xz, D, w, b, gout2)


def _old_dw_ok(got, ref, n):
    """test_dwconv_silu_cross in bf16: out 1e-2 / 1e-2, dx 0.1 / 0.1, dw and db 0.1 relative + 0.1 sqrt(B H W) absolute."""
    tol = {'out': (1e-2, 1e-2), 'dx': (0.1, 0.1), 'dw': (0.1, 0.1 * n ** 0.5), 'db': (0.1, 0.1 * n ** 0.5)}
    return {k: R.old_close(t, ref[k][0], *tol[k]) for k, t in zip(tol, got)}


def test_dwconv_mutants_fail():
    """Every listed mutant misses a counted bound.  The old test's tolerances (bf16: 1e-2 forward, 0.1 backward) reject them as well at
    this shape and with a unit-variance cotangent: O(1) and O(0.1) mistakes; what they could not see is the accuracy, not these."""
    D, H, W, form = 32, 36, 20, 'bf16_f32planes'          # a tile seam along both axes, a partial last tile
    xz, w, b, gout2 = S.dw_inputs(D, H, W, form, True)
    ref = R.dwconv_silu_cross(xz, D, w, b, gout2)
    ab = R.dwconv_bounds(ref['zmax'], S.DW_B, H, W, True, False)
    n = S.DW_B * H * W
    names = ('out', 'dx', 'dw', 'db')

    def run(**kw):
        return dict(zip(names, emu_dwconv(xz, D, w, b, gout2, torch.float32, **kw)))
    assert all(_old_dw_ok(run().values(), ref, n).values())
    # edge-replicate padding in the forward: O(1) on the border pixels; the old tolerance sees it too
    m = run(pad_replicate=True)
    assert not _old_dw_ok(m.values(), ref, n)['out']
    rejected('replicate padding', m['out'], *ref['out'], *ab['out'])
    # the taps transposed in the column-major pass only: plane 0 is right, plane 1 is not; the old tolerance sees it too
    m = run(col_taps_transposed=True)
    assert not _old_dw_ok(m.values(), ref, n)['out']
    S_ = R.check('plane 0', m['out'][:, 0], ref['out'][0][:, 0], ref['out'][1][:, 0], *ab['out'], log=False)
    assert S_ <= 1
    rejected('taps transposed', m['out'][:, 1], ref['out'][0][:, 1], ref['out'][1][:, 1], *ab['out'])
    # halo pixels counted into d(weight) / d(bias) on both sides of a tile seam
    m = run(seam_double=True)
    old = _old_dw_ok(m.values(), ref, n)
    assert old['out'] and old['dx'] and not old['dw']          # (no bf16 shape of the old test has a seam; at this one its rule sees it)
    rejected('seam counted twice', m['dw'], *ref['dw'], *ab['dw'])
    rejected('seam counted twice', m['db'], *ref['db'], *ab['db'])
    xs, ws_, bs, gs = S.dw_inputs(D, 16, 16, form, True)            # (no seam: the same kernel)
    S.dw_assert('seam mutant on one tile', emu_dwconv(xs, D, ws_, bs, gs, torch.float32, seam_double=True), xs, D, ws_, bs, gs)
    # SiLU' without its z (1 - s) term
    m = run(no_z_term=True)
    assert not _old_dw_ok(m.values(), ref, n)['dx']            # (a plain rejection)
    rejected('SiLU\' without z (1 - s)', m['dx'], *ref['dx'], *ab['dx'])
    # the bias left out of the backward's recomputed conv
    m = run(bwd_no_bias=True)
    assert not _old_dw_ok(m.values(), ref, n)['dx']            # (a plain rejection: the old rule accepts 9 elements in 10)
    rejected('no bias in the recomputed conv', m['dx'], *ref['dx'], *ab['dx'])
    rejected('no bias in the recomputed conv', m['dw'], *ref['dw'], *ab['dw'])


# ================================================================================================ MFMA linear and x_proj (tests/gemm_cases.py)
import gemm_cases as GM

MUTANT_TABLE = []      # (family, mutant, passes the old rule, passes the new rule)


def _report_mutants(family):
    """The per-mutant old-rule / new-rule table (profiles/r11_gemm_ref64.txt), written where TAMTR_REF64_REPORT is set."""
    for fam, name, old, new in MUTANT_TABLE:
        if fam == family:
            R.note(f'mutant [{fam}] {name}: old rule {"passes" if old else "fails"}, new rule {"passes" if new else "fails"}')


def _new_rule(fn):
    try:
        fn()
        return True
    except AssertionError:
        return False


def emu_linear(x, w, b, kernel, drop_last_k=False, double_round=False, lose_lo=False, tail_from_m2=False, transpose_tile=False):
    """tamtr_linear_bf16: exact products of bf16 values added in fp32 (torch's order: any order is within the bound), the bias as the
    kernel adds it - in fp32 (tile, n512_k64) or as bf16(b) + bf16(b - bf16(b)) (wstat) - and one rounding to bf16.  Mutants: the last
    k-step of 64 left out; the accumulator rounded to bf16 before the bias is added and again after; the bias's lo half lost; the last
    row computed from row M - 2; the first 32 x 32 tile transposed."""
    xf, wf = x.float(), w.float()
    M = xf.shape[0]
    acc = (xf[:, :-64] @ wf[:, :-64].t()) if drop_last_k else xf @ wf.t()
    if tail_from_m2:
        acc[M - 1] = acc[M - 2]
    if b is None:
        bv = torch.zeros(wf.shape[0])
    elif kernel == 'wstat':
        hi = bf(b)
        bv = hi if lose_lo else hi + bf(b - hi)
    else:
        bv = b
    y = (bf(acc) + bv if double_round else acc + bv).bfloat16()
    if transpose_tile:
        y[:32, :32] = y[:32, :32].t().clone()
    return y


def test_linear_cases_reach_the_kernels_they_are_listed_for():
    """The dispatch of tamtr_linear_bf16 and of ops.linear_bf16's backward as restated in tests/gemm_cases.py."""
    for kernel, M, N, K, _, _ in GM.LINEAR_CASES:
        assert GM.linear_kernel(N, K) == kernel
    assert {k for k, *_ in GM.LINEAR_CASES} == {'wstat', 'n512_k64', 'tile'}
    assert all(sum(1 for k, *_r in GM.LINEAR_CASES if k == kn and not _r[3]) == 1 for kn in ('wstat', 'n512_k64', 'tile'))     # one without bias each
    for M, N, K, kdx, streams, S in GM.GRAD_CASES:
        assert (GM.dx_kernel(N, K), GM.colsum_streams(M, N), GM.split_count(M)) == (kdx, streams, S)
    assert {c[3] for c in GM.GRAD_CASES} == {'wstat', 'n512_k64', 'tile', 'lib'}
    assert {c[4] for c in GM.GRAD_CASES} == {True, False} and {c[5] > 1 for c in GM.GRAD_CASES} == {True, False}
    # the six shapes of test_linear_bf16_kernel: four on wstat, two on the tile kernel, none on the full-row kernel
    old = [(1000, 512, 512), (2048, 128, 64), (77, 256, 192), (8193, 256, 256), (33, 1024, 128), (4999, 2048, 512)]
    assert sorted(GM.linear_kernel(N, K) for _, N, K in old) == ['tile', 'tile'] + ['wstat'] * 4
    assert GM.linear_kernel(1536, 256) == 'n512_k64' and GM.linear_kernel(1536, 512) == 'n512_k64' and GM.linear_kernel(512, 512) == 'wstat'
    B, L, N, K = GM.ZERO_ROWS_CASE
    assert GM.linear_kernel(N, K) == 'n512_k64'
    assert [GM.xproj_ks_mb(c[3]) for c in GM.XPROJ_CASES] == GM.XPROJ_KS_MB


@pytest.mark.parametrize('kernel,M,N,K,bias,what', GM.LINEAR_CASES, ids=GM.LINEAR_IDS)
def test_linear_emulation_passes(kernel, M, N, K, bias, what):
    x, w, b, _ = GM.linear_inputs(M, N, K, bias)
    GM.linear_assert(f'emu linear[{kernel},{M}x{N}x{K}]', emu_linear(x, w, b, kernel), kernel, M, N, K, bias)


def test_linear_emulation_passes_the_poison_and_gradient_assertions():
    for kernel, M, N, K, inf_row in GM.POISON_CASES:
        x, w, b = GM.poison_inputs(M, N, K, inf_row)
        GM.poison_assert(f'emu linear[{kernel}]', emu_linear(x, w, b, kernel), kernel, M, N, K, inf_row)
        leak = emu_linear(x, w, b, kernel)
        leak[inf_row - 1] = float('nan')                      # the poison in a third row
        with pytest.raises(AssertionError):
            GM.poison_assert('leak', leak, kernel, M, N, K, inf_row)
        leak = emu_linear(x, w, b, kernel)
        col = int(torch.isinf(leak[inf_row].float()).nonzero()[0])
        leak[inf_row, col] = float('nan')                     # the last row's NaN in one column of the Inf's row
        with pytest.raises(AssertionError, match='pattern of row'):
            GM.poison_assert('NaN inside the Inf row', leak, kernel, M, N, K, inf_row)
        leak = emu_linear(x, w, b, kernel)
        leak[inf_row, col] = -leak[inf_row, col]              # an Inf of the wrong sign
        with pytest.raises(AssertionError, match='pattern of row'):
            GM.poison_assert('sign flipped inside the Inf row', leak, kernel, M, N, K, inf_row)
    for M, N, K, kdx, _, S in GM.GRAD_CASES[:4]:
        x, w, b, gy = GM.linear_inputs(M, N, K, True, True)
        g, xf, wf = gy.float(), x.float(), w.float()
        dw = (g.t() @ xf).bfloat16().float()                   # S = 1: the library's bf16 result, widened
        GM.grads_assert(f'emu linear_bf16[{M}x{N}x{K}]', (g @ wf).bfloat16(), dw, g.sum(0), M, N, K, True)
    # zero_rows: y and dx of the masked input, dw as the difference of two rounded products
    B, L, N, K = GM.ZERO_ROWS_CASE
    x, w, b, gy, idx, xz = GM.zero_rows_inputs()
    y = emu_linear(xz.reshape(B * L, K), w, b, 'n512_k64').view(B, L, N)
    g, wf = gy.float(), w.float()
    dx = (g @ wf).bfloat16()
    dx[:, idx] = 0
    dw = bf(g.reshape(B * L, N).t() @ x.float().reshape(B * L, K)) - bf(g[:, idx].reshape(-1, N).t() @ x.float()[:, idx].reshape(-1, K))
    GM.zero_rows_assert('emu zero_rows', y, dx, dw, g.sum((0, 1)), 'n512_k64', True)
    with pytest.raises(AssertionError):                       # the masked rows left in dw
        GM.zero_rows_assert('mutant zero_rows, masked rows left in dw:', y, dx, bf(g.reshape(B * L, N).t() @ x.float().reshape(B * L, K)), g.sum((0, 1)), 'n512_k64', True)


def test_linear_emulation_is_exact_where_no_addition_rounds_and_mutants_are_not():
    for kernel, M, N, K in GM.EXACT_CASES:
        if M > 2000:
            continue                                           # (the same kernels at the smaller shapes: the host run stays short)
        x, w, b = GM.exact_inputs(M, N, K)
        n_tie = GM.exact_assert(f'emu linear[{kernel},exact]', emu_linear(x, w, b, kernel), kernel, M, N, K)
        for kw in ({'drop_last_k': True}, {'transpose_tile': True}) + (({'lose_lo': True},) if kernel == 'wstat' else ()):
            with pytest.raises(AssertionError):
                GM.exact_assert('mutant', emu_linear(x, w, b, kernel, **kw), kernel, M, N, K)
        if kernel == 'wstat':                                  # the lost lo half changes exactly the ties
            assert int((emu_linear(x, w, b, kernel, lose_lo=True) != GM.exact_want(M, N, K)).sum()) == n_tie


def test_linear_sums_emulation_passes_and_dropped_rows_fail():
    """db on the streaming kernel's chain and dw in slices: the emulations pass; a column sum that leaves out the one-row tail block and
    a dw that leaves out its last slice miss the counted bounds."""
    M, N, K = 8193, 256, 256                                   # db: 129 workgroups of 64 rows, the last one holds one row
    assert GM.colsum_streams(M, N) and R.colsum_chain(M, N, True) == 8 + 8 + 9 + 16
    g = GM.linear_inputs(M, N, K, True, True)[3].float()
    ref, ab = GM.linear_ref(M, N, K, True, True), R.linear_grad_bounds(M, N, K, 1, True, True)
    R.check('emu db (streaming chain)', g.sum(0), *ref['db'], *ab['db'])
    rejected('db without the one-row tail block', g[:-1].sum(0), *ref['db'], *ab['db'])
    M, N, K = 1000, 512, 512
    assert R.colsum_chain(M, N, False) == 63 + 16
    g = GM.linear_inputs(M, N, K, True, True)[3].float()
    rejected('db without the last row (direct slab_sum)', g[:-1].sum(0), *GM.linear_ref(M, N, K, True, True)['db'], *R.linear_grad_bounds(M, N, K, 1)['db'])
    M, N, K = 8200, 2048, 64                                   # dw in 4 slices of 2050 rows, fp32 partials added in order
    S = GM.split_count(M)
    x, _, _, gy = GM.linear_inputs(M, N, K, True, True)
    parts = [gy.float()[i * (M // S):(i + 1) * (M // S)].t() @ x.float()[i * (M // S):(i + 1) * (M // S)] for i in range(S)]
    ref, ab = GM.linear_ref(M, N, K, True, True), R.linear_grad_bounds(M, N, K, S)
    R.check('emu dw (S = 4)', parts[0] + parts[1] + parts[2] + parts[3], *ref['dw'], *ab['dw'])
    rejected('dw without its last slice', parts[0] + parts[1] + parts[2], *ref['dw'], *ab['dw'])


def _old_linear(y, ref):
    """test_linear_bf16_kernel's forward rule: rtol 2^-8, atol 1e-3."""
    return R.old_close(y.float(), ref['y'][0], 2 ** -8, 1e-3)


def test_linear_mutants_fail():
    """Each mutant misses the counted bound; the old rule (2^-8 relative + 1e-3) accepts the dropped k-step of small products and the
    lost lo half of the bias."""
    # the last k-step dropped, its products small: the last 64 columns of x scaled by 2^-12 (exact in bf16)
    kernel, M, N, K = 'n512_k64', 130, 512, 192
    x, w, b, _ = GM.linear_inputs(M, N, K)
    xs = x.clone()
    xs[:, -64:] = (xs[:, -64:].float() * 2.0 ** -12).bfloat16()
    ref = R.linear(xs, w, b)
    R.linear_check('emu, small last k-step', emu_linear(xs, w, b, kernel).float(), ref, kernel, K)
    m = emu_linear(xs, w, b, kernel, drop_last_k=True)
    old, new = _old_linear(m, ref), _new_rule(lambda: R.linear_check('dropped k-step', m.float(), ref, kernel, K))
    MUTANT_TABLE.append(('linear', 'last k-step of 64 dropped (products of 2^-12)', old, new))
    assert old and not new
    # the bias rounded to bf16 once on the W-stationary model; |b| < 0.5, where bf16(b) is within 2^-10 < 1e-3 of b
    kernel, M, N, K = 'wstat', 33, 2048, 128
    x, w, _, _ = GM.linear_inputs(M, N, K)
    b = urnd((N,), 5, -0.49, 0.49)
    ref = R.linear(x, w, b)
    R.linear_check('emu, |b| < 0.5', emu_linear(x, w, b, kernel).float(), ref, kernel, K)
    m = emu_linear(x, w, b, kernel, lose_lo=True)
    old, new = _old_linear(m, ref), _new_rule(lambda: R.linear_check('lo lost', m.float(), ref, kernel, K))
    MUTANT_TABLE.append(('linear', 'wstat bias rounded to bf16 once (lo lost), |b| < 0.5', old, new))
    assert old and not new
    b1 = GM.linear_inputs(M, N, K)[2]                          # the cases' own bias, |b| of about 1: the old rule may see some elements
    ref1 = GM.linear_ref(M, N, K)
    m = emu_linear(x, w, b1, kernel, lose_lo=True)
    new = _new_rule(lambda: R.linear_check('lo lost', m.float(), ref1, kernel, K))
    MUTANT_TABLE.append(('linear', 'wstat bias rounded to bf16 once (lo lost), |b| ~ 1', _old_linear(m, ref1), new))
    assert not new
    # the other three, on the tile model
    kernel, M, N, K = 'tile', 77, 256, 192
    x, w, b, _ = GM.linear_inputs(M, N, K)
    ref = GM.linear_ref(M, N, K)
    for name, kw in (('accumulator rounded to bf16, bias added, rounded again', {'double_round': True}),
                     ('tail row taken from row M - 2', {'tail_from_m2': True}), ('one 32 x 32 tile transposed', {'transpose_tile': True})):
        m = emu_linear(x, w, b, kernel, **kw)
        new = _new_rule(lambda: R.linear_check(name, m.float(), ref, kernel, K))
        MUTANT_TABLE.append(('linear', name, _old_linear(m, ref), new))
        assert not new, name
    _report_mutants('linear')


# ---- x_proj
def emu_xproj(i, R_, plane_bf16, no_round=False, pad_row=False, swap_B_dirs=False, drop_second_slice=False):
    """csrc/xproj.hip in fp32 on the CPU with the kernels' rounding points and padding: the packed weights zero-padded to MB * 32 rows /
    KS * 16 columns, u and the gradient rows rounded to bf16, the forward and the d/d(u2) product rounded to bf16, the fold in fp32, the
    weight gradient as per-(image, 1 024-pixel slice) partial tiles of MB * 32 rows added in order.  Mutants: the forward not rounded; a
    padding column of wT non-zero (2^-10), met by a padding row of G that re-reads a real row instead of being zero (the clamp the dW
    kernel uses for its loads, without its zeroing); the B rows of directions i and i + 2 exchanged; the second dW slice left out."""
    u2, wx, gdtr, gB, gC, gu = (i[k] for k in ('u2', 'wx', 'gdtr', 'gB', 'gC', 'gu'))
    B, _, D, L = u2.shape
    C = R_ + 2 * R.XP_N
    KS, MB = GM.xproj_ks_mb(R_)
    wc = torch.stack([torch.cat([wx[0], wx[2]], 0), torch.cat([wx[1], wx[3]], 0)]).bfloat16().float()       # [2, 2C, D]
    wcat = torch.nn.functional.pad(wc, (0, 0, 0, MB * 32 - 2 * C))
    wT = torch.nn.functional.pad(wc.transpose(1, 2), (0, KS * 16 - 2 * C))                                   # [2, D, KP]
    U = bf(u2.float())
    out = torch.einsum('imd,bidl->biml', wcat, U)[:, :, :2 * C]
    if not no_round:
        out = bf(out)
    h = out.view(B, 2, 2, C, L).permute(0, 2, 1, 3, 4).reshape(B, 4, C, L)
    got = {'dtr': h[:, :, :R_].contiguous(), 'Bs': h[:, :, R_:R_ + R.XP_N].contiguous(), 'Cs': h[:, :, R_ + R.XP_N:].contiguous()}
    if swap_B_dirs:
        got['Bs'] = got['Bs'][:, [2, 3, 0, 1]].contiguous()
    G = bf(R.xproj_rows(gdtr, gB, gC))                                                                        # [B, 2, 2C, L]
    Gk = torch.nn.functional.pad(G, (0, 0, 0, KS * 16 - 2 * C))
    if pad_row:
        assert KS * 16 > 2 * C
        wT = wT.clone()
        wT[:, :, 2 * C] = 2.0 ** -10
        Gk[:, :, 2 * C] = G[:, :, 0]
    g = gu.float()
    s = g[:, :2] + g[:, 2:] + bf(torch.einsum('idm,biml->bidl', wT, Gk))
    got['gu2'] = s.bfloat16() if plane_bf16 else s
    Gm = torch.nn.functional.pad(G, (0, 0, 0, MB * 32 - 2 * C))
    nsl = R.xproj_slices(L)
    part = torch.zeros(B * nsl, 2, MB * 32, D)
    for b in range(B):
        for sl in range(nsl):
            if drop_second_slice and sl == 1:
                continue
            px = slice(sl * R.XP_SLICE, min((sl + 1) * R.XP_SLICE, L))
            part[b * nsl + sl] = torch.einsum('iml,idl->imd', Gm[b, :, :, px], U[b, :, :, px])
    assert float(part[:, :, 2 * C:].abs().max() if MB * 32 > 2 * C else 0) == 0, 'the accumulator rows beyond 2C are exact zeros'
    got['part'] = part[:, :, :2 * C].contiguous()
    tot = got['part'][0]
    for r in got['part'][1:]:
        tot = tot + r
    got['dw'] = tot
    return got


@pytest.mark.parametrize('planes', ['fp32', 'bf16'])
@pytest.mark.parametrize('B,D,L,R_,what', GM.XPROJ_CASES, ids=[f'{c[0]}x{c[1]}x{c[2]}-R{c[3]}' for c in GM.XPROJ_CASES])
def test_xproj_emulation_passes(B, D, L, R_, what, planes):
    pb = planes == 'bf16'
    GM.xproj_assert(f'emu xproj[{planes},{B}x{D}x{L},R={R_}]', emu_xproj(GM.xproj_inputs(B, D, L, R_, pb), R_, pb), B, D, L, R_, pb)


def _old_xproj(got, ref, i):
    """test_xproj_kernels_vs_fp32_products_of_the_same_bf16_operands: per stored copy, forward 8e-3 relative + 8e-3 max|ref|; d/d(u2) 1e-6
    relative + 8e-3 max|product|; dWcat 1e-4 relative + 1e-4 max|ref|."""
    ok = {'fwd': True, 'gu2': True, 'dw': True}
    rows_g = R.xproj_rows(got['dtr'], got['Bs'], got['Cs'])
    rows_r = R.xproj_rows(ref['dtr'][0], ref['Bs'][0], ref['Cs'][0])
    for c in range(2):
        ok['fwd'] &= R.old_close(rows_g[:, c], rows_r[:, c], 8e-3, 8e-3 * float(rows_r[:, c].abs().max()))
        ok['gu2'] &= R.old_close(got['gu2'][:, c].float(), ref['gu2'][0][:, c], 1e-6, 8e-3 * float(ref['prod'][:, c].abs().max()))
        ok['dw'] &= R.old_close(got['dw'][c], ref['dw'][0][c], 1e-4, 1e-4 * float(ref['dw'][0][c].abs().max()))
    return ok


def test_xproj_mutants_fail():
    """Each mutant misses its assertion; the old rule accepts the unrounded forward and the non-zero padding column."""
    def run(case, key, name, **kw):
        B, D, L, R_ = case
        i, ref = GM.xproj_inputs(B, D, L, R_, False), GM.xproj_ref(B, D, L, R_, False)
        m = emu_xproj(i, R_, False, **kw)
        assert all(_old_xproj(emu_xproj(i, R_, False), ref, i).values())
        old = _old_xproj(m, ref, i)[key]
        new = _new_rule(lambda: GM.xproj_assert(name, m, B, D, L, R_, False))
        MUTANT_TABLE.append(('xproj', name, old, new))
        return old, new
    old, new = run((2, 256, 40, 8), 'fwd', 'forward not rounded to bf16', no_round=True)
    assert old and not new
    old, new = run((2, 256, 8, 5), 'gu2', 'a padding column of wT non-zero (2^-10) against a padding row of G that re-reads row 0', pad_row=True)
    assert old and not new
    old, new = run((2, 256, 40, 8), 'fwd', 'B rows of directions i and i + 2 exchanged', swap_B_dirs=True)
    assert not new
    old, new = run((2, 256, 1032, 16), 'dw', 'second dW slice (8 pixels) dropped', drop_second_slice=True)
    assert not new
    _report_mutants('xproj')


# ================================================================================================ BatchNorm (tests/bn_cases.py)
import bn_cases as K


def _f(v):
    return torch.tensor(v, dtype=torch.float32)


def _fma(a, b, c):
    """fmaf: the product of two fp32 values is exact in fp64; the sum is rounded to fp64 and then to fp32 (the second rounding is the one
    that counts)."""
    return (a.double() * b.double() + c.double()).float()


def _chan(a, b):
    """One Chan combine of (n, mean, M2) triples as combine_slices does it, an empty result left alone."""
    (n, mean, m2), (nb, mb, m2b) = a, b
    nt = n + nb
    ok = nt > 0
    div = torch.where(ok, nt, torch.ones_like(nt))
    d = mb - mean
    return nt, torch.where(ok, mean + d * (nb / div), mean), torch.where(ok, m2 + (m2b + d * d * (n * nb / div)), m2)


def emu_bn_combine(part):
    """combine_slices on partials [C, S, 3]: thread t takes triples t, t + 256, ... in sequence, the 64-lane butterfly, the 4 waves in order."""
    C, S, _ = part.shape
    rounds = -(-S // 256)
    p = torch.zeros(C, rounds * 256, 3)
    p[:, :S] = part
    p = p.view(C, rounds, 256, 3)
    acc = tuple(torch.zeros(C, 256) for _ in range(3))
    for r in range(rounds):
        acc = _chan(acc, tuple(p[:, r, :, i] for i in range(3)))
    lanes = torch.arange(256)
    for o in (32, 16, 8, 4, 2, 1):
        acc = _chan(acc, tuple(t[:, lanes ^ o] for t in acc))
    tot = tuple(torch.zeros(C) for _ in range(3))
    for w in range(4):
        tot = _chan(tot, tuple(t[:, 64 * w] for t in acc))
    return tot


def emu_bn_finalize(part, eps, mom, rm, rv, rv_biased=False, rstd_unbiased=False):
    """bn_finalize_kernel / the head of bn_apply_kernel -> {mean, rstd, running_mean, running_var}.  Mutants: the running variance updated
    with the biased variance; rstd taken from the unbiased one."""
    n, mean, m2 = emu_bn_combine(part)
    var = m2 / n
    unb = torch.where(n > 1, m2 / (n - 1).clamp_min(1), var)
    got = {'mean': mean, 'rstd': torch.rsqrt((unb if rstd_unbiased else var) + _f(eps))}
    if rm is not None:
        keep = _f(1.0) - _f(mom)
        got.update({'running_mean': keep * rm + _f(mom) * mean, 'running_var': keep * rv + _f(mom) * (var if rv_biased else unb)})
    return got


def _bn_gather(layout, dims, plan, N):
    """Row indices [S, L] of every partial's rows and the mask of the real ones; a slot past the end re-reads the partial's first row
    (the channels-last kernels' redirected load)."""
    if layout == 'nchw':
        B, HW = dims
        sh = plan[1]
        starts = (torch.arange(B).view(B, 1) * HW + torch.arange(sh).view(1, sh) * R.BN_SLICE).reshape(-1)
        lens = torch.tensor([min(R.BN_SLICE, HW - s * R.BN_SLICE) for s in range(sh)]).repeat(B)
    else:
        starts = torch.arange(plan[4]) * plan[3]
        lens = (N - starts).clamp_max(plan[3])
    L = int(lens.max())
    mask = torch.arange(L).view(1, L) < lens.view(-1, 1)
    idx = torch.where(mask, starts.view(-1, 1) + torch.arange(L).view(1, L), starts.view(-1, 1))
    return idx, mask, lens.float()


def _bn_partials(layout, xf, idx, mask, lens, tail_4096=False, unshifted=False):
    """bn_stats_kernel (two-pass inside a slice) | bncl_stats_kernel (sums of x - k and (x - k)^2, M2 = s2 - s1 m) -> [C, S, 3].
    Mutants: the NCHW tail slice counted as 4096 elements; the channels-last sums taken of x itself."""
    xp, m = xf[idx], mask.unsqueeze(-1)
    n = lens.view(-1, 1)
    if layout == 'nchw':
        cnt = torch.full_like(n, float(R.BN_SLICE)) if tail_4096 else n
        mean = torch.where(m, xp, torch.zeros(())).sum(1) / cnt
        d = torch.where(m, xp - mean.unsqueeze(1), torch.zeros(()))
        m2 = (d * d).sum(1)
        n = cnt
    else:
        k = torch.zeros_like(xp[:, 0]) if unshifted else xp[:, 0]
        d = xp - k.unsqueeze(1)
        if unshifted:
            d = torch.where(m, d, torch.zeros(()))
        s1, s2 = d.sum(1), (d * d).sum(1)
        mm = s1 / n
        mean, m2 = k + mm, s2 - s1 * mm
    return torch.stack([n.expand_as(mean), mean, m2], -1).permute(1, 0, 2).contiguous()


def _silu(z):
    return z / (1 + torch.exp(-z))


def _dsilu(z):
    s = 1 / (1 + torch.exp(-z))
    return s * (1 + z * (1 - s))


def emu_bn(layout, dims, plan, x, gamma, beta, gout, eps, mom, rm, rv, act, residual=None, tail_4096=False, unshifted=False, rv_biased=False,
           rstd_unbiased=False, no_live=False, no_k2=False, dsilu_at_xhat=False, z_bf16=False, res_after_store=False):
    """The body of emu_bn_nchw / emu_bn_cl: one BatchNorm in either layout on rows [N, C] (layout 'nchw': dims = (B, HW), rows image-major), fp32
    arithmetic in the kernels' order: slice-wise two-pass | shift-by-first-row sums, the Chan combine, the apply with a = rstd gamma in one
    FMA, the backward from the stored mean and rstd with per-partial sums; bf16 rounding only at the stores.  Mutants: see the arguments."""
    st = bf if x.dtype == BF16 else (lambda t: t)
    N, C = x.shape
    xf, g = x.float(), gout.float()
    idx, mask, lens = _bn_gather(layout, dims, plan, N)
    got = emu_bn_finalize(_bn_partials(layout, xf, idx, mask, lens, tail_4096, unshifted), eps, mom, rm, rv, rv_biased, rstd_unbiased)
    mean, rstd = got['mean'], got['rstd']
    z = _fma(xf - mean, rstd * gamma, beta)
    if z_bf16:
        z = bf(z)
    y = _silu(z) if act else z
    if residual is not None:
        y = st(st(y) + residual.float()) if res_after_store else y + residual.float()
        got['dres'] = gout.clone()
    got['out'] = st(y)
    xh = (xf - mean) * rstd
    dz = g * (_dsilu(xh if dsilu_at_xhat else _fma(xh, gamma, beta)) if act else torch.ones(()))
    live = torch.ones_like(mask) if no_live else mask
    s1 = torch.where(live.unsqueeze(-1), dz[idx], torch.zeros(())).sum(1).sum(0)
    s2 = torch.where(live.unsqueeze(-1), (dz * xh)[idx], torch.zeros(())).sum(1).sum(0)
    inv = _f(1.0) / _f(float(N))
    got['dbeta'], got['dgamma'] = s1, s2
    got['dx'] = st(gamma * rstd * (dz - s1 * inv - (0 if no_k2 else xh * (s2 * inv))))
    return got


def emu_bn_nchw(B, HW, plan, *args, **mut):
    """tamtr_bn_act_fwd / _bwd on rows [B * HW, C] (image-major)."""
    return emu_bn('nchw', (B, HW), plan, *args, **mut)


def emu_bn_cl(plan, *args, **mut):
    """tamtr_bncl_act_fwd / _bwd on rows [N, C]."""
    return emu_bn('cl', None, plan, *args, **mut)


def emu_bn_pair(plan, x1, x2, p1, p2, gout, eps, mom, act, drop_beta2=False, swap_k=False):
    """tamtr_bncl2_act_*: both statistics as emu_bn, z = fma(x2 - m2, a2, fma(x1 - m1, a1, beta1 + beta2)).  Mutants: bn2's beta dropped;
    k2 and k3 exchanged in the backward."""
    st = bf if x1.dtype == BF16 else (lambda t: t)
    N, C = x1.shape
    idx, mask, lens = _bn_gather('cl', None, plan, N)
    got, s = {}, []
    for i, (x, p) in enumerate(((x1, p1), (x2, p2))):
        f = emu_bn_finalize(_bn_partials('cl', x.float(), idx, mask, lens), eps, mom, p[2], p[3])
        got.update({f'{n}{i + 1}': v for n, v in f.items()})
        s.append((x.float(), f['mean'], f['rstd'], p[0]))
    be = p1[1] if drop_beta2 else p1[1] + p2[1]
    (xa, ma, ra, ga), (xb, mb, rb, gb) = s
    z = _fma(xb - mb, rb * gb, _fma(xa - ma, ra * ga, be))
    got['out'] = st(_silu(z) if act else z)
    h1, h2 = (xa - ma) * ra, (xb - mb) * rb
    dz = gout.float() * (_dsilu(_fma(h2, gb, _fma(h1, ga, be))) if act else torch.ones(()))
    m = mask.unsqueeze(-1)
    sums = [torch.where(m, t[idx], torch.zeros(())).sum(1).sum(0) for t in (dz, dz * h1, dz * h2)]
    inv = _f(1.0) / _f(float(N))
    k1, k2, k3 = (t * inv for t in sums)
    if swap_k:
        k2, k3 = k3, k2
    got.update({'dbeta1': sums[0], 'dbeta2': sums[0], 'dgamma1': sums[1], 'dgamma2': sums[2],
                'dx1': st(ga * ra * (dz - k1 - h1 * k2)), 'dx2': st(gb * rb * (dz - k1 - h2 * k3))})
    return got


def _bn_case_inputs(layout, N, C, dt, kind, dims=None):
    bf16 = dt == BF16
    plan = K.nchw_plan(dims[0], C, dims[1], bf16) if layout == 'nchw' else K.cl_plan(N, C, bf16)
    home = K.home_row(layout, plan, N, *(dims or ()))
    x, g = K.bn_rows(N, C, dt, kind, 900 + N % 1000 + C, home)
    return plan, x, g, K.bn_params(C, 11 + C)


def _emu_single(layout, N, C, dt, kind, act, dims=None, residual=False, eps=1e-3, mom=0.03, tag='emu', **mut):
    plan, x, g, p = _bn_case_inputs(layout, N, C, dt, kind, dims)
    r = (0.5 * rnd((N, C), 300 + C)).to(dt) if residual else None
    args = (plan, x, p[0], p[1], g, eps, mom, p[2], p[3], act, r)
    got = emu_bn_nchw(*dims, *args, **mut) if layout == 'nchw' else emu_bn_cl(*args, **mut)
    xr, gr = (K.nchw(x, *dims), K.nchw(g, *dims)) if layout == 'nchw' else (x, g)
    K.bn_single_assert(f'{tag} bn[{layout},{K.dtn(dt)},{N}x{C},{kind},act={act}]', got, layout, plan, xr, p[0], p[1], gr, eps, mom, p[2], p[3], act, r)
    if kind == 'constant' and not mut:
        K.bn_constant_assert(tag, got, C, p[1], act, dt, eps)
    return got


def test_bn_cases_reach_the_branches_they_are_listed_for():
    """The dispatch of csrc/bn.hip as restated in tests/bn_cases.py, on every listed case."""
    assert K.reached() == K.REACH, K.reached() ^ K.REACH
    assert K.cl_plan(*K.CL_LARGE['S>256'][:0:-1], False)[4] == 257 and K.cl_plan(*K.CL_LARGE['iters=8'][:0:-1], False)[2:] == (8, 128, 641)
    assert K.cl_plan(K.CL_LARGE['iters=8'][2] - 6, 64, False)[2] == 4                      # one row less than 5 * 2^20 elements: still iters = 4
    assert K.cl_plan(1, 4, True)[:2] == (4, 1) and K.cl_plan(1, 8, True)[:2] == (8, 1) and K.cl_plan(1, 1024, False)[1] == 256
    for dt, C in K.SEG_CASES:                                                              # an image boundary inside a chunk and inside a piece
        V, cg, iters, chunk_rows, S = K.cl_plan(K.SEG_B * K.SEG_LS[0], C, dt == 'bf16')
        assert any(L % chunk_rows and L % (256 * V // C) for L in K.SEG_LS)
    assert all((B * HW) & (B * HW - 1) == 0 for B, C, HW, k in K.NCHW_KIND_CASES if k == 'constant')


@pytest.mark.parametrize('dt', ('fp32', 'bf16'))
def test_bn_nchw_emulation_passes_every_case(dt):
    for B, C, HW in K.NCHW_SHAPES:
        for act in (0, 1):
            for eps, mom in K.EPS_MOM:
                _emu_single('nchw', B * HW, C, K.DT[dt], 'ordinary', act, (B, HW), eps=eps, mom=mom)
    for B, C, HW, kind in K.NCHW_KIND_CASES:
        for act in (0, 1):
            _emu_single('nchw', B * HW, C, K.DT[dt], kind, act, (B, HW))


@pytest.mark.parametrize('dt', ('fp32', 'bf16'))
def test_bn_channels_last_emulation_passes_every_case(dt):
    for C in K.CL_C[dt]:
        for N in K.cl_rows(C, dt == 'bf16').values():
            for act, residual, _ in K.CL_VARIANTS[:3]:                  # (a strided gy is the same arithmetic)
                _emu_single('cl', N, C, K.DT[dt], 'ordinary', act, residual=residual)
            _emu_single('cl', N, C, K.DT[dt], 'ordinary', 1, eps=1e-5, mom=0.1)
    for inst, C in K.CL_KIND_C.items():
        if inst.startswith(dt):
            for kind in K.KINDS[1:]:
                N = K.cl_rows(C, dt == 'bf16')['chunk' if kind == 'constant' else 'inside']
                for act in (0, 1):
                    _emu_single('cl', N, C, K.DT[dt], kind, act, residual=act == 1 and kind != 'constant')


@pytest.mark.parametrize('case', list(K.CL_LARGE))
def test_bn_channels_last_emulation_passes_the_long_chains(case):
    """Both large cases at full size (S = 257 and iters = 8 with S = 641): the emulation is vectorised over the chunks."""
    dt, C, N = K.CL_LARGE[case]
    _emu_single('cl', N, C, K.DT[dt], 'ordinary', 1)


def test_bn_pair_segment_and_statistics_emulations_pass():
    eps, mom = 1e-3, 0.03
    for dt, C, rows_, _ in K.PAIR_CASES:
        N = K.cl_rows(C, dt == 'bf16')[rows_]
        plan = K.cl_plan(N, C, dt == 'bf16')
        x1, g = K.bn_rows(N, C, K.DT[dt], 'ordinary', 400 + C)
        x2 = (1.3 * rnd((N, C), 401 + C) - 0.7).to(K.DT[dt])
        p1, p2 = K.bn_params(C, 21 + C), K.bn_params(C, 31 + C)
        K.bn_pair_assert(f'emu bn2[{dt},{N}x{C}]', emu_bn_pair(plan, x1, x2, p1, p2, g, eps, mom, 1), plan, x1, x2, p1, p2, g, eps, mom, 1)
    for dt, C in K.SEG_CASES:
        _emu_segments(dt, C, False)
    for S in K.FINALIZE_S:
        for empty in ((), (0,), (S // 2,)) if S > 1 else ((),):
            part, data, counts = K.finalize_partials(S, 3, empty)
            _, _, rm, rv = K.bn_params(3, 50)
            K.finalize_assert(f'emu bn_finalize[S={S},empty={empty}]', emu_bn_finalize(part, eps, mom, rm, rv), S, counts, data, eps, mom, rm, rv)
    # the parent's loop (no guard): an empty first triple divides 0 by 0
    n, mean, m2 = (torch.zeros(3) for _ in range(3))
    assert bool(torch.isnan(mean + (mean - mean) * (n / (n + n))).all())
    for dt in K.CL_C:
        for C in K.CL_C[dt]:
            for N in K.cl_rows(C, dt == 'bf16').values():
                for kind in ('ordinary', 'offset'):
                    plan = K.cl_plan(N, C, dt == 'bf16')
                    x, _ = K.bn_rows(N, C, K.DT[dt], kind, 600 + C + N % 1000)
                    p = K.bn_params(C, 11 + C)
                    idx, mask, lens = _bn_gather('cl', None, plan, N)
                    got = emu_bn_finalize(_bn_partials('cl', x.float(), idx, mask, lens), eps, mom, p[2], p[3])
                    K.stats_assert(f'emu bn_stats[{dt},{N}x{C},{kind}]', got, 'cl', plan, x, eps, mom, p[2], p[3])


def _emu_segments(dt, C, wrong_pitch):
    """ops.bn_cat_cl: every level's BatchNorm written into its segment of the [B, sum L, C] token memory.  Mutant: image b of a level
    placed at b * seg_rows * C instead of b * seg_pitch."""
    B, Ls, eps, mom = K.SEG_B, K.SEG_LS, 1e-5, 0.1
    Lt = sum(Ls)
    feats = torch.zeros(B * Lt * C, dtype=K.DT[dt])
    ins = [K.bn_rows(B * L, C, K.DT[dt], 'ordinary', 500 + L + C) for L in Ls]
    ps = [K.bn_params(C, 41 + i + C) for i in range(len(Ls))]
    gots, at = [], 0
    for (x, g), p, L in zip(ins, ps, Ls):
        plan = K.cl_plan(B * L, C, dt == 'bf16')
        got = emu_bn_cl(plan, x, p[0], p[1], g, eps, mom, p[2], p[3], 0)
        for b in range(B):
            o = at * C + b * (L * C if wrong_pitch else Lt * C)
            feats[o:o + L * C] = got['out'][b * L:(b + 1) * L].reshape(-1)
        gots.append((got, plan))
        at += L
    at = 0
    for (got, plan), (x, g), p, L in zip(gots, ins, ps, Ls):
        got = dict(got, out=feats.view(B, Lt, C)[:, at:at + L].reshape(B * L, C))
        del got['mean'], got['rstd']
        K.bn_single_assert(f'emu bn_seg[{dt},C={C},{B}x{L}]', got, 'cl', plan, x, p[0], p[1], g, eps, mom, p[2], p[3], 0)
        at += L


def _old_bn_ok(got, ref, dt, N):
    """The rule of tests/test_gpu_ops.py (test_bn_act_vs_torch and its siblings): out 2e-2 (bf16) | 2e-5 (fp32) relative and absolute, ten
    times that on dx, dgamma and dbeta with sqrt(N) times the absolute term, the running statistics 1e-5 / 1e-6."""
    tol = 2e-2 if dt == BF16 else 2e-5
    rule = {'out': (tol, tol), 'dx': (10 * tol, 10 * tol), 'dgamma': (10 * tol, 10 * tol * N ** 0.5), 'dbeta': (10 * tol, 10 * tol * N ** 0.5),
            'running_mean': (1e-5, 1e-6), 'running_var': (1e-5, 1e-6), 'dres': (tol, tol)}
    return all(R.old_close(t.float(), ref[n][0], *rule[n.rstrip('12')]) for n, t in got.items() if n.rstrip('12') in rule)


def test_bn_mutants_fail():
    """Every mutant misses a counted bound on at least one case; whether the old rule of tests/test_gpu_ops.py accepts it is recorded in
    the mutant table (profiles/r18_bn_ref64.txt)."""
    def single(name, layout, N, C, dt, kind, act, dims=None, residual=False, **mut):
        plan, x, g, p = _bn_case_inputs(layout, N, C, dt, kind, dims)
        r = (0.5 * rnd((N, C), 300 + C)).to(dt) if residual else None
        xr, gr = (K.nchw(x, *dims), K.nchw(g, *dims)) if layout == 'nchw' else (x, g)
        ref = R.batch_norm(xr, p[0], p[1], gr, 1e-3, 0.03, p[2], p[3], act, r, chunk_rows=plan[3] if layout == 'cl' else None)
        assert _old_bn_ok(emu_bn(layout, dims, plan, x, p[0], p[1], g, 1e-3, 0.03, p[2], p[3], act, r), ref, dt, N)
        old = _old_bn_ok(emu_bn(layout, dims, plan, x, p[0], p[1], g, 1e-3, 0.03, p[2], p[3], act, r, **mut), ref, dt, N)
        new = _new_rule(lambda: _emu_single(layout, N, C, dt, kind, act, dims, residual, tag='mutant', **mut))
        MUTANT_TABLE.append(('bn', f'{name} [{layout},{K.dtn(dt)},{N}x{C},{kind}]', old, new))
        assert not new, name
        return old
    n64 = K.cl_rows(64, False)
    n256 = K.cl_rows(256, True)
    single('running variance updated with the biased variance', 'nchw', 128, 3, K.F32, 'ordinary', 0, (2, 64), rv_biased=True)
    single('running variance updated with the biased variance', 'cl', n256['inside'], 256, BF16, 'ordinary', 0, rv_biased=True)
    single('rstd from the unbiased variance', 'nchw', 128, 3, BF16, 'ordinary', 1, (2, 64), rstd_unbiased=True)
    single('rstd from the unbiased variance', 'cl', n64['inside'], 64, K.F32, 'ordinary', 1, rstd_unbiased=True)
    single('NCHW tail slice counted as 4096 elements', 'nchw', 4100, 2, BF16, 'ordinary', 1, (1, 4100), tail_4096=True)
    single('channels-last statistics as unshifted E[x^2] - E[x]^2', 'cl', n64['chunk'], 64, K.F32, 'offset', 0, unshifted=True)
    single('backward reduce without the live mask', 'cl', n256['inside'], 256, BF16, 'ordinary', 1, no_live=True)
    single('backward reduce without the live mask', 'cl', n64['inside'], 64, K.F32, 'ordinary', 1, no_live=True)
    single('dx without the xhat k2 term', 'cl', n256['inside'], 256, BF16, 'ordinary', 1, no_k2=True)
    single('dx without the xhat k2 term', 'nchw', 8200 * 2, 2, BF16, 'ordinary', 1, (2, 8200), no_k2=True)
    single('SiLU\' taken at xhat', 'cl', n256['inside'], 256, BF16, 'ordinary', 1, dsilu_at_xhat=True)
    old = single('z rounded to bf16 before the activation', 'cl', n256['inside'], 256, BF16, 'ordinary', 1, z_bf16=True)
    assert old, 'the old rule was expected to accept a double rounding'
    single('residual added after the bf16 store', 'cl', n256['inside'], 256, BF16, 'ordinary', 1, residual=True, res_after_store=True)
    # the pair
    dt, C = BF16, 256
    N = n256['inside']
    plan = K.cl_plan(N, C, True)
    x1, g = K.bn_rows(N, C, dt, 'ordinary', 400 + C)
    x2 = (1.3 * rnd((N, C), 401 + C) - 0.7).to(dt)
    p1, p2 = K.bn_params(C, 21 + C), K.bn_params(C, 31 + C)
    ref = R.batch_norm_pair(x1, x2, p1[0], p1[1], p2[0], p2[1], g, 1e-3, 0.03, p1[2], p1[3], p2[2], p2[3], 1, chunk_rows=plan[3])
    for name, mut in (('pair with bn2\'s beta dropped', {'drop_beta2': True}), ('pair with k2 and k3 exchanged', {'swap_k': True})):
        m = emu_bn_pair(plan, x1, x2, p1, p2, g, 1e-3, 0.03, 1, **mut)
        new = _new_rule(lambda: K.bn_pair_assert('mutant', m, plan, x1, x2, p1, p2, g, 1e-3, 0.03, 1))
        MUTANT_TABLE.append(('bn', f'{name} [bf16,{N}x{C}]', _old_bn_ok(m, ref, dt, N), new))
        assert not new, name
    # the segments
    for dt_, C_ in K.SEG_CASES:
        new = _new_rule(lambda: _emu_segments(dt_, C_, True))
        MUTANT_TABLE.append(('bn', f'segment b at b * seg_rows * C [{dt_},C={C_}]', False, new))      # (the old test compares bits with ops.bn_act)
        assert not new
    _report_mutants('bn')


# ------------------------------------------------------------------------------------------------ loss terms, matcher cost, box refinement, optimizer
import loss_cases as LC

HOST_LIMIT = 0.5      # the fp32 torch form alone may use half of every bound: the rest is for the device's math functions


def _grid(t):
    return torch.tensor(t, dtype=torch.float64) * LC.U


def _all_family_pairs():
    """Every pair of every family in its four mirrorings (family_pair's layers 0 .. 3), fp64."""
    fams, a, b = zip(*[LC.family_pair(j, l) for j in range(len(LC.PAIRS)) for l in range(4)])
    return fams, _grid(a), _grid(b)


def test_riou_reference_is_float64_autograd_of_bbox_iou_on_every_family():
    """ref64.riou_parts - the plain formulas that csrc/detrloss.hip also states - against float64 autograd of tam-tr_amd/loss.py bbox_iou,
    which the CPU suite pins on the reference project's fixtures: values, and the gradient with its tie, clamp and NaN rules, on every
    family and mirroring.  (bbox_iou's constants in double: eps = 1e-7, 1 + eps.)"""
    import tamtr_amd.loss as LS
    fams, a, b = _all_family_pairs()
    ar = a.clone().requires_grad_()
    loss = 1 - LS.bbox_iou(ar, b, xywh=True, RIOU=True).squeeze(-1)
    loss.sum().backward()
    rp = R.riou_parts(a, b, eps=1e-7, one_eps=1 + 1e-7)
    assert torch.allclose(rp['loss'], loss.detach(), rtol=1e-13, atol=0)
    assert torch.allclose(rp['iou'], LS.bbox_iou(a, b, xywh=True).squeeze(-1), rtol=1e-13, atol=0)
    nan = torch.isnan(ar.grad)
    same = torch.tensor([f == 'same_centre' for f in fams])
    assert torch.equal(nan, same.unsqueeze(-1).expand(-1, 4)), 'coincident centres, and only they, give four NaN components'
    assert torch.equal(torch.isnan(rp['grad']), nan)
    err = (rp['grad'] - ar.grad).abs()[~nan]
    assert bool((err <= 1e-12 * rp['m_grad'][~nan]).all()), float((err / rp['m_grad'][~nan]).max())
    assert bool((rp['m_grad'][~nan] >= rp['grad'][~nan].abs() * (1 - 1e-12)).all()), 'a magnitude is at least the value'
    # the families have what their names say
    ax1, ax2 = a[:, 0] - a[:, 2] / 2, a[:, 0] + a[:, 2] / 2
    bx1, bx2 = b[:, 0] - b[:, 2] / 2, b[:, 0] + b[:, 2] / 2
    ixr = torch.minimum(ax2, bx2) - torch.maximum(ax1, bx1)
    iyr = torch.minimum(a[:, 1] + a[:, 3] / 2, b[:, 1] + b[:, 3] / 2) - torch.maximum(a[:, 1] - a[:, 3] / 2, b[:, 1] - b[:, 3] / 2)
    for i, f in enumerate(fams):
        if f in ('disjoint_x', 'disjoint_xy'):
            assert ixr[i] < 0
        if f in ('disjoint_y', 'disjoint_xy'):
            assert iyr[i] < 0
        if f == 'touching':
            assert (ixr[i] == 0) != (iyr[i] == 0) and rp['iou'][i] == 0
        if f in ('tie_left', 'tie_right'):
            assert (ax1[i] == bx1[i]) != (ax2[i] == bx2[i]) and a[i, 1] != b[i, 1]
        if f == 'identical_shape_shifted':
            assert torch.equal(a[i, 2:], b[i, 2:])
    assert any((ixr[i] == 0) for i, f in enumerate(fams) if f == 'touching') and any((iyr[i] == 0) for i, f in enumerate(fams) if f == 'touching')


@pytest.mark.parametrize('c', LC.CASES, ids=LC.case_id)
def test_loss_torch_form_meets_every_bound_at_half(c):
    """The fp32 torch form of tam-tr_amd/loss.py on the CPU - the three terms and both gradients, and the matcher's cost with three diverged
    predictions - against detr_terms / detr_match_cost on the very inputs of tests/test_gpu_loss_ref64.py: no ratio above 0.5, on every
    family, the NaN rows checked as NaN rows."""
    case, _ = LC.terms_ref(c)
    got = LC.terms_of(LC.torch_form, case)
    LC.assert_terms('host', c, got, limit=HOST_LIMIT)
    for nonfinite in (False, True):
        cc = LC.cost_case(c, nonfinite)
        C = LC.cost_torch_form(cc)
        LC.assert_cost('host' + (' nonfinite' if nonfinite else ''), c, cc, C, limit=HOST_LIMIT)
        if nonfinite:
            assert bool((C[0, 0, [1, 3, 4]] == 0).all()) and int((C == 0).sum()) == 3 * C.shape[-1]


def test_loss_references_on_the_generic_families_in_float64():
    """detr_terms against a float64 restatement of DETRLoss._layers' torch form (the same expressions without its .float() casts) on the
    generic families: the wiring of the reference - pair lists, tables, the three sums, the upstream gradients - apart from the box
    formulas, which the bbox_iou test holds."""
    import torch.nn.functional as F
    import tamtr_amd.loss as LS
    c = (4, 3, 171, 80, [40, 0, 25], False)
    case = LC.make_case(*c, only=LC.GENERIC)
    Lr, B, nq, nc = case['shape']
    n = case['n']
    pb, ps = case['pb'].double().requires_grad_(), case['ps'].double().requires_grad_()
    gtb, li, bi, si, gi = case['gtb'].double(), case['li'], case['bi'], case['si'], case['gi']
    p_sel, g_sel = pb[li, bi, si], gtb[gi]
    tg = torch.full((Lr, B, nq), nc)
    tg[li, bi, si] = case['gtc'][gi]
    sc = torch.zeros(Lr, B, nq, dtype=torch.float64)
    sc[li, bi, si] = LS.bbox_iou(p_sel.detach(), g_sel, eps=R.DL_EPS).squeeze(-1)
    one_hot = F.one_hot(tg, nc + 1)[..., :-1]
    score = sc.unsqueeze(-1) * one_hot
    w = 0.75 * ps.sigmoid().pow(2.0) * (1 - one_hot) + score * one_hot
    l_cls = (F.binary_cross_entropy_with_logits(ps, score, reduction='none') * w).mean(2).sum((1, 2)) / (n / nq) * LC.GAINS_LOSS[0]
    l_box = LC.GAINS_LOSS[1] * (p_sel - g_sel).abs().view(Lr, n, 4).sum((1, 2)) / n
    rp = R.riou_parts(p_sel, g_sel)
    l_iou = LC.GAINS_LOSS[2] * rp['loss'].view(Lr, n).sum(1) / n
    gpb_cls_box, gps = torch.autograd.grad((torch.stack([l_cls, l_box]) * case['up'][:2].double()).sum(), [pb, ps])
    gpb = gpb_cls_box.clone()
    gpb[li, bi, si] += (case['up'][2].double() * LC.GAINS_LOSS[2] / n)[li].unsqueeze(-1) * rp['grad']
    ref = R.detr_terms(case['pb'], case['ps'], case['gtb'], case['gtc'], li, bi, si, gi, n, LC.GAINS_LOSS, case['up'])
    for k, t in (('class', l_cls), ('bbox', l_box), ('giou', l_iou), ('dpb', gpb), ('dps', gps)):
        R.check(f'fp64 {k}', t.detach(), ref[k][0], ref[k][1], 0, 1e-12, log=False)


@pytest.mark.parametrize('ddt', [torch.float32, torch.bfloat16])
def test_box_refine_torch_formula_meets_every_bound_at_half(ddt):
    ref, delta, cot = LC.refine_inputs(ddt)
    d, r = delta.float().clone().requires_grad_(), ref.clone().requires_grad_()
    y = LC.refine_torch_form(d, r)
    (y * cot).sum().backward()
    w = LC.assert_refine('host', ddt, ref, delta, cot, y.detach(), d.grad.to(ddt), r.grad)
    assert w['y'] <= HOST_LIMIT and w['gr'] <= HOST_LIMIT and (w['gd'] <= HOST_LIMIT or ddt == torch.bfloat16)     # (bf16: the one rounding of the store is the bound)
    # float64 autograd of the same formula is the reference
    d64, r64 = delta.double().requires_grad_(), ref.double().requires_grad_()
    x = r64.clamp(min=0, max=1)
    y64 = torch.sigmoid(d64 + torch.log(x.clamp(min=R.REF_EPS) / (1 - x).clamp(min=R.REF_EPS)))
    (y64 * cot.double()).sum().backward()
    want = R.box_refine(delta, ref, cot)
    for k, t in (('y', y64.detach()), ('gd', d64.grad), ('gr', r64.grad)):
        R.check(f'fp64 {k}', t, want[k][0], want[k][1], 0, 1e-12, log=False)


@pytest.mark.parametrize('c', LC.OPT_CASES, ids=LC.opt_case_id)
def test_optim_torch_form_meets_every_bound_at_half(c):
    """clip_grad_norm_ + torch.optim.AdamW + ModelEMA in fp32 on the CPU, from the fp32 constants the C ABI receives, against optim_step:
    one step of every case of tests/test_gpu_loss_ref64.py, no ratio above 0.5."""
    tensors, before, got, _ = LC.optim_run(c, LC.torch_stepper, abi_consts=True)
    LC.assert_optim('host', c, tensors, before, got, limit=HOST_LIMIT)


def test_optim_reference_follows_a_float64_twin_over_three_steps():
    """optim_step chained over three steps against torch.optim.AdamW + clip_grad_norm_ + ModelEMA on a float64 twin, with constants that
    are exact in fp32 and in double alike, so that torch's double scalars are the reference's: 1e-11 of the magnitudes."""
    from tamtr_amd.engine import ModelEMA
    c = (9, 'clipped', 100, False)
    groups = ((2.0 ** -7, 0.0), (2.0 ** -9, 2.0 ** -3), (2.0 ** -11, 2.0 ** -4))
    betas, eps, max_norm = (R.f32(0.9), R.f32(0.999)), R.f32(1e-8), R.f32(0.1)
    tensors = LC.opt_tensors(c[0], c[1])
    names = list(tensors)
    net = LC.opt_module(tensors, 'cpu', torch.float64)
    opt = LC.opt_optimizer(net, tensors, c[0], groups, betas, eps)
    ema = ModelEMA(net, updates=99)
    ema.decay = lambda x: R.f32(LC.ema_decay(x))
    lr = [groups[tensors[n][0]][0] if tensors[n][0] is not None else 0.0 for n in names]
    wd = [groups[tensors[n][0]][1] if tensors[n][0] is not None else 0.0 for n in names]
    state = {n: [t[1].double(), t[3], t[4], t[1].double(), float(c[0])] for n, t in tensors.items()}      # p, m, v, e, step
    g = torch.Generator().manual_seed(3)
    for it in range(3):
        grads = {n: (None if t[2] is None or (n == 'w3' and it == 1) else torch.randn(t[1].shape, generator=g, dtype=torch.float64) * (0.01 if it == 2 else 1.0))
                 for n, t in tensors.items()}
        for n in names:
            if tensors[n][0] is not None:
                getattr(net, n).grad = None if grads[n] is None else grads[n].clone()
        LC.torch_stepper(net, opt, ema, max_norm)
        ref = R.optim_step([state[n][0] for n in names], [grads[n] for n in names], [state[n][1] for n in names], [state[n][2] for n in names],
                           [state[n][3] for n in names], [state[n][4] for n in names], lr, wd, *betas, eps, max_norm, LC.ema_decay(100 + it))
        esd = ema.ema.state_dict()
        for i, n in enumerate(names):
            q = getattr(net, n)
            R.check(f'step {it} p {n}', q.detach(), ref['p'][i][0], ref['p'][i][1] + ref['p'][i][0].abs(), 0, 1e-11, log=False)
            R.check(f'step {it} e {n}', esd[n], ref['e'][i][0], ref['e'][i][1], 0, 1e-11, log=False)
            state[n][0], state[n][3], state[n][4] = ref['p'][i][0], ref['e'][i][0], ref['step'][i]
            if ref['m'][i] is not None:
                st = opt.state[q]
                R.check(f'step {it} m {n}', st['exp_avg'], ref['m'][i][0], ref['m'][i][1], 0, 1e-11, log=False)
                R.check(f'step {it} v {n}', st['exp_avg_sq'], ref['v'][i][0], ref['v'][i][1], 0, 1e-11, log=False)
                R.check(f'step {it} clipped gradient {n}', q.grad, ref['gc'][i][0], ref['gc'][i][1], 0, 1e-11, log=False)
                assert float(st['step']) == ref['step'][i]
                state[n][1], state[n][2] = ref['m'][i][0], ref['v'][i][0]
    assert state['w3'][4] == c[0] + 2 and state['nograd'][4] == c[0] and state['w1'][4] == c[0] + 3


def _fails(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


def test_loss_and_optimizer_mistakes_miss_their_bounds():
    """Each mistake that the kernels could hold - stated in the reference formulas, whose output then stands in for the kernel's - misses a
    bound on the inputs of tests/test_gpu_loss_ref64.py; the same inputs pass unmutated (the tests above).  Which check catches which
    mistake is listed in profiles/loss_optim_ref64.txt."""
    c = LC.CASES[1]                                       # Lr 1, 255 pairs: every family
    case, _ = LC.terms_ref(c)
    caught = {}
    for mut in ('tie0', 'tie1', 'cx_gt', 'dm1_swap', 'dw075'):
        _, bad = LC.terms_ref(c, (mut,))
        got = {k: v[0] for k, v in bad.items()}
        hit = [k for k in ('class', 'bbox', 'giou', 'dpb', 'dps') if _fails(lambda: R.check(k, got[k], LC.terms_ref(c)[1][k][0], LC.terms_ref(c)[1][k][1], 0,
                                                                                               R.detr_bounds(1, 256, 7, 255)[k], log=False))]
        caught[mut] = hit
        assert hit == (['dps'] if mut == 'dw075' else ['dpb']), (mut, hit)
        assert _fails(lambda: LC.assert_terms('mutant', c, got))
    # which families see which mistake: the rows of d/d(pb) that move
    ref = LC.terms_ref(c)[1]['dpb'][0]
    for mut, fams in (('tie0', {'tie_left', 'tie_right', 'tie_top', 'tie_bottom', 'tie_all_but_centre', 'square_pred', 'tiny'}), ('cx_gt', {'touching'})):
        moved = (torch.nan_to_num(LC.terms_ref(c, (mut,))[1]['dpb'][0] - ref).abs().sum(-1) > 0)[case['li'], case['bi'], case['si']]
        assert {f for f, m in zip(case['families'], moved.tolist()) if m} == fams, mut
    # the optimizer: the decay dropped; the scalar tail after the last quad skipped (those elements keep their old values)
    oc = LC.OPT_CASES[1]
    tensors, before, got, _ = LC.optim_run(oc, LC.torch_stepper, abi_consts=True)
    LC.assert_optim('host', oc, tensors, before, got)
    assert _fails(lambda: LC.assert_optim('mutant', oc, tensors, before, got, mut=('no_wd',))), 'a reference without the decay must not accept a step with it'
    for name in ('w3', 'w8193', 'w1'):
        n4 = tensors[name][1].numel() // 4 * 4
        bad = {k: (dict(v) if isinstance(v, dict) else v) for k, v in got.items()}
        p = got[name]['p'].clone()
        p[n4:] = tensors[name][1][n4:]
        bad[name]['p'] = p
        assert _fails(lambda: LC.assert_optim('mutant', oc, tensors, before, bad)), name
