"""bf16 hot-path kernels against fp64 references with an error model (tests/ref64.py): the contrastive head, the decoder self-attention,
the deformable-attention core and ln_gate, at the bench's shapes and on every branch their host dispatch can select.

Each assertion is elementwise |got - ref| <= a 2^-8 |ref| + b mag, with no free absolute term; see tests/ref64.py for what a and b
cover.  Set TAMTR_REF64_REPORT=<file> to collect the worst err / bound ratio of every assertion."""
import math

import pytest
import torch

import ref64 as R
from weights import rnd, urnd

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import tamtr_amd.ops as ops
    return ops


def dev(t):
    return t.detach().cuda()


# ------------------------------------------------------------------------------------------------ contrastive head
# (B, Q, K, C): np = passes over C per lane (bf16: C <= 512, 1024, 2048, 4096), REGS = K <= 16 and np <= 2, Q tails against CT_ROWS = 16
# (forward) and CT_BROWS = 80 (backward), K > 16 = the LDS-atomic backward
CONTRASTIVE = {
    'bench': (16, 292, 10, 512),
    'np2_regs_k1': (2, 81, 1, 1024),
    'np2_regs_q1': (2, 1, 16, 1024),
    'np2_atomic_k17': (2, 81, 17, 600),
    'np4_fwd_lds_90k': (1, 81, 11, 2048),
    'np4': (1, 292, 7, 2048),
    'np8': (1, 81, 3, 4096),
    'np1_atomic_k128': (2, 81, 128, 64),
}


@pytest.mark.parametrize('case', list(CONTRASTIVE))
def test_contrastive_bf16_vs_fp64(ops, case):
    B, Q, K, C = CONTRASTIVE[case]
    x = rnd((B, Q, C), 1, 2.0).bfloat16()
    w = rnd((B, K, C), 2)
    x[0, 0] = 0      # the eps clamp of both norms
    w[0, 0] = 0
    ls, bi = torch.tensor(math.log(1 / 0.07)), torch.tensor([-10.0])
    g = rnd((B, Q, K), 3, 0.05)
    ref = R.contrastive(x, w, ls, bi, g)
    xd, wd = dev(x).requires_grad_(), dev(w).requires_grad_()
    out = ops.contrastive_logits(xd, wd, dev(ls), dev(bi))
    n = C // 64 + 16
    R.check(f'contrastive[{case}] logits', out, *ref['logits'], 0, R.fp32_b(n))
    if (2 * K * C + K) * 4 > 128 * 1024:
        return   # forward-only shape: more LDS than the backward may use (96 KiB forward, 128 KiB backward)
    out.backward(dev(g))
    R.check(f'contrastive[{case}] dx', xd.grad.float(), *ref['dx'], 1, R.fp32_b(K + n))
    R.check(f'contrastive[{case}] dw', wd.grad, *ref['dw'], 0, R.fp32_b(Q // 4 + 2 * n + 16))


# ------------------------------------------------------------------------------------------------ self-attention
def _runs_mask(Q, seed):
    """Blocked runs of random length and phase per row, crossing the 32-bit mask words; the diagonal stays open."""
    g = torch.Generator().manual_seed(seed)
    j = torch.arange(Q)
    run = torch.randint(5, 70, (Q, 1), generator=g)
    ph = torch.randint(0, 97, (Q, 1), generator=g)
    m = ((j[None] + ph) // run) % 2 == 0
    m[j, j] = False
    return m


def _attn_case(name):
    from tamtr_amd.loss import _dn_attn_mask
    c = {'bench_dn16': (16, 292, 8, 64, _dn_attn_mask(192, 100, 8, 12, 'cpu')),     # group edges at multiples of 16
         'dn10': (2, 292, 2, 64, _dn_attn_mask(100, 192, 5, 10, 'cpu')),           # group edges at multiples of 10
         'q1': (2, 1, 2, 64, None),
         'q31_runs': (2, 31, 2, 64, _runs_mask(31, 1)),
         'q32': (2, 32, 2, 64, None),
         'q33_runs': (2, 33, 2, 64, _runs_mask(33, 2)),
         'q292_runs': (1, 292, 2, 64, _runs_mask(292, 3)),
         'q4096': (1, 4096, 1, 64, None),
         'scalar64_unaligned': (2, 77, 2, 64, _runs_mask(77, 4)),
         'scalar32': (2, 77, 4, 32, _runs_mask(77, 5))}
    return c[name]


ATTN = ['bench_dn16', 'dn10', 'q1', 'q31_runs', 'q32', 'q33_runs', 'q292_runs', 'q4096', 'scalar64_unaligned', 'scalar32']


def _packed(B, Q, C, offset, seed):
    """bf16 [B, Q, 3C] packed projection (what modules.py hands the kernel as three column views), `offset` elements into its buffer."""
    buf = torch.zeros(offset + B * Q * 3 * C, dtype=torch.bfloat16, device='cuda')
    p = buf[offset:].view(B, Q, 3 * C)
    p.copy_(rnd((B, Q, 3 * C), seed).bfloat16())
    return p


def _attn_run(ops, B, Q, nh, dh, mask, offset):
    C = nh * dh
    p = _packed(B, Q, C, offset, 1)
    q, k, v = p[..., :C], p[..., C:2 * C], p[..., 2 * C:]
    go = rnd((B, Q, C), 2).bfloat16()
    ref = R.attention(q, k, v, nh, mask, go)
    p.requires_grad_()
    q, k, v = p[..., :C], p[..., C:2 * C], p[..., 2 * C:]
    out = ops.self_attention(q, k, v, nh, None if mask is None else dev(mask))
    out.backward(dev(go))
    gq, gk, gv = p.grad[..., :C], p.grad[..., C:2 * C], p.grad[..., 2 * C:]
    qd, kd = R._d(p[..., :C]).view(B, Q, nh, dh), R._d(p[..., C:2 * C]).view(B, Q, nh, dh)
    S = float(torch.einsum('bihc,bjhc->bhij', qd.abs(), kd.abs()).max()) * dh ** -0.5   # largest |s| the fp32 products can reach
    return out, (gq, gk, gv), ref, S


@pytest.mark.parametrize('case', ATTN)
def test_self_attention_bf16_vs_fp64(ops, case):
    B, Q, nh, dh, mask = _attn_case(case)
    scalar = case.startswith('scalar')
    # scalar64_unaligned: the packed buffer starts 8 bytes past a 16-byte boundary, so the <bf16, 64> scalar kernels serve it
    out, (gq, gk, gv), ref, S = _attn_run(ops, B, Q, nh, dh, mask, 4 if case == 'scalar64_unaligned' else 0)
    fp = R.fp32_b(2 * 64 * S + 2 * Q + 64)          # fp32 products / sums, and exp() of the scores' fp32 error
    p_rnd = 0 if scalar else R.U8                   # P packed to bf16 (MFMA)
    ds_rnd = 0 if scalar else R.U8                  # dS packed to bf16 (MFMA)
    dl_rnd = R.U8                                   # delta_i from the stored bf16 O (both paths)
    R.check(f'attn[{case}] o', out.float(), *ref['o'], 1, p_rnd + fp)
    R.check(f'attn[{case}] dq', gq.float(), *ref['dq'], 1, ds_rnd + dl_rnd + fp)
    R.check(f'attn[{case}] dk', gk.float(), *ref['dk'], 1, ds_rnd + dl_rnd + fp)
    R.check(f'attn[{case}] dv', gv.float(), *ref['dv'], 1, p_rnd + fp)


def test_self_attention_fully_masked_row_is_nan(ops):
    """A query that may attend to nothing: the reference softmax gives 0/0, and the kernel keeps that (selfattn.hip: 'a fully masked row
    gives NaN like the reference softmax').  Pinned: that output row and its dq row are NaN, every dk is NaN (delta of that row is NaN, as
    in the reference), dv treats the row's P as 0, and every other value is held to the fp64 bound."""
    B, Q, nh = 2, 45, 2
    mask = _runs_mask(Q, 6)
    mask[7] = True
    out, (gq, gk, gv), ref, S = _attn_run(ops, B, Q, nh, 64, mask, 0)
    assert bool(torch.isnan(out[:, 7]).all()) and bool(torch.isnan(gq[:, 7]).all()) and bool(torch.isnan(gk).all())
    fp = R.fp32_b(2 * 64 * S + 2 * Q + 64)
    R.check('attn[masked_row] o', out.float(), *ref['o'], 1, R.U8 + fp)
    R.check('attn[masked_row] dq', gq.float(), *ref['dq'], 1, 2 * R.U8 + fp)
    R.check('attn[masked_row] dk', gk.float(), *ref['dk'], 1, 2 * R.U8 + fp)
    R.check('attn[masked_row] dv', gv.float(), *ref['dv'], 1, R.U8 + fp)


# ------------------------------------------------------------------------------------------------ deformable core
SMALL_LEVELS = [(6, 5), (3, 4), (1, 7), (5, 1)]     # non-square, H = 1, W = 1


def _msda_inputs(B, Q, M, D, shapes, P, seed, lo=-0.1, hi=1.1):
    L, nl = sum(h * w for h, w in shapes), len(shapes)
    value = rnd((B, L, M, D), seed).bfloat16()
    loc = urnd((B, Q, M, nl, P, 2), seed + 1, lo, hi)
    aw = torch.softmax(rnd((B, Q, M, nl * P), seed + 2), -1).view(B, Q, M, nl, P)
    gout = rnd((B, Q, M * D), seed + 3).bfloat16()
    return value, loc, aw, gout


def _msda_edges(loc, shapes):
    """Samples on pixel centres, at loc = 0 and 1, and 48 queries piled on one point (long sorted runs)."""
    B, Q, M, nl, P, _ = loc.shape
    for l, (H, W) in enumerate(shapes):
        n = min(Q, 8)
        loc[:, :n, :, l, 0, 0] = (torch.arange(n) % W + 0.5).view(1, n, 1) / W
        loc[:, :n, :, l, 0, 1] = (torch.arange(n) % H + 0.5).view(1, n, 1) / H
        if P > 1:
            loc[:, :n, :, l, 1, 0] = (torch.arange(n) % 2).float().view(1, n, 1)
            loc[:, :n, :, l, 1, 1] = ((torch.arange(n) // 2) % 2).float().view(1, n, 1)
    if Q >= 56:
        loc[:, 8:56, :, :, -1] = torch.tensor([0.37, 0.61])
    return loc


def _msda_check(ops, name, value, shapes, loc, aw, gout, gvalue_b_extra=0):
    ref = R.msda(value, shapes, loc, aw, gout)
    vd, ld, ad = dev(value).requires_grad_(), dev(loc).requires_grad_(), dev(aw).requires_grad_()
    out = ops.ms_deform_attn_core(vd, shapes, ld, ad)
    out.backward(dev(gout))
    nl, P, D = loc.shape[3], loc.shape[4], value.shape[3]
    R.check(f'msda[{name}] out', out.float(), *ref['out'], 1, R.fp32_b(4 * nl * P + 8))
    R.check(f'msda[{name}] gvalue', vd.grad.float(), *ref['gvalue'], 1, R.fp32_b(ref['runs'] + 8 + gvalue_b_extra))
    R.check(f'msda[{name}] gloc', ld.grad, *ref['gloc'], 0, R.fp32_b(D // 8 + 24))
    R.check(f'msda[{name}] gaw', ad.grad, *ref['gaw'], 0, R.fp32_b(D // 8 + 24))
    return ref, out


@pytest.mark.parametrize('D', [8, 16, 32, 64, 128, 256])
def test_msda_bf16_every_D_vs_fp64(ops, D):
    """Every forward LPG (4: D <= 32, 8, 16, 32), every locaw instance and every sorted-backward LPR (1 .. 32), STAGE on, NS = 512 (the
    plain bitonic loop), small and degenerate levels, pixel centres, loc = 0 / 1, a pile of queries on one point."""
    value, loc, aw, gout = _msda_inputs(1, 61, 2, D, SMALL_LEVELS, 2, 10 + D)
    _msda_check(ops, f'D{D}', value, SMALL_LEVELS, _msda_edges(loc, SMALL_LEVELS), aw, gout)


def test_msda_bf16_bench_shape_vs_fp64(ops):
    """The bench's shape per image: 640 px -> levels 160^2, 80^2, 40^2 (L = 33 600), Q = 292 (NS = 8192: the register/shuffle sort),
    8 heads x 64.  The 160^2 level is two full 12 800-row slices, so the sorted backward's first-key table is filled to its last entry;
    samples are placed on the rows around the slice boundary (12 799 | 12 800) and on the level's last row."""
    shapes = [(160, 160), (80, 80), (40, 40)]
    value, loc, aw, gout = _msda_inputs(2, 292, 8, 64, shapes, 4, 20)
    pts = torch.tensor([[159.7, 79.5], [0.3, 79.5], [80.5, 79.9], [159.2, 159.2], [0.5, 80.5], [159.5, 79.5]])
    loc[:, :len(pts), :, 0, 0] = (pts / 160).view(1, len(pts), 1, 2)
    _msda_check(ops, 'bench', value, shapes, loc, aw, gout)


def test_msda_bf16_unstaged_vs_fp64(ops):
    """STAGE = false: Q D 2 bytes = 1 MiB of gout per (image, head) does not fit next to the sort (Q = 2048, P = 1, D = 256, NS = 8192)."""
    shapes = [(8, 8), (4, 4)]
    value, loc, aw, gout = _msda_inputs(1, 2048, 1, 256, shapes, 1, 30)
    _msda_check(ops, 'unstaged', value, shapes, loc, aw, gout)


def test_msda_bf16_slice_boundary_vs_fp64(ops):
    """A 101 x 129 level (13 029 rows > MSDA_SLICE = 12 800: two slices of 6515 rows; the boundary falls inside image row 50, at column 65):
    samples whose four corners lie on both sides of it; plus all-off-map queries, which must give exact zeros."""
    shapes = [(101, 129), (3, 3)]
    H, W = shapes[0]
    value, loc, aw, gout = _msda_inputs(1, 60, 2, 8, shapes, 2, 40)
    g = torch.Generator().manual_seed(41)
    n = 24   # corners (64|65, 49|50) and (64|65, 50|51): rows 6385 .. 6644 around the boundary row 6515 = 50 * 129 + 65
    loc[0, :n, :, 0, :, 0] = (64.5 + torch.rand(n, 2, 2, generator=g) * 0.98 + 0.01) / W
    loc[0, :n, :, 0, :, 1] = (49.5 + torch.rand(n, 2, 2, generator=g) * 1.98 + 0.01) / H
    loc[0, n:n + 6] = -0.7              # every corner of every level off the map
    loc[0, n + 6:n + 12] = 1.8
    ref, out = _msda_check(ops, 'slice', value, shapes, loc, aw, gout)
    assert float(ref['out'][1][0, n:n + 12].abs().max()) == 0 and float(out.detach()[0, n:n + 12].abs().max()) == 0


def test_msda_bf16_atomic_backward_vs_fp64(ops):
    """Q P 4 = 8800 > 8192 corners per level: the float-atomic backward (msda_bwd_kernel), d(value) accumulated in fp32, then rounded."""
    shapes = [(9, 7), (4, 4)]
    value, loc, aw, gout = _msda_inputs(1, 1100, 1, 32, shapes, 2, 50)
    _msda_check(ops, 'atomic', value, shapes, loc, aw, gout)


def test_value_proj_msda_colw_bias_gradient_vs_fp64(ops):
    """ops.value_proj_msda: out, d(loc), d(aw), and the bias gradient from the sorted backward's colw side output, sum_{b,q} gout[b,q,m,:]
    colw[b,q,m], against fp64 (samples over the map's edges, so colw < 1 somewhere); d(value), which the node writes as [B L, N] rows
    (ldg = N = M D: no caller passes a wider ldg), is checked through the products made of it, dx = d(value) W and dW = d(value)^T x.
    Both round d(value) to bf16 first (b gets 2^-8 of the magnitude) and store bf16 (the skinny dW is a bf16 product here)."""
    import torch.nn as nn
    torch.manual_seed(3)
    B, Q, M, D, P = 2, 37, 8, 32, 4
    shapes = [(12, 10), (6, 5), (3, 3)]
    L, N, nl = sum(h * w for h, w in shapes), M * D, len(shapes)
    lin = nn.Linear(N, N).cuda()
    x = rnd((B, L, N), 60).bfloat16().cuda()
    _, loc, aw, gout = _msda_inputs(B, Q, M, D, shapes, P, 61, -0.2, 1.2)
    assert ops.value_proj_msda_ok(x, lin, M, Q, P)
    value = ops.linear_bf16(x, lin.weight, lin.bias).view(B, L, M, D)   # the same GEMM the node runs: the value the core kernels see
    w16 = R._d(ops.bf16_of(lin.weight))
    ref = R.msda(value, shapes, loc, aw, gout)
    xd, ld, ad = x.clone().requires_grad_(), dev(loc).requires_grad_(), dev(aw).requires_grad_()
    out = ops.value_proj_msda(xd, lin, M, shapes, ld, ad)
    out.backward(dev(gout))
    R.check('value_proj_msda out', out.float(), *ref['out'], 1, R.fp32_b(4 * nl * P + 8))
    R.check('value_proj_msda gloc', ld.grad, *ref['gloc'], 0, R.fp32_b(D // 8 + 24))
    R.check('value_proj_msda gaw', ad.grad, *ref['gaw'], 0, R.fp32_b(D // 8 + 24))
    gv, m_gv = (t.reshape(B * L, N) for t in ref['gvalue'])
    x64 = R._d(x).view(B * L, N)
    R.check('value_proj_msda dx', xd.grad.float().view(B * L, N), gv @ w16, m_gv @ w16.abs(), 1, R.U8 + R.fp32_b(ref['runs'] + N + 16))
    R.check('value_proj_msda dW', lin.weight.grad, gv.t() @ x64, m_gv.t() @ x64.abs(), 1, R.U8 + R.fp32_b(ref['runs'] + B * L + 16))
    colw, m_colw = ref['colw']
    assert float(colw.min()) < 0.99
    g64 = R._d(gout).view(B * Q, M, D)
    want = (g64 * colw.view(B * Q, M, 1)).sum(0).view(N)
    mag = (g64.abs() * m_colw.view(B * Q, M, 1)).sum(0).view(N)
    R.check('value_proj_msda dbias', lin.bias.grad, want, mag, 0, R.fp32_b(B * Q + 4 * nl * P + 16))


# ------------------------------------------------------------------------------------------------ ln_gate
@pytest.mark.parametrize('D,tok', [(64, 77), (128, 77), (256, 77), (512, 77), (1024, 77), (512, 2 * 40 * 40)])
def test_ln_gate_bf16_vs_fp64(ops, D, tok):
    """Every D of LG_DISPATCH; 77 tokens is not a multiple of LG_WAVES * LG_TOK_BWD = 64 (a partial last backward block); 3200 tokens: a
    40 x 40 map of two images (the bench's shapes: test_ln_gate_bf16_bench_shape_vs_fp64).  xz is the [tok, 2D] in_proj output (token stride 2D); the xi half of d(xz) must stay exactly 0."""
    x = rnd((tok, D), 70 + D) * 1.5 + 0.3
    xz = rnd((tok, 2 * D), 71 + D).bfloat16()
    gamma, beta = 1 + 0.2 * rnd((D,), 72), 0.1 * rnd((D,), 73)
    gout = rnd((tok, D), 74 + D).bfloat16()
    ref = R.ln_gate(x, xz, gamma, beta, gout)
    xd, zd, gd, bd = dev(x).requires_grad_(), dev(xz).requires_grad_(), dev(gamma).requires_grad_(), dev(beta).requires_grad_()
    out = ops.ln_gate(xd, zd, gd, bd, 1e-5)
    assert out.dtype == torch.bfloat16
    out.backward(dev(gout))
    nblk = (tok + 63) // 64
    R.check(f'ln_gate[{D},{tok}] out', out.float(), *ref['out'], 1, R.fp32_b(48))
    R.check(f'ln_gate[{D},{tok}] dx', xd.grad, *ref['dx'], 0, R.fp32_b(48))
    assert bool((zd.grad[:, :D] == 0).all())
    R.check(f'ln_gate[{D},{tok}] dz', zd.grad[:, D:].float(), *ref['dz'], 1, R.fp32_b(48))
    R.check(f'ln_gate[{D},{tok}] dgamma', gd.grad, *ref['dgamma'], 0, R.fp32_b(nblk + 80))
    R.check(f'ln_gate[{D},{tok}] dbeta', bd.grad, *ref['dbeta'], 0, R.fp32_b(nblk + 80))


@pytest.mark.parametrize('D,side', [(256, 160), (512, 80), (1024, 40)])
def test_ln_gate_bf16_bench_shape_vs_fp64(ops, D, side):
    """The bench's three ln_gate calls: 16 images at 160^2 x 256, 80^2 x 512 and 40^2 x 1024 (MEH VSS blocks, vss.py).  The kernel is
    per token, so out, dx and d(z) are checked against the fp64 reference in blocks of tokens; dgamma and dbeta, which sum over every
    token, are compared with the fp64 sum of the blocks' references."""
    tok, blk = 16 * side * side, 16384
    x = rnd((tok, D), 80 + D) * 1.5 + 0.3
    xz = rnd((tok, 2 * D), 81 + D).bfloat16()
    gamma, beta = 1 + 0.2 * rnd((D,), 82), 0.1 * rnd((D,), 83)
    gout = rnd((tok, D), 84 + D).bfloat16()
    xd, zd, gd, bd = dev(x).requires_grad_(), dev(xz).requires_grad_(), dev(gamma).requires_grad_(), dev(beta).requires_grad_()
    out = ops.ln_gate(xd, zd, gd, bd, 1e-5)
    out.backward(dev(gout))
    out, gx, gz = out.cpu(), xd.grad.cpu(), zd.grad.cpu()
    assert bool((gz[:, :D] == 0).all())
    worst = {'out': 0.0, 'dx': 0.0, 'dz': 0.0}
    ab = {'out': (1, R.fp32_b(48)), 'dx': (0, R.fp32_b(48)), 'dz': (1, R.fp32_b(48))}
    sums = {k: [torch.zeros(D, dtype=torch.float64), torch.zeros(D, dtype=torch.float64)] for k in ('dgamma', 'dbeta')}
    for t0 in range(0, tok, blk):
        s = slice(t0, t0 + blk)
        ref = R.ln_gate(x[s], xz[s], gamma, beta, gout[s])
        for k, got in (('out', out[s].float()), ('dx', gx[s]), ('dz', gz[s, D:].float())):
            worst[k] = max(worst[k], R.check(f'ln_gate[{D},{tok}] {k}', got, *ref[k], *ab[k], log=False))
        for k in sums:
            sums[k][0] += ref[k][0]
            sums[k][1] += ref[k][1]
    for k in worst:
        R.report(f'ln_gate[{D},{tok}] {k}', worst[k], *ab[k], tok * D)
    nblk = (tok + 63) // 64
    R.check(f'ln_gate[{D},{tok}] dgamma', gd.grad, *sums['dgamma'], 0, R.fp32_b(nblk + 80))
    R.check(f'ln_gate[{D},{tok}] dbeta', bd.grad, *sums['dbeta'], 0, R.fp32_b(nblk + 80))
