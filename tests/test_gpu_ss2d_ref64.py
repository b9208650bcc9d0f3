"""The LayerNorm, ln_gate (fp32), cross-merge (csrc/ss2d_out.hip) and depthwise front-end (csrc/dwconv.hip) kernels against fp64 references
with an error model (tests/ref64.py), on every branch their host dispatch can select.  Shapes, seeded inputs, the dispatch restated and
the assertions themselves: tests/ss2d_cases.py (tests/test_ref64_host.py runs the same assertions on CPU emulations and their mutants).

Each assertion is elementwise |got - ref| <= a 2^-8 |ref| + b mag with no free absolute term; a and b are counted in
ref64.layer_norm_bounds / ref64.dwconv_bounds.  Set TAMTR_REF64_REPORT=<file> to collect the worst err / bound ratio of every assertion
(profiles/r10_ss2d_ref64.txt)."""
import pytest
import torch

import ref64 as R
import ss2d_cases as S

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import tamtr_amd.ops as ops
    return ops


def dev(t):
    return t.detach().cuda()


def off(t, nbytes):
    """A device copy of t that starts nbytes into its own buffer."""
    k = nbytes // t.element_size()
    buf = torch.empty(t.numel() + k, device='cuda', dtype=t.dtype)
    assert buf.data_ptr() % 16 == 0
    v = buf[k:].view(t.shape)
    v.copy_(t)
    return v


# ------------------------------------------------------------------------------------------------ LayerNorm
def _ln_op(ops, x, gamma, beta, gout):
    xd, gd, bd = dev(x).requires_grad_(), dev(gamma).requires_grad_(), dev(beta).requires_grad_()
    out = ops.layer_norm(xd, gd, bd, 1e-5)
    assert out.dtype == x.dtype
    out.backward(dev(gout))
    return out.detach(), xd.grad, gd.grad, bd.grad


def _ln_abi(ops, x, gamma, beta, gout, nbytes):
    """tamtr_layernorm_fwd / _bwd called directly, x, out, gout and gx nbytes into their buffers."""
    ntok, D = x.shape
    xd, god = off(x, nbytes), off(gout, nbytes)
    out, gx = off(torch.full_like(x, float('nan')), nbytes), off(torch.full_like(x, float('nan')), nbytes)
    g32, b32 = dev(gamma), dev(beta)
    stats = torch.empty(ntok, 2, device='cuda')
    part = torch.empty(ops._lib.lib().tamtr_ln_gate_blocks(ntok), 2, D, device='cuda')
    assert xd.data_ptr() % 16 == nbytes % 16 and out.data_ptr() % 16 == nbytes % 16
    ops.call('tamtr_layernorm_fwd', ops.ptr(xd), ops.ptr(g32), ops.ptr(b32), ops.ptr(out), ops.ptr(stats), ntok, D, 1e-5, ops.dtype_code(xd), ops.stream_ptr())
    ops.call('tamtr_layernorm_bwd', ops.ptr(god), ops.ptr(xd), ops.ptr(g32), ops.ptr(stats), ops.ptr(gx), ops.ptr(part), ntok, D, ops.dtype_code(xd),
             ops.stream_ptr())
    gsum = ops.slab_sum(part)
    return out, gx, gsum[0], gsum[1]


@pytest.mark.parametrize('ntok', S.LN_NTOK)
@pytest.mark.parametrize('dt,D', [(dt, D) for dt in S.LN_D for D in S.LN_D[dt]])
def test_layer_norm_vs_fp64(ops, dt, D, ntok):
    """ln_fwd / ln_bwd_kernel<float | bf16_t, D> and, for bf16 rows of 64 / 128, ln_fwd / ln_bwd_narrow_kernel<D>: ordinary rows, rows whose
    mean is 32 standard deviations, and constant rows (out == beta exactly; dx == 0 exactly under a cotangent that is flat along the row)."""
    tag = f'ln[{dt},{D},{ntok}'
    for kind in S.LN_KINDS:
        ins = S.ln_inputs(D, ntok, S.DT[dt], kind)
        S.ln_assert(f'{tag},{kind}]', _ln_op(ops, *ins), *ins)
    for flat in (True, False):
        ins = S.ln_constant_inputs(D, ntok, S.DT[dt], flat)
        S.ln_constant_assert(f'{tag},constant{",flat" if flat else ""}]', _ln_op(ops, *ins), *ins, flat)


@pytest.mark.parametrize('kind', S.LN_KINDS)
@pytest.mark.parametrize('D', S.LN_OFFSET_D)
def test_layer_norm_bf16_short_rows_off_16_byte_alignment_vs_fp64(ops, D, kind):
    """x, out, gout and gx 8 bytes into their buffers: the narrow kernels' 16-byte loads do not apply, the host falls back to the
    wave-per-token kernels (8-byte loads on 8-byte aligned rows).  Same bounds as the aligned call, which is run next to it."""
    ins = S.ln_inputs(D, S.LN_OFFSET_NTOK, BF16, kind)
    assert S.ln_kernels(D, True, aligned=False)[0].startswith('ln_fwd_kernel<bf16_t')
    S.ln_assert(f'ln[bf16,{D},{S.LN_OFFSET_NTOK},{kind},+8 bytes]', _ln_abi(ops, *ins, 8), *ins)
    S.ln_assert(f'ln[bf16,{D},{S.LN_OFFSET_NTOK},{kind},abi aligned]', _ln_abi(ops, *ins, 0), *ins)


@pytest.mark.parametrize('D,ntok', S.LN_GATE_F32)
def test_ln_gate_fp32_vs_fp64(ops, D, ntok):
    """ln_gate_fwd / bwd_kernel<float, D> (the bf16 form: tests/test_gpu_bf16_kernels.py); the xi half of d(xz) stays exactly 0."""
    x, xz, gamma, beta, gout = S.ln_gate_inputs(D, ntok)
    xd, zd, gd, bd = (dev(t).requires_grad_() for t in (x, xz, gamma, beta))
    out = ops.ln_gate(xd, zd, gd, bd, 1e-5)
    assert out.dtype == F32
    out.backward(dev(gout))
    assert bool((zd.grad[:, :D] == 0).all())
    S.ln_gate_assert(f'ln_gate[fp32,{D},{ntok}]', (out.detach(), xd.grad, zd.grad[:, D:], gd.grad, bd.grad), x, xz, gamma, beta, gout)


# ------------------------------------------------------------------------------------------------ cross-merge
def _cm_fwd(ops, y4, H, W, nbytes=0):
    B, _, D, L = y4.shape
    yd = off(y4, nbytes)
    ymT = torch.full((B, L, D), float('nan'), device='cuda')
    ops.call('tamtr_cross_merge_fwd', ops.ptr(yd), ops.ptr(ymT), B, D, H, W, ops.dtype_code(yd), ops.stream_ptr())
    return ymT


def _cm_bwd(ops, g, H, W, pdt, nbytes=0):
    B, L, D = g.shape
    g2 = off(torch.full((B, 2, D, L), float('nan'), dtype=pdt), nbytes)
    gd = dev(g)
    ops.call('tamtr_cross_merge_bwd', ops.ptr(gd), ops.ptr(g2), B, D, H, W, ops.dtype_code(g2), ops.stream_ptr())
    return g2


def _cm_run(ops, D, H, W, dt, fwd=True, bwd=True):
    y4, g = S.cm_inputs(D, H, W, dt)
    tag = f'cross_merge[{S.dtn(dt)},{D},{H}x{W}]'
    S.cm_assert(tag, _cm_fwd(ops, y4, H, W) if fwd else None, _cm_bwd(ops, g, H, W, dt) if bwd else None, y4, g, H, W)


@pytest.mark.parametrize('D', S.CM_D)
@pytest.mark.parametrize('H,W', S.CM_GENERIC)
def test_cross_merge_fp32_planes_vs_fp64(ops, H, W, D):
    """cross_merge_fwd_kernel<float> / cross_merge_bwd_kernel<float>."""
    _cm_run(ops, D, H, W, F32)


@pytest.mark.parametrize('D', S.CM_D)
@pytest.mark.parametrize('H,W', S.CM_FWD_BF16_GENERIC)
def test_cross_merge_bf16_odd_map_forward_vs_fp64(ops, H, W, D):
    """cross_merge_fwd_kernel<bf16_t>: H or W odd."""
    assert S.cm_fwd_kernel(H, W, True) == 'cross_merge_fwd_kernel<bf16_t>'
    _cm_run(ops, D, H, W, BF16, bwd=False)


@pytest.mark.parametrize('D', S.CM_D)
@pytest.mark.parametrize('H,W', S.CM_FWD16)
def test_cross_merge_fwd16_vs_fp64(ops, H, W, D):
    assert S.cm_fwd_kernel(H, W, True) == 'cross_merge_fwd16_kernel'
    _cm_run(ops, D, H, W, BF16, bwd=False)


@pytest.mark.parametrize('H,W,D', [(H, W, D) for H, W in S.CM_BWD16 for D in S.CM_D] + [(H, W, 32) for H, W in S.CM_BWD16_D32_ONLY])
def test_cross_merge_bwd16_is_the_adjoint_rounded_to_nearest(ops, H, W, D):
    """cross_merge_bwd16_kernel (32 x 32 tiles that overhang the map by at most 25 %).  (80, 80) is listed with these shapes and does not
    meet the predicate (3 x 3 tiles cover 1.44 x the map): it runs cross_merge_bwd_kernel<bf16_t>, at the size of the bench's second level."""
    assert S.cm_bwd_kernel(H, W, True) == ('cross_merge_bwd_kernel<bf16_t>' if (H, W) in S.CM_BWD16_D32_ONLY else 'cross_merge_bwd16_kernel')
    _cm_run(ops, D, H, W, BF16, fwd=False)


@pytest.mark.parametrize('D', S.CM_D)
@pytest.mark.parametrize('H,W', S.CM_BWD_BF16_GENERIC)
def test_cross_merge_bf16_generic_backward_is_the_adjoint_rounded_to_nearest(ops, H, W, D):
    """cross_merge_bwd_kernel<bf16_t>: even maps that the 32 x 32 tiles would overhang by more than 25 %."""
    assert S.cm_bwd_kernel(H, W, True) == 'cross_merge_bwd_kernel<bf16_t>'
    _cm_run(ops, D, H, W, BF16, fwd=False)


def test_cross_merge_bf16_plane_off_4_byte_alignment_takes_the_generic_kernels(ops):
    """The plane pointer one element (2 bytes) off: the pixel-pair kernels' dword accesses do not apply.  Same result as the aligned call."""
    H, W = S.CM_MISALIGNED_FWD
    y4, _ = S.cm_inputs(32, H, W, BF16)
    assert S.cm_fwd_kernel(H, W, True) == 'cross_merge_fwd16_kernel' and S.cm_fwd_kernel(H, W, True, aligned=False) == 'cross_merge_fwd_kernel<bf16_t>'
    ymT = _cm_fwd(ops, y4, H, W, 2)
    S.cm_assert(f'cross_merge[bf16,32,{H}x{W},+2 bytes]', ymT, None, y4, None, H, W)
    assert torch.equal(ymT, _cm_fwd(ops, y4, H, W))
    H, W = S.CM_MISALIGNED_BWD
    _, g = S.cm_inputs(32, H, W, BF16)
    assert S.cm_bwd_kernel(H, W, True) == 'cross_merge_bwd16_kernel' and S.cm_bwd_kernel(H, W, True, aligned=False) == 'cross_merge_bwd_kernel<bf16_t>'
    g2 = _cm_bwd(ops, g, H, W, BF16, 2)
    S.cm_assert(f'cross_merge[bf16,32,{H}x{W},+2 bytes]', None, g2, None, g, H, W)
    assert torch.equal(g2, _cm_bwd(ops, g, H, W, BF16))


# ------------------------------------------------------------------------------------------------ depthwise front end
def _dw_run(ops, xz, D, w, bias, gout2, pdt):
    """Forward and backward through the launchers of ops.py.  d(xz) arrives filled with a pattern: the kernel must overwrite the xi half
    and leave the rest (z, and any channels beyond 2 D) exactly as it found it."""
    pc = 1 if pdt == BF16 else 0
    xd = dev(xz)
    u2, wd, bvec = ops._dwconv_silu_cross_fwd(xd, dev(w), None if bias is None else dev(bias), D, pc)
    assert u2.dtype == pdt
    keep = torch.arange(xz.numel(), dtype=torch.float32).view(xz.shape).remainder(251).sub(125).to(xz.dtype).cuda()
    gxz = keep.clone()
    gxz[..., :D] = float('nan')
    gw, gb = ops._dwconv_silu_cross_bwd(dev(gout2), xd, wd, bvec, gxz, pc, (D, 9), F32, None if bias is None else F32)
    assert torch.equal(gxz[..., D:], keep[..., D:]), 'the z half of d(xz) was touched'
    return u2, gxz[..., :D], gw, gb


@pytest.mark.parametrize('H,W,form', [(H, W, f) for H, W in S.DW_SHAPES for f in S.dw_forms(H, W)])
def test_dwconv_silu_cross_vs_fp64(ops, H, W, form):
    """dwconv_cross_fwd / bwd_kernel<float, float | bf16_t, float | bf16_t, bf16_t>: out, d(xi), d(weight), d(bias); D = 32 and 64, with
    and without bias.  (bf16 planes where L % 8 == 0, as the bf16 mode requires.)"""
    for D in S.DW_D:
        for bias in (True, False):
            xz, w, b, gout2 = S.dw_inputs(D, H, W, form, bias)
            S.dw_assert(f'dwconv[{form},{D},{H}x{W},{"bias" if bias else "no bias"}]', _dw_run(ops, xz, D, w, b, gout2, S.dw_dtypes(form)[1]), xz, D, w, b, gout2)


@pytest.mark.parametrize('form', S.DW_FORMS)
def test_dwconv_silu_cross_wider_pixel_stride_vs_fp64(ops, form):
    """A pixel stride of 2 D + 8 elements (forward and d(xz))."""
    (H, W), D, extra = S.DW_STRIDE_CASE
    xz, w, b, gout2 = S.dw_inputs(D, H, W, form, True, extra)
    S.dw_assert(f'dwconv[{form},{D},{H}x{W},stride 2D+{extra}]', _dw_run(ops, xz, D, w, b, gout2, S.dw_dtypes(form)[1]), xz, D, w, b, gout2)


@pytest.mark.parametrize('H,W', S.DW_ROUNDED_ONCE)
def test_dwconv_bf16_planes_are_the_f32_planes_rounded_once(ops, H, W):
    """The front end of test_ss2d_bf16_planes_are_the_f32_kernels_rounded_once alone, on the scalar gradient path: the bf16-plane forward is
    the fp32-plane forward rounded once, and fed the same (bf16) cotangent both backwards give the same bits."""
    D = 32
    xz, w, b, g16 = S.dw_inputs(D, H, W, 'bf16_bf16planes', True)
    assert not S.dw_vector_path(H, W)
    u32, dx32, gw32, gb32 = _dw_run(ops, xz, D, w, b, g16.float(), F32)
    u16, dx16, gw16, gb16 = _dw_run(ops, xz, D, w, b, g16, BF16)
    assert torch.equal(u16, u32.bfloat16())
    assert torch.equal(dx16, dx32) and torch.equal(gw16, gw32) and torch.equal(gb16, gb32)


def _dw_forward_f32(ops, xz, D, w, bias):
    u2, _, _ = ops._dwconv_silu_cross_fwd(dev(xz), dev(w), dev(bias), D, 0)
    return u2.cpu()


def test_dwconv_nan_pattern_is_the_references(ops):
    """A NaN at an interior pixel and one at a corner (fp32, D = 32, 8 x 8): both planes are NaN exactly where conv2d + SiLU are, and
    within the bound elsewhere."""
    D, H, W = 32, 8, 8
    xz, w, b, _ = S.dw_inputs(D, H, W, 'fp32', True)
    xz[0, 3, 4, 5] = float('nan')
    xz[1, 0, 7, 9] = float('nan')
    ref = R.dwconv_silu_cross(xz, D, w, b, None)
    assert int(torch.isnan(ref['out'][0]).sum()) == 2 * (9 + 4)
    R.check('dwconv[fp32,nan] out', _dw_forward_f32(ops, xz, D, w, b), *ref['out'], *R.dwconv_bounds(ref['zmax'], S.DW_B, H, W, False, False)['out'])


def test_dwconv_inf_at_a_corner_stays_inf(ops):
    """+Inf at corner pixel (0, 0) of one channel whose nine weights are positive and whose bias is 0 (fp32, D = 32, 8 x 8): the four
    outputs whose window holds the pixel are +Inf in both planes, as conv2d + SiLU give, and every other output is what it is without the
    Inf.  (A halo zeroed by multiplying a clamped load by 0 makes them NaN: Inf * 0.)"""
    D, H, W, c = 32, 8, 8, 5
    xz, w, b, _ = S.dw_inputs(D, H, W, 'fp32', True)
    w[c] = w[c].abs() + 0.05
    b[c] = 0
    clean = _dw_forward_f32(ops, xz, D, w, b)
    xz[1, 0, 0, c] = float('inf')
    want = R.dwconv_silu_cross(xz, D, w, b, None)['out'][0]
    inf = torch.isinf(want)
    hit = torch.zeros(H, W, dtype=torch.bool)
    hit[:2, :2] = True
    where = torch.zeros(S.DW_B, 2, D, H * W, dtype=torch.bool)
    where[1, :, c] = hit.flatten()                       # (the 2 x 2 corner block is its own transpose)
    assert torch.equal(inf, where) and bool((want[inf] > 0).all()) and not bool(torch.isnan(want).any())
    out = _dw_forward_f32(ops, xz, D, w, b)
    assert not bool(torch.isnan(out).any()), f'{int(torch.isnan(out).sum())} outputs are NaN'
    assert torch.equal(torch.isinf(out), inf) and bool((out[inf] > 0).all())
    assert torch.equal(out[~inf], clean[~inf])
