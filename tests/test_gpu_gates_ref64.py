"""The text gate (csrc/gate.hip) and CPAM (csrc/cpam.hip) kernels against fp64 references with an error model (tests/ref64.py), fp32 and
bf16, on every branch their host dispatch can select.  Shapes and seeded inputs: tests/gate_cases.py.

Each assertion is elementwise |got - ref| <= a 2^-8 |ref| + b mag, with no free absolute term; a and b are counted in
ref64.gate_bounds / ref64.cpam_bounds.  The gradients that an argmax routes (dx and dgk of the gate, dx of CPAM) are discontinuous where
the two largest candidates are closer than fp32 can tell apart: every case first asserts, on the reference alone, that its input has no
such decision, then that the kernel's saved argmax is the reference's.  Set TAMTR_REF64_REPORT=<file> to collect the worst err / bound
ratio of every assertion."""
import copy

import pytest
import torch

import gate_cases as G
import ref64 as R
from conftest import assert_close
from weights import rnd

pytestmark = pytest.mark.gpu

DT = {'fp32': torch.float32, 'bf16': torch.bfloat16}
BF = torch.bfloat16


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import tamtr_amd.ops as ops
    return ops


def dev(t):
    return t.detach().cuda()


# ------------------------------------------------------------------------------------------------ gate, NCHW, forward and backward
def _gate_run(ops, name, shape, dt, scale=1.0, bias=None, seed=None):
    B, C, nh, H, W, T = shape
    hc, HW = C // nh, H * W
    x, gk, bias, v, gout = G.gate_inputs(shape, dt, G.GATE_SEED.get((name.split('|')[0], dt), 1) if seed is None else seed, bias)
    ref = R.maxsigmoid_gate(x, gk, bias, v, nh, scale, gout)
    assert R.ambiguous(ref['gap'], ref['gap_mag'], R.fp32_b(hc)) == 0
    xd, gd, bd, vd = (dev(t).requires_grad_() for t in (x, gk, bias, v))
    out = ops.maxsigmoid_gate(xd, gd, bd, vd, nh, scale)
    assert out.dtype == dt
    sx, sgk, sv, aw, arg = out.grad_fn.saved_tensors
    assert torch.equal(arg.cpu().long(), ref['arg'])
    out.backward(dev(gout))
    # dlogit stays inside the autograd node: the backward kernel once more, on the node's own saved tensors
    dx2, dv2 = torch.empty_like(sx), torch.empty_like(sx)
    dlogit = torch.empty(B, nh, HW, device='cuda', dtype=torch.float32)
    go = dev(gout).contiguous()
    ops.call('tamtr_maxsigmoid_gate_bwd', ops.ptr(go), ops.ptr(sx), ops.ptr(sgk), ops.ptr(sv), ops.ptr(aw), ops.ptr(arg), ops.ptr(dx2), ops.ptr(dv2),
             ops.ptr(dlogit), B, nh, hc, HW, T, ops._F(scale), ops.dtype_code(sx), ops.stream_ptr())
    ab = R.gate_bounds(hc, HW, B, ref['zmax'], dt == BF)
    tag = f'gate[{name},{"bf16" if dt == BF else "fp32"}]'
    for n, got in (('out', out), ('dv', vd.grad), ('dx', xd.grad), ('dlogit', dlogit), ('dgk', gd.grad), ('dbias', bd.grad)):
        R.check(f'{tag} {n}', got.float(), *ref[n], *ab[n])
    assert torch.equal(dx2, xd.grad) and torch.equal(dv2, vd.grad)
    return ref, out, arg, gd.grad


@pytest.mark.parametrize('dt', list(DT))
@pytest.mark.parametrize('case', list(G.GATE_NCHW))
def test_gate_nchw_vs_fp64(ops, case, dt):
    """gate_fwd_kernel / gate_bwd_kernel<fp32 | bf16, PX = 4 | 1>: out, dv, dx, dlogit, and the torch reductions dgk, dbias."""
    _gate_run(ops, case, G.GATE_NCHW[case], DT[dt])


@pytest.mark.parametrize('dt', list(DT))
def test_gate_nchw_scale_vs_fp64(ops, dt):
    """scale = 0.37 multiplies out, dv and dlogit (the trunk passes 1.0 everywhere)."""
    _gate_run(ops, 't17|scale', G.GATE_NCHW['t17'], DT[dt], scale=0.37)


@pytest.mark.parametrize('dt', list(DT))
def test_gate_nchw_saturated_vs_fp64(ops, dt):
    """Biases of +20 and -20: one head's gate is 1 - 2e-9 (1 - a keeps no relative accuracy: the model says so), the other's 2e-9."""
    ref, out, _, _ = _gate_run(ops, 'vec_one_pass|saturated', G.GATE_NCHW['vec_one_pass'], DT[dt], bias=[20.0, -20.0])
    assert ref['zmax'] > 16


@pytest.mark.parametrize('dt', list(DT))
def test_gate_nchw_equal_text_rows_take_the_lower_index(ops, dt):
    """Two identical text rows (3 and 7 of 10): the first maximum wins - the saved argmax is never 7, dgk of row 7 is exactly 0 - and the
    forward is bit-identical to the one with row 7 removed."""
    dt = DT[dt]
    B, C, nh, H, W, T = G.GATE_NCHW['vec_one_pass']
    x, gk, bias, v, gout = G.gate_inputs((B, C, nh, H, W, T), dt, 11)
    gk[:, 7] = gk[:, 3]
    xd, gd, bd, vd = (dev(t).requires_grad_() for t in (x, gk, bias, v))
    out = ops.maxsigmoid_gate(xd, gd, bd, vd, nh)
    arg = out.grad_fn.saved_tensors[4]
    ref = R.maxsigmoid_gate(x, gk, bias, v, nh, 1.0, gout)
    assert int((ref['arg'] == 3).sum()) > 0 and int((ref['arg'] == 7).sum()) == 0        # the reference's rule: the first occurrence
    assert int((arg == 7).sum()) == 0 and int((arg == 3).sum()) > 0
    out.backward(dev(gout))
    assert float(gd.grad[:, 7].abs().max()) == 0 and float(gd.grad[:, 3].abs().max()) > 0
    keep = [t for t in range(T) if t != 7]
    out9 = ops.maxsigmoid_gate(dev(x), dev(gk[:, keep]), dev(bias), dev(v), nh)
    assert torch.equal(out.detach(), out9)
    R.check('gate[equal_rows] out', out.float(), *ref['out'], *R.gate_bounds(C // nh, H * W, B, ref['zmax'], dt == BF)['out'])


# ------------------------------------------------------------------------------------------------ gate, channels-last, forward only
def _gate_cl_run(ops, case, dt, wide):
    C, nh, H, W, T = G.GATE_CL[case]
    emap, c0, v, gk, bias, mean_rstd, gamma, beta = G.gate_cl_inputs(case, dt, wide)
    e = emap[:, c0:c0 + C]
    ref = R.maxsigmoid_gate(e, gk, bias, v, nh, 1.0, None, v_affine=(mean_rstd, gamma, beta))
    bn = torch.nn.BatchNorm2d(C).cuda()
    with torch.no_grad():
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
    ed = emap.cuda()[:, c0:c0 + C]
    assert ops.gate_cl_ok(ed, C, nh, T) and (wide == 1) == ops.is_cl(ed)
    out = ops.maxsigmoid_gate_cl(ed, dev(gk), dev(bias), v.cuda(), dev(mean_rstd), bn, nh, 1.0)
    assert out.dtype == dt and ops.is_cl(out) and out.shape == e.shape
    R.check(f'gate_cl[{case},{"bf16" if dt == BF else "fp32"},e pitch {wide}C] out', out.float(), *ref['out'],
            *R.gate_bounds(C // nh, H * W, 2, ref['zmax'], dt == BF)['out'])


@pytest.mark.parametrize('dt', list(DT))
@pytest.mark.parametrize('wide', [2, 3])
@pytest.mark.parametrize('case', list(G.GATE_CL))
def test_gate_channels_last_vs_fp64(ops, case, wide, dt):
    """gate_cl_fwd_kernel<fp32 | bf16, VBN>: e is a channel slice of a map 2 and 3 times as wide; mean_rstd is built from fp64 statistics,
    so this tests the kernel and not the statistics kernel.  Every row of both images is compared (out is allocated by the op): a row tail
    that disturbed the next image's first rows would show there."""
    _gate_cl_run(ops, case, DT[dt], wide)


@pytest.mark.parametrize('dt', list(DT))
@pytest.mark.parametrize('case', G.GATE_CL_CONTIGUOUS)
def test_gate_channels_last_contiguous_e_vs_fp64(ops, case, dt):
    _gate_cl_run(ops, case, DT[dt], 1)


# ------------------------------------------------------------------------------------------------ CPAM
def _cpam_fn(ops, cl):
    return ops._CPAMCL if cl else ops._CPAM


def _cpam_place(t, cl):
    t = t.cuda()
    return t.contiguous(memory_format=torch.channels_last) if cl else t.contiguous()


def _cpam_run(ops, shape, dt, cl, x=None, gout=None, unambiguous=True):
    B, C, H, W = shape
    if x is None:
        x, gout = G.cpam_inputs(shape, dt, G.CPAM_SEED.get((shape, dt), 5))
    ref = R.cpam(x, gout)
    ab = R.cpam_bounds(C // 8, ref['zmax'], dt == BF)
    if unambiguous:
        assert R.ambiguous(ref['gap'], ref['gap_mag'], ab['c'][1]) == 0
    xd = _cpam_place(x, cl).requires_grad_()
    out = _cpam_fn(ops, cl).apply(xd)
    assert out.dtype == dt and ops.is_cl(out) == cl
    sx, p, idx, s2r, argr = out.grad_fn.saved_tensors                     # (taken before backward() frees them)
    s2, arg = s2r, argr
    if cl:
        s2, arg = s2.permute(0, 3, 1, 2), arg.permute(0, 3, 1, 2)
    assert torch.equal(p.cpu().double(), ref['p'])                      # a maximum of the map's values is one of them: exact
    if unambiguous:
        assert torch.equal(arg.cpu().long(), ref['arg'])
    out.backward(_cpam_place(gout, cl))
    tag = f'cpam[{"cl" if cl else "nchw"},{B}x{C}x{H}x{W},{"bf16" if dt == BF else "fp32"}]'
    R.check(f'{tag} s2', s2, *ref['s2'], *ab['s2'])
    R.check(f'{tag} out', out.float(), *ref['out'], *ab['out'])
    R.check(f'{tag} dx', xd.grad.float(), *ref['dx'], *ab['dx'])
    # the stored intermediates stay inside the autograd node: the backward kernels once more, on the node's own saved tensors
    go = _cpam_place(gout, cl)
    dxd, du, dp, dx2 = torch.empty_like(sx), torch.empty_like(sx), torch.empty_like(p), torch.empty_like(sx)
    if cl:
        ops.call('tamtr_cpam_cl_bwd', ops.ptr(go), ops.ptr(sx), ops.ptr(p), ops.ptr(idx), ops.ptr(s2r), ops.ptr(argr), ops.ptr(dxd), ops.ptr(du),
                 ops.ptr(dp), ops.ptr(dx2), B, C, H, W, ops.dtype_code(sx), ops.stream_ptr())
        assert torch.equal(dx2, xd.grad)
    else:
        ops.call('tamtr_cpam_bwd', ops.ptr(go), ops.ptr(sx), ops.ptr(p), ops.ptr(s2r), ops.ptr(argr), ops.ptr(dxd), ops.ptr(du), ops.ptr(dp),
                 B, C, H, W, ops.dtype_code(sx), ops.stream_ptr())
    for n, got in (('dxd', dxd), ('du', du), ('dp', dp)):
        R.check(f'{tag} {n}', got.float(), *ref[n], *ab[n])
    return ref, out, xd.grad


@pytest.mark.parametrize('shape', G.CPAM_CL_BF16)
def test_cpam_channels_last_bf16_vs_fp64(ops, shape):
    """pool3s2_cl_* and cpam_cl_{fwd,bwd,dp}_kernel<bf16>: chunks of 1, 2, 4 and 8 lanes; (1, 128, 2, 2) is one pooled cell (Hp = Wp = 1:
    every border weight of the dp gather is 1)."""
    _cpam_run(ops, shape, BF, True)


@pytest.mark.parametrize('shape', G.CPAM_CL_F32)
def test_cpam_channels_last_fp32_vs_fp64(ops, shape):
    _cpam_run(ops, shape, torch.float32, True)


@pytest.mark.parametrize('dt', list(DT))
@pytest.mark.parametrize('shape', G.CPAM_NCHW)
def test_cpam_nchw_vs_fp64(ops, shape, dt):
    """cpam_fwd_kernel<T, 16 | 0>, cpam_bwd_kernel, cpam_dp_kernel and the NCHW max-pool."""
    _cpam_run(ops, shape, DT[dt], False)


def test_cpam_nchw_near_the_dp_grid_limit_vs_fp64(ops):
    """(255, 256, 2, 2) puts B C = 65 280 rows on cpam_dp_kernel's grid.y, 255 below its limit.  fp32 only: see gate_cases.py."""
    _cpam_run(ops, G.CPAM_NCHW_GRID_LIMIT, torch.float32, False)


@pytest.mark.parametrize('cl', [False, True])
@pytest.mark.parametrize('bad', ['nan', 'inf', 'inf_border'])
def test_cpam_nan_and_inf_in_a_pooled_window(ops, cl, bad):
    """A NaN in x: the pool lets it win, so it spreads to the pixels that tap its cell, and the chunk maximum lets it win, so all of the
    chunk is NaN at those pixels (torch.max) - the NaN pattern of out is the reference's.  An inf at (4, 4), in pooled cell (2, 2) only:
    the gate saturates to 1 around it, out is inf at that one pixel and finite (and within the bound) everywhere else.  An inf at (0, 0),
    in pooled cell (0, 0): pixel row 0 and column 0 form 0 * p[0] + 1 * p[0] (ref64._up2), so the five pixels of row 0 and column 0 that
    tap the cell are NaN in all 16 channels of the chunk, and nothing else is."""
    shape = (1, 128, 12, 16)                  # 16 channels per chunk: two lanes of the channels-last kernel merge their maxima
    x, _ = G.cpam_inputs(shape, BF, 21)
    at = (0, 0) if bad == 'inf_border' else (4, 4)
    x[0, 13, at[0], at[1]] = float(bad.split('_')[0])
    ref = R.cpam(x, None)
    with torch.no_grad():
        out = _cpam_fn(ops, cl).apply(_cpam_place(x, cl)).float().cpu()
    want, mag = ref['out']
    if bad == 'nan':
        assert int(torch.isnan(want).sum()) == 16 * 16 and not bool(torch.isnan(want[:, 16:]).any())
    if bad == 'inf_border':
        nan = torch.zeros(12, 16, dtype=torch.bool)
        nan[0, :3] = nan[:3, 0] = True
        assert torch.equal(torch.isnan(want), nan.expand(1, 128, 12, 16) & (torch.arange(128) < 16).view(1, 128, 1, 1))
    inf = torch.isinf(want)
    assert int(inf.sum()) == (bad == 'inf') and torch.equal(torch.isinf(out), inf) and torch.equal(out[inf].double(), want[inf])
    out, want, mag = (torch.where(inf, torch.zeros_like(t), t) for t in (out.double(), want, mag))
    R.check(f'cpam[{"cl" if cl else "nchw"},{bad}] out', out, want, mag, *R.cpam_bounds(16, ref['zmax'], True)['out'])


@pytest.mark.parametrize('cl', [False, True])
def test_cpam_zero_input_and_zero_cotangent_are_exact(ops, cl):
    """x = 0: every magnitude of out is 0, so out must be exactly 0 (the bound has no free absolute term), and dx = gout / 4 is held to its
    bound; gout = 0: dx must be exactly 0.  (Every argmax is a tie here; nothing is routed through it: S = 0.)"""
    shape = (2, 64, 4, 6)
    x, gout = G.cpam_inputs(shape, BF, 23)
    _, out, _ = _cpam_run(ops, shape, BF, cl, torch.zeros_like(x), gout, unambiguous=False)
    assert float(out.detach().abs().max()) == 0
    _, _, dx = _cpam_run(ops, shape, BF, cl, x, torch.zeros_like(gout), unambiguous=False)
    assert float(dx.abs().max()) == 0


# ------------------------------------------------------------------------------------------------ vocabulary-size fallback
def test_gate_block_long_vocabulary_takes_the_separate_path(ops):
    """80 text rows at a 256-channel site: the fp32 text tile (80 KiB) does not fit the channels-last kernel's 60 KiB of LDS, so
    gate_cl_ok(..., T) is false and the no-grad forward of MaxSigmoidAttnBlock takes the separate path (BatchNorm kernels -> NCHW gate
    kernel) and must not raise.  Same result as the block on an NCHW copy, within the rounding documented in
    test_gate_with_batchnorm_folded_in_equals_the_separate_path; the BatchNorm's running statistics are updated once."""
    import tamtr_amd.modules as modules
    c, nh, hw, T = 256, 8, 12, 80
    torch.manual_seed(3)
    blk = modules.MaxSigmoidAttnBlock(c, c, nh=nh, ec=c).cuda().train()
    with torch.no_grad():
        blk.bias.copy_(0.3 * torch.randn(nh)); blk.proj_conv.bn.weight.copy_(1 + 0.2 * torch.randn(c)); blk.proj_conv.bn.bias.copy_(0.1 * torch.randn(c))
    twin = copy.deepcopy(blk)
    x = (rnd((2, c, hw, hw), 1) * 1.5).bfloat16().cuda().contiguous(memory_format=torch.channels_last)
    guide = rnd((2, T, 512), 2).cuda()
    assert ops.gate_cl_ok(x, c, nh) and ops.gate_cl_ok(x, c, nh, 10) and not ops.gate_cl_ok(x, c, nh, T)
    with torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16):
        out = blk(x, guide)
        ref = twin(x.contiguous(), guide)
    assert_close(out.float(), ref.float(), 3e-2, 3e-2, 'gate out')
    assert_close(blk.proj_conv.bn.running_mean, twin.proj_conv.bn.running_mean, 1e-5, 1e-6, 'running_mean')
    assert_close(blk.proj_conv.bn.running_var, twin.proj_conv.bn.running_var, 1e-4, 1e-6, 'running_var')
    assert int(blk.proj_conv.bn.num_batches_tracked) == int(twin.proj_conv.bn.num_batches_tracked) == 1
    assert float(blk.proj_conv.bn.running_mean.abs().max()) > 0
