"""The BatchNorm kernels of csrc/bn.hip against fp64 references with an error model (tests/ref64.py batch_norm, batch_norm_pair, bn_bounds), on
every branch their host dispatch can select: both layouts, the pair, the segmented form, the statistics alone and tamtr_bn_finalize on
hand-made partials.  The dispatch restated, the cases, the seeded inputs and the assertions themselves: tests/bn_cases.py
(tests/test_ref64_host.py runs the same assertions on CPU emulations and their mutants).

Each assertion is elementwise |got - ref| <= a 2^-8 |ref| + b mag with no free absolute term; a and b are counted in ref64.bn_bounds from
the plan of the case, and tamtr_bn_slices / tamtr_bncl_blocks are asserted against that plan.  Set TAMTR_REF64_REPORT=<file> to collect the
worst err / bound ratio of every assertion (profiles/r18_bn_ref64.txt)."""
import pytest
import torch

import bn_cases as K

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


def module(C, eps, mom, params, track=True):
    import torch.nn as nn
    bn = nn.BatchNorm2d(C, eps=eps, momentum=mom, track_running_stats=track).cuda()
    with torch.no_grad():
        bn.weight.copy_(params[0]); bn.bias.copy_(params[1])
        if track:
            bn.running_mean.copy_(params[2]); bn.running_var.copy_(params[3])
    return bn


def nchw_plan(ops, B, C, HW, bf16):
    plan = K.nchw_plan(B, C, HW, bf16)
    assert ops._lib.lib().tamtr_bn_slices(B, HW) == plan[2], 'the slicing of csrc/bn.hip is no longer what tests/bn_cases.py restates'
    return plan


def cl_plan(ops, N, C, dt):
    plan = K.cl_plan(N, C, dt == BF16)
    assert ops._lib.lib().tamtr_bncl_blocks(N, C, 1 if dt == BF16 else 0) == plan[4], 'the chunking of csrc/bn.hip is no longer what tests/bn_cases.py restates'
    return plan


def strided(g):
    """g [N, C] as the left half of a [N, 2 C] device map (ldgy = 2 C), which the backward must read in place."""
    wide = torch.full((g.shape[0], 2 * g.shape[1]), float('nan'), device='cuda', dtype=g.dtype)
    wide[:, :g.shape[1]] = g
    return wide[:, :g.shape[1]]


def run_single(ops, x, bn, act, gout, residual=None):
    """ops.bn_act forward and backward on device tensors -> {name: tensor}, maps as rows."""
    xd = x.requires_grad_()
    rd = None if residual is None else residual.requires_grad_()
    out = ops.bn_act(xd, bn, bool(act), rd)
    assert out.dtype == x.dtype
    mr = out.grad_fn.saved_tensors[3]
    out.backward(gout)
    as_rows = (lambda t: t) if x.dim() == 2 else K.rows
    got = {'out': as_rows(out.detach()), 'dx': as_rows(xd.grad), 'dgamma': bn.weight.grad, 'dbeta': bn.bias.grad, 'mean': mr[:, 0], 'rstd': mr[:, 1]}
    if bn.track_running_stats:
        got.update({'running_mean': bn.running_mean, 'running_var': bn.running_var})
    if rd is not None:
        got['dres'] = rd.grad
    return got


# ------------------------------------------------------------------------------------------------ NCHW
def _nchw_case(ops, B, C, HW, dt, act, kind, eps, mom, tag):
    plan = nchw_plan(ops, B, C, HW, dt == BF16)
    x, g = K.bn_rows(B * HW, C, dt, kind, 100 + 7 * HW + B, K.home_row('nchw', plan, B * HW, B, HW))
    p = K.bn_params(C, 11 + C)
    H = 1 if HW < 4 or HW % 4 else 4
    got = run_single(ops, dev(K.nchw(x, B, HW)).view(B, C, H, HW // H), module(C, eps, mom, p), act, dev(K.nchw(g, B, HW)).view(B, C, H, HW // H))
    K.bn_single_assert(tag, got, 'nchw', plan, x, p[0], p[1], g, eps, mom, p[2], p[3], act)
    if kind == 'constant':
        K.bn_constant_assert(tag, got, C, p[1], act, dt, eps)


@pytest.mark.parametrize('act', (0, 1))
@pytest.mark.parametrize('dt', ('fp32', 'bf16'))
@pytest.mark.parametrize('B,C,HW', K.NCHW_SHAPES)
def test_bn_nchw_vs_fp64(ops, B, C, HW, dt, act):
    """tamtr_bn_act_fwd / _bwd: bn_stats, bn_apply, bn_bwd_reduce, bn_bwd_apply<float | bf16_t> on the vector and scalar paths, one to three
    slices per plane, an almost empty tail slice, S = 260 partials and a channel of one value; both parameter settings of the model."""
    for eps, mom in K.EPS_MOM:
        _nchw_case(ops, B, C, HW, K.DT[dt], act, 'ordinary', eps, mom, f'bn[nchw,{dt},{B}x{C}x{HW},act={act},eps={eps}]')


@pytest.mark.parametrize('dt', ('fp32', 'bf16'))
@pytest.mark.parametrize('B,C,HW,kind', K.NCHW_KIND_CASES)
def test_bn_nchw_input_kinds_vs_fp64(ops, B, C, HW, dt, kind):
    """A mean of 32 standard deviations, channels of scale 1e-3 and 1e3, a value 64 standard deviations out at the head of the tail slice,
    a constant channel (exact results; on the power-of-two count only, which its exact assertions need), and a NaN | Inf in an ordinary
    place and at the head of the tail slice: that channel follows the reference's NaN pattern, every other channel stays within its
    ordinary bounds."""
    for act in (0, 1):
        _nchw_case(ops, B, C, HW, K.DT[dt], act, kind, 1e-3, 0.03, f'bn[nchw,{dt},{B}x{C}x{HW},act={act},{kind}]')


def test_bn_nchw_bf16_maps_off_8_byte_alignment_take_the_scalar_path(ops):
    """tamtr_bn_act_fwd / _bwd called directly with x, y, gy, gx 4 bytes into their buffers (bf16, HW % 4 == 0): bn_vec sends the call to the
    scalar path; same bounds."""
    B, C, HW, nb = K.NCHW_OFFSET
    plan = K.nchw_plan(B, C, HW, True, aligned=False)
    assert not plan[0] and K.nchw_plan(B, C, HW, True)[0]
    eps, mom, act = 1e-3, 0.03, 1
    x, g = K.bn_rows(B * HW, C, BF16, 'ordinary', 77)
    p = K.bn_params(C, 11 + C)
    xd, gd = off(K.nchw(x, B, HW), nb), off(K.nchw(g, B, HW), nb)
    y, gx = off(torch.full((B, C, HW), float('nan'), dtype=BF16), nb), off(torch.full((B, C, HW), float('nan'), dtype=BF16), nb)
    assert all(t.data_ptr() % 8 == 4 for t in (xd, gd, y, gx))
    ga, be, rm, rv = (dev(t) for t in p)
    mr, gg, gb = torch.empty(C, 2, device='cuda'), torch.empty(C, device='cuda'), torch.empty(C, device='cuda')
    part = torch.empty(C * plan[2] * 3, device='cuda')
    ops.call('tamtr_bn_act_fwd', ops.ptr(xd), ops.ptr(ga), ops.ptr(be), ops.ptr(rm), ops.ptr(rv), ops.ptr(y), ops.ptr(mr), ops.ptr(part), B, C, HW, eps, mom,
             act, ops.dtype_code(xd), ops.stream_ptr())
    ops.call('tamtr_bn_act_bwd', ops.ptr(gd), ops.ptr(xd), ops.ptr(ga), ops.ptr(be), ops.ptr(mr), ops.ptr(gx), ops.ptr(gg), ops.ptr(gb), ops.ptr(part), B, C, HW,
             act, ops.dtype_code(xd), ops.stream_ptr())
    got = {'out': K.rows(y), 'dx': K.rows(gx), 'dgamma': gg, 'dbeta': gb, 'mean': mr[:, 0], 'rstd': mr[:, 1], 'running_mean': rm, 'running_var': rv}
    K.bn_single_assert(f'bn[nchw,bf16,{B}x{C}x{HW},+{nb} bytes]', got, 'nchw', plan, x, p[0], p[1], g, eps, mom, p[2], p[3], act)


# ------------------------------------------------------------------------------------------------ channels-last, one BatchNorm
def _cl_case(ops, N, C, dt, act, residual, strided_gy, kind, tag, eps=1e-3, mom=0.03):
    plan = cl_plan(ops, N, C, dt)
    x, g = K.bn_rows(N, C, dt, kind, 200 + 3 * C + N % 1000, K.home_row('cl', plan, N))
    r = (0.5 * K.rnd((N, C), 300 + C)).to(dt) if residual else None
    p = K.bn_params(C, 11 + C)
    gd = strided(dev(g)) if strided_gy else dev(g)
    if strided_gy:
        assert ops._gy_rows(gd, dev(x)).data_ptr() == gd.data_ptr() and gd.stride(0) == 2 * C
    got = run_single(ops, dev(x), module(C, eps, mom, p), act, gd, None if r is None else dev(r))
    K.bn_single_assert(tag, got, 'cl', plan, x, p[0], p[1], g, eps, mom, p[2], p[3], act, r)
    if kind == 'constant':
        K.bn_constant_assert(tag, got, C, p[1], act, dt, eps)


@pytest.mark.parametrize('dt,C,rows', [(dt, C, n) for dt in K.CL_C for C in K.CL_C[dt] for n in K.cl_rows(C, dt == 'bf16')])
def test_bn_channels_last_vs_fp64(ops, dt, C, rows):
    """tamtr_bncl_act_fwd / _bwd: bncl_stats, bn_finalize, bncl_apply, bncl_bwd_reduce, bncl_sum, bncl_bwd_apply<float, 4 | bf16_t, 4 | bf16_t, 8>
    at cg = 1 .. 256; one row, less than a piece, one chunk, one chunk and a row, a map that ends inside a piece of its last chunk; identity and
    SiLU, with and without the residual, gy packed and as a channel slice of a wider map."""
    N = K.cl_rows(C, dt == 'bf16')[rows]
    for act, residual, sg in K.CL_VARIANTS:
        _cl_case(ops, N, C, K.DT[dt], act, residual, sg, 'ordinary', f'bn[cl,{dt},{N}x{C},act={act},res={int(residual)},ldgy={"2C" if sg else "C"}]')
    _cl_case(ops, N, C, K.DT[dt], 1, False, False, 'ordinary', f'bn[cl,{dt},{N}x{C},eps=1e-5]', 1e-5, 0.1)


@pytest.mark.parametrize('kind', K.KINDS[1:])
@pytest.mark.parametrize('inst', list(K.CL_KIND_C))
def test_bn_channels_last_input_kinds_vs_fp64(ops, inst, kind):
    """Every input kind on one shape per (T, V) instantiation; the map ends inside a piece of its last chunk, whose first row holds the
    outlier | the NaN | the Inf of the `home` kinds (the row that padded loads are redirected to and that the sums are shifted by).  The
    constant kind runs on exactly one chunk: a power-of-two count, which its exact assertions need."""
    dt, C = (BF16 if inst.startswith('bf16') else F32), K.CL_KIND_C[inst]
    N = K.cl_rows(C, dt == BF16)['chunk' if kind == 'constant' else 'inside']
    for act in (0, 1):
        _cl_case(ops, N, C, dt, act, act == 1 and kind != 'constant', False, kind, f'bn[cl,{K.dtn(dt)},{N}x{C},act={act},{kind}]')


@pytest.mark.parametrize('case', list(K.CL_LARGE))
def test_bn_channels_last_long_chains_vs_fp64(ops, case):
    """257 chunks (bn_finalize_kernel, bncl_sum_kernel and both backward kernels loop over S > 256) and the smallest map with iters = 8."""
    dt, C, N = K.CL_LARGE[case]
    plan = cl_plan(ops, N, C, K.DT[dt])
    assert (plan[4] > 256) if case == 'S>256' else (plan[2] == 8)
    _cl_case(ops, N, C, K.DT[dt], 1, False, False, 'ordinary', f'bn[cl,{dt},{N}x{C},{case}]')


# ------------------------------------------------------------------------------------------------ channels-last, the pair
@pytest.mark.parametrize('dt,C,rows,sg', K.PAIR_CASES)
def test_bn_pair_vs_fp64(ops, dt, C, rows, sg):
    """tamtr_bncl2_act_fwd / _bwd: act(bn1(x1) + bn2(x2)) with SiLU: out, dx1, dx2, both dgamma, both dbeta, both BatchNorms' statistics."""
    N = K.cl_rows(C, dt == 'bf16')[rows]
    plan = cl_plan(ops, N, C, K.DT[dt])
    x1, g = K.bn_rows(N, C, K.DT[dt], 'ordinary', 400 + C)
    x2 = (1.3 * K.rnd((N, C), 401 + C) - 0.7).to(K.DT[dt])
    p1, p2 = K.bn_params(C, 21 + C), K.bn_params(C, 31 + C)
    eps, mom = 1e-3, 0.03
    m1, m2 = module(C, eps, mom, p1), module(C, eps, mom, p2)
    a, b = dev(x1).requires_grad_(), dev(x2).requires_grad_()
    out = ops.bn2_act(a, m1, b, m2, True)
    mr = out.grad_fn.saved_tensors[6]
    out.backward(strided(dev(g)) if sg else dev(g))
    got = {'out': out.detach(), 'dx1': a.grad, 'dx2': b.grad}
    for i, m in enumerate((m1, m2)):
        got.update({f'dgamma{i + 1}': m.weight.grad, f'dbeta{i + 1}': m.bias.grad, f'mean{i + 1}': mr[i, :, 0], f'rstd{i + 1}': mr[i, :, 1],
                    f'running_mean{i + 1}': m.running_mean, f'running_var{i + 1}': m.running_var})
    K.bn_pair_assert(f'bn2[{dt},{N}x{C},ldgy={"2C" if sg else "C"}]', got, plan, x1, x2, p1, p2, g, eps, mom, 1)


# ------------------------------------------------------------------------------------------------ channels-last, segmented
@pytest.mark.parametrize('dt,C', K.SEG_CASES)
def test_bn_segmented_vs_fp64(ops, dt, C):
    """tamtr_bncl_act_seg_fwd / _bwd through ops.bn_cat_cl: three levels of three images written into one token memory; every level against
    the fp64 reference of its own BatchNorm, the output and the cotangent taken from their segments."""
    B, Ls, eps, mom = K.SEG_B, K.SEG_LS, 1e-5, 0.1
    Lt = sum(Ls)
    ins = [K.bn_rows(B * L, C, K.DT[dt], 'ordinary', 500 + L + C) for L in Ls]
    ps = [K.bn_params(C, 41 + i + C) for i in range(len(Ls))]
    cot = torch.cat([g.view(B, L, C) for (_, g), L in zip(ins, Ls)], 1)
    xs, ms = [dev(x).requires_grad_() for x, _ in ins], [module(C, eps, mom, p) for p in ps]
    assert ops.bn_cat_cl_ok(xs, ms)
    f = ops.bn_cat_cl(xs, ms, B)
    assert f.shape == (B, Lt, C)
    f.backward(dev(cot))
    at = 0
    for i, L in enumerate(Ls):
        plan = cl_plan(ops, B * L, C, K.DT[dt])
        got = {'out': f.detach()[:, at:at + L].reshape(B * L, C), 'dx': xs[i].grad, 'dgamma': ms[i].weight.grad, 'dbeta': ms[i].bias.grad,
               'running_mean': ms[i].running_mean, 'running_var': ms[i].running_var}
        K.bn_single_assert(f'bn_seg[{dt},C={C},level {i}: {B}x{L}]', got, 'cl', plan, *ins[i][:1], ps[i][0], ps[i][1], ins[i][1], eps, mom, ps[i][2], ps[i][3], 0)
        at += L


# ------------------------------------------------------------------------------------------------ the statistics alone
@pytest.mark.parametrize('dt,C,rows', [(dt, C, n) for dt in K.CL_C for C in K.CL_C[dt] for n in K.cl_rows(C, dt == 'bf16')])
def test_bn_stats_channels_last_vs_fp64(ops, dt, C, rows):
    """tamtr_bncl_stats through ops.bn_stats_cl: mean, rstd and the running statistics, ordinary rows and rows whose mean is 32 standard deviations."""
    N = K.cl_rows(C, dt == 'bf16')[rows]
    plan = cl_plan(ops, N, C, K.DT[dt])
    for kind in ('ordinary', 'offset'):
        x, _ = K.bn_rows(N, C, K.DT[dt], kind, 600 + C + N % 1000)
        p = K.bn_params(C, 11 + C)
        bn = module(C, 1e-3, 0.03, p)
        mr = ops.bn_stats_cl(dev(x), bn)
        got = {'mean': mr[:, 0], 'rstd': mr[:, 1], 'running_mean': bn.running_mean, 'running_var': bn.running_var}
        K.stats_assert(f'bn_stats[{dt},{N}x{C},{kind}]', got, 'cl', plan, x, 1e-3, 0.03, p[2], p[3])


def _finalize(ops, part, eps, mom, rm, rv):
    C, S = part.shape[:2]
    pd, rmd, rvd = dev(part).contiguous(), dev(rm), dev(rv)
    mr = torch.full((C, 2), float('nan'), device='cuda')
    ops.call('tamtr_bn_finalize', ops.ptr(pd), ops.ptr(mr), ops.ptr(rmd), ops.ptr(rvd), C, S, eps, mom, ops.stream_ptr())
    return {'mean': mr[:, 0], 'rstd': mr[:, 1], 'running_mean': rmd, 'running_var': rvd}


@pytest.mark.parametrize('S', K.FINALIZE_S)
def test_bn_finalize_on_hand_made_partials_vs_fp64(ops, S):
    """tamtr_bn_finalize (what conv3x3.hip's epilogue feeds) on (count, mean, M2) triples of unequal counts: the fp64 statistics of the rows
    behind them."""
    C, eps, mom = 3, 1e-3, 0.03
    part, data, counts = K.finalize_partials(S, C, ())
    _, _, rm, rv = K.bn_params(C, 50)
    K.finalize_assert(f'bn_finalize[S={S}]', _finalize(ops, part, eps, mom, rm, rv), S, counts, data, eps, mom, rm, rv)


@pytest.mark.parametrize('S,empty', [(5, (0,)), (5, (2,)), (300, (0,)), (300, (0, 150, 256))])
def test_bn_finalize_takes_an_empty_partial_as_a_no_op(ops, S, empty):
    """A (0, 0, 0) triple in the first position (a thread of combine_slices whose first triple is empty: 0 / 0 without the guard) and in the
    middle: the statistics are those of the other partials' rows."""
    C, eps, mom = 3, 1e-3, 0.03
    part, data, counts = K.finalize_partials(S, C, empty)
    assert all(float(part[:, s].abs().max()) == 0 for s in empty)
    _, _, rm, rv = K.bn_params(C, 50)
    K.finalize_assert(f'bn_finalize[S={S},empty={empty}]', _finalize(ops, part, eps, mom, rm, rv), S, counts, data, eps, mom, rm, rv)


# ------------------------------------------------------------------------------------------------ host branches of bn_act / _bn_train_call
def test_bn_act_cumulative_average_second_call(ops):
    """momentum=None: the cumulative moving average, 1 / num_batches_tracked; the second call moves the running statistics by 1 / 2.  The
    reference of the second call starts from the running statistics the first one left on the device."""
    B, C, HW, dt = 2, 3, 64, F32
    plan = nchw_plan(ops, B, C, HW, False)
    p = K.bn_params(C, 11 + C)
    bn = module(C, 1e-3, None, p)
    for call, mom in ((1, 1.0), (2, 0.5)):
        x, g = K.bn_rows(B * HW, C, dt, 'ordinary', 700 + call)
        rm, rv = bn.running_mean.detach().cpu().clone(), bn.running_var.detach().cpu().clone()
        bn.weight.grad = bn.bias.grad = None
        got = run_single(ops, dev(K.nchw(x, B, HW)).view(B, C, 8, 8), bn, 1, dev(K.nchw(g, B, HW)).view(B, C, 8, 8))
        assert int(bn.num_batches_tracked) == call
        K.bn_single_assert(f'bn[nchw,momentum=None,call {call}]', got, 'nchw', plan, x, p[0], p[1], g, 1e-3, mom, rm, rv, 1)


@pytest.mark.parametrize('layout', ('nchw', 'cl'))
def test_bn_act_without_running_statistics(ops, layout):
    """track_running_stats=False: NULL running pointers; out, the stored statistics and the gradients as with them."""
    B, C, HW, dt, eps = 2, 4, 64, BF16, 1e-5
    N = B * HW
    plan = nchw_plan(ops, B, C, HW, True) if layout == 'nchw' else cl_plan(ops, N, C, dt)
    x, g = K.bn_rows(N, C, dt, 'ordinary', 710)
    p = K.bn_params(C, 11 + C)
    bn = module(C, eps, 0.1, p, track=False)
    assert bn.running_mean is None
    if layout == 'nchw':
        got = run_single(ops, dev(K.nchw(x, B, HW)).view(B, C, 8, 8), bn, 1, dev(K.nchw(g, B, HW)).view(B, C, 8, 8))
    else:
        got = run_single(ops, dev(x), bn, 1, dev(g))
    K.bn_single_assert(f'bn[{layout},no running statistics]', got, layout, plan, x, p[0], p[1], g, eps, 0.1, None, None, 1)
