"""The MFMA linear (csrc/gemm_bf16.hip: the W-stationary, full-row and tile kernels behind tamtr_linear_bf16, and the backward of
ops.linear_bf16) and the x_proj kernels (csrc/xproj.hip, on fp32 and on bf16 planes) elementwise against fp64 references with an error
model (tests/ref64.py).  Shapes, seeded inputs, the dispatch restated and the assertions themselves: tests/gemm_cases.py
(tests/test_ref64_host.py runs the same assertions on CPU emulations and their mutants).

Each assertion is elementwise |got - ref| <= a 2^-8 |ref| + b mag with no free absolute term; a and b are counted in
ref64.linear_bounds / linear_grad_bounds / xproj_bounds.  Set TAMTR_REF64_REPORT=<file> to collect the worst err / bound ratio of every
assertion (profiles/r11_gemm_ref64.txt).

One kernel of csrc/gemm_bf16.hip has no test because no call can reach it: linear_bf16_n512_kernel (the 64-byte, 4-stage ring).  The
entry point refuses K % 64 != 0, and every K % 64 == 0 takes the branch that launches linear_bf16_n512_k64_kernel instead."""
import pytest
import torch

import gemm_cases as G
import ref64 as R

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import tamtr_amd.ops as ops
    return ops


def dev(t):
    return None if t is None else t.detach().cuda()


def nan_like(shape, dtype=F32):
    return torch.full(shape, float('nan'), device='cuda', dtype=dtype)


# ------------------------------------------------------------------------------------------------ tamtr_linear_bf16
def _linear_abi(ops, x, w, b):
    """The C entry point on a NaN-prefilled y, twice: the same bits both times."""
    M, K = x.shape
    N = w.shape[0]
    xd, wd, bd = dev(x), dev(w), dev(b)
    ys = [nan_like((M, N), BF16) for _ in range(2)]
    for y in ys:
        ops.call('tamtr_linear_bf16', ops.ptr(xd), ops.ptr(wd), ops.ptr(bd), ops.ptr(y), M, N, K, ops.stream_ptr())
    assert torch.equal(ys[0].view(torch.int16), ys[1].view(torch.int16)), 'a second call gives other bits'
    return ys[0]


@pytest.mark.parametrize('kernel,M,N,K,bias,what', G.LINEAR_CASES, ids=G.LINEAR_IDS)
def test_linear_kernels_vs_fp64(ops, kernel, M, N, K, bias, what):
    """linear_bf16_wstat_kernel<128 | 256 | 512>, linear_bf16_n512_k64_kernel and linear_bf16_kernel at the shapes of gemm_cases.LINEAR_CASES."""
    x, w, b, _ = G.linear_inputs(M, N, K, bias)
    G.linear_assert(f'linear[{kernel},{M}x{N}x{K}{"" if bias else ",no bias"}]', _linear_abi(ops, x, w, b), kernel, M, N, K, bias)


@pytest.mark.parametrize('kernel,M,N,K,inf_row', G.POISON_CASES, ids=[c[0] for c in G.POISON_CASES])
def test_linear_nan_and_inf_stay_in_their_rows(ops, kernel, M, N, K, inf_row):
    """A NaN in one element of the last valid row of X (the row that the tail of a partial block re-reads) and an Inf in another row:
    exactly those two rows of Y are non-finite.  Pins the fragment layout independently of the values."""
    x, w, b = G.poison_inputs(M, N, K, inf_row)
    G.poison_assert(f'linear[{kernel},{M}x{N}x{K}]', _linear_abi(ops, x, w, b), kernel, M, N, K, inf_row)


@pytest.mark.parametrize('kernel,M,N,K', G.EXACT_CASES, ids=[f'{c[0]}-{c[1]}x{c[2]}x{c[3]}' for c in G.EXACT_CASES])
def test_linear_is_exact_where_no_addition_rounds(ops, kernel, M, N, K):
    """Entries -1, 0, 1 and a bias of nine significant bits: every partial sum is exact in fp32 in any order, so every stored bit is
    decided - a dropped or doubled product, and a bias that lost its lo half (the ties of gemm_cases.exact_inputs), change bits."""
    x, w, b = G.exact_inputs(M, N, K)
    G.exact_assert(f'linear[{kernel},{M}x{N}x{K},exact]', _linear_abi(ops, x, w, b), kernel, M, N, K)


def _linear_op(ops, x, w, b, gy, idx=None):
    """ops.linear_bf16 (or _zero_rows) with a cotangent; the weight is an fp32 parameter holding bf16 values: dw comes back in fp32."""
    xd, wd, bd = dev(x).requires_grad_(), dev(w).float().requires_grad_(), dev(b).requires_grad_()
    y = ops.linear_bf16(xd, wd, bd) if idx is None else ops.linear_bf16_zero_rows(xd, wd, bd, dev(idx))
    y.backward(dev(gy))
    assert xd.grad.dtype == BF16 and wd.grad.dtype == F32 and bd.grad.dtype == F32
    return y.detach(), xd.grad, wd.grad, bd.grad


def _bmm_form(ops):
    form = {None: 'not decided (no call took more than one slice)', True: 'fp32 output', False: 'bf16 partials'}[ops._BMM_F32_OUT]
    R.note(f'dw_splitk: torch.bmm form of this build: {form}')
    return ops._BMM_F32_OUT is not False


@pytest.mark.parametrize('M,N,K,kdx,streams,S', G.GRAD_CASES, ids=[f'{c[0]}x{c[1]}x{c[2]}' for c in G.GRAD_CASES])
def test_linear_bf16_backward_vs_fp64(ops, M, N, K, kdx, streams, S):
    """dx on a second MFMA kernel (N and K exchanged) or on the library, db on the streaming kernel and on the direct slab_sum, dw in one
    slice and in several."""
    assert (G.dx_kernel(N, K), G.colsum_streams(M, N), G.split_count(M)) == (kdx, streams, S)
    assert ops._split_count(M) == S
    x, w, b, gy = G.linear_inputs(M, N, K, True, True)
    y, dx, dw, db = _linear_op(ops, x, w, b, gy)
    tag = f'linear_bf16[{M}x{N}x{K}]'
    G.linear_assert(tag, y, G.linear_kernel(N, K), M, N, K, True)
    G.grads_assert(tag, dx, dw, db, M, N, K, _bmm_form(ops))


def test_linear_bf16_zero_rows_vs_fp64(ops):
    B, L, N, K = G.ZERO_ROWS_CASE
    x, w, b, gy, idx, _ = G.zero_rows_inputs()
    y, dx, dw, db = _linear_op(ops, x, w, b, gy, idx)
    G.zero_rows_assert(f'linear_bf16_zero_rows[{B}x{L}x{N}x{K}]', y, dx, dw, db, 'n512_k64', _bmm_form(ops))


def _off(t, nbytes):
    """A device copy of t that starts nbytes into its own (16-byte aligned) buffer."""
    k = nbytes // t.element_size()
    buf = torch.empty(t.numel() + k, device='cuda', dtype=t.dtype)
    assert buf.data_ptr() % 16 == 0
    v = buf[k:].view(t.shape)
    v.copy_(t)
    return v


def test_linear_refuses_operands_off_16_byte_alignment_and_ops_copies_them(ops):
    """tamtr_linear_bf16 returns TAMTR_EUNSUP for X, W, Y or the bias off a 16-byte boundary before it launches anything (its kernels move
    16 bytes per request); ops.linear_bf16 copies such an operand and gives the aligned call's bits."""
    import tamtr_amd._lib as L_
    for kernel, M, N, K in (('wstat', 33, 256, 128), ('n512_k64', 33, 512, 64), ('tile', 33, 128, 64)):
        assert G.linear_kernel(N, K) == kernel
        x, w, b, _ = G.linear_inputs(M, N, K)
        good = [dev(x), dev(w), dev(b), nan_like((M, N), BF16)]
        # (the W-stationary kernel reads one float of the bias per lane: 4-byte alignment, which every fp32 tensor has, is all it needs)
        for which, nbytes in ((0, 2), (1, 2), (3, 2), (0, 8)) + (((2, 4),) if kernel != 'wstat' else ()):
            args = list(good)
            args[which] = _off(good[which], nbytes)
            y_before = args[3].clone()
            with pytest.raises(L_.TamtrHipError):
                ops.call('tamtr_linear_bf16', *(ops.ptr(t) for t in args), M, N, K, ops.stream_ptr())
            assert torch.equal(args[3].view(torch.int16), y_before.view(torch.int16)), 'y was written by a refused call'
        want = ops.linear_bf16(dev(x), dev(w).float(), dev(b))
        if kernel == 'wstat':                # ... and the entry point takes it there, with the aligned call's bits
            b4, y4 = _off(good[2], 4), nan_like((M, N), BF16)
            assert b4.data_ptr() % 16 == 4
            ops.call('tamtr_linear_bf16', ops.ptr(good[0]), ops.ptr(good[1]), ops.ptr(b4), ops.ptr(y4), M, N, K, ops.stream_ptr())
            assert torch.equal(y4.view(torch.int16), want.view(torch.int16))
        xo = _off(dev(x), 2)
        assert xo.is_contiguous() and xo.data_ptr() % 16 == 2
        got = ops.linear_bf16(xo, dev(w).float(), _off(dev(b), 4))
        assert torch.equal(got.view(torch.int16), want.view(torch.int16))
        G.linear_assert(f'linear_bf16[{kernel},{M}x{N}x{K},x + 2 bytes]', got, kernel, M, N, K, True)
        if G.dx_kernel(N, K) != 'lib':       # the cotangent off alignment too
            xg = dev(x).requires_grad_()
            y = ops.linear_bf16(xg, dev(w).float(), dev(b))
            gy = G.linear_inputs(M, N, K, True, True)[3]
            y.backward(_off(dev(gy), 2))
            a, bb, _ = R.linear_bounds(G.dx_kernel(N, K), M, K, N)
            R.check(f'linear_bf16[{kernel},{M}x{N}x{K},gy + 2 bytes] dx', xg.grad.float(), *G.linear_ref(M, N, K, True, True)['dx'], a, bb)


# ------------------------------------------------------------------------------------------------ x_proj
def _xproj_abi(ops, B, D, L, R_, plane_bf16):
    """The three entry points on NaN-prefilled outputs, twice each: the same bits both times.  Operands at their natural alignment."""
    import tamtr_amd._lib as L_
    i = {k: dev(v) for k, v in G.xproj_inputs(B, D, L, R_, plane_bf16).items()}
    pc, pdt = (1, BF16) if plane_bf16 else (0, F32)
    C = R_ + 2 * R.XP_N
    KS, MB = G.xproj_ks_mb(R_)
    wcat = ops.xproj_pack_weight(i['wx'])
    wT = ops.xproj_pack_weight_t(wcat, C)
    assert tuple(wcat.shape) == (2, 32 * MB, D) and tuple(wT.shape) == (2, D, 16 * KS)
    assert not bool(wcat[:, 2 * C:].any()) and not bool(wT[:, :, 2 * C:].any())
    sp, p = ops.stream_ptr(), ops.ptr
    runs = []
    nsl = L_.lib().tamtr_xproj_dw_slices(L)
    assert nsl == R.xproj_slices(L)
    n_part = B * nsl * 2 * 2 * C * D
    for _ in range(2):
        dtr, Bs, Cs = nan_like((B, 4, R_, L)), nan_like((B, 4, R.XP_N, L)), nan_like((B, 4, R.XP_N, L))
        ops.call('tamtr_xproj_fwd', p(i['u2']), p(wcat), p(dtr), p(Bs), p(Cs), B, D, L, R_, pc, sp)
        gu2 = nan_like((B, 2, D, L), pdt)
        ops.call('tamtr_xproj_bwd_dx', p(i['gu']), p(i['gdtr']), p(i['gB']), p(i['gC']), p(wT), p(gu2), B, D, L, R_, pc, sp)
        buf = nan_like((n_part + 2 * C * D,))                       # the partial tiles and a guard of one copy's size behind them
        ops.call('tamtr_xproj_bwd_dw', p(i['u2']), p(i['gdtr']), p(i['gB']), p(i['gC']), p(buf), B, D, L, R_, pc, sp)
        assert bool(torch.isnan(buf[n_part:]).all()), 'the weight gradient wrote behind its partial tiles'
        part = buf[:n_part].view(B * nsl, 2, 2 * C, D)
        runs.append({'dtr': dtr, 'Bs': Bs, 'Cs': Cs, 'gu2': gu2, 'part': part, 'dw': ops.slab_sum(part)})
    for n in runs[0]:
        a, b = runs[0][n], runs[1][n]
        assert torch.equal(a.view(torch.int16) if a.dtype == BF16 else a.view(torch.int32), b.view(torch.int16) if b.dtype == BF16 else b.view(torch.int32)), \
            f'{n}: a second call gives other bits'
    return runs[0]


@pytest.mark.parametrize('planes', ['fp32', 'bf16'])
@pytest.mark.parametrize('B,D,L,R_,what', G.XPROJ_CASES, ids=[f'{c[0]}x{c[1]}x{c[2]}-R{c[3]}' for c in G.XPROJ_CASES])
def test_xproj_kernels_vs_fp64(ops, B, D, L, R_, what, planes):
    """xproj_fwd_kernel<MB> / xproj_bwd_dx_kernel<KS> / xproj_bwd_dw_kernel<MB, false> on fp32 planes and xproj_fwd16_kernel<MB> /
    xproj_bwd_dx16_kernel<KS> / xproj_bwd_dw_kernel<MB, true> on bf16 planes, each against fp64 on its own."""
    assert G.xproj_ks_mb(R_) == G.XPROJ_KS_MB[[c[:4] for c in G.XPROJ_CASES].index((B, D, L, R_))]
    assert ops.xproj_ok(BF16, D, L, R_, R.XP_N)
    pb = planes == 'bf16'
    G.xproj_assert(f'xproj[{planes},{B}x{D}x{L},R={R_}]', _xproj_abi(ops, B, D, L, R_, pb), B, D, L, R_, pb)
