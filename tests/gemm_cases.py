"""Shapes, seeded inputs, the host dispatch restated, and the assertions of the MFMA linear (csrc/gemm_bf16.hip) and x_proj (csrc/xproj.hip)
checks against fp64.  tests/test_gpu_gemm_ref64.py feeds the assertions the kernels' outputs, tests/test_ref64_host.py feeds them fp32 CPU
emulations of the kernels (which must pass) and mutants of those (which must fail).

Every assertion is ref64.check(): |got - ref| <= a 2^-8 |ref| + b mag, a and b counted in ref64.linear_bounds / linear_grad_bounds /
xproj_bounds.

Not covered, because nothing can reach it: linear_bf16_n512_kernel (the 64-byte, 4-stage ring).  tamtr_linear_bf16 refuses K % 64 != 0
before the `K % 64 == 0` branch that launches linear_bf16_n512_k64_kernel in its place, so that branch is always taken."""
import functools

import torch

import ref64 as R
from weights import rnd

F32, BF16 = torch.float32, torch.bfloat16


# ================================================================================================ MFMA linear
def linear_kernel(N, K):
    """The kernel tamtr_linear_bf16 launches for (N, K) (it takes K % 64 == 0 and N % 128 == 0 only):
      K in (128, 256, 512), N % 256 == 0 and N / 256 divides 32 -> linear_bf16_wstat_kernel<K>   ('wstat')
      else N % 512 == 0                                          -> linear_bf16_n512_k64_kernel   ('n512_k64')
      else                                                       -> linear_bf16_kernel            ('tile')"""
    assert K % 64 == 0 and N % 128 == 0, 'tamtr_linear_bf16 returns TAMTR_EUNSUP'
    if K in (128, 256, 512) and N % 256 == 0 and 32 % (N // 256) == 0:
        return 'wstat'
    return 'n512_k64' if N % 512 == 0 else 'tile'


def dx_kernel(N, K):
    """ops._linear_bf16_dx for a weight [N, K]: the MFMA entry point with N and K exchanged where K % 128 == 0 and N % 64 == 0, else the
    library ('lib')."""
    return linear_kernel(K, N) if K % 128 == 0 and N % 64 == 0 else 'lib'


def split_count(M, min_rows=2048, max_split=64):
    """ops._split_count: the slices of dw_splitk."""
    S = 1
    while S < max_split and M % (2 * S) == 0 and M // (2 * S) >= min_rows:
        S *= 2
    return S


def colsum_streams(M, N):
    """ops.colsum: the streaming kernel (True) or the direct slab_sum (False)."""
    return M >= 4096 and N % 8 == 0 and N <= 2048 and 256 % (N // 8) == 0


# (kernel, M, N, K, bias, what it reaches)
LINEAR_CASES = [
    ('wstat', 1, 256, 128, True, 'single row'),
    ('wstat', 33, 2048, 128, True, 'ncol 8, 32 workers: workers with 0 and with 1 block'),
    ('wstat', 3077, 2048, 128, True, '3 and 4 blocks per worker in one launch'),
    ('wstat', 5151, 2048, 128, True, '5 and 6 blocks per worker'),
    ('wstat', 8193, 256, 256, True, 'ncol 1, 256 workers, 1 and 2 blocks, a one-row tail block'),
    ('wstat', 1000, 512, 512, True, 'K = 512 fragments, ncol 2, ragged tail'),
    ('wstat', 97, 4096, 128, False, 'ncol 16'),
    ('wstat', 1025, 8192, 128, True, 'ncol 32, 8 workers, 4 and 5 blocks'),
    ('n512_k64', 1, 512, 64, True, 'single row'),
    ('n512_k64', 128, 512, 64, False, 'nk = 1, exactly one tile'),
    ('n512_k64', 130, 512, 192, True, 'odd nk, tail tile of 2 rows: the is_lim path'),
    ('n512_k64', 77, 1024, 64, True, 'nbl = 2, M < TM'),
    ('n512_k64', 300, 1536, 256, True, 'nbl = 3, a K that wstat would take at another N'),
    ('n512_k64', 129, 512, 1024, True, 'nk = 16'),
    ('n512_k64', 8200, 2048, 64, True, '260 tiles on 256 workgroups: four run a second tile; a ragged last tile'),
    ('tile', 1, 128, 64, True, 'single row'),
    ('tile', 127, 384, 320, True, 'M < BM, nk = 5'),
    ('tile', 1033, 128, 128, True, 'm_blocks = 9, rounded to 16 panels with 7 idle'),
    ('tile', 2048, 128, 64, False, 'full tiles, nk = 1'),
    ('tile', 77, 256, 192, True, 'ragged rows, nk = 3'),
]
LINEAR_IDS = [f'{k}-{M}x{N}x{K}' for k, M, N, K, _, _ in LINEAR_CASES]

# one case per kernel with a NaN in one element of the LAST valid row of X (the row the tail re-reads) and an Inf in another row
POISON_CASES = [('wstat', 1000, 512, 512, 500), ('n512_k64', 130, 512, 192, 3), ('tile', 77, 256, 192, 40)]      # (..., the Inf's row)

# through ops.linear_bf16 with a cotangent: (M, N, K, kernel of dx, db streams, slices of dw)
GRAD_CASES = [
    (1000, 512, 512, 'wstat', False, 1),       # dx on the W-stationary kernel
    (300, 1536, 256, 'tile', False, 1),        # dx [300, 256] over K' = 1536: the tile kernel with nk = 24
    (130, 384, 512, 'n512_k64', False, 1),     # dx [130, 512] over K' = 384: the full-row kernel (the forward is the tile kernel)
    (127, 384, 320, 'lib', False, 1),          # K % 128 != 0: the library
    (8193, 256, 256, 'wstat', True, 1),        # db on the streaming kernel; an odd M is one slice
    (8200, 2048, 64, 'lib', True, 4),          # dw in 4 slices
]
ZERO_ROWS_CASE = (2, 65, 512, 192)             # B, L, N, K: n512_k64, idx holds the first and the last row of an image


def linear_seed(M, N, K):
    return 7000 + 13 * M + 3 * N + K


@functools.lru_cache(maxsize=None)
def linear_inputs(M, N, K, bias=True, grad=False):
    """x bf16 [M, K], w bf16 [N, K] (scaled K^-0.5: products of about 1), bias fp32 [N] of about 1 (or None), gy bf16 [M, N] (or None).
    Cached and shared: do not write to them."""
    s = linear_seed(M, N, K)
    return (rnd((M, K), s).to(BF16), rnd((N, K), s + 1, K ** -0.5).to(BF16), rnd((N,), s + 2) if bias else None,
            rnd((M, N), s + 3).to(BF16) if grad else None)


@functools.lru_cache(maxsize=None)
def linear_ref(M, N, K, bias=True, grad=False):
    return R.linear(*linear_inputs(M, N, K, bias, grad))


def linear_assert(tag, y, kernel, M, N, K, bias):
    """y [M, N] of the kernel `kernel` against fp64 under ref64.linear_bounds.  Returns the worst ratio."""
    assert linear_kernel(N, K) == kernel, f'{tag}: tamtr_linear_bf16 sends (N, K) = ({N}, {K}) to {linear_kernel(N, K)}, the case is listed for {kernel}'
    assert y.dtype == BF16 and tuple(y.shape) == (M, N)
    return R.linear_check(f'{tag} y', y.float(), linear_ref(M, N, K, bias), kernel, K)


def poison_inputs(M, N, K, inf_row):
    x, w, b, _ = linear_inputs(M, N, K)
    x = x.clone()
    x[M - 1, K // 3] = float('nan')
    x[inf_row, K - 1] = float('inf')
    return x, w, b


def poison_assert(tag, y, kernel, M, N, K, inf_row):
    """Row M - 1 of y is NaN (check()'s NaN rule).  Row inf_row is compared by pattern with the fp64 reference, column by column: +Inf
    where the weight that meets the Inf is positive, -Inf where it is negative, NaN where it is 0 (Inf * 0) - so a NaN that leaks into
    the row from the poisoned last row, or an Inf of the wrong sign, fails.  Every other row is finite and within the bound."""
    x, w, b = poison_inputs(M, N, K, inf_row)
    ref = R.linear(x, w, b)
    ry = ref['y'][0]
    bad = ~torch.isfinite(ry)
    assert bool(torch.isnan(ry[M - 1]).all()) and bool(bad[inf_row].all()) and int(bad.any(1).sum()) == 2
    assert bool(torch.isposinf(ry[inf_row]).any()) and bool(torch.isneginf(ry[inf_row]).any())        # (both signs are in the row)
    yf = y.float().cpu()
    for name, f in (('+Inf', torch.isposinf), ('-Inf', torch.isneginf), ('NaN', torch.isnan)):
        diff = f(yf[inf_row]) != f(ry[inf_row])
        assert not bool(diff.any()), f'{tag}: the {name} pattern of row {inf_row} differs from the reference in {int(diff.sum())} of {N} columns'
    keep = torch.arange(M) != inf_row
    cut = {'y': (ry[keep], ref['y'][1][keep]), 'bias': ref['bias'][keep]}
    return R.linear_check(f'{tag} y (NaN in row {M - 1}, Inf in row {inf_row})', yf[keep], cut, kernel, K)


# ---- exact arithmetic: operands for which no addition rounds, so that the one rounding left - the store to bf16 - decides every bit
EXACT_CASES = [('wstat', 1000, 512, 512), ('wstat', 3077, 2048, 128), ('n512_k64', 130, 512, 192), ('n512_k64', 8200, 2048, 64), ('tile', 1033, 128, 128)]


@functools.lru_cache(maxsize=None)
def exact_inputs(M, N, K):
    """x and w with entries -1, 0, 1 (a quarter, a half, a quarter): every product and every partial sum is a small integer.  The bias of
    column n is 2^(k - 8) (1 + 2^-8), k = n % 6: nine significant bits, so bf16(b) = 2^(k - 8) (a tie, to even), b - bf16(b) = 2^(k - 16) is a
    bf16 value too, and hi + lo is b exactly.  For an integer sum s in [2^k, 2^(k + 1)) the value s + 2^(k - 8) lies exactly between two
    bf16 neighbours: with the lo half it rounds up, without it to even - such elements see a lost lo half in the stored bits."""
    def tern(shape, seed):
        t = rnd(shape, seed)
        return ((t > 0.6745).float() - (t < -0.6745).float()).to(BF16)
    s = linear_seed(M, N, K) + 50000
    return tern((M, K), s), tern((N, K), s + 1), 2.0 ** ((torch.arange(N) % 6).float() - 8) * (1 + 2.0 ** -8)


def exact_want(M, N, K, lo=True):
    """bf16(s + b), computed without any rounding before the last one; lo=False: what a bias of bf16(b) alone gives."""
    x, w, b = exact_inputs(M, N, K)
    s = x.double() @ w.double().t()
    assert float(s.abs().max()) < 128, 'the premise: integer sums of at most 7 bits'
    v = s + (b.double() if lo else b.to(BF16).double())
    assert torch.equal(v.float().double(), v), 'the premise: s + b is an fp32 value (7 + 16 bits)'
    return v.float().to(BF16)


def exact_assert(tag, y, kernel, M, N, K):
    """y is bf16(s + b) bit for bit, whatever the order of the additions: none of them rounds (integers below 2^7 next to a bias whose
    last bit is 2^-16 at least: 23 bits).  Holds for all three kernels, the W-stationary one included: its hi + lo is b exactly."""
    assert linear_kernel(N, K) == kernel
    want = exact_want(M, N, K)
    n_tie = int((want != exact_want(M, N, K, lo=False)).sum())
    assert n_tie > 0, 'no element of this case would see a lost lo half'
    bad = y.cpu() != want
    assert not bool(bad.any()), f'{tag}: {int(bad.sum())} of {bad.numel()} elements are not the exact result rounded once (first at {bad.nonzero()[0].tolist()})'
    return n_tie


def grads_assert(tag, dx, dw, db, M, N, K, bmm_f32_out, ref=None, dw_extra=None):
    """dx bf16 [M, K], dw fp32 [N, K], db fp32 [N] of ops.linear_bf16 against fp64.  dx from an MFMA kernel: that kernel's bound with N
    and K exchanged; everything else: ref64.linear_grad_bounds.  dw_extra = (magnitude, b): one more term of dw's bound (zero_rows)."""
    ref = ref or linear_ref(M, N, K, True, True)
    kdx, S = dx_kernel(N, K), split_count(M)
    ab = R.linear_grad_bounds(M, N, K, S, bmm_f32_out, colsum_streams(M, N))
    worst = {}
    if kdx == 'lib':
        worst['dx'] = R.check(f'{tag} dx (library)', dx.float(), *ref['dx'], *ab['dx'])
    else:
        a, b, _ = R.linear_bounds(kdx, M, K, N)
        worst['dx'] = R.check(f'{tag} dx ({kdx})', dx.float(), *ref['dx'], a, b)
    worst['db'] = R.check(f'{tag} db ({"streaming" if colsum_streams(M, N) else "slab_sum"})', db, *ref['db'], *ab['db'])
    a, b = ab['dw']
    mag = ref['dw'][1]
    if dw_extra is not None:
        mag = b * mag + dw_extra[1] * dw_extra[0]
        a, b = 0, 1.0          # (the rounding of the S = 1 product is relative to that product, not to the difference: it is inside dw_extra)
    worst['dw'] = R.check(f'{tag} dw (S = {S})', dw, ref['dw'][0], mag, a, b)
    return worst


def zero_rows_inputs():
    """x [B, L, K], w, bias, gy [B, L, N], idx (the first and the last row of an image and one between), and x with those rows zeroed."""
    B, L, N, K = ZERO_ROWS_CASE
    x, w, b, gy = linear_inputs(B * L, N, K, True, True)
    idx = torch.tensor([0, L // 2, L - 1])
    xz = x.view(B, L, K).clone()
    xz[:, idx] = 0
    return x.view(B, L, K), w, b, gy.view(B, L, N), idx, xz


def zero_rows_assert(tag, y, dx, dw, db, kernel, bmm_f32_out):
    """ops.linear_bf16_zero_rows against the reference of the input with the rows idx zeroed.  The masked rows of y are bf16(bias) exactly
    and those of dx exactly 0.  dw is formed as (dw of all rows) - (dw of the masked rows), both library products rounded to bf16 before
    the fp32 subtraction: next to the usual bound it carries 2^-8 of each product's magnitude, |gy|^T |x| over all rows (the first) and
    over the masked rows (the second) - together at most twice the unmasked magnitude."""
    B, L, N, K = ZERO_ROWS_CASE
    x, w, b, gy, idx, xz = zero_rows_inputs()
    assert linear_kernel(N, K) == kernel
    ref = R.linear(xz.reshape(B * L, K), w, b, gy.reshape(B * L, N))
    worst = {'y': R.linear_check(f'{tag} y', y.float().reshape(B * L, N), ref, kernel, K)}
    assert torch.equal(y.cpu()[:, idx], b.to(BF16).expand(B, idx.numel(), N)), f'{tag}: masked rows of y are not bf16(bias)'
    # dx of the reference is gy w for every row: the masked rows are zeroed afterwards
    rdx, mdx = ref['dx'][0].view(B, L, K).clone(), ref['dx'][1].view(B, L, K).clone()
    rdx[:, idx] = 0
    mdx[:, idx] = 0
    ref['dx'] = (rdx.view(B * L, K), mdx.view(B * L, K))
    assert float(dx.float()[:, idx].abs().max()) == 0, f'{tag}: masked rows of dx are not 0'
    m_all = R._d(gy).abs().reshape(B * L, N).t() @ R._d(x).abs().reshape(B * L, K)
    worst.update(grads_assert(tag, dx.reshape(B * L, K), dw, db, B * L, N, K, bmm_f32_out, ref=ref, dw_extra=(2 * m_all, R.U8)))
    return worst


# ================================================================================================ x_proj
# tamtr_xproj_fwd / _bwd_dx / _bwd_dw restated: C = R + 32 rows per direction, 2C rows per stored copy;
#   forward and dW: MB = ceil(2C / 32) row blocks (3 | 4) -> xproj_fwd_kernel<MB> | xproj_fwd16_kernel<MB>, xproj_bwd_dw_kernel<MB, planes bf16>
#   d/d(u2):        KS = ceil(2C / 16) k-steps (5 .. 8)   -> xproj_bwd_dx_kernel<KS> | xproj_bwd_dx16_kernel<KS>
#   fp32 planes: a wave owns 32 pixels, a workgroup 128; bf16 planes: 64 and 256.  dW: one partial tile per (image, 1 024-pixel slice).
XPROJ_CASES = [
    (2, 256, 8, 5, 'less than one wave of pixels; 2C = 74: padding rows and columns; odd R'),
    (2, 256, 40, 8, 'ragged against 32 and against 64; KS 5, MB 3'),
    (1, 512, 72, 12, 'KS 6 with 2C = 88'),
    (2, 256, 1032, 16, 'two dW slices, the second one 8 pixels long'),
    (1, 256, 136, 20, 'KS 7, MB 4, 2C = 104'),
    (1, 512, 264, 32, 'KS 8; more than one block of 256 pixels on bf16 planes'),
]
XPROJ_KS_MB = [(5, 3), (5, 3), (6, 3), (6, 3), (7, 4), (8, 4)]


def xproj_ks_mb(R_):
    C2 = 2 * (R_ + 2 * R.XP_N)
    return (C2 + 15) // 16, (C2 + 31) // 32


@functools.lru_cache(maxsize=None)
def xproj_inputs(B, D, L, R_, plane_bf16):
    """u2 [B, 2, D, L] and gu [B, 4, D, L] in the plane dtype, wx fp32 [4, C, D] (scaled D^-0.5), gdtr, gB, gC fp32.  Cached: do not write."""
    pdt = BF16 if plane_bf16 else F32
    s = 9000 + 5 * D + L + 100 * R_
    C = R_ + 2 * R.XP_N
    return {'u2': rnd((B, 2, D, L), s).to(pdt), 'wx': rnd((4, C, D), s + 1, D ** -0.5), 'gdtr': rnd((B, 4, R_, L), s + 2),
            'gB': rnd((B, 4, R.XP_N, L), s + 3), 'gC': rnd((B, 4, R.XP_N, L), s + 4), 'gu': rnd((B, 4, D, L), s + 5).to(pdt)}


@functools.lru_cache(maxsize=None)
def xproj_ref(B, D, L, R_, plane_bf16):
    i = xproj_inputs(B, D, L, R_, plane_bf16)
    return R.xproj(i['u2'], i['wx'], R_, i['gdtr'], i['gB'], i['gC'], i['gu'], plane_bf16)


def is_bf16_value(t):
    t = t.detach().cpu().float()
    return torch.equal(t.bfloat16().float(), t)


def xproj_assert(tag, got, B, D, L, R_, plane_bf16, ref=None):
    """got: dict with any of dtr, Bs, Cs (fp32, each value a bf16 value), gu2 (plane dtype), part (fp32 [B * slices, 2, 2C, D]: the
    partial tiles, every element written; it has 2C rows per copy - the accumulator rows beyond 2C, whose gradient rows the kernel zeroes,
    are never stored) and dw (fp32 [2, 2C, D]: their ordered sum)."""
    ref = ref or xproj_ref(B, D, L, R_, plane_bf16)
    ab = R.xproj_bounds(B, D, L, plane_bf16)
    worst = {}
    for n in ('dtr', 'Bs', 'Cs'):
        if n in got:
            assert got[n].dtype == F32 and is_bf16_value(got[n]), f'{tag} {n}: a stored value is not a bf16 value'
            worst[n] = R.check(f'{tag} {n}', got[n], *ref[n], *ab[n])
    if 'gu2' in got:
        assert got['gu2'].dtype == (BF16 if plane_bf16 else F32)
        worst['gu2'] = R.check(f'{tag} gu2', got['gu2'].float(), *ref['gu2'], *ab['gu2'])
    if 'part' in got:
        C2 = 2 * (R_ + 2 * R.XP_N)
        assert tuple(got['part'].shape) == (B * R.xproj_slices(L), 2, C2, D)
        assert bool(torch.isfinite(got['part']).all()), f'{tag}: unwritten elements in the partial tiles'
    if 'dw' in got:
        worst['dw'] = R.check(f'{tag} dw', got['dw'], *ref['dw'], *ab['dw'])
    return worst
