"""Shapes, seeded inputs, the host dispatch restated, and the assertions of the LayerNorm, cross-merge and depthwise SS2D checks against fp64
(csrc/ss2d_out.hip, csrc/dwconv.hip).  tests/test_gpu_ss2d_ref64.py feeds the assertions the kernels' outputs, tests/test_ref64_host.py
feeds them fp32 CPU emulations of the kernels (which must pass) and mutants of those (which must fail).

Every assertion is ref64.check(): |got - ref| <= a 2^-8 |ref| + b mag, a and b counted in ref64.layer_norm_bounds / dwconv_bounds."""
import torch

import ref64 as R
from weights import rnd

F32, BF16 = torch.float32, torch.bfloat16
DT = {'fp32': F32, 'bf16': BF16}


def dtn(dt):
    return 'bf16' if dt == BF16 else 'fp32'


# ================================================================================================ LayerNorm
# Dispatch of tamtr_layernorm_fwd / _bwd (ss2d_out.hip), restated:
#   bf16 and D in (64, 128) and x, out (fwd) / x, gout, gx (bwd), gamma, beta 16-byte aligned -> ln_fwd_narrow_kernel<D> / ln_bwd_narrow_kernel<D>
#     (D / 8 lanes per token, 64 / (D / 8) = 8 | 4 token slots per wave, 32 | 16 per forward workgroup; slots past ntok clamp to ntok - 1)
#   everything else -> ln_fwd_kernel<T, D> / ln_bwd_kernel<T, D> (a wave per token, 4 tokens per forward workgroup)
#   backward, both: a workgroup walks 64 tokens (4 waves x 16) and writes one row of the d(gamma) / d(beta) partials.
LN_D = {'fp32': (32, 64, 128, 256, 512, 1024), 'bf16': (64, 128, 256, 512, 1024)}
LN_NTOK = (1, 63, 64, 65, 211)      # 1: fewer tokens than one wave's slots; 64 | 65: exactly one backward workgroup | one token more; 63, 211: partial last ones
LN_KINDS = ('ordinary', 'offset')   # 2 randn + 0.5 (the old test's rows) | 8 + 0.25 randn (the mean is 32 standard deviations: the two-pass mean's cancellation)
LN_OFFSET_D = (64, 128)             # bf16, every operand 8 bytes into its buffer: the narrow kernels' alignment fall-back
LN_OFFSET_NTOK = 65
LN_GATE_F32 = [(D, n) for D in (64, 256, 1024) for n in (1, 77)]


def ln_kernels(D, bf16, aligned=True):
    """The kernels tamtr_layernorm_fwd / _bwd launch for this call."""
    if bf16 and D in (64, 128) and aligned:
        return f'ln_fwd_narrow_kernel<{D}>', f'ln_bwd_narrow_kernel<{D}>'
    t = 'bf16_t' if bf16 else 'float'
    return f'ln_fwd_kernel<{t}, {D}>', f'ln_bwd_kernel<{t}, {D}>'


def ln_inputs(D, ntok, dt, kind):
    """x, gamma, beta, gout: x and gout in dt, on the CPU."""
    seed = 1000 + 7 * D + ntok + (0 if kind == 'ordinary' else 500)
    r = rnd((ntok, D), seed)
    x = (2 * r + 0.5) if kind == 'ordinary' else (8 + 0.25 * r)
    return x.to(dt), 1 + 0.2 * rnd((D,), seed + 1), 0.1 * rnd((D,), seed + 2), rnd((ntok, D), seed + 3).to(dt)


def ln_assert(tag, got, x, gamma, beta, gout, eps=1e-5):
    """got = (out, dx, dgamma, dbeta) against ref64.layer_norm under ref64.layer_norm_bounds.  Returns {name: worst ratio}."""
    ref = R.layer_norm(x, gamma, beta, gout, eps)
    # out 28 + 1, dx 2 * 28 + 28; dgamma 28 + 16 (tokens of a wave) + 4 (waves) + ceil(ntok / 64) (slab_sum), dbeta the same without xhat's 28
    ab = R.layer_norm_bounds(x.shape[0], x.dtype == BF16)
    return {n: R.check(f'{tag} {n}', t.float(), *ref[n], *ab[n]) for n, t in zip(('out', 'dx', 'dgamma', 'dbeta'), got)}


def ln_constant_inputs(D, ntok, dt, flat_cotangent):
    """Rows of one value each (multiples of 0.25: every partial sum is exact, so mean == the value and xhat == 0 in fp32 as in fp64).
    LayerNorm's Jacobian at such a row is (I - 1 1^T / D) / sqrt(eps), not 0: dx = rstd (gout gamma - mean(gout gamma)), which is 0
    exactly where gout gamma is constant along the row.  flat_cotangent: gamma = 1.5 and gout one value per row (multiples of 0.125), so
    dx == 0; otherwise the ordinary gamma and gout, and dx is held to its bound."""
    rows = torch.arange(ntok, dtype=torch.float32).view(ntok, 1)
    x = (((rows % 13) - 6) * 0.25 + 0.25).expand(ntok, D).contiguous().to(dt)
    beta = 0.1 * rnd((D,), 40 + D)
    if flat_cotangent:
        return x, torch.full((D,), 1.5), beta, (((rows % 5) - 2) * 0.125 + 0.125).expand(ntok, D).contiguous().to(dt)
    return x, 1 + 0.2 * rnd((D,), 41 + D), beta, rnd((ntok, D), 42 + D).to(dt)


def ln_constant_assert(tag, got, x, gamma, beta, gout, flat_cotangent):
    out, dx, dgamma, dbeta = got
    assert torch.equal(out.cpu(), beta.to(x.dtype).expand_as(x)), f'{tag}: out of a constant row is not beta'
    if flat_cotangent:
        assert float(dx.float().abs().max()) == 0, f'{tag}: dx of a constant row under a flat cotangent is not 0'
        assert float(dgamma.abs().max()) == 0, f'{tag}: dgamma (xhat == 0)'
    return ln_assert(tag, got, x, gamma, beta, gout)


def ln_gate_inputs(D, ntok):
    """x, xz, gamma, beta, gout of ln_gate in fp32 (the generators of test_ln_gate_bf16_vs_fp64 without the rounding to bf16)."""
    return (rnd((ntok, D), 170 + D) * 1.5 + 0.3, rnd((ntok, 2 * D), 171 + D), 1 + 0.2 * rnd((D,), 172), 0.1 * rnd((D,), 173), rnd((ntok, D), 174 + D))


def ln_gate_assert(tag, got, x, xz, gamma, beta, gout):
    """got = (out, dx, dz, dgamma, dbeta), all fp32."""
    ref = R.ln_gate(x, xz, gamma, beta, gout)
    ab = R.ln_gate_f32_bounds(x.shape[0])
    return {n: R.check(f'{tag} {n}', t, *ref[n], *ab[n]) for n, t in zip(('out', 'dx', 'dz', 'dgamma', 'dbeta'), got)}


# ================================================================================================ cross-merge
# Dispatch of tamtr_cross_merge_fwd / _bwd (ss2d_out.hip), restated:
#   fp32 planes                                                      -> cross_merge_fwd_kernel<float> / cross_merge_bwd_kernel<float> (16 x 16 pixel x 32 channel tiles)
#   bf16 planes, H and W even, plane % 4 == 0, token-major map % 16 == 0 -> forward: cross_merge_fwd16_kernel (32 x 32 pixel x 16 channel tiles, pixel pairs)
#     and, backward only, the 32 x 32 tiles overhang the map by at most 25 %  -> cross_merge_bwd16_kernel
#   bf16 planes otherwise                                            -> cross_merge_fwd_kernel<bf16_t> / cross_merge_bwd_kernel<bf16_t>
CM_B, CM_D = 2, (32, 64)
CM_GENERIC = [(1, 1), (16, 16), (17, 16), (13, 21), (5, 40), (33, 31)]        # fp32 planes: one pixel, one tile, partial tiles both ways, more than one tile
CM_FWD_BF16_GENERIC = [(15, 8), (13, 21), (1, 8)]                             # H or W odd
CM_FWD16 = [(2, 2), (32, 32), (34, 30), (64, 52), (6, 40)]                    # one pixel pair, one tile, a 2-row second tile, 2 x 2 tiles, two tiles along w
CM_BWD16 = [(32, 32), (32, 28), (26, 32), (64, 52)]                           # overhang 0, 14 %, 23 %, 23 % (2 x 2 tiles)
CM_BWD16_D32_ONLY = [(80, 80)]                                                # 3 x 3 tiles of 32 cover 96^2 = 1.44 x the map: the predicate is false, the generic kernel runs
CM_BWD_BF16_GENERIC = [(2, 2), (34, 30), (24, 40)]                            # even maps whose 32 x 32 tiles overhang by more than 25 %
CM_MISALIGNED_FWD, CM_MISALIGNED_BWD = (34, 30), (32, 32)                     # the plane 2 bytes off: would be fwd16 / bwd16, must take the generic kernels


def cm_fwd_kernel(H, W, bf16, aligned=True):
    if not bf16:
        return 'cross_merge_fwd_kernel<float>'
    return 'cross_merge_fwd16_kernel' if H % 2 == 0 and W % 2 == 0 and aligned else 'cross_merge_fwd_kernel<bf16_t>'


def cm_bwd_kernel(H, W, bf16, aligned=True):
    if not bf16:
        return 'cross_merge_bwd_kernel<float>'
    t = ((W + 31) // 32) * ((H + 31) // 32)
    return 'cross_merge_bwd16_kernel' if H % 2 == 0 and W % 2 == 0 and aligned and t * 32 * 32 * 4 <= H * W * 5 else 'cross_merge_bwd_kernel<bf16_t>'


def cm_inputs(D, H, W, dt):
    """The four scan planes y4 [B, 4, D, L] in dt and the token-major cotangent g [B, L, D] fp32."""
    L = H * W
    return rnd((CM_B, 4, D, L), 300 + D + L).to(dt), rnd((CM_B, L, D), 301 + D + L)


def cm_assert(tag, ymT, g2, y4, g, H, W):
    """The forward against fp64 (three fp32 additions: (y0 + y2) + (y1 + y3), a = 0, b = fp32_b(3)); the backward is data movement: fp32
    planes equal the adjoint's gather, bf16 planes equal it rounded to nearest-even.  Either output may be None."""
    worst = None
    if ymT is not None:
        worst = R.check(f'{tag} fwd', ymT, *R.cross_merge(y4, H, W), 0, R.fp32_b(3))
    if g2 is not None:
        assert not bool(torch.isnan(g2.float()).any()), f'{tag} bwd: unwritten elements'
        assert torch.equal(g2.cpu(), R.cross_merge_adjoint(g, H, W).to(g2.dtype)), f'{tag} bwd: not the adjoint\'s gather'
    return worst


# ================================================================================================ depthwise front end
# tamtr_dwconv_silu_cross_fwd / _bwd (dwconv.hip), restated: one kernel each per (activation dtype, plane dtype); 16 x 16 pixel tiles
# (x 32 channels forward, x 16 backward).  The backward reads the gradient planes with aligned 4-pixel vector loads when H % 4 == 0 and
# W % 4 == 0 (six vectors cover [w0 - 4, w0 + 20) of a tile row), else pixel by pixel.
DW_B, DW_D = 2, (32, 64)
DW_SHAPES = [(1, 1), (3, 3),     # a map smaller than the 3 x 3 window; every pixel on the border
             (4, 4),             # the vector path on a map of one vector: every clamped address collapses onto it
             (16, 16),           # exactly one tile, vector path
             (17, 15),           # scalar path, partial tiles both ways
             (20, 12),           # vector path, partial tiles
             (32, 16), (36, 20),  # a tile seam on the vector path; the second with a partial last tile
             (13, 21),           # scalar path, a seam along w
             (8, 5), (6, 4)]     # bf16 planes (L % 8 == 0) on the scalar path
DW_FORMS = ('fp32', 'bf16_f32planes', 'bf16_bf16planes')
DW_STRIDE_CASE = ((20, 12), 32, 8)    # (H, W), D, extra channels per pixel: a pixel stride of 2 D + 8
DW_ROUNDED_ONCE = [(8, 5), (6, 4)]


def dw_vector_path(H, W):
    return H % 4 == 0 and W % 4 == 0


def dw_forms(H, W):
    return [f for f in DW_FORMS if f != 'bf16_bf16planes' or (H * W) % 8 == 0]


def dw_dtypes(form):
    """(activation dtype, plane dtype)."""
    return {'fp32': (F32, F32), 'bf16_f32planes': (BF16, F32), 'bf16_bf16planes': (BF16, BF16)}[form]


def dw_inputs(D, H, W, form, bias, extra=0):
    """xz [B, H, W, 2 D + extra] in the activation dtype, weight [D, 9] and bias [D] (or None) fp32, the cotangent pair [B, 2, D, L] in
    the plane dtype.  The generators of test_dwconv_silu_cross."""
    adt, pdt = dw_dtypes(form)
    seed = 500 + D + 31 * H + W
    xz = rnd((DW_B, H, W, 2 * D + extra), seed).to(adt)
    return xz, rnd((D, 9), seed + 1, 0.4), (rnd((D,), seed + 2, 0.2) if bias else None), rnd((DW_B, 2, D, H * W), seed + 3).to(pdt)


def dw_assert(tag, got, xz, D, w, bias, gout2):
    """got = (out [B,2,D,L], dx [B,H,W,D], dw [D,9], db [D] or None) against ref64.dwconv_silu_cross under ref64.dwconv_bounds."""
    B, H, W = xz.shape[:3]
    ref = R.dwconv_silu_cross(xz, D, w, bias, gout2)
    # out 12 + __expf; d(conv) 15 + (1 + zmax) (2 + __expf); dx + 9; dw, db + 1 + 21 (halo pixels of a thread) + 4 (16 lanes) + B * tiles (slab_sum)
    ab = R.dwconv_bounds(ref['zmax'], B, H, W, xz.dtype == BF16, gout2.dtype == BF16)        # (the cotangent pair is in the plane dtype)
    worst = {}
    for n, t in zip(('out', 'dx', 'dw', 'db'), got):
        if t is not None:
            worst[n] = R.check(f'{tag} {n}', t.float(), *ref[n], *ab[n])
    return worst
