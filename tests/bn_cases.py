"""The host dispatch of csrc/bn.hip restated, the cases, the seeded inputs and the assertions of the BatchNorm checks against fp64.
tests/test_gpu_bn_ref64.py feeds the assertions the kernels' outputs, tests/test_ref64_host.py feeds them fp32 CPU emulations of the kernels
(which must pass) and mutants of those (which must fail).

Every assertion is ref64.check(): |got - ref| <= a 2^-8 |ref| + b mag, a and b counted in ref64.bn_bounds from the plan of the case.
Maps travel as rows [N, C]; an NCHW map [B, C, HW] is rows [B * HW, C], image-major (nchw() / rows())."""
import torch

import ref64 as R
from weights import rnd

F32, BF16 = torch.float32, torch.bfloat16
DT = {'fp32': F32, 'bf16': BF16}
EPS_MOM = ((1e-3, 0.03), (1e-5, 0.1))      # the trunk's BatchNorms (the reference rewrites them after construction) | torch's defaults (MEH, RepConvN)


def dtn(dt):
    return 'bf16' if dt == BF16 else 'fp32'


# ================================================================================================ the dispatch, restated
# bn_vec:            NCHW kernels take 4-element vector accesses when HW % 4 == 0 and every map pointer is aligned to 4 elements, else the scalar path
# tamtr_bn_slices:   B * ceil(HW / 4096) workgroups per channel, one (count, mean, M2) triple each
# bncl_vec:          V = 8 for bf16 with C % 8 == 0, else 4 (fp32, and bf16 with C = 4, 12, ...)
# bncl_iters:        pieces (256 x V elements) per chunk: total / piece / 1024 rounded up to a multiple of 4, within [4, 64]
# tamtr_bncl_blocks: ceil(total / (iters * 256 * V)) chunks = workgroups = partials per channel
def nchw_plan(B, C, HW, bf16, aligned=True):
    """(vec, slices_per_plane, S)."""
    sh = -(-HW // R.BN_SLICE)
    return HW % 4 == 0 and aligned, sh, B * sh


def cl_plan(N, C, bf16):
    """(V, cg, iters, chunk_rows, S)."""
    V = 8 if bf16 and C % 8 == 0 else 4
    piece, total = 256 * V, N * C
    it = (total // piece // 1024 + 3) // 4 * 4
    iters = min(max(it, 4), 64)
    chunk = iters * piece
    return V, C // V, iters, chunk // C, -(-total // chunk)


def home_row(layout, plan, N, B=None, HW=None):
    """The first row of the last chunk (channels-last: where padded loads are redirected and what the chunk's sums are shifted by); for
    NCHW the first pixel of the last image's last slice."""
    if layout == 'nchw':
        return (B - 1) * HW + (plan[1] - 1) * R.BN_SLICE
    return (plan[4] - 1) * plan[3]


# ================================================================================================ the cases
NCHW_SHAPES = [(2, 3, 63),      # scalar path, a thread with a partial cnt (63 = 3 * 16 + 15)
               (2, 3, 64),      # vector path
               (1, 2, 4096),    # exactly one full slice
               (1, 2, 4100),    # a second slice of four elements: nearly every thread has cnt = 0
               (2, 2, 8200),    # three slices per plane
               (260, 2, 3),     # S = 260: thread 0 .. 3 combine two triples before the butterfly
               (1, 1, 1)]       # one value per channel: the biased variance in the running update
NCHW_KIND_SHAPES = [(2, 3, 64), (1, 2, 4100)]
NCHW_KIND_CASES = [(B, C, HW, k) for B, C, HW in NCHW_KIND_SHAPES for k in
                   ('offset', 'scales', 'outlier', 'constant', 'nan_row', 'inf_row', 'nan_home', 'inf_home') if k != 'constant' or (B * HW) & (B * HW - 1) == 0]
NCHW_OFFSET = (2, 3, 64, 4)     # B, C, HW, bytes: bf16, HW % 4 == 0, every map 4 bytes into its buffer -> bn_vec sends it to the scalar path

CL_C = {'fp32': (4, 64, 1024), 'bf16': (4, 8, 256, 1024)}     # fp32: cg = 1, 16, 256; bf16: V = 4 (cg = 1), V = 8 with cg = 1, 32, 128
CL_KIND_C = {'fp32': 64, 'bf16_v4': 4, 'bf16_v8': 256}        # one channels-last shape per (T, V) instantiation for every input kind
CL_LARGE = {'S>256': ('fp32', 4, 256 * 1024 + 3),            # 257 chunks of 1024 rows: bn_finalize, bncl_sum and the backward loop twice for thread 0
            'iters=8': ('fp32', 64, 5 * 1024 * 16 + 5)}       # 5 * 2^20 elements and five rows: the smallest map with iters = 8
CL_VARIANTS = [(0, False, False), (1, False, False), (1, True, False), (0, False, True), (1, True, True)]      # (act, residual, strided gy)
KINDS = ('ordinary', 'offset', 'scales', 'outlier', 'constant', 'nan_row', 'inf_row', 'nan_home', 'inf_home')
PAIR_CASES = [('fp32', 64, 'inside', False), ('bf16', 256, 'inside', True), ('bf16', 4, 'chunk+1', False), ('fp32', 4, 'one', True)]   # dt, C, rows, strided gy
SEG_B, SEG_LS = 3, (50, 21, 7)      # three levels: image boundaries at rows 50, 100 / 21, 42 / 7, 14: inside a chunk and inside a piece at every C below
SEG_CASES = [('fp32', 64), ('bf16', 256), ('bf16', 8)]
FINALIZE_S = (1, 5, 300)


def cl_rows(C, bf16):
    """{name: N}: the row counts that reach each branch of the chunking at this width (iters = 4 at these sizes)."""
    V, cg, iters, chunk_rows, _ = cl_plan(1, C, bf16)
    piece_rows = 256 * V // C
    rows = {'one': 1, 'chunk': chunk_rows, 'chunk+1': chunk_rows + 1,
            'inside': 2 * chunk_rows + piece_rows + max(1, piece_rows // 2)}      # the third chunk ends inside its second piece
    if piece_rows > 2:
        rows['<piece'] = piece_rows - 1
    return rows


def reached():
    """Every branch the cases are listed for, as a set of strings; tests/test_ref64_host.py asserts the whole list."""
    got = set()
    for B, C, HW in NCHW_SHAPES:
        for bf16 in (False, True):
            vec, sh, S = nchw_plan(B, C, HW, bf16)
            got |= {'nchw vec' if vec else 'nchw scalar', f'nchw slices {min(sh, 3)}'}
            if HW % 16:
                got.add('nchw partial cnt')
            if sh > 1 and HW % R.BN_SLICE <= R.BN_SLICE - 16:
                got.add('nchw cnt = 0')
            if S > 256:
                got.add('nchw S > 256')
            if B * HW == 1:
                got.add('nchw one value')
    B, C, HW, nb = NCHW_OFFSET
    if HW % 4 == 0 and not nchw_plan(B, C, HW, True, aligned=False)[0]:
        got.add('nchw unaligned scalar')
    cases = [(dt, C, N) for dt in CL_C for C in CL_C[dt] for N in cl_rows(C, dt == 'bf16').values()] + list(CL_LARGE.values())
    for dt, C, N in cases:
        V, cg, iters, chunk_rows, S = cl_plan(N, C, dt == 'bf16')
        piece_rows = 256 * V // C
        got |= {f'cl {dt} V={V}', f'cl cg={cg}', f'cl iters={iters}'}
        if N == 1:
            got.add('cl one row')
        if N * C < 256 * V:
            got.add('cl < piece')
        if N == chunk_rows:
            got.add('cl one chunk')
        if N == chunk_rows + 1:
            got.add('cl chunk + 1 row')
        if S > 1 and (N % chunk_rows) % piece_rows:
            got.add('cl ends inside a piece')
        if S > 256:
            got.add('cl S > 256')
    return got


REACH = {'nchw vec', 'nchw scalar', 'nchw slices 1', 'nchw slices 2', 'nchw slices 3', 'nchw partial cnt', 'nchw cnt = 0', 'nchw S > 256',
         'nchw one value', 'nchw unaligned scalar', 'cl fp32 V=4', 'cl bf16 V=4', 'cl bf16 V=8', 'cl cg=1', 'cl cg=16', 'cl cg=32', 'cl cg=128', 'cl cg=256', 'cl iters=4', 'cl iters=8',
         'cl one row', 'cl < piece', 'cl one chunk', 'cl chunk + 1 row', 'cl ends inside a piece', 'cl S > 256'}


# ================================================================================================ the inputs
def bn_params(C, seed):
    """gamma, beta, running_mean, running_var (fp32), as the old tests set them."""
    return 1 + 0.3 * rnd((C,), seed), 0.2 * rnd((C,), seed + 1), 0.1 * rnd((C,), seed + 2), 1 + 0.1 * rnd((C,), seed + 3).abs()


def bn_rows(N, C, dt, kind, seed, home=0):
    """x, gout as rows [N, C] in dt, on the CPU.
    ordinary  1.7 randn + 0.4, the old tests' rows         offset   8 + 0.25 randn: the mean is 32 standard deviations
    scales    channel 0 times 1e-3 (eps dominates), channel 1 times 1e3 (eps is negligible)
    outlier   row `home` of channel 0 lies 64 standard deviations out     constant  the last channel is 0.375, its cotangent 0.25
    nan_row | inf_row | nan_home | inf_home   one NaN | Inf in channel 1 (0 where C = 1), in row 1 | in row `home`"""
    r = rnd((N, C), seed)
    x = 8 + 0.25 * r if kind == 'offset' else 1.7 * r + 0.4
    g = rnd((N, C), seed + 1)
    if kind == 'scales':
        x[:, 0] *= 1e-3
        x[:, min(1, C - 1)] *= 1e3
    elif kind == 'outlier':
        x[home, 0] = 0.4 + 64 * 1.7
    elif kind == 'constant':
        x[:, C - 1], g[:, C - 1] = 0.375, 0.25
    elif kind != 'ordinary' and kind != 'offset':
        x[home if kind.endswith('home') else min(1, N - 1), min(1, C - 1)] = float(kind[:3])
    return x.to(dt), g.to(dt)


def nchw(t, B, HW):
    """rows [B * HW, C] -> [B, C, HW]."""
    return t.view(B, HW, -1).permute(0, 2, 1).contiguous()


def rows(t):
    """[B, C, ...] -> rows [B * HW, C]."""
    t = t.reshape(t.shape[0], t.shape[1], -1)
    return t.permute(0, 2, 1).reshape(-1, t.shape[1])


def finalize_partials(S, C, empty, seed=7):
    """Hand-made (count, mean, M2) partials [C, S, 3] (fp32) of unequal counts 1 + (5 s) % 7 and the data [n, C] behind them; the partials
    listed in `empty` hold no rows: (0, 0, 0)."""
    counts = [0 if s in empty else 1 + (5 * s) % 7 for s in range(S)]
    data = (1.7 * rnd((sum(counts), C), seed + S) + 0.4).double()
    part = torch.zeros(C, S, 3, dtype=torch.float64)
    at = 0
    for s, n in enumerate(counts):
        if n:
            d = data[at:at + n]
            part[:, s, 0], part[:, s, 1], part[:, s, 2] = n, d.mean(0), ((d - d.mean(0)) ** 2).sum(0)
            at += n
    return part.float(), data, [n for n in counts if n]


# ================================================================================================ the assertions
def bn_assert(tag, got, ref, ab):
    """got = {name: tensor} (maps as rows) against a reference of ref64.batch_norm / batch_norm_pair under ref64.bn_bounds."""
    return {n: R.check(f'{tag} {n}', t.float(), *ref[n], *ab[n]) for n, t in got.items()}


def bn_single_assert(tag, got, layout, plan, x, gamma, beta, gout, eps, mom, rm, rv, act, residual=None):
    """x, gout [, residual] as rows; the plan decides the counts and, for channels-last, the magnitudes of the statistics."""
    ref = R.batch_norm(x, gamma, beta, gout, eps, mom, rm, rv, act, residual, chunk_rows=plan[3] if layout == 'cl' else None)
    ab = R.bn_bounds(layout, plan, x.dtype == BF16, act, ref['zmax'], residual is not None)
    return bn_assert(tag, got, ref, ab)


def bn_pair_assert(tag, got, plan, x1, x2, p1, p2, gout, eps, mom, act):
    """p_i = (gamma, beta, running_mean, running_var)."""
    ref = R.batch_norm_pair(x1, x2, p1[0], p1[1], p2[0], p2[1], gout, eps, mom, p1[2], p1[3], p2[2], p2[3], act, chunk_rows=plan[3])
    return bn_assert(tag, got, ref, R.bn_bounds('cl2', plan, x1.dtype == BF16, act, ref['zmax']))


def bn_constant_assert(tag, got, C, beta, act, dt, eps=1e-3):
    """The constant channel (the last one) of the `constant` kind, N a power of two: every sum the kernels form of it is exact, so
    xhat == 0 and out is the one value act(beta) (exactly beta for the identity); dgamma == 0; under the channel's constant cotangent
    and the identity dx == 0 exactly (sum dz / N is dz itself).  With SiLU the sum of N rounded dz rounds, and dx is held to its bound
    only.  M2 == 0 exactly, so rstd == eps^-1/2 to fp32 rounding: eps as an fp32 constant, the sum with 0, rsqrtf (4)."""
    c = C - 1
    out = got['out'][:, c].float()
    if act:
        assert bool((out == out[0]).all()), f'{tag}: out of a constant channel is not one value'
        R.check(f'{tag} out == SiLU(beta)', out[:1], *R._bn_act(R._d(beta[c:c + 1]), R._d(beta[c:c + 1]).abs(), 1)[:2], 1 if dt == BF16 else 0,
                R.fp32_b(3) + R.expf_b(1))
    else:
        assert bool((out == beta[c].to(dt).float()).all()), f'{tag}: out of a constant channel is not beta'
        assert float(got['dx'][:, c].float().abs().max()) == 0, f'{tag}: dx of a constant channel under a constant cotangent is not 0'
    assert float(got['dgamma'][c]) == 0, f'{tag}: dgamma of a constant channel (xhat == 0)'
    want = torch.tensor([eps ** -0.5], dtype=torch.float64)
    R.check(f'{tag} rstd == eps^-1/2', got['rstd'][c:c + 1], want, want, 0, R.fp32_b(4))


def stats_assert(tag, got, layout, plan, x, eps, mom, rm, rv):
    """got = {mean, rstd, running_mean, running_var} of the statistics-only entry points against the same reference."""
    C = x.shape[1]
    ref = R.batch_norm(x, torch.ones(C), torch.zeros(C), torch.zeros_like(x), eps, mom, rm, rv, 0, chunk_rows=plan[3] if layout == 'cl' else None)
    return bn_assert(tag, got, ref, R.bn_bounds(layout, plan, x.dtype == BF16, 0))


def finalize_assert(tag, got, S, counts, data, eps, mom, rm, rv):
    """tamtr_bn_finalize on hand-made partials: the partials are the fp64 statistics of their rows rounded once to fp32 (1 on the mean,
    1 on M2), then only the combine's roundings: the counts of ref64.bn_stat_counts with those in place of the producers' chains."""
    C = data.shape[1]
    ref = R.batch_norm(data, torch.ones(C), torch.zeros(C), torch.zeros_like(data), eps, mom, rm, rv, 0, parts=counts)
    T = R.bn_combine_steps(S)
    n_mean = 1 + 4 * T
    n_var = max(1 + 7 * T + 1, 2 * n_mean * min(S - 1, T))
    ab = {'mean': (0, R.fp32_b(n_mean)), 'rstd': (0, R.fp32_b(n_var + 4)), 'running_mean': (0, R.fp32_b(n_mean + 4)), 'running_var': (0, R.fp32_b(n_var + 5))}
    return bn_assert(tag, got, ref, ab)
