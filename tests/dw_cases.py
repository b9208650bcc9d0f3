"""Cases, seeded inputs, the fp64 reference, the bounds and a CPU emulation of the summation of csrc/dwgrad.hip (tamtr_dw_bf16: the
row-slice weight gradient dW = dY^T X and bias gradient db of the short and mid-size token-wise products), shared by
tests/test_dw_host.py (CPU) and tests/test_gpu_dw_ref64.py (GPU).

Bounds (tests/ref64.py check(): |got - ref| <= b mag, a = 0 - the results are fp32): with R = the rows of a slice and S slices
    dW: b = fp32_b(R + slab_sum_chain(S, N K + Npad))   R products, each exact in fp32 (8 + 8 significant bits), enter an fp32 accumulator
                                                        (worst case one rounding each, as ref64.linear_bounds counts an MFMA chain); then
                                                        the ordered sum over the slices
    db: the same b                                      a thread adds its R / 8 rows, 8 threads' shares are added in order: at most R
with chain 0 for S = 1 (the sum over one slice is a copy)."""
import torch

import ref64 as R

MS = (292, 1000, 4672)            # a single short block of rows; a ragged last block; S > 1 at the decoder's own row count
NKS = ((16, 16), (96, 512), (512, 192), (256, 128))   # narrow tiles; partial tiles; N != K on both sides
CASES = [(M, N, K) for M in MS for N, K in NKS]
IDS = [f'{M}x{N}x{K}' for M, N, K in CASES]
STAGE = 64                        # rows per stage of the kernel (DW_ROWS)


def rows_per_slice(M, S):
    """Rows of every slice but the last (include/tamtr_hip.h): ceil(ceil(M / S) / 64) * 64."""
    return -(-(-(-M // S)) // STAGE) * STAGE


def slices(M, S):
    """[(first row, end row)] of the S slices."""
    rows = rows_per_slice(M, S)
    return [(s * rows, min(M, (s + 1) * rows)) for s in range(S)]


def inputs(M, N, K, seed=0):
    """dY bf16 [M, N], X bf16 [M, K] (CPU), seeded per shape."""
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * M + 31 * N + K)
    return torch.randn(M, N, generator=g).bfloat16(), torch.randn(M, K, generator=g).bfloat16()


def reference(gy, x):
    """{'dw': (value, magnitude), 'db': (value, magnitude)} in fp64 from the operands as the kernel reads them."""
    G, X = gy.double(), x.double()
    aG = G.abs()
    return {'dw': (G.t() @ X, aG.t() @ X.abs()), 'db': (G.sum(0), aG.sum(0))}


def bounds(M, N, K, S):
    """{name: (a, b)}: see the module docstring.  R = the longest slice's real row count."""
    rows = max(hi - lo for lo, hi in slices(M, S))
    chain = 0 if S == 1 else R.slab_sum_chain(S, N * K + (N + 3) // 4 * 4)
    b = R.fp32_b(rows + chain)
    return {'dw': (0, b), 'db': (0, b)}


def emulate(gy, x, S, drop=None):
    """(dW, db) in fp32 the way the kernel and the ordered sum add them: per slice the rows' products (exact in fp32) added into an fp32
    accumulator row by row; the column sums per 8-row group of each 64-row stage, the 8 groups then added in order; the slices added in
    order.  drop = (slice, row of the slice): that row is left out (the mutant a bound must catch)."""
    G, X = gy.float(), x.float()
    N, K = G.shape[1], X.shape[1]
    dw = db = None
    for s, (lo, hi) in enumerate(slices(G.shape[0], S)):
        acc = torch.zeros(N, K)
        col = torch.zeros(8, N)
        for m in range(lo, hi):
            if drop == (s, m - lo):
                continue
            acc += torch.outer(G[m], X[m])
            col[((m - lo) % STAGE) // 8] += G[m]
        cs = torch.zeros(N)
        for g in range(8):
            cs += col[g]
        dw, db = (acc, cs) if dw is None else (dw + acc, db + cs)
    return dw, db


def check(what, dw, db, ref, bd):
    """Both assertions; returns the worst err / bound ratios."""
    return (R.check(what + ' dw', dw, ref['dw'][0], ref['dw'][1], *bd['dw']),
            R.check(what + ' db', db, ref['db'][0], ref['db'][1], *bd['db']))
