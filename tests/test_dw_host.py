"""csrc/dwgrad.hip on the CPU: the slice plan of tamtr_dw_slices (a host function), and the bounds of tests/dw_cases.py held against a CPU
emulation of the kernel's summation and against a mutant that loses one row - so that tests/test_gpu_dw_ref64.py, which asserts the same
bounds on the GPU, is known to pass a correct sum and to see a lost row."""
import pytest

import dw_cases as D


@pytest.fixture(scope='module')
def slices_of():
    from tamtr_amd import _lib
    return _lib.lib().tamtr_dw_slices


def test_slice_plan_invariants(slices_of):
    """1 <= S <= 64; the slices (rows per slice a multiple of 64, the last one the rest) cover M exactly with none empty; S = 1 below two
    slices' worth of rows; 0 for N or K not a multiple of 16; the fill the plan aims at: a 512 x 512 output about 32 slices, a 1024 x 2048
    output 4."""
    for M in (1, 63, 64, 65, 292, 511, 512, 1000, 4672, 6400, 25600, 102400, 537600, (1 << 31) + 5):
        for N, K in ((16, 16), (16, 512), (64, 64), (96, 512), (512, 192), (256, 128), (512, 512), (1024, 2048), (2048, 512)):
            S = slices_of(M, N, K)
            assert 1 <= S <= 64, (M, N, K, S)
            rows = D.rows_per_slice(M, S)
            assert rows % 64 == 0 and (S - 1) * rows < M <= S * rows, (M, N, K, S, rows)
            sl = D.slices(M, S)
            assert sl[0][0] == 0 and sl[-1][1] == M and all(a[1] == b[0] for a, b in zip(sl, sl[1:])) and all(hi > lo for lo, hi in sl)
            if M < 512:
                assert S == 1, (M, N, K, S)
    assert 24 <= slices_of(537600, 512, 512) <= 40 and slices_of(537600, 1024, 2048) == 4
    for N, K in ((8, 16), (16, 8), (17, 16), (16, 24), (0, 16), (100, 64)):
        assert slices_of(4672, N, K) == 0, (N, K)
    assert slices_of(0, 16, 16) == 0 and slices_of(-5, 16, 16) == 0


@pytest.mark.parametrize('M,N,K', D.CASES, ids=D.IDS)
def test_emulated_summation_is_inside_the_bounds(slices_of, M, N, K):
    S = slices_of(M, N, K)
    assert S == 1 if M == 292 else S >= 1
    gy, x = D.inputs(M, N, K)
    dw, db = D.emulate(gy, x, S)
    worst = D.check(f'emulated[{M}x{N}x{K},S={S}]', dw, db, D.reference(gy, x), D.bounds(M, N, K, S))
    print(f'{M}x{N}x{K} S={S}: worst err / bound dw {worst[0]:.3f} db {worst[1]:.3f}')


@pytest.mark.parametrize('N,K', D.NKS, ids=[f'{n}x{k}' for n, k in D.NKS])
def test_a_lost_row_misses_the_bounds(slices_of, N, K):
    """M = 292, one slice: the sum without row 37 must miss both bounds."""
    M = 292
    assert slices_of(M, N, K) == 1
    gy, x = D.inputs(M, N, K)
    dw, db = D.emulate(gy, x, 1, drop=(0, 37))
    ref, bd = D.reference(gy, x), D.bounds(M, N, K, 1)
    import ref64 as R
    with pytest.raises(AssertionError):
        R.check('mutant dw', dw, ref['dw'][0], ref['dw'][1], *bd['dw'], log=False)
    with pytest.raises(AssertionError):
        R.check('mutant db', db, ref['db'][0], ref['db'][1], *bd['db'], log=False)
