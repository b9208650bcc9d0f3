"""csrc/dwgrad.hip (tamtr_dw_bf16: the row-slice weight and bias gradient of the short and mid-size token-wise products) elementwise against
fp64 with the bounds of tests/dw_cases.py (tests/test_dw_host.py holds the same bounds against a CPU emulation and a lost-row mutant);
its routing in ops.dw_splitk / ops._param_grads against the batched library path (TAMTR_DW_OWN=0); the two autograd nodes that use it; and
a HIP-graph capture of ops._param_grads on it: two kernel nodes, no memset node, replays equal to eager execution."""
import gc

import pytest
import torch

import dw_cases as D
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


_REF = {}


def case(M, N, K):
    """(dY, X on the GPU, fp64 reference), computed once per shape and shared."""
    if (M, N, K) not in _REF:
        gy, x = D.inputs(M, N, K)
        _REF[(M, N, K)] = (gy.cuda(), x.cuda(), D.reference(gy, x))
    return _REF[(M, N, K)]


def _launch(ops, gy, x, S, with_db):
    """The C entry point on a NaN-prefilled partial buffer + the ordered sum -> (dW [N, K], db [N], the partials)."""
    M, N = gy.shape
    K = x.shape[1]
    part = torch.full((S, N * K + N), float('nan'), device='cuda', dtype=F32)
    ops.call('tamtr_dw_bf16', ops.ptr(gy), ops.ptr(x), ops.ptr(part), int(with_db), M, N, K, ops.stream_ptr())
    tot = ops.slab_sum(part)
    return tot[:N * K].view(N, K), tot[N * K:], part


@pytest.mark.parametrize('with_db', [True, False], ids=['db', 'nodb'])
@pytest.mark.parametrize('M,N,K', D.CASES, ids=D.IDS)
def test_dw_kernel_vs_fp64(ops, M, N, K, with_db):
    gy, x, ref = case(M, N, K)
    S = ops._lib.lib().tamtr_dw_slices(M, N, K)
    assert (S == 1) if M == 292 else (S > 1 if M == 4672 else S >= 1), S
    dw, db, part = _launch(ops, gy, x, S, with_db)
    dw2, db2, part2 = _launch(ops, gy, x, S, with_db)
    assert torch.equal(part.view(torch.int32), part2.view(torch.int32)), 'a second launch gives other bits'   # (also: every element written)
    assert torch.equal(dw, dw2) and torch.equal(db, db2)
    bd = D.bounds(M, N, K, S)
    what = f'dw_bf16[{M}x{N}x{K},S={S}]'
    w = R.check(what + ' dw', dw, ref['dw'][0], ref['dw'][1], *bd['dw'])
    print(f'{what}: worst err / bound dw {w:.3f}')
    if with_db:
        w = R.check(what + ' db', db, ref['db'][0], ref['db'][1], *bd['db'])
        print(f'{what}: worst err / bound db {w:.3f}')
    else:
        assert not bool(db.any()), 'without with_db the column-sum tail is zeros'


@pytest.mark.parametrize('M,N,K', D.CASES, ids=D.IDS)
def test_param_grads_new_path_vs_library_path(ops, M, N, K, monkeypatch):
    """ops._param_grads (as _LinearMaster calls it) through csrc/dwgrad.hip and, with the switch off, through the batched library product +
    colsum: each is inside its own bound around the fp64 value, so they differ by at most the sum of both."""
    gy, x, ref = case(M, N, K)
    assert ops._dw_own_slices(gy, x) > 0
    gw, gb = ops._param_grads(gy, x, F32, F32, True, True, ops._LM_MIN_ROWS)
    assert torch.equal(gw, ops.dw_splitk(gy, x, ops._LM_MIN_ROWS))
    monkeypatch.setattr(ops, '_DW_OWN', False)
    assert ops._dw_own_slices(gy, x) == 0
    gw0, gb0 = ops._param_grads(gy, x, F32, F32, True, True, ops._LM_MIN_ROWS)
    assert gw.dtype == gw0.dtype == F32 and gb.dtype == gb0.dtype == F32 and gw.shape == gw0.shape == (N, K) and gb.shape == gb0.shape == (N,)
    new = D.bounds(M, N, K, ops._lib.lib().tamtr_dw_slices(M, N, K))
    old = R.linear_grad_bounds(M, N, K, G.split_count(M, ops._LM_MIN_ROWS), ops._BMM_F32_OUT is not False, G.colsum_streams(M, N))
    for name, a, b in (('dw', gw, gw0), ('db', gb, gb0)):
        val, mag = ref[name]
        tol = old[name][0] * R.U8 * val.abs() + (old[name][1] + new[name][1]) * mag
        err = (a.double().cpu() - b.double().cpu()).abs()
        worst = float((err / tol).max())
        print(f'{M}x{N}x{K} {name}: |new - library| / (sum of bounds) = {worst:.3f}')
        assert worst <= 1, (name, worst)


def test_autograd_nodes_on_the_new_path(ops):
    """A _Conv1x1CL (fp32 master of a bf16 copy) and a _LinearMaster backward at these sizes: finite gradients, the masters' dtype and shape,
    and the values of the library path within the bounds' sum (fp64 reference of the same operands)."""
    torch.manual_seed(3)
    B, C1, C2, H, W = 2, 96, 64, 25, 20   # M = 1 000
    x = torch.randn(B, C1, H, W, device='cuda').to(BF16).contiguous(memory_format=torch.channels_last)
    master = torch.nn.Parameter(torch.randn(C2, C1, 1, 1, device='cuda') * 0.1)
    w16 = master.detach().to(BF16)
    y = ops._Conv1x1CL.apply(x, w16, master)
    cot = torch.randn_like(y)
    gm, = torch.autograd.grad(y, [master], cot)
    assert gm.dtype == F32 and gm.shape == master.shape and bool(torch.isfinite(gm).all())
    g2, x2 = cot.permute(0, 2, 3, 1).reshape(-1, C2), x.permute(0, 2, 3, 1).reshape(-1, C1)
    assert ops._dw_own_slices(g2.contiguous(), x2.contiguous()) > 0
    ref = D.reference(g2.cpu(), x2.cpu())
    R.check('conv1x1 master gradient', gm.view(C2, C1), *ref['dw'], *D.bounds(B * H * W, C2, C1, ops._lib.lib().tamtr_dw_slices(B * H * W, C2, C1))['dw'])

    lin = torch.nn.Linear(256, 128).cuda()
    xl = torch.randn(16, 292, 256, device='cuda')   # M = 4 672
    with torch.autocast('cuda', dtype=BF16):
        assert ops.linear_master_ok(xl, lin)
        yl = ops.linear(xl, lin)
    cl = torch.randn_like(yl)
    gw, gb = torch.autograd.grad(yl, [lin.weight, lin.bias], cl)
    assert gw.dtype == F32 and gb.dtype == F32 and gw.shape == lin.weight.shape and gb.shape == lin.bias.shape
    assert bool(torch.isfinite(gw).all()) and bool(torch.isfinite(gb).all())
    ref = D.reference(cl.reshape(-1, 128).cpu(), xl.to(BF16).reshape(-1, 256).cpu())
    D.check('linear master gradients', gw, gb, ref, D.bounds(4672, 128, 256, ops._lib.lib().tamtr_dw_slices(4672, 128, 256)))


def test_param_grads_capture_replays_equal_eager(ops):
    """ops._param_grads on the new path recorded into a HIP graph on a side stream: two kernel nodes (the product, the ordered sum), no
    memset node; two replays on changed inputs give the bits of eager execution."""
    import tamtr_amd.graphs as graphs
    M, N, K = 4672, 256, 128
    gy, x, _ = case(M, N, K)
    sg, sx = gy.clone(), x.clone()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        for _ in range(2):
            ops._param_grads(sg, sx, F32, F32, True, True, ops._LM_MIN_ROWS)
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    gc.collect()
    gc_was_on = gc.isenabled()
    gc.disable()
    try:
        with torch.cuda.graph(graph, stream=stream):
            gw, gb = ops._param_grads(sg, sx, F32, F32, True, True, ops._LM_MIN_ROWS)
            census = graphs.capture_census(stream)
    finally:
        if gc_was_on:
            gc.enable()
    assert census['memset'] == 0 and census['kernel'] == 2 and census['memcpy'] == 0, census
    for seed in (1, 2):
        ngy, nx = (t.cuda() for t in D.inputs(M, N, K, seed))
        sg.copy_(ngy)
        sx.copy_(nx)
        graph.replay()
        torch.cuda.synchronize()
        ew, eb = ops._param_grads(ngy, nx, F32, F32, True, True, ops._LM_MIN_ROWS)
        assert torch.equal(gw, ew) and torch.equal(gb, eb), seed
        assert not torch.equal(gw, ops._param_grads(gy, x, F32, F32, True, True, ops._LM_MIN_ROWS)[0])   # (the replay did read the new inputs)
