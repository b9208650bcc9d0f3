"""act(bn(x))[:, ::2, ::2] in one call (csrc/bn.hip tamtr_bncl_act_down2_*, ops.bn_act_down2, backbone.Conv.forward(x, then=Upsample(0.5))).

Forward: the bits of ops.bn_act on the full map followed by [:, ::2, ::2] - the statistics pass is the same launch and the per-element
arithmetic of the apply kernel is the same expression - and the same running statistics and call counter.
Backward: dx, dgamma, dbeta against ref64.batch_norm given the quarter-map cotangent scattered into a zero full map (exactly the composed
function), under ref64.bn_bounds for the channels-last layout at the FULL map's plan.  The new reduce runs in the full map's chunks and
adds every thread's rows in bncl_bwd_reduce's order (a dropped pixel contributes an exact 0), so its chain is the one that bound counts; the
three pixels a work item fills without a cotangent form (gamma rstd) (0 - k1 - xhat k2), bncl_bwd_apply's expression at dz = 0.  For the
same reason the three gradients are also held to the bits of ops.bn_act's backward under the scattered cotangent."""
import pytest
import torch

import bn_cases as K
import ref64 as R

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
EPS, MOM = 1e-3, 0.03

SHAPES = [(2, 4, 6, 8, 'bf16'),         # V = 8, one column group, H != W
          (3, 6, 4, 64, 'fp32'),        # 16 column groups, odd image count
          (2, 2, 2, 4, 'bf16'),         # V = 4, one output pixel per image
          (1, 10, 14, 1024, 'bf16'),    # 128 column groups; the 35 output rows end inside a chunk
          (2, 66, 62, 256, 'bf16')]     # many chunks in all three kernels
KIND_SHAPES = {'fp32': (3, 6, 4, 64, 'fp32'), 'bf16_v4': (2, 2, 2, 4, 'bf16'), 'bf16_v8': (2, 4, 6, 8, 'bf16')}   # one per (T, V) instantiation
SLICED = [(2, 4, 6, 8, 'bf16'), (3, 6, 4, 64, 'fp32')]      # gy as a channel slice, ldgy = 2 C


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import tamtr_amd.ops as ops
    return ops


def dev(t):
    return t.detach().cuda()


def module(C, params):
    bn = torch.nn.BatchNorm2d(C, eps=EPS, momentum=MOM).cuda()
    with torch.no_grad():
        bn.weight.copy_(params[0]); bn.bias.copy_(params[1]); bn.running_mean.copy_(params[2]); bn.running_var.copy_(params[3])
    return bn


def strided(g):
    """g [N, C] as the left half of a [N, 2 C] device map (ldgy = 2 C), which the backward must read in place."""
    wide = torch.full((g.shape[0], 2 * g.shape[1]), float('nan'), device='cuda', dtype=g.dtype)
    wide[:, :g.shape[1]] = g
    return wide[:, :g.shape[1]]


def scatter(gq, B, H, W):
    """The quarter map's rows as the rows of a full map that is zero at every pixel the resample drops."""
    C = gq.shape[1]
    full = torch.zeros(B, H, W, C, dtype=gq.dtype, device=gq.device)
    full[:, ::2, ::2] = gq.view(B, H // 2, W // 2, C)
    return full.view(B * H * W, C)


def full_plan(ops, B, H, W, C, dt):
    N = B * H * W
    code = 1 if dt == BF16 else 0
    plan, quarter = K.cl_plan(N, C, dt == BF16), K.cl_plan(N // 4, C, dt == BF16)
    assert ops._lib.lib().tamtr_bncl_blocks(N, C, code) == plan[4] and ops._lib.lib().tamtr_bncl_blocks(N // 4, C, code) == quarter[4], \
        'the chunking of csrc/bn.hip is no longer what tests/bn_cases.py restates'
    return plan


def _case(ops, B, H, W, C, dtn, act, kind='ordinary', sliced=False):
    dt = K.DT[dtn]
    N = B * H * W
    tag = f'bn_down2[{dtn},{B}x{H}x{W}x{C},act={act},{kind},ldgy={"2C" if sliced else "C"}]'
    plan = full_plan(ops, B, H, W, C, dt)
    x, _ = K.bn_rows(N, C, dt, kind, 800 + 3 * C + N % 1000, K.home_row('cl', plan, N))
    _, gq = K.bn_rows(N // 4, C, dt, 'ordinary', 850 + C)
    p = K.bn_params(C, 11 + C)
    # forward: the full map's BatchNorm, then the resample's index pattern
    bn_full, bn = module(C, p), module(C, p)
    xf = dev(x).requires_grad_()
    full = ops.bn_act(xf, bn_full, bool(act))
    want = full.detach().view(B, H, W, C)[:, ::2, ::2].reshape(N // 4, C)
    xd = dev(x).requires_grad_()
    out = ops.bn_act_down2(xd, bn, bool(act), B, H, W)
    assert out.shape == (N // 4, C) and out.dtype == dt and out.is_contiguous()
    assert torch.equal(out, want), f'{tag}: out differs from bn_act(x)[:, ::2, ::2] in {int((out != want).sum())} elements'
    assert torch.equal(bn.running_mean, bn_full.running_mean) and torch.equal(bn.running_var, bn_full.running_var), f'{tag}: running statistics'
    assert int(bn.num_batches_tracked) == int(bn_full.num_batches_tracked) == 1
    # backward
    gd = strided(dev(gq)) if sliced else dev(gq)
    if sliced:
        assert ops._gy_rows(gd, xd).data_ptr() == gd.data_ptr() and gd.stride(0) == 2 * C
    mr = out.grad_fn.saved_tensors[3]
    out.backward(gd)
    got = {'dx': xd.grad, 'dgamma': bn.weight.grad, 'dbeta': bn.bias.grad, 'mean': mr[:, 0], 'rstd': mr[:, 1],
           'running_mean': bn.running_mean, 'running_var': bn.running_var}
    assert xd.grad.shape == (N, C) and bool(torch.isfinite(xd.grad).all())
    K.bn_single_assert(tag, got, 'cl', plan, x, p[0], p[1], scatter(gq, B, H, W), EPS, MOM, p[2], p[3], act)
    full.backward(scatter(dev(gq), B, H, W))
    for name, a, b in (('dx', xd.grad, xf.grad), ('dgamma', bn.weight.grad, bn_full.weight.grad), ('dbeta', bn.bias.grad, bn_full.bias.grad)):
        assert torch.equal(a, b), f'{tag}: {name} differs from the backward of bn_act under the scattered cotangent in {int((a != b).sum())} elements'


@pytest.mark.parametrize('act', (0, 1))
@pytest.mark.parametrize('B,H,W,C,dt', SHAPES)
def test_bn_down2_vs_full_map_and_fp64(ops, B, H, W, C, dt, act):
    _case(ops, B, H, W, C, dt, act)


@pytest.mark.parametrize('B,H,W,C,dt', SLICED)
def test_bn_down2_reads_a_channel_slice_in_place(ops, B, H, W, C, dt):
    _case(ops, B, H, W, C, dt, 1, sliced=True)


@pytest.mark.parametrize('kind', ('ordinary', 'offset', 'outlier'))
@pytest.mark.parametrize('inst', list(KIND_SHAPES))
def test_bn_down2_input_kinds(ops, inst, kind):
    for act in (0, 1):
        _case(ops, *KIND_SHAPES[inst], act, kind)


def test_bn_down2_ok_is_what_the_entry_points_take(ops):
    import torch.nn as nn
    bn = nn.BatchNorm2d(64).cuda().train()
    cl = lambda *s, dt=BF16: torch.zeros(*s, device='cuda', dtype=dt).contiguous(memory_format=torch.channels_last)
    assert ops.bn_down2_ok(cl(2, 64, 4, 6), bn) and ops.bn_down2_ok(cl(2, 64, 4, 6, dt=F32), bn)
    assert not ops.bn_down2_ok(cl(2, 64, 5, 6), bn) and not ops.bn_down2_ok(cl(2, 64, 4, 7), bn)              # odd sizes
    assert not ops.bn_down2_ok(torch.zeros(2, 64, 4, 6, device='cuda', dtype=BF16), bn)                        # NCHW
    assert not ops.bn_down2_ok(cl(2, 64, 4, 6).cpu(), bn) and not ops.bn_down2_ok(cl(2, 64, 4, 6, dt=torch.float16), bn)
    assert not ops.bn_down2_ok(cl(2, 24, 4, 6), nn.BatchNorm2d(24).cuda())                                     # a channel count the kernels refuse
    assert not ops.bn_down2_ok(cl(2, 64, 4, 6), nn.BatchNorm2d(64).cuda().eval())
    assert not ops.bn_down2_ok(cl(2, 64, 4, 6), nn.BatchNorm2d(64, affine=False).cuda())


@pytest.mark.parametrize('dtn', ('bf16', 'fp32'))
def test_conv_then_upsample_switch_on_and_off(ops, monkeypatch, dtn):
    """A Conv(1x1) + Upsample(0.5) pair through Conv.forward(x, then=up), what the layer loop calls, with TAMTR_BN_DOWN2 on and off.  The
    outputs are equal bit for bit.  The gradient that enters the convolution's backward (d of the convolution output) and the BatchNorm's
    parameter gradients are held to bn_bounds on both paths.  The convolution's own input and weight gradients come from the same
    backward kernels fed with those two gradients g_on, g_off; they may differ by |g_on - g_off| carried through the linear map, plus,
    once per path, the rounding of that map: Cout (input gradient) | N (weight gradient) fp32 additions in any order and the store."""
    from tamtr_amd.backbone import Conv, Upsample
    dt = K.DT[dtn]
    B, H, W, Cin, C = 2, 12, 10, 32, 64
    N = B * H * W
    plan = full_plan(ops, B, H, W, C, dt)
    conv, up = Conv(Cin, C, 1, 1).cuda().train(), Upsample(None, 0.5, 'nearest')
    p = K.bn_params(C, 11 + C)
    with torch.no_grad():
        conv.conv.weight.copy_(0.2 * K.rnd((C, Cin, 1, 1), 900))
        for t, v in zip((conv.bn.weight, conv.bn.bias), p):
            t.copy_(v)
    conv.conv.to(dt)
    state = {k: v.clone() for k, v in conv.state_dict().items()}
    x0 = K.rnd((B, Cin, H, W), 901).to(dt).cuda().contiguous(memory_format=torch.channels_last)
    gq = K.rnd((B, C, H // 2, W // 2), 902).to(dt).cuda().contiguous(memory_format=torch.channels_last)
    real = {'down2': ops.bn_act_down2, 'full': ops.bn_act}
    runs = {}
    for on in (True, False):
        cap, calls = {}, []

        def spy(name):
            def f(x_rows, *a, **k):
                calls.append(name)
                cap['y'] = x_rows.detach().clone()
                x_rows.register_hook(lambda g: cap.__setitem__('gy', g.detach().clone()))
                return real[name](x_rows, *a, **k)
            return f
        monkeypatch.setattr(ops, '_BN_DOWN2', on)
        monkeypatch.setattr(ops, 'bn_act_down2', spy('down2'))
        monkeypatch.setattr(ops, 'bn_act', spy('full'))
        conv.load_state_dict(state)
        conv.zero_grad(set_to_none=True)
        x = x0.clone().requires_grad_()
        out = conv(x, then=up)
        assert calls == ['down2' if on else 'full'] and out.shape == (B, C, H // 2, W // 2)
        out.backward(gq)
        runs[on] = {'out': out.detach(), 'y': cap['y'], 'gy': cap['gy'], 'dx': K.rows(x.grad), 'dw': conv.conv.weight.grad.view(C, Cin),
                    'dgamma': conv.bn.weight.grad.clone(), 'dbeta': conv.bn.bias.grad.clone(),
                    'running_mean': conv.bn.running_mean.clone(), 'running_var': conv.bn.running_var.clone()}
    a, b = runs[True], runs[False]
    assert torch.equal(a['out'], b['out']) and torch.equal(a['y'], b['y'])
    assert torch.equal(a['running_mean'], b['running_mean']) and torch.equal(a['running_var'], b['running_var'])
    gfull = scatter(K.rows(gq).contiguous(), B, H, W).cpu()
    for on, r in runs.items():
        K.bn_single_assert(f'conv+up[{dtn},TAMTR_BN_DOWN2={int(on)}]', {'dx': r['gy'], 'dgamma': r['dgamma'], 'dbeta': r['dbeta']}, 'cl', plan,
                           r['y'].cpu(), p[0], p[1], gfull, EPS, MOM, None, None, 1)
    d = R._d
    E, G = (d(a['gy']) - d(b['gy'])).abs(), torch.maximum(d(a['gy']).abs(), d(b['gy']).abs())
    Wm, X = d(conv.conv.weight).view(C, Cin).abs(), d(K.rows(x0)).abs()
    st = 2.0 ** -8 if dt == BF16 else 0.0
    for name, carried, mag, n in (('dx', E @ Wm, G @ Wm, C), ('dw', E.t() @ X, G.t() @ X, N)):
        diff = (d(a[name]) - d(b[name])).abs()
        bound = carried + 2 * (st * torch.maximum(d(a[name]).abs(), d(b[name]).abs()) + R.fp32_b(n + 2) * mag)
        worst = float((diff / bound.clamp_min(1e-300)).max())
        print(f'conv+up[{dtn}] {name}: worst |on - off| / bound {worst:.3f}; bit-equal {torch.equal(a[name], b[name])}')
        assert bool((diff <= bound).all()), f'conv+up[{dtn}] {name}: |on - off| is {worst:.2f} times its bound'
