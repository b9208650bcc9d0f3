"""CPU: the BatchNorm + x0.5 resample pair (csrc/bn.hip tamtr_bncl_act_down2_*, model.down2_pairs, backbone.Conv.forward(x, then=...)):
the symbols and their refusals, which rows of a spec are paired, and the layer loop on the CPU, where the pair stays two plain torch calls."""
import ctypes
import os
import re

import torch
import torch.nn as nn

from conftest import ROOT

NEW = ('tamtr_bncl_act_down2_fwd', 'tamtr_bncl_act_down2_bwd')


def test_new_symbols_are_exported_declared_and_the_abi_version_stays():
    import tamtr_amd
    from tamtr_amd import _lib
    h = ctypes.CDLL(tamtr_amd.LIB_PATH)
    header = open(os.path.join(ROOT, 'include', 'tamtr_hip.h')).read()
    for n in NEW:
        assert hasattr(h, n), f'{n} is not exported'
        assert re.search(r'^int\s+%s\s*\(' % n, header, flags=re.M), f'{n} is not declared in tamtr_hip.h'
        assert n in _lib.EXPORTS
    assert h.tamtr_abi_version() == 36 == _lib.ABI_VERSION


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """-1 invalid (a NULL operand, a size below 1, an unknown dtype or activation), -2 unsupported (odd H or W, a channel count bncl_check
    refuses, a misaligned map, a bad ldgy).  The non-null addresses are never dereferenced: every row returns before a launch, on a
    machine without a GPU."""
    from tamtr_amd import _lib
    h = _lib.lib()
    z, one, odd = ctypes.c_void_p(0), ctypes.c_void_p(16), ctypes.c_void_p(8)   # null | 16-byte aligned | 8-byte aligned only
    eps, mom = 1e-3, 0.03

    def fwd(x=one, gamma=one, beta=one, y=one, mr=one, partials=one, B=2, H=4, W=6, C=64, act=1, dtype=1):
        return h.tamtr_bncl_act_down2_fwd(x, gamma, beta, z, z, y, mr, partials, B, H, W, C, eps, mom, act, dtype, z)

    def bwd(gy=one, ldgy=64, x=one, gamma=one, beta=one, mr=one, gx=one, gg=one, gb=one, partials=one, B=2, H=4, W=6, C=64, act=1, dtype=1):
        return h.tamtr_bncl_act_down2_bwd(gy, ldgy, x, gamma, beta, mr, gx, gg, gb, partials, B, H, W, C, act, dtype, z)

    for k in ('x', 'gamma', 'beta', 'y', 'mr', 'partials'):
        assert fwd(**{k: z}) == -1, k
    for k in ('gy', 'x', 'gamma', 'beta', 'mr', 'gx', 'gg', 'gb', 'partials'):
        assert bwd(**{k: z}) == -1, k
    for f in (fwd, bwd):
        assert f(H=5) == -2 and f(W=7) == -2 and f(H=5, W=7) == -2          # odd sizes
        assert f(B=0) == -1 and f(H=0) == -1 and f(W=-2) == -1
        assert f(C=6) == -2 and f(C=2048) == -2 and f(C=24) == -2            # C % 4; C > 1024; bf16: V = 8 and 256 % (24 / 8)
        assert f(act=2) == -1 and f(dtype=5) == -1
        assert f(x=odd) == -2
        assert f(B=1 << 20, H=1 << 10, W=1 << 10) == -2                      # more than 2e9 elements
    assert fwd(y=odd) == -2
    assert bwd(gy=odd) == -2 and bwd(gx=odd) == -2
    assert bwd(ldgy=32) == -2 and bwd(ldgy=68) == -2                         # ldgy < C; ldgy % V
    assert fwd(x=z, H=5) == -1                                               # the operands are checked first


def test_pairing_on_the_model_spec():
    from tamtr_amd.model import TAMTR_SPEC, down2_pairs
    assert down2_pairs(TAMTR_SPEC) == {13, 21, 29}
    for i in (13, 21, 29):
        assert TAMTR_SPEC[i][1] == 'Conv' and TAMTR_SPEC[i][2][1] == 1 and TAMTR_SPEC[i + 1] == [-1, 'Upsample', [0.5]]


SMALL = [[-1, 'Conv', [8, 3, 1]], [-1, 'Conv', [8, 1, 1]], [-1, 'Upsample', [0.5]], [0, 'Conv', [16, 1, 1]], [-1, 'Upsample', [0.5]],
         [[-1, 2], 'Concat', [1]], [[5], 'Detect', ['nc']]]


def test_pairing_needs_the_upsample_to_be_the_only_consumer():
    from tamtr_amd.model import down2_pairs
    assert down2_pairs(SMALL) == {1, 3}
    also_saved = [list(r) for r in SMALL]
    also_saved[5] = [[-1, 2, 1], 'Concat', [1]]             # layer 1's full map has a second consumer
    assert down2_pairs(also_saved) == {3}
    x2 = [list(r) for r in SMALL]
    x2[4] = [-1, 'Upsample', [2.0]]
    assert down2_pairs(x2) == {1}
    from_elsewhere = [list(r) for r in SMALL]
    from_elsewhere[4] = [0, 'Upsample', [0.5]]              # the Upsample does not read the Conv before it
    assert down2_pairs(from_elsewhere) == {1}
    assert down2_pairs([]) == set() and down2_pairs(SMALL[:1]) == set()


def _by_hand(model, x):
    """The layer loop as it was: every row its own call."""
    y = []
    for m in model.model[:-1]:
        if m.f != -1:
            x = y[m.f] if isinstance(m.f, int) else [x if j == -1 else y[j] for j in m.f]
        x = m(x)
        y.append(x if m.i in model.save else None)
    return x


def test_the_layer_loop_on_the_cpu_gives_what_separate_calls_give():
    """token_memory on a small spec with two pairs, in training and evaluation mode and after fuse(): the output, the running statistics
    and the call counters are those of calling every row on its own; state_dict keys are the rows' own."""
    from tamtr_amd.backbone import Conv
    from tamtr_amd.model import RTDETRDetectionWorldModel
    torch.manual_seed(0)
    model = RTDETRDetectionWorldModel(cfg=SMALL, nc=3)
    assert model.down2 == {1, 3} and model.save == [0, 2, 5]
    assert {k.split('.')[1] for k in model.state_dict() if k.startswith('model.')} >= {'0', '1', '3'}
    assert not any(k.startswith(('model.2.', 'model.4.')) for k in model.state_dict())
    model.model[-1].encode = lambda feats, drop_scales: (feats[0], None)   # the head is not under test: hand the trunk's map through
    x = torch.randn(2, 3, 8, 12)
    for mode in ('train', 'eval', 'fused'):
        if mode == 'fused':
            for m in model.model[:-1]:
                if isinstance(m, Conv):
                    m.fuse()     # the BatchNorm folded into the convolution: nothing left to pair
        model.train(mode == 'train')
        state = {k: v.clone() for k, v in model.state_dict().items()}
        with torch.no_grad():
            want = _by_hand(model, x)
        after = {k: v.clone() for k, v in model.state_dict().items()}
        model.load_state_dict(state)
        with torch.no_grad():
            got, _ = model.token_memory(x, None)
        assert got.shape == (2, 24, 4, 6) and torch.equal(got, want), mode
        for k, v in model.state_dict().items():
            assert torch.equal(v, after[k]), (mode, k)
        if mode == 'train':
            assert int(model.model[1].bn.num_batches_tracked) == 1 and not torch.equal(after['model.1.bn.running_mean'], state['model.1.bn.running_mean'])


def test_conv_then_upsample_on_the_cpu_is_the_two_calls():
    from tamtr_amd.backbone import Conv, Upsample
    torch.manual_seed(1)
    conv, up = Conv(6, 8, 1, 1).train(), Upsample(None, 0.5, 'nearest')
    x = torch.randn(2, 6, 6, 10)
    state = {k: v.clone() for k, v in conv.state_dict().items()}
    want = up(conv(x))
    conv.load_state_dict(state)
    got = conv(x, then=up)
    assert torch.equal(got, want) and got.shape == (2, 8, 3, 5)
    odd = torch.randn(2, 6, 5, 7)
    conv.load_state_dict(state)
    want = nn.Upsample(scale_factor=0.5, mode='nearest')(conv(odd))
    conv.load_state_dict(state)
    assert torch.equal(conv(odd, then=up), want)
