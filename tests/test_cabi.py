"""CPU: the C-ABI library loads and exports every symbol include/tamtr_hip.h declares (no compute without a GPU),
and the product refuses CPU tensors instead of falling back."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT


def _declared():
    src = open(os.path.join(ROOT, 'include', 'tamtr_hip.h')).read()
    return sorted(set(re.findall(r'^int\s+(tamtr_\w+)\s*\(', src, flags=re.M)))


def test_library_exports_every_declared_symbol():
    import tamtr_amd
    from tamtr_amd import _lib
    if not os.path.exists(tamtr_amd.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    names = _declared()
    assert len(names) >= 13
    h = ctypes.CDLL(tamtr_amd.LIB_PATH)
    for n in names:
        assert hasattr(h, n), f'{n} declared in tamtr_hip.h but not exported'
    assert sorted(_lib.EXPORTS) == names, 'ctypes signature table out of sync with the header'
    assert _lib.lib().tamtr_abi_version() == _lib.ABI_VERSION


def test_bad_arguments_are_rejected_without_a_gpu():
    from tamtr_amd import _lib
    h = _lib.lib()
    z = ctypes.c_void_p(0)
    assert h.tamtr_maxsigmoid_gate_fwd(z, z, z, z, z, z, z, 1, 1, 32, 16, 10, 1.0, 0, z) == -1
    assert h.tamtr_msdeform_attn_fwd(z, z, z, z, z, 1, 1, 1, 64, 1, 1, 4, 0, z) == -1
    assert h.tamtr_contrastive_logits_fwd(z, z, z, z, z, z, z, 1, 1, 1, 64, 0, z) == -1
    # next-3: the gate's 3x3 value convolution and the BatchNorm combine (null operands; channel counts the kernel is not built for)
    one = ctypes.c_void_p(16)   # a non-null, 16-byte aligned address that is never dereferenced: the checks come first
    assert h.tamtr_conv3x3_cl_stats_fwd(z, 64, z, z, z, z, z, z, 1, 8, 16, 64, 64, 1e-3, 0.03, z) == -1
    assert h.tamtr_conv3x3_cl_stats_fwd(one, 48, one, one, z, z, z, one, 1, 8, 16, 48, 64, 1e-3, 0.03, z) == -2     # C1 % 32
    assert h.tamtr_conv3x3_cl_stats_fwd(one, 64, one, one, z, z, z, one, 1, 8, 16, 64, 96, 1e-3, 0.03, z) == -2     # C2 % 64
    assert h.tamtr_conv3x3_cl_stats_fwd(one, 32, one, one, z, z, z, one, 1, 8, 16, 64, 64, 1e-3, 0.03, z) == -1     # pitch < C1
    assert h.tamtr_conv3x3_pack_weight(z, z, 64, 64, 0, z) == -1
    assert h.tamtr_conv3x3_pack_weight(one, one, 40, 64, 0, z) == -2
    assert h.tamtr_bn_finalize(z, z, z, z, 64, 10, 1e-3, 0.03, z) == -1
    assert h.tamtr_conv3x3_tiles(2, 40, 40) == 2 * 5 * 3 and h.tamtr_conv3x3_tiles(1, 8, 16) == 1
    assert h.tamtr_selective_scan_chunk() == 64                                     # checkpoint interval of hstate (ABI 23)


def test_bn_entry_points_refuse_bad_arguments_without_a_gpu():
    """Every BatchNorm entry point of csrc/bn.hip: the return code of each refusal, which also pins the order of the checks (-1 invalid,
    -2 unsupported).  Every row is refused before any launch: the non-null addresses are never dereferenced."""
    from tamtr_amd import _lib
    h = _lib.lib()
    z, one, odd = ctypes.c_void_p(0), ctypes.c_void_p(16), ctypes.c_void_p(8)   # null | 16-byte aligned | 8-byte aligned only
    eps, mom = 1e-3, 0.03

    def cl_fwd(x=one, gamma=one, partials=one, residual=z, N=8, C=64, act=0, dtype=0):
        return h.tamtr_bncl_act_fwd(x, gamma, one, z, z, residual, one, one, partials, N, C, eps, mom, act, dtype, z)

    def seg_fwd(seg_rows, seg_pitch=512, x=one, N=8, C=64):
        return h.tamtr_bncl_act_seg_fwd(x, one, one, z, z, one, seg_rows, seg_pitch, one, one, N, C, eps, mom, 0, 0, z)

    def cl_bwd(gy=one, ldgy=64, gx=one, C=64):
        return h.tamtr_bncl_act_bwd(gy, ldgy, one, one, one, one, gx, one, one, one, 8, C, 0, 0, z)

    def seg_bwd(seg_rows, seg_pitch=512, C=64):
        return h.tamtr_bncl_act_seg_bwd(one, seg_rows, seg_pitch, one, one, one, one, one, one, one, one, 8, C, 0, 0, z)

    def stats(x=one, partials=one, C=64):
        return h.tamtr_bncl_stats(x, z, z, one, partials, 8, C, eps, mom, 0, z)

    def pair_fwd(x2=one, gamma2=one):
        return h.tamtr_bncl2_act_fwd(one, one, one, z, z, x2, gamma2, one, z, z, one, one, one, 8, 64, eps, mom, 0, 0, z)

    def pair_bwd(ldgy=64, x2=one, gx2=one):
        return h.tamtr_bncl2_act_bwd(one, ldgy, one, x2, one, one, one, one, one, one, gx2, one, one, one, one, one, 8, 64, 0, 0, z)

    def nchw_fwd(x=one, gamma=one, B=2, act=0):
        return h.tamtr_bn_act_fwd(x, gamma, one, z, z, one, one, one, B, 3, 64, eps, mom, act, 0, z)

    def nchw_bwd(gx=one, HW=64):
        return h.tamtr_bn_act_bwd(one, one, one, one, one, gx, one, one, one, 2, 3, HW, 0, 0, z)

    assert cl_fwd(x=z) == -1
    assert cl_fwd(C=6) == -2
    assert cl_fwd(C=2048) == -2
    assert cl_fwd(dtype=1, C=24) == -2            # bf16: V = 8, 256 % (24 / 8)
    assert cl_fwd(act=2) == -1
    assert cl_fwd(dtype=5) == -1
    assert cl_fwd(N=0) == -1
    assert cl_fwd(x=odd) == -2
    assert cl_fwd(gamma=z) == -1
    assert cl_fwd(partials=z) == -1
    assert cl_fwd(residual=odd) == -2

    assert seg_fwd(0, x=z) == -2                  # the segment is checked before the operands
    assert seg_fwd(3) == -2                       # N % seg_rows
    assert seg_fwd(4, 128) == -2                  # seg_pitch < seg_rows * C
    assert seg_fwd(1, 12, N=2, C=12) == -2        # seg_pitch % 8
    assert seg_fwd(4, 96, C=12) == -2             # C no power of two
    assert seg_fwd(4, 512, x=z) == -1

    assert cl_bwd(gy=z) == -1
    assert cl_bwd(ldgy=32) == -2                  # ldgy < C
    assert cl_bwd(ldgy=66) == -2                  # ldgy % V
    assert cl_bwd(C=12, ldgy=12) == -2
    assert cl_bwd(gx=z) == -1
    assert cl_bwd(gx=odd) == -1
    assert cl_bwd(ldgy=32, gx=z) == -2            # the pitch is checked before the outputs

    assert seg_bwd(0) == -2
    assert seg_bwd(4, 96, C=12) == -2

    assert stats(x=z) == -1
    assert stats(partials=z) == -1
    assert stats(C=6) == -2

    assert pair_fwd(x2=z) == -1
    assert pair_fwd(gamma2=z) == -1
    assert pair_bwd(x2=z) == -1
    assert pair_bwd(gx2=z) == -1
    assert pair_bwd(ldgy=32) == -2

    assert nchw_fwd(x=z) == -1
    assert nchw_fwd(B=70000) == -2
    assert nchw_fwd(act=2) == -1
    assert nchw_fwd(gamma=z) == -1
    assert nchw_bwd(gx=z) == -1
    assert nchw_bwd(HW=0) == -1

    assert h.tamtr_bncl_blocks(8, 64, 0) == 1 and h.tamtr_bncl_blocks(0, 64, 0) == 0
    assert h.tamtr_bncl_blocks(262147, 4, 0) == 257 and h.tamtr_bncl_blocks(81925, 64, 0) == 641     # S > 256 | iters = 8
    assert h.tamtr_bn_slices(2, 4100) == 4


def test_cpu_tensors_are_refused_not_emulated():
    import tamtr_amd.ops as ops
    from tamtr_amd import TamtrHipError
    with pytest.raises(TamtrHipError):
        ops.contrastive_logits(torch.zeros(1, 1, 64), torch.zeros(1, 1, 64), torch.zeros(()), torch.zeros(1))
    with pytest.raises(TamtrHipError):
        ops.ms_deform_attn_core(torch.zeros(1, 4, 1, 8), [(2, 2)], torch.zeros(1, 1, 1, 1, 1, 2), torch.zeros(1, 1, 1, 1, 1))
    with pytest.raises(TamtrHipError):
        ops.maxsigmoid_gate(torch.zeros(1, 32, 2, 2), torch.zeros(1, 3, 32), torch.zeros(1), torch.zeros(1, 32, 2, 2), 1)


def test_product_does_not_import_the_oracle():
    pkg = os.path.join(ROOT, 'tam-tr_amd')
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith('.py'):
                s = open(os.path.join(dirpath, f)).read()
                assert not re.search(r'^\s*(from|import)\s+oracle\b', s, flags=re.M), f'{f} imports the oracle'
