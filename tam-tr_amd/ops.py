"""torch.autograd.Function wrappers around the C-ABI kernels (libtamtr_hip.so).

Each op launches on torch.cuda.current_stream(); tensors are plain device buffers to the kernels (data_ptr + sizes).
No op has a CPU or eager-PyTorch fallback: CPU tensors or a missing library raise TamtrHipError.
"""
import ctypes
import math

import torch

from . import _lib
from ._lib import call, dtype_code, ptr, require_gpu, stream_ptr
import os as _os

_PROJ_CONV_LIB = _os.environ.get('TAMTR_PROJ_CONV') == 'miopen'   # A/B switch: the gate's 3x3 value convolution on the library

_I, _F = ctypes.c_int, ctypes.c_float


def _c(t):
    return t if t.is_contiguous() else t.contiguous()


# ------------------------------------------------------------------------------------------------ layout edges
def _is_cl(t):
    return t.dim() == 4 and not t.is_contiguous() and t.is_contiguous(memory_format=torch.channels_last)


def is_cl(t):
    return _is_cl(t)


def _cl_pitch(t):
    """Pixel pitch ld if t [B,C,H,W] is a channels-last map or a channel slice of one (strides (H*W*ld, 1, W*ld, ld), ld >= C), else 0."""
    if t.dim() != 4:
        return 0
    B, C, H, W = t.shape
    sb, sc, sh, sw = t.stride()
    ok = sc == 1 and sw >= C and sh == W * sw and (B == 1 or sb == H * W * sw)
    return sw if ok else 0


class _Relayout(torch.autograd.Function):
    """Channels-last map -> NCHW-contiguous copy (to_nchw) or back, by the tiled transpose of csrc/layout.hip; values unchanged.
    The backward is the opposite repacking of the gradient."""

    @staticmethod
    def forward(ctx, x, to_nchw):
        require_gpu(x)
        ctx.to_nchw = to_nchw
        return _relayout(x, to_nchw)

    @staticmethod
    def backward(ctx, g):
        if ctx.to_nchw:   # gradient arrives NCHW-shaped; hand it back channels-last like the input was
            return (_relayout(g, False) if g.is_contiguous() else g.contiguous(memory_format=torch.channels_last)), None
        return (_relayout(g, True) if _cl_pitch(g) else g.contiguous()), None


def _relayout(x, to_nchw):
    B, C, H, W = x.shape
    if x.dtype not in (torch.float32, torch.bfloat16):
        return x.contiguous() if to_nchw else x.contiguous(memory_format=torch.channels_last)
    out = torch.empty(x.shape, dtype=x.dtype, device=x.device, memory_format=torch.contiguous_format if to_nchw else torch.channels_last)
    call('tamtr_relayout', ptr(x), ptr(out), B, C, H * W, _cl_pitch(x) if to_nchw else C, 0 if to_nchw else 1, dtype_code(x), stream_ptr())
    return out


def to_nchw(x):
    """NCHW-contiguous version of a feature map; a channels-last one (or a channel slice of one) goes through the transpose kernel."""
    if x.is_contiguous():
        return x
    return _Relayout.apply(x, True) if (x.is_cuda and _cl_pitch(x)) else x.contiguous()


class _CatChannels(torch.autograd.Function):
    """torch.cat(maps, 1) for channels-last maps (or channel slices of such): one 16-byte-vector row copy per input
    (csrc/layout.hip tamtr_copy_rows); the backward hands out channel slices of the gradient, no copies."""

    @staticmethod
    def forward(ctx, *maps):
        B, _, H, W = maps[0].shape
        widths = [m.shape[1] for m in maps]
        out = torch.empty((B, sum(widths), H, W), dtype=maps[0].dtype, device=maps[0].device, memory_format=torch.channels_last)
        ct, e, v = sum(widths), maps[0].element_size(), 16 // maps[0].element_size()
        N = B * H * W
        pitches = [_cl_pitch(m) for m in maps]
        if all(c % v == 0 and ld % v == 0 and m.data_ptr() % 16 == 0 for m, c, ld in zip(maps, widths, pitches)):
            for i in range(0, len(maps), 4):   # up to four inputs per launch
                grp = list(range(i, min(i + 4, len(maps))))
                n = len(grp)
                src = (ctypes.c_void_p * n)(*[maps[j].data_ptr() for j in grp])
                lds = (ctypes.c_longlong * n)(*[pitches[j] for j in grp])
                cs = (ctypes.c_int * n)(*[widths[j] for j in grp])
                call('tamtr_cat_rows', ctypes.cast(src, ctypes.c_void_p), ctypes.cast(lds, ctypes.c_void_p), ctypes.cast(cs, ctypes.c_void_p), n,
                     out.data_ptr() + sum(widths[:i]) * e, ct, N, dtype_code(maps[0]), stream_ptr())
        else:
            off = 0
            for m, c, ld in zip(maps, widths, pitches):
                call('tamtr_copy_rows', ptr(m), ld, out.data_ptr() + off * e, ct, N, c, dtype_code(m), stream_ptr())
                off += c
        ctx.widths = widths
        return out

    @staticmethod
    def backward(ctx, g):
        return tuple(g.split(ctx.widths, 1))


def cat_channels(maps):
    """torch.cat(maps, 1); channels-last CUDA maps of one dtype take the row-copy kernel."""
    maps = list(maps)
    if len(maps) > 1 and all(m.is_cuda and m.dim() == 4 and m.dtype == maps[0].dtype and m.dtype in (torch.float32, torch.bfloat16)
                             and m.shape[0] == maps[0].shape[0] and m.shape[2:] == maps[0].shape[2:] and _cl_pitch(m) and not m.is_contiguous()
                             for m in maps):
        return _CatChannels.apply(*maps)
    return torch.cat(maps, 1)


class _ChunkChannels(torch.autograd.Function):
    """x.chunk(2, 1) of a channels-last map with the backward on the row-copy kernel: autograd's own backward of `chunk` concatenates
    the two gradients - one of them a channel slice of a wider gradient - through torch's generic strided copy."""

    @staticmethod
    def forward(ctx, x):
        h = x.shape[1] // 2
        return x[:, :h], x[:, h:]

    @staticmethod
    def backward(ctx, g0, g1):
        return cat_channels([g0, g1])


def chunk2_channels(x):
    """x.chunk(2, 1); channels-last CUDA maps get the kernel-backed backward."""
    if x.is_cuda and _is_cl(x) and x.shape[1] % 2 == 0 and x.dtype in (torch.float32, torch.bfloat16) and x.requires_grad:
        return _ChunkChannels.apply(x)
    return x.chunk(2, 1)


class _PackChannels(torch.autograd.Function):
    """Packed channels-last copy of a channel slice of a channels-last map (what a convolution makes of `x.chunk(2, 1)[1]`)."""

    @staticmethod
    def forward(ctx, x):
        B, C, H, W = x.shape
        out = torch.empty((B, C, H, W), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
        call('tamtr_copy_rows', ptr(x), _cl_pitch(x), ptr(out), C, B * H * W, C, dtype_code(x), stream_ptr())
        return out

    @staticmethod
    def backward(ctx, g):
        return g


def pack_channels(x):
    if x.is_cuda and x.dim() == 4 and not _is_cl(x) and not x.is_contiguous() and _cl_pitch(x) and x.dtype in (torch.float32, torch.bfloat16):
        return _PackChannels.apply(x)
    return x


class _Resample2(torch.autograd.Function):
    """nn.Upsample(scale_factor=2.0 | 0.5, mode='nearest') on a channels-last map - csrc/layout.hip tamtr_resample2."""

    @staticmethod
    def forward(ctx, x, up):
        B, C, H, W = x.shape
        ctx.cfg = (up, B, C, H, W)
        Ho, Wo = (2 * H, 2 * W) if up else (H // 2, W // 2)
        out = torch.empty((B, C, Ho, Wo), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
        call('tamtr_resample2', ptr(x), ptr(out), B, H, W, C, 0 if up else 2, dtype_code(x), stream_ptr())
        return out

    @staticmethod
    def backward(ctx, g):
        up, B, C, H, W = ctx.cfg
        g = g if _is_cl(g) else (pack_channels(g) if _cl_pitch(g) else g.contiguous(memory_format=torch.channels_last))
        gx = torch.empty((B, C, H, W), dtype=g.dtype, device=g.device, memory_format=torch.channels_last)
        call('tamtr_resample2', ptr(g), ptr(gx), B, H, W, C, 1 if up else 3, dtype_code(g), stream_ptr())
        return gx, None


def resample2(x, up):
    """Nearest x2 (up) / x0.5 of a channels-last CUDA map whose channel count fills 16-byte vectors; None if the kernel does not apply."""
    v = 8 if x.dtype == torch.bfloat16 else 4
    if x.is_cuda and _is_cl(x) and x.dtype in (torch.float32, torch.bfloat16) and x.shape[1] % v == 0 and (up or (x.shape[2] % 2 == 0 and x.shape[3] % 2 == 0)):
        return _Resample2.apply(x, bool(up))
    return None


def to_channels_last(x):
    if x.dim() != 4 or _is_cl(x):
        return x
    return _Relayout.apply(x, False) if (x.is_contiguous() and x.is_cuda) else x.contiguous(memory_format=torch.channels_last)


class _MaxPool(torch.autograd.Function):
    """nn.MaxPool2d(k, s, p) on an NCHW or channels-last map - csrc/pool.hip (one-byte winner codes, gather backward)."""

    @staticmethod
    def forward(ctx, x, k, s, p):
        require_gpu(x)
        nhwc = _is_cl(x)
        if not nhwc:
            x = _c(x)
        B, C, H, W = x.shape
        Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
        fmt = torch.channels_last if nhwc else torch.contiguous_format
        y = torch.empty((B, C, Ho, Wo), dtype=x.dtype, device=x.device, memory_format=fmt)
        code = torch.empty((B, C, Ho, Wo), dtype=torch.uint8, device=x.device, memory_format=fmt)
        call('tamtr_maxpool_fwd', ptr(x), ptr(y), ptr(code), B, C, H, W, k, s, p, int(nhwc), dtype_code(x), stream_ptr())
        ctx.save_for_backward(code)
        ctx.cfg = (B, C, H, W, k, s, p, nhwc, x.dtype)
        return y

    @staticmethod
    def backward(ctx, gy):
        code, = ctx.saved_tensors
        B, C, H, W, k, s, p, nhwc, dt = ctx.cfg
        gy = gy.to(dt)
        gy = (pack_channels(gy) if _cl_pitch(gy) else gy.contiguous(memory_format=torch.channels_last)) if nhwc else _c(gy)
        gx = torch.empty((B, C, H, W), dtype=dt, device=gy.device, memory_format=torch.channels_last if nhwc else torch.contiguous_format)
        call('tamtr_maxpool_bwd', ptr(gy), ptr(code), None, ptr(gx), B, C, H, W, k, s, p, int(nhwc), dtype_code(gy), stream_ptr())
        return gx, None, None, None


def max_pool2d(x, k, s, p):
    """F.max_pool2d(x, k, s, p) for fp32 / bf16 CUDA maps (NCHW or channels-last); anything else goes to torch."""
    if x.is_cuda and x.dim() == 4 and x.dtype in (torch.float32, torch.bfloat16) and k <= 15 and 2 * p <= k:
        return _MaxPool.apply(x, int(k), int(s), int(p))
    return torch.nn.functional.max_pool2d(x, k, s, p)


# ------------------------------------------------------------------------------------------------ a-1 text gate
class _MaxSigmoidGate(torch.autograd.Function):
    """out = v * sigmoid(max_n <x, gk_n> / sqrt(hc) + bias) * scale  (extra_modules/block.py:217-226)."""

    @staticmethod
    def forward(ctx, x, gk, bias, v, nh, scale):
        require_gpu(x, gk, bias, v)
        B, C, H, W = x.shape
        T = gk.shape[1]
        hc = C // nh
        x, v = to_nchw(x), to_nchw(v)   # the kernels read NCHW planes; channels-last maps (NHWC trunk) are repacked
        gk32, b32 = _c(gk.float()), _c(bias.float())
        out = torch.empty_like(x)
        aw = torch.empty(B, nh, H * W, device=x.device, dtype=torch.float32)
        arg = torch.empty(B, nh, H * W, device=x.device, dtype=torch.int32)
        call('tamtr_maxsigmoid_gate_fwd', ptr(x), ptr(gk32), ptr(b32), ptr(v), ptr(out), ptr(aw), ptr(arg), B, nh, hc, H * W, T,
             _F(scale), dtype_code(x), stream_ptr())
        ctx.save_for_backward(x, gk32, v, aw, arg)
        ctx.cfg = (nh, hc, T, scale, gk.dtype, bias.dtype)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, gk32, v, aw, arg = ctx.saved_tensors
        nh, hc, T, scale, gk_dt, b_dt = ctx.cfg
        B, C, H, W = x.shape
        HW = H * W
        dout = _c(dout.to(x.dtype))
        dx, dv = torch.empty_like(x), torch.empty_like(x)
        dlogit = torch.empty(B, nh, HW, device=x.device, dtype=torch.float32)
        call('tamtr_maxsigmoid_gate_bwd', ptr(dout), ptr(x), ptr(gk32), ptr(v), ptr(aw), ptr(arg), ptr(dx), ptr(dv), ptr(dlogit),
             B, nh, hc, HW, T, _F(scale), dtype_code(x), stream_ptr())
        # text-side reductions: a [T x HW] x [HW x hc] batched GEMM per (image, head) - plain library GEMM
        sel = torch.zeros(B, nh, T, HW, device=x.device, dtype=torch.float32)
        sel.scatter_(2, arg.long().unsqueeze(2), dlogit.unsqueeze(2))
        dgk = torch.matmul(sel, x.view(B, nh, hc, HW).float().transpose(2, 3))  # [B,nh,T,hc]
        dgk = dgk.permute(0, 2, 1, 3).reshape(B, T, C)
        dbias = dlogit.sum((0, 2)) * math.sqrt(hc)
        return dx, dgk.to(gk_dt), dbias.to(b_dt), dv, None, None


def gate_cl_ok(x, C, nh, T=None):
    """Shapes / layouts tamtr_maxsigmoid_gate_cl_fwd takes: x a channels-last CUDA map (or a channel slice of one), C = nh * hc with
    C / 8 and hc / 8 powers of two, C <= 512; with T (the number of text rows) given, also that the fp32 text tile [T, C] fits the
    kernel's 60 KiB of LDS (T <= 60 at C = 256, 30 at C = 512)."""
    hc = C // nh if nh else 0
    lpr, lph = C // 8, hc // 8
    if T is not None and T * C * 4 > 60 * 1024:
        return False
    return (x.is_cuda and x.dtype in (torch.float32, torch.bfloat16) and _cl_pitch(x) and nh * hc == C and C % 8 == 0 and hc % 8 == 0
            and 0 < lpr <= 64 and lpr & (lpr - 1) == 0 and lph & (lph - 1) == 0 and _cl_pitch(x) % (16 // x.element_size()) == 0
            and x.data_ptr() % 16 == 0)


def conv3x3_cl_ok(x, conv):
    """What tamtr_conv3x3_cl_stats_fwd takes: a bf16 channels-last map (or a channel slice of one) into a plain 3x3 / stride 1 / pad 1
    convolution without bias, C1 % 32 == 0, C2 % 64 == 0.  TAMTR_PROJ_CONV=miopen keeps the library convolution (A/B switch)."""
    if _PROJ_CONV_LIB or not (x.is_cuda and x.dtype == torch.bfloat16 and x.dim() == 4):
        return False
    ld = _cl_pitch(x)
    return (isinstance(conv, torch.nn.Conv2d) and conv.kernel_size == (3, 3) and conv.stride == (1, 1) and conv.padding == (1, 1)
            and conv.dilation == (1, 1) and conv.groups == 1 and conv.bias is None and conv.padding_mode == 'zeros'
            and conv.in_channels == x.shape[1] and conv.in_channels % 32 == 0 and conv.out_channels % 64 == 0
            and ld and ld % 8 == 0 and x.data_ptr() % 16 == 0 and conv.weight.dtype in (torch.float32, torch.bfloat16))


@torch.no_grad()
def conv3x3_cl_stats(x, conv, bn):
    """proj_conv of the text gate (block.py:205,223) without its BatchNorm's apply pass: returns (v_raw, mean_rstd) - the raw 3x3
    convolution of the channels-last bf16 map x [B,C1,H,W] as [B,C2,H,W] channels-last bf16, and the BatchNorm's batch statistics
    f32 [C2, 2], taken in the convolution's epilogue; the running statistics and the counter of `bn` are updated like a training-mode
    forward.  Forward only (the discarded evaluation); feeds maxsigmoid_gate_cl."""
    require_gpu(x)
    B, C1, H, W = x.shape
    C2 = conv.out_channels
    w = _c(conv.weight)
    wpk = torch.empty(9 * C1 * C2, device=x.device, dtype=torch.bfloat16)
    call('tamtr_conv3x3_pack_weight', ptr(w), ptr(wpk), C1, C2, dtype_code(w), stream_ptr())
    y = torch.empty((B, C2, H, W), dtype=torch.bfloat16, device=x.device, memory_format=torch.channels_last)
    rm, rv, mom = _bn_train_call(bn)
    mr = torch.empty(C2, 2, device=x.device, dtype=torch.float32)
    part = torch.empty(C2 * _lib.lib().tamtr_conv3x3_tiles(B, H, W) * 3, device=x.device, dtype=torch.float32)
    call('tamtr_conv3x3_cl_stats_fwd', ptr(x), _cl_pitch(x), ptr(wpk), ptr(y), ptr(rm), ptr(rv), ptr(mr), ptr(part), B, H, W, C1, C2,
         float(bn.eps), float(mom), stream_ptr())
    return y, mr


@torch.no_grad()
def maxsigmoid_gate_cl(e, gk, bias, v_raw, v_stats, v_bn, nh, scale=1.0):
    """Forward-only gate on channels-last operands with the value branch's BatchNorm (batch statistics v_stats from bn_stats_cl, affine
    of v_bn) applied inside the kernel: e [B,C,H,W] channels-last or a channel slice of such, v_raw [B,C,H,W] channels-last = the raw
    proj_conv output.  Returns out [B,C,H,W] channels-last.  (The differentiable path is maxsigmoid_gate.)"""
    require_gpu(e, gk, bias, v_raw)
    B, C, H, W = e.shape
    v_raw = v_raw if _is_cl(v_raw) else v_raw.contiguous(memory_format=torch.channels_last)
    out = torch.empty((B, C, H, W), dtype=e.dtype, device=e.device, memory_format=torch.channels_last)
    gk32, b32 = _c(gk.float()), _c(bias.float())
    ga, be = _c(v_bn.weight.float()), _c(v_bn.bias.float())
    call('tamtr_maxsigmoid_gate_cl_fwd', ptr(e), _cl_pitch(e), None, None, None, ptr(v_raw), ptr(v_stats), ptr(ga), ptr(be), ptr(gk32), ptr(b32),
         ptr(out), None, None, B, nh, C // nh, H * W, gk.shape[1], _F(scale), dtype_code(e), stream_ptr())
    return out


def maxsigmoid_gate(x, gk, bias, v, nh, scale=1.0):
    """x, v: [B,C,H,W] (f32|bf16); gk: [B,T,C] guide after `gl`; bias: [nh]."""
    return _MaxSigmoidGate.apply(x, gk, bias, v, int(nh), float(scale))


# ------------------------------------------------------------------------------------------------ a-6 deformable core
_MSDA_ATOMICS = _os.environ.get('TAMTR_MSDA_ATOMICS') == '1'   # A/B switch: the round-1/2 float-atomic scatter


def deterministic():
    """TAMTR_DETERMINISTIC=1 or torch.use_deterministic_algorithms(True): the reference's `deterministic: True`
    (cfg/default.yaml:26, utils/torch_utils.py:371-389).  Kernels of this package are order-fixed by construction; the few shapes that
    only an atomic kernel serves go through _atomic_fallback(), which follows torch's own convention for nondeterministic ops."""
    return _os.environ.get('TAMTR_DETERMINISTIC') == '1' or torch.are_deterministic_algorithms_enabled()


_WARNED = set()


def _atomic_fallback(what):
    """Called before a float-atomic kernel runs in deterministic mode.  Strict mode (use_deterministic_algorithms(True)) raises, like
    torch's own nondeterministic ops; warn-only mode - what the reference sets (utils/torch_utils.py:376: warn_only=True) and what
    tuning.use_deterministic_convolutions() therefore sets - warns once per shape class and lets the atomic kernel run."""
    if not deterministic():
        return
    if torch.are_deterministic_algorithms_enabled() and not torch.is_deterministic_algorithms_warn_only_enabled():
        raise _lib.TamtrHipError(f'deterministic mode: {what}')
    if what not in _WARNED:
        _WARNED.add(what)
        import warnings
        warnings.warn(f'{what}; running the float-atomic kernel, this step is not bitwise reproducible '
                      '(torch.use_deterministic_algorithms(True) without warn_only raises here instead)', UserWarning, stacklevel=3)


def msda_sorted_ok(Q, P, D):
    return Q * P * 4 <= 8192 and D % 8 == 0 and D <= 256


class _MSDeformCore(torch.autograd.Function):
    @staticmethod
    def forward(ctx, value, shapes, loc, aw):
        require_gpu(value, loc, aw)
        B, L, M, D = value.shape
        _, Q, _, nl, P, _ = loc.shape
        value = _c(value)
        loc32, aw32 = _c(loc.float()), _c(aw.float())
        sh = (ctypes.c_int32 * (2 * nl))(*[int(v) for hw in shapes for v in hw])
        out = torch.empty(B, Q, M * D, device=value.device, dtype=value.dtype)
        call('tamtr_msdeform_attn_fwd', ptr(value), ctypes.cast(sh, ctypes.c_void_p), ptr(loc32), ptr(aw32), ptr(out), B, L, M, D,
             Q, nl, P, dtype_code(value), stream_ptr())
        ctx.save_for_backward(value, loc32, aw32)
        ctx.cfg = (sh, nl, P, loc.dtype, aw.dtype)
        return out

    @staticmethod
    def backward(ctx, gout):
        value, loc32, aw32 = ctx.saved_tensors
        sh, nl, P, loc_dt, aw_dt = ctx.cfg
        B, L, M, D = value.shape
        Q = loc32.shape[1]
        gout = _c(gout.to(value.dtype))
        gloc = torch.empty_like(loc32)
        gaw = torch.empty_like(aw32)
        if msda_sorted_ok(Q, P, D) and not _MSDA_ATOMICS:
            # ordered segmented sum (csrc/msdeform.hip): every element of the value gradient written once, in the value's dtype -
            # no 1.1 GB fp32 zero fill, no float atomics, no cast pass, and the same bits on every run
            gvalue = torch.empty(B, L, M, D, device=value.device, dtype=value.dtype)
            call('tamtr_msdeform_attn_bwd_sorted', ptr(gout), ptr(value), ctypes.cast(sh, ctypes.c_void_p), ptr(loc32), ptr(aw32),
                 ptr(gvalue), ptr(gloc), ptr(gaw), None, B, L, M, D, Q, nl, P, M * D, dtype_code(value), stream_ptr())
            return gvalue, None, gloc.to(loc_dt), gaw.to(aw_dt)
        _atomic_fallback(f'the deformable-attention backward has no atomics-free kernel for Q*P*4 = {Q * P * 4} > 8192 corners per level '
                         f'or D = {D} (csrc/msdeform.hip)')
        gvalue = torch.zeros(B, L, M, D, device=value.device, dtype=torch.float32)  # float-atomic accumulator
        call('tamtr_msdeform_attn_bwd', ptr(gout), ptr(value), ctypes.cast(sh, ctypes.c_void_p), ptr(loc32), ptr(aw32),
             ptr(gvalue), ptr(gloc), ptr(gaw), B, L, M, D, Q, nl, P, dtype_code(value), stream_ptr())
        return gvalue.to(value.dtype), None, gloc.to(loc_dt), gaw.to(aw_dt)


def ms_deform_attn_core(value, shapes, loc, aw):
    """value [B,L,M,D]; shapes [[H,W]]*nl; loc [B,Q,M,nl,P,2]; aw [B,Q,M,nl,P] -> [B,Q,M*D] (nn/modules/utils.py:42-89)."""
    return _MSDeformCore.apply(value, [tuple(int(v) for v in s) for s in shapes], loc, aw)


class _ValueProjMSDA(torch.autograd.Function):
    """MSDeformAttn's value projection and its sampling core as ONE node (reference nn/modules/transformer.py:273-311,
    nn/modules/utils.py:42-89): out = msda(x W^T + b, loc, aw).  Same kernels as linear_bf16 + ms_deform_attn_core in both directions;
    what the pairing buys is the BIAS gradient: db = column sums of d(value) over its B*L rows = sum_{b,q} gout[b,q,m,:] * colw[b,q,m],
    where colw is the weight an item put on the map (1 unless a corner falls off) - the backward kernel that computes d/d(loc), d/d(aw)
    emits it on the side, so the 550 MB pass over d(value) that colsum() made per decoder layer (111 us each) is a product of
    [B*Q, M, D] operands."""

    @staticmethod
    def forward(ctx, x, weight, bias, shapes, loc, aw, M):
        require_gpu(x, weight, bias, loc, aw)
        B, L, K = x.shape
        N = weight.shape[0]
        D = N // M
        _, Q, _, nl, P, _ = loc.shape
        x2 = _c(x.reshape(-1, K))
        w16, b32 = _c(bf16_of(weight)), _c(bias.float())
        value = _linear_bf16_fwd(x2, w16, b32).view(B, L, M, D)
        loc32, aw32 = _c(loc.float()), _c(aw.float())
        sh = (ctypes.c_int32 * (2 * nl))(*[int(v) for hw in shapes for v in hw])
        out = torch.empty(B, Q, N, device=x.device, dtype=torch.bfloat16)
        call('tamtr_msdeform_attn_fwd', ptr(value), ctypes.cast(sh, ctypes.c_void_p), ptr(loc32), ptr(aw32), ptr(out), B, L, M, D,
             Q, nl, P, dtype_code(value), stream_ptr())
        ctx.save_for_backward(x2, w16, value, loc32, aw32)
        ctx.cfg = (x.shape, sh, nl, P, M, weight.dtype, bias.dtype, loc.dtype, aw.dtype)
        return out

    @staticmethod
    def backward(ctx, gout):
        x2, w16, value, loc32, aw32 = ctx.saved_tensors
        (B, L, K), sh, nl, P, M, w_dt, b_dt, loc_dt, aw_dt = ctx.cfg
        N = w16.shape[0]
        D = N // M
        Q = loc32.shape[1]
        gout = _c(gout.to(torch.bfloat16))
        gloc, gaw = torch.empty_like(loc32), torch.empty_like(aw32)
        colw = torch.empty(B, Q, M, device=gout.device, dtype=torch.float32)
        gvalue = torch.empty(B * L, N, device=gout.device, dtype=torch.bfloat16)
        call('tamtr_msdeform_attn_bwd_sorted', ptr(gout), ptr(value), ctypes.cast(sh, ctypes.c_void_p), ptr(loc32), ptr(aw32),
             ptr(gvalue), ptr(gloc), ptr(gaw), ptr(colw), B, L, M, D, Q, nl, P, N, dtype_code(value), stream_ptr())
        gx = _linear_bf16_dx(gvalue, w16).view(B, L, K) if ctx.needs_input_grad[0] else None
        gw = dw_splitk(gvalue, x2).to(w_dt) if ctx.needs_input_grad[1] else None
        gb = (gout.view(B * Q, M, D).float() * colw.view(B * Q, M, 1)).sum(0).view(N).to(b_dt) if ctx.needs_input_grad[2] else None
        return gx, gw, gb, None, gloc.to(loc_dt), gaw.to(aw_dt), None


def value_proj_msda_ok(x, lin, n_heads, Q, P):
    """The paired node serves the bf16 token memory on the W-stationary GEMM's shapes with the sorted (atomics-free) backward
    (TAMTR_VALUE_BIAS=colsum: linear_bf16 + ms_deform_attn_core as separate nodes, the bias gradient as a pass over d(value))."""
    K, N = lin.in_features, lin.out_features
    return (x.is_cuda and x.dtype == torch.bfloat16 and x.dim() == 3 and lin.bias is not None and N % n_heads == 0 and K % 128 == 0 and N % 128 == 0
            and msda_sorted_ok(Q, P, N // n_heads) and not _MSDA_ATOMICS and _os.environ.get('TAMTR_VALUE_BIAS') != 'colsum')


def value_proj_msda(x, lin, n_heads, shapes, loc, aw):
    """msda(value_proj(x), loc, aw): x [B, L, K] bf16 -> [B, Q, N] bf16; see _ValueProjMSDA."""
    return _ValueProjMSDA.apply(x, lin.weight, lin.bias, [tuple(int(v) for v in s) for s in shapes], loc, aw, int(n_heads))


# ------------------------------------------------------------------------------------------------ a-8 contrastive head
class _ContrastiveLogits(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, logit_scale, bias):
        require_gpu(x, w, logit_scale, bias)
        B, Q, C = x.shape
        K = w.shape[1]
        x = _c(x)
        w32 = _c(w.float())
        ls, bi = _c(logit_scale.float().reshape(1)), _c(bias.float().reshape(1))
        logits = torch.empty(B, Q, K, device=x.device, dtype=torch.float32)
        xinv = torch.empty(B, Q, device=x.device, dtype=torch.float32)
        winv = torch.empty(B, K, device=x.device, dtype=torch.float32)
        call('tamtr_contrastive_logits_fwd', ptr(x), ptr(w32), ptr(ls), ptr(bi), ptr(logits), ptr(xinv), ptr(winv), B, Q, K, C,
             dtype_code(x), stream_ptr())
        ctx.save_for_backward(x, w32, ls, bi, logits, xinv, winv)
        ctx.cfg = (w.dtype, logit_scale.dtype, logit_scale.shape, bias.dtype, bias.shape)
        return logits

    @staticmethod
    def backward(ctx, g):
        x, w32, ls, bi, logits, xinv, winv = ctx.saved_tensors
        w_dt, ls_dt, ls_shape, b_dt, b_shape = ctx.cfg
        B, Q, C = x.shape
        K = w32.shape[1]
        g = _c(g.float())
        dx = torch.empty_like(x)
        if K > 16:
            _atomic_fallback(f'the contrastive head backward sums d(what) with LDS atomics for K = {K} > 16 prompts (csrc/contrastive.hip)')
        slabs = _lib.lib().tamtr_contrastive_bwd_slabs(Q)   # per-workgroup partials of d(what), added below in a fixed order
        dwhat = torch.empty(B, slabs, K, C, device=x.device, dtype=torch.float32)
        call('tamtr_contrastive_logits_bwd', ptr(g), ptr(x), ptr(w32), ptr(ls), ptr(xinv), ptr(winv), ptr(dx), ptr(dwhat), B, Q, K,
             C, dtype_code(x), stream_ptr())
        dwhat = dwhat.sum(1) if slabs > 1 else dwhat[:, 0]
        what = w32 * winv.unsqueeze(-1)
        dw = winv.unsqueeze(-1) * (dwhat - (dwhat * what).sum(-1, keepdim=True) * what)
        dls = (g * (logits - bi)).sum().reshape(ls_shape).to(ls_dt)
        dbias = g.sum().reshape(b_shape).to(b_dt)
        return dx, dw.to(w_dt), dls, dbias


def contrastive_logits(x, w, logit_scale, bias):
    """x [B,Q,C] (f32|bf16), w [B,K,C] -> f32 logits [B,Q,K] (nn/modules/block.py:534-541)."""
    return _ContrastiveLogits.apply(x, w, logit_scale, bias)


# ------------------------------------------------------------------------------------------------ a-5 token-wise linears
_SPLIT_MAX = int(_os.environ.get('TAMTR_SPLITK_MAX', '64'))   # A/B knob: slices of the row-sliced weight-gradient products


def _split_count(M, min_rows=2048, max_split=None):
    max_split = _SPLIT_MAX if max_split is None else max_split
    S = 1
    while S < max_split and M % (2 * S) == 0 and M // (2 * S) >= min_rows:
        S *= 2
    return S


_BMM_F32_OUT = None  # does this torch build take bmm(..., out_dtype=float32) on the GPU?

_DW_OWN = _os.environ.get('TAMTR_DW_OWN') != '0'   # A/B switch: 0 = every weight gradient on the batched library product, as before csrc/dwgrad.hip
# Below this many rows dW = dY^T X (and db) runs on csrc/dwgrad.hip; from it on, on the batched library product.  Measured per shape in
# profiles/r17_dw_shapes.txt: the decoder-side linears (M = B Q = 4 672) 1.25 - 3.2 x and the trunk's 1x1 convolutions at M <= 6 400 mostly
# 1.1 - 1.3 x faster; at M = 25 600 and 102 400 wins and losses alternate by shape, from 409 600 rows on the library wins throughout.
_DW_OWN_MAX_ROWS = 8192


def _dw_own_slices(g2, x2):
    """The slice count of csrc/dwgrad.hip for dW = g2^T x2, or 0 where the product stays on the library: not bf16 on the GPU, not contiguous
    or not 16-byte aligned, a shape the kernel does not serve (N, K multiples of 16), M at or above _DW_OWN_MAX_ROWS, TAMTR_DW_OWN=0."""
    if not (_DW_OWN and g2.is_cuda and x2.is_cuda and g2.dtype == torch.bfloat16 and x2.dtype == torch.bfloat16 and g2.dim() == 2 and x2.dim() == 2
            and g2.shape[0] == x2.shape[0] and 0 < g2.shape[0] < _DW_OWN_MAX_ROWS and g2.is_contiguous() and x2.is_contiguous()
            and g2.data_ptr() % 16 == 0 and x2.data_ptr() % 16 == 0):
        return 0
    return _lib.lib().tamtr_dw_slices(g2.shape[0], g2.shape[1], x2.shape[1])


def _dw_own(g2, x2, S, with_db):
    """(dW f32 [N, K], db f32 [N]) = (g2^T x2, column sums of g2) in two launches: the S row slices' partial products and column sums
    (tamtr_dw_bf16), then the ordered sum over the slices of both at once (slab_sum).  Bitwise reproducible; no memset, no atomics.
    db is zeros without with_db."""
    M, N = g2.shape
    K = x2.shape[1]
    part = torch.empty(S, N * K + N, device=g2.device, dtype=torch.float32)   # (N % 16 == 0: the row pitch N K + N needs no padding)
    call('tamtr_dw_bf16', ptr(g2), ptr(x2), ptr(part), int(with_db), M, N, K, stream_ptr())
    tot = slab_sum(part)
    return tot[:N * K].view(N, K), tot[N * K:]


def dw_splitk(g2, x2, min_rows=2048):
    """dW [N, K] = g2^T x2 for very tall operands (M = B*L rows >> N, K), fp32 result.
    A single M-reduction GEMM of this shape has only (N/64)*(K/128) = 8..32 output tiles: hipBLASLt ran it on that many
    workgroups (945 us for M = 537 600, N = K = 512: 0.3 PF/s).  Sliced into S row blocks it is ONE batched GEMM with S x
    the tiles, and the S partial products are summed in fp32.  Short operands (fewer than _DW_OWN_MAX_ROWS rows, bf16) take the own
    row-slice kernel instead (_dw_own: csrc/dwgrad.hip), whose slice count follows the shape."""
    M, N = g2.shape
    K = x2.shape[1]
    S = _dw_own_slices(g2, x2)
    if S:
        return _dw_own(g2, x2, S, False)[0]
    S = _split_count(M, min_rows)
    if S == 1:
        return (g2.t() @ x2).float()
    a, b = g2.view(S, M // S, N).transpose(1, 2), x2.view(S, M // S, K)
    global _BMM_F32_OUT
    if _BMM_F32_OUT is not False and N % 8 == 0 and K % 8 == 0:   # (skinny operands - a 4-wide box head - take the bf16 partials below)
        try:
            out = torch.bmm(a, b, out_dtype=torch.float32)
            _BMM_F32_OUT = True
            return slab_sum(out)
        except (NotImplementedError, RuntimeError, TypeError):
            if _BMM_F32_OUT:
                raise
            _BMM_F32_OUT = False
    return slab_sum(torch.bmm(a, b))


def slab_sum(t):
    """t [R, ...] (f32 | bf16, contiguous) -> f32 [...] = t.sum(0) in a fixed order in ONE kernel (csrc/fold.hip tamtr_slab_sum_rows): the
    last stage of the two-stage reductions (partial rows written by a kernel's workgroups, per-image rows, split-K slices).  torch's
    `t.sum(0)` of such a shape is a multi-workgroup reduction behind a memset node (its arrival semaphores), the node kind that breaks
    HIP-graph replays under AQL packet capture; it also needs `.float()` first for bf16 slices."""
    R = t.shape[0]
    C = t.numel() // max(R, 1)
    if not (t.is_cuda and t.dtype in (torch.float32, torch.bfloat16) and t.is_contiguous() and R > 0 and C % 4 == 0 and t.data_ptr() % 16 == 0):
        return t.float().sum(0)
    if R == 1:
        return t[0].float()
    out = torch.empty(t.shape[1:], device=t.device, dtype=torch.float32)
    call('tamtr_slab_sum_rows', ptr(t), ptr(out), R, C, dtype_code(t), stream_ptr())
    return out


def colsum(g2):
    """Column sums (fp32) of a [M, N] gradient: the bias gradient of a token-wise Linear.  Tall bf16 matrices take the streaming kernel of
    csrc/fold.hip (torch's generic reduction runs M = 537 600, N = 512 at 2.9 TB/s); everything else torch."""
    M, N = g2.shape
    if g2.is_cuda and g2.dtype == torch.bfloat16 and M >= 4096 and N % 8 == 0 and N <= 2048 and 256 % (N // 8) == 0 and g2.is_contiguous():
        nblk = _lib.lib().tamtr_colsum_blocks(M)
        part = torch.empty(nblk, N, device=g2.device, dtype=torch.float32)
        call('tamtr_colsum_bf16', ptr(g2), ptr(part), M, N, stream_ptr())
        return slab_sum(part)
    if g2.is_cuda and g2.dtype in (torch.float32, torch.bfloat16) and N % 4 == 0:
        return slab_sum(_c(g2))   # short or fp32 matrices: the ordered row sum directly (no torch reduction: see slab_sum)
    return g2.sum(0, dtype=torch.float32)


def bf16_shadow(p):
    """The bf16 copy of an fp32 parameter that the optimizer kernel keeps next to it (engine.FusedOptimStep(shadows=True)), if it is there and
    still describes the parameter's current value (same tensor version as when it was last derived); else None."""
    s = getattr(p, '_tamtr_bf16', None)
    if s is not None:
        base = getattr(p, '_tamtr_alias_of', p)   # (graphs.GraphedPart records through aliases of the parameters: the version is the real one's)
        if s._tamtr_version == base._version and s.device == p.device and s.shape == p.shape:
            return s
    return None


def bf16_of(p):
    """A weight as bf16 for this step's products: the optimizer's shadow copy when there is one (no kernel), else the cast that autocast does."""
    if p.dtype == torch.bfloat16:
        return p
    s = bf16_shadow(p)
    return s if s is not None else p.to(torch.bfloat16)


# measurement hook (bench.py): KERNEL_EVENTS['tamtr_linear_bf16'] = [] makes the forward launcher bracket the C call itself (not the
# dtype casts around it) with a pair of events on the launch stream and append (start, end, algorithmic flops)
KERNEL_EVENTS = {}


def _a16(t):
    """t, or a copy of it where it does not start on a 16-byte boundary (a contiguous view into the middle of a buffer): tamtr_linear_bf16
    refuses such operands, its kernels move 16 bytes per request.  The caller keeps the result in a name until its launch is issued: a
    copy dropped before that returns its block to the allocator, and the next copy made on the same stream is written into it first."""
    return t if t is None or t.data_ptr() % 16 == 0 else t.clone()


def _linear_bf16_fwd(x2, w16, b32):
    """y [M, N] = x2 [M, K] w16[N, K]^T + b32 (or no bias: None), bf16 in and out, on the MFMA kernel: the forward launch of every node
    below and of _ValueProjMSDA, and the one launch that the measurement hook brackets."""
    M, K = x2.shape
    N = w16.shape[0]
    y = torch.empty(M, N, device=x2.device, dtype=torch.bfloat16)
    x2, w16, b32 = _a16(x2), _a16(w16), _a16(b32)
    rec = KERNEL_EVENTS.get('tamtr_linear_bf16')
    if rec is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    call('tamtr_linear_bf16', ptr(x2), ptr(w16), ptr(b32), ptr(y), M, N, K, stream_ptr())
    if rec is not None:
        e1.record()
        rec.append((e0, e1, 2.0 * M * N * K))
    return y


def _linear_bf16_dx(g2, w16):
    """dX [M, K] = g2 [M, N] w16[N, K]: the same "NT" GEMM against W^T (a 0.5 MB transpose) on the same MFMA kernel where its shapes allow,
    else the library.  Never recorded by the measurement hook: bench.py's roofline.launches counts forward launches."""
    N, K = w16.shape
    if K % 128 == 0 and N % 64 == 0:
        gx = torch.empty(g2.shape[0], K, device=g2.device, dtype=torch.bfloat16)
        g2, wt = _a16(g2), _a16(_c(w16.t()))
        call('tamtr_linear_bf16', ptr(g2), ptr(wt), None, ptr(gx), g2.shape[0], K, N, stream_ptr())
        return gx
    return g2 @ w16


def _bias_rows(y, idx, b32):
    """The rows idx (along L) of y [B, L, N] = x W^T + b as if those rows of x had been zero: the bias."""
    if idx.numel():
        y[:, idx] = b32.to(torch.bfloat16)


def _param_grads(g2, x2, w_dt, b_dt, need_w, need_b, min_rows=2048):
    """(dW, db) of a token-wise linear from dY [M, N] and X [M, K], in the parameters' dtypes: dW = dY^T X by row slices (dw_splitk), db the
    ordered column sums of dY (colsum); None for one that is not needed (b_dt None: no bias).  Short and mid-size bf16 operands: both from
    csrc/dwgrad.hip's one product launch and one ordered sum (_dw_own)."""
    S = _dw_own_slices(g2, x2) if need_w else 0
    if S:
        with_db = b_dt is not None and need_b
        gw, gb = _dw_own(g2, x2, S, with_db)
        return gw.to(w_dt), (gb.to(b_dt) if with_db else None)
    gw = dw_splitk(g2, x2, min_rows).to(w_dt) if need_w else None
    gb = colsum(g2).to(b_dt) if (b_dt is not None and need_b) else None
    return gw, gb


def _linear_lib_bwd(needs, gy, x, w16, x_dt, w_dt, b_dt, min_rows=2048):
    """(dX, dW, db) of y = x w16^T + b run on the library: dX = dY W one library GEMM in x's dtype, cast to x_dt; the rest _param_grads."""
    N, K = w16.shape
    g2 = _c(gy.reshape(-1, N).to(x.dtype))
    x2 = _c(x.reshape(-1, K))
    gx = (g2 @ w16).view(x.shape).to(x_dt) if needs[0] else None
    return (gx,) + _param_grads(g2, x2, w_dt, b_dt, needs[1], needs[2], min_rows)


_LM_MIN_ROWS = 256   # least rows per slice of _LinearMaster's weight gradient (the measured winner: see its backward)


class _LinearMaster(torch.autograd.Function):
    """y = x W^T + b for the SHORT token-wise linears of the decoder side (M = B * Q rows; nn.Linear under bf16 autocast, transformer.py:
    539-558,869-889) with the gradients of W and b produced in fp32 FOR THE fp32 MASTERS: autocast's form casts W and b to bf16 per use, gets
    bf16 gradients for the copies (the bias gradient from a torch reduction behind a memset) and casts each back - per linear and step four
    cast kernels, a reduction and a memset around three GEMMs.  Here: the optimizer's shadow copies (ops.bf16_of), dW = dY^T X by row slices with
    fp32 output (dw_splitk), db by the ordered column-sum kernels."""

    @staticmethod
    def forward(ctx, x, weight, bias, w16=None, b16=None):
        # (w16 / b16: the caller's bf16 copies, for a SLICE of a parameter - e.g. the q/k and v rows of a packed in_proj - whose shadow is
        # the same slice of the parameter's shadow)
        w16 = bf16_of(weight) if w16 is None else w16
        b16 = None if bias is None else (bf16_of(bias) if b16 is None else b16)
        x16 = x if x.dtype == torch.bfloat16 else x.to(torch.bfloat16)
        ctx.save_for_backward(x16, w16)
        ctx.cfg = (x.dtype, weight.dtype, None if bias is None else bias.dtype)
        return torch.nn.functional.linear(x16, w16, b16)

    @staticmethod
    def backward(ctx, gy):
        x16, w16 = ctx.saved_tensors
        x_dt, w_dt, b_dt = ctx.cfg
        # M = B * Q = 4 672 rows against N x K <= 1 024 x 1 024 outputs: as ONE product the library runs it on 16 - 64 workgroups (35 us
        # whatever N and K: profiles/r03_gemm_census.txt); as 16 row slices it is a batched product on 16 x the tiles + the ordered sum (A/B: 77.5 -> 77.1 ms per step)
        return _linear_lib_bwd(ctx.needs_input_grad, gy, x16, w16, x_dt, w_dt, b_dt, _LM_MIN_ROWS) + (None, None)


class _LinearSplitK(torch.autograd.Function):
    """y = x W^T + b through the library GEMM (forward and dX); dW through dw_splitk.  For the tall-skinny linears of the
    VSS blocks (in_proj / out_proj / fc1 / fc2: M = B*H*W rows, 128..2048 features)."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        bf = x.dtype == torch.bfloat16
        w16 = bf16_of(weight) if bf else weight.to(x.dtype)
        ctx.save_for_backward(x, w16)
        ctx.cfg = (weight.dtype, None if bias is None else bias.dtype)
        return torch.nn.functional.linear(x, w16, None if bias is None else (bf16_of(bias) if bf else bias.to(x.dtype)))

    @staticmethod
    def backward(ctx, gy):
        x, w16 = ctx.saved_tensors
        w_dt, b_dt = ctx.cfg
        return _linear_lib_bwd(ctx.needs_input_grad, gy, x, w16, x.dtype, w_dt, b_dt)


class _LinearBF16(torch.autograd.Function):
    """Y = X W^T + b on the hand-written MFMA kernel (bf16 in/out, fp32 accumulate).  Backward: dX = dY W on the same kernel
    (against W^T); dW = dY^T X (a reduction over the M = B*L rows) is a batched library GEMM over row slices (dw_splitk).

    With idx (int64 [n] positions along L of x [B, L, K]: the invalid anchors of the MEH token memory, head.py:1210-1213: 1 580 of 33 600
    at 640 px): y = (x with the rows idx of every image zeroed) W^T + b, without materialising the masked x: the few masked rows of y are
    set to b.  Backward: dX with those rows zeroed, dW minus the masked rows' contribution (a small GEMM), db = column sums of dY over
    ALL rows."""

    @staticmethod
    def forward(ctx, x, weight, bias, idx):
        require_gpu(x, weight, bias)
        K = x.shape[-1]
        N = weight.shape[0]
        x2 = _c(x.reshape(-1, K))
        if x2.dtype != torch.bfloat16:
            raise _lib.TamtrHipError('linear_bf16 needs bf16 activations')
        w16 = _c(bf16_of(weight))
        b32 = _c(bias.float()) if bias is not None else None
        y = _linear_bf16_fwd(x2, w16, b32).view(*x.shape[:-1], N)
        if idx is not None:
            _bias_rows(y, idx, b32)
        ctx.save_for_backward(x2, w16, idx)
        ctx.cfg = (x.shape, weight.dtype, None if bias is None else bias.dtype)
        return y

    @staticmethod
    def backward(ctx, gy):
        x2, w16, idx = ctx.saved_tensors
        xshape, w_dt, b_dt = ctx.cfg
        N, K = w16.shape
        g2 = _c(gy.reshape(-1, N).to(torch.bfloat16))
        gx = _linear_bf16_dx(g2, w16).view(xshape) if ctx.needs_input_grad[0] else None
        masked = idx is not None and idx.numel() > 0
        gw, gb = _param_grads(g2, x2, torch.float32 if masked else w_dt, b_dt, *ctx.needs_input_grad[1:3])   # (masked: dW stays fp32 until the rows are off)
        if masked and gx is not None:
            gx.index_fill_(1, idx, 0)   # (not `gx[:, idx] = 0`: assigning a Python scalar through an index synchronises the host)
        if masked and gw is not None:
            gi, xi = g2.view(*xshape[:-1], N)[:, idx].reshape(-1, N), x2.view(xshape)[:, idx].reshape(-1, K)
            gw = (gw - (gi.t() @ xi).float()).to(w_dt)
        return gx, gw, gb, None


class _EncSelect(torch.autograd.Function):
    """The encoder side of the MEH query selection as ONE node (reference head.py:1205-1245, `_get_decoder_input`): token memory
    x [B, L, K] bf16 -> enc_output (Linear with the invalid-anchor rows treated as zero + LayerNorm) -> enc_score_head -> top-k over the
    tokens by best class score -> the picked rows of the normalised memory and of the scores.  Plus `n_dec` handles on x for the decoder
    layers' value projections (what ops.fanout gives).

    Why one node: everything downstream reads only the num_queries picked rows per image (4 800 of 537 600 at the bench shape), so the
    gradient of this whole branch with respect to the LayerNorm output, the Linear output and x is ZERO outside those rows.  Autograd
    on the separate ops runs the dense backward anyway - zero fill + sorted index_put + add for the two gathers, the score head's dX / dW
    over all rows, LayerNorm backward over all rows, the 512 x 512 dX GEMM and the split dW over all rows, a fourth 550 MB operand in the
    fan-out sum: ~1.9 ms per step - multiplying zeros.  Here the backward gathers the picked rows (Linear input, Linear output) in the
    forward, keeps NOTHING of the three [B, L, .] intermediates, does the whole chain on [B * num_queries, .] rows in fp32, and adds the
    rows' dX into the sum of the decoder handles' gradients (its own buffer).  Same function, same gradient (sums over rows lose only
    exact zeros); the forward is the same kernels as before."""

    @staticmethod
    def forward(ctx, x, w, b, gamma, beta, eps, ws, bs, invalid, nq, fixed_top, n_dec):
        require_gpu(x, w, b)
        B, L, K = x.shape
        N = w.shape[0]
        if x.dtype != torch.bfloat16:
            raise _lib.TamtrHipError('enc_select needs a bf16 token memory')
        x2 = _c(x.reshape(-1, K))
        w16, b32 = _c(bf16_of(w)), _c(b.float())
        y = _linear_bf16_fwd(x2, w16, b32).view(B, L, N)
        _bias_rows(y, invalid, b32)
        g32, be32 = _c(gamma.float()), _c(beta.float())
        mem = torch.empty_like(y)
        stats = torch.empty(B * L, 2, device=x.device, dtype=torch.float32)
        call('tamtr_layernorm_fwd', ptr(y), ptr(g32), ptr(be32), ptr(mem), ptr(stats), B * L, N, float(eps), dtype_code(y), stream_ptr())
        ws16 = bf16_of(ws)
        scores = torch.nn.functional.linear(mem, ws16, bs.to(torch.bfloat16))
        top = torch.topk(scores.max(-1).values, nq, dim=1).indices if fixed_top is None else fixed_top.to(x.device)
        bi = torch.arange(B, device=x.device).unsqueeze(-1)
        top_feat, enc_scores = mem[bi, top], scores[bi, top]
        valid = torch.ones(L, device=x.device, dtype=torch.bool)
        if invalid.numel():
            valid.index_fill_(0, invalid, False)   # (not `valid[invalid] = False`: assigning a Python scalar through an index synchronises the host)
        ctx.save_for_backward(top, x.view(B, L, K)[bi, top], y[bi, top], stats.view(B, L, 2)[bi, top], top_feat, valid[top], w16, ws16, g32)
        ctx.cfg = (x.shape, w.dtype, b.dtype, gamma.dtype, beta.dtype, ws.dtype, bs.dtype, fixed_top is None)
        ctx.mark_non_differentiable(top)
        return (top_feat, enc_scores, top) + tuple(x.view_as(x) for _ in range(int(n_dec)))

    @staticmethod
    def backward(ctx, g_feat, g_sc, _g_top, *g_dec):
        top, xr, yr, st, top_feat, vr, w16, ws16, g32 = ctx.saved_tensors
        (B, L, K), w_dt, b_dt, ga_dt, be_dt, ws_dt, bs_dt, distinct = ctx.cfg
        N, nc = w16.shape[0], ws16.shape[0]
        R = top.numel()
        gx = _sum_handles([g for g in g_dec if g is not None], (B, L, K), xr.dtype, xr.device)   # ours: the rows are added in place
        ge = g_sc.reshape(R, nc).float() if g_sc is not None else torch.zeros(R, nc, device=top.device)
        gm = ge @ ws16.float()                                                   # d/d(memory rows): score head ...
        if g_feat is not None:
            gm = gm + g_feat.reshape(R, N).float()                               # ... + the picked features' own gradient
        gws = ge.t() @ top_feat.reshape(R, N).float()
        gbs = ge.sum(0)
        st = st.reshape(R, 2)
        xh = (yr.reshape(R, N).float() - st[:, :1]) * st[:, 1:]                  # normalised rows from the forward's (mean, rstd)
        ggam, gbet = (gm * xh).sum(0), gm.sum(0)
        gxh = gm * g32
        gy = st[:, 1:] * (gxh - gxh.mean(-1, keepdim=True) - xh * (gxh * xh).mean(-1, keepdim=True))
        m = vr.reshape(R, 1).float()                                             # rows of invalid anchors entered the Linear as zeros
        xm = xr.reshape(R, K).float() * m
        gw, gb = gy.t() @ xm, gy.sum(0)
        gxr = ((gy @ w16.float()) * m).to(gx.dtype).view(B, -1, K)
        bi = torch.arange(B, device=top.device).unsqueeze(-1)
        if distinct:
            gx[bi, top] = gx[bi, top] + gxr                                      # top-k indices are distinct per image: plain gather / scatter
        else:
            gx.index_put_((bi, top), gxr, accumulate=True)                       # injected picks may repeat a row: the (sorted, ordered) accumulating form
        return (gx, gw.to(w_dt), gb.to(b_dt), ggam.to(ga_dt), gbet.to(be_dt), None, gws.to(ws_dt), gbs.to(bs_dt), None, None, None, None)


def _master_mode(x, weight):
    """bf16-autocast training on the GPU with an fp32 master weight, and _LinearMaster not switched off (TAMTR_LINEAR_MASTER=0: A/B)."""
    return (x.is_cuda and torch.is_grad_enabled() and torch.is_autocast_enabled('cuda') and torch.get_autocast_dtype('cuda') == torch.bfloat16
            and weight.dtype == torch.float32 and _os.environ.get('TAMTR_LINEAR_MASTER') != '0')


def linear_master_ok(x, lin):
    return (isinstance(lin, torch.nn.Linear) and _master_mode(x, lin.weight) and x.dtype in (torch.float32, torch.bfloat16)
            and lin.in_features % 4 == 0 and lin.out_features % 4 == 0)


def linear(x, lin):
    """lin(x) for an nn.Linear of the decoder side: in bf16 training mode on the GPU through _LinearMaster, else the module itself."""
    if linear_master_ok(x, lin):
        return _LinearMaster.apply(x, lin.weight, lin.bias)
    return lin(x)


def shared_bf16(x, *lins):
    """x as the bf16 operand of SEVERAL ops.linear calls (one cast, and one cast of the summed input gradient, instead of one per consumer);
    x itself where ops.linear would not take the _LinearMaster path."""
    if x.dtype == torch.float32 and lins and all(linear_master_ok(x, lin) for lin in lins):
        return x.to(torch.bfloat16)
    return x


def linear_rows(x, weight, bias, lo, hi):
    """F.linear(x, weight[lo:hi], bias[lo:hi]) - a row block of a packed projection (nn.MultiheadAttention's in_proj) - the same way."""
    w, b = weight[lo:hi], bias[lo:hi]
    if _master_mode(x, weight) and weight.shape[1] % 8 == 0 and (hi - lo) % 8 == 0:
        return _LinearMaster.apply(x, w, b, bf16_of(weight)[lo:hi], bf16_of(bias)[lo:hi])
    return torch.nn.functional.linear(x, w, b)


def linear_splitk(x, weight, bias=None):
    return _LinearSplitK.apply(x, weight, bias)


def linear_bf16(x, weight, bias=None):
    """x [..., K] bf16, weight [N, K], bias [N] -> [..., N] bf16 (transformer.py:273 value_proj)."""
    return _LinearBF16.apply(x, weight, bias, None)


def linear_bf16_zero_rows(x, weight, bias, idx):
    """linear_bf16 of x [B, L, K] with the rows idx (along L) treated as zero; see _LinearBF16."""
    return _LinearBF16.apply(x, weight, bias, idx)


def enc_select(x, lin, norm, score_head, invalid, nq, fixed_top=None, n_dec=0):
    """(top_feat [B, nq, hd], enc_scores [B, nq, nc], top [B, nq], n_dec handles on x) - see _EncSelect."""
    out = _EncSelect.apply(x, lin.weight, lin.bias, norm.weight, norm.bias, norm.eps, score_head.weight, score_head.bias, invalid, int(nq),
                           fixed_top, int(n_dec))
    return out[0], out[1], out[2], list(out[3:])


def enc_select_ok(x, lin, norm, score_head):
    """The one-node query selection serves the bf16 HIP path in training (TAMTR_ENC_SELECT=dense: the separate ops, A/B)."""
    return (x.is_cuda and x.dtype == torch.bfloat16 and x.dim() == 3 and torch.is_grad_enabled() and x.requires_grad
            and isinstance(lin, torch.nn.Linear) and isinstance(score_head, torch.nn.Linear) and lin.bias is not None and score_head.bias is not None
            and lin.in_features % 64 == 0 and lin.out_features % 128 == 0 and lin.out_features in (32, 64, 128, 256, 512, 1024)
            and _os.environ.get('TAMTR_ENC_SELECT') != 'dense')


# ------------------------------------------------------------------------------------------------ box refinement, fan-out sum, embedding rows
class _BoxRefine(torch.autograd.Function):
    """sigmoid(delta + inverse_sigmoid(ref)) - the decoder's box refinement (transformer.py:881-887) - as one kernel each way."""

    @staticmethod
    def forward(ctx, delta, ref):
        require_gpu(delta, ref)
        d, r = _c(delta.float()), _c(ref.float())
        out = torch.empty_like(d)
        call('tamtr_box_refine_fwd', ptr(d), ptr(r), ptr(out), d.numel(), stream_ptr())
        ctx.save_for_backward(out, r)
        ctx.cfg = (delta.dtype, ref.dtype)
        return out

    @staticmethod
    def backward(ctx, g):
        out, r = ctx.saved_tensors
        d_dt, r_dt = ctx.cfg
        g = _c(g.float())
        gd = torch.empty_like(out)
        gr = torch.empty_like(out) if ctx.needs_input_grad[1] else None
        call('tamtr_box_refine_bwd', ptr(g), ptr(out), ptr(r), ptr(gd), ptr(gr), out.numel(), stream_ptr())
        return gd.to(d_dt), None if gr is None else gr.to(r_dt)


def box_refine(delta, ref):
    """sigmoid(delta + inverse_sigmoid(ref)); delta, ref of the same shape."""
    if delta.is_cuda and delta.shape == ref.shape and delta.dtype in (torch.float32, torch.bfloat16) and _os.environ.get('TAMTR_BOX_REFINE') != 'torch':
        return _BoxRefine.apply(delta, ref)
    x = ref.clamp(min=0, max=1)
    return torch.sigmoid(delta + torch.log(x.clamp(min=1e-5) / (1 - x).clamp(min=1e-5)))


class _Fanout(torch.autograd.Function):
    """n handles on one tensor for n consumers; the backward adds their n gradients in ONE pass (csrc/fold.hip tamtr_sum_n) instead of
    autograd's n - 1 pairwise accumulations (three 2-read-1-write passes over the 550 MB token memory gradient per step)."""

    @staticmethod
    def forward(ctx, x, n):
        return tuple(x.view_as(x) for _ in range(n))

    @staticmethod
    def backward(ctx, *gs):
        live = [g for g in gs if g is not None]
        if len(live) == 1:
            return live[0], None
        return _sum_handles(live, live[0].shape, live[0].dtype, live[0].device), None


def _sum_handles(live, shape, dtype, device):
    """Sum of the gradients of fan-out handles in one pass (tamtr_sum_n) into a buffer of our own; zeros when nobody sent one."""
    if not live:
        return torch.zeros(shape, dtype=dtype, device=device)
    if len(live) == 1:
        return live[0].clone()
    g0 = live[0]
    if (g0.is_cuda and g0.dtype in (torch.float32, torch.bfloat16) and g0.numel() % 4 == 0 and len(live) <= 8
            and all(g.dtype == g0.dtype and g.shape == g0.shape for g in live)):
        live = [_c(g) for g in live]
        out = torch.empty_like(live[0])
        src = (ctypes.c_void_p * len(live))(*[g.data_ptr() for g in live])
        call('tamtr_sum_n', ctypes.cast(src, ctypes.c_void_p), len(live), ptr(out), out.numel(), dtype_code(out), stream_ptr())
        return out
    acc = live[0].clone()
    for g in live[1:]:
        acc += g
    return acc


def fanout(x, n):
    """x -> n tensors with x's values (views), whose gradients are summed in one kernel; for tensors that feed several heavy consumers."""
    if n <= 1 or not (x.requires_grad and torch.is_grad_enabled()):
        return (x,) * max(n, 1)
    return _Fanout.apply(x, int(n))


class _EmbedRows(torch.autograd.Function):
    """weight[idx] for a SMALL table and MANY lookups (the denoising queries' class embeddings, reference models/utils/ops.py:215-216:
    3 072 lookups into 11 rows at the bench shape).  torch's backward of that index is its sorted `index_put` accumulate, which walks the
    duplicates of a row one after the other: 293 us for a [11, 256] gradient.  Here: dW = onehot(idx)^T @ g, one tiny GEMM, fixed order."""

    @staticmethod
    def forward(ctx, weight, idx):
        ctx.save_for_backward(idx)
        ctx.rows = weight.shape[0]
        return weight.index_select(0, idx)

    @staticmethod
    def backward(ctx, g):
        idx, = ctx.saved_tensors
        onehot = (idx.view(1, -1) == torch.arange(ctx.rows, device=idx.device).view(-1, 1)).to(torch.float32)   # [rows, n]
        return (onehot @ g.reshape(idx.numel(), -1).float()).to(g.dtype).view(ctx.rows, *g.shape[1:]), None


def embed_rows(weight, idx):
    """weight[idx] (idx 1-D int64); on the GPU with a gradient the one-hot product backward of _EmbedRows (TAMTR_EMBED_ROWS=torch: plain index)."""
    if (weight.is_cuda and idx.dim() == 1 and weight.dim() == 2 and weight.shape[0] <= 4096 and weight.requires_grad and torch.is_grad_enabled()
            and _os.environ.get('TAMTR_EMBED_ROWS') != 'torch'):
        return _EmbedRows.apply(weight, idx)
    return weight[idx]


# ------------------------------------------------------------------------------------------------ trunk: 1x1 convolutions' weight gradient
_CONV1X1_NO_MASTER = _os.environ.get('TAMTR_CONV1X1_MASTER') == '0'   # A/B switch: the weight gradient rounded to bf16 for the cast group's copy


class _Conv1x1CL(torch.autograd.Function):
    """y = conv2d(x, w) for a 1x1 / stride 1 / ungrouped convolution on a channels-last map, with the WEIGHT gradient taken off MIOpen.
    The forward stays on the library (tuned tables).  MIOpen's weight-gradient solvers for these shapes (and, for some, its input-gradient
    solvers) split the reduction across workgroups and add with atomics into a buffer they zero with hipMemsetAsync - a memset NODE in a recorded
    graph, the one node kind that does not replay in order under the HIP runtime's AQL packet capture (profiles/r04_packet_capture_bisect.txt:
    inf / NaN weight gradients on exactly the trunk's 1x1 convolutions).  A 1x1 convolution IS a per-pixel linear map, so its backward is
    two GEMMs over the [B*H*W, C] views of the channels-last maps: dX = dY W (library GEMM) and dW [C2, C1] = dY^T X as the row-sliced
    batched product + ordered slab sum of the tall linears (dw_splitk, slab_sum) - fp32 result, bitwise reproducible, no memset, no atomics."""

    @staticmethod
    def forward(ctx, x, w, master=None):
        # master: the fp32 parameter `w` is this step's bf16 copy of (model._CastGroup).  The weight gradient comes out of the slab sum in
        # fp32: it goes to the master as it is - not rounded to bf16 for the copy's sake and widened again by the cast group's backward
        # (one cast kernel per 1x1 convolution and step, ~100 on the TAM-TR-s trunk) - and the copy gets no gradient.
        xp = x if _is_cl(x) else _pack_cl(x)            # a channel slice of a wider map: packed once, kept for the backward
        ctx.save_for_backward(xp, w)
        ctx.to_master = master is not None
        return torch.nn.functional.conv2d(xp, w)

    @staticmethod
    def backward(ctx, gy):
        xp, w = ctx.saved_tensors
        B, C1, H, W = xp.shape
        C2 = w.shape[0]
        gy = gy.to(xp.dtype)
        gp = gy if _is_cl(gy) else (_pack_cl(gy) if _cl_pitch(gy) else gy.contiguous(memory_format=torch.channels_last))
        g2, x2 = gp.permute(0, 2, 3, 1).reshape(B * H * W, C2), xp.permute(0, 2, 3, 1).reshape(B * H * W, C1)   # views of packed NHWC maps
        gx = gw = None
        if ctx.needs_input_grad[0]:   # dX [M, C1] = dY [M, C2] W [C2, C1]: a library GEMM (MIOpen's input-gradient solvers for some of these shapes memset too)
            gx = torch.mm(g2, w.view(C2, C1)).view(B, H, W, C1).permute(0, 3, 1, 2)
        if ctx.to_master:
            return gx, None, (dw_splitk(g2, x2).view(C2, C1, 1, 1) if ctx.needs_input_grad[2] else None)
        if ctx.needs_input_grad[1]:
            gw = dw_splitk(g2, x2).view(C2, C1, 1, 1).to(w.dtype)
        return gx, gw, None


def _pack_cl(x):
    """Packed channels-last copy of a channel slice of a channels-last map (no autograd: for use inside Functions)."""
    B, C, H, W = x.shape
    out = torch.empty((B, C, H, W), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
    call('tamtr_copy_rows', ptr(x), _cl_pitch(x), ptr(out), C, B * H * W, C, dtype_code(x), stream_ptr())
    return out


def conv1x1_cl_ok(x, conv):
    """A plain 1x1 / stride 1 / unpadded / ungrouped / unbiased nn.Conv2d on a channels-last (or channel-slice) fp32 / bf16 CUDA map whose
    weight needs a gradient: the case _Conv1x1CL serves."""
    return (x.is_cuda and x.dim() == 4 and x.dtype in (torch.float32, torch.bfloat16) and torch.is_grad_enabled()
            and isinstance(conv, torch.nn.Conv2d) and conv.kernel_size == (1, 1) and conv.stride == (1, 1) and conv.padding == (0, 0)
            and conv.dilation == (1, 1) and conv.groups == 1 and conv.bias is None
            and (conv.weight.requires_grad or getattr(conv.weight, '_tamtr_master', None) is not None)
            and bool(_cl_pitch(x)) and not x.is_contiguous() and x.shape[1] % 8 == 0 and x.data_ptr() % 16 == 0 and _cl_pitch(x) % 8 == 0)


def conv2d_module(conv, x):
    """conv(x) for an nn.Conv2d of the trunk; 1x1 convolutions on channels-last maps take _Conv1x1CL (library forward / input gradient,
    own weight gradient), everything else the module itself."""
    if conv1x1_cl_ok(x, conv):
        w = conv.weight
        if torch.is_autocast_enabled('cuda') and w.dtype != x.dtype and x.dtype == torch.get_autocast_dtype('cuda'):
            w = w.to(x.dtype)    # (what autocast does inside conv2d; the trunk normally hands in the layer's bf16 copies already)
        if w.dtype == x.dtype:
            master = None if _CONV1X1_NO_MASTER else getattr(w, '_tamtr_master', None)   # set by model.token_memory on the cast group's copies
            if master is not None and master.requires_grad and master.dtype == torch.float32 and master.shape == w.shape:
                return _Conv1x1CL.apply(x, w, master)
            return _Conv1x1CL.apply(x, w)
    return conv(x)


# ------------------------------------------------------------------------------------------------ a-7 self-attention
_mask_cache = []   # [(mask tensor, its _version, packed words)]: the entry keeps the mask alive, so its address cannot be reused


def pack_mask(mask):
    """bool [Q,Q] (True = blocked) -> int32 bit words [Q, ceil(Q/32)]; cached per mask tensor (reused by all layers).
    The hit test is object identity + version: an address/shape key could match a NEW mask allocated in a freed one's block."""
    if _mask_cache and _mask_cache[0][0] is mask and _mask_cache[0][1] == mask._version:
        return _mask_cache[0][2]
    words = mask_words(mask)
    _mask_cache[:] = [(mask, mask._version, words)]
    return words


def mask_words(mask):
    """pack_mask without its one-entry cache: for a caller that keeps the words itself (text.ClipTextEncoder's causal mask)."""
    Q = mask.shape[1]
    W = (Q + 31) // 32
    m = torch.zeros(mask.shape[0], W * 32, dtype=torch.int64, device=mask.device)
    m[:, :Q] = mask.to(torch.int64)
    words = (m.view(mask.shape[0], W, 32) << torch.arange(32, device=mask.device)).sum(-1)
    return torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32).contiguous()


class _SelfAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, nh, mask_bits):
        require_gpu(q, k, v)
        B, Q, C = q.shape
        dh = C // nh
        for t in (q, k, v):
            if t.stride(-1) != 1 or t.stride(0) != Q * t.stride(1):
                raise _lib.TamtrHipError('self_attention operands must be row-strided views [B,Q,C] of a packed projection')
        if not (q.dtype == k.dtype == v.dtype):
            raise _lib.TamtrHipError('self_attention operands must share a dtype')
        o = torch.empty(B, Q, C, device=q.device, dtype=q.dtype)
        lse = torch.empty(B, nh, Q, device=q.device, dtype=torch.float32)
        call('tamtr_selfattn_fwd', ptr(q), ptr(k), ptr(v), ptr(mask_bits), ptr(o), ptr(lse), B, Q, nh, dh, q.stride(1), k.stride(1),
             v.stride(1), dtype_code(q), stream_ptr())
        ctx.save_for_backward(q, k, v, o, lse, mask_bits)
        ctx.nh = nh
        return o

    @staticmethod
    def backward(ctx, go):
        q, k, v, o, lse, mask_bits = ctx.saved_tensors
        nh = ctx.nh
        B, Q, C = q.shape
        go = _c(go.to(q.dtype))
        gq, gk, gv = torch.empty_like(o), torch.empty_like(o), torch.empty_like(o)
        ws = torch.empty(B, nh, Q, device=q.device, dtype=torch.float32)
        call('tamtr_selfattn_bwd', ptr(go), ptr(q), ptr(k), ptr(v), ptr(o), ptr(lse), ptr(mask_bits), ptr(gq), ptr(gk), ptr(gv),
             ptr(ws), B, Q, nh, C // nh, q.stride(1), k.stride(1), v.stride(1), dtype_code(q), stream_ptr())
        return gq, gk, gv, None, None


def self_attention(q, k, v, nh, attn_mask=None):
    """softmax(q k^T / sqrt(dh) + mask) v per head; q,k,v [B,Q,C] (may be column slices of a packed projection);
    attn_mask bool [Q,Q], True = blocked (transformer.py:546)."""
    bits = pack_mask(attn_mask) if attn_mask is not None else None
    return _SelfAttention.apply(q, k, v, int(nh), bits)


def self_attention_packed(q, k, v, nh, mask_bits):
    """self_attention with the mask already packed by mask_words (or None)."""
    return _SelfAttention.apply(q, k, v, int(nh), mask_bits)


# ------------------------------------------------------------------------------------------------ CLIP text tower (csrc/text.hip)
def _f32c(what, *tensors):
    for t in tensors:
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
            raise _lib.TamtrHipError(f'{what}: operands must be contiguous float32 tensors (got {t.dtype}, strides {tuple(t.stride())})')


def text_embed(ids, token_embedding, positional_embedding):
    """x[n * L, W] = token_embedding[ids] + positional_embedding[:L] in fp32; ids int32 [n, L].  An id outside the vocabulary is refused
    here, before the launch (one read-back of the ids' range; prompts are encoded once and cached, so it is off the hot path)."""
    require_gpu(ids, token_embedding, positional_embedding)
    _f32c('text_embed', token_embedding, positional_embedding)
    if ids.dtype != torch.int32 or ids.dim() != 2 or not ids.is_contiguous():
        raise _lib.TamtrHipError('text_embed: ids must be a contiguous int32 [n, L] tensor')
    n, L = ids.shape
    V, W = token_embedding.shape
    if L > positional_embedding.shape[0] or positional_embedding.shape[1] != W:
        raise _lib.TamtrHipError(f'text_embed: context {L} x {W} does not fit positional_embedding {tuple(positional_embedding.shape)}')
    lo, hi = (int(v) for v in torch.aminmax(ids))
    if lo < 0 or hi >= V:
        raise _lib.TamtrHipError(f'text_embed: token ids span [{lo}, {hi}], outside the vocabulary [0, {V}) (TAMTR_EINVAL)')
    x = torch.empty(n * L, W, device=ids.device, dtype=torch.float32)
    call('tamtr_text_embed', ptr(ids), ptr(token_embedding), ptr(positional_embedding), ptr(x), n, L, W, V, stream_ptr())
    return x


_LINEAR_F32_EPI = {None: 0, 'quick_gelu': 1}


def linear_f32(x, w, b, act=None, residual=None, out=None):
    """epi(x @ w^T + b) in fp32 on the fp32 MFMA: x [M, K], w [N, K], b [N] or None; act None | 'quick_gelu'; residual [M, N] is added
    after the bias (not together with act) and may be `out` itself.  K % 32 == 0, N % 64 == 0, any M."""
    require_gpu(x, w, b, residual, out)
    _f32c('linear_f32', x, w, b, residual, out)
    if act not in _LINEAR_F32_EPI or (act is not None and residual is not None):
        raise _lib.TamtrHipError(f'linear_f32: act {act!r} with residual={residual is not None} is not an epilogue of the kernel')
    if x.dim() != 2 or w.dim() != 2 or x.shape[1] != w.shape[1] or (b is not None and b.shape != (w.shape[0],)):
        raise _lib.TamtrHipError(f'linear_f32: shapes x {tuple(x.shape)} w {tuple(w.shape)} do not form x @ w^T + b')
    M, K = x.shape
    N = w.shape[0]
    if out is None:
        out = torch.empty(M, N, device=x.device, dtype=torch.float32)
    for t in (residual, out):
        if t is not None and t.shape != (M, N):
            raise _lib.TamtrHipError(f'linear_f32: residual / out must be [{M}, {N}], got {tuple(t.shape)}')
    if out.data_ptr() == x.data_ptr():
        raise _lib.TamtrHipError('linear_f32: out must not be x (only the residual may alias the output)')
    call('tamtr_linear_f32', ptr(x), ptr(w), ptr(b), ptr(residual), ptr(out), M, N, K, 2 if residual is not None else _LINEAR_F32_EPI[act],
         stream_ptr())
    return out


def text_pool_project(x, ids, gamma, beta, proj, eps=1e-5, normalize=True):
    """Per prompt: the row of x [n * L, W] at the first maximum of ids [n, L] -> LayerNorm(gamma, beta, eps) -> @ proj [W, E], divided by
    its L2 norm when `normalize`; fp32 [n, E]."""
    require_gpu(x, ids, gamma, beta, proj)
    _f32c('text_pool_project', x, gamma, beta, proj)
    if ids.dtype != torch.int32 or ids.dim() != 2 or not ids.is_contiguous():
        raise _lib.TamtrHipError('text_pool_project: ids must be a contiguous int32 [n, L] tensor')
    n, L = ids.shape
    W, E = proj.shape
    if x.shape != (n * L, W) or gamma.shape != (W,) or beta.shape != (W,):
        raise _lib.TamtrHipError(f'text_pool_project: x {tuple(x.shape)} does not match ids {tuple(ids.shape)} and proj {tuple(proj.shape)}')
    out = torch.empty(n, E, device=x.device, dtype=torch.float32)
    call('tamtr_text_pool_project', ptr(x), ptr(ids), ptr(gamma), ptr(beta), ptr(proj), ptr(out), n, L, W, E, float(eps), int(bool(normalize)),
         stream_ptr())
    return out


# ------------------------------------------------------------------------------------------------ a-9 selective scan
def _scan_row_sums(Bn, KD, device):
    """Workspace of the scan backward's per-(image, row) sums over time (include/tamtr_hip.h: grow)."""
    return torch.empty(Bn, KD, _lib.lib().tamtr_selective_scan_row_sums(), device=device, dtype=torch.float32)


def _split_row_sums(grow, R):
    """Add the images (a fixed-order reduction: no float atomics, bitwise reproducible) and cut the row into d(Wdt) [KD, R], dA [KD, 16],
    dD [KD], d(bias) [KD]."""
    rs = slab_sum(grow)
    return rs[:, 16:16 + R], rs[:, :16], rs[:, 48], rs[:, 49]


def _scan_hstate(Bn, KD, L, N, device):
    """The state at every chunk boundary, which the scan forward leaves for its backward (include/tamtr_hip.h: hstate)."""
    chunk = _lib.lib().tamtr_selective_scan_chunk()
    return torch.empty(Bn, KD, (L + chunk - 1) // chunk, N, device=device, dtype=torch.float32)


def _scan_bwd_slabs(Bm, Dk):
    """Workspace of the scan backward's per-workgroup dB/dC slabs."""
    nslab = _lib.lib().tamtr_selective_scan_bwd_slabs(Dk)
    return torch.empty(2 * nslab * Bm.numel(), device=Bm.device, dtype=torch.float32)


def _fold_directions(gu):
    """[B, 4*Dk, L] per direction (un-reversed) -> gradient of the two stored copies [B, 2, Dk, L]."""
    g4 = gu.view(gu.shape[0], 4, -1, gu.shape[2])
    return g4[:, :2] + g4[:, 2:]


class _SelectiveScan(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, delta, A, Bm, Cm, D, dbias, xmode):
        require_gpu(u, delta, A, Bm, Cm, D, dbias)
        Bn, KD, L = delta.shape
        K, N = Bm.shape[1], Bm.shape[2]
        u, delta, A, Bm, Cm, D, dbias = (_c(t.float()) for t in (u, delta, A, Bm, Cm, D, dbias))
        y = torch.empty_like(delta)
        hstate = _scan_hstate(Bn, KD, L, N, u.device)
        call('tamtr_selective_scan_fwd', ptr(u), ptr(delta), ptr(A), ptr(Bm), ptr(Cm), ptr(D), ptr(dbias), ptr(y), ptr(hstate), Bn, K,
             KD // K, N, L, int(xmode), stream_ptr())
        ctx.save_for_backward(u, delta, A, Bm, Cm, D, dbias, hstate)
        ctx.xmode = int(xmode)
        return y

    @staticmethod
    def backward(ctx, gy):
        u, delta, A, Bm, Cm, D, dbias, hstate = ctx.saved_tensors
        Bn, KD, L = delta.shape
        K, N = Bm.shape[1], Bm.shape[2]
        gy = _c(gy.float())
        gu, gdelta = torch.empty_like(delta), torch.empty_like(delta)
        gB, gC = torch.empty_like(Bm), torch.empty_like(Cm)
        grow = _scan_row_sums(Bn, KD, u.device)
        ws = _scan_bwd_slabs(Bm, KD // K)
        call('tamtr_selective_scan_bwd', ptr(gy), ptr(u), ptr(delta), ptr(A), ptr(Bm), ptr(Cm), ptr(D), ptr(dbias), ptr(hstate), ptr(gu),
             ptr(gdelta), ptr(grow), ptr(gB), ptr(gC), ptr(ws), Bn, K, KD // K, N, L, ctx.xmode, stream_ptr())
        _, gA, gD, gbias = _split_row_sums(grow, 0)
        return (_fold_directions(gu) if ctx.xmode else gu), gdelta, gA, gB, gC, gD, gbias, None


def selective_scan(u, delta, A, Bm, Cm, D, delta_bias):
    """S6 scan with softplus(delta + bias): u, delta [B,K*Dk,L]; A [K*Dk,16]; Bm, Cm [B,K,16,L]; D, delta_bias [K*Dk]."""
    return _SelectiveScan.apply(u, delta, A, Bm, Cm, D, delta_bias, 0)


def selective_scan_cross_delta(u2, delta, A, Bm, Cm, D, delta_bias):
    """Cross-scan layout with a materialised delta (kept for testing the layout on its own)."""
    return _SelectiveScan.apply(u2, delta, A, Bm, Cm, D, delta_bias, 1)


# The host side of every kernel of the SS2D chain, once: each launcher allocates its kernel's outputs and workspaces, launches and returns
# the tensors; the chained autograd nodes below and _SS2DCore both go through them.  `pc` = 1: the big time-indexed planes (u2, y, d(y),
# d(u), d(u2)) are bf16 (include/tamtr_hip.h "bf16 PLANES"), 0: fp32.  A workspace that only the kernel reads dies with its launcher's frame.
def _plane_dtype(pc):
    return torch.bfloat16 if pc else torch.float32


def _scan_dtproj_fwd(u, dtr, Wdt, A, Bm, Cm, D, dbias, xmode, pc):
    """Scan with the dt projection inside: y [B, K*Dk, L] (a plane) and the chunk states for the backward."""
    Bn, K, R, L = dtr.shape
    KD, N = A.shape
    y = torch.empty(Bn, KD, L, device=u.device, dtype=_plane_dtype(pc))
    hstate = _scan_hstate(Bn, KD, L, N, u.device)
    call('tamtr_selective_scan_dtproj_fwd', ptr(u), ptr(dtr), ptr(Wdt), ptr(A), ptr(Bm), ptr(Cm), ptr(D), ptr(dbias), ptr(y),
         ptr(hstate), Bn, K, KD // K, N, R, L, xmode, pc, stream_ptr())
    return y, hstate


def _scan_dtproj_bwd(gy, u, dtr, Wdt, A, Bm, Cm, D, dbias, hstate, xmode, ws16, pc):
    """Backward of _scan_dtproj_fwd.  xmode 1: gy is d(y) [B, K*Dk, L]; 3: the merged gradient in its two flattenings [B, 2, Dk, L].
    Returns d(u) per direction [B, K*Dk, L] (a plane), d(dtr), dB, dC and the row sums d(Wdt), dA, dD, d(bias) of _split_row_sums."""
    Bn, K, R, L = dtr.shape
    KD, N = A.shape
    gu = torch.empty(Bn, KD, L, device=u.device, dtype=_plane_dtype(pc))
    # d(delta) is a workspace between the two backward kernels (the operand of d(dtr) = Wdt^T d(delta)); ws16: kept in bf16
    gdelta = torch.empty(Bn, KD, L, device=u.device, dtype=_plane_dtype(ws16))
    gdtr = torch.empty_like(dtr)
    gB, gC = torch.empty_like(Bm), torch.empty_like(Cm)
    grow = _scan_row_sums(Bn, KD, u.device)
    ws = _scan_bwd_slabs(Bm, KD // K)
    call('tamtr_selective_scan_dtproj_bwd', ptr(gy), ptr(u), ptr(dtr), ptr(Wdt), ptr(A), ptr(Bm), ptr(Cm), ptr(D), ptr(dbias),
         ptr(hstate), ptr(gu), ptr(gdelta), ptr(gdtr), ptr(grow), ptr(gB), ptr(gC), ptr(ws), Bn, K,
         KD // K, N, R, L, xmode, int(bool(ws16)) | (2 * pc), stream_ptr())
    return (gu, gdtr, gB, gC) + _split_row_sums(grow, R)


class _SelectiveScanDtProj(torch.autograd.Function):
    """Scan with the dt projection fused in: delta = Wdt . dtr is formed inside the kernels (never materialised)."""

    @staticmethod
    def forward(ctx, u, dtr, Wdt, A, Bm, Cm, D, dbias, xmode):
        require_gpu(u, dtr, Wdt, A, Bm, Cm, D, dbias)
        u, dtr, Wdt, A, Bm, Cm, D, dbias = (_c(t.float()) for t in (u, dtr, Wdt, A, Bm, Cm, D, dbias))
        y, hstate = _scan_dtproj_fwd(u, dtr, Wdt, A, Bm, Cm, D, dbias, int(xmode), 0)
        ctx.save_for_backward(u, dtr, Wdt, A, Bm, Cm, D, dbias, hstate)
        ctx.xmode = int(xmode)
        return y

    @staticmethod
    def backward(ctx, gy):
        gy = _c(gy.float())
        gu, gdtr, gB, gC, gW, gA, gD, gbias = _scan_dtproj_bwd(gy, *ctx.saved_tensors, ctx.xmode, False, 0)
        return (_fold_directions(gu) if ctx.xmode else gu), gdtr, gW, gA, gB, gC, gD, gbias, None


class _CrossScanInput(torch.autograd.Function):
    """u2 [B, 2, D, H*W] fp32 = SiLU(xc) in its row-major and column-major flattening (what CrossScan, csms6s.py:4-14, needs
    in the pair layout of the scan kernels) as one autograd node: three kernels forward, three backward, instead of the
    silu / float / stack / transpose chain and its slice-and-add autograd graph."""

    @staticmethod
    def forward(ctx, xc):
        B, D, H, W = xc.shape
        a = torch.nn.functional.silu(xc)  # in xc's dtype, as the reference's act (vmamba.py:951)
        u2 = torch.empty(B, 2, D, H * W, device=xc.device, dtype=torch.float32)
        u2[:, 0].view(B, D, H, W).copy_(a)
        u2[:, 1].view(B, D, W, H).copy_(a.transpose(2, 3))
        ctx.save_for_backward(xc)
        return u2

    @staticmethod
    def backward(ctx, g2):
        (xc,) = ctx.saved_tensors
        B, D, H, W = xc.shape
        ga = g2[:, 0].view(B, D, H, W) + g2[:, 1].view(B, D, W, H).transpose(2, 3)
        return torch.ops.aten.silu_backward(ga.to(xc.dtype), xc)


def cross_scan_input(xc):
    return _CrossScanInput.apply(xc)


def _dwconv_silu_cross_fwd(xz, weight, bias, D, pc):
    """u2 [B, 2, D, H*W] (a plane) from xz [B, H, W, 2*D], and the fp32 forms of the parameters that the kernels read."""
    B, H, W, C2 = xz.shape
    w = _c(weight.float().reshape(D, 9))
    bvec = _c(bias.float()) if bias is not None else None
    u2 = torch.empty(B, 2, D, H * W, device=xz.device, dtype=_plane_dtype(pc))
    call('tamtr_dwconv_silu_cross_fwd', ptr(xz), C2, ptr(w), ptr(bvec), ptr(u2), B, D, H, W, dtype_code(xz), pc, stream_ptr())
    return u2, w, bvec


def _dwconv_silu_cross_bwd(g2, xz, w, bvec, gxz, pc, w_shape, w_dt, b_dt):
    """Writes the xi half of the caller's d(xz) buffer `gxz` (the z half belongs to the gate); returns d(weight), d(bias) in the
    parameters' shape and dtypes (b_dt None: no bias)."""
    B, H, W, C2 = xz.shape
    D = w.shape[0]
    tiles = _lib.lib().tamtr_dwconv_tiles(H, W)
    ws = torch.empty(B, tiles, D, 10, device=xz.device, dtype=torch.float32)
    call('tamtr_dwconv_silu_cross_bwd', ptr(g2), ptr(xz), C2, ptr(w), ptr(bvec if b_dt is not None else None), ptr(gxz), C2,
         ptr(ws), B, D, H, W, dtype_code(xz), pc, stream_ptr())
    gwb = slab_sum(ws.view(-1, D, 10))
    return gwb[:, :9].reshape(w_shape).to(w_dt), (gwb[:, 9].to(b_dt) if b_dt is not None else None)


class _DWConvSiluCross(torch.autograd.Function):
    """SS2D front end on the in_proj output as it lies: xz [B, H, W, 2*D] (xi = the first D channels of every pixel) ->
    u2 [B, 2, D, H*W] fp32 = SiLU(dwconv3x3(xi) + bias) in both flattenings (csrc/dwconv.hip)."""

    @staticmethod
    def forward(ctx, xz, weight, bias, D):
        require_gpu(xz, weight)
        xz = _c(xz)
        u2, w, bvec = _dwconv_silu_cross_fwd(xz, weight, bias, D, 0)
        ctx.save_for_backward(xz, w, bvec if bvec is not None else w.new_empty(0))
        ctx.cfg = (weight.shape, weight.dtype, None if bias is None else bias.dtype)
        return u2

    @staticmethod
    def backward(ctx, g2):
        xz, w, bvec = ctx.saved_tensors
        gxz = torch.zeros_like(xz)  # the second half (z) gets its gradient from the gate path; autograd adds the two
        gw, gb = _dwconv_silu_cross_bwd(_c(g2.float()), xz, w, bvec, gxz, 0, *ctx.cfg)
        return gxz, gw, gb, None


def dwconv_silu_cross(xz, weight, bias, D):
    return _DWConvSiluCross.apply(xz, weight, bias, D)


def _split_len(L, min_len=1024, max_split=16):
    S = 1
    while S < max_split and L % (2 * S) == 0 and L // (2 * S) >= min_len:
        S *= 2
    return S


def _xproj_torch_fwd(wx, u2, cdt, R, N):
    """x_proj as torch ops in the compute dtype `cdt`: wx [4, C, D] (C = R + 2N), u2 [B, 2, D, L] -> (dtr [B,4,R,L], Bs [B,4,N,L],
    Cs [B,4,N,L]) fp32, contiguous, un-reversed, and what the backward reads: u2 and the two stacked weights [2C, D] in cdt.
    Directions k and k + 2 share a base copy, so it is two [2C, D] x [D, L] products."""
    C = R + 2 * N
    ub = u2.to(cdt)
    wa, wb = torch.cat([wx[0], wx[2]], 0).to(cdt), torch.cat([wx[1], wx[3]], 0).to(cdt)
    with torch.autocast('cuda', enabled=False):
        xa, xb = torch.matmul(wa, ub[:, 0]), torch.matmul(wb, ub[:, 1])  # [B, 2C, L]
    parts = tuple(torch.stack([xa[:, lo:lo + n], xb[:, lo:lo + n], xa[:, C + lo:C + lo + n], xb[:, C + lo:C + lo + n]], 1).float()
                  for lo, n in ((0, R), (R, N), (R + N, N)))
    return parts, ub, wa, wb


def _xproj_torch_bwd(gdtr, gBs, gCs, ub, wa, wb, R, N, gu2=None):
    """Backward of _xproj_torch_fwd: per copy one [D, 2C] x [2C, L] product, d/d(u2) of that copy, and the weight gradient (a
    reduction over L per image) as a batched GEMM over L slices.  With `gu2` [B, 2, D, L] each product is cast straight into its plane
    (no stack + cast) as soon as it exists; without, the two products are returned for the caller's fold.  Returns (products, the two
    stacked weight gradients [2C, D] fp32)."""
    Bn, _, D, L = ub.shape
    C = R + 2 * N
    S = _split_len(L)
    gws, ms = [], []
    with torch.autocast('cuda', enabled=False):
        for i, w in ((0, wa), (1, wb)):
            gx = torch.cat([gdtr[:, i], gBs[:, i], gCs[:, i], gdtr[:, i + 2], gBs[:, i + 2], gCs[:, i + 2]], 1).to(ub.dtype)  # [B, 2C, L]
            m = torch.matmul(w.t(), gx)                                                                                      # [B, D, L]
            if gu2 is None:
                ms.append(m)
            else:
                gu2[:, i].copy_(m)
            ga = gx.view(Bn, 2 * C, S, L // S).transpose(1, 2).reshape(Bn * S, 2 * C, L // S)
            ua = ub[:, i].reshape(Bn, D, S, L // S).transpose(1, 2).reshape(Bn * S, D, L // S)
            gws.append(slab_sum(torch.bmm(ga, ua.transpose(1, 2))))  # [2C, D]
    return ms, gws


def _xproj_unstack_wgrad(gws, C, dt):
    """The gradients of the two stacked weights [2C, D] (rows [W_i ; W_(i+2)] of copy i) -> d(x_proj_weight) [4, C, D]."""
    return torch.stack([gws[0][:C], gws[1][:C], gws[0][C:], gws[1][C:]], 0).to(dt)


class _XProjCross(torch.autograd.Function):
    """x_proj of SS2D (vmamba.py:962-970) on the pair layout in autocast's dtype, with an explicit backward of the output assembly
    (one concatenation per copy instead of ~30 slice kernels): _xproj_torch_fwd / _xproj_torch_bwd."""

    @staticmethod
    def forward(ctx, wx, u2, R, N):
        cdt = torch.get_autocast_dtype('cuda') if torch.is_autocast_enabled('cuda') else torch.float32
        parts, ub, wa, wb = _xproj_torch_fwd(wx, u2, cdt, R, N)
        ctx.save_for_backward(ub, wa, wb)
        ctx.cfg = (R, N, wx.dtype, u2.dtype)
        return parts

    @staticmethod
    def backward(ctx, gdtr, gBs, gCs):
        ub, wa, wb = ctx.saved_tensors
        R, N, w_dt, u_dt = ctx.cfg
        gu2 = torch.empty(ub.shape, device=ub.device, dtype=u_dt)
        _, gws = _xproj_torch_bwd(gdtr, gBs, gCs, ub, wa, wb, R, N, gu2)
        return _xproj_unstack_wgrad(gws, R + 2 * N, w_dt), gu2, None, None


def x_proj_cross(wx, u2, R, N):
    return _XProjCross.apply(wx, u2, R, N)


def _cross_merge_fwd(y, H, W, pc):
    """CrossMerge (csms6s.py:26-34) of the scan's planes y [B, 4*Dk, H*W] straight into [B, H*W, Dk] fp32 (what out_norm / out_proj
    consume): one tiled-transpose kernel."""
    Bn, Dk = y.shape[0], y.shape[1] // 4
    ymT = torch.empty(Bn, H * W, Dk, device=y.device, dtype=torch.float32)
    call('tamtr_cross_merge_fwd', ptr(y), ptr(ymT), Bn, Dk, H, W, pc, stream_ptr())
    return ymT


def _cross_merge_bwd(gm, H, W, pc):
    """gm [B, H*W, Dk] fp32 -> the merged gradient in its two flattenings [B, 2, Dk, H*W] (a plane), the xmode 3 operand of the scan
    backward."""
    Bn, L, Dk = gm.shape
    g2 = torch.empty(Bn, 2, Dk, L, device=gm.device, dtype=_plane_dtype(pc))
    call('tamtr_cross_merge_bwd', ptr(gm), ptr(g2), Bn, Dk, H, W, pc, stream_ptr())
    return g2


class _SelectiveScanCrossMerged(torch.autograd.Function):
    """Cross-scan + fused dt projection + CrossMerge (csms6s.py:4-46) as one autograd node: forward returns the merged map
    [B, Dk, H*W]; backward hands the scan kernel the merged gradient in its two flattenings instead of four planes (the
    slice/add autograd graph of the merge cost 5.4 ms per level-0 block: 1.7 GB zero fills, copies and adds)."""

    @staticmethod
    def forward(ctx, u2, dtr, Wdt, A, Bm, Cm, D, dbias, H, W, token_major=False):
        require_gpu(u2, dtr, Wdt, A, Bm, Cm, D, dbias)
        u2, dtr, Wdt, A, Bm, Cm, D, dbias = (_c(t.float()) for t in (u2, dtr, Wdt, A, Bm, Cm, D, dbias))
        y, hstate = _scan_dtproj_fwd(u2, dtr, Wdt, A, Bm, Cm, D, dbias, 1, 0)
        ctx.save_for_backward(u2, dtr, Wdt, A, Bm, Cm, D, dbias, hstate)
        ctx.hw = (H, W, token_major)
        if token_major:
            return _cross_merge_fwd(y, H, W, 0)
        Bn, _, Dk, L = u2.shape
        y = y.view(Bn, 4, Dk, L)
        ym = y[:, 0] + y[:, 2]
        ym += (y[:, 1] + y[:, 3]).view(Bn, Dk, W, H).transpose(2, 3).reshape(Bn, Dk, L)
        return ym

    @staticmethod
    def backward(ctx, gm):
        H, W, token_major = ctx.hw
        if token_major:
            g2 = _cross_merge_bwd(_c(gm.float()), H, W, 0)
        else:
            Bn, Dk, L = gm.shape
            g2 = torch.empty(Bn, 2, Dk, L, device=gm.device, dtype=torch.float32)
            g2[:, 0] = gm
            g2[:, 1].view(Bn, Dk, W, H).copy_(gm.view(Bn, Dk, H, W).transpose(2, 3))
        gu, gdtr, gB, gC, gW, gA, gD, gbias = _scan_dtproj_bwd(g2, *ctx.saved_tensors, 3, False, 0)
        return _fold_directions(gu), gdtr, gW, gA, gB, gC, gD, gbias, None, None, None


def selective_scan_cross_merged(u2, dtr, Wdt, A, Bm, Cm, D, delta_bias, H, W, token_major=False):
    """selective_scan_cross followed by the cross-merge: returns [B, Dk, H*W] in row-major pixel order, or with
    token_major=True [B, H*W, Dk] (needs Dk % 32 == 0)."""
    return _SelectiveScanCrossMerged.apply(u2, dtr, Wdt, A, Bm, Cm, D, delta_bias, H, W, token_major)


def _ln_gate_fwd(x, xz, gamma, beta, eps):
    """out = LayerNorm(x; gamma, beta) * SiLU(z) in xz's dtype, the per-token statistics, and the fp32 forms of gamma and beta."""
    D = x.shape[-1]
    ntok = x.numel() // D
    g32, b32 = _c(gamma.float()), _c(beta.float())
    out = torch.empty(x.shape, device=x.device, dtype=xz.dtype)
    stats = torch.empty(ntok, 2, device=x.device, dtype=torch.float32)
    call('tamtr_ln_gate_fwd', ptr(x), ptr(xz), xz.shape[-1], ptr(g32), ptr(b32), ptr(out), ptr(stats), ntok, D, float(eps),
         dtype_code(xz), stream_ptr())
    return out, stats, g32, b32


def _ln_gate_bwd(gout, x, xz, g32, b32, stats, gxz):
    """Writes the z half of the caller's d(xz) buffer `gxz` (the xi half belongs to the front end); returns d(x) and the fp32 sums
    [2, D]: d(gamma), d(beta)."""
    D = x.shape[-1]
    ntok = x.numel() // D
    gx = torch.empty_like(x)
    nblk = _lib.lib().tamtr_ln_gate_blocks(ntok)
    part = torch.empty(nblk, 2, D, device=x.device, dtype=torch.float32)
    call('tamtr_ln_gate_bwd', ptr(gout), ptr(x), ptr(xz), xz.shape[-1], ptr(g32), ptr(b32), ptr(stats), ptr(gx), ptr(gxz), ptr(part),
         ntok, D, dtype_code(xz), stream_ptr())
    return gx, slab_sum(part)


class _LNGate(torch.autograd.Function):
    """out = LayerNorm(x; gamma, beta) * SiLU(z) with z = the second half of the channels-last in_proj output xz [B,H,W,2D]
    (vmamba.py:1005-1008,1029-1036) - csrc/ss2d_out.hip.  x fp32 [B, L, D] -> out [B, L, D] in xz's dtype."""

    @staticmethod
    def forward(ctx, x, xz, gamma, beta, eps):
        require_gpu(x, xz, gamma, beta)
        x, xz = _c(x.float()), _c(xz)
        out, stats, g32, b32 = _ln_gate_fwd(x, xz, gamma, beta, eps)
        ctx.save_for_backward(x, xz, g32, b32, stats)
        ctx.cfg = (gamma.dtype, beta.dtype)
        return out

    @staticmethod
    def backward(ctx, gout):
        x, xz, g32, b32, stats = ctx.saved_tensors
        gout = _c(gout.to(xz.dtype))
        gxz = torch.zeros_like(xz)  # the xi half gets its gradient from the conv path; autograd adds the two
        gx, gsum = _ln_gate_bwd(gout, x, xz, g32, b32, stats, gxz)
        return gx, gxz, gsum[0].to(ctx.cfg[0]), gsum[1].to(ctx.cfg[1]), None


def ln_gate(x, xz, gamma, beta, eps=1e-5):
    return _LNGate.apply(x, xz, gamma, beta, eps)


# ------------------------------------------------------------------------------------------------ a-10 loss terms (csrc/detrloss.hip)
class _DetrLayerLosses(torch.autograd.Function):
    """(class, bbox, giou) terms of all stacked decoder layers of one DETRLoss._layers call (loss.py:85-166,282-326 of the reference's
    models/utils: varifocal class loss on the matched IoU, 5 x L1, 2 x (1 - RIOU)) in three launches forward and two backward
    (csrc/detrloss.hip) instead of ~190 elementwise / gather / scatter / reduce launches each way.  fp32; sums in a fixed order."""

    @staticmethod
    def forward(ctx, pb, ps, gt_bboxes, gt_cls, li, bi, si, gi, n, gains):
        require_gpu(pb, ps, gt_bboxes, gt_cls, li, bi, si, gi)
        pb, ps, gt_bboxes = _c(pb.float()), _c(ps.float()), _c(gt_bboxes.float())
        gt_cls, li, bi, si, gi = (_c(t.long()) for t in (gt_cls, li, bi, si, gi))
        Lr, B, nq, nc = ps.shape
        dev = pb.device
        tgt = torch.empty(Lr, B, nq, device=dev, dtype=torch.int64).fill_(nc)      # (fill kernels, not memsets: tam-tr_amd/graphs.py)
        score = torch.empty(Lr, B, nq, device=dev, dtype=torch.float32).fill_(0.0)
        pair = torch.empty(2, Lr * n, device=dev, dtype=torch.float32)
        partial = torch.empty(Lr * _lib.lib().tamtr_detr_blocks(B * nq), device=dev, dtype=torch.float32)
        out = torch.empty(3, Lr, device=dev, dtype=torch.float32)
        gc, gb, gg = (float(v) for v in gains)
        call('tamtr_detr_layers_fwd', ptr(pb), ptr(ps), ptr(gt_bboxes), ptr(gt_cls), ptr(li), ptr(bi), ptr(si), ptr(gi), Lr, B, nq, nc, n, ptr(tgt),
             ptr(score), ptr(pair[0]), ptr(pair[1]), ptr(partial), gc, gb, gg, ptr(out), stream_ptr())
        ctx.save_for_backward(pb, ps, gt_bboxes, li, bi, si, gi, tgt, score)
        ctx.cfg = (n, gc, gb, gg)
        return out[0], out[1], out[2]

    @staticmethod
    def backward(ctx, g_cls, g_box, g_iou):
        pb, ps, gt_bboxes, li, bi, si, gi, tgt, score = ctx.saved_tensors
        n, gc, gb, gg = ctx.cfg
        Lr, B, nq, nc = ps.shape
        up = torch.stack([g_cls, g_box, g_iou]).float().contiguous()
        gpb = torch.empty_like(pb).fill_(0.0)
        gps = torch.empty_like(ps)
        call('tamtr_detr_layers_bwd', ptr(pb), ptr(ps), ptr(gt_bboxes), ptr(li), ptr(bi), ptr(si), ptr(gi), ptr(tgt), ptr(score), ptr(up), Lr, B, nq, nc, n,
             gc, gb, gg, ptr(gpb), ptr(gps), stream_ptr())
        return gpb, gps, None, None, None, None, None, None, None, None


def detr_layer_losses(pb, ps, gt_bboxes, gt_cls, li, bi, si, gi, n, gains):
    """pb [Lr,B,nq,4], ps [Lr,B,nq,nc], flat matched pairs (layer-major, n per layer) -> three [Lr] tensors (class, bbox, giou)."""
    return _DetrLayerLosses.apply(pb, ps, gt_bboxes, gt_cls, li, bi, si, gi, int(n), tuple(gains))


@torch.no_grad()
def detr_match_cost(ps, pb, gt_bboxes, gt_cls, gains, alpha, gamma):
    """The Hungarian matcher's cost (models/utils/ops.py:84-112) of all layers at once: ps [Lr,B,nq,nc] logits, pb [Lr,B,nq,4] ->
    C f32 [Lr, B, nq, G] over the flattened box list, non-finite entries zeroed."""
    require_gpu(ps, pb, gt_bboxes, gt_cls)
    Lr, B, nq, nc = ps.shape
    G = gt_bboxes.shape[0]
    ps, pb, gt_bboxes, gt_cls = _c(ps.float()), _c(pb.float()), _c(gt_bboxes.float()), _c(gt_cls.long())
    C = torch.empty(Lr, B, nq, G, device=ps.device, dtype=torch.float32)
    call('tamtr_detr_match_cost', ptr(ps), ptr(pb), ptr(gt_bboxes), ptr(gt_cls), Lr * B * nq, nc, G, float(gains[0]), float(gains[1]), float(gains[2]),
         float(alpha), float(gamma), ptr(C), stream_ptr())
    return C


# ------------------------------------------------------------------------------------------------ x_proj of SS2D (csrc/xproj.hip)
_SS2D_PLANES_F32 = _os.environ.get('TAMTR_SS2D_PLANES') == 'f32'   # A/B switch: the cross-scan planes in fp32 also in bf16 mode (rounds 1-3)


def ss2d_bf16_planes(dtype, D, L, R, N):
    """bf16 mode keeps SS2D's big time-indexed planes in bf16 (include/tamtr_hip.h "bf16 PLANES"): every kernel of the chain has that form
    only on its vector path and with the own x_proj kernels."""
    return dtype == torch.bfloat16 and not _SS2D_PLANES_F32 and L % 8 == 0 and xproj_ok(dtype, D, L, R, N)


_XPROJ_LIB = _os.environ.get('TAMTR_XPROJ') == 'torch'   # A/B switch: the torch-op form (cast, two batched library GEMMs, stack, ...)


def xproj_ok(cdt, D, L, R, N):
    """What tamtr_xproj_{fwd, bwd_dx, bwd_dw} take: the bf16 mode, d_state 16, d_inner a multiple of 256, L a multiple of 8."""
    return not _XPROJ_LIB and cdt == torch.bfloat16 and N == 16 and 1 <= R <= 32 and D % 256 == 0 and L % 8 == 0


def xproj_pack_weight(wx):
    """x_proj_weight [4, C, D] -> bf16 [2, MP, D]: rows [W_i ; W_(i+2)] per stored copy i, zero-padded to a multiple of 32 rows."""
    C = wx.shape[1]
    w = torch.stack([torch.cat([wx[0], wx[2]], 0), torch.cat([wx[1], wx[3]], 0)]).to(torch.bfloat16)
    pad = (-2 * C) % 32
    return _c(torch.nn.functional.pad(w, (0, 0, 0, pad)) if pad else w)


def xproj_pack_weight_t(wcat, C):
    """[2, MP, D] -> bf16 [2, D, KP]: the transposed blocks for the d/d(u2) product, zero-padded to a multiple of 16 columns."""
    w = wcat[:, :2 * C].transpose(1, 2)
    pad = (-2 * C) % 16
    return _c(torch.nn.functional.pad(w, (0, pad)) if pad else w)


class _SS2DCore(torch.autograd.Function):
    """SS2D between in_proj and out_proj as ONE autograd node (vmamba.py:949-1008): depthwise 3x3 + SiLU + cross-scan layout ->
    x_proj -> selective scan with the dt projection inside -> cross-merge -> out_norm x SiLU(z).  It calls the launchers that
    dwconv_silu_cross / x_proj_cross / selective_scan_cross_merged / ln_gate chained call, so the kernels and the arithmetic are theirs;
    only the x_proj on own kernels (csrc/xproj.hip) has no chained form.  What the single node buys is the backward's buffer plan,
    which autograd otherwise dictates:
      * d/d(u2) = fold of the scan's four planes + the two x_proj products in one pass (csrc/fold.hip) instead of a slice add, a cast
        and an accumulation (5 reads + 3 writes of an 839 MB plane pair at level 0 -> 3 + 1);
      * d/d(xz): the gate kernel writes the z half and the depthwise-conv kernel the xi half of ONE buffer (before: two zero-filled
        [B,H,W,2D] maps and their sum).
    The `del` statements are that plan: a plane is released as soon as its last reader has been launched."""

    @staticmethod
    def forward(ctx, xz, conv_w, conv_b, wx, Wdt, A, Ds, dbias, gamma, beta, eps, R, N):
        require_gpu(xz, conv_w, wx, Wdt, A, Ds, dbias, gamma, beta)
        xz = _c(xz)
        B, H, W, C2 = xz.shape
        D, L, K = C2 // 2, H * W, 4
        # bf16 mode: the big time-indexed planes that only cross HBM between kernels (u2, y, and in the backward d(y), d(u), d(u2)) are bf16;
        # the recurrence, its states and every gradient sum stay fp32 (include/tamtr_hip.h "bf16 PLANES")
        pc = int(ss2d_bf16_planes(xz.dtype, D, L, R, N))
        u2, cw, cb = _dwconv_silu_cross_fwd(xz, conv_w, conv_b, D, pc)
        # x_proj on the two copies (directions k and k + 2 share one)
        cdt = xz.dtype if xz.dtype == torch.bfloat16 else torch.float32
        own_xp = xproj_ok(cdt, D, L, R, N)
        ub = wa = wb = wcat = None
        if own_xp:   # csrc/xproj.hip: u2 read once as f32, the three outputs written in the scan's layout
            wcat = xproj_pack_weight(wx)
            dtr, Bs, Cs = (torch.empty(B, K, n, L, device=xz.device, dtype=torch.float32) for n in (R, N, N))
            call('tamtr_xproj_fwd', ptr(u2), ptr(wcat), ptr(dtr), ptr(Bs), ptr(Cs), B, D, L, R, pc, stream_ptr())
        else:
            (dtr, Bs, Cs), ub, wa, wb = _xproj_torch_fwd(wx, u2, cdt, R, N)
        # scan + cross-merge, token-major
        Wdt32, A32, D32, db32 = (_c(t.float()) for t in (Wdt, A, Ds, dbias))
        y, hstate = _scan_dtproj_fwd(u2, dtr, Wdt32, A32, Bs, Cs, D32, db32, 1, pc)
        ymT = _cross_merge_fwd(y, H, W, pc)
        del y
        # out_norm x SiLU(z)
        out, stats, g32, b32 = _ln_gate_fwd(ymT, xz, gamma, beta, eps)
        none = cw.new_empty(0)
        ctx.save_for_backward(xz, cw, cb if cb is not None else none, u2, ub if ub is not None else none, wa if wa is not None else none,
                              wb if wb is not None else none, wcat if wcat is not None else none, dtr, Bs, Cs, Wdt32, A32, D32, db32, hstate,
                              ymT, g32, b32, stats)
        ctx.own_xp = own_xp
        ctx.cfg = (R, N, H, W, conv_w.shape, conv_w.dtype, None if conv_b is None else conv_b.dtype, wx.dtype, Wdt.dtype, A.dtype, Ds.dtype,
                   dbias.dtype, gamma.dtype, beta.dtype)
        return out

    @staticmethod
    def backward(ctx, gout):
        (xz, cw, cb, u2, ub, wa, wb, wcat, dtr, Bs, Cs, Wdt32, A32, D32, db32, hstate, ymT, g32, b32, stats) = ctx.saved_tensors
        R, N, H, W, cw_shape, cw_dt, cb_dt, wx_dt, wdt_dt, a_dt, d_dt, db_dt, ga_dt, be_dt = ctx.cfg
        B, _, _, C2 = xz.shape
        D, L, C = C2 // 2, H * W, R + 2 * N
        pc = int(u2.dtype == torch.bfloat16)   # the planes' element type (forward's choice)
        # gate: d/d(ymT), the z half of d/d(xz), d(gamma), d(beta)
        gxz = torch.empty_like(xz)   # z half from the gate kernel here, xi half from the depthwise-conv kernel below
        gout = _c(gout.to(xz.dtype))
        gy, gsum = _ln_gate_bwd(gout, ymT, xz, g32, b32, stats, gxz)
        # cross-merge and scan
        g2 = _cross_merge_bwd(gy, H, W, pc)
        del gy
        # in bf16 mode d(dtr) is rounded to bf16 below anyway, so the d(delta) workspace is kept in bf16
        ws16 = pc or (xz.dtype == torch.bfloat16 and L % 4 == 0)
        gu, gdtr, gB, gC, gW, gA, gD, gdb = _scan_dtproj_bwd(g2, u2, dtr, Wdt32, A32, Bs, Cs, D32, db32, hstate, 3, ws16, pc)
        del g2
        gu2 = torch.empty(B, 2, D, L, device=xz.device, dtype=_plane_dtype(pc))
        if ctx.own_xp:
            # csrc/xproj.hip: d/d(u2) = fold of the scan's four planes + Wcat^T G in one pass; dWcat as per-slice partial tiles + ordered sum
            wT = xproj_pack_weight_t(wcat, C)
            call('tamtr_xproj_bwd_dx', ptr(gu), ptr(gdtr), ptr(gB), ptr(gC), ptr(wT), ptr(gu2), B, D, L, R, pc, stream_ptr())
            del gu
            nsl = _lib.lib().tamtr_xproj_dw_slices(L)
            part = torch.empty(B * nsl, 2, 2 * C, D, device=xz.device, dtype=torch.float32)
            call('tamtr_xproj_bwd_dw', ptr(u2), ptr(gdtr), ptr(gB), ptr(gC), ptr(part), B, D, L, R, pc, stream_ptr())
            gws = slab_sum(part)
            del part
        else:
            ms, gws = _xproj_torch_bwd(gdtr, gB, gC, ub, wa, wb, R, N)
            call('tamtr_fold_add', ptr(gu), ptr(_c(ms[0])), ptr(_c(ms[1])), ptr(gu2), B, D * L, dtype_code(ms[0]), stream_ptr())
            del gu, ms
        gwx = _xproj_unstack_wgrad(gws, C, wx_dt)
        # front end: the xi half of d/d(xz), d(conv weight), d(conv bias)
        gcw, gcb = _dwconv_silu_cross_bwd(gu2, xz, cw, cb, gxz, pc, cw_shape, cw_dt, cb_dt)
        return (gxz, gcw, gcb, gwx, gW.to(wdt_dt), gA.to(a_dt), gD.to(d_dt), gdb.to(db_dt), gsum[0].to(ga_dt), gsum[1].to(be_dt), None, None,
                None)


def ss2d_core(xz, conv_w, conv_b, x_proj_weight, Wdt, A, Ds, dt_bias, out_norm_weight, out_norm_bias, eps, R, N):
    """xz [B,H,W,2D] (in_proj output) -> out_norm(cross-merged scan) * SiLU(z) as [B, H*W, D] in xz's dtype; see _SS2DCore."""
    return _SS2DCore.apply(xz, conv_w, conv_b, x_proj_weight, Wdt, A, Ds, dt_bias, out_norm_weight, out_norm_bias, float(eps), int(R), int(N))


def selective_scan_cross(u2, dtr, Wdt, A, Bm, Cm, D, delta_bias):
    """Cross-scan layout + fused dt projection: u2 [B,2,Dk,L] (row-major / column-major copies), dtr [B,4,R,L] low-rank dt
    factors, Wdt [4*Dk, R]; Bm, Cm [B,4,16,L]; everything stored UN-reversed (directions 2, 3 walk the buffers backwards).
    Returns y [B, 4*Dk, L] (un-reversed)."""
    return _SelectiveScanDtProj.apply(u2, dtr, Wdt, A, Bm, Cm, D, delta_bias, 1)


@torch.no_grad()
def lsap_assign(cost, gt_groups):
    """Device-side Hungarian assignment (models/utils/ops.py:98-119 without the host round trip).
    cost f32 [bs, nq, G] on the GPU, gt_groups: python list of boxes per image (sum == G).
    Returns int64 device tensors (batch_idx, query_idx, gt_idx) of length sum(min(nq, n_b)): scipy's pairs in scipy's
    order, gt_idx already offset into the flattened box list.  No synchronisation."""
    require_gpu(cost)
    bs, nq, G = cost.shape
    groups = [int(n) for n in gt_groups]
    if len(groups) != bs or sum(groups) != G:
        raise _lib.TamtrHipError(f'lsap_assign: group sizes {groups} do not tile cost {tuple(cost.shape)}')
    m = sum(min(nq, n) for n in groups)
    out = torch.empty(3, m, device=cost.device, dtype=torch.int64)
    if m:
        cost = _c(cost.float())
        sizes = (ctypes.c_int32 * bs)(*groups)
        call('tamtr_lsap_assign', ptr(cost), ctypes.cast(sizes, ctypes.c_void_p), bs, nq, G, ptr(out[0]), ptr(out[1]), ptr(out[2]),
             stream_ptr())
    return out[0], out[1], out[2]


def _f32_at_most(x):
    """Largest float32 <= x: `iou_f32 > it` is then the same test as torchvision's `iou_f32 > x` in double."""
    import numpy as np
    f = np.float32(x)
    return float(np.nextafter(f, np.float32(-np.inf)) if float(f) > x else f)


def _f32_nearest(x):
    """The float32 nearest to x: what torch turns a Python scalar into before it compares an fp32 tensor with it."""
    import numpy as np
    return float(np.float32(x))


def _class_filter(classes):
    """classes: None, a tensor or a list -> (i32 tensor or None, n_classes).  An empty filter keeps nothing (the reference's `.any(1)`
    over no classes) and still needs a non-NULL pointer: it travels as one zero with n_classes = 0."""
    if classes is None:
        return None, 0
    cl = torch.as_tensor(classes, dtype=torch.int32).reshape(-1)
    return (cl if cl.numel() else torch.zeros(1, dtype=torch.int32, device=cl.device)), cl.numel()


def _upload(dev, *parts):
    """Flat i32 / f32 operands (None passes through) -> the same, contiguous, those on the host now on dev: they go up in ONE copy (a
    float operand travels as its bits), without synchronisation."""
    host = [p for p in parts if p is not None and not p.is_cuda]
    up = iter(torch.cat([p.view(torch.int32) for p in host]).to(dev, non_blocking=True).split([p.numel() for p in host])) if host else None
    return [None if p is None else _c(p if p.is_cuda else next(up).view(p.dtype)) for p in parts]


def _merge_operands(vt_host, classes, dev, B, max_out, nd, n_counters):
    """What tta_merge and slice_merge share: the view table f32 (host) and the class filter on dev in one copy, and the outputs
    -> (vt, cl, n_classes, ym f32 [B, max_out, nd], src i32 [B, max_out], n_counters counters i32 [B])."""
    cl, n_cl = _class_filter(classes)
    vt, cl = _upload(dev, vt_host.reshape(-1), cl)
    ym = torch.empty(B, max(max_out, 0), nd, device=dev, dtype=torch.float32)
    src = torch.empty(B, max(max_out, 0), device=dev, dtype=torch.int32)
    return vt, cl, n_cl, ym, src, tuple(torch.empty(B, device=dev, dtype=torch.int32) for _ in range(n_counters))


@torch.no_grad()
def detect_postprocess(y, orig_hw, conf, iou, classes=None, single_cls=False, max_wh=7680.):
    """RTDETRPredictor.postprocess (models/rtdetrworld/predict.py:34-78) for the whole batch in one launch: class max,
    `score > conf` (and the class filter), class-aware NMS with torchvision's rule, boxes scaled to the original images.
    y (f32 / bf16) [B, nq, 4 + nc] eval output on the GPU; orig_hw [B, 2] (h, w) and classes: tensors or lists.
    Returns device tensors out f32 [B, nq, 6] (x1 y1 x2 y2 score cls, zero after the count), keep i32 [B, nq] (source query,
    -1 after the count), counts i32 [B].  No synchronisation (orig_hw / classes given as lists cost one small upload)."""
    require_gpu(y)
    if y.dim() != 3:
        raise _lib.TamtrHipError(f'detect_postprocess: expected y [B, nq, 4 + nc], got {tuple(y.shape)}')
    B, nq, nd = y.shape
    dev = y.device
    y = _c(y if y.dtype in (torch.float32, torch.bfloat16) else y.float())
    hw = torch.as_tensor(orig_hw, dtype=torch.int32)
    if tuple(hw.shape) != (B, 2):
        raise _lib.TamtrHipError(f'detect_postprocess: orig_hw must be [B, 2] = [{B}, 2], got {tuple(hw.shape)}')
    cl, n_cl = _class_filter(classes)
    hw, cl = _upload(dev, hw.reshape(-1), cl)      # host operands go up in one copy
    out = torch.empty(B, nq, 6, device=dev, dtype=torch.float32)
    keep = torch.empty(B, nq, device=dev, dtype=torch.int32)
    counts = torch.empty(B, device=dev, dtype=torch.int32)
    call('tamtr_detect_postprocess', ptr(y), dtype_code(y), B, nq, nd, ptr(hw), float(conf), _f32_at_most(float(iou)), int(bool(single_cls)),
         float(max_wh), ptr(cl) if cl is not None else None, n_cl, ptr(out), ptr(keep), ptr(counts), stream_ptr())
    return out, keep, counts


def tta_view_sizes(H, W, ratio, gs=64):
    """scale_img's sizes (utils/torch_utils.py:322-326), in Python double: content (sh, sw) = (int(H ratio), int(W ratio)) and canvas
    (Hp, Wp) = (ceil(H ratio / gs) gs, ceil(W ratio / gs) gs)."""
    import math
    ratio, gs = float(ratio), int(gs)
    if not (ratio > 0 and math.isfinite(ratio)) or gs < 1 or H < 1 or W < 1:
        raise _lib.TamtrHipError(f'tta view: ratio must be positive and finite, gs and the input size at least 1; got ratio {ratio!r}, gs {gs}, '
                                 f'size {(H, W)}')
    sh, sw = int(H * ratio), int(W * ratio)
    if sh < 1 or sw < 1:
        raise _lib.TamtrHipError(f'tta view: ratio {ratio} leaves nothing of a {H} x {W} input')
    return (sh, sw), (math.ceil(H * ratio / gs) * gs, math.ceil(W * ratio / gs) * gs)


def tta_view_factors(views, size, gs=64):
    """[(ratio, flip)] and the input size (H, W) -> [(kx, ky, flip)]: what a view's normalised cx / w (kx) and cy / h (ky) are
    multiplied by to land in the input's normalised frame: canvas pixels (Wp), / ratio as _descale_pred divides (nn/tasks.py:289),
    / W.  Computed in double, rounded to fp32: ratio 1 on a size that is a multiple of gs gives exactly 1.0."""
    import numpy as np
    H, W = (int(s) for s in size)
    out = []
    for ratio, flip in views:
        _, (Hp, Wp) = tta_view_sizes(H, W, ratio, gs)
        out.append((float(np.float32(Wp / (float(ratio) * W))), float(np.float32(Hp / (float(ratio) * H))), bool(flip)))
    return out


@torch.no_grad()
def tta_view(x, ratio, flip, gs=64):
    """One test-time-augmentation view of a batch in one launch (csrc/tta.hip): scale_img(x.flip(3) if flip else x, ratio, gs)
    (utils/torch_utils.py:316-327) - bilinear align_corners=False to (int(H ratio), int(W ratio)), padded with 0.447 to the next
    multiples of gs.  x f32 [B, 3, H, W] on the GPU -> f32 [B, 3, Hp, Wp].  ratio 1 is a copy (mirrored when flip), bit for bit.
    No synchronisation."""
    require_gpu(x)
    if x.dim() != 4 or x.shape[1] != 3 or x.dtype != torch.float32:
        raise _lib.TamtrHipError(f'tta_view: expected x f32 [B, 3, H, W], got {x.dtype} {tuple(x.shape)}')
    B, _, H, W = x.shape
    (sh, sw), (Hp, Wp) = tta_view_sizes(H, W, ratio, gs)
    x = _c(x)
    out = torch.empty(B, 3, Hp, Wp, device=x.device, dtype=torch.float32)
    call('tamtr_tta_view', ptr(x), ptr(out), B, H, W, sh, sw, Hp, Wp, int(bool(flip)), stream_ptr())
    return out


@torch.no_grad()
def tta_merge(ys, views, conf, iou, classes=None, single_cls=False, max_wh=7680., max_out=512, size=None, gs=64):
    """The views' raw eval outputs of a batch -> one ordinary prediction tensor, in one launch (csrc/tta.hip): every row de-augmented
    as _descale_pred does (nn/tasks.py:286-295: descale, then de-flip), the views concatenated along the query axis (tasks.py:284) and
    merged by the predictor's NMS rule (class max, `score > conf`, the class filter, class-aware torchvision NMS; detect_postprocess
    states it).  ys: V tensors (all f32 or all bf16) [B, nq, 4 + nc] on the GPU, V * nq <= 2048 and V <= 16; views: V entries
    (ratio, flip) with `size` = the input's (H, W) and the views' gs (tta_view_factors), or V ready (kx, ky, flip) with size=None;
    classes: a tensor or a list.  Returns device tensors ym f32 [B, max_out, 4 + nc] (the first max_out survivors in NMS order:
    de-augmented cx cy w h and the source row's scores; zero rows after the count), src i32 [B, max_out] (candidate v * nq + q, -1
    after the count), counts i32 [B], dropped i32 [B] (survivors beyond max_out).  ym goes to detect_postprocess,
    val_postprocess_match and the rest unchanged, with the same conf / iou / classes / single_cls: they keep what the same rule keeps
    of the concatenation.  With identity views ((1, False) each) the op is the NMS merge of the reference's Ensemble (nn/tasks.py
    Ensemble.forward: torch.cat(y, 1) of several models' outputs).  No synchronisation (views and classes go up in one copy)."""
    ys = list(ys)
    if not ys:
        raise _lib.TamtrHipError('tta_merge: needs at least one view output')
    require_gpu(*ys)
    y0 = ys[0]
    if y0.dim() != 3 or any(y.shape != y0.shape or y.dtype != y0.dtype or y.device != y0.device for y in ys):
        raise _lib.TamtrHipError(f'tta_merge: expected V tensors of one shape [B, nq, 4 + nc], dtype and device, got '
                                 f'{[(y.dtype, tuple(y.shape)) for y in ys]}')
    if y0.dtype not in (torch.float32, torch.bfloat16):
        ys = [y.float() for y in ys]
    ys = [_c(y) for y in ys]
    V, (B, nq, nd), dev = len(ys), ys[0].shape, ys[0].device
    views = list(views)
    table = tta_view_factors(views, size, gs) if size is not None else [(float(kx), float(ky), bool(f)) for kx, ky, f in views]
    if len(table) != V:
        raise _lib.TamtrHipError(f'tta_merge: {V} outputs need {V} views, got {len(table)}')
    max_out = int(max_out)
    vt = torch.tensor([[kx, ky, float(f), 0.0] for kx, ky, f in table], dtype=torch.float32)
    vt, cl, n_cl, ym, src, (counts, dropped) = _merge_operands(vt, classes, dev, B, max_out, nd, 2)
    pv = (ctypes.c_void_p * V)(*[y.data_ptr() for y in ys])
    call('tamtr_tta_merge', ctypes.cast(pv, ctypes.c_void_p), V, dtype_code(ys[0]), B, nq, nd, ptr(vt), float(conf), _f32_at_most(float(iou)),
         int(bool(single_cls)), float(max_wh), ptr(cl) if cl is not None else None, n_cl, max_out, ptr(ym), ptr(src), ptr(counts),
         ptr(dropped), stream_ptr())
    return ym, src, counts, dropped


SLICE_MAX_VIEWS, SLICE_MAX_CAND = 64, 4096      # csrc/slice.hip: views per frame, candidates that may pass the filter per frame
SLICE_MATCH = {'iou': 0, 'ios': 1}


def _slice_windows_array(what, windows):
    import numpy as np
    win = np.ascontiguousarray(np.asarray(windows, dtype=np.int64).reshape(-1, 4).astype(np.int32))
    if not len(win):
        raise _lib.TamtrHipError(f'{what}: needs at least one window')
    return win


def slice_view_factors(windows, view_off, hws):
    """Windows i32 [N, 4] (x0 y0 x1 y1 in pixels), the frames' view ranges view_off [B + 1] and sizes hws [B] (h, w) -> f32 numpy
    [N, 4] = ox oy kx ky, what maps a view's normalised box to its frame's: ox = x0 / w, oy = y0 / h, kx = (x1 - x0) / w,
    ky = (y1 - y0) / h, each computed in double and rounded once.  The whole frame gives exactly (0, 0, 1, 1)."""
    import numpy as np
    win = _slice_windows_array('slice_view_factors', windows)
    off = [int(o) for o in view_off]
    hws = [(int(h), int(w)) for h, w in hws]
    if len(off) != len(hws) + 1 or off[0] != 0 or off[-1] != len(win) or any(b <= a for a, b in zip(off, off[1:])):
        raise _lib.TamtrHipError(f'slice: view_off {off} must run from 0 to the {len(win)} views in {len(hws)} non-empty steps')
    out = np.empty((len(win), 4), np.float32)
    for b, (h, w) in enumerate(hws):
        for v in range(off[b], off[b + 1]):
            x0, y0, x1, y1 = (int(t) for t in win[v])
            out[v] = (x0 / w, y0 / h, (x1 - x0) / w, (y1 - y0) / h)
    return out


@torch.no_grad()
def slice_views(src, windows, S, out=None):
    """The windows of one original frame as network inputs, in one launch (csrc/slice.hip): src u8 [h, w, 3] on the GPU (RGB, as
    data.decode_image returns it), windows i32 [V, 4] on the host (x0 y0 x1 y1 in pixels inside the frame, V <= 64) -> f32
    [V, 3, S, S], out[v] = data.resize_linear_u8 of the crop (a copy at S x S, the 2 x 2 mean at 2S x 2S, else the fixed-point
    two-pass rule), CHW, * float(1 / 255) - what predict.letterbox_scalefill and to_model_input make of the crop, bit for bit.
    out: a contiguous f32 [V, 3, S, S] tensor (e.g. a slice of a larger batch) to write into.  No synchronisation."""
    require_gpu(src)
    if src.dim() != 3 or src.shape[2] != 3 or src.dtype != torch.uint8:
        raise _lib.TamtrHipError(f'slice_views: expected src u8 [h, w, 3], got {src.dtype} {tuple(src.shape)}')
    win = _slice_windows_array('slice_views', windows)
    V, S = len(win), int(S)
    src = _c(src)
    if out is None:
        out = torch.empty(V, 3, max(S, 0), max(S, 0), device=src.device, dtype=torch.float32)
    elif tuple(out.shape) != (V, 3, S, S) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != src.device:
        raise _lib.TamtrHipError(f'slice_views: out must be a contiguous f32 [{V}, 3, {S}, {S}] on {src.device}, got {out.dtype} {tuple(out.shape)}')
    call('tamtr_slice_views', ptr(src), src.shape[0], src.shape[1], win.ctypes.data_as(ctypes.c_void_p), V, S, ptr(out), stream_ptr())
    return out


@torch.no_grad()
def slice_merge(y, view_off, windows, hws, conf, iou, classes=None, single_cls=False, match='iou', max_wh=7680., max_out=512):
    """The raw eval outputs of all views of a batch -> one ordinary prediction tensor, in one launch (csrc/slice.hip), one workgroup
    per frame.  y (f32 / bf16) [N, nq, 4 + nc] on the GPU; frame b owns views view_off[b] .. view_off[b + 1] - 1 (host ints [B + 1], at
    most 64 views per frame, nq <= 512); windows i32 [N, 4] and hws [B] (h, w) on the host give every view's place in its frame
    (slice_view_factors).  Every row is mapped to its frame (cx' = cx kx + ox ...) and the frame's candidates are merged by
    tta_merge's rule: class max, `score > conf`, the class filter, class-aware greedy NMS on `match`: 'iou' (torchvision's) or 'ios'
    (intersection over the smaller box), both `> iou`.  The candidates that pass the filter are compacted in ascending order into a
    table of 4096; those beyond it are left out and counted.  Returns device tensors ym f32 [B, max_out, 4 + nc], src i32 [B, max_out]
    (candidate v_local * nq + q, -1 after the count), counts, dropped (survivors beyond max_out), overflow (passing candidates beyond
    the table) i32 [B].  ym goes to detect_postprocess unchanged with the same conf / iou / classes / single_cls.  No synchronisation
    (the factors and classes go up in one copy)."""
    require_gpu(y)
    if y.dim() != 3:
        raise _lib.TamtrHipError(f'slice_merge: expected y [N, nq, 4 + nc], got {tuple(y.shape)}')
    if match not in SLICE_MATCH:
        raise _lib.TamtrHipError(f"slice_merge: match must be 'iou' or 'ios', got {match!r}")
    y = _c(y if y.dtype in (torch.float32, torch.bfloat16) else y.float())
    N, nq, nd = y.shape
    dev = y.device
    off = [int(o) for o in view_off]
    B = len(off) - 1
    fac = slice_view_factors(windows, off, hws)
    if len(fac) != N:
        raise _lib.TamtrHipError(f'slice_merge: {N} view outputs need {N} windows, got {len(fac)}')
    max_out = int(max_out)
    vt, cl, n_cl, ym, src, (counts, dropped, overflow) = _merge_operands(torch.from_numpy(fac), classes, dev, B, max_out, nd, 3)
    offs = (ctypes.c_int32 * (B + 1))(*off)
    call('tamtr_slice_merge', ptr(y), dtype_code(y), N, B, nq, nd, ctypes.cast(offs, ctypes.c_void_p), ptr(vt), SLICE_MATCH[match], float(conf),
         _f32_at_most(float(iou)), int(bool(single_cls)), float(max_wh), ptr(cl) if cl is not None else None, n_cl, max_out, ptr(ym), ptr(src),
         ptr(counts), ptr(dropped), ptr(overflow), stream_ptr())
    return ym, src, counts, dropped, overflow


TRACK_STATE_SPEC =(('mean', torch.float64, (8,)), ('cov', torch.float64, (8, 8)), ('meta', torch.int32, (8,)), ('sc', torch.float32, (2,)))


def _check_streams(what, streams):
    """streams=None: one tracker, today's shapes.  streams=S: S stacked trackers -> S as an int."""
    if streams is None:
        return None
    if isinstance(streams, bool) or not isinstance(streams, int) or streams < 1:
        raise _lib.TamtrHipError(f'{what}: streams must be None or a positive int, got {streams!r}')
    return streams


def _check_state(what, state, wanted, note=''):
    """Every (key, dtype, full shape) of `wanted` must be a contiguous tensor of that dtype and shape in the dict `state`; `note`
    says in the message what fixed the shapes."""
    for k, dt, want in wanted:
        t = state.get(k) if isinstance(state, dict) else None
        if t is None or t.dtype != dt or tuple(t.shape) != want or not t.is_contiguous():
            got = None if t is None else (t.dtype, tuple(t.shape))
            raise _lib.TamtrHipError(f'{what}: state[{k!r}] must be a contiguous {dt} tensor of shape {want}{note and f" ({note})"}, got {got}')


def _check_counts(what, counts, B, name='counts'):
    if not torch.is_tensor(counts) or tuple(counts.shape) != (B,) or counts.dtype != torch.int32:
        got = (counts.dtype, tuple(counts.shape)) if torch.is_tensor(counts) else type(counts).__name__
        raise _lib.TamtrHipError(f'{what}: {name} must be an int32 tensor [B] = [{B}], got {got}')


def _workspace(what, workspace, need, device, align=None):
    """The caller's workspace, checked (align: the pointer must be a multiple of it), or a new one of `need` bytes."""
    if workspace is None:
        workspace = torch.empty(need, device=device, dtype=torch.uint8)
    require_gpu(workspace)
    if workspace.dtype != torch.uint8 or workspace.numel() < need or not workspace.is_contiguous() or (align and workspace.data_ptr() % align):
        aligned = f', {align}-byte aligned' if align else ''
        raise _lib.TamtrHipError(f'{what}: workspace must be a contiguous{aligned} uint8 tensor of at least {need} bytes')
    return workspace


def bytetrack_workspace_bytes(capacity, nq, streams=None):
    """Bytes of device workspace tamtr_bytetrack_update needs for a table of `capacity` slots and nq rows per frame (no GPU call);
    streams=S: what tamtr_bytetrack_update_streams needs for S stacked tables."""
    S = _check_streams('bytetrack', streams)
    L = _lib.lib()
    n = L.tamtr_bytetrack_workspace_bytes(int(capacity), int(nq)) if S is None else L.tamtr_bytetrack_streams_workspace_bytes(S, int(capacity), int(nq))
    if n <= 0:
        raise _lib.TamtrHipError(f'bytetrack: capacity {capacity} with nq {nq}' + (f' and {S} streams' if S else '') +
                                 ' is outside what the kernel is built for')
    return n


def bytetrack_update(out, counts, state, capacity, track_high_thresh=0.5, track_low_thresh=0.1, new_track_thresh=0.6, match_thresh=0.8,
                     max_time_lost=30, workspace=None, streams=None):
    """BYTETracker.update (trackers/byte_tracker.py:238-351) for the B frames of a batch, in order, in one launch; the rule is stated
    in csrc/track.hip.  out f32 [B, nq, 6] and counts i32 [B] are detect_postprocess's outputs on the GPU; state: the tracker's table,
    a dict of device tensors mean f64 [T, 8], cov f64 [T, 8, 8], meta i32 [T, 8], sc f32 [T, 2], hdr i32 [8] with T = capacity,
    updated in place.  Returns device tensors tracks f32 [B, nq, 8] (x1 y1 x2 y2 id score cls idx, zero after the count) and
    tcounts i32 [B].  hdr[3] counts the new tracks that found no free slot.  Every check comes before the launch; no synchronisation.
    streams=S: one tracker per stream, still one launch (trackers/track.py:33-53).  The B = F * S images are frame-major, image
    f * S + s being the f-th frame of stream s; every state tensor carries a leading S (mean [S, T, 8] ... hdr [S, 8]) and the
    workspace is bytetrack_workspace_bytes(T, nq, S).  Stream s gets what streams=None computes on its own images and state[k][s],
    bit for bit.  A stream without a frame at some position keeps its image, with counts 0."""
    return _tracker_update('bytetrack_update', None, out, counts, state, capacity, track_high_thresh, track_low_thresh, new_track_thresh,
                           match_thresh, max_time_lost, workspace, streams=streams)


def botsort_update(out, counts, state, capacity, warps=None, track_high_thresh=0.5, track_low_thresh=0.1, new_track_thresh=0.6,
                   match_thresh=0.8, max_time_lost=30, workspace=None, streams=None):
    """BOTSORT.update (trackers/bot_sort.py; with_reid off, as the reference runs it) for the B frames of a batch, in order, in one
    launch: bytetrack_update's operands, table layout, workspace and outputs, with the XYWH filter and the frames' warps; the rule is
    stated in csrc/track.hip.  warps f64 [B, 2, 3] on the GPU, in the pixels of `out` (gmc_estimate's output or the caller's own);
    None = the identity for every frame.  Every check comes before the launch; no synchronisation.  streams=S as in bytetrack_update
    (warps stay [B, 2, 3], one per image)."""
    return _tracker_update('botsort_update', warps, out, counts, state, capacity, track_high_thresh, track_low_thresh, new_track_thresh,
                           match_thresh, max_time_lost, workspace, streams=streams)


REID_MAX_D = 1024


def botsort_reid_workspace_bytes(capacity, nq, streams=None):
    """Bytes of device workspace tamtr_botsort_reid_update needs (its cost matrix is fp64; no GPU call); streams=S: what
    tamtr_botsort_reid_update_streams needs for S stacked tables."""
    S = _check_streams('botsort_reid', streams)
    L = _lib.lib()
    n = L.tamtr_botsort_reid_workspace_bytes(int(capacity), int(nq)) if S is None else \
        L.tamtr_botsort_reid_streams_workspace_bytes(S, int(capacity), int(nq))
    if n <= 0:
        raise _lib.TamtrHipError(f'botsort_reid: capacity {capacity} with nq {nq}' + (f' and {S} streams' if S else '') +
                                 ' is outside what the kernel is built for')
    return n


def reid_rows(embed, keep, counts):
    """One feature row per kept detection, for botsort_reid_update: feat[b, j] = embed[b, keep[b, j]] widened to fp32 and divided by
    its norm twice (what BOTrack.__init__ does to a detection's feature, bot_sort.py:50-64) for j < counts[b], zero after.  embed
    f32 | bf16 [B, nqm, D] (e.g. the decoder's per-query hidden state), keep i32 [B, nq] and counts i32 [B] are detect_postprocess's;
    all on the GPU.  Returns feat f32 [B, nq, D].  One launch; every check comes before it; no synchronisation."""
    if not torch.is_tensor(embed) or embed.dim() != 3 or min(embed.shape) < 1:
        got = tuple(embed.shape) if torch.is_tensor(embed) else type(embed).__name__
        raise _lib.TamtrHipError(f'reid_rows: expected embed [B, nqm, D], got {got}')
    B, nqm, D = embed.shape
    if D > REID_MAX_D:
        raise _lib.TamtrHipError(f'reid_rows: D = {D} is above the {REID_MAX_D} the kernels are built for')
    if not torch.is_tensor(keep) or keep.dim() != 2 or keep.shape[0] != B or keep.shape[1] < 1 or keep.dtype != torch.int32:
        got = (keep.dtype, tuple(keep.shape)) if torch.is_tensor(keep) else type(keep).__name__
        raise _lib.TamtrHipError(f'reid_rows: keep must be an int32 tensor [B, nq] with B = {B}, got {got}')
    _check_counts('reid_rows', counts, B)
    code = dtype_code(embed)
    require_gpu(embed, keep, counts)
    embed, keep, counts = _c(embed), _c(keep), _c(counts)
    nq = keep.shape[1]
    feat = torch.empty(B, nq, D, device=embed.device, dtype=torch.float32)
    call('tamtr_reid_rows', ptr(embed), code, ptr(keep), ptr(counts), B, nqm, nq, D, ptr(feat), stream_ptr())
    return feat


def botsort_reid_update(out, counts, feat, state, capacity, warps=None, track_high_thresh=0.5, track_low_thresh=0.1, new_track_thresh=0.6,
                        match_thresh=0.8, max_time_lost=30, proximity_thresh=0.5, appearance_thresh=0.25, workspace=None, streams=None):
    """BOTSORT.update with with_reid on (trackers/bot_sort.py:55-64, 166-190 with utils/matching.py:84-105) for the B frames of a
    batch, in order, in one launch: botsort_update's operands and outputs plus feat f32 [B, nq, D], one feature row per row of `out`
    (reid_rows), and state['feat'] f32 [T, D], the tracks' smooth features, updated in place; the rule is stated in csrc/track.hip.
    The workspace is botsort_reid_workspace_bytes(T, nq).  Every check comes before the launch; no synchronisation.  streams=S as in
    bytetrack_update, with state['feat'] [S, T, D] and the workspace botsort_reid_workspace_bytes(T, nq, S)."""
    what = 'botsort_reid_update'
    S = _check_streams(what, streams)
    if not torch.is_tensor(feat) or feat.dim() != 3 or feat.dtype != torch.float32 or out.dim() != 3 or tuple(feat.shape[:2]) != tuple(out.shape[:2]) \
            or feat.shape[2] < 1:
        got = (feat.dtype, tuple(feat.shape)) if torch.is_tensor(feat) else type(feat).__name__
        raise _lib.TamtrHipError(f'{what}: feat must be a float32 tensor [B, nq, D] aligned with out {tuple(out.shape)}, got {got}')
    D = int(feat.shape[2])
    if D > REID_MAX_D:
        raise _lib.TamtrHipError(f'{what}: D = {D} is above the {REID_MAX_D} the kernel is built for')
    _check_state(what, state, [('feat', torch.float32, (() if S is None else (S,)) + (int(capacity), D))])
    return _tracker_update(what, warps, out, counts, state, capacity, track_high_thresh, track_low_thresh, new_track_thresh,
                           match_thresh, max_time_lost, workspace, reid=(feat, state['feat'], D, float(proximity_thresh), float(appearance_thresh)),
                           streams=S)


# ------------------------------------------------------------------------------------------------ camera-motion estimate (csrc/gmc.hip)
GMC_SLOTS = 1024
GMC_SECTIONS = (('pyr', torch.uint8), ('lam', torch.float32), ('tilemax', torch.float32), ('kp', torch.int32), ('pts', torch.float32),
                ('status', torch.int32), ('fit', torch.int32), ('pair', torch.int32))


def _gmc_check_hw(H, W):
    if H < 64 or W < 64 or H % 8 or W % 8 or H > 8192 or W > 8192:
        raise _lib.TamtrHipError(f'gmc: frames must be at least 64 x 64 and at most 8192 x 8192 with H and W multiples of 8, got {H} x {W}')


def gmc_workspace_bytes(B, H, W):
    """Bytes of device workspace tamtr_gmc_estimate needs for B frames of H x W (no GPU call)."""
    _gmc_check_hw(int(H), int(W))
    n = _lib.lib().tamtr_gmc_workspace_bytes(int(B), int(H), int(W))
    if n <= 0:
        raise _lib.TamtrHipError(f'gmc: a batch of {B} frames of {H} x {W} is outside what the kernels are built for')
    return n


def gmc_levels(H, W):
    """The pyramid of an H x W frame as the kernels lay it out: [(h, w, byte offset)] per level."""
    _gmc_check_hw(int(H), int(W))
    m, L = min(H, W) // 32, 1
    while L < 4 and (m >> L):
        L += 1
    out, o = [], 0
    for l in range(L):
        out.append((H >> l, W >> l, o))
        o += (H >> l) * (W >> l)
    return out


def gmc_state(H, W, device, streams=None):
    """A fresh persistent state for frames of H x W: the pyramid and keypoint slots of the last tracked frame, hdr[0] = valid.
    streams=S: one state per stream, stacked (pyr [S, P], kp [S, 1024], hdr [S, 4])."""
    _gmc_check_hw(int(H), int(W))
    S = _check_streams('gmc_state', streams)
    lead = () if S is None else (S,)
    n = _lib.lib().tamtr_gmc_state_bytes(int(H), int(W))
    return {'pyr': torch.zeros(lead + (n,), device=device, dtype=torch.uint8),
            'kp': torch.full(lead + (GMC_SLOTS,), -1, device=device, dtype=torch.int32),
            'hdr': torch.zeros(lead + (4,), device=device, dtype=torch.int32)}


def gmc_workspace_views(workspace, B, H, W):
    """The sections of a gmc workspace as tensors sharing its memory (csrc/gmc.hip lists them): what each stage left, for tests."""
    off = [_lib.lib().tamtr_gmc_workspace_offset(int(B), int(H), int(W), i) for i in range(9)]
    P = _lib.lib().tamtr_gmc_state_bytes(int(H), int(W))
    nt = ((H + 63) // 64) * ((W + 63) // 64)
    shapes = {'pyr': (B, P), 'lam': (B, H, W), 'tilemax': (B, nt), 'kp': (B, GMC_SLOTS), 'pts': (B, GMC_SLOTS, 4), 'status': (B, GMC_SLOTS),
              'fit': (B, GMC_SLOTS + 8), 'pair': (B,)}
    out = {}
    for i, (k, dt) in enumerate(GMC_SECTIONS):
        n = math.prod(shapes[k]) * torch.empty(0, dtype=dt).element_size()
        out[k] = workspace[off[i]:off[i] + n].view(dt).view(shapes[k])
    return out


def gmc_estimate(frames, counts, scale, state, workspace=None, stages=15, streams=None):
    """One 2x3 camera-motion warp per frame from the frames of a batch, on the device; the rule is written out in csrc/gmc.hip (it is
    the project's own, standing where the reference runs OpenCV's sparse optical flow on the host, trackers/utils/gmc.py:247-302).
    frames u8 [B, H, W, 3] RGB on the GPU (the network input as uploaded), counts i32 [B] on the GPU, scale [B, 2] = (w0 / W, h0 / H)
    (any array-like; a host one goes up in one copy), state: gmc_state(H, W), updated in place.  Returns device tensors warps f64
    [B, 2, 3] in original pixels, ready for botsort_update, and stats i32 [B, 4] (keypoints, tracked, inliers, used).  `stages` is for
    tests (see the header).  At most four launches; every check comes before the first; no synchronisation.
    streams=S: the B = F * S frames are frame-major (frame f * S + s is the f-th of stream s), state is gmc_state(H, W, streams=S),
    and pairing and the state's update run per stream; stream s gets what streams=None computes on its own frames and state[k][s]."""
    S = _check_streams('gmc_estimate', streams)
    if not torch.is_tensor(frames) or frames.dim() != 4 or frames.shape[-1] != 3 or frames.shape[0] < 1:
        got = tuple(frames.shape) if torch.is_tensor(frames) else type(frames).__name__
        raise _lib.TamtrHipError(f'gmc_estimate: expected frames [B, H, W, 3], got {got}')
    if frames.dtype != torch.uint8:
        raise _lib.TamtrHipError(f'gmc_estimate: frames must be uint8 (the network input as uploaded), got {frames.dtype}')
    B, H, W, _ = frames.shape
    _gmc_check_hw(H, W)
    if S is not None and B % S:
        raise _lib.TamtrHipError(f'gmc_estimate: a batch of {B} frames is no multiple of streams = {S}')
    lead = () if S is None else (S,)
    _check_counts('gmc_estimate', counts, B)
    if not torch.is_tensor(scale):
        scale = torch.as_tensor(scale, dtype=torch.float64)
    if tuple(scale.shape) != (B, 2) or scale.dtype != torch.float64:
        raise _lib.TamtrHipError(f'gmc_estimate: scale must be float64 [B, 2] = [{B}, 2], got {scale.dtype} {tuple(scale.shape)}')
    need_st = _lib.lib().tamtr_gmc_state_bytes(H, W)
    _check_state('gmc_estimate', state, (('pyr', torch.uint8, lead + (need_st,)), ('kp', torch.int32, lead + (GMC_SLOTS,)), ('hdr', torch.int32, lead + (4,))),
                 f'gmc_state({H}, {W})' if S is None else f'gmc_state({H}, {W}, streams={S})')
    if int(stages) < 1 or int(stages) > 15:
        raise _lib.TamtrHipError(f'gmc_estimate: stages must be a mask in 1 .. 15, got {stages}')
    require_gpu(frames, counts, state['pyr'], state['kp'], state['hdr'])
    if not scale.is_cuda:
        scale = scale.to(frames.device, non_blocking=True)
    workspace = _workspace('gmc_estimate', workspace, gmc_workspace_bytes(B, H, W), frames.device)
    frames, counts, scale = _c(frames), _c(counts), _c(scale)
    warps = torch.empty(B, 2, 3, device=frames.device, dtype=torch.float64)
    stats = torch.empty(B, 4, device=frames.device, dtype=torch.int32)
    call('tamtr_gmc_estimate_streams', ptr(frames), ptr(counts), ptr(scale), B, S or 1, H, W, ptr(state['pyr']), ptr(state['kp']),
         ptr(state['hdr']), ptr(warps), ptr(stats), ptr(workspace), workspace.numel(), int(stages), stream_ptr())
    return warps, stats


def _tracker_update(what, warps, out, counts, state, capacity, track_high_thresh, track_low_thresh, new_track_thresh, match_thresh,
                    max_time_lost, workspace, reid=None, streams=None):
    """The one place the tracker kernel is launched from: tamtr_<what>_streams, of which the single-tracker entry is S = 1."""
    S = _check_streams(what, streams)
    if out.dim() != 3 or out.shape[-1] != 6 or out.shape[0] < 1 or out.shape[1] < 1:
        raise _lib.TamtrHipError(f'{what}: expected out [B, nq, 6], got {tuple(out.shape)}')
    B, nq, _ = out.shape
    if tuple(counts.shape) != (B,):
        raise _lib.TamtrHipError(f'{what}: counts must be [B] = [{B}], got {tuple(counts.shape)}')
    if S is not None and B % S:
        raise _lib.TamtrHipError(f'{what}: a batch of {B} images is no multiple of streams = {S} (frame-major: image f * S + s)')
    lead = () if S is None else (S,)
    if out.dtype != torch.float32 or counts.dtype != torch.int32:
        raise _lib.TamtrHipError(f'{what}: out must be float32 and counts int32, got {out.dtype} and {counts.dtype}')
    T = int(capacity)
    if T < 1:
        raise _lib.TamtrHipError(f'{what}: capacity must be positive, got {capacity}')
    _check_state(what, state, [(k, dt, lead + (T,) + tail) for k, dt, tail in TRACK_STATE_SPEC] + [('hdr', torch.int32, lead + (8,))],
                 f'capacity {T}' if S is None else f'capacity {T}, streams {S}')
    if warps is not None and (not torch.is_tensor(warps) or tuple(warps.shape) != (B, 2, 3) or warps.dtype != torch.float64):
        got = (warps.dtype, tuple(warps.shape)) if torch.is_tensor(warps) else type(warps).__name__
        raise _lib.TamtrHipError(f'{what}: warps must be a float64 tensor [B, 2, 3] = [{B}, 2, 3], got {got}')
    require_gpu(out, counts, warps, *(state[k] for k in ('mean', 'cov', 'meta', 'sc', 'hdr')), *(reid[:2] if reid else ()))
    warps = _c(warps) if warps is not None else None
    workspace = _workspace(what, workspace, botsort_reid_workspace_bytes(T, nq, S) if reid else bytetrack_workspace_bytes(T, nq, S), out.device)
    out, counts = _c(out), _c(counts)
    tracks = torch.empty(B, nq, 8, device=out.device, dtype=torch.float32)
    tcounts = torch.empty(B, device=out.device, dtype=torch.int32)
    if reid:
        feat, tf, D, prox, app = reid
        call(f'tamtr_{what}_streams', ptr(out), ptr(counts), ptr(warps) if warps is not None else None, ptr(_c(feat)), B, S or 1, nq, ptr(state['mean']),
             ptr(state['cov']), ptr(state['meta']), ptr(state['sc']), ptr(state['hdr']), ptr(tf), D, T, float(track_high_thresh),
             float(track_low_thresh), float(new_track_thresh), float(match_thresh), int(max_time_lost), prox, app, ptr(tracks), ptr(tcounts),
             ptr(workspace), int(workspace.numel()), stream_ptr())
        return tracks, tcounts
    args = (ptr(out), ptr(counts)) + ((ptr(warps) if warps is not None else None,) if what == 'botsort_update' else ())
    call(f'tamtr_{what}_streams', *args, B, S or 1, nq, ptr(state['mean']), ptr(state['cov']), ptr(state['meta']), ptr(state['sc']),
         ptr(state['hdr']), T, float(track_high_thresh), float(track_low_thresh), float(new_track_thresh), float(match_thresh),
         int(max_time_lost), ptr(tracks), ptr(tcounts), ptr(workspace), int(workspace.numel()), stream_ptr())
    return tracks, tcounts


# the MOT evaluator's state (csrc/mot.hip states the columns): name, dtype, shape from (nc, caps); caps = (gt identities, track ids);
# all zero when fresh
MOT_STATE_SPEC = (('gstate', torch.int32, lambda nc, c: (c[0], 8)), ('counts', torch.int32, lambda nc, c: (nc, 16)),
                  ('iou_sum', torch.float64, lambda nc, c: (nc,)), ('pair', torch.int32, lambda nc, c: (c[0], c[1])),
                  ('hdr', torch.int32, lambda nc, c: (8,)))
MOT_CAPS = ('gt', 'tracks')


def mot_workspace_bytes(nq, ng, nc, gt_capacity, track_capacity, streams=None):
    """Bytes of device workspace tamtr_mot_update and tamtr_mot_end_sequence need (no GPU call); streams=S: what
    tamtr_mot_update_streams and tamtr_mot_end_streams need for S stacked states (S slices, each rounded up to 16 bytes)."""
    S = _check_streams('mot', streams)
    sizes = (int(nq), int(ng), int(nc), int(gt_capacity), int(track_capacity))
    n = _lib.lib().tamtr_mot_workspace_bytes(*sizes) if S is None else _lib.lib().tamtr_mot_streams_workspace_bytes(S, *sizes)
    if n <= 0:
        raise _lib.TamtrHipError(f'mot: nq {nq}, ng {ng}, nc {nc} with capacities {gt_capacity} x {track_capacity}' +
                                 (f' and {S} streams' if S else '') + ' is outside what the kernel is built for')
    return n


def _mot_frames(what, tracks, tcounts, gt, gcounts, iou):
    """The checks every tracking evaluator's update makes on a batch's rows -> B, nq, ng and the four tensors, contiguous."""
    if tracks.dim() != 3 or tracks.shape[-1] != 8 or tracks.shape[0] < 1 or tracks.shape[1] < 1:
        raise _lib.TamtrHipError(f'{what}: expected tracks [B, nq, 8], got {tuple(tracks.shape)}')
    B, nq, _ = tracks.shape
    if gt.dim() != 3 or gt.shape[0] != B or gt.shape[1] < 1 or gt.shape[2] != 7:
        raise _lib.TamtrHipError(f'{what}: expected gt [B, ng, 7] with B = {B}, got {tuple(gt.shape)}')
    if tuple(tcounts.shape) != (B,) or tuple(gcounts.shape) != (B,):
        raise _lib.TamtrHipError(f'{what}: tcounts and gcounts must be [B] = [{B}], got {tuple(tcounts.shape)} and {tuple(gcounts.shape)}')
    if tracks.dtype != torch.float32 or gt.dtype != torch.float32 or tcounts.dtype != torch.int32 or gcounts.dtype != torch.int32:
        raise _lib.TamtrHipError(f'{what}: tracks and gt must be float32, tcounts and gcounts int32')
    if not float(iou) > 0:
        raise _lib.TamtrHipError(f'{what}: iou must be positive, got {iou}')
    return B, nq, gt.shape[1], _c(tracks), _c(tcounts), _c(gt), _c(gcounts)


def _eval_streams(what, B, streams, active):
    """The stream dimension of a stacked evaluator's update: S or None, and the active words (i32 [B] on the device, or None for
    "every image is a frame") as the kernel reads them."""
    S = _check_streams(what, streams)
    if S is not None and B % S:
        raise _lib.TamtrHipError(f'{what}: a batch of {B} images is no multiple of streams = {S} (frame-major: image f * S + s)')
    if active is None:
        return S, None
    if S is None:
        raise _lib.TamtrHipError(f'{what}: active belongs to a stacked evaluator (streams=S)')
    _check_counts(what, active, B, 'active')
    require_gpu(active)
    return S, _c(active)


def _eval_masks(what, S, **masks):
    """The per-stream words of a stacked evaluator's end of sequence (ending, gt_used): i32 [S] on the device, or None."""
    out = []
    for k, t in masks.items():
        if t is not None:
            if not torch.is_tensor(t) or tuple(t.shape) != (S,) or t.dtype != torch.int32:
                got = (t.dtype, tuple(t.shape)) if torch.is_tensor(t) else type(t).__name__
                raise _lib.TamtrHipError(f'{what}: {k} must be an int32 tensor [S] = [{S}], got {got}')
            require_gpu(t)
            t = _c(t)
        out.append(t)
    return out


def _eval_state(what, spec, cap_names, state, nc, caps, streams=None):
    """Check an evaluator's state against its spec (streams=S: every tensor with a leading S) -> (host array of its device pointers in
    the spec's order, host array of the capacities)."""
    lead = () if streams is None else (streams,)
    caps = tuple(int(c) for c in caps)
    if int(nc) < 1 or len(caps) != len(cap_names) or min(caps) < 1:
        raise _lib.TamtrHipError(f'{what}: nc and the {len(cap_names)} capacities ({", ".join(cap_names)}) must be positive, got {nc} and {caps}')
    _check_state(what, state, [(k, dt, lead + shape(int(nc), caps)) for k, dt, shape in spec], '' if streams is None else f'streams {streams}')
    require_gpu(*(state[k] for k, _, _ in spec))
    return (ctypes.c_void_p * len(spec))(*(state[k].data_ptr() for k, _, _ in spec)), (ctypes.c_int * len(caps))(*caps)


def mot_update(tracks, tcounts, gt, gcounts, state, nc, gt_capacity, track_capacity, iou=0.5, workspace=None, streams=None, active=None):
    """Steps 1 to 4 of the MOT evaluation rule (csrc/mot.hip; engine.mot_evaluate is its numpy statement) for the B frames of a batch,
    in order, in one launch.  tracks f32 [B, nq, 8] and tcounts i32 [B] are bytetrack_update's outputs on the GPU; gt f32 [B, ng, 7]
    (x1 y1 x2 y2 id cls kind, the id of a kind-0 row being its dense row in [0, gt_capacity)) and gcounts i32 [B] are on the GPU too.
    state: a dict of device tensors as MOT_STATE_SPEC lists them, updated in place.  Every check comes before the launch; no
    synchronisation.
    streams=S: one evaluator state per stream, still one launch (one workgroup per stream).  The B = F * S images are frame-major,
    image f * S + s is the f-th frame of stream s, as bytetrack_update(streams=S) leaves them; every state tensor has a leading S and
    the workspace is mot_workspace_bytes(..., streams=S).  active i32 [B] on the GPU (None: every image counts): an image whose word
    is 0 is no frame of its stream.  Stream s gets what streams=None computes on its own frames and state[k][s]."""
    B, nq, ng, tracks, tcounts, gt, gcounts = _mot_frames('mot_update', tracks, tcounts, gt, gcounts, iou)
    S, active = _eval_streams('mot_update', B, streams, active)
    nc, G, T = int(nc), int(gt_capacity), int(track_capacity)
    _eval_state('mot_update', MOT_STATE_SPEC, MOT_CAPS, state, nc, (G, T), S)
    require_gpu(tracks, tcounts, gt, gcounts)
    workspace = _workspace('mot_update', workspace, mot_workspace_bytes(nq, ng, nc, G, T, S), tracks.device, align=16)
    call('tamtr_mot_update_streams', ptr(tracks), ptr(tcounts), ptr(gt), ptr(gcounts), B, S or 1, nq, ng, nc, float(iou), ptr(active),
         ptr(state['gstate']), ptr(state['counts']), ptr(state['iou_sum']), ptr(state['pair']), ptr(state['hdr']), G, T, ptr(workspace),
         int(workspace.numel()), stream_ptr())


def mot_end_sequence(state, nc, gt_capacity, track_capacity, gt_used, workspace=None, streams=None, ending=None):
    """The per-sequence reduction of the MOT evaluation (MT / PT / ML / Frag and the identity assignment per class) in one launch; adds
    to state['counts'] and clears the per-sequence state.  gt_used: the number of dense gt rows the host handed out.  No synchronisation.
    streams=S: the same launch with the stream as a second grid dimension.  gt_used is then i32 [S] on the GPU, and ending i32 [S] on
    the GPU (None: every stream ends) names the streams to reduce: slice s of a stream whose word is 0 is left untouched."""
    S = _check_streams('mot_end_sequence', streams)
    nc, G, T = int(nc), int(gt_capacity), int(track_capacity)
    if S is None:
        if ending is not None:
            raise _lib.TamtrHipError('mot_end_sequence: ending belongs to a stacked evaluator (streams=S)')
        if int(gt_used) < 0:
            raise _lib.TamtrHipError(f'mot_end_sequence: gt_used must be >= 0, got {gt_used}')
    else:
        if gt_used is None:
            raise _lib.TamtrHipError(f'mot_end_sequence: gt_used must be an int32 tensor [S] = [{S}], got None')
        ending, gt_used = _eval_masks('mot_end_sequence', S, ending=ending, gt_used=gt_used)
    _eval_state('mot_end_sequence', MOT_STATE_SPEC, MOT_CAPS, state, nc, (G, T), S)
    workspace = _workspace('mot_end_sequence', workspace, mot_workspace_bytes(1, 1, nc, G, T, S), state['hdr'].device, align=16)
    if S is None:      # the host's scalar goes as it is: no upload
        call('tamtr_mot_end_sequence', nc, ptr(state['gstate']), ptr(state['counts']), ptr(state['pair']), ptr(state['hdr']), G, T,
             min(int(gt_used), G), ptr(workspace), int(workspace.numel()), stream_ptr())
    else:
        call('tamtr_mot_end_streams', nc, S, ptr(ending), ptr(gt_used), ptr(state['gstate']), ptr(state['counts']), ptr(state['pair']),
             ptr(state['hdr']), G, T, ptr(workspace), int(workspace.numel()), stream_ptr())


# the HOTA evaluator's state (csrc/hota.hip states it): name, dtype, shape from (nc, caps); caps = (gt identities, track ids, pair
# slots, log entries, frames of a sequence); all zero when fresh.  The order is the kernel's.
HOTA_STATE_SPEC = (('gstate', torch.int32, lambda nc, c: (c[0], 2)), ('tcount', torch.int32, lambda nc, c: (nc, c[1])),
                   ('pkey', torch.int64, lambda nc, c: (c[2],)), ('ppot', torch.float64, lambda nc, c: (c[2],)),
                   ('phist', torch.int32, lambda nc, c: (c[2], 20)), ('fidx', torch.int32, lambda nc, c: (c[4], 4)),
                   ('log', torch.int32, lambda nc, c: (c[3], 4)), ('dets', torch.int32, lambda nc, c: (nc, 2)),
                   ('tp_lvl', torch.int32, lambda nc, c: (nc, 20)), ('loc_lvl', torch.float64, lambda nc, c: (nc, 20)),
                   ('ass', torch.float64, lambda nc, c: (3, nc, 19)), ('hdr', torch.int32, lambda nc, c: (16,)))
HOTA_CAPS = ('gt', 'tracks', 'pairs', 'log', 'frames')
HOTA_END_WORKGROUPS = 64     # workgroups of the matching launch: each strides over the logged frames and owns a slice of the workspace
HOTA_EPS = 2.0 ** -52        # np.finfo(float).eps


def hota_end_workgroups(streams=None):
    """Workgroups per stream of the matching launch: HOTA_END_WORKGROUPS for one evaluator, min(64, 1024 / S), at least 1, for S."""
    return HOTA_END_WORKGROUPS if streams is None else max(1, min(HOTA_END_WORKGROUPS, 1024 // streams))


def hota_workspace_bytes(nq, ng, workgroups=None, streams=None):
    """Bytes of device workspace tamtr_hota_update and tamtr_hota_end_sequence need (no GPU call); streams=S: what
    tamtr_hota_update_streams and tamtr_hota_end_streams need for S stacked states (S slices, each rounded up to 16 bytes).
    workgroups: per stream, hota_end_workgroups(streams) by default."""
    S = _check_streams('hota', streams)
    workgroups = hota_end_workgroups(S) if workgroups is None else int(workgroups)
    L = _lib.lib()
    n = L.tamtr_hota_workspace_bytes(int(nq), int(ng), workgroups) if S is None else L.tamtr_hota_streams_workspace_bytes(S, int(nq), int(ng), workgroups)
    if n <= 0:
        raise _lib.TamtrHipError(f'hota: nq {nq}, ng {ng} with {workgroups} workgroups' + (f' and {S} streams' if S else '') +
                                 ' is outside what the kernel is built for')
    return n


def hota_update(tracks, tcounts, gt, gcounts, state, nc, caps, iou=0.5, workspace=None, streams=None, active=None):
    """Steps 1 and 2 of the MOT rule and pass 1 of HOTA (csrc/hota.hip; engine.hota_evaluate is its numpy statement) for the B frames of a
    batch, in order, in one launch.  tracks / tcounts / gt / gcounts as mot_update takes them.  state: a dict of device tensors as
    HOTA_STATE_SPEC lists them, updated in place; caps: (gt identities, track ids, pair slots, log entries, frames).  Every check
    comes before the launch; no synchronisation.  streams=S and active as in mot_update: every state tensor has a leading S, the
    workspace is hota_workspace_bytes(nq, ng, 1, streams=S), one workgroup per stream."""
    B, nq, ng, tracks, tcounts, gt, gcounts = _mot_frames('hota_update', tracks, tcounts, gt, gcounts, iou)
    S, active = _eval_streams('hota_update', B, streams, active)
    ptrs, ccaps = _eval_state('hota_update', HOTA_STATE_SPEC, HOTA_CAPS, state, nc, caps, S)
    require_gpu(tracks, tcounts, gt, gcounts)
    workspace = _workspace('hota_update', workspace, hota_workspace_bytes(nq, ng, 1, S), tracks.device, align=16)
    call('tamtr_hota_update_streams', ptr(tracks), ptr(tcounts), ptr(gt), ptr(gcounts), B, S or 1, nq, ng, int(nc), float(iou), HOTA_EPS,
         ptr(active), ptrs, ccaps, ptr(workspace), int(workspace.numel()), stream_ptr())


def hota_end_sequence(state, nc, caps, nq, ng, workspace=None, workgroups=None, streams=None, ending=None):
    """Pass 2 of HOTA and the per-sequence reduction in three launches (matching over `workgroups` workgroups, the reduction over the
    pair table, the clearing of the sequence's state); adds to the run totals of `state`.  nq / ng: the widest rows any update of the
    sequence was given.  No synchronisation.  streams=S: the same three launches with the stream as a second grid dimension,
    `workgroups` per stream (hota_end_workgroups(S) by default); ending i32 [S] on the GPU (None: every stream ends) names the streams
    to reduce, and slice s of a stream whose word is 0 is left untouched."""
    S = _check_streams('hota_end_sequence', streams)
    nq, ng, workgroups = int(nq), int(ng), hota_end_workgroups(S) if workgroups is None else int(workgroups)
    if nq < 1 or ng < 1 or workgroups < 1:
        raise _lib.TamtrHipError(f'hota_end_sequence: nq, ng and workgroups must be positive, got {nq}, {ng}, {workgroups}')
    if ending is not None and S is None:
        raise _lib.TamtrHipError('hota_end_sequence: ending belongs to a stacked evaluator (streams=S)')
    ending, = _eval_masks('hota_end_sequence', S, ending=ending)
    ptrs, ccaps = _eval_state('hota_end_sequence', HOTA_STATE_SPEC, HOTA_CAPS, state, nc, caps, S)
    workspace = _workspace('hota_end_sequence', workspace, hota_workspace_bytes(nq, ng, workgroups, S), state['hdr'].device, align=16)
    import numpy as np
    alpha = (ctypes.c_double * 19)(*np.arange(0.05, 0.99, 0.05))   # the thresholds as TrackEval makes them, never k / 20
    call('tamtr_hota_end_streams', alpha, HOTA_EPS, int(nc), S or 1, ptr(ending), nq, ng, workgroups, ptrs, ccaps, ptr(workspace),
         int(workspace.numel()), stream_ptr())


# the track-mAP evaluator's state (csrc/trackmap.hip states it): name, dtype, shape from (nc, caps); caps = (gt identities, track ids,
# pair slots, rows of the run's table); all zero when fresh.  The order is the kernel's.
TRACKMAP_STATE_SPEC = (('gstate', torch.int32, lambda nc, c: (c[0], 2)), ('garea', torch.float64, lambda nc, c: (c[0],)),
                       ('tframes', torch.int32, lambda nc, c: (nc, c[1])), ('tsum', torch.float64, lambda nc, c: (nc, c[1], 2)),
                       ('pkey', torch.int64, lambda nc, c: (c[2],)), ('pinter', torch.float64, lambda nc, c: (c[2],)),
                       ('rscore', torch.float64, lambda nc, c: (c[3],)), ('rmeta', torch.int32, lambda nc, c: (c[3], 2)),
                       ('gt_tracks', torch.int32, lambda nc, c: (nc,)), ('hdr', torch.int32, lambda nc, c: (16,)))
TRACKMAP_CAPS = ('gt', 'tracks', 'pairs', 'rows')


def trackmap_workspace_bytes(nq, ng, nc, caps):
    """Bytes of device workspace tamtr_trackmap_update and tamtr_trackmap_end_sequence need (no GPU call)."""
    caps = tuple(int(c) for c in caps)
    if len(caps) != 4:
        raise _lib.TamtrHipError(f'trackmap: 4 capacities (gt, tracks, pairs, rows) are needed, got {caps}')
    ok = all(0 < v < 2 ** 31 for v in (int(nq), int(ng), int(nc)) + caps)
    n = _lib.lib().tamtr_trackmap_workspace_bytes(int(nq), int(ng), int(nc), *caps[:3]) if ok else 0
    if n <= 0:
        raise _lib.TamtrHipError(f'trackmap: nq {nq}, ng {ng}, nc {nc} with capacities {caps} is outside what the kernel is built for')
    return n


def trackmap_update(tracks, tcounts, gt, gcounts, state, nc, caps, iou=0.5, workspace=None):
    """Steps 1 and 2 of the MOT rule and the sums of track-mAP (csrc/trackmap.hip; engine.track_map_evaluate is its numpy statement) for
    the B frames of a batch, in order, in one launch.  tracks / tcounts / gt / gcounts as mot_update takes them; a track's score is
    column 5 of its row.  state: a dict of device tensors as TRACKMAP_STATE_SPEC lists them, updated in place; caps: (gt identities,
    track ids, pair slots, run rows).  Every check comes before the launch; no synchronisation."""
    B, nq, ng, tracks, tcounts, gt, gcounts = _mot_frames('trackmap_update', tracks, tcounts, gt, gcounts, iou)
    ptrs, ccaps = _eval_state('trackmap_update', TRACKMAP_STATE_SPEC, TRACKMAP_CAPS, state, nc, caps)
    require_gpu(tracks, tcounts, gt, gcounts)
    workspace = _workspace('trackmap_update', workspace, trackmap_workspace_bytes(nq, ng, nc, caps), tracks.device, align=16)
    call('tamtr_trackmap_update', ptr(tracks), ptr(tcounts), ptr(gt), ptr(gcounts), B, nq, ng, int(nc), float(iou), ptrs, ccaps,
         ptr(workspace), int(workspace.numel()), stream_ptr())


def _trackmap_thresholds(what, thresholds):
    import numpy as np
    thr = np.asarray(thresholds, np.float64).reshape(-1)
    if not 1 <= len(thr) <= 10 or not np.all((thr > 0) & (thr <= 1)):
        raise _lib.TamtrHipError(f'{what}: 1 to 10 thresholds in (0, 1] are needed, got {thresholds}')
    return thr


def trackmap_end_sequence(state, nc, caps, thresholds, workspace=None):
    """The end of a sequence of track-mAP in six launches (csrc/trackmap.hip: mean scores, the tracks' order, the candidate lists, the
    greedy matching at every threshold, the append to the run's table, the clearing of the sequence's state).  thresholds: 1 to 10
    fp64 values, handed over as they are.  No synchronisation."""
    thr = _trackmap_thresholds('trackmap_end_sequence', thresholds)
    ptrs, ccaps = _eval_state('trackmap_end_sequence', TRACKMAP_STATE_SPEC, TRACKMAP_CAPS, state, nc, caps)
    workspace = _workspace('trackmap_end_sequence', workspace, trackmap_workspace_bytes(1, 1, nc, caps), state['hdr'].device, align=16)
    call('tamtr_trackmap_end_sequence', (ctypes.c_double * len(thr))(*thr), len(thr), HOTA_EPS, int(nc), ptrs, ccaps, ptr(workspace),
         int(workspace.numel()), stream_ptr())


@torch.no_grad()
def trackmap_accumulate(state, nc, caps, n_thresholds):
    """The run's accumulation of track-mAP: tamtr_val_coco_accumulate (csrc/cocoeval.hip; fp64, serial in grid order, no floating-point
    atomics) on the run's table with one range and one cut.  The rows in use (state['hdr'][0], read on the device) are ordered by
    class, then score descending, then table order with two stable torch.sort calls, as val_coco_accumulate orders its rows.
    -> ap, ar f64 [n_thresholds, nc] on the device, -1 for a class without ground truth.  Nothing synchronises."""
    nt = int(n_thresholds)
    if not 1 <= nt <= 10:
        raise _lib.TamtrHipError(f'trackmap_accumulate: n_thresholds must be 1 .. 10, got {n_thresholds}')
    _eval_state('trackmap_accumulate', TRACKMAP_STATE_SPEC, TRACKMAP_CAPS, state, nc, caps)
    nc, R = int(nc), int(caps[3])
    dev = state['hdr'].device
    valid = torch.arange(R, device=dev, dtype=torch.int32) < state['hdr'][0]
    key = torch.where(valid, state['rmeta'][:, 0], nc)
    _, by_score = torch.sort(-state['rscore'], stable=True)
    key, by_cls = torch.sort(key[by_score], stable=True)
    order = by_score[by_cls]
    bits = torch.zeros(R, 4, device=dev, dtype=torch.int32)
    bits[:, 0] = state['rmeta'][:, 1][order]
    rank = _c(torch.where(valid[order], 0, -1).to(torch.int32))
    seg = _c(torch.searchsorted(key, torch.arange(nc + 1, device=dev, dtype=key.dtype)).to(torch.int32))
    npig = torch.zeros(nc, 4, device=dev, dtype=torch.int32)
    npig[:, 0] = state['gt_tracks']
    cuts = torch.ones(1, device=dev, dtype=torch.int32)
    packed = torch.empty(103 * 40 * nc, device=dev, dtype=torch.float64)
    ap_tkam, recall, precision = val_coco_split(packed, nc, 1)
    call('tamtr_val_coco_accumulate', ptr(bits), ptr(rank), ptr(seg), R, nc, ptr(npig), ptr(cuts), 1,
         ctypes.c_void_p(_coco_grids(dev).data_ptr() + 80), ptr(precision), ptr(recall), ptr(ap_tkam), stream_ptr())
    return ap_tkam[:nt, :, 0, 0], recall[:nt, :, 0, 0]


@torch.no_grad()
def val_postprocess_match(y, cls, bboxes, batch_idx, ori_hw, imgsz, conf, iou, single_cls=False, max_wh=7680., return_device_labels=False):
    """engine.Validator.update's per-image work (RTDETRValidator.postprocess, models/rtdetrworld/val.py:102-173, and match_predictions,
    engine/validator.py:208-247) for the whole batch in one launch; the rule is stated in csrc/valmatch.hip and is "the host rule on
    y.float()".  y (f32 / bf16) [B, nq, 4 + nc] eval output on the GPU; cls [M] or [M, 1], bboxes [M, 4] (normalised xywh) and
    batch_idx [M] (integer-valued) are the batch's labels, on the host (as data.preprocess_batch leaves them) or on the device;
    ori_hw: B (h, w) pairs, or None for (imgsz, imgsz).
    Returns predn f32 [B, nq, 6] (native-space x1 y1 x2 y2, score, cls; zero after the count), correct u8 [B, nq, 10], counts i32 [B]
    on the device, and the labels grouped by image, where they came from: lab_cls f32 [M'] and lab_off i32 [B + 1] (numpy arrays for
    host labels, device tensors otherwise).  Host labels go up in ONE non-blocking copy; nothing synchronises.
    return_device_labels: a sixth element, the device-side operands of that upload (lab_cls f32 [M], lab_box f32 [M, 4],
    lab_off i32 [B + 1], scale f32 [B, 4]) - what val_confusion reads, so the two ops share one copy per batch."""
    import numpy as np
    require_gpu(y)
    if y.dim() != 3:
        raise _lib.TamtrHipError(f'val_postprocess_match: expected y [B, nq, 4 + nc], got {tuple(y.shape)}')
    B, nq, nd = y.shape
    dev = y.device
    y = _c(y if y.dtype in (torch.float32, torch.bfloat16) else y.float())
    hw = np.full((B, 2), imgsz, dtype=np.int64) if ori_hw is None else np.asarray(ori_hw).reshape(-1, 2)
    if hw.shape[0] != B:
        raise _lib.TamtrHipError(f'val_postprocess_match: ori_hw must hold {B} (h, w) pairs, got {hw.shape[0]}')
    # the four fp32 factors per image, rounded as the host rule rounds them (Python double division, then fp32)
    scale = np.array([[float(w) / imgsz, float(h) / imgsz, float(w), float(h)] for h, w in hw.tolist()], dtype=np.float64).astype(np.float32)
    M = int(batch_idx.numel())
    if cls.numel() != M or bboxes.numel() != 4 * M:
        raise _lib.TamtrHipError(f'val_postprocess_match: {M} batch indices, {cls.numel()} classes, {tuple(bboxes.shape)} boxes')
    if not (cls.is_cuda or bboxes.is_cuda or batch_idx.is_cuda):
        bi = batch_idx.reshape(-1).numpy().astype(np.float32)
        order = np.argsort(bi, kind='stable')          # the host rule's mask keeps file order inside an image
        off = np.searchsorted(bi[order], np.arange(B + 1, dtype=np.float32)).astype(np.int32)
        order = order[off[0]:off[B]]                   # (indices outside 0 .. B - 1 belong to no image)
        lab_cls = cls.reshape(-1).float().numpy()[order]
        lab_box = bboxes.reshape(-1, 4).float().numpy()[order]
        off = off - off[0]
        M = len(order)
        buf = np.concatenate([off.view(np.float32), scale.reshape(-1), lab_cls, lab_box.reshape(-1)])
        up = torch.from_numpy(buf).to(dev, non_blocking=True)
        d_off, d_scale, d_cls, d_box = up.split([B + 1, 4 * B, M, 4 * M])
        d_off = d_off.view(torch.int32)
        ret_cls, ret_off = lab_cls, off
    else:
        bi = batch_idx.reshape(-1).to(dev).float()
        sbi, order = torch.sort(bi, stable=True)
        d_off = torch.searchsorted(sbi, torch.arange(B + 1, device=dev, dtype=torch.float32)).to(torch.int32)
        d_cls = _c(cls.reshape(-1).to(dev).float()[order])
        d_box = _c(bboxes.reshape(-1, 4).to(dev).float()[order])
        d_scale = torch.from_numpy(scale).to(dev, non_blocking=True)
        ret_cls, ret_off = d_cls, d_off               # (rows outside lab_off[0] .. lab_off[B] belong to no image)
    predn = torch.empty(B, nq, 6, device=dev, dtype=torch.float32)
    correct = torch.empty(B, nq, 10, device=dev, dtype=torch.uint8)
    counts = torch.empty(B, device=dev, dtype=torch.int32)
    call('tamtr_val_postprocess_match', ptr(y), dtype_code(y), B, nq, nd, float(imgsz), float(conf), _f32_at_most(float(iou)),
         int(bool(single_cls)), float(max_wh), ptr(d_cls) if M else None, ptr(d_box) if M else None, ptr(d_off), M, ptr(d_scale),
         ptr(predn), ptr(correct), ptr(counts), stream_ptr())
    if return_device_labels:
        return predn, correct, counts, ret_cls, ret_off, (d_cls, d_box, d_off, d_scale)
    return predn, correct, counts, ret_cls, ret_off


@torch.no_grad()
def val_confusion(predn, counts, device_labels, nc, conf, iou_thres, matrix):
    """engine.ConfusionMatrix.process_batch (the reference's ConfusionMatrix.process_batch, utils/metrics.py:833-877, as the validator
    calls it per image) for the whole batch in one launch; the rule is stated in csrc/confusion.hip.  predn f32 [B, nq, 6] and counts
    i32 [B]: the outputs of val_postprocess_match; device_labels: the sixth element it returns with return_device_labels=True.
    matrix i32 [nc + 1, nc + 1] on the device is ADDED TO in place (row = predicted, column = true, nc = background) and returned.
    conf and iou_thres are rounded to the nearest fp32, the value torch compares an fp32 tensor with when the other side is a Python
    scalar.  Nothing is uploaded, allocated or synchronised."""
    require_gpu(predn, counts, matrix, *device_labels)
    d_cls, d_box, d_off, d_scale = device_labels
    nc = int(nc)
    if predn.dim() != 3 or predn.shape[2] != 6 or predn.dtype != torch.float32 or counts.dtype != torch.int32 or counts.numel() != predn.shape[0]:
        raise _lib.TamtrHipError(f'val_confusion: expected predn f32 [B, nq, 6] and counts i32 [B], got {tuple(predn.shape)} {predn.dtype}, '
                                 f'{tuple(counts.shape)} {counts.dtype}')
    B, nq, _ = predn.shape
    M = int(d_cls.numel())
    if (matrix.dtype != torch.int32 or matrix.numel() != (nc + 1) ** 2 or not matrix.is_contiguous() or d_off.dtype != torch.int32
            or d_off.numel() != B + 1 or d_scale.numel() != 4 * B or d_box.numel() != 4 * M
            or any(t.dtype != torch.float32 for t in (d_cls, d_box, d_scale))):
        raise _lib.TamtrHipError(f'val_confusion: matrix must be contiguous i32 [{nc + 1}, {nc + 1}] and the labels those of val_postprocess_match')
    predn, counts, d_cls, d_box, d_off, d_scale = _c(predn), _c(counts), _c(d_cls), _c(d_box), _c(d_off), _c(d_scale)
    call('tamtr_val_confusion', ptr(predn), ptr(counts), B, nq, nc, ptr(d_cls) if M else None, ptr(d_box) if M else None, ptr(d_off), M,
         ptr(d_scale), _f32_nearest(conf), _f32_nearest(iou_thres), ptr(matrix), stream_ptr())
    return matrix


VAL_AP_TILE = 256      # rows per tile of the scans of csrc/metrics.hip (= tamtr_val_ap_tile(); a host test holds the two together)
_VAL_AP_GRIDS = {}     # device -> f64 [1000 + 101]: numpy's own linspace(0, 1, 1000) and linspace(0, 1, 101), uploaded once


def val_ap_split(packed, nc):
    """The packed f64 buffer of val_ap_curves (a device tensor, or its copy as a numpy array) -> ap [nc, 10], p_curve, r_curve,
    pr_curve [nc, 1000] (f64), n_gt, n_pred [nc] (i32), all views."""
    import numpy as np
    i32 = torch.int32 if isinstance(packed, torch.Tensor) else np.int32
    cut = [0, 10 * nc, 1010 * nc, 2010 * nc, 3010 * nc]
    ap, p, r, pr = (packed[a:b].reshape(nc, -1) for a, b in zip(cut[:-1], cut[1:]))
    counts = packed[3010 * nc:3011 * nc].view(i32)
    return ap, p, r, pr, counts[:nc], counts[nc:]


@torch.no_grad()
def val_ap_curves(batches, lab_cls, nc, return_packed=False):
    """The reduction of a validation run, engine.ap_per_class(stable=True, curves=True), on the device: AP per class and IoU threshold and
    the precision / recall / PR curves of every class in [0, nc) from the rows val_postprocess_match left there; the rule is stated in
    csrc/metrics.hip.  batches: a list of (predn f32 [B, nq, 6], correct u8 [B, nq, 10], counts i32 [B]) device tensors, in run order.
    lab_cls: the run's label classes - a numpy array or device tensor, or a list of them (host arrays go up in ONE non-blocking copy).
    The rows are concatenated, dead rows (row >= counts[b]) get the class key nc, two stable torch.sort calls order them by class, then
    score descending, then original order, torch.searchsorted finds the class segments, and one launch does the rest.
    Returns ap f64 [nc, 10], p_curve, r_curve, pr_curve f64 [nc, 1000], n_gt, n_pred i32 [nc]: views of one packed device buffer
    (return_packed: a seventh element, that buffer, f64 [3011 * nc]; val_ap_split undoes it).  Nothing synchronises."""
    import numpy as np
    nc = int(nc)
    if not batches or nc < 1:
        raise _lib.TamtrHipError('val_ap_curves: needs at least one batch and nc >= 1')
    for predn, correct, counts in batches:
        require_gpu(predn, correct, counts)
        if (predn.dim() != 3 or predn.shape[2] != 6 or predn.dtype != torch.float32 or correct.dtype != torch.uint8
                or tuple(correct.shape) != (*predn.shape[:2], 10) or counts.dtype != torch.int32 or counts.numel() != predn.shape[0]):
            raise _lib.TamtrHipError(f'val_ap_curves: expected predn f32 [B, nq, 6], correct u8 [B, nq, 10], counts i32 [B], got '
                                     f'{tuple(predn.shape)} {predn.dtype}, {tuple(correct.shape)} {correct.dtype}, {tuple(counts.shape)} {counts.dtype}')
    dev = batches[0][0].device
    labs = list(lab_cls) if isinstance(lab_cls, (list, tuple)) else [lab_cls]
    on_dev = [t.reshape(-1).float() for t in labs if isinstance(t, torch.Tensor)]
    require_gpu(*on_dev)
    host = [np.asarray(a, dtype=np.float32).reshape(-1) for a in labs if not isinstance(a, torch.Tensor)]
    if sum(len(a) for a in host):
        on_dev.append(torch.from_numpy(np.concatenate(host)).to(dev, non_blocking=True))
    lab = _c(torch.cat(on_dev)) if on_dev else None
    M = int(lab.numel()) if lab is not None else 0
    grids = _VAL_AP_GRIDS.get(dev)
    if grids is None:
        grids = _VAL_AP_GRIDS[dev] = torch.from_numpy(np.concatenate([np.linspace(0, 1, 1000), np.linspace(0, 1, 101)])).to(dev, non_blocking=True)

    conf = torch.cat([b[0][..., 4].reshape(-1) for b in batches])
    cls = torch.cat([b[0][..., 5].reshape(-1) for b in batches])
    hits = torch.cat([b[1].reshape(-1, 10) for b in batches])
    if len({b[0].shape[1] for b in batches}) == 1:            # the usual run, one nq: one comparison for all batches
        live = (torch.arange(batches[0][0].shape[1], device=dev)[None, :] < torch.cat([b[2] for b in batches])[:, None]).reshape(-1)
    else:
        live = torch.cat([(torch.arange(b[0].shape[1], device=dev)[None, :] < b[2][:, None]).reshape(-1) for b in batches])
    key = torch.where(live, cls, float(nc))
    _, by_conf = torch.sort(-conf, stable=True)              # the host rule's np.argsort(-conf, kind='stable') ...
    key, by_cls = torch.sort(key[by_conf], stable=True)      # ... and its per-class masks, which keep that order
    order = by_conf[by_cls]
    conf, hits = _c(conf[order]), _c(hits[order])
    seg = _c(torch.searchsorted(key, torch.arange(nc + 1, device=dev, dtype=torch.float32)).to(torch.int32))
    N = int(conf.numel())
    tpc = torch.empty(10 * N, device=dev, dtype=torch.int32)
    env = torch.empty(10 * N, device=dev, dtype=torch.float64)
    packed = torch.empty(3011 * nc, device=dev, dtype=torch.float64)
    ap, p, r, pr, n_gt, n_pred = val_ap_split(packed, nc)
    call('tamtr_val_ap_curves', ptr(conf), ptr(hits), ptr(seg), N, nc, ptr(lab) if M else None, M, ptr(grids), ctypes.c_void_p(grids.data_ptr() + 8000),
         ptr(tpc), ptr(env), ptr(ap), ptr(p), ptr(r), ptr(pr), ptr(n_gt), ptr(n_pred), stream_ptr())
    return (ap, p, r, pr, n_gt, n_pred) + ((packed,) if return_packed else ())


_VAL_COCO_GRIDS = {}   # device -> f64 [10 + 101 + 1]: numpy's own linspace(0.5, 0.95, 10) and linspace(0, 1, 101) (+ padding), uploaded once


def _coco_grids(dev):
    import numpy as np
    g = _VAL_COCO_GRIDS.get(dev)
    if g is None:
        g = _VAL_COCO_GRIDS[dev] = torch.from_numpy(np.concatenate([np.linspace(0.5, 0.95, 10), np.linspace(0, 1, 101), [0.0]])).to(dev, non_blocking=True)
    return g


def _coco_max_dets(max_dets):
    md = tuple(int(m) for m in max_dets)
    if not 1 <= len(md) <= 4 or md[0] < 1 or any(b <= a for a, b in zip(md, md[1:])):
        raise _lib.TamtrHipError(f'val_coco: max_dets must be 1 to 4 ascending positive integers, got {tuple(max_dets)}')
    return md


def val_coco_workspace_bytes(B, nq, M):
    """Bytes of device workspace tamtr_val_coco_match needs for a batch of B images, nq rows and M labels (no GPU call)."""
    n = _lib.lib().tamtr_val_coco_workspace_bytes(int(B), int(nq), int(M))
    if n <= 0:
        raise _lib.TamtrHipError(f'val_coco_match: B {B}, nq {nq}, M {M} is outside what the kernel is built for (nq <= 512)')
    return n


@torch.no_grad()
def val_coco_match(predn, counts, device_labels, nc, max_det, npig, workspace=None):
    """The per-image matching of the COCO bbox protocol (pycocotools' COCOeval.evaluateImg, which the reference reaches through
    valTAMTR.py:15 save_json + dataset/yolo2coco.py) for the whole batch in one launch; the rule is stated in csrc/cocoeval.hip and by
    engine.coco_evaluate.  predn f32 [B, nq, 6] and counts i32 [B]: the outputs of val_postprocess_match; device_labels: the sixth element
    it returns with return_device_labels=True; max_det: the last entry of max_dets.  npig i32 [nc, 4] on the device is ADDED TO in place
    (non-ignored ground truths per class and size range).  Returns bits i32 [B, nq, 4] (per range all / small / medium / large: bit t =
    matched at threshold t, bit 16 + t = ignored) and rank i32 [B, nq] (rank among the image's rows of the class; -1: the row takes part
    in nothing).  workspace: a uint8 device tensor of val_coco_workspace_bytes(B, nq, M), made here when None.  Every check comes before
    the launch; nothing is uploaded or synchronised (the two threshold grids go up once per device)."""
    require_gpu(predn, counts, npig, *device_labels)
    d_cls, d_box, d_off, d_scale = device_labels
    nc, max_det = int(nc), int(max_det)
    if predn.dim() != 3 or predn.shape[2] != 6 or predn.dtype != torch.float32 or counts.dtype != torch.int32 or counts.numel() != predn.shape[0]:
        raise _lib.TamtrHipError(f'val_coco_match: expected predn f32 [B, nq, 6] and counts i32 [B], got {tuple(predn.shape)} {predn.dtype}, '
                                 f'{tuple(counts.shape)} {counts.dtype}')
    B, nq, _ = predn.shape
    M = int(d_cls.numel())
    if nc < 1 or max_det < 1:
        raise _lib.TamtrHipError(f'val_coco_match: nc and max_det must be positive, got {nc} and {max_det}')
    if (npig.dtype != torch.int32 or npig.numel() != 4 * nc or not npig.is_contiguous() or d_off.dtype != torch.int32
            or d_off.numel() != B + 1 or d_scale.numel() != 4 * B or d_box.numel() != 4 * M
            or any(t.dtype != torch.float32 for t in (d_cls, d_box, d_scale))):
        raise _lib.TamtrHipError(f'val_coco_match: npig must be contiguous i32 [{nc}, 4] and the labels those of val_postprocess_match')
    workspace = _workspace('val_coco_match', workspace, val_coco_workspace_bytes(B, nq, M), predn.device)
    predn, counts, d_cls, d_box, d_off, d_scale = _c(predn), _c(counts), _c(d_cls), _c(d_box), _c(d_off), _c(d_scale)
    bits = torch.empty(B, nq, 4, device=predn.device, dtype=torch.int32)
    rank = torch.empty(B, nq, device=predn.device, dtype=torch.int32)
    call('tamtr_val_coco_match', ptr(predn), ptr(counts), B, nq, nc, ptr(d_cls) if M else None, ptr(d_box) if M else None, ptr(d_off), M,
         ptr(d_scale), ptr(_coco_grids(predn.device)), max_det, ptr(bits), ptr(rank), ptr(npig), ptr(workspace), int(workspace.numel()),
         stream_ptr())
    return bits, rank


def val_coco_split(packed, nc, n_max_dets):
    """The packed f64 buffer of val_coco_accumulate (a device tensor, or its copy as a numpy array) -> ap_tkam, recall [10, nc, 4, M] and
    precision [10, 101, nc, 4, M], all views.  The buffer's head - ap_tkam and recall, 2 * 40 * nc * M values - is what a run copies to
    the host; given only that head, precision is None."""
    n = 40 * nc * n_max_dets
    ap_tkam, recall = (packed[i * n:(i + 1) * n].reshape(10, nc, 4, n_max_dets) for i in range(2))
    precision = packed[2 * n:103 * n].reshape(10, 101, nc, 4, n_max_dets) if packed.shape[0] >= 103 * n else None
    return ap_tkam, recall, precision


@torch.no_grad()
def val_coco_accumulate(batches, npig, nc, max_dets, return_packed=False):
    """The accumulation of the COCO bbox protocol (pycocotools' COCOeval.accumulate) for a whole run in one launch; the rule is stated in
    csrc/cocoeval.hip and by engine.coco_accumulate.  batches: a list of (predn f32 [B, nq, 6], bits i32 [B, nq, 4], rank i32 [B, nq])
    device tensors in run order (predn from val_postprocess_match, bits and rank from val_coco_match); npig i32 [nc, 4]: the table
    val_coco_match added to; max_dets: 1 to 4 ascending cuts, the last one the max_det the matching ran with.
    The rows are concatenated, rows that take part in nothing (rank < 0) or lie beyond the last cut get the class key nc, two stable
    torch.sort calls order them by class, then score descending, then original order, torch.searchsorted finds the class segments, and
    one launch does the rest.  Returns ap_tkam, recall f64 [10, nc, 4, M] and precision f64 [10, 101, nc, 4, M]: views of one packed
    device buffer (return_packed: a fourth element, that buffer; val_coco_split undoes it).  Nothing synchronises."""
    nc, md = int(nc), _coco_max_dets(max_dets)
    if not batches or nc < 1:
        raise _lib.TamtrHipError('val_coco_accumulate: needs at least one batch and nc >= 1')
    require_gpu(npig)
    for predn, bits, rank in batches:
        require_gpu(predn, bits, rank)
        if (predn.dim() != 3 or predn.shape[2] != 6 or predn.dtype != torch.float32 or bits.dtype != torch.int32 or rank.dtype != torch.int32
                or tuple(bits.shape) != (*predn.shape[:2], 4) or tuple(rank.shape) != tuple(predn.shape[:2])):
            raise _lib.TamtrHipError(f'val_coco_accumulate: expected predn f32 [B, nq, 6], bits i32 [B, nq, 4], rank i32 [B, nq], got '
                                     f'{tuple(predn.shape)} {predn.dtype}, {tuple(bits.shape)} {bits.dtype}, {tuple(rank.shape)} {rank.dtype}')
    if npig.dtype != torch.int32 or npig.numel() != 4 * nc or not npig.is_contiguous():
        raise _lib.TamtrHipError(f'val_coco_accumulate: npig must be contiguous i32 [{nc}, 4]')
    dev = batches[0][0].device
    grids = _coco_grids(dev)
    conf = torch.cat([b[0][..., 4].reshape(-1) for b in batches])
    cls = torch.cat([b[0][..., 5].reshape(-1) for b in batches])
    bits = torch.cat([b[1].reshape(-1, 4) for b in batches])
    rank = torch.cat([b[2].reshape(-1) for b in batches])
    key = torch.where((rank >= 0) & (rank < md[-1]), torch.trunc(cls), float(nc))
    _, by_conf = torch.sort(-conf, stable=True)              # the host rule's np.argsort(-score, kind='stable') ...
    key, by_cls = torch.sort(key[by_conf], stable=True)      # ... and its per-class selection, which keeps that order
    order = by_conf[by_cls]
    bits, rank = _c(bits[order]), _c(rank[order])
    seg = _c(torch.searchsorted(key, torch.arange(nc + 1, device=dev, dtype=torch.float32)).to(torch.int32))
    cuts = torch.tensor(md, dtype=torch.int32).to(dev, non_blocking=True)
    N = int(rank.numel())
    packed = torch.empty(103 * 40 * nc * len(md), device=dev, dtype=torch.float64)
    ap_tkam, recall, precision = val_coco_split(packed, nc, len(md))
    call('tamtr_val_coco_accumulate', ptr(bits), ptr(rank), ptr(seg), N, nc, ptr(npig), ptr(cuts), len(md),
         ctypes.c_void_p(grids.data_ptr() + 80), ptr(precision), ptr(recall), ptr(ap_tkam), stream_ptr())
    return (ap_tkam, recall, precision) + ((packed,) if return_packed else ())


def img_augment(src, inv_affine, luts, flags, out_hw, border=114):
    """The pixel half of the training transforms for a whole batch (affine warp -> HSV look-up -> flips -> CHW float / 255;
    ultralytics/data/augment.py:415-420,590-609,636-666,920-926).  src u8 [B, SH, SW, 3], inv_affine f64 [B, 6]
    (destination -> source), luts u8 [B, 3, 256], flags i32 [B] (bit 0 up-down, bit 1 left-right) -> f32 [B, 3, H, W].
    Bit-identical to the host kernels of libtamtr_host.so followed by `img.float() / 255` on the device."""
    require_gpu(src, inv_affine, luts, flags)
    B, SH, SW, ch = src.shape
    H, W = out_hw
    if (ch != 3 or src.dtype != torch.uint8 or inv_affine.dtype != torch.float64 or luts.dtype != torch.uint8 or flags.dtype != torch.int32
            or tuple(inv_affine.shape) != (B, 6) or tuple(luts.shape) != (B, 3, 256) or tuple(flags.shape) != (B,)):
        raise _lib.TamtrHipError('img_augment: expected src u8 [B,SH,SW,3], inv_affine f64 [B,6], luts u8 [B,3,256], flags i32 [B]')
    src, inv_affine, luts, flags = _c(src), _c(inv_affine), _c(luts), _c(flags)
    out = torch.empty(B, 3, H, W, device=src.device, dtype=torch.float32)
    call('tamtr_img_augment_u8', ptr(src), ptr(inv_affine), ptr(luts), ptr(flags), ptr(out), B, SH, SW, H, W, int(border), stream_ptr())
    return out


class _CPAM(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        require_gpu(x)
        x = _c(x)
        B, C, H, W = x.shape
        Hp, Wp = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        p = torch.empty(B, C, Hp, Wp, dtype=x.dtype, device=x.device)   # ChannelAttentionModule.Maxpool 3/2/1 (block.py:274): csrc/pool.hip
        idx = torch.empty(B, C, Hp, Wp, dtype=torch.uint8, device=x.device)
        call('tamtr_maxpool_fwd', ptr(x), ptr(p), ptr(idx), B, C, H, W, 3, 2, 1, 0, dtype_code(x), stream_ptr())
        out = torch.empty_like(x)
        s2 = torch.empty(B, 8, H, W, device=x.device, dtype=torch.float32)
        arg = torch.empty(B, 8, H, W, device=x.device, dtype=torch.int32)
        call('tamtr_cpam_fwd', ptr(x), ptr(p), ptr(out), ptr(s2), ptr(arg), B, C, H, W, dtype_code(x), stream_ptr())
        ctx.save_for_backward(x, p, idx, s2, arg)
        return out

    @staticmethod
    def backward(ctx, gout):
        x, p, idx, s2, arg = ctx.saved_tensors
        B, C, H, W = x.shape
        gout = _c(gout.to(x.dtype))
        dxd, du, dp = torch.empty_like(x), torch.empty_like(x), torch.empty_like(p)
        call('tamtr_cpam_bwd', ptr(gout), ptr(x), ptr(p), ptr(s2), ptr(arg), ptr(dxd), ptr(du), ptr(dp), B, C, H, W, dtype_code(x),
             stream_ptr())
        dx = torch.empty_like(x)
        call('tamtr_maxpool_bwd', ptr(dp), ptr(idx), ptr(dxd), ptr(dx), B, C, H, W, 3, 2, 1, 0, dtype_code(x), stream_ptr())  # + the direct term
        return dx


class _CPAMCL(torch.autograd.Function):
    """CPAM on a channels-last map where it lies (csrc/cpam.hip tamtr_cpam_cl_*, csrc/pool.hip with nhwc = 1): no transposing copies."""

    @staticmethod
    def forward(ctx, x):
        require_gpu(x)
        B, C, H, W = x.shape
        Hp, Wp = H // 2, W // 2
        cl = torch.channels_last
        p = torch.empty((B, C, Hp, Wp), dtype=x.dtype, device=x.device, memory_format=cl)
        idx = torch.empty((B, C, Hp, Wp), dtype=torch.uint8, device=x.device, memory_format=cl)
        out = torch.empty_like(x, memory_format=cl)
        s2 = torch.empty(B, H, W, 8, device=x.device, dtype=torch.float32)
        arg = torch.empty(B, H, W, 8, device=x.device, dtype=torch.int32)
        call('tamtr_cpam_cl_fwd', ptr(x), ptr(p), ptr(idx), ptr(out), ptr(s2), ptr(arg), B, C, H, W, dtype_code(x), stream_ptr())   # pool + gates
        ctx.save_for_backward(x, p, idx, s2, arg)
        return out

    @staticmethod
    def backward(ctx, gout):
        x, p, idx, s2, arg = ctx.saved_tensors
        B, C, H, W = x.shape
        gout = gout.to(x.dtype)
        if not _is_cl(gout):
            gout = gout.contiguous(memory_format=torch.channels_last)
        cl = torch.channels_last
        dxd, du, dp = torch.empty_like(x, memory_format=cl), torch.empty_like(x, memory_format=cl), torch.empty_like(p, memory_format=cl)
        dx = torch.empty_like(x, memory_format=cl)
        call('tamtr_cpam_cl_bwd', ptr(gout), ptr(x), ptr(p), ptr(idx), ptr(s2), ptr(arg), ptr(dxd), ptr(du), ptr(dp), ptr(dx), B, C, H, W, dtype_code(x),
             stream_ptr())
        return dx


def cpam_cl_ok(x):
    """What tamtr_cpam_cl_* take: a packed channels-last map, even H and W, a chunk (C / 8 channels) = a power-of-two number of 16-byte vectors."""
    if not (x.is_cuda and x.dim() == 4 and x.dtype in (torch.float32, torch.bfloat16) and _is_cl(x) and x.data_ptr() % 16 == 0):
        return False
    B, C, H, W = x.shape
    V = 8 if x.dtype == torch.bfloat16 else 4
    lpc = C // (8 * V)
    return (H % 2 == 0 and W % 2 == 0 and C % (8 * V) == 0 and lpc >= 1 and lpc & (lpc - 1) == 0 and lpc <= 64 and C // V <= 256 and 256 % (C // V) == 0
            and _os.environ.get('TAMTR_CPAM') != 'nchw')


def cpam(x):
    """CPAM (extra_modules/block.py:271-308): x [B,C,H,W] fp32/bf16 -> channel gate sigmoid(up2(maxpool3s2(x))) * x followed by
    the per-chunk (8 chunks) spatial gate sigmoid(max over the chunk's channels).  One fused kernel after the pool.
    Channels-last maps (the trunk's layout) take the channels-last kernels; the NCHW kernels remain for NCHW maps (deterministic mode)
    and for channel counts the lane mapping does not cover (there a channels-last map is repacked on the way in and out)."""
    if cpam_cl_ok(x):
        return _CPAMCL.apply(x)
    if _is_cl(x):
        return to_channels_last(_CPAM.apply(to_nchw(x)))
    return _CPAM.apply(x)


class _LayerNorm(torch.autograd.Function):
    """LayerNorm over the last axis in the activation's own dtype (VSSBlock.norm / norm2) - csrc/ss2d_out.hip."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps):
        require_gpu(x, gamma, beta)
        x = _c(x)
        D = x.shape[-1]
        ntok = x.numel() // D
        g32, b32 = _c(gamma.float()), _c(beta.float())
        out = torch.empty_like(x)
        stats = torch.empty(ntok, 2, device=x.device, dtype=torch.float32)
        call('tamtr_layernorm_fwd', ptr(x), ptr(g32), ptr(b32), ptr(out), ptr(stats), ntok, D, float(eps), dtype_code(x), stream_ptr())
        ctx.save_for_backward(x, g32, stats)
        ctx.cfg = (gamma.dtype, beta.dtype)
        return out

    @staticmethod
    def backward(ctx, gout):
        x, g32, stats = ctx.saved_tensors
        D = x.shape[-1]
        ntok = x.numel() // D
        gout = _c(gout.to(x.dtype))
        gx = torch.empty_like(x)
        part = torch.empty(_lib.lib().tamtr_ln_gate_blocks(ntok), 2, D, device=x.device, dtype=torch.float32)
        call('tamtr_layernorm_bwd', ptr(gout), ptr(x), ptr(g32), ptr(stats), ptr(gx), ptr(part), ntok, D, dtype_code(x), stream_ptr())
        gsum = slab_sum(part)
        return gx, gsum[0].to(ctx.cfg[0]), gsum[1].to(ctx.cfg[1]), None


def layer_norm(x, gamma, beta, eps=1e-5):
    return _LayerNorm.apply(x, gamma, beta, eps)


def layer_norm_module(norm, x):
    """norm(x) for an nn.LayerNorm over the last axis: on the GPU the wave-per-token kernel (one launch forward; one + an ordered partial sum
    backward, where torch launches three), in x's dtype - what torch's autocast gives for fp32 inputs; else the module."""
    D = x.shape[-1]
    if (x.is_cuda and x.dtype in (torch.float32, torch.bfloat16) and len(norm.normalized_shape) == 1 and norm.elementwise_affine and norm.bias is not None
            and D in (32, 64, 128, 256, 512, 1024) and _os.environ.get('TAMTR_DECODER_LN') != 'torch'):
        return _LayerNorm.apply(x, norm.weight, norm.bias, norm.eps)
    return norm(x)


# ------------------------------------------------------------------------------------------------ BatchNorm (csrc/bn.hip)
# Every entry point is called from one place, which sizes its `partials` workspace (the PART_* layouts of csrc/bn.hip: floats per chunk, then
# a per-channel tail).  The channels-last pair serves two autograd nodes and is a pair of launchers (_bncl_fwd, _bncl_bwd: allocate the outputs
# and the workspace, launch, return the tensors); the NCHW and the two-BatchNorm entry points have one caller each, their autograd node.
def _f32(dev, *shape):
    return torch.empty(*shape, device=dev, dtype=torch.float32)


def _bncl_blocks(x):
    return _lib.lib().tamtr_bncl_blocks(x.shape[0], x.shape[1], dtype_code(x))


def _bncl_stats_buffers(x):
    """mean_rstd [C, 2] and the (count, mean, M2) partials of the statistics pass over rows x [N, C]."""
    C = x.shape[1]
    return _f32(x.device, C, 2), _f32(x.device, C * _bncl_blocks(x) * 3)


def _bncl_fwd(x, gamma, beta, rm, rv, eps, mom, act, residual=None, seg=None):
    """Channels-last rows x [N, C] -> y, the fp32 forms of gamma and beta, mean_rstd [C, 2].  seg = (destination pointer, seg_rows,
    seg_pitch): the result is written as image segments of a wider buffer (include/tamtr_hip.h tamtr_bncl_act_seg_fwd) and y is None."""
    N, C = x.shape
    g32, b32 = _c(gamma.float()), _c(beta.float())
    y = None if seg else torch.empty_like(x)
    mr, part = _bncl_stats_buffers(x)
    tail = (ptr(mr), ptr(part), N, C, float(eps), float(mom), act, dtype_code(x), stream_ptr())
    if seg:
        call('tamtr_bncl_act_seg_fwd', ptr(x), ptr(g32), ptr(b32), ptr(rm), ptr(rv), *seg, *tail)
    else:
        res = None if residual is None else _c(residual.to(x.dtype))
        call('tamtr_bncl_act_fwd', ptr(x), ptr(g32), ptr(b32), ptr(rm), ptr(rv), ptr(res), ptr(y), *tail)
    return y, g32, b32, mr


def _bncl_bwd(gy, x, g32, b32, mr, act, seg=None):
    """-> d(x), and d(gamma), d(beta) in fp32.  gy: rows as _gy_rows leaves them; or seg = (pointer, seg_rows, seg_pitch): the gradient is
    read as image segments of a wider buffer (the gradient of _bncl_fwd's segmented result)."""
    N, C = x.shape
    gx = torch.empty_like(x)
    gg, gb = _f32(x.device, C), _f32(x.device, C)
    part = _f32(x.device, C * _bncl_blocks(x) * 2 + 2 * C)
    src = seg if seg else (ptr(gy), gy.stride(0))
    call('tamtr_bncl_act_seg_bwd' if seg else 'tamtr_bncl_act_bwd', *src, ptr(x), ptr(g32), ptr(b32), ptr(mr), ptr(gx), ptr(gg), ptr(gb), ptr(part),
         N, C, act, dtype_code(x), stream_ptr())
    return gx, gg, gb


def _gy_rows(gy, x):
    """gy as the kernels take it: x's dtype, unit column stride, 16-byte aligned rows (a channel slice of a wider map is fine)."""
    C = x.shape[1]
    gy = gy.to(x.dtype)
    v = 8 if (x.dtype == torch.bfloat16 and C % 8 == 0) else 4
    if not (gy.stride(1) == 1 and gy.stride(0) >= C and gy.stride(0) % v == 0 and gy.data_ptr() % 16 == 0 and (C & (C - 1)) == 0):
        gy = gy.contiguous()
    return gy


class _BNAct(torch.autograd.Function):
    """Training-mode BatchNorm2d (+ SiLU) on an NCHW map - csrc/bn.hip.  running_mean / running_var are updated in place."""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, eps, momentum, silu):
        require_gpu(x, gamma, beta)
        x = _c(x)
        B, C = x.shape[:2]
        HW = x.numel() // (B * C)
        g32, b32 = _c(gamma.float()), _c(beta.float())
        y = torch.empty_like(x)
        mr = _f32(x.device, C, 2)
        part = _f32(x.device, C * _lib.lib().tamtr_bn_slices(B, HW) * 3)
        call('tamtr_bn_act_fwd', ptr(x), ptr(g32), ptr(b32), ptr(running_mean), ptr(running_var), ptr(y), ptr(mr), ptr(part), B, C, HW,
             float(eps), float(momentum), int(bool(silu)), dtype_code(x), stream_ptr())
        ctx.save_for_backward(x, g32, b32, mr)
        ctx.cfg = (int(bool(silu)), gamma.dtype, beta.dtype)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, g32, b32, mr = ctx.saved_tensors
        act, g_dt, b_dt = ctx.cfg
        B, C = x.shape[:2]
        HW = x.numel() // (B * C)
        gy = _c(gy.to(x.dtype))
        gx = torch.empty_like(x)
        gg, gb = _f32(x.device, C), _f32(x.device, C)
        part = _f32(x.device, C * _lib.lib().tamtr_bn_slices(B, HW) * 2)
        call('tamtr_bn_act_bwd', ptr(gy), ptr(x), ptr(g32), ptr(b32), ptr(mr), ptr(gx), ptr(gg), ptr(gb), ptr(part), B, C, HW, act,
             dtype_code(x), stream_ptr())
        return gx, gg.to(g_dt), gb.to(b_dt), None, None, None, None, None


class _BNActCL(torch.autograd.Function):
    """Same on a channels-last [N, C] map (token-major)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, eps, momentum, silu, residual=None):
        require_gpu(x, gamma, beta)
        x = _c(x)
        y, *saved = _bncl_fwd(x, gamma, beta, running_mean, running_var, eps, momentum, int(bool(silu)), residual)
        ctx.save_for_backward(x, *saved)
        ctx.cfg = (int(bool(silu)), gamma.dtype, beta.dtype, None if residual is None else residual.dtype)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, g32, b32, mr = ctx.saved_tensors
        act, g_dt, b_dt, res_dt = ctx.cfg
        g_res = None if res_dt is None else gy.to(res_dt)   # y = act(bn(x)) + residual: the shortcut's gradient is gy itself
        # (a channel slice of a concatenation's gradient is read in place through its row pitch)
        gx, gg, gb = _bncl_bwd(_gy_rows(gy, x), x, g32, b32, mr, act)
        return gx, gg.to(g_dt), gb.to(b_dt), None, None, None, None, None, g_res


def _bncl_down2_fwd(x, gamma, beta, rm, rv, eps, mom, act, B, H, W):
    """Channels-last rows x [B * H * W, C] -> act(bn(x)) at the pixels (2h, 2w) as rows [B * H/2 * W/2, C], the fp32 forms of gamma and
    beta, mean_rstd [C, 2]: the statistics pass of _bncl_fwd over the full map, the apply pass over the kept rows."""
    N, C = x.shape
    g32, b32 = _c(gamma.float()), _c(beta.float())
    y = x.new_empty(N // 4, C)
    mr, part = _bncl_stats_buffers(x)
    call('tamtr_bncl_act_down2_fwd', ptr(x), ptr(g32), ptr(b32), ptr(rm), ptr(rv), ptr(y), ptr(mr), ptr(part), B, H, W, C, float(eps), float(mom),
         act, dtype_code(x), stream_ptr())
    return y, g32, b32, mr


def _bncl_down2_bwd(gy, x, g32, b32, mr, act, B, H, W):
    """-> d(x) over the full map, and d(gamma), d(beta) in fp32.  gy: the quarter map's rows as _gy_rows leaves them."""
    C = x.shape[1]
    gx = torch.empty_like(x)
    gg, gb = _f32(x.device, C), _f32(x.device, C)
    part = _f32(x.device, C * _bncl_blocks(x) * 2 + 2 * C)   # the reduce runs in the full map's chunks (the sums keep _bncl_bwd's bits)
    call('tamtr_bncl_act_down2_bwd', ptr(gy), gy.stride(0), ptr(x), ptr(g32), ptr(b32), ptr(mr), ptr(gx), ptr(gg), ptr(gb), ptr(part), B, H, W, C,
         act, dtype_code(x), stream_ptr())
    return gx, gg, gb


class _BNActDown2CL(torch.autograd.Function):
    """act(bn(x))[:, ::2, ::2] on a channels-last map given as rows x [B * H * W, C]: a Conv whose only consumer is Upsample(0.5).  Three
    quarters of the BatchNorm output are never made, and the backward never reads the zeros a resample backward would have filled in
    (csrc/bn.hip tamtr_bncl_act_down2_*).  Returns rows [B * H/2 * W/2, C]."""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, eps, momentum, silu, B, H, W):
        require_gpu(x, gamma, beta)
        x = _c(x)
        y, *saved = _bncl_down2_fwd(x, gamma, beta, running_mean, running_var, eps, momentum, int(bool(silu)), B, H, W)
        ctx.save_for_backward(x, *saved)
        ctx.cfg = (int(bool(silu)), gamma.dtype, beta.dtype, B, H, W)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, g32, b32, mr = ctx.saved_tensors
        act, g_dt, b_dt, B, H, W = ctx.cfg
        gx, gg, gb = _bncl_down2_bwd(_gy_rows(gy, x), x, g32, b32, mr, act, B, H, W)
        return gx, gg.to(g_dt), gb.to(b_dt), None, None, None, None, None, None, None, None


class _BN2ActCL(torch.autograd.Function):
    """y = act(bn1(x1) + bn2(x2)) on channels-last [N, C] maps, both BatchNorms in training mode: RepConvN's training form
    (extra_modules/block.py:66-69) in one apply pass and one backward pair (csrc/bn.hip tamtr_bncl2_act_*)."""

    @staticmethod
    def forward(ctx, x1, ga1, be1, rm1, rv1, x2, ga2, be2, rm2, rv2, eps, momentum, silu):
        require_gpu(x1, x2, ga1, ga2)
        x1, x2 = _c(x1), _c(x2)
        N, C = x1.shape
        p1 = [_c(t.float()) for t in (ga1, be1, ga2, be2)]
        y = torch.empty_like(x1)
        mr = _f32(x1.device, 2, C, 2)
        part = _f32(x1.device, 2 * C * _bncl_blocks(x1) * 3)
        call('tamtr_bncl2_act_fwd', ptr(x1), ptr(p1[0]), ptr(p1[1]), ptr(rm1), ptr(rv1), ptr(x2), ptr(p1[2]), ptr(p1[3]), ptr(rm2), ptr(rv2),
             ptr(y), ptr(mr), ptr(part), N, C, float(eps), float(momentum), int(bool(silu)), dtype_code(x1), stream_ptr())
        ctx.save_for_backward(x1, x2, *p1, mr)
        ctx.cfg = (int(bool(silu)), ga1.dtype, be1.dtype, ga2.dtype, be2.dtype)
        return y

    @staticmethod
    def backward(ctx, gy):
        x1, x2, g1, b1, g2, b2, mr = ctx.saved_tensors
        act, dt_g1, dt_b1, dt_g2, dt_b2 = ctx.cfg
        N, C = x1.shape
        gy = _gy_rows(gy, x1)
        gx1, gx2 = torch.empty_like(x1), torch.empty_like(x2)
        gg = _f32(x1.device, 4, C)
        part = _f32(x1.device, C * _bncl_blocks(x1) * 3 + 3 * C)
        call('tamtr_bncl2_act_bwd', ptr(gy), gy.stride(0), ptr(x1), ptr(x2), ptr(g1), ptr(b1), ptr(g2), ptr(b2), ptr(mr), ptr(gx1), ptr(gx2),
             gg[0].data_ptr(), gg[1].data_ptr(), gg[2].data_ptr(), gg[3].data_ptr(), ptr(part), N, C, act, dtype_code(x1), stream_ptr())
        return (gx1, gg[0].to(dt_g1), gg[1].to(dt_b1), None, None, gx2, gg[2].to(dt_g2), gg[3].to(dt_b2), None, None, None, None, None)


def _cat_segments(t, Ls):
    """The levels' segments of t [B, sum L_i, C] as the launchers take them: (pointer to image 0's rows, seg_rows, seg_pitch)."""
    C = t.shape[2]
    return [(t.data_ptr() + sum(Ls[:i]) * C * t.element_size(), L, sum(Ls) * C) for i, L in enumerate(Ls)]


class _BNCatCL(torch.autograd.Function):
    """feats [B, sum L_i, C] = torch.cat([BatchNorm_i(y_i).view(B, L_i, C) for i], 1) with every level's BatchNorm (training mode, no
    activation) written straight into its segment of the result, and the backward reading its segment of d(feats) where it lies
    (csrc/bn.hip tamtr_bncl_act_seg_*): the MEH token memory (head.py:1087,1202-1219) without the 550 MB concatenation copy and the three
    slice copies of its gradient.  y_i [B * L_i, C]; running statistics are updated in place like ops.bn_act."""

    @staticmethod
    def forward(ctx, B, eps, moms, n, *args):
        ys, gammas, betas, rms, rvs = (args[k * n:(k + 1) * n] for k in range(5))
        require_gpu(*ys)
        ys = [_c(y) for y in ys]
        Ls = [y.shape[0] // B for y in ys]
        feats = torch.empty(B, sum(Ls), ys[0].shape[1], device=ys[0].device, dtype=ys[0].dtype)
        saved = []
        for y, ga, be, rm, rv, mom, seg in zip(ys, gammas, betas, rms, rvs, moms, _cat_segments(feats, Ls)):
            saved += [y, *_bncl_fwd(y, ga, be, rm, rv, eps, mom, 0, seg=seg)[1:]]
        ctx.save_for_backward(*saved)
        ctx.cfg = (B, n, Ls, [g.dtype for g in gammas], [b.dtype for b in betas])
        return feats

    @staticmethod
    def backward(ctx, gf):
        B, n, Ls, gdt, bdt = ctx.cfg
        saved = ctx.saved_tensors
        gf = _c(gf.to(saved[0].dtype))
        gxs, ggs, gbs = [], [], []
        for i, seg in enumerate(_cat_segments(gf, Ls)):
            gx, gg, gb = _bncl_bwd(None, *saved[4 * i:4 * i + 4], 0, seg=seg)
            gxs.append(gx); ggs.append(gg.to(gdt[i])); gbs.append(gb.to(bdt[i]))
        return (None, None, None, None, *gxs, *ggs, *gbs, *([None] * (2 * n)))


_BN_COUNTERS = None


def begin_bn_counter_batch():
    """Defer the `num_batches_tracked += 1` of every bn_act call (170 one-element kernels per step) to end_bn_counter_batch()."""
    global _BN_COUNTERS
    _BN_COUNTERS = []
    return _BN_COUNTERS


def end_bn_counter_batch():
    global _BN_COUNTERS
    pending, _BN_COUNTERS = _BN_COUNTERS, None
    if pending:
        torch._foreach_add_(pending, 1)


def _bn_train_call(bn):
    """(running_mean, running_var, momentum) for one training-mode call of `bn`, the statistics None when it tracks none; counts the call:
    num_batches_tracked += 1 (deferred to one multi-tensor kernel inside a counter batch)."""
    if bn.track_running_stats:
        if _BN_COUNTERS is not None and bn.momentum is not None:
            _BN_COUNTERS.append(bn.num_batches_tracked)
        else:
            bn.num_batches_tracked += 1
    mom = bn.momentum if bn.momentum is not None else 1.0 / float(bn.num_batches_tracked)
    return (bn.running_mean, bn.running_var, mom) if bn.track_running_stats else (None, None, mom)


def bn_cl_ok(C, dtype):
    """Channel counts the channels-last BatchNorm kernels take (include/tamtr_hip.h: tamtr_bncl_act_fwd)."""
    v = 8 if dtype == torch.bfloat16 and C % 8 == 0 else 4
    return C % 4 == 0 and C <= 1024 and C // v <= 256 and 256 % (C // v) == 0


def bn_act(x, bn, silu, residual=None):
    """act(bn(x)) [+ residual] for an nn.BatchNorm2d in training mode (batch statistics; running stats and num_batches_tracked
    updated).  residual: only with the channels-last [N, C] form."""
    rm, rv, mom = _bn_train_call(bn)
    if x.dim() == 2:   # [N, C] token-major / channels-last map
        return _BNActCL.apply(x, bn.weight, bn.bias, rm, rv, bn.eps, mom, silu, residual)
    y = _BNAct.apply(x, bn.weight, bn.bias, rm, rv, bn.eps, mom, silu)
    return y if residual is None else y + residual


_BN_DOWN2 = _os.environ.get('TAMTR_BN_DOWN2') != '0'   # A/B switch: 0 = the full BatchNorm map, then the resample kernel, as before bn_act_down2


def bn_down2_ok(y, bn):
    """A convolution output y [B, C, H, W] whose BatchNorm (+ activation) can run together with a following nearest x0.5 resample:
    channels-last on the GPU, a channel count the [N, C] kernels take, even H and W, training mode, affine, fp32 or bf16; TAMTR_BN_DOWN2 != 0."""
    return (_BN_DOWN2 and y.is_cuda and y.dim() == 4 and y.dtype in (torch.float32, torch.bfloat16) and is_cl(y) and bn_cl_ok(y.shape[1], y.dtype)
            and y.shape[2] % 2 == 0 and y.shape[3] % 2 == 0 and bn.training and bn.affine)


def bn_act_down2(x_rows, bn, silu, B, H, W):
    """act(bn(x))[:, ::2, ::2] for an nn.BatchNorm2d in training mode on the rows [B * H * W, C] of a channels-last map: rows
    [B * H/2 * W/2, C].  Batch statistics over the full map; running stats and num_batches_tracked as bn_act."""
    rm, rv, mom = _bn_train_call(bn)
    return _BNActDown2CL.apply(x_rows, bn.weight, bn.bias, rm, rv, bn.eps, mom, silu, B, H, W)


def bn2_act(x1, bn1, x2, bn2, silu):
    """act(bn1(x1) + bn2(x2)) on channels-last [N, C] maps, both BatchNorm2d in training mode with running statistics."""
    if bn1.eps != bn2.eps or bn1.momentum != bn2.momentum or not (bn1.track_running_stats and bn2.track_running_stats):
        raise _lib.TamtrHipError('bn2_act: the two BatchNorms must share eps / momentum and track running statistics')
    rm1, rv1, mom = _bn_train_call(bn1)
    rm2, rv2, _ = _bn_train_call(bn2)
    return _BN2ActCL.apply(x1, bn1.weight, bn1.bias, rm1, rv1, x2, bn2.weight, bn2.bias, rm2, rv2, bn1.eps, mom, silu)


def bn_cat_cl(ys, bns, B):
    """The token memory: per level y_i [B * L_i, C] -> BatchNorm_i (training mode, batch statistics, no activation) -> [B, sum L_i, C],
    each level written into its segment directly.  All BatchNorms share eps; C a power of two."""
    rms, rvs, moms = zip(*[_bn_train_call(bn) for bn in bns])
    return _BNCatCL.apply(int(B), float(bns[0].eps), tuple(float(m) for m in moms), len(ys), *ys, *[bn.weight for bn in bns],
                          *[bn.bias for bn in bns], *rms, *rvs)


def bn_cat_cl_ok(ys, bns):
    C = ys[0].shape[1]
    return (all(y.is_cuda and y.dim() == 2 and y.shape[1] == C and y.dtype == ys[0].dtype and y.dtype in (torch.float32, torch.bfloat16) for y in ys)
            and C & (C - 1) == 0 and bn_cl_ok(C, ys[0].dtype) and all(bn.training and bn.track_running_stats and bn.affine and bn.eps == bns[0].eps for bn in bns))


@torch.no_grad()
def bn_stats_cl(x2d, bn):
    """Batch statistics of a channels-last [N, C] map for a consumer that normalises in its own load: mean_rstd f32 [C, 2]; updates the
    BatchNorm's running statistics and counter like a training-mode forward."""
    require_gpu(x2d)
    x2d = _c(x2d)
    N, C = x2d.shape
    rm, rv, mom = _bn_train_call(bn)
    mr, part = _bncl_stats_buffers(x2d)
    call('tamtr_bncl_stats', ptr(x2d), ptr(rm), ptr(rv), ptr(mr), ptr(part), N, C, float(bn.eps), float(mom), dtype_code(x2d), stream_ptr())
    return mr

