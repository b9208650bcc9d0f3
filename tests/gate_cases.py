"""Shapes and seeded inputs of the text gate and CPAM checks against fp64 (tests/test_gpu_gates_ref64.py), shared with the host test
that proves every one of them free of ambiguous argmax decisions (tests/test_ref64_host.py)."""
import torch

from weights import rnd

# (B, C, nh, H, W, T): gate_fwd_kernel / gate_bwd_kernel (NCHW).  TC = 16 text rows per pass, 256 threads x PX pixels per block.
GATE_NCHW = {
    'vec_one_pass': (2, 64, 2, 12, 12, 10),       # PX = 4, one TC pass
    'px1_t37_hc64': (1, 64, 1, 5, 7, 37),         # HW = 35: PX = 1; three passes, the last of 5 rows
    'hc48_t80': (2, 96, 2, 6, 6, 80),             # five full passes
    't17': (1, 64, 2, 6, 6, 17),                  # one row past TC
    't1': (3, 128, 4, 5, 20, 1),
    'two_blocks': (1, 256, 8, 18, 58, 10),        # HW = 1044 > 1024: a second, partly filled block along x
}

# (C, nh, H, W, T) at B = 2: gate_cl_fwd_kernel (channels-last, BatchNorm folded into the load)
GATE_CL = {
    'hc64_shuffle': (64, 1, 10, 6, 10),           # lph = 8: the __shfl_xor step after the two DPP steps
    'c512_wave_row': (512, 8, 6, 6, 10),          # one row = 64 lanes
    'tile_tail_row_tail': (256, 8, 9, 7, 13),     # T C = 3328 > 3072: the text tile's tail loop; 63 rows against 32 per workgroup
    't80': (64, 8, 12, 12, 80),                   # T C = 5120
    'rows25_of_64': (128, 8, 5, 5, 10),
    'c8_lane_row': (8, 1, 40, 30, 3),             # one lane per row, 1200 rows against 1024 per workgroup
}
GATE_CL_CONTIGUOUS = ('hc64_shuffle', 'c512_wave_row')

# (B, C, H, W)
CPAM_CL_BF16 = [(2, 64, 4, 6), (1, 128, 2, 2), (2, 256, 6, 4), (1, 512, 10, 12)]
CPAM_CL_F32 = [(1, 32, 8, 8), (1, 512, 4, 2), (2, 128, 10, 6)]
CPAM_NCHW = [(2, 16, 2, 2), (1, 8, 14, 30), (2, 64, 12, 16), (1, 256, 6, 6)]      # (1, 256, 6, 6): 32 channels per chunk, KEEP = 0


def gate_inputs(shape, dt, seed=1, bias=None):
    """x, gk, bias, v, gout for the NCHW gate: maps in dt, text rows and bias fp32."""
    B, C, nh, H, W, T = shape
    x, v, gout = (rnd((B, C, H, W), seed + i).to(dt) for i in (0, 2, 4))
    gk = rnd((B, T, C), seed + 1, 0.3)
    return x, gk, (rnd((nh,), seed + 3, 0.2) if bias is None else torch.tensor(bias)), v, gout


def gate_cl_inputs(case, dt, wide, seed=1):
    """The channels-last gate's operands at B = 2: e = channel slice number wide - 1 of a map `wide` times as wide (wide = 1: contiguous),
    the raw convolution output v, text rows, bias, and a BatchNorm's gamma, beta and mean_rstd [C, 2] (fp64 batch statistics of v,
    rounded to fp32).  Everything on the CPU; e is returned as (whole map, channel offset)."""
    C, nh, H, W, T = GATE_CL[case]
    B = 2
    emap = (rnd((B, wide * C, H, W), seed) * 1.5).to(dt).contiguous(memory_format=torch.channels_last)
    v = (rnd((B, C, H, W), seed + 1) * 2 + 0.5 * rnd((1, C, 1, 1), seed + 2)).to(dt).contiguous(memory_format=torch.channels_last)
    gk, bias = rnd((B, T, C), seed + 3, 0.3), rnd((nh,), seed + 4, 0.3)
    gamma, beta = 1 + 0.2 * rnd((C,), seed + 5), 0.1 * rnd((C,), seed + 6)
    vd = v.double()
    mean, var = vd.mean((0, 2, 3)), vd.var((0, 2, 3), unbiased=False)
    mean_rstd = torch.stack([mean, (var + 1e-5).rsqrt()], 1).float().contiguous()
    return emap, (wide - 1) * C, v, gk, bias, mean_rstd, gamma, beta


def cpam_inputs(shape, dt, seed=5):
    """x and gout of CPAM, rounded to dt, as fp32-free CPU tensors in dt (NCHW-contiguous)."""
    return (rnd(shape, seed) * 2).to(dt), rnd(shape, seed + 1).to(dt)


# B C = 65 280 of the 65 535 rows cpam_dp_kernel's grid.y can take.  fp32 only: with 32 bf16 channels per chunk on a 2 x 2 map (one pooled
# cell, so one channel gate per channel) equal values in two channels tie the chunk maximum exactly, at about 70 of the 8160 decisions
# whatever the seed, and the routed gradient is then not defined.
CPAM_NCHW_GRID_LIMIT = (255, 256, 2, 2)

# Seeds for which the input has no ambiguous argmax (ref64.ambiguous on the fp64 reference alone; tests/test_ref64_host.py proves it for
# every entry).  Cases not listed use the generators' default seed.
GATE_SEED = {('two_blocks', torch.float32): 301, ('two_blocks', torch.bfloat16): 101}
CPAM_SEED = {((2, 64, 4, 6), torch.bfloat16): 105, ((1, 512, 10, 12), torch.bfloat16): 305, ((2, 128, 10, 6), torch.float32): 105,
             ((1, 256, 6, 6), torch.bfloat16): 205, ((255, 256, 2, 2), torch.float32): 505}
