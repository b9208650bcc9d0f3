#!/usr/bin/env python
"""Time the CLIP text tower (tamtr_amd.text.ClipTextEncoder.encode_tokens) at ViT-B/32 geometry against the same tower composed of torch's
fp32 library ops (F.linear, F.layer_norm, F.scaled_dot_product_attention with a causal mask) on the same card; one JSON line.

    python tools/text_bench.py [--n 10 80 1203] [--windows 5] [--reps 3] [--once 80]

Random weights at CLIP's initialisation scales and seeded ids.  Per n the two paths run in alternating windows of --reps encodes, each
window timed with device events after a warm-up of both; the median window and the min..max spread are reported per encode.  `linear_f32`
is also timed alone on the 512 -> 2048 product at M = 77 * 80 and given as a fraction of the fp32 MFMA peak (157.3 TFLOP/s).
--once N: warm up, then one own-path encode of N prompts and nothing else - the program to put under `rocprofv3 --kernel-trace --stats`.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_F32_MFMA = 157.3e12


def torch_tower(enc, ids, normalize=True):
    """The tower on library ops, fp32: what a user without this package would run."""
    import torch
    import torch.nn.functional as F
    n, L = ids.shape
    W, H = enc.width, enc.heads
    x = enc.token_embedding.weight[ids.long()] + enc.positional_embedding[:L]
    for b in enc.transformer.resblocks:
        h = F.layer_norm(x, (W,), b.ln_1.weight, b.ln_1.bias, b.ln_1.eps)
        q, k, v = (t.reshape(n, L, H, W // H).transpose(1, 2) for t in F.linear(h, b.attn.in_proj_weight, b.attn.in_proj_bias).split(W, -1))
        o = F.scaled_dot_product_attention(q, k, v, is_causal=True).transpose(1, 2).reshape(n, L, W)
        x = x + F.linear(o, b.attn.out_proj.weight, b.attn.out_proj.bias)
        h = F.linear(F.layer_norm(x, (W,), b.ln_2.weight, b.ln_2.bias, b.ln_2.eps), b.mlp.c_fc.weight, b.mlp.c_fc.bias)
        x = x + F.linear(h * torch.sigmoid(1.702 * h), b.mlp.c_proj.weight, b.mlp.c_proj.bias)
    x = F.layer_norm(x, (W,), enc.ln_final.weight, enc.ln_final.bias, enc.ln_final.eps)
    f = x[torch.arange(n, device=x.device), ids.long().argmax(-1)] @ enc.text_projection
    return f / f.norm(dim=-1, keepdim=True) if normalize else f


def prompts(n, vocab, context, seed=0):
    import torch
    g = torch.Generator().manual_seed(seed)
    ids = torch.zeros(n, context, dtype=torch.int32)
    for i in range(n):
        m = int(torch.randint(3, 20, (1,), generator=g))      # class-name prompts are short
        ids[i, 0], ids[i, m - 1] = vocab - 2, vocab - 1
        ids[i, 1:m - 1] = torch.randint(1, vocab - 2, (m - 2,), generator=g, dtype=torch.int32)
    return ids


def window(fn, reps):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--n', type=int, nargs='+', default=[10, 80, 1203])
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--once', type=int, default=0, help='one own-path encode of this many prompts after a warm-up, nothing else (for a kernel trace)')
    args = ap.parse_args(argv)
    import torch
    import tamtr_amd  # noqa: F401
    from tamtr_amd import ops
    from tamtr_amd.text import ClipTextEncoder
    assert torch.cuda.is_available(), 'text_bench needs an MI355X'
    torch.manual_seed(0)
    enc = ClipTextEncoder().cuda()
    if args.once:
        ids = prompts(args.once, enc.vocab_size, enc.context_length).cuda()
        enc.encode_tokens(ids)
        torch.cuda.synchronize()
        enc.encode_tokens(ids)
        torch.cuda.synchronize()
        print(json.dumps({'tool': 'text_bench', 'once': args.once}))
        return
    res = {'tool': 'text_bench', 'geometry': 'ViT-B/32 text tower (width 512, 12 layers, 8 heads, context 77)', 'windows': args.windows,
           'reps': args.reps, 'encode_ms': {}}
    with torch.no_grad():
        for n in args.n:
            ids = prompts(n, enc.vocab_size, enc.context_length).cuda()
            own, lib = (lambda: enc.encode_tokens(ids)), (lambda: torch_tower(enc, ids))
            diff = float((own() - lib()).abs().max())
            for _ in range(2):
                own(), lib()
            torch.cuda.synchronize()
            t_own, t_lib = [], []
            for _ in range(args.windows):        # alternating windows
                t_own.append(window(own, args.reps))
                t_lib.append(window(lib, args.reps))
            res['encode_ms'][str(n)] = {
                'own': round(statistics.median(t_own), 3), 'own_min_max': [round(min(t_own), 3), round(max(t_own), 3)],
                'torch_fp32': round(statistics.median(t_lib), 3), 'torch_min_max': [round(min(t_lib), 3), round(max(t_lib), 3)],
                'max_abs_diff': diff}
        M, K, N = 77 * 80, 512, 2048
        x, w, b = torch.randn(M, K, device='cuda'), torch.randn(N, K, device='cuda') * K ** -0.5, torch.randn(N, device='cuda')
        out = torch.empty(M, N, device='cuda')
        fn = lambda: ops.linear_f32(x, w, b, act='quick_gelu', out=out)   # noqa: E731
        lf = lambda: torch.nn.functional.linear(x, w, b)                   # noqa: E731
        for _ in range(5):
            fn(), lf()
        t = statistics.median(window(fn, 50) for _ in range(5))
        tl = statistics.median(window(lf, 50) for _ in range(5))
        flops = 2.0 * M * N * K
        res['linear_f32_512_to_2048'] = {'M': M, 'ms': round(t, 4), 'tflops': round(flops / t / 1e9, 2),
                                         'fraction_of_f32_mfma_peak': round(flops / (t * 1e-3) / PEAK_F32_MFMA, 3),
                                         'torch_linear_ms': round(tl, 4), 'note': 'device events around 50 back-to-back launches'}
    print(json.dumps(res))


if __name__ == '__main__':
    main()
