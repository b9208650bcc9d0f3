"""fp64 restatement of CLIP's text tower (clip/model.py CLIP.encode_text) for tests/test_text_host.py and tests/test_gpu_text.py, with the
magnitudes (the same contraction on absolute values) that ref64.check takes.  `sd` holds OpenAI CLIP's parameter names.  encode() runs in
whatever dtype / device `sd` is in, so the same lines evaluated in fp32 on the GPU are the tests' independent fp32 yardstick."""
import torch
import torch.nn.functional as F


def embed(ids, tok, pos):
    return tok[ids.long()] + pos[:ids.shape[1]]


def linear(x, w, b, act=None, residual=None):
    """epi(x w^T + b) and its magnitude |x| |w|^T + |b| (+ |residual|); QuickGELU y sigmoid(1.702 y) keeps the magnitude (|g(y)| <= |y|)."""
    y, m = x @ w.T + b, x.abs() @ w.abs().T + b.abs()
    if act == 'quick_gelu':
        y = y * torch.sigmoid(1.702 * y)
    if residual is not None:
        y, m = y + residual, m + residual.abs()
    return y, m


def layer_norm(x, g, b, eps=1e-5):
    mu = x.mean(-1, keepdim=True)
    rstd = ((x - mu).pow(2).mean(-1, keepdim=True) + eps).rsqrt()
    return (x - mu) * rstd * g + b, (x.abs() + x.abs().mean(-1, keepdim=True)) * rstd * g.abs() + b.abs()


def attention(qkv, heads, sdpa=False):
    """Causal softmax attention on a packed [n, L, 3W] projection -> [n, L, W]."""
    n, L, W3 = qkv.shape
    q, k, v = (t.reshape(n, L, heads, -1).transpose(1, 2) for t in qkv.split(W3 // 3, -1))
    if sdpa:
        o = F.scaled_dot_product_attention(q, k, v, is_causal=True)
    else:
        s = q @ k.transpose(-1, -2) * q.shape[-1] ** -0.5
        s = s.masked_fill(torch.ones(L, L, dtype=torch.bool, device=s.device).triu(1), float('-inf'))
        o = torch.softmax(s, -1) @ v
    return o.transpose(1, 2).reshape(n, L, W3 // 3)


def pool_project(x, ids, g, b, proj, eps=1e-5, normalize=True):
    """x [n, L, W]: ln_final of the row at argmax(ids) (first maximum), @ proj, optional L2 normalisation; value and magnitude."""
    row = x[torch.arange(x.shape[0], device=x.device), ids.long().argmax(-1)]
    y, my = layer_norm(row, g, b, eps)
    o, mo = y @ proj, my @ proj.abs()
    if normalize:
        nrm = o.norm(dim=-1, keepdim=True)
        o, mo = o / nrm, mo / nrm + (o / nrm).abs() * mo.norm(dim=-1, keepdim=True) / nrm     # d|o| <= |d o|
    return o, mo


def encode(sd, ids, heads, normalize=True, sdpa=False):
    x = embed(ids, sd['token_embedding.weight'], sd['positional_embedding'])
    n, L, W = x.shape
    i = 0
    while f'transformer.resblocks.{i}.ln_1.weight' in sd:
        p = {k: sd[f'transformer.resblocks.{i}.{k}'] for k in ('ln_1.weight', 'ln_1.bias', 'ln_2.weight', 'ln_2.bias', 'attn.in_proj_weight',
             'attn.in_proj_bias', 'attn.out_proj.weight', 'attn.out_proj.bias', 'mlp.c_fc.weight', 'mlp.c_fc.bias', 'mlp.c_proj.weight', 'mlp.c_proj.bias')}
        h = layer_norm(x, p['ln_1.weight'], p['ln_1.bias'])[0]
        o = attention(linear(h, p['attn.in_proj_weight'], p['attn.in_proj_bias'])[0], heads, sdpa)
        x = linear(o, p['attn.out_proj.weight'], p['attn.out_proj.bias'], residual=x)[0]
        h = layer_norm(x, p['ln_2.weight'], p['ln_2.bias'])[0]
        h = linear(h, p['mlp.c_fc.weight'], p['mlp.c_fc.bias'], act='quick_gelu')[0]
        x = linear(h, p['mlp.c_proj.weight'], p['mlp.c_proj.bias'], residual=x)[0]
        i += 1
    return pool_project(x, ids, sd['ln_final.weight'], sd['ln_final.bias'], sd['text_projection'], 1e-5, normalize)[0]


# ---------------------------------------------------------------------------------------------------- seeded inputs shared by the tests
def random_state(vocab, width, layers, context, embed, seed=0, dtype=torch.float64):
    """CLIP's initialisation scales (clip/model.py initialize_parameters) from a seeded generator; LayerNorm affine and biases are made
    non-trivial so that a dropped bias or gain shows."""
    g = torch.Generator().manual_seed(seed)

    def rn(*shape, std=1.0):
        return (torch.randn(*shape, generator=g, dtype=torch.float64) * std).to(dtype)
    W = width
    ps, at, fc = W ** -0.5 * (2 * layers) ** -0.5, W ** -0.5, (2 * W) ** -0.5
    sd = {'token_embedding.weight': rn(vocab, W, std=0.02), 'positional_embedding': rn(context, W, std=0.01),
          'ln_final.weight': 1 + rn(W, std=0.1), 'ln_final.bias': rn(W, std=0.1), 'text_projection': rn(W, embed, std=at)}
    for i in range(layers):
        b = f'transformer.resblocks.{i}.'
        sd.update({b + 'ln_1.weight': 1 + rn(W, std=0.1), b + 'ln_1.bias': rn(W, std=0.1), b + 'ln_2.weight': 1 + rn(W, std=0.1),
                   b + 'ln_2.bias': rn(W, std=0.1), b + 'attn.in_proj_weight': rn(3 * W, W, std=at), b + 'attn.in_proj_bias': rn(3 * W, std=0.02),
                   b + 'attn.out_proj.weight': rn(W, W, std=ps), b + 'attn.out_proj.bias': rn(W, std=0.02),
                   b + 'mlp.c_fc.weight': rn(4 * W, W, std=fc), b + 'mlp.c_fc.bias': rn(4 * W, std=0.02),
                   b + 'mlp.c_proj.weight': rn(W, 4 * W, std=ps), b + 'mlp.c_proj.bias': rn(W, std=0.02)})
    return sd


def random_prompts(lengths, vocab, context=77, seed=1):
    """int32 [n, context]: id vocab - 2 (start), random ids below vocab - 2, id vocab - 1 (end: the arg-max), zero padding; `lengths` count
    the start and end tokens, so 2 is the empty prompt and `context` a full one."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.zeros(len(lengths), context, dtype=torch.int32)
    for i, n in enumerate(lengths):
        ids[i, 0], ids[i, n - 1] = vocab - 2, vocab - 1
        ids[i, 1:n - 1] = torch.randint(1, vocab - 2, (n - 2,), generator=g, dtype=torch.int32)
    return ids
