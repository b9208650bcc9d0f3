"""The frozen CLIP text tower on the package's own kernels, and CLIP's byte-level BPE tokenizer.

Replaces `clip.tokenize` + `text_model.encode_text` of the reference (models/rtdetrworld/train.py:148-150, nn/tasks.py:552-571 set_classes,
the validator's vocabulary): 12 pre-LN residual blocks of width 512 at ViT-B/32 geometry, causal attention over a context of 77, QuickGELU
MLP, ln_final, the row at the end-of-text token, `@ text_projection`.  Forward only (the tower is frozen, train.py:24-25) and fp32 end to
end: a feature is encoded once per distinct prompt and then enters every class logit of every image.

Kernels: csrc/text.hip (embedding, fp32 MFMA dense layer with fused epilogues, pooled projection) + the existing self-attention and
LayerNorm kernels.  No CPU path: a module that is not on the GPU raises TamtrHipError.
"""
import gzip
import html
import re

import torch
import torch.nn as nn

from . import ops
from ._lib import TamtrHipError

CHUNK = 256   # prompts per pass of encode_tokens: bounds the activations (256 * 77 rows * 2048 MLP columns * 4 B = 161 MB at ViT-B/32)


class _Attention(nn.Module):
    """Parameter holder named as nn.MultiheadAttention names them (in_proj_weight, in_proj_bias, out_proj)."""

    def __init__(self, width):
        super().__init__()
        self.in_proj_weight = nn.Parameter(torch.empty(3 * width, width))
        self.in_proj_bias = nn.Parameter(torch.zeros(3 * width))
        self.out_proj = nn.Linear(width, width)


class _MLP(nn.Module):
    def __init__(self, width):
        super().__init__()
        self.c_fc = nn.Linear(width, 4 * width)
        self.c_proj = nn.Linear(4 * width, width)


class _ResBlock(nn.Module):
    def __init__(self, width):
        super().__init__()
        self.ln_1 = nn.LayerNorm(width)
        self.attn = _Attention(width)
        self.ln_2 = nn.LayerNorm(width)
        self.mlp = _MLP(width)


class _Transformer(nn.Module):
    def __init__(self, width, layers):
        super().__init__()
        self.resblocks = nn.ModuleList(_ResBlock(width) for _ in range(layers))


class ClipTextEncoder(nn.Module):
    """CLIP's text tower with OpenAI CLIP's parameter names, so a CLIP checkpoint's state_dict loads unchanged."""

    def __init__(self, vocab_size=49408, width=512, layers=12, context_length=77, embed_dim=512, heads=None):
        super().__init__()
        self.vocab_size, self.width, self.layers, self.context_length, self.embed_dim = vocab_size, width, layers, context_length, embed_dim
        self.heads = heads or width // 64
        if width % self.heads or width // self.heads not in (32, 64):
            raise ValueError(f'width {width} with {self.heads} heads: the attention kernel is built for head sizes 32 and 64')
        self.token_embedding = nn.Embedding(vocab_size, width)
        self.positional_embedding = nn.Parameter(torch.empty(context_length, width))
        self.transformer = _Transformer(width, layers)
        self.ln_final = nn.LayerNorm(width)
        self.text_projection = nn.Parameter(torch.empty(width, embed_dim))
        self._mask_bits = {}
        self.reset_parameters()
        self.requires_grad_(False)

    def reset_parameters(self):
        """CLIP's initialisation scales (clip/model.py initialize_parameters)."""
        W, n = self.width, self.layers
        nn.init.normal_(self.token_embedding.weight, std=0.02)
        nn.init.normal_(self.positional_embedding, std=0.01)
        proj_std, attn_std, fc_std = W ** -0.5 * (2 * n) ** -0.5, W ** -0.5, (2 * W) ** -0.5
        for b in self.transformer.resblocks:
            nn.init.normal_(b.attn.in_proj_weight, std=attn_std)
            nn.init.normal_(b.attn.out_proj.weight, std=proj_std)
            nn.init.normal_(b.mlp.c_fc.weight, std=fc_std)
            nn.init.normal_(b.mlp.c_proj.weight, std=proj_std)
        nn.init.normal_(self.text_projection, std=W ** -0.5)

    @classmethod
    def from_state_dict(cls, sd):
        """Build the tower from a CLIP state_dict (the text tower's or a full checkpoint's: `visual.*`, `logit_scale` and the other
        non-text keys are ignored); vocabulary, width, layers, context and embed dim follow from the shapes, heads = width // 64; fp16
        weights are widened to fp32.  A missing tensor raises KeyError with its name."""
        for k in ('token_embedding.weight', 'positional_embedding', 'text_projection'):
            if k not in sd:
                raise KeyError(f'not a CLIP text state_dict: {k} is missing')
        V, W = sd['token_embedding.weight'].shape
        blocks = [int(m.group(1)) for m in (re.match(r'transformer\.resblocks\.(\d+)\.', k) for k in sd) if m]
        if not blocks:
            raise KeyError('not a CLIP text state_dict: no transformer.resblocks.* tensors')
        enc = cls(vocab_size=V, width=W, layers=max(blocks) + 1, context_length=sd['positional_embedding'].shape[0],
                  embed_dim=sd['text_projection'].shape[1])
        own = enc.state_dict()
        missing = [k for k in own if k not in sd]
        if missing:
            raise KeyError(f'CLIP state_dict lacks {missing[0]}' + (f' (and {len(missing) - 1} more)' if len(missing) > 1 else ''))
        enc.load_state_dict({k: torch.as_tensor(sd[k]).detach().to(torch.float32) for k in own})
        return enc

    def _causal_bits(self, L, device):
        key = (L, str(device))
        if key not in self._mask_bits:
            blocked = torch.ones(L, L, dtype=torch.bool, device=device).triu_(1)    # query i may not attend to key j > i
            self._mask_bits[key] = ops.mask_words(blocked)
        return self._mask_bits[key]

    @torch.no_grad()
    def encode_tokens(self, ids, normalize=True):
        """ids integer [n, L <= context] (SimpleTokenizer's output) -> fp32 [n, embed_dim], unit-norm rows when `normalize`."""
        dev = self.text_projection.device
        if dev.type != 'cuda':
            raise TamtrHipError('ClipTextEncoder runs on the HIP kernels only: move it to the GPU (there is no CPU fallback)')
        for p in self.parameters():
            if p.dtype != torch.float32:
                raise TamtrHipError(f'ClipTextEncoder is fp32 end to end (found a {p.dtype} parameter)')
        ids = torch.as_tensor(ids)
        if ids.dim() != 2 or ids.is_floating_point():
            raise TamtrHipError(f'encode_tokens takes integer ids [n, L], got {ids.dtype} {tuple(ids.shape)}')
        if ids.shape[1] > self.positional_embedding.shape[0]:
            raise TamtrHipError(f'context {ids.shape[1]} is longer than positional_embedding ({self.positional_embedding.shape[0]})')
        ids = ids.to(device=dev, dtype=torch.int32).contiguous()
        if ids.shape[0] == 0:
            return torch.empty(0, self.embed_dim, device=dev)
        return torch.cat([self._encode_chunk(ids[i:i + CHUNK], normalize) for i in range(0, ids.shape[0], CHUNK)], 0)

    def _encode_chunk(self, ids, normalize):
        n, L = ids.shape
        W = self.width
        bits = self._causal_bits(L, ids.device)
        x = ops.text_embed(ids, self.token_embedding.weight, self.positional_embedding)
        for b in self.transformer.resblocks:
            h = ops.layer_norm(x, b.ln_1.weight, b.ln_1.bias, b.ln_1.eps)
            qkv = ops.linear_f32(h, b.attn.in_proj_weight, b.attn.in_proj_bias).view(n, L, 3 * W)
            o = ops.self_attention_packed(qkv[..., :W], qkv[..., W:2 * W], qkv[..., 2 * W:], self.heads, bits)
            ops.linear_f32(o.view(n * L, W), b.attn.out_proj.weight, b.attn.out_proj.bias, residual=x, out=x)
            h = ops.layer_norm(x, b.ln_2.weight, b.ln_2.bias, b.ln_2.eps)
            h = ops.linear_f32(h, b.mlp.c_fc.weight, b.mlp.c_fc.bias, act='quick_gelu')
            ops.linear_f32(h, b.mlp.c_proj.weight, b.mlp.c_proj.bias, residual=x, out=x)
        return ops.text_pool_project(x, ids, self.ln_final.weight, self.ln_final.bias, self.text_projection, self.ln_final.eps, normalize)

    def forward(self, ids, normalize=True):
        return self.encode_tokens(ids, normalize)


def load_clip_state_dict(path):
    """The state_dict of a CLIP checkpoint file: a torch-saved state_dict / {'state_dict': ...} / module, or the TorchScript archive
    that `clip.load` downloads."""
    try:
        ck = torch.load(path, map_location='cpu')
    except RuntimeError:   # a TorchScript archive is not a pickle torch.load reads
        return torch.jit.load(path, map_location='cpu').state_dict()
    if isinstance(ck, dict) and 'state_dict' in ck and 'token_embedding.weight' not in ck:
        ck = ck['state_dict']
    return ck.state_dict() if hasattr(ck, 'state_dict') else ck


# ---------------------------------------------------------------------------------------------------- tokenizer
def _bytes_to_unicode():
    """CLIP's reversible byte -> printable unicode character table (the 188 printable latin-1 bytes map to themselves, the other 68 to
    256 + i), in CLIP's order: it fixes the first 256 vocabulary ids."""
    bs = list(range(ord('!'), ord('~') + 1)) + list(range(ord('\xa1'), ord('\xac') + 1)) + list(range(ord('\xae'), ord('\xff') + 1))
    cs = bs[:]
    n = 0
    for b in range(256):
        if b not in bs:
            bs.append(b)
            cs.append(256 + n)
            n += 1
    return dict(zip(bs, (chr(c) for c in cs)))


class SimpleTokenizer:
    """CLIP's byte-level BPE (clip/simple_tokenizer.py restated) over the user's own merges file: `bpe_simple_vocab_16e6.txt.gz` or a
    plain-text merges file (an optional `#version` header line, then one `left right` merge per line).  Vocabulary order as CLIP's: the 256
    byte characters, the same with `</w>`, the merges, `<|startoftext|>`, `<|endoftext|>` - so the end-of-text token has the highest id.

    Differences from CLIP's: no `ftfy.fix_text` pass (mojibake in a prompt is not repaired; HTML entities are unescaped and whitespace is
    collapsed as CLIP does), and the word pattern uses the standard `re` module: letters are `[^\\W\\d_]`, a number is one `\\d` character
    (Unicode class Nd, where CLIP's `\\p{N}` also takes Nl / No such as superscripts and Roman numerals, which fall to the punctuation
    branch here).  ASCII and ordinary accented prompts tokenize identically."""

    N_MERGES = 49152 - 256 - 2   # how many merges CLIP keeps of its file

    def __init__(self, bpe_path, context_length=77):
        opener = gzip.open if str(bpe_path).endswith('.gz') else open
        with opener(bpe_path, 'rb') as f:
            lines = f.read().decode('utf-8').split('\n')
        if lines and lines[0].startswith('#version'):
            lines = lines[1:]
        merges = [tuple(ln.split()) for ln in lines if ln.strip()][:self.N_MERGES]
        bad = [m for m in merges if len(m) != 2]
        if bad:
            raise ValueError(f'{bpe_path}: a merge is two symbols on a line, got {" ".join(bad[0])!r}')
        self.byte_encoder = _bytes_to_unicode()
        vocab = list(self.byte_encoder.values())
        vocab = vocab + [v + '</w>' for v in vocab] + [''.join(m) for m in merges] + ['<|startoftext|>', '<|endoftext|>']
        self.encoder = dict(zip(vocab, range(len(vocab))))
        self.decoder = {v: k for k, v in self.encoder.items()}
        self.bpe_ranks = dict(zip(merges, range(len(merges))))
        self.cache = {'<|startoftext|>': '<|startoftext|>', '<|endoftext|>': '<|endoftext|>'}
        self.pat = re.compile(r"<\|startoftext\|>|<\|endoftext\|>|'s|'t|'re|'ve|'m|'ll|'d|[^\W\d_]+|\d|(?:[^\s\w]|_)+", re.IGNORECASE)
        self.context_length = context_length
        self.sot, self.eot = self.encoder['<|startoftext|>'], self.encoder['<|endoftext|>']

    @property
    def vocab_size(self):
        return len(self.encoder)

    def bpe(self, token):
        if token in self.cache:
            return self.cache[token]
        word = tuple(token[:-1]) + (token[-1] + '</w>',)
        while len(word) > 1:
            pairs = set(zip(word[:-1], word[1:]))
            best = min(pairs, key=lambda p: self.bpe_ranks.get(p, float('inf')))
            if best not in self.bpe_ranks:
                break
            first, second = best
            new, i = [], 0
            while i < len(word):
                if i < len(word) - 1 and word[i] == first and word[i + 1] == second:
                    new.append(first + second)
                    i += 2
                else:
                    new.append(word[i])
                    i += 1
            word = tuple(new)
        out = ' '.join(word)
        self.cache[token] = out
        return out

    def encode(self, text):
        text = html.unescape(html.unescape(text)).strip()
        text = re.sub(r'\s+', ' ', text).strip().lower()
        ids = []
        for token in self.pat.findall(text):
            token = ''.join(self.byte_encoder[b] for b in token.encode('utf-8'))
            ids.extend(self.encoder[t] for t in self.bpe(token).split(' '))
        return ids

    def decode(self, ids):
        text = ''.join(self.decoder[int(i)] for i in ids)
        inv = {v: k for k, v in self.byte_encoder.items()}
        return bytearray(inv[c] for c in text).decode('utf-8', errors='replace').replace('</w>', ' ')

    def tokenize(self, texts, context_length=None, truncate=False):
        """str | [str] -> int32 [n, context_length]: <|startoftext|> ids <|endoftext|>, zero padded (clip.tokenize).  A prompt that
        does not fit raises unless `truncate`, which cuts it and keeps the end-of-text token in the last slot."""
        if isinstance(texts, str):
            texts = [texts]
        L = context_length or self.context_length
        out = torch.zeros(len(texts), L, dtype=torch.int32)
        for i, t in enumerate(texts):
            ids = [self.sot] + self.encode(t) + [self.eot]
            if len(ids) > L:
                if not truncate:
                    raise RuntimeError(f'Input {t!r} is too long for context length {L}')
                ids = ids[:L]
                ids[-1] = self.eot
            out[i, :len(ids)] = torch.tensor(ids, dtype=torch.int32)
        return out

    __call__ = tokenize
