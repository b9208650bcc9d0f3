"""CPU: the CLIP text tower's host side - the fp64 restatement (tests/text_ref64.py) pinned to an independent implementation, the
state_dict loader, the BPE tokenizer, the caching TextFeatures and the new C-ABI entries' argument checks (no compute without a GPU)."""
import ctypes
import json
import os

import pytest
import torch

import text_ref64 as TR

VOCAB, WIDTH, HEADS, LAYERS, CONTEXT, EMBED = 96, 128, 2, 2, 77, 64
LENGTHS = (2, 3, 10, 40, 77)


# ---------------------------------------------------------------------------------------------------- the restatement
def _openai_names(hf):
    """state_dict of a transformers CLIPTextModelWithProjection under OpenAI CLIP's names: q / k / v stacked into in_proj_*,
    text_projection.weight ([E, W], an nn.Linear) transposed to CLIP's [W, E] matrix."""
    s = hf.state_dict()
    sd = {'token_embedding.weight': s['text_model.embeddings.token_embedding.weight'],
          'positional_embedding': s['text_model.embeddings.position_embedding.weight'],
          'ln_final.weight': s['text_model.final_layer_norm.weight'], 'ln_final.bias': s['text_model.final_layer_norm.bias'],
          'text_projection': s['text_projection.weight'].T.contiguous()}
    for i in range(LAYERS):
        a, b = f'text_model.encoder.layers.{i}.', f'transformer.resblocks.{i}.'
        for wb in ('weight', 'bias'):
            sd[b + f'attn.in_proj_{wb}'] = torch.cat([s[a + f'self_attn.{p}_proj.{wb}'] for p in 'qkv'], 0)
            for src, dst in (('layer_norm1', 'ln_1'), ('layer_norm2', 'ln_2'), ('self_attn.out_proj', 'attn.out_proj'), ('mlp.fc1', 'mlp.c_fc'),
                             ('mlp.fc2', 'mlp.c_proj')):
                sd[b + f'{dst}.{wb}'] = s[a + f'{src}.{wb}']
    return sd


def test_restatement_equals_an_independent_implementation():
    transformers = pytest.importorskip('transformers', reason='transformers is not installed: no independent CLIP text model to compare with')
    torch.manual_seed(0)
    cfg = transformers.CLIPTextConfig(vocab_size=VOCAB, hidden_size=WIDTH, intermediate_size=4 * WIDTH, projection_dim=EMBED,
                                      num_hidden_layers=LAYERS, num_attention_heads=HEADS, max_position_embeddings=CONTEXT,
                                      hidden_act='quick_gelu', eos_token_id=2, bos_token_id=0, pad_token_id=1)   # eos 2: pools at the arg-max id
    hf = transformers.CLIPTextModelWithProjection(cfg).double().eval()
    with torch.no_grad():
        for p in hf.parameters():            # biases and LayerNorm affines start at 0 / 1: make every one of them count
            p.add_(torch.randn_like(p) * 0.05)
        ids = TR.random_prompts(LENGTHS, VOCAB, CONTEXT)
        want = hf(input_ids=ids.long()).text_embeds
        sd = _openai_names(hf)
        got = TR.encode(sd, ids, HEADS, normalize=False)
        got_sdpa = TR.encode(sd, ids, HEADS, normalize=False, sdpa=True)
        unit = TR.encode(sd, ids, HEADS, normalize=True)
    assert want.shape == (len(LENGTHS), EMBED) and want.dtype == torch.float64
    scale = float(want.abs().max())
    assert float((got - want).abs().max()) <= 1e-12 * scale, float((got - want).abs().max()) / scale
    assert float((got_sdpa - want).abs().max()) <= 1e-12 * scale
    assert float((unit - want / want.norm(dim=-1, keepdim=True)).abs().max()) <= 1e-12


# ---------------------------------------------------------------------------------------------------- from_state_dict
def test_from_state_dict_infers_the_geometry_and_ignores_the_image_tower():
    from tamtr_amd.text import ClipTextEncoder
    sd = TR.random_state(VOCAB, WIDTH, LAYERS, CONTEXT, EMBED, dtype=torch.float16)
    full = dict(sd)
    full.update({'visual.conv1.weight': torch.zeros(8, 3, 4, 4, dtype=torch.float16), 'visual.transformer.resblocks.0.ln_1.weight': torch.zeros(8),
                 'visual.transformer.resblocks.7.ln_1.weight': torch.zeros(8), 'logit_scale': torch.tensor(4.6), 'context_length': torch.tensor(77)})
    enc = ClipTextEncoder.from_state_dict(full)
    assert (enc.vocab_size, enc.width, enc.layers, enc.context_length, enc.embed_dim, enc.heads) == (VOCAB, WIDTH, LAYERS, CONTEXT, EMBED, WIDTH // 64)
    own = enc.state_dict()
    assert sorted(own) == sorted(sd), 'parameter names differ from OpenAI CLIP\'s'
    for k, v in own.items():
        assert v.dtype == torch.float32 and torch.equal(v, sd[k].float()), k
    assert not any(p.requires_grad for p in enc.parameters())
    enc.load_state_dict({k: v.float() for k, v in sd.items()})     # a text-only CLIP state_dict loads unchanged, strictly


def test_from_state_dict_names_the_missing_tensor():
    from tamtr_amd.text import ClipTextEncoder
    sd = TR.random_state(VOCAB, WIDTH, LAYERS, CONTEXT, EMBED, dtype=torch.float32)
    cut = {k: v for k, v in sd.items() if not k.startswith('transformer.resblocks.0.')}
    with pytest.raises(KeyError, match=r'transformer\.resblocks\.0\.ln_1\.weight'):
        ClipTextEncoder.from_state_dict(cut)
    with pytest.raises(KeyError, match='text_projection'):
        ClipTextEncoder.from_state_dict({k: v for k, v in sd.items() if k != 'text_projection'})


def test_encoder_on_the_cpu_is_refused():
    from tamtr_amd import TamtrHipError
    from tamtr_amd.text import ClipTextEncoder
    enc = ClipTextEncoder(VOCAB, WIDTH, LAYERS, CONTEXT, EMBED)
    with pytest.raises(TamtrHipError):
        enc.encode_tokens(TR.random_prompts((3,), VOCAB, CONTEXT))


# ---------------------------------------------------------------------------------------------------- tokenizer
# Vocabulary order (CLIP's): ids 0..255 the byte characters - printable ASCII '!'..'~' first, so chr(c) has id c - 33 ('a' = 64, 'c' = 66,
# 'e' = 68, 'n' = 77, 'o' = 78, 's' = 82, 't' = 83) - ids 256..511 the same with </w> (id + 256), merge k has id 512 + k, then
# <|startoftext|> = 522 and <|endoftext|> = 523.
MERGES = ['c a',        # 512 ca
          'ca t</w>',   # 513 cat</w>
          'd o',        # 514 do
          'do g</w>',   # 515 dog</w>
          't h',        # 516 th
          'th e</w>',   # 517 the</w>
          'r e',        # 518 re
          're d</w>',   # 519 red</w>
          'o n',        # 520 on
          'c o']        # 521 co
SOT, EOT = 522, 523
PROMPTS = {
    # a -> a</w> = 64 + 256;  cat = c a t</w> -> ca t</w> -> cat</w> = 513
    'a cat': [320, 513],
    # the = t h e</w> -> th e</w> -> the</w> 517;  red -> re d</w> -> red</w> 519;  dog -> do g</w> -> dog</w> 515
    'the red dog': [517, 519, 515],
    # cats = c a t s</w> -> ca t s</w>: (ca, t) is no merge (merge 1 needs t</w>) -> ca 512, t 83, s</w> 82 + 256
    # on = o n</w>: (o, n</w>) is no merge (merge 8 is o n) -> o 78, n</w> 77 + 256
    # cone = c o n e</w>: (o, n) has rank 8, (c, o) rank 9 -> the lower rank first: c on e</w> -> c 66, on 520, e</w> 68 + 256
    'cats on cone': [512, 83, 338, 78, 333, 66, 520, 324],
}


@pytest.fixture()
def tokenizer(tmp_path):
    from tamtr_amd.text import SimpleTokenizer
    path = tmp_path / 'merges.txt'
    path.write_text('#version: 0.2\n' + '\n'.join(MERGES) + '\n', encoding='utf-8')
    return SimpleTokenizer(str(path))


def test_tokenizer_ids_derived_by_hand(tokenizer, tmp_path):
    assert (tokenizer.vocab_size, tokenizer.sot, tokenizer.eot) == (524, SOT, EOT)
    for text, want in PROMPTS.items():
        assert tokenizer.encode(text) == want, text
    assert tokenizer.encode('  A   CAT \n') == PROMPTS['a cat']                    # lower-casing, whitespace collapse
    assert tokenizer.encode('the&amp;') == [517, ord('&') - 33 + 256]              # HTML entities are unescaped
    assert tokenizer.decode(PROMPTS['the red dog']).strip() == 'the red dog'
    ids = tokenizer(list(PROMPTS))
    assert ids.dtype == torch.int32 and ids.shape == (3, 77)
    for row, want in zip(ids, PROMPTS.values()):
        n = len(want) + 2
        assert row[:n].tolist() == [SOT] + want + [EOT] and not row[n:].any()     # SOT / EOT placement, zero padding
        assert int(row.argmax()) == n - 1
    assert tokenizer('a cat', context_length=4).tolist() == [[SOT, 320, 513, EOT]]
    # a gzip file reads the same
    import gzip
    from tamtr_amd.text import SimpleTokenizer
    gz = tmp_path / 'merges.txt.gz'
    with gzip.open(gz, 'wb') as f:
        f.write(('#version: 0.2\n' + '\n'.join(MERGES) + '\n').encode())
    assert SimpleTokenizer(str(gz)).encode('cats on cone') == PROMPTS['cats on cone']


def test_tokenizer_overflow_and_truncation(tokenizer):
    long = ' '.join(['cat'] * 100)
    with pytest.raises(RuntimeError, match='too long'):
        tokenizer(long)
    row = tokenizer(long, truncate=True)[0]
    assert row.tolist() == [SOT] + [513] * 75 + [EOT]
    assert int(row[-1]) == EOT and int(row.argmax()) == 76
    with pytest.raises(RuntimeError):
        tokenizer('the red dog', context_length=4)
    assert tokenizer('the red dog', context_length=4, truncate=True).tolist() == [[SOT, 517, 519, EOT]]


def test_tokenizer_agrees_with_transformers(tokenizer, tmp_path):
    transformers = pytest.importorskip('transformers', reason='transformers is not installed')
    (tmp_path / 'vocab.json').write_text(json.dumps(tokenizer.encoder), encoding='utf-8')
    (tmp_path / 'hf_merges.txt').write_text('#version: 0.2\n' + '\n'.join(MERGES) + '\n', encoding='utf-8')
    try:
        hf = transformers.CLIPTokenizer(str(tmp_path / 'vocab.json'), str(tmp_path / 'hf_merges.txt'))
    except Exception as e:   # noqa: BLE001 - a transformers build that cannot make the slow tokenizer from files
        pytest.skip(f'transformers.CLIPTokenizer cannot be built from a merges file here: {e!r}')
    for text in list(PROMPTS) + ['  A   CAT \n', "the dog's red cone, on 42 cats!"]:
        assert hf(text)['input_ids'] == [SOT] + tokenizer.encode(text) + [EOT], text


# ---------------------------------------------------------------------------------------------------- TextFeatures.from_encoder
class _StubEncoder:
    """Counts what it is asked to encode; the feature of a prompt is a fixed function of its ids."""
    embed_dim = 8

    def __init__(self):
        self.calls, self.rows = 0, 0

    def encode_tokens(self, ids, normalize=True):
        assert normalize
        self.calls += 1
        self.rows += ids.shape[0]
        f = torch.stack([torch.cos(ids.float().sum(-1) * (k + 1)) for k in range(self.embed_dim)], -1) + 0.1
        return f / f.norm(dim=-1, keepdim=True)


def test_text_features_from_encoder_encodes_each_prompt_once(tokenizer):
    from tamtr_amd.data import TextFeatures
    enc = _StubEncoder()
    tf = TextFeatures.from_encoder(enc, tokenizer)
    a = tf.encode(['the red dog', 'a cat', 'the red dog'])
    assert (enc.calls, enc.rows) == (1, 2)                       # two distinct prompts, one batch
    b = tf.encode(['a cat', 'cats on cone', 'the red dog'])
    assert (enc.calls, enc.rows) == (2, 3)                       # only the new prompt
    tf.encode(['a cat', 'the red dog'])
    assert (enc.calls, enc.rows) == (2, 3)
    assert a.shape == (3, 8) and b.shape == (3, 8) and a.dtype == torch.float32
    assert torch.allclose(a.norm(dim=-1), torch.ones(3), atol=1e-6) and torch.allclose(b.norm(dim=-1), torch.ones(3), atol=1e-6)
    assert torch.equal(a[0], a[2]) and torch.equal(a[0], b[2]) and torch.equal(a[1], b[0])       # the order follows the request
    want = enc.encode_tokens(tokenizer(['cats on cone']))[0]
    assert torch.allclose(b[1], want, atol=1e-6)
    # the table-only forms keep their behaviour
    with pytest.raises(KeyError):
        TextFeatures({'x': torch.ones(4)}).encode(['y'])
    with pytest.raises(ValueError):
        TextFeatures.from_args(None, None, None, 'cpu')
    with pytest.raises(ValueError):
        TextFeatures.from_args('feats.npz', 'clip.pt', 'vocab.gz', 'cpu')


# ---------------------------------------------------------------------------------------------------- C ABI
def test_new_symbols_are_exported_and_the_abi_version_stays():
    import tamtr_amd
    from tamtr_amd import _lib
    if not os.path.exists(tamtr_amd.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    h = ctypes.CDLL(tamtr_amd.LIB_PATH)
    for n in ('tamtr_text_embed', 'tamtr_linear_f32', 'tamtr_text_pool_project'):
        assert hasattr(h, n) and n in _lib.EXPORTS, n
    assert _lib.ABI_VERSION == 36 and _lib.lib().tamtr_abi_version() == 36


def test_text_entries_reject_bad_arguments_without_a_gpu():
    from tamtr_amd import _lib
    h = _lib.lib()
    z = ctypes.c_void_p(0)
    one = ctypes.c_void_p(16)   # a non-null, 16-byte aligned address that is never dereferenced: the checks come first
    assert h.tamtr_linear_f32(z, z, z, z, z, 77, 64, 32, 0, z) == -1
    assert h.tamtr_linear_f32(one, one, one, z, z, 77, 64, 32, 0, z) == -1          # no output
    assert h.tamtr_linear_f32(one, one, one, z, one, 77, 64, 32, 2, z) == -1        # residual epilogue without a residual
    assert h.tamtr_linear_f32(one, one, one, z, one, 77, 64, 32, 3, z) == -1        # no such epilogue
    assert h.tamtr_linear_f32(one, one, one, z, one, 0, 64, 32, 0, z) == -1         # M < 1
    assert h.tamtr_linear_f32(one, one, one, z, one, 77, 64, 48, 0, z) == -2        # K % 32
    assert h.tamtr_linear_f32(one, one, one, z, one, 77, 96, 32, 0, z) == -2        # N % 64
    assert h.tamtr_text_embed(z, z, z, z, 1, 77, 128, 96, z) == -1
    assert h.tamtr_text_embed(one, one, one, one, 1, 77, 128, 0, z) == -1           # empty vocabulary
    assert h.tamtr_text_embed(one, one, one, one, 1, 77, 126, 96, z) == -2          # W % 4
    assert h.tamtr_text_pool_project(z, z, z, z, z, z, 1, 77, 128, 64, 1e-5, 1, z) == -1
    assert h.tamtr_text_pool_project(one, one, one, one, one, one, 1, 77, 2048, 64, 1e-5, 1, z) == -2   # W > 1024
    assert h.tamtr_text_pool_project(one, one, one, one, one, one, 1, 77, 128, 2048, 1e-5, 1, z) == -2   # E > 1024


def test_ops_refuse_cpu_tensors():
    import tamtr_amd.ops as ops
    from tamtr_amd import TamtrHipError
    with pytest.raises(TamtrHipError):
        ops.linear_f32(torch.zeros(3, 32), torch.zeros(64, 32), torch.zeros(64))
    with pytest.raises(TamtrHipError):
        ops.text_embed(torch.zeros(1, 4, dtype=torch.int32), torch.zeros(8, 32), torch.zeros(4, 32))
    with pytest.raises(TamtrHipError):
        ops.text_pool_project(torch.zeros(4, 32), torch.zeros(1, 4, dtype=torch.int32), torch.ones(32), torch.zeros(32), torch.zeros(32, 64))
