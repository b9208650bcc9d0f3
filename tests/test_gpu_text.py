"""GPU: the CLIP text tower (csrc/text.hip, tam-tr_amd/text.py) against the fp64 restatement of tests/text_ref64.py.

Kernel by kernel the assertion is ref64.check's |got - ref| <= b mag with b = fp32_b(chain length + c) and no free absolute term; the
whole encoder, whose 12 residual blocks have no tight a-priori bound, is held to 4 x the error of an independent fp32 evaluation (the same
restatement run by torch in fp32 on the GPU)."""
import os
import sys

import pytest
import torch

import ref64 as R
import text_ref64 as TR
from conftest import ROOT

pytestmark = pytest.mark.gpu

LENGTHS = (2, 3, 10, 40, 77)
TINY = dict(vocab=96, width=128, layers=2, context=77, embed=64)       # 2 heads of 64
VITB32 = dict(vocab=49408, width=512, layers=12, context=77, embed=512)  # 8 heads of 64


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import tamtr_amd.ops as ops
    return ops


def dev(t):
    return t.detach().float().cuda().contiguous()


def rnd64(shape, seed, std=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * std


def f32(t):
    """An fp32 operand as the kernel sees it, in fp64 for the reference."""
    return t.float().double()


# ---------------------------------------------------------------------------------------------------- linear_f32
MS = (1, 63, 77, 154, 385)   # below a tile, one off a tile edge, one prompt, two, five
NK = [(64, 32), (128, 128), (384, 128), (512, 128), (128, 512), (1536, 512), (512, 2048)]
# c: roundings of a result beyond the K fused multiply-adds of its chain.
#   none / residual: the bias add and the residual add -> 2.
#   QuickGELU y / (1 + exp(-1.702 y)): the product 1.702 y, expf (its error, at most 2 ulp, enters the quotient scaled by
#   exp / (1 + exp) < 1), the add, the division, and y's own error passed on by the slope of y sigmoid(1.702 y), which is at most 1.1: the
#   0.1 excess over the K + 1 of y is worth 0.1 (K + 1) more roundings only if every one of the K roundings of the chain has the same sign;
#   2 + 1 + 1 + 1 = 5 in the epilogue, 8 with that slack.
C_EPI = {'none': 2, 'residual': 2, 'residual_alias': 2, 'quick_gelu': 8}
SENTINEL = 12345.0


@pytest.mark.parametrize('N,K', NK)
def test_linear_f32_vs_fp64(ops, N, K):
    Mx = max(MS)
    x, w, b, res = f32(rnd64((Mx, K), 1)), f32(rnd64((N, K), 2, K ** -0.5)), f32(rnd64((N,), 3, 0.5)), f32(rnd64((Mx, N), 4))
    ref = {'none': TR.linear(x, w, b), 'quick_gelu': TR.linear(x, w, b, act='quick_gelu'), 'residual': TR.linear(x, w, b, residual=res)}
    ref['residual_alias'] = ref['residual']
    xd, wd, bd, rd = dev(x), dev(w), dev(b), dev(res)
    for M in MS:
        for epi, c in C_EPI.items():
            def run():
                buf = torch.full((M + 3, N), SENTINEL, device='cuda')     # over-allocated: rows >= M must stay as they are
                out = buf[:M]
                if epi == 'residual_alias':
                    out.copy_(rd[:M])
                    got = ops.linear_f32(xd[:M], wd, bd, residual=out, out=out)
                else:
                    got = ops.linear_f32(xd[:M], wd, bd, act='quick_gelu' if epi == 'quick_gelu' else None,
                                         residual=rd[:M] if epi == 'residual' else None, out=out)
                assert got.data_ptr() == buf.data_ptr()
                return buf
            buf, again = run(), run()
            assert bool((buf[M:] == SENTINEL).all()), f'M={M} {epi}: rows beyond M were written'
            assert torch.equal(buf, again), f'M={M} {epi}: two runs differ'
            val, mag = ref[epi]
            worst = R.check(f'linear_f32[{N}x{K} M={M} {epi}]', buf[:M], val[:M], mag[:M], 0, R.fp32_b(K + c))
            print(f'linear_f32 N={N} K={K} M={M} {epi}: err / bound = {worst:.3f}')
    fresh = ops.linear_f32(xd, wd, bd)                                    # without `out`: a new [M, N] tensor
    assert fresh.shape == (Mx, N) and torch.equal(fresh, ops.linear_f32(xd, wd, bd, out=torch.empty(Mx, N, device='cuda')))


def test_linear_f32_refusals(ops):
    from tamtr_amd import TamtrHipError
    x, w, b = torch.zeros(5, 64, device='cuda'), torch.zeros(64, 64, device='cuda'), torch.zeros(64, device='cuda')
    for bad in (lambda: ops.linear_f32(x.cpu(), w, b), lambda: ops.linear_f32(x, w.cpu(), b), lambda: ops.linear_f32(x.double(), w, b),
                lambda: ops.linear_f32(x.t().contiguous().t(), w, b), lambda: ops.linear_f32(x, w, b, act='gelu'),
                lambda: ops.linear_f32(x, w, b, act='quick_gelu', residual=torch.zeros(5, 64, device='cuda')),
                lambda: ops.linear_f32(x[:, :48].contiguous(), w[:, :48].contiguous(), b),          # K % 32
                lambda: ops.linear_f32(x, torch.zeros(96, 64, device='cuda'), torch.zeros(96, device='cuda')),   # N % 64
                lambda: ops.linear_f32(x, w, b, out=x)):
        with pytest.raises(TamtrHipError):
            bad()


# ---------------------------------------------------------------------------------------------------- text_embed
@pytest.mark.parametrize('n,L,W,V', [(5, 77, 128, 96), (3, 5, 36, 7), (300, 77, 128, 96)])
def test_text_embed_is_bit_exact(ops, n, L, W, V):
    tok, pos = dev(rnd64((V, W), 1, 0.02)), dev(rnd64((L + 2, W), 2, 0.01))
    ids = torch.randint(0, V, (n, L), generator=torch.Generator().manual_seed(3), dtype=torch.int32).cuda()
    ids[0, 0], ids[-1, -1] = 0, V - 1
    got = ops.text_embed(ids, tok, pos)
    assert got.shape == (n * L, W) and torch.equal(got, (tok[ids.long()] + pos[:L]).reshape(n * L, W))     # one fp32 add


def test_text_embed_refusals(ops):
    from tamtr_amd import TamtrHipError
    tok, pos = torch.zeros(96, 128, device='cuda'), torch.zeros(77, 128, device='cuda')
    ids = torch.zeros(2, 77, dtype=torch.int32, device='cuda')
    with pytest.raises(TamtrHipError):
        ops.text_embed(ids.cpu(), tok, pos)
    with pytest.raises(TamtrHipError):
        ops.text_embed(ids.long(), tok, pos)
    for bad in (96, 1000, -1):                       # refused on the host, before any launch
        ids2 = ids.clone()
        ids2[1, 5] = bad
        with pytest.raises(TamtrHipError, match='vocabulary'):
            ops.text_embed(ids2, tok, pos)
    with pytest.raises(TamtrHipError, match='positional_embedding'):
        ops.text_embed(torch.zeros(2, 78, dtype=torch.int32, device='cuda'), tok, pos)


# ---------------------------------------------------------------------------------------------------- text_pool_project
@pytest.mark.parametrize('W,E', [(128, 64), (512, 512), (64, 320)])
@pytest.mark.parametrize('normalize', [True, False])
def test_text_pool_project_vs_fp64(ops, W, E, normalize):
    n, L, V = 6, 77, 96
    ids = TR.random_prompts(LENGTHS + (20,), V, L)
    ids[5, 7] = V - 1                      # the maximum id twice (positions 7 and 19): the first must win
    assert int(ids[5].long().argmax()) == 7 and int((ids[5] == V - 1).sum()) == 2
    x, g, b, proj = f32(rnd64((n, L, W), 1) + 0.3), f32(1 + rnd64((W,), 2, 0.1)), f32(rnd64((W,), 3, 0.1)), f32(rnd64((W, E), 4, W ** -0.5))
    val, mag = TR.pool_project(x, ids, g, b, proj, 1e-5, normalize)
    got = ops.text_pool_project(dev(x).view(n * L, W), ids.cuda(), dev(g), dev(b), dev(proj), 1e-5, normalize)
    # chain: mean and variance over W, the W products of the projection, the E squares of the norm; c = 8: rsqrt, the affine's
    # three operations, the division by W twice, square root and division of the normalisation
    worst = R.check(f'text_pool_project[{W}x{E} norm={normalize}]', got, val, mag, 0, R.fp32_b(W + E + 8))
    print(f'text_pool_project W={W} E={E} normalize={normalize}: err / bound = {worst:.3f}')
    if normalize:
        assert float((got.double().norm(dim=-1) - 1).abs().max()) < 1e-6


# ---------------------------------------------------------------------------------------------------- causal attention (existing kernel)
def test_causal_attention_through_the_existing_kernel(ops):
    n, L, nh, dh = 2, 77, 2, 64
    W = nh * dh
    qkv = f32(rnd64((n, L, 3 * W), 1))
    bits = ops.mask_words(torch.ones(L, L, dtype=torch.bool, device='cuda').triu_(1))
    assert bits.shape == (L, 3) and bits.dtype == torch.int32

    def run(p):
        p = dev(p)
        return ops.self_attention_packed(p[..., :W], p[..., W:2 * W], p[..., 2 * W:], nh, bits)      # views with ld = 3 W
    out = run(qkv)
    for i in (0, 30, 63, 75):               # tokens after i replaced: outputs up to i keep their bits
        other = qkv.clone()
        other[:, i + 1:] = f32(rnd64((n, L - i - 1, 3 * W), 2 + i, 3.0))
        out2 = run(other)
        assert torch.equal(out2[:, :i + 1], out[:, :i + 1]), f'position <= {i} saw a later token'
        assert not torch.equal(out2[:, i + 1:], out[:, i + 1:])
    mask = torch.ones(L, L, dtype=torch.bool).triu_(1)
    q, k, v = qkv[..., :W], qkv[..., W:2 * W], qkv[..., 2 * W:]
    val, mag = R.attention(q, k, v, nh, mask, torch.zeros(n, L, W))['o']
    S = float(torch.einsum('bihc,bjhc->bhij', q.reshape(n, L, nh, dh).abs(), k.reshape(n, L, nh, dh).abs()).max()) * dh ** -0.5
    worst = R.check('causal attention o', out, val, mag, 0, R.fp32_b(2 * 64 * S + 2 * L + 64))      # tests/test_gpu_bf16_kernels.py's fp32 term
    print(f'causal attention: err / bound = {worst:.3f}')
    assert torch.allclose(out.cpu().double(), TR.attention(qkv, nh), atol=1e-5)                   # and the restatement's own attention


# ---------------------------------------------------------------------------------------------------- the whole encoder
def _encoder(geo, sd):
    from tamtr_amd.text import ClipTextEncoder
    enc = ClipTextEncoder.from_state_dict({k: v.float() for k, v in sd.items()}).cuda()
    assert (enc.width, enc.layers, enc.embed_dim, enc.heads) == (geo['width'], geo['layers'], geo['embed'], geo['width'] // 64)
    return enc


def _prompts(n, geo):
    return TR.random_prompts([LENGTHS[i % len(LENGTHS)] for i in range(n)], geo['vocab'], geo['context'], seed=n)


def _figures(a, ref):
    """max |a - ref| / (|ref| + rms(ref)) over elements, and 1 - cos per prompt, in fp64."""
    a, ref = a.detach().cpu().double(), ref.double()
    e = float(((a - ref).abs() / (ref.abs() + ref.pow(2).mean().sqrt())).max())
    return e, 1 - torch.nn.functional.cosine_similarity(a, ref, dim=-1)


@pytest.mark.parametrize('name,geo,n', [('tiny', TINY, 5), ('tiny', TINY, 300), ('vitb32', VITB32, 4)])   # 300 crosses the 256-prompt chunk
@pytest.mark.parametrize('normalize', [True])
def test_encoder_is_as_good_as_an_independent_fp32_evaluation(ops, name, geo, n, normalize):
    sd32 = {k: v.float() for k, v in TR.random_state(**geo, seed=7).items()}      # the fp32 weights every path sees
    ids = _prompts(n, geo)
    heads = geo['width'] // 64
    with torch.no_grad():
        ref = TR.encode({k: v.double() for k, v in sd32.items()}, ids, heads, normalize)
        lib = TR.encode({k: v.cuda() for k, v in sd32.items()}, ids.cuda(), heads, normalize, sdpa=True)      # library GEMMs + SDPA, fp32
    assert lib.dtype == torch.float32
    own = _encoder(geo, sd32).encode_tokens(ids, normalize=normalize)
    assert own.shape == (n, geo['embed']) and own.dtype == torch.float32 and own.is_cuda
    (e_own, c_own), (e_lib, c_lib) = _figures(own, ref), _figures(lib, ref)
    print(f'encoder[{name} n={n}]: e_own {e_own:.3e}  e_torch {e_lib:.3e}  max(1-cos) own {float(c_own.max()):.3e}  torch {float(c_lib.max()):.3e}')
    assert e_own <= 4 * e_lib, f'own path {e_own:.3e} vs torch fp32 {e_lib:.3e}'
    assert bool((c_own <= 4 * c_lib + 2.0 ** -22).all()), f'1 - cos: own {c_own.tolist()} torch {c_lib.tolist()}'
    if n > 256:   # a prompt gives the same bits whichever chunk it falls in
        enc = _encoder(geo, sd32)
        assert torch.equal(enc.encode_tokens(ids[250:262], normalize=normalize), own[250:262])


def test_padding_has_no_influence(ops):
    sd = TR.random_state(**TINY, seed=7)
    enc = _encoder(TINY, sd)
    ids = _prompts(10, TINY)
    eot = TINY['vocab'] - 1
    other = ids.clone()
    fill = torch.randint(0, eot, ids.shape, generator=torch.Generator().manual_seed(5), dtype=torch.int32)
    after = torch.arange(ids.shape[1])[None] > ids.long().argmax(-1, keepdim=True)
    other[after] = fill[after]
    assert int(after.sum()) > 0 and not torch.equal(other, ids) and torch.equal(other.long().argmax(-1), ids.long().argmax(-1))
    for normalize in (True, False):
        assert torch.equal(enc.encode_tokens(other, normalize=normalize), enc.encode_tokens(ids, normalize=normalize))


def test_encoder_refusals(ops):
    from tamtr_amd import TamtrHipError
    from tamtr_amd.text import ClipTextEncoder
    enc = ClipTextEncoder(96, 128, 1, 77, 64).cuda()
    ids = _prompts(2, TINY)
    assert enc.encode_tokens(ids).shape == (2, 64) and enc.encode_tokens(ids[:, :40].clone()).shape == (2, 64)     # a shorter context is fine
    with pytest.raises(TamtrHipError, match='positional_embedding'):
        enc.encode_tokens(torch.zeros(2, 78, dtype=torch.int32))
    bad = ids.clone()
    bad[0, 1] = 96
    with pytest.raises(TamtrHipError, match='vocabulary'):
        enc.encode_tokens(bad)
    with pytest.raises(TamtrHipError):
        ClipTextEncoder(96, 128, 1, 77, 64).encode_tokens(ids)             # a CPU module
    with pytest.raises(TamtrHipError):
        enc.encode_tokens(ids.float())


# ---------------------------------------------------------------------------------------------------- set_classes
class _Deterministic:
    """MIOpen on its deterministic solvers + the NCHW trunk (what TAMTR_DETERMINISTIC=1 selects, tuning.use_deterministic_convolutions) for
    the body of a `with`.  MIOpen's default solver set sums with float atomics / split-K in a run-dependent order: two evaluation forwards
    on the SAME model state then differ in the last bit (measured on an MI355X at 128 x 128, fp32: max |a - again| = 1.8e-7), so logits
    of two forwards can be compared bit for bit only in the package's reproducible mode."""

    def __init__(self, model):
        self.model = model

    def __enter__(self):
        from tamtr_amd import tuning
        self.keep = (torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark, torch.are_deterministic_algorithms_enabled(),
                     torch.is_deterministic_algorithms_warn_only_enabled(), os.environ.get('MIOPEN_DEBUG_CONVOLUTION_DETERMINISTIC'))
        tuning.use_deterministic_convolutions()
        self.model.set_channels_last(False)
        return self

    def __exit__(self, *exc):
        self.model.set_channels_last(True)
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = self.keep[0], self.keep[1]
        torch.use_deterministic_algorithms(self.keep[2], warn_only=self.keep[3])
        if self.keep[4] is None:
            os.environ.pop('MIOPEN_DEBUG_CONVOLUTION_DETERMINISTIC', None)
        else:
            os.environ['MIOPEN_DEBUG_CONVOLUTION_DETERMINISTIC'] = self.keep[4]
        return False


@pytest.fixture(scope='module')
def set_classes_run(ops, tmp_path_factory):
    """A tiny model (128 x 128, one image, fp32, eval) with its vocabulary set three ways; every forward in the reproducible mode."""
    sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
    from weights import fill_state, urnd
    from tamtr_amd.model import RTDETRDetectionWorldModel
    from tamtr_amd.text import ClipTextEncoder, SimpleTokenizer
    merges = tmp_path_factory.mktemp('bpe') / 'merges.txt'
    merges.write_text('#version: 0.2\nc a\nca t</w>\nd o\ndo g</w>\n', encoding='utf-8')
    tok = SimpleTokenizer(str(merges))
    torch.manual_seed(0)
    enc = ClipTextEncoder(tok.vocab_size, 128, 1, 77, 512).cuda()
    model = RTDETRDetectionWorldModel(nc=10)
    model.load_state_dict(fill_state(model.state_dict(), 78))
    model.cuda().eval()
    img = urnd((1, 3, 128, 128), 1).cuda()
    first = lambda y: y[0] if isinstance(y, (tuple, list)) else y   # noqa: E731
    with torch.no_grad(), _Deterministic(model):
        model.set_classes(['cat/kitten', 'dog', 'a cat and a dog'], enc, tok)      # of `a/b` the first synonym
        assert model.txt_feats.shape == (1, 3, 512) and model.model[-1].nc == 3
        fa = model.txt_feats.clone()
        a, again = first(model(img)), first(model(img))
        model.set_text_features(enc.encode_tokens(tok(['cat', 'dog', 'a cat and a dog'])))
        fb = model.txt_feats.clone()
        b = first(model(img))
        model.set_classes({0: 'dog', 1: 'cat'}, enc, tok)
        c = first(model(img))
        model.set_text_features(enc.encode_tokens(tok(['dog', 'cat', 'a cat and a dog'])))     # another vocabulary of three
        d = first(model(img))
    return dict(fa=fa, fb=fb, a=a, again=again, b=b, c=c, d=d)


def test_set_classes_sets_the_features_of_encode_tokens(set_classes_run):
    """What set_classes hands the model is, bit for bit, set_text_features(encoder.encode_tokens(tokenizer(names))); the class count
    follows the names."""
    r = set_classes_run
    assert torch.equal(r['fa'], r['fb']) and float((r['fa'].norm(dim=-1) - 1).abs().max()) < 1e-6
    assert r['a'].shape[-1] == 4 + 3 and r['b'].shape[-1] == 4 + 3 and r['c'].shape[-1] == 4 + 2
    assert bool(torch.isfinite(r['a']).all())


def test_set_classes_logits_equal_bit_for_bit(set_classes_run):
    """The logits after set_classes equal, bit for bit, those after set_text_features(encoder.encode_tokens(tokenizer(names))), and the
    vocabulary reaches them: the same names in another order give other logits."""
    r = set_classes_run
    print('set_classes: max |a - b|', float((r['a'] - r['b']).abs().max()), ' two forwards on the same model state: max |a - again|',
          float((r['a'] - r['again']).abs().max()), ' another vocabulary: max |a - d|', float((r['a'] - r['d']).abs().max()))
    assert torch.equal(r['a'], r['again']), 'the reproducible mode is not reproducible: the comparison below would say nothing'
    assert torch.equal(r['a'], r['b'])
    assert not torch.equal(r['a'], r['d'])
