"""The cases, the inputs and the assertions of the loss, matcher-cost, box-refinement and optimizer checks against fp64 (tests/ref64.py
detr_terms, detr_match_cost, box_refine, optim_step).  tests/test_gpu_loss_ref64.py feeds the assertions the kernels' outputs
(csrc/detrloss.hip, csrc/optim.hip); tests/test_ref64_host.py feeds them the fp32 torch form of tam-tr_amd/loss.py and torch's own
optimizer on the CPU, which must meet every bound at a ratio of at most 0.5, and mistaken references, which must not.

Boxes live on a grid: centres are multiples of U = 2^-10, sizes multiples of 2 U and at least 4 U = 2^-8.  Then every edge x +- w / 2 and
every difference of edges is exact in fp32, so fp32 and fp64 take the same branch of every min / max / clamp, ties included.  Every
assertion is ref64.check(): |got - ref| <= b mag (a = 0: everything is fp32), b counted in ref64.detr_bounds / optim_bounds."""
import math

import torch

import ref64 as R

U = 2.0 ** -10
GAINS_LOSS = (1, 5, 2)             # DETRLoss.loss_gain: class, bbox, giou
GAINS_COST = (2, 5, 2)             # the matcher's cost_gain
ALPHA, GAMMA = 0.25, 2.0


def _ok(b):
    x, y, w, h = b
    assert all(int(v) == v for v in b) and w % 2 == 0 and h % 2 == 0 and w >= 4 and h >= 4, b
    return b


# family -> [(prediction, box)], xywh in units of U.  The comment states what the pair has, as edges (x1, x2 | y1, y2).
FAMILIES = {
    'overlap': [((500, 480, 200, 120), (540, 500, 160, 180)), ((300, 620, 90, 260), (280, 600, 140, 200)), ((700, 300, 320, 64), (660, 310, 200, 100))],
    'disjoint_x': [((200, 500, 100, 200), (700, 520, 120, 160)), ((800, 400, 60, 90), (300, 410, 100, 50))],
    'disjoint_y': [((500, 200, 200, 100), (520, 700, 160, 120)), ((400, 800, 90, 60), (410, 300, 50, 100))],
    'disjoint_xy': [((200, 200, 100, 120), (700, 720, 140, 90)), ((800, 150, 60, 40), (100, 900, 80, 120))],
    'touching': [((300, 500, 200, 180), (500, 520, 200, 160)),       # ax2 = bx1 = 400
                 ((500, 300, 180, 200), (520, 500, 160, 200)),       # ay2 = by1 = 400
                 ((700, 500, 200, 180), (500, 520, 200, 160))],      # ax1 = bx2 = 600
    'tie_left': [((400, 500, 200, 100), (420, 540, 240, 140))],      # ax1 = bx1 = 300
    'tie_right': [((400, 500, 200, 100), (380, 540, 240, 140))],     # ax2 = bx2 = 500
    'tie_top': [((500, 400, 100, 200), (540, 420, 140, 240))],       # ay1 = by1 = 300
    'tie_bottom': [((500, 400, 100, 200), (540, 380, 140, 240))],    # ay2 = by2 = 500
    # both x edges and the top edge tie; the fourth edge cannot tie too without the centres coinciding (that is same_centre)
    'tie_all_but_centre': [((400, 500, 200, 100), (400, 520, 200, 140)),      # x: 300, 500 both; ay1 = by1 = 450
                           ((500, 400, 100, 200), (520, 400, 140, 200))],     # y: 300, 500 both; ax1 = bx1 = 450
    'contained': [((500, 500, 100, 60), (520, 510, 300, 200))],
    'containing': [((520, 510, 300, 200), (500, 500, 100, 60))],
    'square_pred': [((500, 480, 160, 160), (540, 500, 120, 200)), ((300, 300, 64, 64), (310, 290, 64, 64))],
    'thin': [((500, 500, 4, 512), (510, 520, 100, 300))],            # aspect 2^-8 : 0.5
    'tall': [((500, 500, 512, 4), (520, 502, 300, 100))],            # and the reverse
    'same_centre': [((500, 500, 200, 100), (500, 500, 120, 160))],   # the NaN row
    'tiny': [((500, 500, 4, 4), (502, 501, 4, 4)), ((300, 300, 4, 6), (302, 302, 6, 4))],
    'identical_shape_shifted': [((500, 500, 200, 100), (530, 480, 200, 100))],   # v = 0, alpha = 0
}
GENERIC = ('overlap', 'contained', 'containing', 'identical_shape_shifted')      # no tie, no closed clamp, no NaN: every form of the formulas agrees
PAIRS = [(f, _ok(a), _ok(b)) for f, ps_ in FAMILIES.items() for a, b in ps_]

# (Lr, B, nq, nc, counts): the smallest shapes that cross every boundary of the launch geometry.  Class kernels and the partial-sum table:
# 256 rows per workgroup, B nq = 255, 256, 257, 513.  Pair kernels: 256 pairs per workgroup, Lr n = 1, 255, 257, 260.  n = 1, G = 1, nc = 1, 7,
# 80, Lr = 1, 4, ragged counts with an image without boxes.
SHAPES = [(1, 1, 255, 1, [1]), (1, 1, 256, 7, [255]), (1, 1, 257, 7, [257]), (4, 3, 171, 80, [40, 0, 25])]
CASES = [(*s, False) for s in SHAPES] + [(4, 3, 171, 80, [40, 0, 25], True)]     # True: the fixed-pair (dn) form, one pair list for every layer
SPECIAL = (88.0, -88.0, 100.0, -100.0, 0.0, 30.0, -30.0)                         # expf overflows / underflows at the first four


def case_id(c):
    Lr, B, nq, nc, counts, fixed = c
    return f'Lr{Lr}-B{B}-nq{nq}-nc{nc}-n{sum(counts)}' + ('-fixed' if fixed else '')


def family_pair(j, l=0):
    """Pair j of a batch for layer l: family j mod len(PAIRS), translated by the repetition (no two columns of a cost matrix are equal) and,
    in layers 1.., the prediction mirrored about the box's centre in x (odd l) and y (l & 2): a tie or a closed clamp stays one, on the
    opposite edge.  Returns (family, prediction, box) in units of U."""
    f, a, b = PAIRS[j % len(PAIRS)]
    rep = j // len(PAIRS)
    dx, dy = 3 * rep, 5 * rep
    ax, ay = (2 * b[0] - a[0] if l & 1 else a[0]), (2 * b[1] - a[1] if l & 2 else a[1])
    return f, (ax + dx, ay + dy, a[2], a[3]), (b[0] + dx, b[1] + dy, b[2], b[3])


def make_case(Lr, B, nq, nc, counts, fixed, only=None):
    """The inputs of one case, on the CPU: pb, ps, gtb, gtc, the per-layer matches (a list over layers of per-image (query, box) index
    pairs, the form DETRLoss.fixed_matches takes; fixed: one list for every layer) and their flat form li, bi, si, gi, n, the upstream
    gradient up [3, Lr].  only: restrict the pairs to these families."""
    G = sum(counts)
    idx = [j for j in range(10 ** 6) if only is None or PAIRS[j % len(PAIRS)][0] in only][:G]
    g = torch.Generator().manual_seed(Lr * 1000 + nq)
    pb = torch.cat([torch.randint(200, 824, (Lr, B, nq, 2), generator=g), 2 * torch.randint(2, 200, (Lr, B, nq, 2), generator=g)], -1).double()
    N = Lr * B * nq * nc
    ps = (-30 + 60 * ((torch.arange(N, dtype=torch.float64) * 0.6180339887 + 0.25) % 1)).view(Lr, B, nq, nc)   # a ramp over [-30, 30), scattered
    k = min(N, 3 * len(SPECIAL))
    ps.view(-1)[(torch.arange(k) * 53 + 1) % N] = torch.tensor(SPECIAL * 3, dtype=torch.float64)[:k]      # the special logits on unmatched classes
    gtb = torch.tensor([family_pair(j)[2] for j in idx], dtype=torch.float64).view(G, 4)
    gtc = (torch.arange(G) * 7 + 3) % nc
    offs = [sum(counts[:i]) for i in range(B)]
    matches, fams = [], []
    for l in range(Lr):
        per_image = []
        for i, c in enumerate(counts):
            q = (torch.arange(c) * 37 + (0 if fixed else 11 * l) + 5) % nq
            per_image.append((q, torch.arange(c) + offs[i]))
            for k in range(c):
                f, a, _ = family_pair(idx[offs[i] + k], l)
                pb[l, i, q[k]] = torch.tensor(a, dtype=torch.float64)
                fams.append(f)
                if offs[i] + k < len(SPECIAL):          # the matched class of the first matched rows sits on the special logits
                    ps[l, i, q[k], gtc[offs[i] + k]] = SPECIAL[(offs[i] + k + l) % len(SPECIAL)]
        matches.append(per_image)
    assert all(len(set(q.tolist())) == len(q) for m in matches for q, _ in m), 'a query matched twice'
    li = torch.arange(Lr).repeat_interleave(G)
    bi = torch.cat([torch.cat([torch.full_like(q, i) for i, (q, _) in enumerate(m)]) for m in matches])
    si = torch.cat([torch.cat([q for q, _ in m]) for m in matches])
    gi = torch.cat([torch.cat([k for _, k in m]) for m in matches])
    up = torch.arange(1, 3 * Lr + 1, dtype=torch.float32).view(3, Lr) / Lr
    return {'pb': (pb * U).float(), 'ps': ps.float(), 'gtb': (gtb * U).float(), 'gtc': gtc, 'matches': matches, 'fixed': fixed, 'li': li, 'bi': bi,
            'si': si, 'gi': gi, 'n': G, 'up': up, 'counts': list(counts), 'families': fams, 'shape': (Lr, B, nq, nc)}


def terms_of(fn, case, dev='cpu'):
    """fn(pb, ps, gtb, gtc, li, bi, si, gi, n, case) -> the three [Lr] terms; returns them with d/d(pb), d/d(ps) for case['up']."""
    pb, ps = case['pb'].to(dev).requires_grad_(), case['ps'].to(dev).requires_grad_()
    terms = fn(pb, ps, case['gtb'].to(dev), case['gtc'].to(dev), *(case[k].to(dev) for k in ('li', 'bi', 'si', 'gi')), case['n'], case)
    gpb, gps = torch.autograd.grad((torch.stack(list(terms)) * case['up'].to(dev)).sum(), [pb, ps])
    return {'class': terms[0].detach(), 'bbox': terms[1].detach(), 'giou': terms[2].detach(), 'dpb': gpb, 'dps': gps}


def torch_form(pb, ps, gtb, gtc, li, bi, si, gi, n, case):
    """The elementwise torch form of tam-tr_amd/loss.py (DETRLoss._layers off the GPU), in the dtype of pb."""
    import tamtr_amd.loss as LS
    crit = LS.DETRLoss(nc=ps.shape[-1], use_vfl=True)
    if case['fixed']:
        return crit._layers(pb, ps, gtb, gtc, case['counts'], LS.Matches(case['matches'][0]))
    crit.fixed_matches = case['matches']
    return crit._layers(pb, ps, gtb, gtc, case['counts'], None)


_REFS = {}


def terms_ref(c, mut=()):
    key = (case_id(c), tuple(mut))
    if key not in _REFS:
        case = make_case(*c)
        _REFS[key] = (case, R.detr_terms(case['pb'], case['ps'], case['gtb'], case['gtc'], case['li'], case['bi'], case['si'], case['gi'], case['n'],
                                         GAINS_LOSS, case['up'], mut=mut))
    return _REFS[key]


def old_rule(got, ref):
    """Would the tolerances of test_fused_loss_terms_and_matcher_cost_equal_the_torch_form have passed these outputs (NaN rows set aside)?"""
    ok = all(R.old_close(got[k], ref[k][0], 2e-5, 1e-6) for k in ('class', 'bbox', 'giou'))
    for k in ('dpb', 'dps'):
        want = torch.nan_to_num(ref[k][0], nan=0.0)
        ok = ok and R.old_close(torch.nan_to_num(got[k].detach().cpu().double(), nan=0.0), want, 2e-4, 2e-6 * float(want.abs().max()))
    return ok


def assert_terms(tag, c, got, ref=None, limit=1.0):
    """Every output of one case against detr_terms.  d/d(ps) may lose a product below fp32's smallest normal number (p^3 at logit -30 is
    1e-39): tiny = FLT_MIN times the largest upstream factor.  Returns the worst ratio per output."""
    case, want = terms_ref(c)
    want = ref or want
    Lr, B, nq, nc = case['shape']
    b = R.detr_bounds(B, nq, nc, case['n'])
    worst = {}
    for k in ('class', 'bbox', 'giou', 'dpb', 'dps'):
        tiny = 4 * R.FLT_MIN * float(case['up'].abs().max()) * max(GAINS_LOSS) if k == 'dps' else 0.0
        worst[k] = R.check(f'{tag} {case_id(c)} {k}', got[k], want[k][0], want[k][1], 0, b[k], tiny=tiny)
        assert worst[k] <= limit, f'{tag} {case_id(c)} {k}: ratio {worst[k]:.3g} > {limit}'
    nan_rows = torch.isnan(want['dpb'][0]).all(-1)
    assert int(nan_rows.sum()) == case['families'].count('same_centre') and bool((torch.isnan(want['dpb'][0]).any(-1) == nan_rows).all())
    assert int((got['dpb'].detach().cpu() != 0).any(-1).sum()) == case['shape'][0] * case['n'], 'exactly the matched rows carry a box gradient'
    R.note(f'{tag} {case_id(c)}: the old assert_close rule would have {"passed" if old_rule(got, want) else "FAILED"}')
    return worst


# ================================================================================================ the matcher's cost
def cost_case(c, nonfinite=False):
    """The inputs of make_case as a cost problem (every prediction against every box).  nonfinite: three diverged predictions of layer 0 -
    a NaN coordinate, a 0 x 0 box (0 / 0 in the aspect term), a NaN logit row - whose entries must come out as exact zeros."""
    case = make_case(*c)
    if nonfinite:
        case['pb'][0, 0, 1, 0] = float('nan')
        case['pb'][0, 0, 3, 2:] = 0.0
        case['ps'][0, 0, 4, :] = float('nan')
    return case


def assert_cost(tag, c, case, got, limit=1.0):
    val, mag, lo, hi = R.detr_match_cost(case['ps'], case['pb'], case['gtb'], case['gtc'], GAINS_COST, ALPHA, GAMMA)
    w = R.check(f'{tag} {case_id(c)} cost', got, val, mag, 0, R.fp32_b(R.DL_COST_N), envelope=(lo, hi))
    assert w <= limit, f'{tag} {case_id(c)} cost: ratio {w:.3g} > {limit}'
    R.note(f'{tag} {case_id(c)} cost: the old assert_close rule (rtol 2e-5, atol 1e-6) would have {"passed" if R.old_close(got, val, 2e-5, 1e-6) else "FAILED"}')
    return w


def scipy_pairs(C, counts):
    """scipy's assignment per image on the cost C [B, nq, G] (the matcher's host branch): (bi, si, gi) over the flattened box list."""
    from scipy.optimize import linear_sum_assignment
    bi, si, gi, off = [], [], [], 0
    for i, cols in enumerate(C.detach().cpu().split(list(counts), -1)):
        r, k = linear_sum_assignment(cols[i].numpy())
        bi += [i] * len(r); si += r.tolist(); gi += (k + off).tolist()
        off += counts[i]
    return tuple(torch.tensor(t, dtype=torch.long) for t in (bi, si, gi))


# ================================================================================================ box refinement
REFINE_EDGES = (0.0, 1.0, 5e-6, 1 - 5e-6, 3e-5, 1 - 3e-5, -0.2, 1.3, 0.5, 2e-5)   # (not eps itself: float(1e-5) < 1e-5, a tie fp64 breaks the other way)
REFINE_DELTAS = (100.0, -100.0, 20.0, -20.0)


def refine_inputs(ddt):
    """ref, delta, cot [16, 292, 4]: random references with the clamp edges in front, and every edge once more against each extreme delta."""
    g = torch.Generator().manual_seed(5)
    ref = torch.rand(16, 292, 4, generator=g)
    delta = torch.randn(16, 292, 4, generator=g) * 2
    cot = torch.randn(16, 292, 4, generator=g)
    edge = torch.tensor(REFINE_EDGES)
    ne, k = edge.numel(), edge.numel()
    ref.view(-1)[:ne] = edge
    for d in REFINE_DELTAS:
        ref.view(-1)[k:k + ne] = edge
        delta.view(-1)[k:k + ne] = d
        k += ne
    for d in REFINE_DELTAS:                               # and against an ordinary reference
        delta.view(-1)[k] = d
        k += 1
    return ref, delta.to(ddt), cot


def assert_refine(tag, ddt, ref, delta, cot, y, gd, gr, limit=1.0):
    """y, d/d(delta) (in delta's dtype: a = 1 for bf16), d/d(ref).  y = sigmoid(-100 ..) is 4e-44, below fp32's normal range: tiny."""
    want = R.box_refine(delta, ref, cot)
    tiny = 4 * R.FLT_MIN * float(cot.abs().max()) * 1e5          # (x 1 / eps: the factor of d/d(ref))
    worst = {}
    for k, t, a in (('y', y, 0), ('gd', gd, 1 if ddt == torch.bfloat16 else 0), ('gr', gr, 0)):
        worst[k] = R.check(f'{tag} box_refine {str(ddt)[6:]} {k}', t, want[k][0], want[k][1], a, R.BOX_REFINE_B[k], tiny=tiny)
        assert worst[k] <= limit, (k, worst[k])
    return worst


# ================================================================================================ the optimizer
OPT_LENGTHS = (1, 3, 4, 8191, 8192, 8193, 16385)          # the quad tail, the chunk boundary and one element past it, a third chunk of one element
OPT_GROUPS = ((1e-2, 0.0), (2e-3, 0.1), (5e-4, 0.1))      # (lr, weight decay); lr wd p is 3 000 / 800 ulp of p in the decayed groups
# (step count before the step, gradient scale: 'clipped' | 'below' | 'noclip' (max_norm = 0), EMA update number, shadows)
OPT_CASES = [(0, 'clipped', 1, False), (1, 'clipped', 100, True), (1, 'below', 100000, False), (9, 'below', 100, True), (9, 'clipped', 1, False),
             (999, 'noclip', 100, True), (99999, 'clipped', 100000, False), (99999, 'below', 1, True)]
OPT_BETAS, OPT_EPS, OPT_MAX_NORM = (0.9, 0.999), 1e-8, 0.1


def opt_case_id(c):
    return f'step{c[0]}-{c[1]}-ema{c[2]}' + ('-shadows' if c[3] else '')


def opt_tensors(step0, mode):
    """name -> (group, p, g | None, m, v) on the CPU, fp32.  'off1': taken by the test as a view one element into a larger buffer;
    'bias0': all zeros; 'nograd': no gradient this step; plus an EMA-only buffer 'stat' (group None)."""
    g = torch.Generator().manual_seed(step0 + len(mode))
    gs = {'clipped': 1.0, 'below': 1e-6, 'noclip': 3.0}[mode]
    out = {}
    names = [(f'w{n}', n) for n in OPT_LENGTHS] + [('off1', 8193 + 2), ('bias0', 37), ('nograd', 9)]
    for j, (name, n) in enumerate(names):
        p = torch.randn(n, generator=g) * 0.5
        if name == 'bias0':
            p.zero_()
        grad = None if name == 'nograd' else torch.randn(n, generator=g) * gs
        fresh = step0 == 0
        m = torch.zeros(n) if fresh else torch.randn(n, generator=g) * gs * 0.3
        v = torch.zeros(n) if fresh else (torch.randn(n, generator=g) * gs * 0.4) ** 2
        out[name] = (j % len(OPT_GROUPS), p, grad, m, v)
    out['stat'] = (None, torch.randn(21, generator=g), None, None, None)
    return out


def ema_decay(updates, decay=0.9999, tau=2000):
    return decay * (1 - math.exp(-updates / tau))


def assert_optim(tag, c, tensors, ema_before, got, limit=1.0, mut=()):
    """got: {'norm', 'coef': floats, name: {'gc', 'm', 'v', 'p', 'e', 'step'}} after one step from `tensors` (opt_tensors) and the EMA values
    ema_before (name -> tensor).  The update is formed here from the stored p': p' - (1 - lr wd) p in fp64.  Returns the worst ratio per
    quantity."""
    step0, mode, upd, _ = c
    names = list(tensors)
    lr = [OPT_GROUPS[tensors[n][0]][0] if tensors[n][0] is not None else 0.0 for n in names]
    wd = [OPT_GROUPS[tensors[n][0]][1] if tensors[n][0] is not None else 0.0 for n in names]
    ref = R.optim_step([tensors[n][1] for n in names], [tensors[n][2] for n in names], [tensors[n][3] for n in names], [tensors[n][4] for n in names],
                       [ema_before[n] for n in names], [step0] * len(names), lr, wd, *OPT_BETAS, OPT_EPS, 0.0 if mode == 'noclip' else OPT_MAX_NORM,
                       ema_decay(upd), mut=mut)
    clipped = float(ref['coef'][0]) < 1
    assert clipped == (mode == 'clipped')
    b = R.optim_bounds(clipped)
    worst = {k: 0.0 for k in ('norm', 'coef', 'gc', 'm', 'v', 'update', 'p', 'e')}
    for k in ('norm', 'coef'):
        worst[k] = R.check(f'{tag} {opt_case_id(c)} {k}', torch.tensor(float(got[k]), dtype=torch.float64), ref[k][0], ref[k][1], 0, b[k])
    if not clipped:
        assert float(got['coef']) == 1.0
    old = True
    for i, n in enumerate(names):
        o = got[n]
        for k in ('gc', 'm', 'v', 'p', 'e'):
            if ref[k][i] is None:
                continue
            worst[k] = max(worst[k], R.check(f'{tag} {opt_case_id(c)} {k} {n}', o[k], ref[k][i][0], ref[k][i][1], 0, b[k], log=False))
        if ref['update'][i] is not None:
            lw = R.f32(R.f32(lr[i]) * R.f32(wd[i]))
            upd_got = o['p'].detach().cpu().double() - (1 - lw) * tensors[n][1].double()
            worst['update'] = max(worst['update'], R.check(f'{tag} {opt_case_id(c)} update {n}', upd_got, ref['update'][i][0], ref['update'][i][1], 0,
                                                           b['update'], log=False))
            if not clipped:
                assert torch.equal(o['gc'].cpu(), tensors[n][2]), f'{n}: a gradient below max_norm is left bit for bit'
            old = old and R.old_close(o['p'], ref['p'][i][0], 1e-5, 2e-6)
        assert tensors[n][0] is None or float(o['step']) == ref['step'][i], (n, float(o['step']), ref['step'][i])
    for k, w in worst.items():
        R.report(f'{tag} {opt_case_id(c)} {k}', w, 0, b[k], sum(t[1].numel() for t in tensors.values()))
        assert w <= limit, f'{tag} {opt_case_id(c)} {k}: ratio {w:.3g} > {limit}'
    R.note(f'{tag} {opt_case_id(c)}: the old rule on the parameter (rtol 1e-5, atol 2e-6) would have {"passed" if old else "FAILED"}')
    return worst


def opt_module(tensors, dev, dtype=torch.float32):
    """A module that owns the tensors of opt_tensors: parameters by name, 'stat' as a buffer, 'off1' as a view that starts one element
    (4 bytes off 16-byte alignment) into a larger buffer."""
    import torch.nn as nn
    net = nn.Module()
    for name, (grp, p, _, _, _) in tensors.items():
        if grp is None:
            net.register_buffer(name, p.to(dev, dtype).clone())
        elif name == 'off1':
            buf = torch.zeros(p.numel() + 1, device=dev, dtype=dtype)
            buf[1:].copy_(p)
            net.register_parameter(name, nn.Parameter(buf[1:]))
        else:
            net.register_parameter(name, nn.Parameter(p.to(dev, dtype).clone()))
    return net


def opt_optimizer(net, tensors, step0, groups=OPT_GROUPS, betas=OPT_BETAS, eps=OPT_EPS):
    """torch.optim.AdamW over three parameter groups with the gradients and, past step 0, the state of opt_tensors."""
    pg = [{'params': [getattr(net, n) for n, t in tensors.items() if t[0] == gi], 'lr': lr, 'weight_decay': wd} for gi, (lr, wd) in enumerate(groups)]
    opt = torch.optim.AdamW(pg, betas=betas, eps=eps)
    for n, (grp, _, g, m, v) in tensors.items():
        if grp is None:
            continue
        q = getattr(net, n)
        q.grad = None if g is None else g.to(q).clone()
        if step0 > 0:
            opt.state[q] = {'step': torch.tensor(float(step0)), 'exp_avg': m.to(q).clone(), 'exp_avg_sq': v.to(q).clone()}
    return opt


def torch_stepper(net, opt, ema, max_norm):
    """clip_grad_norm_ + AdamW.step + ModelEMA.update: what engine.FusedOptimStep.step replaces."""
    ps = [p for p in net.parameters() if p.grad is not None]
    norm = torch.nn.utils.clip_grad_norm_(ps, max_norm if max_norm > 0 else float('inf'))
    opt.step()
    ema.update(net)
    return float(norm), (min(1.0, max_norm / (float(norm) + 1e-6)) if max_norm > 0 else 1.0)


def optim_run(c, stepper, dev='cpu', dtype=torch.float32, abi_consts=False):
    """One step of case c on `dev`: returns (tensors, ema_before, got, net) for assert_optim.  stepper(net, opt, ema, max_norm) ->
    (norm, coef).  The EMA copy is moved off the model's values first, so that its own term shows.
    abi_consts: hand torch the betas, eps and EMA decay as the fp32 values the C ABI of csrc/optim.hip receives.  torch forms 1 - beta in
    double from the double it is given: from 0.999 that is 0.001, from the fp32 value 0.00100005, 4.7e-5 apart; optim_step() is stated on the
    fp32 values, and a torch run that is held to its bound has to start from the same ones."""
    from tamtr_amd.engine import ModelEMA
    step0, mode, upd, _ = c
    tensors = opt_tensors(step0, mode)
    net = opt_module(tensors, dev, dtype)
    opt = opt_optimizer(net, tensors, step0, betas=tuple(R.f32(b) for b in OPT_BETAS) if abi_consts else OPT_BETAS, eps=R.f32(OPT_EPS) if abi_consts else OPT_EPS)
    ema = ModelEMA(net, updates=upd - 1)
    if abi_consts:
        ema.decay = lambda x: R.f32(ema_decay(x))
    with torch.no_grad():
        for v in ema.ema.state_dict().values():
            v.mul_(0.875).add_(0.03125)
    before = {n: v.detach().cpu().clone() for n, v in ema.ema.state_dict().items()}
    norm, coef = stepper(net, opt, ema, 0.0 if mode == 'noclip' else OPT_MAX_NORM)
    got, esd = {'norm': float(norm), 'coef': float(coef)}, ema.ema.state_dict()
    for n, (grp, _, _, _, _) in tensors.items():
        q = getattr(net, n)
        st = opt.state.get(q, {}) if grp is not None else {}
        got[n] = {'gc': q.grad, 'm': st.get('exp_avg'), 'v': st.get('exp_avg_sq'), 'p': q.detach(), 'e': esd[n], 'step': float(st.get('step', 0.0))}
    assert ema.updates == upd
    return tensors, before, got, net


def cost_torch_form(case):
    """The matcher's cost as the elementwise fp32 torch form of tam-tr_amd/loss.py states it (HungarianMatcher.forward off the GPU)."""
    import tamtr_amd.loss as LS
    Lr, B, nq, nc = case['shape']
    ps = case['ps'].reshape(-1, nc).sigmoid()[:, case['gtc']]
    pb = case['pb'].reshape(-1, 4)
    neg = (1 - ALPHA) * ps ** GAMMA * (-(1 - ps + 1e-8).log())
    pos = ALPHA * (1 - ps) ** GAMMA * (-(ps + 1e-8).log())
    c_l1 = (pb.unsqueeze(1) - case['gtb'].unsqueeze(0)).abs().sum(-1)
    c_iou = 1.0 - LS.bbox_iou(pb.unsqueeze(1), case['gtb'].unsqueeze(0), xywh=True, RIOU=True).squeeze(-1)
    C = GAINS_COST[0] * (pos - neg) + GAINS_COST[1] * c_l1 + GAINS_COST[2] * c_iou
    return torch.where(torch.isfinite(C), C, torch.zeros_like(C)).view(Lr, B, nq, -1)


def refine_torch_form(d, r):
    x = r.clamp(min=0, max=1)
    return torch.sigmoid(d + torch.log(x.clamp(min=1e-5) / (1 - x).clamp(min=1e-5)))
