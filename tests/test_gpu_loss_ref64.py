"""The loss-term, matcher-cost and box-refinement kernels of csrc/detrloss.hip and the clip / AdamW / EMA kernels of csrc/optim.hip against
fp64 references with an error model (tests/ref64.py detr_terms, detr_match_cost, box_refine, optim_step).  The cases, the inputs and the
assertions themselves: tests/loss_cases.py (tests/test_ref64_host.py runs the same assertions on the fp32 torch forms on the CPU, held to
half of every bound, and on mistaken references, which miss them).

Each assertion is elementwise |got - ref| <= b mag with no free absolute term beyond fp32's underflow threshold; b is counted in
ref64.detr_bounds / optim_bounds.  Set TAMTR_REF64_REPORT=<file> to collect the worst err / bound ratio of every assertion
(profiles/loss_optim_ref64.txt)."""
import pytest
import torch

import loss_cases as LC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import tamtr_amd.ops as ops
    return ops


@pytest.mark.parametrize('c', LC.CASES, ids=LC.case_id)
def test_detr_terms_and_gradients_vs_fp64(ops, c):
    """ops.detr_layer_losses: the three terms per layer and d/d(boxes), d/d(logits) for distinct upstream gradients, over every pair
    family (ties, closed and touching clamps, containment, extreme aspects, the NaN row of coincident centres, logits where expf
    overflows) at shapes around every workgroup boundary, and the fixed-pair (dn) form."""
    case, _ = LC.terms_ref(c)
    got = LC.terms_of(lambda pb, ps, gtb, gtc, li, bi, si, gi, n, _: ops.detr_layer_losses(pb, ps, gtb, gtc, li, bi, si, gi, n, LC.GAINS_LOSS), case, 'cuda')
    LC.assert_terms('gpu', c, got)
    assert bool(torch.isfinite(got['dps']).all()) and all(bool(torch.isfinite(got[k]).all()) for k in ('class', 'bbox', 'giou'))


@pytest.mark.parametrize('nonfinite', [False, True], ids=['finite', 'nonfinite'])
@pytest.mark.parametrize('c', LC.CASES[:4], ids=LC.case_id)
def test_match_cost_vs_fp64_and_its_assignment_vs_scipy(ops, c, nonfinite):
    """ops.detr_match_cost: every prediction against every box, p rounded where the kernel rounds it (the envelope of its fp32
    neighbours); diverged predictions give exact zeros.  The assignment ops.lsap_assign draws from the kernel's own cost is scipy's."""
    cc = LC.cost_case(c, nonfinite)
    C = ops.detr_match_cost(cc['ps'].cuda(), cc['pb'].cuda(), cc['gtb'].cuda(), cc['gtc'].cuda(), LC.GAINS_COST, LC.ALPHA, LC.GAMMA)
    assert C.shape == (*cc['shape'][:3], cc['n']) and C.dtype == torch.float32
    LC.assert_cost('gpu' + (' nonfinite' if nonfinite else ''), c, cc, C)
    if nonfinite:
        assert bool((C[0, 0, [1, 3, 4]] == 0).all()) and int((C == 0).sum()) == 3 * C.shape[-1]
        return
    for l in range(cc['shape'][0]):
        got = ops.lsap_assign(C[l], cc['counts'])
        for g, w in zip(got, LC.scipy_pairs(C[l], cc['counts'])):
            assert torch.equal(g.cpu(), w), f'layer {l}: the assignment is not scipy\'s on the same cost'


@pytest.mark.parametrize('ddt', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
def test_box_refine_vs_fp64(ops, ddt):
    """ops.box_refine, value and both gradients: references on and beyond the clamps, each also against delta = +-100 and +-20."""
    ref, delta, cot = LC.refine_inputs(ddt)
    d, r = delta.cuda().requires_grad_(), ref.cuda().requires_grad_()
    y = ops.box_refine(d, r)
    assert y.dtype == torch.float32 and y.shape == ref.shape
    (y * cot.cuda()).sum().backward()
    assert d.grad.dtype == ddt
    LC.assert_refine('gpu', ddt, ref, delta, cot, y.detach(), d.grad, r.grad)


@pytest.mark.parametrize('c', LC.OPT_CASES, ids=LC.opt_case_id)
def test_fused_optim_single_step_vs_fp64(ops, c):
    """engine.FusedOptimStep.step, one step from a set state: the norm, the clip coefficient, the clipped gradients, both moments, the
    update p' - (1 - lr wd) p, the parameters, the EMA and the step counts, over tensor lengths around the quad tail and the chunk
    boundary, a parameter 4 bytes off 16-byte alignment (the scalar span), an all-zero parameter, one without a gradient, an EMA-only
    buffer, three parameter groups; with shadows each bf16 copy is the new master rounded to nearest even, bit for bit."""
    from tamtr_amd.engine import FusedOptimStep

    def stepper(net, opt, ema, max_norm):
        assert net.off1.data_ptr() % 16 == 4 and net.w4.data_ptr() % 16 == 0
        st = FusedOptimStep.create(net, opt, ema, max_norm=max_norm, shadows=c[3])
        assert st is not None
        out = st.step()
        return float(out[0]), float(out[1])
    tensors, before, got, net = LC.optim_run(c, stepper, 'cuda')
    LC.assert_optim('gpu', c, tensors, before, got)
    for n, p in net.named_parameters():
        sh = ops.bf16_shadow(p)
        assert (sh is not None) == c[3]
        if c[3]:
            assert sh.dtype == torch.bfloat16 and torch.equal(sh, p.detach().bfloat16()), f'bf16 copy of {n}'
