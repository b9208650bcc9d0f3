"""GPU: test-time augmentation.  tamtr_tta_view (csrc/tta.hip) against an fp64 statement of scale_img's rule, tamtr_tta_merge
bit-exact against tta.merge_host (whose claims test_tta_host.py checks on the CPU), and the predictor / validator / CLI end to end."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from test_gpu_predict import CONF, NC, SIZES, _images, _model, _text_feats, make_preds
from test_predict_host import reference_postprocess
from test_tta_host import SIZE, VIEWS, view_outputs
from test_val_host import engine_rule

pytestmark = pytest.mark.gpu

SIX_VIEWS = ((1.0, False), (0.83, True), (0.67, False), (1.0, True), (0.75, False), (1.25, True))


# ------------------------------------------------------------------------------------------------ the view kernel
def view_rule_fp64(x, ratio, flip, gs=64):
    """scale_img on x.flip(3) in pure fp64, the coordinates included: src = max(sc (d + 0.5) - 0.5, 0) with sc = n_in / n_out,
    i0 = floor(src), i1 = min(i0 + 1, n_in - 1), weights l1 = src - i0 and l0 = 1 - l1; float32(0.447) outside the content."""
    from tamtr_amd import tta
    B, C, H, W = x.shape
    (sh, sw), (Hp, Wp) = tta.tta_view_sizes(H, W, ratio, gs)
    x = (x.flip(3) if flip else x).double()

    def axis(n_in, n_out):
        src = (torch.arange(n_out, dtype=torch.float64) + 0.5) * (n_in / n_out) - 0.5
        src = src.clamp(min=0)
        i0 = src.floor().long()
        return i0, (i0 + 1).clamp(max=n_in - 1), src - i0

    y0, y1, ly = axis(H, sh)
    x0, x1, lx = axis(W, sw)
    ly, lx = ly[:, None], lx[None, :]
    top = (1 - lx) * x[:, :, y0][:, :, :, x0] + lx * x[:, :, y0][:, :, :, x1]
    bot = (1 - lx) * x[:, :, y1][:, :, :, x0] + lx * x[:, :, y1][:, :, :, x1]
    out = torch.full((B, C, Hp, Wp), float(np.float32(0.447)), dtype=torch.float64)
    out[:, :, :sh, :sw] = (1 - ly) * top + ly * bot
    return out, (sh, sw)


@pytest.mark.parametrize('shape,ratio,flip', [((2, 3, 128, 128), 0.83, True), ((2, 3, 128, 128), 0.67, False), ((1, 3, 96, 160), 0.75, True),
                                              ((1, 3, 64, 72), 1.25, False)])
def test_view_against_the_fp64_rule(shape, ratio, flip):
    """Bound 4 ulp_fp32(max(H, W)) + 2^-22: torch computes each axis's source coordinate in fp32 from three roundings at magnitude
    below the input size - at most 2 ulp of that size per axis - pixel differences are at most 1 (inputs in [0, 1]) and there are two
    axes; 2^-22 covers the interpolation's own roundings of values in [0, 1].  view_host (torch's own interpolate) must meet the same
    bound, so the bound never hides a failure the reference would not share."""
    from tamtr_amd import ops, tta
    x = torch.rand(*shape, generator=torch.Generator().manual_seed(shape[2] + shape[3]))
    want, (sh, sw) = view_rule_fp64(x, ratio, flip)
    got = ops.tta_view(x.cuda(), ratio, flip)
    torch.cuda.synchronize()
    got, host = got.cpu(), tta.view_host(x, ratio, flip)
    bound = 4 * float(np.spacing(np.float32(max(shape[2], shape[3])))) + 2.0 ** -22
    assert got.shape == want.shape == host.shape and got.dtype == torch.float32
    err, err_host = (got.double() - want).abs().max().item(), (host.double() - want).abs().max().item()
    print(f'tta_view {shape} ratio {ratio} flip {flip}: kernel {err:.3e} view_host {err_host:.3e} bound {bound:.3e}')
    assert err_host <= bound and err <= bound
    pad = torch.tensor(0.447, dtype=torch.float32)
    assert (got[:, :, sh:] == pad).all() and (got[:, :, :, sw:] == pad).all()
    assert got[:, :, sh:].numel() + got[:, :, :, sw:].numel() > 0


def test_view_of_ratio_one_is_a_copy():
    from tamtr_amd import ops
    x = torch.rand(2, 3, 128, 128, generator=torch.Generator().manual_seed(4)).cuda()
    assert torch.equal(ops.tta_view(x, 1.0, True), x.flip(3)) and torch.equal(ops.tta_view(x, 1.0, False), x)
    y = ops.tta_view(x[:, :, :100, :90], 1.0, True)      # not a multiple of gs: the copy sits in a padded canvas
    assert y.shape == (2, 3, 128, 128) and torch.equal(y[:, :, :100, :90], x[:, :, :100, :90].flip(3))
    assert (y[:, :, 100:] == 0.447).all() and (y[:, :, :, 90:] == 0.447).all()


# ------------------------------------------------------------------------------------------------ the merge kernel
def run_both(ys, views, conf, iou, classes=None, single_cls=False, max_out=512, size=SIZE):
    from tamtr_amd import ops, tta
    got = ops.tta_merge([y.cuda() for y in ys], views, conf, iou, classes, single_cls, max_out=max_out, size=size)
    torch.cuda.synchronize()
    return tuple(t.cpu() for t in got), tta.merge_host(ys, views, conf, iou, classes, single_cls, max_out=max_out, size=size)


def assert_same(got, want, what):
    for g, w, name in zip(got, want, ('ym', 'src', 'counts', 'dropped')):
        assert g.dtype == w.dtype and g.shape == w.shape, f'{what}: {name} {g.dtype}{tuple(g.shape)} vs {w.dtype}{tuple(w.shape)}'
        assert torch.equal(g, w), f'{what}: {name} differs at {(g != w).nonzero()[:5].tolist()}'


@pytest.mark.parametrize('dt', ['f32', 'bf16'])
@pytest.mark.parametrize('B,V,nq,nc', [(3, 3, 300, 10), (2, 2, 37, 1), (1, 6, 300, 80), (1, 1, 5, 3), (2, 4, 512, 10)])
def test_merge_bit_exact(B, V, nq, nc, dt):
    ys = view_outputs(B, V, nq, nc, seed=V * nq + nc, dtype=torch.bfloat16 if dt == 'bf16' else torch.float32)
    for conf, iou in ((0.25, 0.7), (0.4, 0.45)):
        got, want = run_both(ys, SIX_VIEWS[:V], conf, iou)
        assert_same(got, want, f'B{B} V{V} nq{nq} nc{nc} {dt} conf{conf} iou{iou}')
        assert int(want[2].sum()) > 0


@pytest.mark.parametrize('dt', ['f32', 'bf16'])
def test_merge_on_the_edge_images(dt):
    """make_preds' six images (heavy overlap, duplicated rows, a NaN score and zero-width boxes, nothing above conf, one box, scores
    on a coarse grid), and what the following postprocess makes of the merged tensor: exactly what it makes of the concatenation."""
    from tamtr_amd import ops, tta
    ys = view_outputs(6, 3, 300, 10, seed=3, dtype=torch.bfloat16 if dt == 'bf16' else torch.float32)
    hw = [(480 + 10 * b, 640 - 7 * b) for b in range(6)]
    for conf, iou, classes, single_cls in ((0.4, 0.45, None, False), (0.25, 0.7, [1, 3, 7], True), (0.001, 0.6, [], False)):
        got, want = run_both(ys, VIEWS, conf, iou, classes, single_cls)
        what = f'{dt} conf{conf} iou{iou} classes{classes} single{single_cls}'
        assert_same(got, want, what)
        assert want[3].tolist() == [0] * 6, 'a condition of the test: nothing is dropped'
        assert want[2][3] == 0 and (classes == [] or want[2].sum() > 20)
        out, keep, counts = ops.detect_postprocess(got[0].cuda(), hw, conf, iou, classes, single_cls)
        co, ck, cc = reference_postprocess(tta.deaugment_host(ys, tta.tta_view_factors(VIEWS, SIZE)), hw, conf, iou, classes, single_cls)
        out, keep, counts = out.cpu(), keep.cpu(), counts.cpu()
        assert torch.equal(counts, cc), what
        for b, n in enumerate(cc.tolist()):
            assert torch.equal(out[b, :n], co[b, :n]) and not out[b, n:].any(), f'{what}: image {b}'
            assert torch.equal(got[1][b, keep[b, :n].long()], ck[b, :n]), f'{what}: image {b} sources'


def test_duplicate_rows_across_views_tie_by_candidate_index():
    y = make_preds(2, 37, 4, seed=9)
    views = [(1.0, 1.0, False)] * 3      # identity views: the Ensemble merge
    got, want = run_both([y, y.clone(), make_preds(2, 37, 4, seed=10)], views, 0.1, 0.7, size=None)
    assert_same(got, want, 'duplicates')
    for b in range(2):
        s = got[1][b, :got[2][b]]
        assert got[2][b] > 0 and not ((s >= 37) & (s < 74)).any()


def test_threshold_follows_torchvision_double_comparison():
    """As test_gpu_predict's: 60/100 rounds to fp32(0.6) > 0.6, so the second view's box goes; 70/100 rounds to fp32(0.7) < 0.7."""
    for h2, iou, kept in ((6.0, 0.6, 1), (7.0, 0.7, 2)):
        ys = [torch.tensor([[[5.0, 5.0, 10.0, 10.0, 0.9]]]), torch.tensor([[[5.0, h2 / 2, 10.0, h2, 0.8]]])]
        got, want = run_both(ys, [(1.0, 1.0, False)] * 2, 0.25, iou, size=None, max_out=4)
        assert int(want[2][0]) == kept
        assert_same(got, want, f'iou {iou}')


def test_negative_conf_and_signed_zero_scores_tie():
    y = torch.tensor([[[0.1, 0.1, 0.05, 0.05, -0.0], [0.3, 0.3, 0.05, 0.05, 0.0], [0.5, 0.5, 0.05, 0.05, -0.25],
                       [0.7, 0.7, 0.05, 0.05, -0.0], [0.9, 0.9, 0.05, 0.05, 0.5]]])
    got, want = run_both([y, y[:, [4, 3, 2, 1, 0]] * torch.tensor([1.0, 1.0, 1.0, 1.0, 0.5])], VIEWS[:2], -0.5, 0.7, max_out=12)
    assert want[1][0, :3].tolist() == [4, 5, 0] and int(want[2][0]) == 10
    assert_same(got, want, 'negative conf')


@pytest.mark.parametrize('dt', ['f32', 'bf16'])
def test_merge_with_max_out_16_reports_what_it_dropped(dt):
    ys = view_outputs(3, 3, 300, 10, seed=3, dtype=torch.bfloat16 if dt == 'bf16' else torch.float32)
    got, want = run_both(ys, VIEWS, 0.25, 0.7, max_out=16)
    assert (want[3] > 0).all() and want[2].tolist() == [16] * 3 and got[0].shape == (3, 16, 14)
    assert_same(got, want, f'overflow {dt}')
    full = run_both(ys, VIEWS, 0.25, 0.7, max_out=512)[0]
    assert torch.equal(got[3], full[2] + full[3] - 16) and torch.equal(got[0], full[0][:, :16])


def test_val_postprocess_match_takes_the_merged_tensor():
    """The validator's kernel on ym equals the host Validator's rule on ym (engine.postprocess + process_batch)."""
    from tamtr_amd import ops
    from test_val_host import make_case, orig_shapes
    cases = [make_case(2, 300, 10, (37, 5), 50 + v) for v in range(3)]
    _, cls, boxes, bidx = cases[0]
    got, _ = run_both([torch.from_numpy(c[0]) for c in cases], VIEWS, 0.001, 0.7)
    ym, hw = got[0], orig_shapes(2, 3)
    assert int(got[3].sum()) == 0 and int(got[2].min()) > 0
    predn, correct, counts, _, _ = ops.val_postprocess_match(ym.cuda(), cls, boxes, bidx, hw, 640, 0.001, 0.7)
    want = engine_rule(ym.numpy(), cls, boxes, bidx, hw, 640, 0.001, 0.7)
    for g, w, name in zip((predn, correct, counts), want, ('predn', 'correct', 'counts')):
        assert torch.equal(g.cpu(), torch.from_numpy(w)), name
    assert (counts.cpu() <= got[2]).all() and int(counts.min()) > 0 and int(correct.sum()) > 0


def test_merge_does_not_synchronise():
    from tamtr_amd import ops
    ys = [y.cuda() for y in view_outputs(4, 3, 300, 10, seed=7)]
    cls_dev = torch.tensor([1, 2], dtype=torch.int32, device='cuda')
    x = torch.rand(2, 3, 128, 128, device='cuda')
    ops.tta_merge(ys, VIEWS, 0.25, 0.7, size=SIZE)      # first call: library load, allocator warm-up
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode('error')
    try:
        a = ops.tta_merge(ys, VIEWS, 0.25, 0.7, cls_dev, size=SIZE)
        b = ops.tta_merge(ys, VIEWS, 0.25, 0.7, [1, 2], size=SIZE)      # host lists: one upload, no sync
        ops.tta_merge(ys, VIEWS, 0.25, 0.7, size=SIZE)
        ops.tta_view(x, 0.83, True)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    for u, v in zip(a, b):
        assert torch.equal(u, v)


def test_capacities_are_refused():
    from tamtr_amd import TamtrHipError, ops
    ident = [(1.0, 1.0, False)]
    with pytest.raises(TamtrHipError):
        ops.tta_merge([torch.zeros(1, 2049, 14, device='cuda')], ident, 0.25, 0.7)      # N = 2049
    with pytest.raises(TamtrHipError):
        ops.tta_merge([torch.zeros(1, 683, 14, device='cuda')] * 3 + [torch.zeros(1, 683, 14, device='cuda')], ident * 4, 0.25, 0.7)
    with pytest.raises(TamtrHipError):
        ops.tta_merge([torch.zeros(1, 300, 14, device='cuda')], ident, 0.25, 0.7, max_out=513)
    with pytest.raises(TamtrHipError):
        ops.tta_merge([torch.zeros(1, 300, 14, device='cuda')] * 2, ident, 0.25, 0.7)      # two outputs, one view


# ------------------------------------------------------------------------------------------------ end to end
IMGSZ = 256      # 128 would scale to maps with fewer than 300 tokens; the canvases are 256, 256 and 192


def _predictor(augment, views=None, dtype='fp32', **kw):
    from tamtr_amd.predict import Predictor
    names = {i: f'c{i}' for i in range(NC)}
    return Predictor(_model().cuda(), names, _text_feats(), imgsz=IMGSZ, conf=CONF, iou=0.7, batch=2, dtype=dtype, keep_raw=True, augment=augment,
                     tta_views=views, **kw)


def test_track_refuses_augment():
    pred = _predictor(True)
    with pytest.raises(ValueError):
        pred.track('nowhere/')      # refused when called, before any file is looked for
    with pytest.raises(ValueError):
        pred.track_streams(['nowhere/'])
    assert 'tta' in pred.times and 'tta' not in _predictor(False).times


def test_identity_view_gives_the_plain_predictors_detections(tmp_path):
    """With the one view (1, False) the detections are the non-augmented predictor's, exactly - on ONE forward: the view is the input
    bit for bit, and the plain predictor's own call (ops.detect_postprocess with its arguments) on the raw output of that forward
    gives the same rows.  Two predict() passes cannot show this: the trunk is not reproducible from one call to the next
    (test_gpu_botsort_reid.decoder_outputs_keep_their_bits; measured here on MI355X, the plain predictor against the augmented one
    on these five images: the same 16 rows per image, boxes up to 4.6e-05 px apart).  The second pass is still made: it must give the
    same rows with the same classes in the same order."""
    from tamtr_amd import data as D, ops
    src = _images(tmp_path)
    files = sorted(str(p) for p in src.iterdir())
    plain = [d.boxes for d in _predictor(False).predict(str(src))]
    pred = _predictor(True, ((1.0, False),))
    total = 0
    for i, det in enumerate(pred.predict(str(src))):
        k = i % 2
        if k == 0:
            hw = [D.decode_image(f).shape[:2] for f in files[i:i + 2]]
            assert len(pred.last_views) == len(pred.last_ys) == 1 and torch.equal(pred.last_views[0], pred.last_img)
            out, _, counts = ops.detect_postprocess(pred.last_ys[0], hw, CONF, 0.7)      # the plain predictor's call on this forward
            out, counts = out.cpu(), counts.cpu()
        n = int(counts[k])
        assert torch.equal(det.boxes, out[k, :n]), f'image {i}'
        worst = float((det.boxes - plain[i]).abs().max()) if det.boxes.shape == plain[i].shape and n else 0.0
        print(f'identity view, image {i}: {n} rows vs {len(plain[i])} of another pass, max |difference| {worst:.3e}')
        assert det.boxes.shape == plain[i].shape and torch.equal(det.boxes[:, 5], plain[i][:, 5]), f'image {i}'
        total += n
    assert total > 0 and pred.seen == len(SIZES) and pred.tta_dropped == 0


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
def test_predictor_with_the_default_views(tmp_path, dtype):
    from tamtr_amd import data as D, tta
    src = _images(tmp_path)
    pred = _predictor(True, dtype=dtype)
    files = sorted(str(p) for p in src.iterdir())
    total = 0
    for i, det in enumerate(pred.predict(str(src))):
        k = i % 2
        if k == 0:      # a new batch: its views and raw outputs are the predictor's last ones
            hw = [D.decode_image(f).shape[:2] for f in files[i:i + 2]]
            assert [tuple(v.shape[2:]) for v in pred.last_views] == [(256, 256), (256, 256), (192, 192)]
            assert torch.equal(pred.last_views[0], pred.last_img) and len(pred.last_ys) == 3
            print(f'default views {dtype}: raw outputs {[tuple(y.shape) for y in pred.last_ys]}, merged {tuple(pred.last_y.shape)}')
            nq = pred.last_ys[0].shape[1]
            assert all(y.shape == (len(hw), nq, 4 + NC) for y in pred.last_ys) and pred.last_y.shape == (len(hw), 512, 4 + NC)
            cat = tta.deaugment_host(pred.last_ys, tta.tta_view_factors(tta.DEFAULT_VIEWS, (IMGSZ, IMGSZ)))
            wo, _, wc = reference_postprocess(cat, hw, CONF, 0.7)
            print(f'default views {dtype}, batch at image {i}: survivors {wc.tolist()}')
        n = int(wc[k])
        assert torch.equal(det.boxes, wo[k, :n]), f'image {i}'
        total += n
    assert total > 0 and pred.seen == len(SIZES) and pred.tta_dropped == 0
    sp = pred.speed()
    assert sp['tta'] > 0 and all(v >= 0 for v in sp.values())


def _val_batches():
    g = torch.Generator().manual_seed(5)
    out = []
    for _ in range(2):
        out.append({'img': torch.rand(2, 3, IMGSZ, IMGSZ, generator=g).cuda(), 'cls': torch.randint(0, NC, (6, 1), generator=g).float(),
                    'bboxes': torch.cat([0.2 + 0.6 * torch.rand(6, 2, generator=g), 0.05 + 0.4 * torch.rand(6, 2, generator=g)], 1),
                    'batch_idx': torch.arange(2).repeat_interleave(3).float(), 'ori_shape': [(190, 300), (256, 256)]})
    return out


def test_validate_with_augment_equals_a_device_validator_fed_by_hand():
    from tamtr_amd import engine as E, tta
    model = _model().cuda().eval()
    model.set_text_features(_text_feats()[None].cuda())
    batches = _val_batches()
    res = E.validate(model, batches, imgsz=IMGSZ, conf=CONF, iou=0.7, on_device=True, augment=True)
    dv = E.DeviceValidator(IMGSZ, CONF, 0.7)
    dropped = 0
    for b in batches:
        ym, _, counts, drop = tta.tta_forward(model, b['img'], None, tta.DEFAULT_VIEWS, CONF, 0.7)
        assert ym.shape == (2, 512, 4 + NC) and int(counts.min()) > 0
        dropped += int(drop.sum())
        dv.update(ym, b)
    assert res.pop('tta_dropped') == dropped
    assert res == dv.results() and res['seen'] == 4
    plain = E.validate(model, batches, imgsz=IMGSZ, conf=CONF, iou=0.7, on_device=True)
    assert 'tta_dropped' not in plain and set(plain) == set(res)


def test_predict_cli_with_augment_writes_the_in_process_labels(tmp_path):
    src = _images(tmp_path)
    sd = _model().state_dict()
    ck = tmp_path / 'best.pt'
    torch.save({'model': sd, 'ema': sd}, ck)
    names = [f'c{i}' for i in range(NC)]
    feats = tmp_path / 'feats.npz'
    np.savez(feats, texts=np.array(names), feats=_text_feats().numpy())
    project = tmp_path / 'runs'
    cmd = [sys.executable, os.path.join(ROOT, 'tools', 'predict.py'), '--weights', str(ck), '--text-feats', str(feats), '--names', ','.join(names),
           '--source', str(src), '--imgsz', str(IMGSZ), '--batch', '2', '--conf', str(CONF), '--save-txt', '--save-conf', '--project', str(project),
           '--name', 'TTA', '--dtype', 'fp32', '--augment']
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res['images'] == len(SIZES) and res['detections'] > 0 and res['augment'] is True and res['tta_dropped'] == 0
    assert set(res['ms_per_image']) == {'load', 'forward', 'tta', 'postprocess'}
    here = tmp_path / 'here'
    n = 0
    for det in _predictor(True).predict(str(src)):
        det.save_txt(here / (os.path.splitext(os.path.basename(det.path))[0] + '.txt'), save_conf=True)
        n += len(det)
    assert n == res['detections']
    labels = sorted(p.name for p in (project / 'TTA' / 'labels').iterdir())
    assert labels == sorted(p.name for p in here.iterdir()) and labels
    for name in labels:      # two processes, two forwards: the trunk is not reproducible bit for bit, '%g' keeps six digits
        a, b = np.loadtxt(project / 'TTA' / 'labels' / name, ndmin=2), np.loadtxt(here / name, ndmin=2)
        assert a.shape == b.shape and np.array_equal(a[:, 0], b[:, 0]), name
        np.testing.assert_allclose(a[:, 1:], b[:, 1:], rtol=1e-5, atol=1e-6, err_msg=name)      # test_gpu_predict's label-file tolerance
