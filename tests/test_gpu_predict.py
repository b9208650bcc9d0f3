"""GPU: tamtr_detect_postprocess (csrc/predict.hip) bit-exact against the restated RTDETRPredictor.postprocess rule
(test_predict_host.reference_postprocess), and the predictor end to end (tam-tr_amd/predict.py, tools/predict.py)."""
import itertools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from test_predict_host import reference_postprocess

pytestmark = pytest.mark.gpu


def make_preds(B, nq, nc, seed):
    """Eval-output-like y [B, nq, 4 + nc] (fp32) whose images hit the edges of the rule, by image index:
    0 clustered boxes with heavy overlap; 1 duplicated rows (exact score ties, identical boxes); 2 a NaN score row and zero-width
    boxes (0/0 IoU); 3 nothing above any tested conf; 4 every box identical; 5 scores on a coarse grid (many ties)."""
    g = torch.Generator().manual_seed(seed)
    centres = torch.cat([torch.rand(6, 2, generator=g) * 0.6 + 0.2, torch.rand(6, 2, generator=g) * 0.25 + 0.05], 1)
    pick = centres[torch.randint(0, 6, (B, nq), generator=g)]
    xy = pick[..., :2] + torch.randn(B, nq, 2, generator=g) * 0.01
    wh = pick[..., 2:] * (0.85 + 0.3 * torch.rand(B, nq, 2, generator=g))
    scores = torch.sigmoid(torch.randn(B, nq, nc, generator=g) * 2 - 1)
    y = torch.cat([xy, wh, scores], -1)
    for b in range(B):
        kind = b % 6
        if kind == 1:
            k = nq // 3
            y[b, k:2 * k] = y[b, :k]
        elif kind == 2:
            y[b, nq // 2, 4 + nc // 2] = float('nan')
            y[b, ::7, 2] = 0.0
            y[b, 1::7, 3] = 0.0
        elif kind == 3:
            y[b, :, 4:] *= 0.0009
        elif kind == 4:
            y[b, :, :4] = torch.tensor([0.5, 0.4, 0.3, 0.2])
        elif kind == 5:
            y[b, :, 4:] = torch.round(y[b, :, 4:] * 8) / 8
    return y


def orig_sizes(B, seed):
    g = torch.Generator().manual_seed(seed + 1)
    return torch.stack([torch.randint(200, 1100, (B,), generator=g), torch.randint(200, 1100, (B,), generator=g)], 1).tolist()


def run_both(y, hw, conf, iou, classes=None, single_cls=False):
    from tamtr_amd import ops
    out, keep, counts = ops.detect_postprocess(y.cuda(), hw, conf, iou, classes, single_cls)
    torch.cuda.synchronize()
    return (out.cpu(), keep.cpu(), counts.cpu()), reference_postprocess(y, hw, conf, iou, classes, single_cls)


def assert_same(got, want, what):
    (o, k, c), (wo, wk, wc) = got, want
    assert torch.equal(c, wc), f'{what}: counts {c.tolist()} vs {wc.tolist()}'
    assert torch.equal(k, wk), f'{what}: keep differs at {(k != wk).nonzero()[:5].tolist()}'
    assert torch.equal(o, wo), f'{what}: out differs at {(o != wo).nonzero()[:5].tolist()}'


CONFS, IOUS = (0.001, 0.25, 0.4), (0.45, 0.6, 0.7)
CASES = list(itertools.product((1, 4, 16), (37, 300, 512), (1, 10, 80), ('f32', 'bf16')))


@pytest.mark.parametrize('B,nq,nc,dt', CASES)
def test_detect_postprocess_bit_exact(B, nq, nc, dt):
    n = CASES.index((B, nq, nc, dt))
    conf, iou = CONFS[n % 3], IOUS[(n // 3) % 3]
    single_cls = n % 4 == 1
    classes = [c for c in range(0, nc, 3)] if n % 5 == 2 else None
    y = make_preds(B, nq, nc, seed=n)
    if dt == 'bf16':
        y = y.to(torch.bfloat16)
    hw = orig_sizes(B, n)
    got, want = run_both(y, hw, conf, iou, classes, single_cls)
    assert_same(got, want, f'B{B} nq{nq} nc{nc} {dt} conf{conf} iou{iou} single{single_cls} classes{classes}')
    if B > 4:
        assert want[2][3] == 0                                                   # nothing above conf
        score, cls = y[4, :, 4:].float().max(-1)                                 # every box identical: one row per class
        surv = cls[(score > conf) & (torch.isin(cls, torch.tensor(classes)) if classes is not None else True)]
        assert want[2][4] == (min(1, len(surv)) if single_cls else len(surv.unique()))


@pytest.mark.parametrize('dt', ['f32', 'bf16'])
@pytest.mark.parametrize('single_cls,classes', [(False, None), (True, None), (False, [1, 3, 7]), (True, [0, 9]), (False, [])])
def test_detect_postprocess_options(dt, single_cls, classes):
    y = make_preds(6, 300, 10, seed=100)
    if dt == 'bf16':
        y = y.to(torch.bfloat16)
    hw = orig_sizes(6, 100)
    for conf, iou in ((0.001, 0.7), (0.25, 0.45), (0.4, 0.6)):
        got, want = run_both(y, hw, conf, iou, classes, single_cls)
        assert_same(got, want, f'{dt} single{single_cls} classes{classes} conf{conf} iou{iou}')
    if classes == []:
        assert int(want[2].sum()) == 0


def test_threshold_follows_torchvision_double_comparison():
    """IoU exactly fp32(iou): torchvision compares the float IoU with the double threshold.  60/100 rounds to fp32(0.6) > 0.6, so
    the second box goes; 70/100 rounds to fp32(0.7) < 0.7, so it stays."""
    for h2, iou, kept in ((6.0, 0.6, 1), (7.0, 0.7, 2)):
        y = torch.tensor([[[5.0, 5.0, 10.0, 10.0, 0.9], [5.0, h2 / 2, 10.0, h2, 0.8]]])
        got, want = run_both(y, [(1, 1)], 0.25, iou)
        assert int(want[2][0]) == kept
        assert_same(got, want, f'iou {iou}')


def test_negative_conf_and_signed_zero_scores_tie():
    """conf < 0: scores 0.0 and -0.0 tie (stable order by query), negative scores sort below them."""
    y = torch.tensor([[[0.1, 0.1, 0.05, 0.05, -0.0], [0.3, 0.3, 0.05, 0.05, 0.0], [0.5, 0.5, 0.05, 0.05, -0.25],
                       [0.7, 0.7, 0.05, 0.05, -0.0], [0.9, 0.9, 0.05, 0.05, 0.5]]])
    got, want = run_both(y, [(100, 100)], -0.5, 0.7)
    assert want[1][0].tolist() == [4, 0, 1, 3, 2]
    assert_same(got, want, 'negative conf')


def test_detect_postprocess_does_not_synchronise():
    from tamtr_amd import ops
    y = make_preds(4, 300, 10, seed=7).cuda()
    hw_dev = torch.tensor(orig_sizes(4, 7), dtype=torch.int32, device='cuda')
    cls_dev = torch.tensor([1, 2], dtype=torch.int32, device='cuda')
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode('error')
    try:
        a = ops.detect_postprocess(y, hw_dev, 0.25, 0.7, cls_dev)
        b = ops.detect_postprocess(y, orig_sizes(4, 7), 0.25, 0.7, [1, 2])   # host lists: one upload, no sync
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    for u, v in zip(a, b):
        assert torch.equal(u, v)


def test_more_than_512_queries_are_refused():
    from tamtr_amd import TamtrHipError, ops
    with pytest.raises(TamtrHipError):
        ops.detect_postprocess(torch.zeros(1, 513, 14, device='cuda'), [(480, 640)], 0.25, 0.7)


# ------------------------------------------------------------------------------------------------ end to end
SIZES = ((100, 150), (128, 128), (200, 90), (77, 333), (128, 96))
IMGSZ, NC = 128, 10
CONF = 1e-5   # the seeded weights score every class of every query below 5e-4 (median about 4e-5)


def _model():
    sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
    from weights import fill_state
    from tamtr_amd.model import RTDETRDetectionWorldModel
    torch.manual_seed(0)
    model = RTDETRDetectionWorldModel(nc=NC)
    model.load_state_dict(fill_state(model.state_dict(), 78))
    return model


def _images(tmp_path):
    from PIL import Image
    rng = np.random.default_rng(3)
    d = tmp_path / 'images'
    d.mkdir()
    for i, (h, w) in enumerate(SIZES):
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(d / f'im{i}.png')
    return d


def _text_feats():
    g = torch.Generator().manual_seed(11)
    return torch.nn.functional.normalize(torch.randn(NC, 512, generator=g), dim=-1)


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
def test_predictor_end_to_end(tmp_path, dtype):
    from tamtr_amd import data as D
    from tamtr_amd.predict import Predictor
    src = _images(tmp_path)
    names = {i: f'c{i}' for i in range(NC)}
    pred = Predictor(_model().cuda(), names, _text_feats(), imgsz=IMGSZ, conf=CONF, iou=0.7, batch=2, dtype=dtype, keep_raw=True)
    files = sorted(str(p) for p in src.iterdir())
    dets, total = [], 0
    for i, det in enumerate(pred.predict(str(src))):
        assert det.path == files[i]
        k = i % 2
        if k == 0:   # a new batch: its input and raw output are the predictor's last ones
            chunk = files[i:i + 2]
            ims = [D.decode_image(f) for f in chunk]
            hand = np.stack([im if im.shape[:2] == (IMGSZ, IMGSZ) else D.resize_linear_u8(im, IMGSZ, IMGSZ) for im in ims])
            want_img = torch.from_numpy(hand).cuda().permute(0, 3, 1, 2).float() / 255
            assert torch.equal(pred.last_img, want_img)
            y = pred.last_y
            assert y.shape[0] == len(chunk) and y.shape[2] == 4 + NC
            wo, wk, wc = reference_postprocess(y, [im.shape[:2] for im in ims], CONF, 0.7)
        assert det.orig_shape == SIZES[int(os.path.basename(det.path)[2])]
        n = int(wc[k])
        assert torch.equal(det.boxes, wo[k, :n]), f'image {i}'
        total += n
        txt = tmp_path / 'labels' / f'im{i}.txt'
        det.save_txt(txt, save_conf=True)
        if n:
            rows = np.loadtxt(txt, ndmin=2)
            np.testing.assert_array_equal(rows[:, 0], det.cls.numpy())
            np.testing.assert_allclose(rows[:, 1:5], det.xywhn.numpy(), rtol=1e-5, atol=1e-6)
            np.testing.assert_allclose(rows[:, 5], det.conf.numpy(), rtol=1e-5, atol=1e-6)
        else:
            assert not txt.exists()
        dets.append(det)
    assert len(dets) == len(SIZES) and pred.seen == len(SIZES)   # 2 + 2 + a tail batch of 1
    assert total > 0
    assert all(v >= 0 for v in pred.speed().values())


def test_predict_cli_runs_in_a_child_process(tmp_path):
    src = _images(tmp_path)
    sd = _model().state_dict()
    ck = tmp_path / 'best.pt'
    torch.save({'model': sd, 'ema': sd}, ck)
    names = [f'c{i}' for i in range(NC)]
    feats = tmp_path / 'feats.npz'
    np.savez(feats, texts=np.array(names), feats=_text_feats().numpy())
    project = tmp_path / 'runs'
    (project / 'TAMTR').mkdir(parents=True)   # an earlier run: this one goes to TAMTR2
    cmd = [sys.executable, os.path.join(ROOT, 'tools', 'predict.py'), '--weights', str(ck), '--text-feats', str(feats), '--names', ','.join(names),
           '--source', str(src), '--imgsz', str(IMGSZ), '--batch', '2', '--conf', str(CONF), '--save', '--save-txt', '--save-conf',
           '--project', str(project), '--name', 'TAMTR', '--dtype', 'bf16']
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res['images'] == len(SIZES) and res['detections'] > 0
    out = project / 'TAMTR2'
    assert res['save_dir'] == str(out)
    labels = sorted(p.name for p in (out / 'labels').iterdir())
    assert labels and set(labels) <= {f'im{i}.txt' for i in range(len(SIZES))}
    assert sum(len(open(out / 'labels' / p).read().splitlines()) for p in labels) == res['detections']
    assert sorted(p.name for p in out.glob('*.png')) == [f'im{i}.png' for i in range(len(SIZES))]
    assert set(res['ms_per_image']) == {'load', 'forward', 'postprocess'}
