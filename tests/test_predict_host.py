"""CPU: the predictor's host side (tam-tr_amd/predict.py, tools/predict.py) and the argument checks of tamtr_detect_postprocess,
plus the restated postprocess rule the GPU suite (test_gpu_predict.py) checks the kernel against."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT


# ------------------------------------------------------------------------------------------------ the restated rule
def reference_nms(boxes, scores, iou):
    """torchvision.ops.nms as its CPU kernel computes it (fp32 boxes, IoU without eps, `iou_f32 > iou` compared in double),
    scores sorted descending and stable.  -> indices into boxes, in keep order."""
    order = scores.sort(descending=True, stable=True).indices
    b = boxes[order]
    x1, y1, x2, y2 = b.unbind(1)
    areas = (x2 - x1) * (y2 - y1)
    n = len(order)
    later = torch.arange(n)
    suppressed = torch.zeros(n, dtype=torch.bool)
    keep = []
    zero = torch.zeros((), dtype=torch.float32)
    for i in range(n):
        if suppressed[i]:
            continue
        keep.append(i)
        xx1 = torch.where(x1[i] < x1, x1, x1[i])      # std::max(ix1, x1[j])
        yy1 = torch.where(y1[i] < y1, y1, y1[i])
        xx2 = torch.where(x2 < x2[i], x2, x2[i])      # std::min(ix2, x2[j])
        yy2 = torch.where(y2 < y2[i], y2, y2[i])
        dx, dy = xx2 - xx1, yy2 - yy1
        w = torch.where(zero < dx, dx, zero)
        h = torch.where(zero < dy, dy, zero)
        inter = w * h
        ovr = inter / ((areas[i] + areas) - inter)
        suppressed |= (ovr.double() > iou) & (later > i)
    return order[torch.as_tensor(keep, dtype=torch.long)]


def reference_postprocess(y, orig_hw, conf, iou, classes=None, single_cls=False, max_wh=7680):
    """RTDETRPredictor.postprocess, ultralytics/models/rtdetrworld/predict.py:34-78, restated on the CPU in fp32 for y [B, nq, 4 + nc]
    (widened to fp32 first), in the kernel's output form: out [B, nq, 6] (zero after the count), keep [B, nq] (-1 after), counts [B]."""
    y = y.detach().cpu().float()
    B, nq, _ = y.shape
    out = torch.zeros(B, nq, 6)
    keep = torch.full((B, nq), -1, dtype=torch.int32)
    counts = torch.zeros(B, dtype=torch.int32)
    for i in range(B):
        bbox, scores = y[i, :, :4], y[i, :, 4:]
        dw, dh = bbox[:, 2] / 2, bbox[:, 3] / 2                                   # xywh2xyxy, utils/ops.py:360-380
        xyxy = torch.stack([bbox[:, 0] - dw, bbox[:, 1] - dh, bbox[:, 0] + dw, bbox[:, 1] + dh], 1)
        score, cls = scores.max(-1)
        idx = score > conf
        if classes is not None:
            idx = (cls[:, None] == torch.tensor(classes, dtype=torch.long)).any(1) & idx
        q = idx.nonzero().view(-1)
        pred = torch.cat([xyxy, score[:, None], cls[:, None].float()], -1)[q]
        b = pred[:, :4] + pred[:, 5:6] * (0 if single_cls else max_wh)
        oi = reference_nms(b, pred[:, 4], iou)
        rows = pred[oi]
        oh, ow = orig_hw[i]
        rows[:, [0, 2]] *= ow
        rows[:, [1, 3]] *= oh
        n = len(oi)
        out[i, :n] = rows
        keep[i, :n] = q[oi].to(torch.int32)
        counts[i] = n
    return out, keep, counts


def test_restated_nms_keeps_what_engine_nms_keeps():
    """Self-check of the oracle on untied random boxes: the same rows as the project's host NMS, in the same order."""
    from tamtr_amd.engine import nms
    g = torch.Generator().manual_seed(0)
    for n, thr in ((37, 0.45), (300, 0.6), (300, 0.7), (512, 0.7)):
        xy = torch.rand(n, 2, generator=g) * 40
        wh = torch.rand(n, 2, generator=g) * 30 + 1
        boxes = torch.cat([xy, xy + wh], 1)
        scores = torch.rand(n, generator=g)
        assert len(scores.unique()) == n
        got = reference_nms(boxes, scores, thr)
        want = nms(boxes, scores, thr)
        assert 0 < len(got) < n
        assert torch.equal(got, want)


def test_restated_rule_shifts_boxes_by_class_and_scales_to_the_image():
    # two identical boxes of different classes both survive class-aware NMS, one survives class-agnostic NMS
    y = torch.tensor([[[0.5, 0.5, 0.25, 0.5, 0.875, 0.125], [0.5, 0.5, 0.25, 0.5, 0.125, 0.75], [0.5, 0.5, 0.25, 0.5, 0.125, 0.125]]])
    out, keep, counts = reference_postprocess(y, [(100, 200)], 0.25, 0.7)
    assert counts.tolist() == [2] and keep[0].tolist() == [0, 1, -1]
    assert torch.equal(out[0, 0], torch.tensor([75., 25., 125., 75., 0.875, 0.]))
    assert torch.equal(out[0, 2], torch.zeros(6))
    _, keep, counts = reference_postprocess(y, [(100, 200)], 0.25, 0.7, single_cls=True)
    assert counts.tolist() == [1] and keep[0].tolist() == [0, -1, -1]
    _, keep, counts = reference_postprocess(y, [(100, 200)], 0.25, 0.7, classes=[1])
    assert counts.tolist() == [1] and keep[0].tolist() == [1, -1, -1]


# ------------------------------------------------------------------------------------------------ results and files
def test_save_txt_writes_the_reference_format(tmp_path):
    from tamtr_amd.predict import Detections
    boxes = torch.tensor([[10., 20., 50., 80., 0.875, 3.], [0., 0., 200., 100., 0.5, 0.]])
    d = Detections('a.jpg', (100, 200), {0: 'x', 3: 'y'}, boxes)
    f = tmp_path / 'labels' / 'a.txt'
    d.save_txt(f)
    assert f.read_text() == '3 0.15 0.5 0.2 0.6\n0 0.5 0.5 1 1\n'
    d.save_txt(f, save_conf=True)   # append mode, as the reference opens it
    assert f.read_text().splitlines()[2:] == ['3 0.15 0.5 0.2 0.6 0.875', '0 0.5 0.5 1 1 0.5']
    empty = Detections('b.jpg', (100, 200), {0: 'x'}, torch.zeros(0, 6))
    empty.save_txt(tmp_path / 'labels' / 'b.txt')
    assert not (tmp_path / 'labels' / 'b.txt').exists()
    np.testing.assert_array_equal(d.xywhn.numpy(), np.float32([[0.15, 0.5, 0.2, 0.6], [0.5, 0.5, 1, 1]]))
    assert d.cls.tolist() == [3., 0.] and d.conf.tolist() == [0.875, 0.5]


def test_save_draws_an_annotated_copy(tmp_path):
    from PIL import Image
    from tamtr_amd.predict import Detections
    im = np.full((60, 90, 3), 128, np.uint8)
    d = Detections('a.png', (60, 90), {0: 'car'}, torch.tensor([[10., 10., 50., 40., 0.9, 0.]]), orig_img=im)
    d.save(tmp_path / 'a.png')
    out = np.asarray(Image.open(tmp_path / 'a.png'))
    assert out.shape == im.shape and (out != 128).any()


def test_preprocess_is_a_scale_fill_resize(tmp_path):
    from PIL import Image
    from tamtr_amd import data as D
    from tamtr_amd.predict import letterbox_scalefill, load_image, to_model_input
    rng = np.random.default_rng(0)
    src = rng.integers(0, 256, (300, 500, 3), dtype=np.uint8)
    Image.fromarray(src).save(tmp_path / 'a.png')
    orig, inp = load_image(str(tmp_path / 'a.png'), 64)
    assert np.array_equal(orig, src) and inp.shape == (64, 64, 3)
    x = to_model_input(np.stack([inp]), torch.device('cpu'))
    want = torch.from_numpy(D.resize_linear_u8(src, 64, 64)).permute(2, 0, 1).float() / 255
    assert x.shape == (1, 3, 64, 64) and x.dtype == torch.float32 and torch.equal(x[0], want)
    same = rng.integers(0, 256, (64, 64, 3), dtype=np.uint8)
    assert letterbox_scalefill(same, 64) is same   # already at imgsz: not resampled


def test_sources_and_save_dir_increment(tmp_path):
    from PIL import Image
    from tamtr_amd.predict import increment_path, list_sources
    d = tmp_path / 'imgs'
    (d / 'sub').mkdir(parents=True)
    for p in ('b.png', 'a.jpg', 'sub/c.png'):
        Image.fromarray(np.zeros((8, 8, 3), np.uint8)).save(d / p)
    (d / 'notes.txt').write_text('x')
    assert list_sources(str(d)) == sorted(str(d / p) for p in ('a.jpg', 'b.png', 'sub/c.png'))
    assert list_sources(str(d / 'b.png')) == [str(d / 'b.png')]   # an image file, not a list file
    base = tmp_path / 'runs' / 'TAMTR'
    assert increment_path(base) == base
    base.mkdir(parents=True)
    assert str(increment_path(base)) == str(base) + '2'
    (tmp_path / 'runs' / 'TAMTR2').mkdir()
    assert str(increment_path(base, mkdir=True)) == str(base) + '3' and (tmp_path / 'runs' / 'TAMTR3').is_dir()
    assert increment_path(base, exist_ok=True) == base


def test_predict_cli_help_runs_without_a_gpu():
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'predict.py'), '--help'], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    for flag in ('--weights', '--text-feats', '--source', '--save-txt', '--single-cls', '--classes', '--project', '--dtype'):
        assert flag in r.stdout


# ------------------------------------------------------------------------------------------------ the packed copy and the batch records
def test_to_host_makes_one_cat_and_returns_aligned_views_of_every_part(monkeypatch):
    """The uint8 part is 60 bytes long: without padding everything after it would start at an odd multiple of 4."""
    from tamtr_amd._lib import to_host
    g = torch.Generator().manual_seed(0)
    parts = {'out': torch.randn(2, 3, 6, generator=g), 'hits': torch.randint(0, 256, (2, 3, 10), generator=g, dtype=torch.uint8),
             'counts': torch.tensor([3, -7], dtype=torch.int32), 'curve': torch.randn(5, generator=g, dtype=torch.float64),
             'keys': torch.tensor([2 ** 40, -1, 5]), 'none': torch.zeros(0, 6)}
    assert [t.dtype for t in parts.values()] == [torch.float32, torch.uint8, torch.int32, torch.float64, torch.int64, torch.float32]
    want = {k: t.clone() for k, t in parts.items()}
    cats, cat = [], torch.cat
    monkeypatch.setattr(torch, 'cat', lambda *a, **kw: cats.append(1) or cat(*a, **kw))
    host = to_host(parts)
    monkeypatch.undo()
    assert len(cats) == 1 and list(host) == list(parts)
    for k, t in want.items():
        a = host[k]
        assert isinstance(a, np.ndarray) and a.dtype == t.numpy().dtype and a.shape == tuple(t.shape), k
        assert np.array_equal(a, t.numpy()) and a.ctypes.data % 8 == 0, k
    assert to_host({}) == {}


def test_batch_records_of_a_sequence_are_plain_chunks():
    from tamtr_amd.predict import sequence_records
    files = [f'{i}.png' for i in range(5)]
    gt = [np.full((1, 7), i, np.float32) for i in range(4)]      # the fifth frame's is missing: empty
    plain = sequence_records(files, 2)
    assert [r[0] for r in plain] == [files[0:2], files[2:4], files[4:5]]
    assert all(r[1:] == (None, None, []) for r in plain)
    scored = sequence_records(files, 2, gt)
    assert [(r[0], r[1], r[3]) for r in scored] == [(r[0], None, []) for r in plain]
    for r, (a, b) in zip(scored, ((0, 2), (2, 4), (4, 5))):
        assert len(r[2]) == b - a and all(g is w for g, w in zip(r[2], gt[a:b]))
    assert scored[2][2][0].shape == (0, 7) and scored[2][2][0].dtype == np.float32
    assert sequence_records([], 2) == [] and len(sequence_records(files, 2, gt + gt)[2][2]) == 1      # surplus ground truth is cut


def test_batch_records_of_streams_follow_stream_batches():
    from tamtr_amd.predict import stream_batches, stream_records
    files = [['a0', 'a1', 'a2'], ['b0']]
    gt = [[np.full((1, 7), i, np.float32) for i in range(3)], [np.full((2, 7), 9, np.float32)]]
    batches = stream_batches(files, 2)
    assert [a for _, a in batches] == [[True, True, True, False], [True, False, False, False]]
    plain = stream_records(files, 2)
    assert [(r[0], r[1]) for r in plain] == batches and all(r[2:] == (None, []) for r in plain)
    scored = stream_records(files, 2, gt)
    assert [(r[0], r[1]) for r in scored] == batches
    (f0, e0), (f1, e1) = [r[2:] for r in scored]
    assert f0[0] is gt[0][0] and f0[1] is gt[1][0] and f0[2] is gt[0][1] and f0[3] is None and e0 == [1]
    assert f1[0] is gt[0][2] and f1[1:] == [None, None, None] and e1 == [0]
    half = stream_records(files, 2, [gt[0], None])      # a stream that is not scored is no frame to the evaluators and never ends
    assert [[g is not None for g in r[2]] for r in half] == [[True, False, True, False], [True, False, False, False]]
    assert [r[3] for r in half] == [[], [0]]


# ------------------------------------------------------------------------------------------------ the C ABI without a GPU
def _lib():
    import tamtr_amd
    from tamtr_amd import _lib
    if not os.path.exists(tamtr_amd.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


def test_detect_postprocess_arguments_are_checked_before_any_launch():
    h = _lib()
    z, one = ctypes.c_void_p(0), ctypes.c_void_p(16)   # one: non-null, never dereferenced (the checks come first)
    f = h.tamtr_detect_postprocess

    def call(preds=one, dtype=0, B=2, nq=300, nd=14, hw=one, classes=z, n_classes=0, out=one, keep=one, counts=one):
        return f(preds, dtype, B, nq, nd, hw, 0.25, 0.7, 0, 7680.0, classes, n_classes, out, keep, counts, z)

    for k in ('preds', 'hw', 'out', 'keep', 'counts'):
        assert call(**{k: z}) == -1, k
    assert call(nd=4) == -1 and call(B=0) == -1 and call(nq=0) == -1 and call(n_classes=-1) == -1 and call(dtype=2) == -1
    assert call(nq=513) == -2 and call(nq=513, dtype=1) == -2
    assert call(nq=513, preds=z) == -1


def test_detect_postprocess_refuses_cpu_tensors():
    import tamtr_amd.ops as ops
    from tamtr_amd import TamtrHipError
    with pytest.raises(TamtrHipError):
        ops.detect_postprocess(torch.zeros(1, 300, 14), [(480, 640)], 0.25, 0.7)
