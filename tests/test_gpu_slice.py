"""GPU: sliced prediction.  tamtr_slice_views (csrc/slice.hip) bit-exact against slicing.views_host on every branch of the resize
rule, tamtr_slice_merge bit-exact against slicing.merge_host (whose claims test_slice_host.py checks on the CPU), and the predictor /
CLI end to end."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from test_gpu_predict import CONF, NC, _model, _text_feats, make_preds
from test_slice_host import abi_argument_checks, in_window

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ the view kernel
WINDOWS_32 = [(10, 20, 42, 52),       # 32 x 32: the copy
              (30, 5, 94, 69),        # 64 x 64: the 2 x 2 mean
              (50, 40, 70, 67),       # 20 x 27, upscaled
              (20, 30, 110, 80),      # 90 x 50, downscaled, not square
              (0, 10, 40, 60), (15, 0, 75, 45), (91, 20, 131, 70), (30, 57, 100, 97),      # touching the left, top, right, bottom border
              (99, 65, 131, 97), (67, 33, 131, 97),      # the copy and the mean in the frame's last corner
              (60, 10, 61, 50), (10, 60, 70, 61), (130, 96, 131, 97),      # one pixel wide, one pixel high, the last pixel
              (0, 0, 131, 97)]        # the whole frame
WINDOWS_64 = [(0, 0, 128, 64),        # 2S wide, S high: the mean's size on one axis only - the general rule
              (0, 0, 64, 64), (64, 0, 128, 64), (3, 2, 100, 61), (0, 0, 128, 32)]


@pytest.mark.parametrize('h,w,S,windows', [(97, 131, 32, WINDOWS_32), (64, 128, 64, WINDOWS_64)])
def test_views_bit_exact(h, w, S, windows):
    from tamtr_amd import ops, slicing
    im = np.random.default_rng(h + w).integers(0, 256, (h, w, 3), dtype=np.uint8)
    want = slicing.views_host(im, windows, S)
    got = ops.slice_views(torch.from_numpy(im).cuda(), windows, S)      # all windows in one launch
    torch.cuda.synchronize()
    got = got.cpu()
    assert got.shape == want.shape == (len(windows), 3, S, S) and got.dtype == torch.float32
    for v, win in enumerate(windows):
        bad = (got[v] != want[v]).nonzero()
        assert not len(bad), f'window {win}: {len(bad)} values differ, first at {bad[0].tolist()}: {got[v][tuple(bad[0])]} vs {want[v][tuple(bad[0])]}'
    # into a slice of a larger tensor, as sliced_forward calls it
    buf = torch.full((len(windows) + 2, 3, S, S), -1.0, device='cuda')
    ops.slice_views(torch.from_numpy(im).cuda(), windows, S, out=buf[1:-1])
    assert torch.equal(buf[1:-1].cpu(), want) and (buf[0] == -1).all() and (buf[-1] == -1).all()


# ------------------------------------------------------------------------------------------------ the merge kernel
NQ, MNC = 40, 3
FRAMES = [(50, 60), (64, 150), (100, 190)]      # at slice 64, overlap 0.2: 1, 1 + 3 and 1 + 2 x 4 views


def merge_case(dtype=torch.float32):
    """B = 3 frames owning 1, 4 and 9 views of make_preds' edge images (heavy overlap, duplicated rows, a NaN score, zero-width boxes,
    identical boxes, scores on a coarse grid), with, planted in frame 2: one object seen by the whole-frame view and by two
    overlapping windows at EQUAL scores (the lower candidate must win), and one seen by two windows at different scores.  Frame 0's
    scores lie below every tested conf.  -> (y [14, NQ, 4 + MNC], view_off, windows [14, 4], hws)."""
    from tamtr_amd.slicing import slice_windows
    wins = [slice_windows(h, w, 64, 0.2) for h, w in FRAMES]
    assert [len(w) for w in wins] == [1, 4, 9]
    off = np.concatenate([[0], np.cumsum([len(w) for w in wins])]).tolist()
    y = make_preds(14, NQ, MNC, seed=21)
    y[0, :, 4:] *= 0.0009
    y[off[2]:, :, 4:] *= 0.9         # the planted rows lead their frame
    h, w = FRAMES[2]
    w2 = wins[2].tolist()
    assert w2[1] == [0, 0, 64, 64] and w2[2] == [52, 0, 116, 64]
    tie = (58 / w, 30 / h, 10 / w, 10 / h)      # pixels x 53 .. 63: inside windows 1 and 2
    for v, score in ((0, 0.97), (1, 0.99), (2, 0.99)):
        y[off[2] + v, 0, :4] = torch.tensor(in_window(tie, w2[v], (h, w)))
        y[off[2] + v, 0, 4:] = torch.tensor([0.0, score, 0.0])
    two = (57 / w, 50 / h, 8 / w, 12 / h)
    for v, score in ((1, 0.93), (2, 0.96)):
        y[off[2] + v, 1, :4] = torch.tensor(in_window(two, w2[v], (h, w)))
        y[off[2] + v, 1, 4:] = torch.tensor([score, 0.0, 0.0])
    return y.to(dtype), off, np.concatenate(wins), FRAMES


def run_both(y, off, wins, hws, conf, iou, classes=None, single_cls=False, match='iou', max_out=512):
    from tamtr_amd import ops, slicing
    got = ops.slice_merge(y.cuda(), off, wins, hws, conf, iou, classes, single_cls, match, max_out=max_out)
    torch.cuda.synchronize()
    return tuple(t.cpu() for t in got), slicing.merge_host(y, off, wins, hws, conf, iou, classes, single_cls, match, max_out=max_out)


def assert_same(got, want, what):
    for g, w, name in zip(got, want, ('ym', 'src', 'counts', 'dropped', 'overflow')):
        assert g.dtype == w.dtype and g.shape == w.shape, f'{what}: {name} {g.dtype}{tuple(g.shape)} vs {w.dtype}{tuple(w.shape)}'
        assert torch.equal(g, w), f'{what}: {name} differs at {(g != w).nonzero()[:5].tolist()}'


@pytest.mark.parametrize('dt', ['f32', 'bf16'])
@pytest.mark.parametrize('conf,iou,classes,single_cls,match', [(0.25, 0.7, None, False, 'iou'), (0.25, 0.7, None, False, 'ios'),
                                                               (0.25, 0.7, [0, 1], True, 'ios'), (0.4, 0.45, [1], False, 'iou'),
                                                               (0.25, 0.7, [], False, 'iou')])
def test_merge_bit_exact(conf, iou, classes, single_cls, match, dt):
    y, off, wins, hws = merge_case(torch.bfloat16 if dt == 'bf16' else torch.float32)
    got, want = run_both(y, off, wins, hws, conf, iou, classes, single_cls, match)
    what = f'{dt} conf{conf} iou{iou} classes{classes} single{single_cls} {match}'
    assert_same(got, want, what)
    ym, src, counts, dropped, overflow = want
    assert counts[0] == 0 and dropped.tolist() == [0] * 3 and overflow.tolist() == [0] * 3, 'conditions of the test'
    if classes != []:
        assert counts[1] > 0 and counts[2] > 3
        s2 = src[2, :counts[2]].tolist()
        assert s2[0] == 1 * NQ + 0 and 0 not in s2 and 2 * NQ not in s2, 'the tie between views 1 and 2 goes to the lower candidate'
        assert (2 * NQ + 1 in s2 and 1 * NQ + 1 not in s2) or 0 not in (classes or [0])


@pytest.mark.parametrize('dt', ['f32', 'bf16'])
def test_merge_with_max_out_8_reports_what_it_dropped(dt):
    y, off, wins, hws = merge_case(torch.bfloat16 if dt == 'bf16' else torch.float32)
    got, want = run_both(y, off, wins, hws, 0.25, 0.7, max_out=8)
    assert want[3][0] == 0 and (want[3][1:] > 0).all() and want[2].tolist() == [0, 8, 8] and got[0].shape == (3, 8, 4 + MNC)
    assert_same(got, want, f'max_out 8 {dt}')
    full = run_both(y, off, wins, hws, 0.25, 0.7)[0]
    assert torch.equal(got[3], (full[2] + full[3] - 8).clamp(min=0)) and torch.equal(got[0], full[0][:, :8])


def test_more_passing_candidates_than_the_table_holds():
    """64 views x nq 300 at conf 0: nearly all of frame 0's 19200 candidates pass, the first 4096 go on, the others - the highest
    indices - are counted; frame 1 (three views) is not touched by it."""
    from tamtr_amd import ops
    from tamtr_amd.slicing import slice_windows
    wins = [slice_windows(448, 576, 64, 0.0), slice_windows(60, 100, 64, 0.2)]
    assert [len(w) for w in wins] == [64, 3]
    y = make_preds(67, 300, MNC, seed=8)
    off, hws = [0, 64, 67], [(448, 576), (60, 100)]
    got, want = run_both(y, off, np.concatenate(wins), hws, 0.0, 0.7)
    passing = int((y[:64, :, 4:].max(-1).values > 0).sum())
    assert passing > 19000 and want[4].tolist() == [passing - ops.SLICE_MAX_CAND, 0] and int(want[1][0].max()) < 4200 and want[2][1] > 0
    assert_same(got, want, 'overflow')


def test_threshold_follows_torchvision_double_comparison():
    """As test_gpu_tta's: 60/100 rounds to fp32(0.6) > 0.6, so the second view's box goes; 70/100 rounds to fp32(0.7) < 0.7 - for
    IoU and, with the second box inside the first (inter / smaller = inter / its own area = 1), never for IoS below 1."""
    full = [(0, 0, 10, 10)] * 2
    for h2, iou, match, kept in ((6.0, 0.6, 'iou', 1), (7.0, 0.7, 'iou', 2), (7.0, 0.7, 'ios', 1), (7.0, 1.0, 'ios', 2)):
        y = torch.tensor([[[5.0, 5.0, 10.0, 10.0, 0.9]], [[5.0, h2 / 2, 10.0, h2, 0.8]]])
        got, want = run_both(y, [0, 2], full, [(10, 10)], 0.25, iou, match=match, max_out=4)
        assert int(want[2][0]) == kept, (h2, iou, match)
        assert_same(got, want, f'iou {iou} {match}')


def test_merge_and_views_do_not_synchronise():
    from tamtr_amd import ops
    y, off, wins, hws = merge_case()
    y = y.cuda()
    im = torch.randint(0, 256, (97, 131, 3), dtype=torch.uint8).cuda()
    cls_dev = torch.tensor([0, 1], dtype=torch.int32, device='cuda')
    ops.slice_merge(y, off, wins, hws, 0.25, 0.7)      # first call: library load, allocator warm-up
    ops.slice_views(im, WINDOWS_32, 32)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode('error')
    try:
        a = ops.slice_merge(y, off, wins, hws, 0.25, 0.7, cls_dev)
        b = ops.slice_merge(y, off, wins, hws, 0.25, 0.7, [0, 1])      # host lists: one upload, no sync
        ops.slice_views(im, WINDOWS_32, 32)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    for u, v in zip(a, b):
        assert torch.equal(u, v)


def test_arguments_are_checked_through_the_abi():
    from tamtr_amd import TamtrHipError, ops
    abi_argument_checks()
    im = torch.zeros(20, 30, 3, dtype=torch.uint8, device='cuda')
    for bad in ([(0, 0, 31, 20)], [(0, 0, 30, 21)], [(5, 5, 5, 10)], [(0, 0, 30, 20)] * 65, []):
        with pytest.raises(TamtrHipError):
            ops.slice_views(im, bad, 16)
    with pytest.raises(TamtrHipError):
        ops.slice_views(im.float(), [(0, 0, 30, 20)], 16)
    y = torch.zeros(66, 5, 7, device='cuda')
    full = [(0, 0, 30, 20)]
    with pytest.raises(TamtrHipError):
        ops.slice_merge(y, [0, 65, 66], full * 66, [(20, 30)] * 2, 0.25, 0.7)      # 65 views in one frame
    with pytest.raises(TamtrHipError):
        ops.slice_merge(torch.zeros(2, 513, 7, device='cuda'), [0, 2], full * 2, [(20, 30)], 0.25, 0.7)      # nq 513
    with pytest.raises(TamtrHipError):
        ops.slice_merge(y[:2], [0, 2], full * 2, [(20, 30)], 0.25, 0.7, max_out=513)
    with pytest.raises(TamtrHipError):
        ops.slice_merge(y[:2], [0, 2], full * 3, [(20, 30)], 0.25, 0.7)      # two outputs, three windows
    with pytest.raises(TamtrHipError):
        ops.slice_merge(y[:2], [0, 2], full * 2, [(20, 30)], 0.25, 0.7, match='giou')


# ------------------------------------------------------------------------------------------------ end to end
IMGSZ, SLICE = 128, 64      # 64-pixel windows of the frame, magnified twice for the network (see the docstring below)
E2E_SIZES = ((100, 130), (50, 60))      # 1 + 2 x 3 views; smaller than the slice: the whole frame alone


@pytest.fixture(scope='module')
def model():
    return _model().cuda()


def _predictor(model, **kw):
    from tamtr_amd.predict import Predictor
    names = {i: f'c{i}' for i in range(NC)}
    return Predictor(model, names, _text_feats(), imgsz=IMGSZ, conf=CONF, iou=0.7, batch=4, dtype='fp32', keep_raw=True, **kw)


def _frames(tmp_path):
    from PIL import Image
    rng = np.random.default_rng(5)
    d = tmp_path / 'frames'
    d.mkdir()
    for i, (h, w) in enumerate(E2E_SIZES):
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(d / f'im{i}.png')
    return d


def test_track_and_augment_refuse_slice(model):
    pred = _predictor(model, slice=SLICE)
    with pytest.raises(ValueError):
        pred.track('nowhere/')      # refused when called, before any file is looked for
    with pytest.raises(ValueError):
        pred.track_streams(['nowhere/'])
    with pytest.raises(ValueError):
        _predictor(model, slice=SLICE, augment=True)
    with pytest.raises(ValueError):
        _predictor(model, slice=SLICE, slice_overlap=1.0)
    with pytest.raises(ValueError):
        _predictor(model, slice=SLICE, slice_match='giou')
    assert 'slice' in pred.times and 'slice' not in _predictor(model).times and pred.slice == (SLICE, SLICE)


@pytest.mark.parametrize('match', ['iou', 'ios'])
def test_predictor_with_slices(model, tmp_path, match):
    """imgsz 128 with 64-pixel slices, not the 64 / 32 one might pick for speed: at 64 x 64 the three feature maps hold 84 tokens, fewer
    than the decoder's 300 queries, and the model's top-k has nothing to pick from (128 x 128: 336 tokens)."""
    from tamtr_amd import data as D, ops, slicing
    src = _frames(tmp_path)
    files = sorted(str(p) for p in src.iterdir())
    pred = _predictor(model, slice=SLICE, slice_match=match)
    dets = list(pred.predict(str(src)))      # one batch: both frames, 7 + 1 views, two forwards of 4
    ims = [D.decode_image(f) for f in files]
    hw = [im.shape[:2] for im in ims]
    wins = [slicing.slice_windows(h, w, SLICE, 0.2) for h, w in hw]
    assert [len(w) for w in wins] == [7, 1] and [d.orig_shape for d in dets] == list(E2E_SIZES)
    want_views = torch.cat([slicing.views_host(im, w, IMGSZ) for im, w in zip(ims, wins)])
    assert pred.last_views.shape == (8, 3, IMGSZ, IMGSZ) and torch.equal(pred.last_views.cpu(), want_views)
    assert pred.last_ys.shape[0] == 8 and pred.last_ys.shape[2] == 4 + NC and pred.last_img is None
    ym, _, counts, dropped, overflow = slicing.merge_host(pred.last_ys, [0, 7, 8], np.concatenate(wins), hw, CONF, 0.7, match=match)
    assert torch.equal(pred.last_y.cpu(), ym) and overflow.tolist() == [0, 0] and dropped[1] == 0      # (frame 0 may fill all 512 rows)
    out, _, cnt = ops.detect_postprocess(ym.cuda(), hw, CONF, 0.7)
    out, cnt = out.cpu(), cnt.cpu()
    print(f'sliced predictor ({match}): merged rows {counts.tolist()}, detections {cnt.tolist()}')
    assert torch.equal(cnt, counts), 'the second NMS, at the same threshold, removes nothing'
    for k, det in enumerate(dets):
        assert torch.equal(det.boxes, out[k, :int(cnt[k])]), f'frame {k}'
    assert int(cnt.min()) > 0 and pred.seen == 2 and pred.slice_dropped == int(dropped.sum())
    sp = pred.speed()
    assert sp['slice'] > 0 and all(v >= 0 for v in sp.values())


def test_without_slice_nothing_changes(model, tmp_path):
    """Predictor(slice=None) is the plain predictor: the same keys of times, the hand-made network input bit for bit, and on its own
    forward exactly the plain postprocess; against a second plain predictor the same rows and classes (two forwards: the trunk is not
    reproducible bit for bit from one call to the next, see test_gpu_tta, so the boxes are compared to 1e-3 pixels)."""
    from tamtr_amd import data as D, ops
    src = _frames(tmp_path)
    files = sorted(str(p) for p in src.iterdir())
    a, b = _predictor(model, slice=None), _predictor(model)
    da, db = list(a.predict(str(src))), list(b.predict(str(src)))
    assert set(a.times) == set(b.times) == {'load', 'h2d', 'forward', 'postprocess', 'track', 'd2h'} and a.slice is None and a.last_views is None
    ims = [D.decode_image(f) for f in files]
    hand = np.stack([D.resize_linear_u8(im, IMGSZ, IMGSZ) for im in ims])
    assert torch.equal(a.last_img, torch.from_numpy(hand).cuda().permute(0, 3, 1, 2).float() / 255)
    out, _, cnt = ops.detect_postprocess(a.last_y, [im.shape[:2] for im in ims], CONF, 0.7)
    for k, (x, y) in enumerate(zip(da, db)):
        assert torch.equal(x.boxes, out[k, :int(cnt[k])].cpu()) and len(x) > 0, f'frame {k}'
        assert x.boxes.shape == y.boxes.shape, f'frame {k}'
        xs, ys = (t.boxes.numpy()[np.lexsort((t.boxes[:, 1].numpy(), t.boxes[:, 0].numpy(), t.boxes[:, 5].numpy()))] for t in (x, y))
        assert np.array_equal(xs[:, 5], ys[:, 5]) and float(np.abs(xs - ys).max()) < 1e-3, f'frame {k}'      # as sets: near-tied scores may swap


def test_predict_cli_with_slice_writes_the_in_process_labels(model, tmp_path):
    src = _frames(tmp_path)
    sd = _model().state_dict()
    ck = tmp_path / 'best.pt'
    torch.save({'model': sd, 'ema': sd}, ck)
    names = [f'c{i}' for i in range(NC)]
    feats = tmp_path / 'feats.npz'
    np.savez(feats, texts=np.array(names), feats=_text_feats().numpy())
    project = tmp_path / 'runs'
    cmd = [sys.executable, os.path.join(ROOT, 'tools', 'predict.py'), '--weights', str(ck), '--text-feats', str(feats), '--names', ','.join(names),
           '--source', str(src), '--imgsz', str(IMGSZ), '--batch', '4', '--conf', str(CONF), '--save-txt', '--save-conf', '--project', str(project),
           '--name', 'SL', '--dtype', 'fp32', '--slice', str(SLICE), '--slice-match', 'ios']
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res['images'] == 2 and res['detections'] > 0 and res['slice'] == [SLICE, SLICE] and res['slice_dropped'] >= 0
    assert res['views_per_image'] == 4.0 and res['slice_match'] == 'ios'
    assert set(res['ms_per_image']) == {'load', 'forward', 'slice', 'postprocess'}
    here = tmp_path / 'here'
    n = 0
    for det in _predictor(model, slice=SLICE, slice_match='ios').predict(str(src)):
        det.save_txt(here / (os.path.splitext(os.path.basename(det.path))[0] + '.txt'), save_conf=True)
        n += len(det)
    assert n == res['detections']
    labels = sorted(p.name for p in (project / 'SL' / 'labels').iterdir())
    assert labels == sorted(p.name for p in here.iterdir()) and labels
    for name in labels:      # two processes, two forwards: the trunk is not reproducible bit for bit, '%g' keeps six digits; and two
        # scores that differ in the last bits may change places from one forward to the next, so the rows are compared as sets
        a, b = np.loadtxt(project / 'SL' / 'labels' / name, ndmin=2), np.loadtxt(here / name, ndmin=2)
        assert a.shape == b.shape, name
        a, b = a[np.lexsort((a[:, 2], a[:, 1], a[:, 0]))], b[np.lexsort((b[:, 2], b[:, 1], b[:, 0]))]
        assert np.array_equal(a[:, 0], b[:, 0]), name
        np.testing.assert_allclose(a[:, 1:], b[:, 1:], rtol=1e-5, atol=1e-6, err_msg=name)      # test_gpu_predict's label-file tolerance
