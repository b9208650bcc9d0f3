"""GPU: tamtr_val_confusion (csrc/confusion.hip) against engine.ConfusionMatrix fed the same predn / counts the matching op produced and
the same labels - exact integer equality throughout; accumulation, repeatability, DeviceValidator(confusion=True), validate(confusion=True)
and tools/val.py --confusion end to end."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from test_confusion_host import CM, confusion_rule
from test_val_host import make_case, orig_shapes

pytestmark = pytest.mark.gpu

IMGSZ = 640
F = np.float32
LABELS = (0, 1, 7, 513, 1100)          # per image: none, one, a few, one past the tile of 512, three tiles


def run_both(y, cls, boxes, bidx, hw, nc, conf=0.001, bf16=False, device_labels=False, single_cls=False, matrix=None, cm=None):
    """The matching op, then the confusion op on its outputs -> (kernel matrix i32 tensor on the device, engine.ConfusionMatrix fed the
    same predn / counts, counts)."""
    from tamtr_amd import engine as E, ops
    yd = torch.from_numpy(y).cuda()
    if bf16:
        yd = yd.to(torch.bfloat16)
    lab = (cls.cuda(), boxes.cuda(), bidx.cuda()) if device_labels else (cls, boxes, bidx)
    out = ops.val_postprocess_match(yd, *lab, hw, IMGSZ, conf, 0.7, single_cls, return_device_labels=True)
    assert len(out) == 6
    if matrix is None:
        matrix = torch.zeros(nc + 1, nc + 1, dtype=torch.int32, device='cuda')
    ops.val_confusion(out[0], out[2], out[5], nc, E.cm_conf(conf), 0.45, matrix)
    torch.cuda.synchronize()
    cm = confusion_rule(out[0].cpu(), out[2].cpu(), cls, boxes, bidx, hw, IMGSZ, nc, conf, matrix=cm)
    return matrix, cm, out[2].cpu().numpy()


def special_images(y, cls, boxes, bidx, B, k):
    """In a batch of three: image 1 loses every score above 0.25 (exact scaling by 1/4, scores stay above the validator's conf) or every
    score above the validator's conf (counts == 0), image 2 gets its labels moved into a corner (no pair above 0.45)."""
    if B < 3:
        return
    y[1, :, 4:] *= F(2.0 ** -13) if k % 2 else F(0.25)
    mine = bidx == 2
    boxes[mine] = torch.tensor([0.02, 0.02, 0.01, 0.01])


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
@pytest.mark.parametrize('nc', [1, 3, 80])
@pytest.mark.parametrize('nq', [5, 37, 300, 512])
@pytest.mark.parametrize('B', [1, 3])
def test_kernel_equals_engine_confusion_matrix(B, nq, nc, dtype):
    """Labels per image rotate through 0, 1, 7, 513, 1100 (mixed inside a batch of three); ori_shape, shuffled labels and the special
    images rotate with the case so that every one meets every shape family.  make_case puts most detections on the image's first
    labels with the label's class four times out of five: several detections per label, one detection over several (clustered)
    labels, cross-class matches, scores on both sides of 0.25."""
    k = (0 if B == 1 else 1) + 2 * (5, 37, 300, 512).index(nq) + 8 * (1, 3, 80).index(nc) + 24 * (dtype == 'bf16')
    lpi = tuple(LABELS[(k + i) % 5] for i in range(B)) if B == 3 else (LABELS[(k // 2) % 5],)
    y, cls, boxes, bidx = make_case(B, nq, nc, lpi, 300 + k, bf16=dtype == 'bf16', shuffle_labels=k % 4 < 2)
    special_images(y, cls, boxes, bidx, B, k)
    hw = orig_shapes(B, k) if k % 3 else None
    got, want, counts = run_both(y, cls, boxes, bidx, hw, nc, bf16=dtype == 'bf16')
    what = f'B {B} nq {nq} nc {nc} {dtype} labels {lpi} shape {hw is not None}'
    assert torch.equal(got.cpu().long(), torch.from_numpy(want.matrix)), what
    m = want.matrix
    in_range = int(((cls.view(-1) >= 0) & (cls.view(-1) < nc) & (bidx >= 0) & (bidx < B)).sum())
    assert m[:, :nc].sum() == in_range, what                # every label is counted exactly once
    if B == 3:
        assert (counts[1] == 0) == (k % 2 == 1)
    if nq >= 37 and max(lpi[:1]) >= 7:
        assert m[:nc, :nc].sum() > 0, what                   # the case has matches in it


def test_the_special_images_are_what_they_claim():
    """One batch, looked at image by image: counts == 0, no score above 0.25, no pair above 0.45, no labels."""
    nc = 10
    y, cls, boxes, bidx = make_case(4, 300, nc, (37, 37, 37, 0), 77)
    y[0, :, 4:] *= F(2.0 ** -13)
    y[1, :, 4:] *= F(0.25)
    boxes[bidx == 2] = torch.tensor([0.02, 0.02, 0.01, 0.01])
    got, want, counts = run_both(y, cls, boxes, bidx, None, nc)
    assert counts[0] == 0 and counts[1] > 0 and counts[2] > 0 and counts[3] > 0
    assert y[1, :, 4:].max() <= 0.25 < y[2, :, 4:].max()
    m = want.matrix
    assert torch.equal(got.cpu().long(), torch.from_numpy(m))
    # all 3 x 37 labels are background misses; images 2 and 3 have confident detections, none is a false positive
    assert m[nc, :nc].sum() == 111 and m[:nc].sum() == 0


def hand_case(dets, labels, nc, conf=0.25, thr=0.45, wh=(100, 100)):
    """predn / counts / labels written by hand for one image of wh = (w, h): dets rows x1 y1 x2 y2 score cls (pixels), labels rows
    cls cx cy w h (normalised).  -> (kernel matrix, engine matrix)."""
    from tamtr_amd import engine as E, ops
    nq = max(len(dets), 1) + 2                        # two rows past the count, filled with a box that would match
    predn = torch.zeros(1, nq, 6)
    if dets:
        predn[0, :len(dets)] = torch.tensor(dets, dtype=torch.float32)
    predn[0, len(dets):] = torch.tensor([0., 0., 100., 100., 0.99, 0.])
    lab = torch.tensor(labels, dtype=torch.float32).reshape(-1, 5)
    dl = (lab[:, 0].contiguous().cuda(), lab[:, 1:].contiguous().cuda(), torch.tensor([0, len(lab)], dtype=torch.int32).cuda(),
          torch.tensor([[1., 1., wh[0], wh[1]]]).cuda())
    matrix = torch.zeros(nc + 1, nc + 1, dtype=torch.int32, device='cuda')
    counts = torch.tensor([len(dets)], dtype=torch.int32).cuda()
    ops.val_confusion(predn.cuda(), counts, dl, nc, conf, thr, matrix)
    torch.cuda.synchronize()
    cm = CM(nc, conf, thr)
    tbox = E.xywh2xyxy(lab[:, 1:])
    tbox[..., [0, 2]] *= wh[0]
    tbox[..., [1, 3]] *= wh[1]
    if len(dets) == 0:
        cm.process_batch(None, lab[:, 0])
    elif len(lab):
        cm.process_batch(predn[0, :len(dets)], torch.cat((lab[:, :1], tbox), 1))
    return matrix.cpu().long().numpy(), cm.matrix


def test_exact_ties_quirks_nan_and_out_of_range_classes_by_hand():
    box = [0.25, 0.25, 0.2, 0.2]                       # pixels 15 .. 35
    px = [15., 15., 35., 35.]
    # identical label boxes: the lower label index takes the detection
    got, want = hand_case([px + [0.9, 0.]], [[1.] + box, [2.] + box], 3)
    np.testing.assert_array_equal(got, want)
    assert got[0, 1] == 1 and got[3, 2] == 1 and got.sum() == 2
    # identical detection boxes: the lower row takes the label, the other is a false positive
    got, want = hand_case([px + [0.5, 1.], px + [0.9, 2.]], [[0.] + box], 3)
    np.testing.assert_array_equal(got, want)
    assert got[1, 0] == 1 and got[2, 3] == 1 and got.sum() == 2
    # no match in the image: no false positives; no labels: nothing; no detections: every label to background
    got, want = hand_case([[60., 60., 80., 80., 0.9, 0.]], [[1.] + box], 3)
    np.testing.assert_array_equal(got, want)
    assert got[3, 1] == 1 and got.sum() == 1
    got, want = hand_case([px + [0.9, 0.]], [], 3)
    assert got.sum() == 0 and want.sum() == 0
    got, want = hand_case([], [[1.] + box, [1.] + box, [0.] + box], 3)
    np.testing.assert_array_equal(got, want)
    assert got[3].tolist() == [1, 2, 0, 0] and got.sum() == 3
    # NaN boxes, a NaN score, classes that truncate and classes out of range
    nan = float('nan')
    got, want = hand_case([[nan, 15., 35., 35., 0.9, 0.], px + [0.9, 1.9], px + [nan, 0.], [60., 60., 80., 80., 0.9, 2.], [60., 60., 80., 80., 0.9, -0.5]],
                          [[0.7] + box, [1.] + [0.25, nan, 0.2, 0.2], [2.] + [0.7, 0.7, 0.2, 0.2], [-1.] + box, [nan] + box], 2)
    np.testing.assert_array_equal(got, want)
    assert got[1, 0] == 1 and got[2, 1] == 1 and got[0, 2] == 2 and got.sum() == 4
    # IoUs equal to the fp32 threshold are not candidates: 90 / 200 = float32(0.45), 300 / 500 = float32(0.6) (which exceeds 0.6 in double)
    for thr, lab, det in ((0.45, [0.5, 0.5, 1.0, 1.0], [0., 0., 9., 10.]), (0.6, [0.5, 0.5, 1.0, 1.0], [0., 0., 30., 10.])):
        wh = (20, 10) if thr == 0.45 else (50, 10)
        got, want = hand_case([det + [0.9, 0.]], [[0.] + lab], 1, thr=thr, wh=wh)
        np.testing.assert_array_equal(got, want)
        assert got.tolist() == [[0, 0], [1, 0]]
        got, want = hand_case([det + [0.9, 0.]], [[0.] + lab], 1, thr=float(np.nextafter(F(thr), F(0))), wh=wh)
        np.testing.assert_array_equal(got, want)
        assert got.tolist() == [[1, 0], [0, 0]]
    # a score equal to the confidence does not pass
    got, want = hand_case([px + [0.25, 0.]], [[0.] + box], 1)
    np.testing.assert_array_equal(got, want)
    assert got.tolist() == [[0, 0], [1, 0]]


def test_duplicated_rows_and_labels_tie_through_the_matching_op():
    """Rows duplicated with another winning class survive the class-aware NMS with identical boxes; labels duplicated give equal IoUs."""
    nc = 3
    y, cls, boxes, bidx = make_case(2, 300, nc, (37, 5), 17)
    y[0, 100:200, :4] = y[0, :100, :4]
    y[0, 100:200, 4:] = np.roll(y[0, :100, 4:], 1, axis=1)
    cls, boxes, bidx = torch.cat([cls, cls]), torch.cat([boxes, boxes]), torch.cat([bidx, bidx])
    got, want, _ = run_both(y, cls, boxes, bidx, None, nc)
    assert torch.equal(got.cpu().long(), torch.from_numpy(want.matrix))
    assert want.matrix[:nc, :nc].sum() > 0 and want.matrix[:nc, nc].sum() > 0


def test_single_cls_and_device_resident_labels():
    nc = 10
    y, cls, boxes, bidx = make_case(3, 300, nc, (37, 0, 700), 13, shuffle_labels=True)
    hw = orig_shapes(3, 13)
    host, want, _ = run_both(y, cls, boxes, bidx, hw, nc)
    dev, _, _ = run_both(y, cls, boxes, bidx, hw, nc, device_labels=True)
    assert torch.equal(host, dev) and torch.equal(host.cpu().long(), torch.from_numpy(want.matrix))
    got, want, _ = run_both(y, cls, boxes, bidx, hw, nc, single_cls=True)
    assert torch.equal(got.cpu().long(), torch.from_numpy(want.matrix))
    assert want.matrix[1:nc].sum() == 0 and want.matrix[0, 1:nc].sum() > 0      # every detection is class 0, labels keep their classes


def test_two_calls_accumulate_and_two_runs_agree():
    nc = 10
    a = make_case(3, 300, nc, (37, 513, 7), 21)
    b = make_case(2, 300, nc, (120, 1), 22)
    ma, ca, _ = run_both(*a, None, nc)
    mb, cb, _ = run_both(*b, None, nc)
    both, cm, _ = run_both(*a, None, nc)
    both, cm, _ = run_both(*b, None, nc, matrix=both, cm=cm)
    assert torch.equal(both, ma + mb) and torch.equal(both.cpu().long(), torch.from_numpy(cm.matrix))
    assert np.array_equal(cm.matrix, ca.matrix + cb.matrix) and both.sum() > 0
    again, _, _ = run_both(*a, None, nc)
    assert torch.equal(again, ma)


def test_unsupported_shapes_raise():
    from tamtr_amd import TamtrHipError, ops
    labels = (torch.zeros(0).cuda(), torch.zeros(0, 4).cuda(), torch.zeros(2, dtype=torch.int32).cuda(), torch.ones(1, 4).cuda())
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device='cuda')    # noqa: E731
    with pytest.raises(TamtrHipError):
        ops.val_confusion(z(1, 513, 6), z(1, dt=torch.int32), labels, 3, 0.25, 0.45, z(4, 4, dt=torch.int32))
    with pytest.raises(TamtrHipError):
        ops.val_confusion(z(1, 300, 6), z(1, dt=torch.int32), labels, 3, 0.25, 0.45, z(3, 3, dt=torch.int32))      # matrix of another nc
    with pytest.raises(TamtrHipError):
        ops.val_confusion(z(1, 300, 6), z(1, dt=torch.int32), labels, 0, 0.25, 0.45, z(1, 1, dt=torch.int32))


# ------------------------------------------------------------------------------------------------ the validators
@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_device_validator_confusion_equals_validator_and_never_synchronises(dtype):
    from tamtr_amd import engine as E
    hv = E.Validator(IMGSZ, 0.001, 0.7, confusion=True)
    batches = []
    for k, B in enumerate((4, 4, 3)):        # a tail batch of another size
        y, cls, boxes, bidx = make_case(B, 300, 10, (37, 0, 120, 1), 40 + k, bf16=dtype == 'bf16')
        yd = torch.from_numpy(y).cuda().to(torch.bfloat16 if dtype == 'bf16' else torch.float32)
        batches.append((yd, {'cls': cls, 'bboxes': boxes, 'batch_idx': bidx, 'ori_shape': orig_shapes(B, k)}))
    E.DeviceValidator(IMGSZ, 0.001, 0.7, confusion=True).update(*batches[0])     # first call: library load, allocator warm-up
    dv = E.DeviceValidator(IMGSZ, 0.001, 0.7, confusion=True)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        for yd, batch in batches:
            dv.update(yd, batch)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    for yd, batch in batches:
        hv.update(yd.float().cpu(), batch)
    got, want = dv.results(), hv.results()
    got.pop('per_class')
    assert got == want and got['seen'] == 11 and dv.nc == hv.nc == 10
    m = np.array(got['confusion_matrix'])
    assert m.shape == (11, 11) and m[:10, :10].sum() > 0 and m[:, :10].sum() == sum(len(b['cls']) for _, b in batches)
    assert all(isinstance(x, int) for row in got['confusion_matrix'] for x in row)
    plain = E.DeviceValidator(IMGSZ, 0.001, 0.7)
    for yd, batch in batches:
        plain.update(yd, batch)
    got.pop('confusion_matrix')
    rest = plain.results()
    rest.pop('per_class')
    assert rest == got                       # with confusion off nothing else differs, and the key is absent


def test_validate_on_device_returns_the_matrix():
    from tamtr_amd import engine as E
    from test_gpu_val import CONF, NC, S, _batches, _model, _text_feats
    model = _model().cuda().eval()
    model.set_text_features(_text_feats()[None].cuda())
    seen = []
    hook = model.register_forward_hook(lambda m, i, o: seen.append((o[0] if isinstance(o, (list, tuple)) else o).float().cpu()))
    batches = _batches()
    res = E.validate(model, batches, imgsz=S, conf=CONF, iou=0.7, on_device=True, confusion=True)
    hook.remove()
    hv = E.Validator(S, CONF, 0.7, confusion=True)
    for y, b in zip(seen, batches):
        hv.update(y, b)
    m = np.array(res['confusion_matrix'])
    assert m.shape == (NC + 1, NC + 1) and res['confusion_matrix'] == hv.results()['confusion_matrix']
    assert m[:, :NC].sum() == 15                                                  # every label once
    assert 'confusion_matrix' not in E.validate(model, batches[:1], imgsz=S, conf=CONF, iou=0.7, on_device=True)


def test_val_cli_writes_both_tables(tmp_path):
    """tools/val.py --confusion in a child process, on the device path and with --host-postprocess: both write the two tables, whose
    columns count every label once."""
    import yaml
    from tamtr_amd import data as D
    from test_gpu_val import CONF, NC, S, _dataset, _model
    names = _dataset(tmp_path)
    sd = _model().state_dict()
    ck = tmp_path / 'best.pt'
    torch.save({'model': sd, 'ema': sd}, ck)
    tf = D.TextFeatures.synthetic(names, dim=512, seed=2)
    feats = tmp_path / 'feats.npz'
    np.savez(feats, texts=np.array(names), feats=torch.stack([tf.table[n] for n in names]).numpy())
    spec = tmp_path / 'data.yaml'
    spec.write_text(yaml.safe_dump({'path': str(tmp_path), 'val': 'images', 'names': names}))
    label_hist = np.zeros(NC, int)
    for f in (tmp_path / 'labels').iterdir():
        for line in f.read_text().splitlines():
            label_hist[int(line.split()[0])] += 1
    for extra, folder in (([], 'TAMTR'), (['--host-postprocess'], 'TAMTR2')):
        cmd = [sys.executable, os.path.join(ROOT, 'tools', 'val.py'), '--data', str(spec), '--text-feats', str(feats), '--weights', str(ck),
               '--imgsz', str(S), '--batch', '2', '--workers', '0', '--conf', str(CONF), '--dtype', 'fp32', '--confusion',
               '--project', str(tmp_path / 'runs'), '--name', 'TAMTR'] + extra
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
        assert r.returncode == 0, r.stderr[-3000:]
        res = json.loads(r.stdout.strip().splitlines()[-1])
        out = tmp_path / 'runs' / folder
        assert res['save_dir'] == str(out) and res['confusion_csv'] == str(out / 'confusion_matrix.csv')
        assert res['confusion_normalized_csv'] == str(out / 'confusion_matrix_normalized.csv') and 'json' not in res
        rows = [line.split(',') for line in (out / 'confusion_matrix.csv').read_text().strip().splitlines()]
        assert rows[0][1:] == names + ['background'] and [r[0] for r in rows[1:]] == names + ['background']
        m = np.array([[int(x) for x in r[1:]] for r in rows[1:]])
        assert m.tolist() == res['confusion_matrix'] and np.array_equal(m[:, :NC].sum(0), label_hist) and label_hist.sum() == 12
        norm = np.array([[float(x) for x in line.split(',')[1:]] for line in
                         (out / 'confusion_matrix_normalized.csv').read_text().strip().splitlines()[1:]])
        np.testing.assert_allclose(norm, m / (m.sum(0)[None, :] + 1e-9), rtol=1e-12)
