"""Host: engine.coco_evaluate (the statement of csrc/cocoeval.hip's rule) on the hand-worked cases and against the literal step-by-step
restatement in coco_cases.py; the validators' new option and unchanged defaults; the C ABI; argument checks of the two ops; the CLI."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from coco_cases import HAND, KEYS, SECOND_CHOICE, arrays, literal, random_images
from test_val_host import make_case, orig_shapes

F = np.float32
TWELVE_PLUS = set(KEYS) | {'max_dets', 'per_class'}


@pytest.mark.parametrize('name', sorted(HAND))
def test_hand_cases(name):
    """Each expected value is held to 1e-12; the derivations are in coco_cases.py."""
    from tamtr_amd import engine as E
    nc, md, images, want = HAND[name]
    res = E.coco_evaluate(arrays(images), nc, md, return_matches=True)
    got = [res['summary'][k] for k in KEYS]
    print(name, got)
    assert np.abs(np.array(got) - np.array(want, float)).max() <= 1e-12, (name, got, want)
    assert set(res['summary']) == TWELVE_PLUS and res['summary']['max_dets'] == list(md)
    precision, recall, matches, npig = literal(arrays(images), nc, md)
    np.testing.assert_array_equal(res['precision'], precision)
    np.testing.assert_array_equal(res['recall'], recall)
    np.testing.assert_array_equal(res['npig'], npig)
    for (b, r), (wb, wr) in zip(res['matches'], matches):
        np.testing.assert_array_equal(b, wb)
        np.testing.assert_array_equal(r, wr)


def test_hand_case_details():
    from tamtr_amd import engine as E
    m = {n: E.coco_evaluate(arrays(HAND[n][2]), HAND[n][0], HAND[n][1], return_matches=True) for n in HAND}
    b, r = m['ignored_last']['matches'][0]
    assert b[0].tolist() == [0x3ff, 0x3ff | (0x3f8 << 16), 0x3ff, 0x3ff | (0x3ff << 16)] and r.tolist() == [0]    # large: both are ignored, one is taken
    b, _ = m['iou_half']['matches'][0]
    assert b[0, 0] == 1 and b[0, 1] == 1                       # matches at 0.5, not at 0.55
    b, _ = m['later_wins']['matches'][0]
    assert b[:, 0].tolist() == [0x1f, 0x3ff]
    assert m['area_1024']['npig'].tolist() == [[1, 1, 1, 0]]
    b, r = m['beyond_max_dets']['matches'][0]
    assert r.tolist() == [0, 1, 2] and b[2].tolist() == [0, 0, 0, 0] and b[1, 0] == 0x3ff
    s = m['classes_without']['summary']['per_class']
    assert [c['AP'] for c in s] == [pytest.approx(1, abs=1e-12), -1.0, 0.0] and [c['npig'] for c in s] == [1, 0, 1]
    assert (m['classes_without']['recall'][:, 2, 0] == 0).all() and (m['classes_without']['precision'][:, :, 1] == -1).all()
    _, r = m['out_of_range']['matches'][0]
    assert r.tolist() == [-1, -1, 0] and m['out_of_range']['npig'].tolist() == [[1, 0, 1, 0], [0, 0, 0, 0]]
    b, r = m['nan_score']['matches'][0]
    assert r.tolist() == [-1, 0] and b[0].tolist() == [0, 0, 0, 0]
    assert m['no_rows']['summary']['per_class'][0]['AP'] == 0.0


@pytest.mark.parametrize('seed,nc,levels,md', [(0, 1, None, (1, 10, 100)), (1, 3, 8, (1, 3, 5)), (2, 4, None, (2,)), (3, 2, 4, (1, 2, 3, 4))])
def test_vectorised_rule_equals_the_literal_walk(seed, nc, levels, md):
    from tamtr_amd import engine as E
    images = random_images(seed, 4, nc, 14, 9, levels)
    res = E.coco_evaluate(images, nc, md, return_matches=True)
    precision, recall, matches, npig = literal(images, nc, md)
    np.testing.assert_array_equal(res['precision'], precision)
    np.testing.assert_array_equal(res['recall'], recall)
    np.testing.assert_array_equal(res['npig'], npig)
    for (b, r), (wb, wr) in zip(res['matches'], matches):
        np.testing.assert_array_equal(b, wb)
        np.testing.assert_array_equal(r, wr)
    assert (precision > 0).any() and (np.concatenate([b for b, _ in matches]) >> 16).any()      # hits and ignored rows both occur
    np.testing.assert_allclose(res['ap_tkam'], np.where(precision[:, 0] > -1, precision.mean(1), -1), rtol=0, atol=1e-12)


def hits(bits_all):
    return ((bits_all[:, None] >> np.arange(10)) & 1).astype(bool)


def test_coco_and_ultralytics_matching_on_case_b_and_where_they_differ():
    """The validator's `correct` table gives each detection its overall best label and lets the lower row (the more confident claimant) win
    it.  On case B that rule and COCO's greedy one mark the SAME hits - the first detection holds the first ground truth up to 0.75, the
    second gets it above - and what separates the two protocols there is the ignore state in "large" (and the AP integral).  The rules
    part where a detection loses its best label and has a second choice: COCO hands it the best ground truth still free, the `correct`
    table leaves it false."""
    from tamtr_amd import engine as E
    det, lab = arrays(HAND['B'][2])[0]
    correct = E.process_batch(torch.from_numpy(det), torch.from_numpy(lab), E.IOUV).numpy()
    bits = E.coco_evaluate([(det, lab)], 1, return_matches=True)['matches'][0][0]
    coco = hits(bits[:, 0])
    assert coco[1].tolist() == [False] * 6 + [True] * 4 and coco[0].tolist() == [True] * 6 + [False] * 4
    assert np.array_equal(correct, coco)
    assert (bits[0, 3] >> 16) == 0x3c0 and (bits[0, 0] >> 16) == 0          # ignored in "large" above 0.77, false in "all"
    det, lab = arrays(SECOND_CHOICE)[0]
    correct = E.process_batch(torch.from_numpy(det), torch.from_numpy(lab), E.IOUV).numpy()
    coco = hits(E.coco_evaluate([(det, lab)], 1, return_matches=True)['matches'][0][0][:, 0])
    assert not np.array_equal(correct, coco)
    assert not correct[1].any() and coco[1].tolist() == [True] * 6 + [False] * 4 and correct[0].all() and coco[0].all()


def test_max_dets_are_checked():
    from tamtr_amd import engine as E
    for bad in ((), (1, 10, 100, 500, 1000), (10, 1), (1, 1), (0, 5)):
        with pytest.raises(ValueError):
            E.coco_evaluate([], 1, bad)
        with pytest.raises(ValueError):
            E.Validator(coco=True, coco_max_dets=bad)
        with pytest.raises(ValueError):
            E.DeviceValidator(coco=True, coco_max_dets=bad)
    assert E.coco_evaluate([], 2, (1, 10, 100, 500))['summary']['AP'] == -1.0


def test_defaults_are_unchanged_and_the_option_adds_one_key():
    from tamtr_amd import engine as E
    y, cls, boxes, bidx = make_case(3, 64, 10, (0, 1, 37), 5)
    batch = {'cls': cls, 'bboxes': boxes, 'batch_idx': bidx, 'ori_shape': orig_shapes(3, 5)}
    plain, coco = E.Validator(160, 0.3, 0.7), E.Validator(160, 0.3, 0.7, coco=True, coco_max_dets=(1, 10, 100, 500))
    plain.update(torch.from_numpy(y), batch), coco.update(torch.from_numpy(y), batch)
    a, b = plain.results(), coco.results()
    assert set(a) == {'precision', 'recall', 'mAP50', 'mAP50-95', 'seen'}
    c = b.pop('coco')
    assert a == b and set(c) == TWELVE_PLUS and c['max_dets'] == [1, 10, 100, 500] and len(c['per_class']) == 10
    assert 0 < c['AP'] <= c['AP50'] <= 1 and c['AR1'] <= c['AR10'] <= c['AR100'] and coco.nc == 10
    json.dumps(c)
    assert set(E.DeviceValidator().results()) == {'precision', 'recall', 'mAP50', 'mAP50-95', 'seen', 'per_class'}
    assert set(E.Validator().results()) == {'precision', 'recall', 'mAP50', 'mAP50-95', 'seen'}
    empty = E.Validator(coco=True).results()['coco']
    assert [empty[k] for k in KEYS] == [-1.0] * 12 and empty['per_class'] == []
    empty = E.DeviceValidator(coco=True).results()['coco']
    assert [empty[k] for k in KEYS] == [-1.0] * 12
    assert [E.DeviceValidator(coco=True, device_metrics=True).results()['coco'][k] for k in KEYS] == [-1.0] * 12


def test_validator_coco_is_the_rule_on_its_own_detections():
    """Validator(coco=True) evaluates EVERY image - also one without labels (detections = false positives) and one without detections."""
    from tamtr_amd import engine as E
    y, cls, boxes, bidx = make_case(4, 48, 3, (9, 0, 20, 5), 11)
    y[3, :, 4:] *= F(2.0 ** -13)                                            # image 3 keeps no detection
    hw = orig_shapes(4, 2)
    v = E.Validator(160, 0.05, 0.7, coco=True)
    v.update(torch.from_numpy(y), {'cls': cls, 'bboxes': boxes, 'batch_idx': bidx, 'ori_shape': hw})
    images = []
    for si, pred in enumerate(E.postprocess(torch.from_numpy(y), 160, 0.05, 0.7)):
        predn = pred.clone()
        predn[:, [0, 2]] *= hw[si][1] / 160
        predn[:, [1, 3]] *= hw[si][0] / 160
        tbox = E.xywh2xyxy(boxes[bidx == si])
        tbox[:, [0, 2]] *= hw[si][1]
        tbox[:, [1, 3]] *= hw[si][0]
        images.append((predn.numpy(), torch.cat((cls[bidx == si].view(-1, 1), tbox), 1).numpy()))
    assert len(images[1][0]) > 0 and len(images[1][1]) == 0 and len(images[3][0]) == 0 and len(images[3][1]) == 5
    want = E.coco_evaluate(images, 3)
    assert v.results()['coco'] == want['summary'] and want['npig'][:, 0].sum() == 34


def test_the_symbols_are_exported_and_the_abi_is_still_36():
    from tamtr_amd import _lib
    new = ('tamtr_val_coco_match', 'tamtr_val_coco_workspace_bytes', 'tamtr_val_coco_accumulate')
    assert _lib.ABI_VERSION == 36 and all(n in _lib.EXPORTS for n in new)
    h = _lib.lib()
    assert h.tamtr_abi_version() == 36 and all(hasattr(h, n) for n in new)
    header = open(os.path.join(ROOT, 'include', 'tamtr_hip.h')).read()
    assert all(re.search(rf'\bint {n}\(', header) for n in new)
    assert h.tamtr_val_coco_workspace_bytes(3, 512, 1800) >= 44 * 1800 and h.tamtr_val_coco_workspace_bytes(1, 513, 0) == 0
    assert h.tamtr_val_coco_workspace_bytes(1, 5, 0) > 0


def test_ops_refuse_cpu_tensors_and_check_arguments_before_any_launch():
    from tamtr_amd import ops
    from tamtr_amd._lib import TamtrHipError
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt)     # noqa: E731
    labels = (z(2), z(2, 4), z(2, dt=torch.int32), z(1, 4))
    with pytest.raises(TamtrHipError, match='CPU tensor'):
        ops.val_coco_match(z(1, 5, 6), z(1, dt=torch.int32), labels, 3, 100, z(3, 4, dt=torch.int32))
    batch = (z(1, 5, 6), z(1, 5, 4, dt=torch.int32), z(1, 5, dt=torch.int32))
    with pytest.raises(TamtrHipError, match='CPU tensor'):
        ops.val_coco_accumulate([batch], z(3, 4, dt=torch.int32), 3, (1, 10, 100))
    for bad in ((), (1, 10, 100, 500, 1000), (10, 1), (0,)):
        with pytest.raises(TamtrHipError, match='max_dets'):
            ops.val_coco_accumulate([batch], z(3, 4, dt=torch.int32), 3, bad)
    with pytest.raises(TamtrHipError, match='at least one batch'):
        ops.val_coco_accumulate([], z(3, 4, dt=torch.int32), 3, (1,))
    with pytest.raises(TamtrHipError):
        ops.val_coco_workspace_bytes(1, 513, 10)
    assert ops.val_coco_workspace_bytes(16, 300, 1120) >= 44 * 1120


@pytest.mark.parametrize('kind', ['numpy', 'torch'])
def test_val_coco_split_undoes_the_packing(kind):
    from tamtr_amd import ops
    nc, m = 3, 4
    n = 40 * nc * m
    flat = np.arange(103 * n, dtype=np.float64)
    packed = flat if kind == 'numpy' else torch.from_numpy(flat)
    ap, rc, pr = ops.val_coco_split(packed, nc, m)
    assert tuple(ap.shape) == tuple(rc.shape) == (10, nc, 4, m) and tuple(pr.shape) == (10, 101, nc, 4, m)
    assert float(ap[1, 2, 3, 1]) == ((1 * nc + 2) * 4 + 3) * m + 1 and float(rc[0, 0, 0, 0]) == n and float(pr[0, 0, 0, 0, 0]) == 2 * n
    assert float(pr[9, 100, nc - 1, 3, m - 1]) == 103 * n - 1
    ap[0, 0, 0, 0] = -5                                      # views, not copies
    assert float(packed[0]) == -5
    ap2, rc2, none = ops.val_coco_split(packed[:2 * n], nc, m)
    assert none is None and float(rc2[9, nc - 1, 3, m - 1]) == 2 * n - 1 and tuple(ap2.shape) == (10, nc, 4, m)


def test_validate_passes_the_option_on_the_host_path():
    from tamtr_amd import engine as E

    class Model(torch.nn.Module):
        def forward(self, img, txt_feats=None):
            return self.y

    y, cls, boxes, bidx = make_case(2, 32, 3, (6, 4), 2)
    model = Model()
    model.y = torch.from_numpy(y)
    batch = {'img': torch.zeros(2, 3, 8, 8), 'cls': cls, 'bboxes': boxes, 'batch_idx': bidx}
    res = E.validate(model, [batch], imgsz=160, conf=0.05, coco=True, coco_max_dets=(1, 5))
    assert res['coco']['max_dets'] == [1, 5] and res['coco']['AR100'] == -1.0 and res['coco']['AP'] > 0
    assert 'coco' not in E.validate(model, [batch], imgsz=160, conf=0.05)


def test_val_cli_help_lists_the_flags():
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'val.py'), '--help'], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and '--coco ' in r.stdout + ' ' and '--coco-max-dets' in r.stdout


def test_cli_lines_and_file(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import val as V
    from tamtr_amd import engine as E
    nc, md, images, want = HAND['B']
    coco = E.coco_evaluate(arrays(images), nc, (1, 10, 100, 500))['summary']
    lines = V.coco_lines(coco)
    assert len(lines) == 12
    assert lines[0] == ' Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=500 ] = 0.768'
    assert lines[5] == ' Average Precision  (AP) @[ IoU=0.50:0.95 | area= large | maxDets=500 ] = 0.901'
    assert lines[6] == ' Average Recall     (AR) @[ IoU=0.50:0.95 | area=   all | maxDets=  1 ] = 0.300'
    assert lines[3].endswith('= -1.000')
    path = V.write_coco(coco, str(tmp_path))
    assert os.path.basename(path) == 'coco_metrics.json' and json.load(open(path)) == coco
