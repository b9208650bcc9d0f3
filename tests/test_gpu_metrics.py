"""GPU: ops.val_ap_curves (csrc/metrics.hip) against engine.ap_per_class(stable=True, curves=True) in fp64 on the same rows brought to
the host, and against the reference's stored results; repeatability, no synchronisation; DeviceValidator(device_metrics=True),
validate(device_metrics=True) and tools/val.py --device-metrics --curves end to end.
Bound of every kernel comparison: 1e-12 absolute on values <= 1 (both sides compute the same fp64 operations; they differ in the order
of the 101-term trapezoid sum of values <= 1, serial on the device and pairwise in numpy: at most 100 * 2^-53 * 101 = 1.2e-12 before
the factor h = 0.01, so 1.2e-14 in the worst case).  n_gt and n_pred are exact."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from test_metrics_host import TOL, fixture_cases
from test_val_host import make_case, orig_shapes

pytestmark = pytest.mark.gpu

IMGSZ = 640
F = np.float32
LABELS = (513, 0, 1, 7)      # labels per image, in rotation
BATCH_LISTS = {'one': [(1, 37)], 'three': [(4, 300)] * 3, 'long': [(16, 300)] * 3}
KINDS = ('tie_free', 'ties', 'all_false', 'all_true', 'no_live_row', 'no_label', 'on_grid', 'first_row_fp')


def host_rows(batches):
    """The live rows of a list of numpy batches in image order, then row order: tp bool [n, 10], conf [n], cls [n]."""
    tp, conf, cls = [], [], []
    for predn, correct, counts in batches:
        live = np.arange(predn.shape[1])[None, :] < counts[:, None]
        tp.append(correct[live].astype(bool)), conf.append(predn[live][:, 4]), cls.append(predn[live][:, 5])
    return np.concatenate(tp), np.concatenate(conf), np.concatenate(cls)


def make_run(shapes, nc, kind, seed):
    """-> (batches of numpy (predn f32 [B, nq, 6], correct u8 [B, nq, 10], counts i32 [B]), labels: one f32 array per image).
    Dead rows carry a high score, a class and hits, which nobody may count.  Hits never outnumber a class's labels in the stable order
    (a label is matched at most once per threshold): the rule's assumption."""
    rng = np.random.default_rng(seed)
    total = sum(B * nq for B, nq in shapes)
    scores = ((rng.permutation(total) + rng.uniform(0.1, 0.9, total)) / total * 0.97 + 0.002).astype(F)     # pairwise distinct
    if kind == 'ties':
        scores = (rng.integers(1, 65, total) / 64).astype(F)
    batches, labels, first, image = [], [], 0, 0
    for B, nq in shapes:
        predn = rng.uniform(0, 600, (B, nq, 6)).astype(F)
        predn[..., 4] = scores[first:first + B * nq].reshape(B, nq)
        predn[..., 5] = rng.integers(0, nc, (B, nq))
        first += B * nq
        counts = rng.integers(1, nq, B).astype(np.int32)
        counts[0] = nq
        if B > 1:
            counts[1] = 0
        if kind == 'no_live_row':
            counts[:] = 0
        if nc >= 3:
            predn[..., 5][predn[..., 5] == 1] = 0                 # class 1 gets labels and no predictions
        correct = (rng.random((B, nq, 1)) < np.linspace(0.6, 0.1, 10)[None, None, :]).astype(np.uint8)
        if kind == 'all_false':
            correct[:] = 0
        if kind == 'all_true':
            correct[:] = 1
        batches.append((predn, correct, counts))
        for b in range(B):
            lab = rng.integers(0, nc, 0 if kind == 'no_label' else LABELS[image % 4]).astype(F)
            if nc >= 3:
                lab[lab == 2] = 0                                 # class 2 gets predictions and no labels
            if kind == 'all_true':                                # every prediction matched a label: there is one label per live row
                lab = np.concatenate([lab, predn[b, :counts[b], 5]])
            labels.append(lab)
            image += 1
    tp, conf, cls = host_rows(batches)
    if kind == 'on_grid' and len(conf):                           # 1.0 = px[999] and 0.0 = px[0] are the grid values fp32 can hold
        batches[0][0][0, 0, 4], batches[0][0][0, 1 % batches[0][0].shape[1], 4] = 1.0, 0.0
    if kind == 'first_row_fp' and (cls == 0).any():                    # the most confident row of class 0 misses: recall knot 0 is repeated
        for predn, correct, counts in batches:
            live = np.arange(predn.shape[1])[None, :] < counts[:, None]
            top = live & (predn[..., 5] == 0) & (predn[..., 4] == conf[cls == 0].max())
            correct[top] = 0
    # cap the hits of every class and threshold at its label count, in the rule's order
    tp, conf, cls = host_rows(batches)
    all_lab = np.concatenate(labels) if labels else np.zeros(0, F)
    order = np.argsort(-conf, kind='stable')
    keep = np.ones_like(tp)
    for c in range(nc):
        rows = order[cls[order] == c]
        keep[rows] = tp[rows].cumsum(0) <= int((all_lab == c).sum())
    at = 0
    for predn, correct, counts in batches:
        live = np.arange(predn.shape[1])[None, :] < counts[:, None]
        n = int(live.sum())
        correct[live] &= keep[at:at + n].astype(np.uint8)
        at += n
    if kind == 'all_true':
        assert host_rows(batches)[0].all()
    return batches, labels


def run_op(batches, labels, nc, **kw):
    from tamtr_amd import ops
    dev = [tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in b) for b in batches]
    return ops.val_ap_curves(dev, labels, nc, **kw)


def dense_host(batches, labels, nc):
    """engine.ap_per_class(stable=True, curves=True) spread over [0, nc): the six outputs of the op."""
    from tamtr_amd import engine as E
    tp, conf, cls = host_rows(batches)
    tcls = np.concatenate(labels) if labels else np.zeros(0, F)
    with np.errstate(all='ignore'):
        *_, ap, classes, cv = E.ap_per_class(tp, conf, cls, tcls, curves=True, stable=True)
    out = [np.zeros((nc, 10)), np.zeros((nc, 1000)), np.zeros((nc, 1000)), np.zeros((nc, 1000))]
    for row, c in enumerate(classes):
        for dst, src in zip(out, (ap, cv['p'], cv['r'], cv['pr'])):
            dst[c] = src[row]
    n_gt = np.array([(tcls == c).sum() for c in range(nc)], np.int32)
    n_pred = np.array([(cls == c).sum() for c in range(nc)], np.int32)
    return (*out, n_gt, n_pred)


def assert_outputs(got, want, what):
    names = ('ap', 'p_curve', 'r_curve', 'pr_curve')
    for name, g, w in zip(names, got[:4], want[:4]):
        g = g.cpu().numpy()
        assert g.dtype == np.float64 and g.shape == w.shape, (what, name)
        err = float(np.abs(g - w).max())
        print(f'{what}: {name} max abs difference {err:.3e}')
        assert err <= TOL, (what, name, err)
    assert np.array_equal(got[4].cpu().numpy(), want[4]) and np.array_equal(got[5].cpu().numpy(), want[5]), what


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('shapes,nc', [('one', 1), ('one', 10), ('one', 80), ('three', 1), ('three', 10), ('three', 80), ('long', 1)])
def test_op_equals_the_host_rule(shapes, nc, kind):
    from tamtr_amd import ops
    batches, labels = make_run(BATCH_LISTS[shapes], nc, kind, 100 * KINDS.index(kind) + nc + len(shapes))
    want = dense_host(batches, labels, nc)
    if shapes == 'long' and kind not in ('no_live_row',):
        assert want[5].max() >= 4 * ops.VAL_AP_TILE                   # the carry between tiles is exercised
    if kind in ('tie_free', 'ties', 'all_true') and shapes != 'one':
        assert want[0].max() > 0.01                                   # the case is not trivially zero
    if kind == 'ties':
        conf = host_rows(batches)[1]
        assert len(np.unique(conf)) <= 64 < len(conf) or shapes == 'one'
    got = run_op(batches, labels, nc)
    assert_outputs(got, want, f'{shapes} nc {nc} {kind}')
    if kind in ('no_live_row', 'no_label', 'all_false'):
        assert not got[0].any()


def test_labels_may_live_on_either_side():
    """Also: batches of different B and nq in one run."""
    batches, labels = make_run([(4, 300), (2, 37), (3, 64)], 10, 'tie_free', 3)
    want = dense_host(batches, labels, 10)
    flat = np.concatenate(labels)
    for form in (flat, torch.from_numpy(flat).cuda(), [labels[0], torch.from_numpy(np.concatenate(labels[1:])).cuda()]):
        assert_outputs(run_op(batches, form, 10), want, 'label forms')


def test_fixture_through_the_op():
    """The reference's stored results (tests/golden/curves.npz), every case as one image."""
    for k, c in fixture_cases():
        n, nc = len(c['conf']), int(c['nc'])
        nq = max(n, 1)
        predn = np.zeros((1, nq, 6), F)
        predn[0, :n, 4], predn[0, :n, 5] = c['conf'], c['pcls']
        correct = np.zeros((1, nq, 10), np.uint8)
        correct[0, :n] = c['tp']
        got = run_op([(predn, correct, np.array([n], np.int32))], c['tcls'], nc)
        want = [np.zeros((nc, 10)), np.zeros((nc, 1000)), np.zeros((nc, 1000)), np.zeros((nc, 1000))]
        for row, cl in enumerate(c['classes'].astype(int)):
            for dst, src in zip(want, (c['ap'], c['pcurve'], c['rcurve'], c['pr'])):
                dst[cl] = src[row]
        n_gt = np.array([(c['tcls'] == x).sum() for x in range(nc)], np.int32)
        n_pred = np.array([(c['pcls'] == x).sum() for x in range(nc)], np.int32)
        assert_outputs(got, (*want, n_gt, n_pred), f'fixture case {k}')


def test_two_runs_give_the_same_bits():
    batches, labels = make_run(BATCH_LISTS['long'], 1, 'ties', 11)
    a = run_op(batches, labels, 1, return_packed=True)[-1].clone()
    b = run_op(batches, labels, 1, return_packed=True)[-1]
    assert a.dtype == torch.float64 and a.numel() == 3011 and torch.equal(a.view(torch.int64), b.view(torch.int64))


def test_op_never_synchronises():
    from tamtr_amd import ops
    batches, labels = make_run(BATCH_LISTS['three'], 10, 'ties', 12)
    dev = [tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in b) for b in batches]
    ops.val_ap_curves(dev, labels, 10)               # first call: library load, grids, allocator warm-up
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        out = ops.val_ap_curves(dev, labels, 10)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert_outputs(out, dense_host(batches, labels, 10), 'under sync debug')


# ------------------------------------------------------------------------------------------------ the validators
def close(a, b, tol=1e-9):
    """Equal structure, numbers within tol."""
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(close(a[k], b[k], tol) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(close(x, y, tol) for x, y in zip(a, b))
    if isinstance(a, float) or isinstance(b, float):
        return abs(a - b) <= tol
    return a == b


def fed(dtype, **kw):
    """(a DeviceValidator with the keywords, the default one) after the same three updates; device-side labels in the second batch."""
    from tamtr_amd import engine as E
    dm, plain = E.DeviceValidator(IMGSZ, 0.001, 0.7, device_metrics=True, **kw), E.DeviceValidator(IMGSZ, 0.001, 0.7, **kw)
    for k, B in enumerate((4, 4, 3)):
        y, cls, boxes, bidx = make_case(B, 300, 10, (37, 0, 120, 1), 60 + k, bf16=dtype == 'bf16')
        yd = torch.from_numpy(y).cuda().to(torch.bfloat16 if dtype == 'bf16' else torch.float32)
        batch = {'cls': cls, 'bboxes': boxes, 'batch_idx': bidx, 'ori_shape': orig_shapes(B, k), 'im_file': [f'/data/{k}_{i}.jpg' for i in range(B)]}
        if k == 1:
            batch.update(cls=cls.cuda(), bboxes=boxes.cuda(), batch_idx=bidx.cuda())
        dm.update(yd, batch), plain.update(yd, batch)
    return dm, plain


@pytest.mark.parametrize('kw', [{}, {'confusion': True}, {'save_json': True}], ids=['plain', 'confusion', 'save_json'])
def test_device_metrics_equal_the_default_device_validator(kw):
    """fp32 y with pairwise distinct scores: the stable order is the default's, so the two paths state the same numbers; they differ by
    the trapezoid's summation order only.  per_class: same classes, images and instances, numbers within the same 1e-9."""
    dm, plain = fed('f32', **kw)
    conf = plain._reduce()[0][:, 4]
    assert len(np.unique(conf)) == len(conf) > 1000
    got, want = dm.results(curves=True), plain.results(curves=True)
    assert got.keys() == want.keys() and want['mAP50'] > 0 and len(want['per_class']) == 10
    assert close(got, want), {k: (got[k], want[k]) for k in ('precision', 'recall', 'mAP50', 'mAP50-95')}
    assert [(r['class'], r['images'], r['instances']) for r in got['per_class']] == [(r['class'], r['images'], r['instances']) for r in want['per_class']]
    assert 'curves' not in dm.results() and close(dm.results(), plain.results())
    if 'confusion' in kw:
        assert got['confusion_matrix'] == want['confusion_matrix'] and np.array(got['confusion_matrix']).sum() > 0
    if 'save_json' in kw:
        assert dm.jdict == plain.jdict and len(dm.jdict) == len(conf)


def test_device_metrics_on_bf16_scores_follow_the_stable_order():
    from tamtr_amd import engine as E
    dm, plain = fed('bf16')
    predn, correct, _, tcls, _ = plain._reduce()
    *_, p, r, _, ap, classes = E.ap_per_class(correct, predn[:, 4], predn[:, 5], tcls, stable=True)
    got = dm.results()
    want = {'precision': float(p.mean()), 'recall': float(r.mean()), 'mAP50': float(ap[:, 0].mean()), 'mAP50-95': float(ap.mean())}
    assert want['mAP50'] > 0 and all(abs(got[k] - want[k]) <= 1e-9 for k in want), (got, want)
    assert [r['class'] for r in got['per_class']] == classes.tolist()


def test_device_metrics_without_rows_or_hits():
    from tamtr_amd import engine as E
    dv = E.DeviceValidator(IMGSZ, device_metrics=True)
    assert dv.results(curves=True) == {**E.DeviceValidator(IMGSZ).results(), 'curves': {}}
    y, cls, boxes, bidx = make_case(2, 37, 10, (5, 3), 1)
    y[..., 4:] *= F(2.0 ** -13)                      # nothing above the validator's conf
    dv.update(torch.from_numpy(y).cuda(), {'cls': cls, 'bboxes': boxes, 'batch_idx': bidx})
    assert dv.results() == {'precision': 0.0, 'recall': 0.0, 'mAP50': 0.0, 'mAP50-95': 0.0, 'seen': 2, 'per_class': []}


def test_validate_with_device_metrics_and_curves():
    from tamtr_amd import engine as E
    from test_gpu_val import CONF, NC, S, _batches, _model, _text_feats
    model = _model().cuda().eval()
    model.set_text_features(_text_feats()[None].cuda())
    batches = _batches()
    want = E.validate(model, batches, imgsz=S, conf=CONF, iou=0.7, on_device=True, curves=True)
    got = E.validate(model, batches, imgsz=S, conf=CONF, iou=0.7, on_device=True, device_metrics=True, curves=True)
    assert got.keys() == want.keys() and 'curves' in got and close(got, want)
    with pytest.raises(ValueError):
        E.validate(model, batches, imgsz=S, conf=CONF, iou=0.7, device_metrics=True)


def test_val_cli_writes_the_curve_tables_on_both_paths(tmp_path):
    import yaml
    from tamtr_amd import data as D
    from test_gpu_val import CONF, S, _dataset, _model
    names = _dataset(tmp_path)
    sd = _model().state_dict()
    ck = tmp_path / 'best.pt'
    torch.save({'model': sd, 'ema': sd}, ck)
    tf = D.TextFeatures.synthetic(names, dim=512, seed=2)
    feats = tmp_path / 'feats.npz'
    np.savez(feats, texts=np.array(names), feats=torch.stack([tf.table[n] for n in names]).numpy())
    spec = tmp_path / 'data.yaml'
    spec.write_text(yaml.safe_dump({'path': str(tmp_path), 'val': 'images', 'names': names}))
    lines, tables = [], []
    for extra, folder in ((['--device-metrics'], 'TAMTR'), ([], 'TAMTR2')):
        cmd = [sys.executable, os.path.join(ROOT, 'tools', 'val.py'), '--data', str(spec), '--text-feats', str(feats), '--weights', str(ck),
               '--imgsz', str(S), '--batch', '2', '--workers', '0', '--conf', str(CONF), '--dtype', 'fp32', '--curves',
               '--project', str(tmp_path / 'runs'), '--name', 'TAMTR'] + extra
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
        assert r.returncode == 0, r.stderr[-3000:]
        res = json.loads(r.stdout.strip().splitlines()[-1])
        out = tmp_path / 'runs' / folder
        assert res['curves_csv'] == [str(out / f) for f in ('PR_curve.csv', 'P_curve.csv', 'R_curve.csv', 'F1_curve.csv')] and 'curves' not in res
        tables.append([[line.split(',') for line in open(p).read().strip().splitlines()] for p in res['curves_csv']])
        assert all(t[0][-1] == 'all classes' and set(t[0][1:-1]) <= set(names) for t in tables[-1])
        res.pop('curves_csv'), res.pop('save_dir')
        lines.append(res)
    assert close(lines[0], lines[1])
    for a, b in zip(*tables):
        assert a[0] == b[0] and len(a) == len(b)
        if len(a) > 1:
            assert len(a) == 1001
            np.testing.assert_allclose(np.array(a[1:], float), np.array(b[1:], float), rtol=0, atol=1e-9, equal_nan=True)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'val.py'), '--data', str(spec), '--text-feats', str(feats), '--weights', str(ck),
                        '--device-metrics', '--host-postprocess'], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and '--device-metrics' in r.stderr
