"""GPU: tamtr_val_postprocess_match (csrc/valmatch.hip) bit-exact against engine.Validator's pieces run on CPU fp32 copies of the same
inputs and against the restated rule (test_val_host.val_rule); engine.DeviceValidator, validate(on_device=True), fit(val_on_device=True)
and tools/val.py --save-json end to end."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from test_val_host import assert_conditions, engine_rule, make_case, orig_shapes, settle_case, tie_case, val_rule

pytestmark = pytest.mark.gpu

IMGSZ = 640


def run_kernel(y, cls, boxes, bidx, hw, imgsz, conf, iou, single_cls=False, bf16=False, device_labels=False):
    from tamtr_amd import ops
    yd = torch.from_numpy(y).cuda()
    if bf16:
        yd = yd.to(torch.bfloat16)
        assert torch.equal(yd.float().cpu(), torch.from_numpy(y))     # the case lies on the bf16 grid: both sides see the same numbers
    if device_labels:
        cls, boxes, bidx = cls.cuda(), boxes.cuda(), bidx.cuda()
    predn, correct, counts, _, _ = ops.val_postprocess_match(yd, cls, boxes, bidx, hw, imgsz, conf, iou, single_cls)
    torch.cuda.synchronize()
    return predn.cpu().numpy(), correct.cpu().numpy(), counts.cpu().numpy()


def assert_same(got, want, what, nan_scores=False):
    """torch.equal on predn, correct, counts; nan_scores: the inputs hold a NaN score, which both sides must show in the same places."""
    for g, w, name in zip(got, want, ('predn', 'correct', 'counts')):
        assert g.dtype == w.dtype and g.shape == w.shape, f'{what}: {name} {g.dtype}{g.shape} vs {w.dtype}{w.shape}'
        if nan_scores and name == 'predn':
            assert np.array_equal(np.isnan(g), np.isnan(w)), f'{what}: NaN pattern differs'
            g, w = np.nan_to_num(g, nan=-1.0), np.nan_to_num(w, nan=-1.0)
        assert torch.equal(torch.from_numpy(g), torch.from_numpy(w)), f'{what}: {name} differs in {int((g != w).sum())} places'


SHAPES = [(B, nq) for B in (1, 3, 16) for nq in (1, 64, 300, 512)]


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
@pytest.mark.parametrize('nc', [1, 10, 80])
@pytest.mark.parametrize('B,nq', SHAPES)
def test_kernel_equals_the_engine_on_cpu_fp32(B, nq, nc, dtype):
    """Labels per image mixed from {0, 1, 37, 700} in one batch; the remaining switches rotate over the cases so that every one meets
    every shape family: conf 0.3 (the quirk drops and keeps the 'wrong' rows) / 0.001, single_cls, non-square ori_shape or none,
    shuffled (unsorted) batch_idx, an image whose rows all fall below conf but which has labels."""
    k = SHAPES.index((B, nq)) + 3 * (nc == 10) + 5 * (nc == 80) + (dtype == 'bf16')
    conf, iou = (0.3, 0.001)[k % 2], (0.7, 0.45)[(k // 2) % 2]
    single_cls, with_shape, shuffle = (k // 3) % 2 == 1, k % 3 != 0, k % 4 < 2
    y, cls, boxes, bidx = make_case(B, nq, nc, (37, 0, 700, 1), 100 + k, bf16=dtype == 'bf16', shuffle_labels=shuffle)
    if B > 1:
        y[B - 1, :, 4:] *= F32_2_M13     # image B - 1: no score above conf (exact scaling, the bf16 grid is kept), labels stay
    hw = orig_shapes(B, k) if with_shape else None
    settle_case(y, cls, boxes, bidx, hw, IMGSZ, conf, iou, single_cls, bf16=dtype == 'bf16')
    diag = {}
    rule = val_rule(y, cls, boxes, bidx, hw, IMGSZ, conf, iou, single_cls, diag=diag)
    assert_conditions(diag)
    want = engine_rule(y, cls, boxes, bidx, hw, IMGSZ, conf, iou, single_cls)
    got = run_kernel(y, cls, boxes, bidx, hw, IMGSZ, conf, iou, single_cls, bf16=dtype == 'bf16')
    what = f'B {B} nq {nq} nc {nc} {dtype} conf {conf} iou {iou} single_cls {single_cls} shape {with_shape} shuffled {shuffle}'
    assert_same(got, want, what)
    assert_same(got, rule, what + ' (restated rule)')
    if B > 1:
        assert got[2][B - 1] == 0
    if nq >= 64:    # the case has work in it (under single_cls only labels of class 0 can match: label classes are not zeroed)
        assert got[2].sum() > 0 and (got[1].sum() > 0 or (single_cls and nc > 1))


F32_2_M13 = np.float32(2.0 ** -13)


def test_confidence_quirk_is_exercised():
    y, cls, boxes, bidx = make_case(2, 300, 10, (37, 5), 7)
    got = run_kernel(y, cls, boxes, bidx, None, IMGSZ, 0.3, 0.7)
    kept = got[0][0, :got[2][0], 4]
    assert (kept <= 0.3).any()         # rows below conf survive because the mask is read at the sorted position
    assert_same(got, engine_rule(y, cls, boxes, bidx, None, IMGSZ, 0.3, 0.7), 'quirk')


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_batch_without_labels(dtype):
    y, _, _, _ = make_case(3, 300, 10, (0,), 11, bf16=dtype == 'bf16')
    e = (torch.zeros(0, 1), torch.zeros(0, 4), torch.zeros(0))
    got = run_kernel(y, *e, None, IMGSZ, 0.001, 0.7, bf16=dtype == 'bf16')
    assert_same(got, engine_rule(y, *e, None, IMGSZ, 0.001, 0.7), 'M = 0')
    assert got[2].sum() > 0 and got[1].sum() == 0


def test_device_resident_labels_give_the_same_result():
    y, cls, boxes, bidx = make_case(3, 300, 10, (37, 0, 700), 13, shuffle_labels=True)
    hw = orig_shapes(3, 13)
    assert_same(run_kernel(y, cls, boxes, bidx, hw, IMGSZ, 0.001, 0.7, device_labels=True),
                run_kernel(y, cls, boxes, bidx, hw, IMGSZ, 0.001, 0.7), 'device labels')


def test_tie_cases_and_a_nan_score_row_follow_the_restated_rule():
    y, cls, boxes, bidx = tie_case()
    for iou in (0.7, 0.85):
        assert_same(run_kernel(y, cls, boxes, bidx, None, 100, 0.001, iou), val_rule(y, cls, boxes, bidx, None, 100, 0.001, iou), f'ties iou {iou}')
    y, cls, boxes, bidx = make_case(2, 300, 10, (37, 5), 17)
    k = 300 // 3
    y[0, k:2 * k] = y[0, :k]                        # duplicated rows: equal scores, identical boxes
    cls, boxes, bidx = torch.cat([cls, cls]), torch.cat([boxes, boxes]), torch.cat([bidx, bidx])    # duplicated labels: equal IoUs
    y[1, 150, 4 + 5] = float('nan')                 # a NaN score row: sorts first, its own position fails the mask
    y[1, 7::7, 4:] = np.round(y[1, 7::7, 4:] * 8) / 8  # scores on a coarse grid: many ties
    assert y[1, 0, 4:].max() > 0.001
    for conf in (0.001, 0.3):
        diag = {}
        want = val_rule(y, cls, boxes, bidx, None, IMGSZ, conf, 0.7, diag=diag)
        assert diag['equal_scores'] > 0 and diag['iou_ties'] > 0
        assert_same(run_kernel(y, cls, boxes, bidx, None, IMGSZ, conf, 0.7), want, f'ties + NaN conf {conf}', nan_scores=True)
        # the NaN row sorts first; it is kept iff the score of QUERY 0 passes the mask (nothing can suppress the first row)
        assert np.isnan(want[0][1, :want[2][1], 4]).sum() == int(y[1, 0, 4:].max() > conf)


def test_unsupported_shapes_raise():
    from tamtr_amd import TamtrHipError, ops
    e = (torch.zeros(0, 1), torch.zeros(0, 4), torch.zeros(0))
    with pytest.raises(TamtrHipError):
        ops.val_postprocess_match(torch.zeros(1, 513, 14, device='cuda'), *e, None, IMGSZ, 0.001, 0.7)
    with pytest.raises(TamtrHipError):
        ops.val_postprocess_match(torch.zeros(2, 300, 14, device='cuda'), *e, [(480, 640)], IMGSZ, 0.001, 0.7)


# ------------------------------------------------------------------------------------------------ DeviceValidator
@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_device_validator_equals_validator_and_never_synchronises(dtype):
    from tamtr_amd import engine as E
    dv, hv = E.DeviceValidator(IMGSZ, 0.001, 0.7), E.Validator(IMGSZ, 0.001, 0.7)
    batches = []
    for k, B in enumerate((4, 4, 3)):        # a tail batch of another size
        y, cls, boxes, bidx = make_case(B, 300, 10, (37, 0, 120, 1), 40 + k, bf16=dtype == 'bf16')
        yd = torch.from_numpy(y).cuda().to(torch.bfloat16 if dtype == 'bf16' else torch.float32)
        batches.append((yd, {'cls': cls, 'bboxes': boxes, 'batch_idx': bidx, 'ori_shape': orig_shapes(B, k)}))
    dv.update(*batches[0])                   # first call: library load, allocator warm-up
    dv = E.DeviceValidator(IMGSZ, 0.001, 0.7)
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
    per_class = got.pop('per_class')
    assert got == want and want['mAP50'] > 0 and got['seen'] == 11
    assert sum(r['instances'] for r in per_class) == sum(len(b['cls']) for _, b in batches)


# ------------------------------------------------------------------------------------------------ the real graph
NC, S, CONF = 10, 128, 1e-5        # the seeded weights score below 5e-4


def _model():
    sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
    from weights import fill_state
    from tamtr_amd.model import RTDETRDetectionWorldModel
    torch.manual_seed(0)
    model = RTDETRDetectionWorldModel(nc=NC)
    model.load_state_dict(fill_state(model.state_dict(), 78))
    return model


def _text_feats():
    g = torch.Generator().manual_seed(11)
    return torch.nn.functional.normalize(torch.randn(NC, 512, generator=g), dim=-1)


def _batches():
    g = torch.Generator().manual_seed(5)
    out = []
    for B in (2, 2, 1):
        n = 3 * B
        out.append({'img': torch.rand(B, 3, S, S, generator=g).cuda(),
                    'cls': torch.randint(0, NC, (n, 1), generator=g).float(),
                    'bboxes': torch.cat([0.2 + 0.6 * torch.rand(n, 2, generator=g), 0.05 + 0.4 * torch.rand(n, 2, generator=g)], 1),
                    'batch_idx': torch.arange(B).repeat_interleave(3).float(), 'ori_shape': [(90 + 7 * i, 200 - 11 * i) for i in range(B)]})
    return out


@pytest.mark.parametrize('dtype', [None, torch.bfloat16])
def test_validate_on_device_equals_the_host_validator_on_the_same_outputs(dtype):
    from tamtr_amd import engine as E
    model = _model().cuda().eval()
    model.set_text_features(_text_feats()[None].cuda())
    seen = []
    hook = model.register_forward_hook(lambda m, i, o: seen.append((o[0] if isinstance(o, (list, tuple)) else o).float().cpu()))
    batches = _batches()
    res = E.validate(model, batches, imgsz=S, conf=CONF, iou=0.7, autocast_dtype=dtype, on_device=True)
    hook.remove()
    assert len(seen) == len(batches)
    hv = E.Validator(S, CONF, 0.7)
    for y, b in zip(seen, batches):
        hv.update(y, b)
    per_class = res.pop('per_class')
    assert res == hv.results() and res['seen'] == 5
    assert sum(len(s[1]) for s in hv.stats) > 0            # detections did reach the matching
    assert isinstance(per_class, list)
    host = E.validate(model, batches, imgsz=S, conf=CONF, iou=0.7, autocast_dtype=dtype)      # the library default is the host path
    assert 'per_class' not in host and set(host) == set(res)


def test_fit_with_val_on_device_records_the_same_keys(tmp_path):
    import tamtr_amd.engine as E
    from tamtr_amd import data as D
    names = _dataset(tmp_path)
    hist = {}
    for on_device in (False, True):
        train = D.PromptDetDataset(str(tmp_path / 'images'), names, imgsz=S, augment=True, hyp={'scale': 0.2}, batch_size=2)
        val = D.PromptDetDataset(str(tmp_path / 'images'), names, imgsz=S, augment=False)
        tl, vl = D.build_dataloader(train, 2, workers=0, shuffle=False), D.build_dataloader(val, 2, workers=0, shuffle=False)
        tf = D.TextFeatures.synthetic(names + [''], dim=512, seed=2)
        model = _model().cuda().train()
        model.autocast_dtype = torch.bfloat16
        model.set_text_features(tf.encode(names)[None])
        hist[on_device] = E.fit(model, tl, lambda b, training: D.preprocess_batch(b, tf if training else None, 'cuda'), epochs=1,
                                val_loader=vl, warmup_iters=10, imgsz=S, val_on_device=on_device)[0]
    assert set(hist[True]) == set(hist[False]) | {'per_class'} and 'per_class' not in hist[False]
    assert hist[True]['seen'] == hist[False]['seen'] == 5 and 0.0 <= hist[True]['mAP50'] <= 1.0


def _dataset(tmp_path):
    from PIL import Image
    g = np.random.default_rng(0)
    (tmp_path / 'images').mkdir(), (tmp_path / 'labels').mkdir()
    names = ['pedestrian', 'people', 'bicycle', 'car', 'van', 'truck', 'tricycle', 'awning-tricycle', 'bus', 'motor']
    for i in range(5):
        Image.fromarray(g.integers(0, 255, (90 + 10 * i, 120, 3), dtype=np.uint8)).save(tmp_path / 'images' / f'im{i}.png')
        rows = [f'{int(g.integers(0, 10))} {g.uniform(0.3, 0.7):.5f} {g.uniform(0.3, 0.7):.5f} {g.uniform(0.2, 0.4):.5f} {g.uniform(0.2, 0.4):.5f}'
                for _ in range(0 if i == 1 else 3)]
        (tmp_path / 'labels' / f'im{i}.txt').write_text('\n'.join(rows))
    return names


def test_val_cli_writes_predictions_json(tmp_path):
    """tools/val.py --save-json in a child process; the file's rows are the kernel's predn rows of the same flow run here."""
    import yaml
    from tamtr_amd import data as D, engine as E
    names = _dataset(tmp_path)
    sd = _model().state_dict()
    ck = tmp_path / 'best.pt'
    torch.save({'model': sd, 'ema': sd}, ck)
    tf = D.TextFeatures.synthetic(names, dim=512, seed=2)
    feats = tmp_path / 'feats.npz'
    np.savez(feats, texts=np.array(names), feats=torch.stack([tf.table[n] for n in names]).numpy())
    spec = tmp_path / 'data.yaml'
    spec.write_text(yaml.safe_dump({'path': str(tmp_path), 'val': 'images', 'names': names}))
    project = tmp_path / 'runs'
    (project / 'TAMTR').mkdir(parents=True)   # an earlier run: this one goes to TAMTR2
    cmd = [sys.executable, os.path.join(ROOT, 'tools', 'val.py'), '--data', str(spec), '--text-feats', str(feats), '--weights', str(ck),
           '--imgsz', str(S), '--batch', '2', '--workers', '0', '--conf', str(CONF), '--dtype', 'fp32', '--save-json', '--project', str(project),
           '--name', 'TAMTR']
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    out = project / 'TAMTR2'
    assert res['save_dir'] == str(out) and res['json'] == str(out / 'predictions.json') and res['seen'] == 5
    assert isinstance(res['per_class'], list) and {'precision', 'recall', 'mAP50', 'mAP50-95'} <= set(res)
    with open(out / 'predictions.json') as f:
        rows = json.load(f)
    # the same flow in this process
    model = _model().cuda()
    model.set_text_features(tf.encode(names)[None].cuda())
    model.eval()
    model.autocast_dtype = None
    model.fuse()
    loader = D.build_dataloader(D.PromptDetDataset(str(tmp_path / 'images'), names, S, augment=False), 2, 0, shuffle=False)
    dv = E.DeviceValidator(S, CONF, 0.7, save_json=True)
    with torch.no_grad():
        for b in loader:
            b = D.preprocess_batch(b, None, 'cuda')
            dv.update(model(b['img']), b)
    dv.results()
    assert len(rows) == len(dv.jdict) > 0 and [r['image_id'] for r in rows] == [r['image_id'] for r in dv.jdict]
    predn, _, image, _, _ = dv._reduce()
    # the seeded weights give nearly equal scores (all below 5e-4, classes within the last bits of each other), so neither the ORDER of an
    # image's rows nor the winning class survives the last-bit differences between two processes' forwards: rows are compared per image
    # as sets (optimal one-to-one matching) on box and score - the kernel's predn rows in the file's form
    from conftest import assert_rows_match
    for i in range(5):
        mine = [r for r in rows if r['image_id'] == f'im{i}']
        p = predn[image == i]
        assert len(mine) == len(p)
        if len(p):
            want = np.concatenate([p[:, :2], p[:, 2:4] - p[:, :2], p[:, 4:5]], 1)
            got = np.array([r['bbox'] + [r['score']] for r in mine])
            assert all(isinstance(r['category_id'], int) and 0 <= r['category_id'] < NC for r in mine)
            assert_rows_match(torch.from_numpy(got), want, 0.05, f'im{i}')
    assert all(set(r) == {'image_id', 'category_id', 'bbox', 'score'} for r in rows)
