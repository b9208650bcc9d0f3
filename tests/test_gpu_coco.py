"""GPU: tamtr_val_coco_match and tamtr_val_coco_accumulate (csrc/cocoeval.hip) against engine.coco_evaluate, the host statement of the
rule.  Match bits, ranks and ground-truth counts are compared as integers; precision and recall must be EQUAL (each entry is one
correctly rounded fp64 division followed by a max or a pick); ap_tkam and the twelve numbers are held to 1e-12 (summation order).  Then
the hand cases through both kernels, accumulation, repeatability, DeviceValidator(coco=True), validate(coco=True) and tools/val.py --coco."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from coco_cases import HAND, KEYS, SECOND_CHOICE, SIDE, arrays, random_images, sized_case, to_xywh
from test_val_host import make_case, orig_shapes

pytestmark = pytest.mark.gpu

IMGSZ = 640
F = np.float32
LABELS = (0, 1, 70, 600)                # per image: none, one, the VisDrone mean, one past the LDS table of 512
TWELVE_PLUS = set(KEYS) | {'max_dets', 'per_class'}


def host_images(predn, counts, cls, boxes, bidx, hw, B):
    """The images as engine.Validator would hand them to coco_evaluate: the live rows of predn, and the labels converted as
    Validator.update converts them (xywh -> xyxy on the normalised fp32 values, then times the image's width / height)."""
    from tamtr_amd import engine as E
    images = []
    for b in range(B):
        h, w = hw[b] if hw is not None else (IMGSZ, IMGSZ)
        mine = bidx.view(-1) == b
        tbox = E.xywh2xyxy(boxes[mine].float())
        tbox[..., [0, 2]] *= w
        tbox[..., [1, 3]] *= h
        images.append((predn[b, :counts[b]].numpy(), torch.cat((cls.view(-1, 1)[mine].float(), tbox), 1).numpy()))
    return images


def match_both(y, cls, boxes, bidx, hw, nc, md, bf16=False, device_labels=False, npig=None):
    """The matching op, then the COCO match on its outputs -> (bits, rank, npig) of the kernel as numpy, and coco_evaluate's dict on the
    same rows and labels."""
    from tamtr_amd import engine as E, ops
    yd = torch.from_numpy(y).cuda()
    if bf16:
        yd = yd.to(torch.bfloat16)
    lab = (cls.cuda(), boxes.cuda(), bidx.cuda()) if device_labels else (cls, boxes, bidx)
    out = ops.val_postprocess_match(yd, *lab, hw, IMGSZ, 0.001, 0.7, False, return_device_labels=True)
    if npig is None:
        npig = torch.zeros(nc, 4, dtype=torch.int32, device='cuda')
    bits, rank = ops.val_coco_match(out[0], out[2], out[5], nc, md[-1], npig)
    torch.cuda.synchronize()
    predn, counts = out[0].cpu(), out[2].cpu().numpy()
    host = E.coco_evaluate(host_images(predn, counts, cls, boxes, bidx, hw, y.shape[0]), nc, md, return_matches=True)
    return bits.cpu().numpy(), rank.cpu().numpy(), npig.cpu().numpy(), host, counts, out


def assert_matches(bits, rank, npig, host, counts, what):
    for b, (wb, wr) in enumerate(host['matches']):
        n = counts[b]
        np.testing.assert_array_equal(bits[b, :n], wb, err_msg=f'{what} bits image {b}')
        np.testing.assert_array_equal(rank[b, :n], wr, err_msg=f'{what} rank image {b}')
        assert not bits[b, n:].any() and (rank[b, n:] == -1).all(), what         # rows past the count take part in nothing
    np.testing.assert_array_equal(npig, host['npig'], err_msg=what)


@pytest.mark.parametrize('nc', [1, 3, 80])
@pytest.mark.parametrize('nq', [5, 37, 300, 512])
@pytest.mark.parametrize('B', [1, 3])
def test_match_kernel_equals_the_host_rule(B, nq, nc):
    """Labels per image rotate through 0, 1, 70, 600 (mixed inside a batch of three); ori_shape, shuffled labels and the cuts rotate with
    the case.  sized_case puts most detections on the image's first labels with the label's class four times out of five and draws the
    label sides in pixels, 10 .. 200, so every size range has ground truths whatever the image size (asserted below)."""
    k = (0 if B == 1 else 1) + 2 * (5, 37, 300, 512).index(nq) + 8 * (1, 3, 80).index(nc)
    lpi = tuple(LABELS[(k + i) % 4] for i in range(B)) if B == 3 else (LABELS[(k // 2 + k // 8) % 4],)
    md = (1, 10, 100, 500) if k % 3 == 0 and nc > 1 else (1, 10, 100)
    hw = orig_shapes(B, k) if k % 3 else None
    y, cls, boxes, bidx = sized_case(B, nq, nc, lpi, 500 + k, hw, shuffle_labels=k % 4 < 2)
    bits, rank, npig, host, counts, _ = match_both(y, cls, boxes, bidx, hw, nc, md)
    what = f'B {B} nq {nq} nc {nc} labels {lpi} shape {hw is not None} cuts {md}'
    assert_matches(bits, rank, npig, host, counts, what)
    in_range = int(((cls.view(-1) >= 0) & (cls.view(-1) < nc)).sum())
    assert npig[:, 0].sum() == in_range, what                                     # every label is inside "all"
    if max(lpi) >= 70:
        assert (npig.sum(0) > 0).all(), what                                      # all four size ranges are populated
    if nq >= 37 and lpi[0] >= 1:
        assert (bits[0, :counts[0], 0] & 0x3ff).any(), what                       # the case has matches in it


def test_match_kernel_details_on_one_batch():
    """One batch looked at closely: labels on the device, a bf16 output through the matching op, 600 labels of ONE class (every lane of the
    walk strides ten times, the table lives in the workspace), more rows of a class than the last cut, ignored bits in every range."""
    nc, md = 1, (1, 10, 100)
    hw = orig_shapes(3, 4)
    y, cls, boxes, bidx = sized_case(3, 300, nc, (600, 70, 0), 901, hw, bf16=True)
    bits, rank, npig, host, counts, _ = match_both(y, cls, boxes, bidx, hw, nc, md, bf16=True, device_labels=True)
    assert_matches(bits, rank, npig, host, counts, 'bf16, device labels')
    assert counts.max() > 100 and rank.max() >= 100                               # rows beyond the last cut exist ...
    assert not bits[rank >= 100].any()                                            # ... and take part in nothing
    live = rank >= 0
    assert all(((bits[live][:, a] >> 16) & 0x3ff).any() for a in (1, 2, 3)) and (bits[live][:, 0] & 0x3ff).any()
    assert npig.tolist() == host['npig'].tolist() and npig[0, 0] == 670


@pytest.mark.parametrize('name', sorted(HAND) + ['second_choice'])
def test_hand_cases_through_both_kernels(name):
    """predn / counts / labels written by hand (labels as normalised xywh of side 512, exact), two rows past each count filled with a box
    that would match; the twelve numbers within 1e-12 of the hand-worked values, bits and ranks equal to the host rule's."""
    from tamtr_amd import engine as E, ops
    nc, md, images, want = HAND[name] if name in HAND else (1, (1, 10, 100), SECOND_CHOICE, None)
    imgs = arrays(images)
    B, nq = len(imgs), max(len(d) for d, _ in imgs) + 2
    predn = torch.zeros(B, nq, 6)
    predn[:, :] = torch.tensor([0., 0., 40., 40., 0.99, 0.])
    lab_cls, lab_box, off = [], [], [0]
    for b, (d, g) in enumerate(imgs):
        predn[b, :len(d)] = torch.from_numpy(d)
        c, xywh = to_xywh(g)
        lab_cls.append(c), lab_box.append(xywh), off.append(off[-1] + len(c))
    dl = (torch.from_numpy(np.concatenate(lab_cls)).cuda(), torch.from_numpy(np.concatenate(lab_box)).cuda(),
          torch.tensor(off, dtype=torch.int32).cuda(), torch.tensor([[1., 1., SIDE, SIDE]] * B).cuda())
    counts = torch.tensor([len(d) for d, _ in imgs], dtype=torch.int32).cuda()
    npig = torch.zeros(nc, 4, dtype=torch.int32, device='cuda')
    pd = predn.cuda()
    bits, rank = ops.val_coco_match(pd, counts, dl, nc, md[-1], npig)
    ap_tkam, recall, precision = ops.val_coco_accumulate([(pd, bits, rank)], npig, nc, md)
    torch.cuda.synchronize()
    host = E.coco_evaluate(imgs, nc, md, return_matches=True)
    assert_matches(bits.cpu().numpy(), rank.cpu().numpy(), npig.cpu().numpy(), host, counts.cpu().numpy(), name)
    np.testing.assert_array_equal(precision.cpu().numpy(), host['precision'])
    np.testing.assert_array_equal(recall.cpu().numpy(), host['recall'])
    got = E.coco_summary(ap_tkam.cpu().numpy(), recall.cpu().numpy(), md, npig.cpu().numpy())
    twelve = [got[k] for k in KEYS]
    print(name, twelve)
    if want is not None:
        assert np.abs(np.array(twelve) - np.array(want, float)).max() <= 1e-12, (name, twelve, want)
    assert np.abs(np.array(twelve) - np.array([host['summary'][k] for k in KEYS])).max() <= 1e-12


# ------------------------------------------------------------------------------------------------ accumulation
def device_run(images, nc, md, B=16):
    """Host matching of synthetic images (engine.coco_evaluate), its bits / ranks / counts uploaded in batches of B images with dead rows
    padded in -> the inputs of ops.val_coco_accumulate, and the host dict."""
    from tamtr_amd import engine as E
    host = E.coco_evaluate(images, nc, md, return_matches=True)
    nq = max(max(len(d) for d, _ in images), 1) + 3
    batches = []
    for first in range(0, len(images), B):
        part = images[first:first + B]
        predn = torch.zeros(len(part), nq, 6)
        predn[..., 4] = 0.999                                    # dead rows would come first if they took part
        bits, rank = torch.zeros(len(part), nq, 4, dtype=torch.int32), torch.full((len(part), nq), -1, dtype=torch.int32)
        for b, (d, _) in enumerate(part):
            mb, mr = host['matches'][first + b]
            predn[b, :len(d)], bits[b, :len(d)], rank[b, :len(d)] = torch.from_numpy(d), torch.from_numpy(mb), torch.from_numpy(mr)
        batches.append((predn.cuda(), bits.cuda(), rank.cuda()))
    return batches, torch.from_numpy(host['npig'].astype(np.int32)).cuda(), host


ACC_CASES = [  # nc, images, detections and labels per image (at most), score levels (None: tie-free), cuts
    (1, 1, 30, 12, None, (1, 10, 100)),
    (1, 48, 160, 20, None, (1, 10, 100, 500)),       # one class: a segment of more than four tiles of 256 rows
    (1, 48, 160, 20, 64, (1, 10, 100)),
    (10, 7, 60, 40, 64, (1, 10, 100, 500)),
    (10, 48, 60, 40, None, (1, 5, 20)),              # rows beyond the last cut
    (80, 33, 60, 70, None, (1, 10, 100)),
    (80, 48, 60, 70, 64, (1, 10, 100, 500)),
]


@pytest.mark.parametrize('nc,n_images,n_det,n_lab,levels,md', ACC_CASES)
def test_accumulate_kernel_equals_the_host_rule(nc, n_images, n_det, n_lab, levels, md):
    from tamtr_amd import engine as E, ops
    images = random_images(7 * nc + n_images, n_images, nc, n_det, n_lab, levels)
    batches, npig, host = device_run(images, nc, md)
    ap_tkam, recall, precision, packed = ops.val_coco_accumulate(batches, npig, nc, md, return_packed=True)
    again = ops.val_coco_accumulate(batches, npig, nc, md, return_packed=True)[-1]
    torch.cuda.synchronize()
    assert torch.equal(packed.view(torch.int64), again.view(torch.int64))                     # two runs give the same bits
    p, r, a = precision.cpu().numpy(), recall.cpu().numpy(), ap_tkam.cpu().numpy()
    off = np.argwhere(p != host['precision'])
    assert off.size == 0, (len(off), off[:5], p[tuple(off[0])], host['precision'][tuple(off[0])])
    np.testing.assert_array_equal(r, host['recall'])
    err = np.abs(a - host['ap_tkam']).max()
    got, want = E.coco_summary(a, r, md, host['npig']), host['summary']
    err12 = max(abs(got[k] - want[k]) for k in KEYS)
    print(f'nc {nc} images {n_images} levels {levels} cuts {md}: ap_tkam err {err:.3e}, twelve numbers err {err12:.3e}')
    assert err <= 1e-12 and err12 <= 1e-12
    assert np.array_equal(a == -1, host['ap_tkam'] == -1) and (a > 0).any() and (n_images < 7 or (host['npig'] > 0).all(1).any())
    if nc == 1 and n_images == 48:
        assert sum(int((m[1] >= 0).sum()) for m in host['matches']) > 4 * 256
    if levels:
        s = np.concatenate([d[:, 4] for d, _ in images])
        assert len(np.unique(s)) <= 64 < len(s)
    ap2, rc2, pr2 = ops.val_coco_split(packed.cpu().numpy(), nc, len(md))
    assert np.array_equal(ap2, a) and np.array_equal(rc2, r) and np.array_equal(pr2, p)


def test_unsupported_shapes_and_bad_operands_raise():
    from tamtr_amd import ops
    from tamtr_amd._lib import TamtrHipError
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device='cuda')     # noqa: E731
    labels = (z(2), z(2, 4), torch.tensor([0, 2], dtype=torch.int32).cuda(), z(1, 4))
    with pytest.raises(TamtrHipError):
        ops.val_coco_match(z(1, 513, 6), z(1, dt=torch.int32), labels, 3, 100, z(3, 4, dt=torch.int32))      # nq > 512
    with pytest.raises(TamtrHipError):
        ops.val_coco_match(z(1, 300, 6), z(1, dt=torch.int32), labels, 3, 100, z(4, 4, dt=torch.int32))      # table of another nc
    with pytest.raises(TamtrHipError):
        ops.val_coco_match(z(1, 300, 6), z(1, dt=torch.int32), labels, 3, 0, z(3, 4, dt=torch.int32))
    with pytest.raises(TamtrHipError):
        ops.val_coco_match(z(1, 300, 6), z(1, dt=torch.int32), labels, 3, 100, z(3, 4, dt=torch.int32), workspace=z(8, dt=torch.uint8))
    with pytest.raises(TamtrHipError):
        ops.val_coco_accumulate([(z(1, 5, 6), z(1, 5, 4), z(1, 5, dt=torch.int32))], z(3, 4, dt=torch.int32), 3, (1, 10))   # f32 bits


# ------------------------------------------------------------------------------------------------ the validators
def run_batches(dtype, nc=10):
    batches = []
    for k, B in enumerate((4, 4, 3)):        # a tail batch of another size
        y, cls, boxes, bidx = sized_case(B, 300, nc, (70, 0, 120, 1), 60 + k, orig_shapes(B, k), bf16=dtype == 'bf16')
        yd = torch.from_numpy(y).cuda().to(torch.bfloat16 if dtype == 'bf16' else torch.float32)
        batches.append((yd, {'cls': cls, 'bboxes': boxes, 'batch_idx': bidx, 'ori_shape': orig_shapes(B, k),
                             'im_file': [f'/data/images/{k}_{i}.jpg' for i in range(B)]}))
    return batches


def assert_same_coco(got, want):
    assert set(got) == set(want) == TWELVE_PLUS and got['max_dets'] == want['max_dets']
    assert max(abs(got[k] - want[k]) for k in KEYS) <= 1e-12, (got, want)
    for g, w in zip(got['per_class'], want['per_class']):
        assert set(g) == set(w) and all(abs(g[k] - w[k]) <= 1e-12 for k in g), (g, w)


@pytest.mark.parametrize('kw', [{}, {'confusion': True}, {'device_metrics': True}, {'save_json': True},
                                {'confusion': True, 'device_metrics': True, 'save_json': True, 'coco_max_dets': (1, 10, 100, 500)}],
                         ids=['plain', 'confusion', 'device_metrics', 'save_json', 'all'])
def test_device_validator_coco_equals_validator_and_never_synchronises(kw):
    from tamtr_amd import engine as E
    md = kw.get('coco_max_dets', (1, 10, 100))
    batches = run_batches('f32')
    E.DeviceValidator(IMGSZ, 0.001, 0.7, coco=True, **kw).update(*batches[0])     # first call: library load, allocator warm-up, grids
    dv = E.DeviceValidator(IMGSZ, 0.001, 0.7, coco=True, **kw)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        for yd, batch in batches:
            dv.update(yd, batch)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    hv = E.Validator(IMGSZ, 0.001, 0.7, coco=True, coco_max_dets=md)
    for yd, batch in batches:
        hv.update(yd.float().cpu(), batch)
    got, want = dv.results(), hv.results()
    assert_same_coco(got['coco'], want['coco'])
    assert 0 < got['coco']['AP'] < 1 and got['coco']['APs'] > -1 and got['coco']['APl'] > -1 and dv.nc == 10
    assert sum(c['npig'] for c in got['coco']['per_class']) == sum(len(b['cls']) for _, b in batches)
    same = E.DeviceValidator(IMGSZ, 0.001, 0.7, **{k: v for k, v in kw.items() if k != 'coco_max_dets'})
    for yd, batch in batches:
        same.update(yd, batch)
    rest = same.results()
    got.pop('coco')
    assert rest == got                       # with coco off nothing else differs, and the key is absent
    if kw.get('save_json'):
        assert len(dv.jdict) == len(same.jdict) > 0
    assert dv.results()['coco'] == dv.results()['coco']


def test_two_updates_accumulate_and_grouping_does_not_matter():
    from tamtr_amd import engine as E
    nc = 3
    hw = orig_shapes(6, 1)
    y, cls, boxes, bidx = sized_case(6, 300, nc, (70, 1, 0, 600, 70, 9), 77, hw)
    whole = E.DeviceValidator(IMGSZ, 0.001, 0.7, coco=True)
    whole.update(torch.from_numpy(y).cuda(), {'cls': cls, 'bboxes': boxes, 'batch_idx': bidx, 'ori_shape': hw})
    parts = E.DeviceValidator(IMGSZ, 0.001, 0.7, coco=True)
    for lo, hi in ((0, 2), (2, 3), (3, 6)):
        mine = (bidx >= lo) & (bidx < hi)
        parts.update(torch.from_numpy(y[lo:hi]).cuda(), {'cls': cls[mine], 'bboxes': boxes[mine], 'batch_idx': bidx[mine] - lo, 'ori_shape': hw[lo:hi]})
    a, b = whole.results()['coco'], parts.results()['coco']
    assert a == b and a['AP'] > 0                                                # the same rows in the same order: the same bits
    assert torch.equal(whole._npig, parts._npig) and int(whole._npig[:, 0].sum()) == 750
    first = E.DeviceValidator(IMGSZ, 0.001, 0.7, coco=True)
    first.update(torch.from_numpy(y[:2]).cuda(), {'cls': cls[bidx < 2], 'bboxes': boxes[bidx < 2], 'batch_idx': bidx[bidx < 2], 'ori_shape': hw[:2]})
    assert int(first._npig[:, 0].sum()) == 71 and first.results()['coco'] != a


def test_device_validator_without_rows():
    """Every score below conf: no live row in the run; classes with ground truth get 0, the others -1."""
    from tamtr_amd import engine as E
    y, cls, boxes, bidx = make_case(2, 37, 3, (9, 0), 5)
    y[..., 4:] *= F(2.0 ** -13)
    for kw in ({}, {'device_metrics': True}):
        dv = E.DeviceValidator(IMGSZ, 0.001, 0.7, coco=True, **kw)
        dv.update(torch.from_numpy(y).cuda(), {'cls': cls, 'bboxes': boxes, 'batch_idx': bidx})
        res = dv.results()
        assert res['coco']['AP'] == 0.0 and res['coco']['AR100'] == 0.0 and res['mAP50'] == 0.0
        hv = E.Validator(IMGSZ, 0.001, 0.7, coco=True)
        hv.update(torch.from_numpy(y), {'cls': cls, 'bboxes': boxes, 'batch_idx': bidx})
        assert_same_coco(res['coco'], hv.results()['coco'])


def test_validate_on_device_returns_the_dict():
    from tamtr_amd import engine as E
    from test_gpu_val import CONF, NC, S, _batches, _model, _text_feats
    model = _model().cuda().eval()
    model.set_text_features(_text_feats()[None].cuda())
    seen = []
    hook = model.register_forward_hook(lambda m, i, o: seen.append((o[0] if isinstance(o, (list, tuple)) else o).float().cpu()))
    batches = _batches()
    res = E.validate(model, batches, imgsz=S, conf=CONF, iou=0.7, on_device=True, coco=True, coco_max_dets=(1, 10, 100, 500))
    hook.remove()
    hv = E.Validator(S, CONF, 0.7, coco=True, coco_max_dets=(1, 10, 100, 500))
    for y, b in zip(seen, batches):
        hv.update(y, b)
    assert_same_coco(res['coco'], hv.results()['coco'])
    assert len(res['coco']['per_class']) == NC and sum(c['npig'] for c in res['coco']['per_class']) == 15
    assert 'coco' not in E.validate(model, batches[:1], imgsz=S, conf=CONF, iou=0.7, on_device=True)


def test_val_cli_writes_coco_metrics(tmp_path):
    """tools/val.py --coco in a child process: on the device path with every other option on, and with --host-postprocess."""
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
    for extra, folder, md in ((['--coco-max-dets', '1', '10', '100', '500', '--confusion', '--save-json', '--device-metrics'], 'TAMTR', [1, 10, 100, 500]),
                              (['--host-postprocess'], 'TAMTR2', [1, 10, 100])):
        cmd = [sys.executable, os.path.join(ROOT, 'tools', 'val.py'), '--data', str(spec), '--text-feats', str(feats), '--weights', str(ck),
               '--imgsz', str(S), '--batch', '2', '--workers', '0', '--conf', str(CONF), '--dtype', 'fp32', '--coco',
               '--project', str(tmp_path / 'runs'), '--name', 'TAMTR'] + extra
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
        assert r.returncode == 0, r.stderr[-3000:]
        res = json.loads(r.stdout.strip().splitlines()[-1])
        out = tmp_path / 'runs' / folder
        assert res['coco_json'] == str(out / 'coco_metrics.json')
        coco = json.loads((out / 'coco_metrics.json').read_text())
        assert coco == res['coco'] and set(coco) == TWELVE_PLUS and coco['max_dets'] == md and len(coco['per_class']) == NC
        assert sum(c['npig'] for c in coco['per_class']) == 12
        lines = [ln for ln in r.stderr.splitlines() if ln.startswith(' Average ')]
        assert len(lines) == 12 and lines[0].startswith(' Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=')
        assert all(-1 <= coco[k] <= 1 for k in KEYS)
