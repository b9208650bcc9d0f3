#!/usr/bin/env python3
"""Validator measurements (profiles/r06_val.txt):

  (a) one batch, B = 16, nq = 300, nc = 10 and 80, conf 0.001, about 50 and about 500 labels per image: engine.Validator.update (the
      per-image host loop) against engine.DeviceValidator.update (one HIP launch), on the same batch, ALTERNATING windows of >= 1 s
      each after warm-up, device events around every window;
  (b) engine.validate end to end at 640 x 640, batch 16, fp32 and bf16, host against device path, from synthetic JPEG files with
      labels: seconds for the pass (second pass timed) and images/s.

  (c) --confusion: the shapes of (a); DeviceValidator.update with and without confusion=True, and
      Validator.update with and without it for scale, ALTERNATING windows as in (a).

  (d) --metrics: DeviceValidator.results() at VisDrone-val scale on synthetic rows (548 images x 300 live rows, 70 labels per image,
      nc = 10 and 80, about a tenth of the rows hit at IoU 0.5): the host reduction (every row to the host, engine.ap_per_class) against
      device_metrics=True (ops.val_ap_curves, one packed copy), ALTERNATING windows as in (a); and the bytes each path copies.

  (e) --coco: COCO-protocol evaluation at VisDrone-val scale (548 images x 300 rows, 70 labels per image, nc = 10 and 80; the labels are
      70 of the image's own predicted boxes with their predicted class, so the matching has work): DeviceValidator.update on one batch of
      16 with and without coco=True, ALTERNATING windows as in (a); DeviceValidator(coco=True).results() over the whole run (the
      accumulation launch and the run's one copy), windows as in (a), against ONE timed call of engine.coco_evaluate - the project's own
      numpy statement of the rule, not pycocotools - on the same rows; and the bytes the copy gains.

    python tools/val_bench.py [--images 64] [--rounds 3] [--kernel-only] [--confusion | --metrics | --coco]
--kernel-only runs only the device loop of (a) - with --confusion the loop with confusion=True, with --metrics the device reduction of
(d), with --coco the update loop with coco=True and the device results() of (e) - for a `rocprofv3 --kernel-trace --stats` run of its own.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from predict_bench import synthetic_preds  # noqa: E402  (the predictor bench's clustered predictions)


def synthetic_labels(B, per_image, nc, seed=1):
    g = torch.Generator().manual_seed(seed)
    n = B * per_image
    boxes = torch.cat([torch.rand(n, 2, generator=g) * 0.8 + 0.1, torch.rand(n, 2, generator=g) * 0.2 + 0.02], 1)
    return {'cls': torch.randint(0, nc, (n, 1), generator=g).float(), 'bboxes': boxes,
            'batch_idx': torch.arange(B).repeat_interleave(per_image).float(), 'ori_shape': [(540 + 20 * i, 960 - 10 * i) for i in range(B)]}


def window(fn, min_s=1.0):
    """ms per call over one window of >= min_s, bracketed by device events (the stop event is recorded after the last call's work)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n, t0 = 0, time.perf_counter()
    e0.record()
    while time.perf_counter() - t0 < min_s:
        fn()
        n += 1
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n, n


def bench_confusion(rounds, kernel_only=False):
    from tamtr_amd import engine as E
    rows = []
    B, nq, conf, iou = 16, 300, 0.001, 0.7
    for nc in (10, 80):
        for per_image in (50, 500):
            y = synthetic_preds(B, nq, nc).cuda()
            batch = synthetic_labels(B, per_image, nc)

            def run(cls, confusion):
                v = cls(640, conf, iou, confusion=confusion)
                v.update(y, batch)
                return v

            for _ in range(5):
                run(E.DeviceValidator, True), run(E.DeviceValidator, False)
            if kernel_only:
                t, n = window(lambda: run(E.DeviceValidator, True))
                rows.append({'nc': nc, 'labels_per_image': per_image, 'device_update_confusion_ms': round(t, 4), 'iters': n})
                continue
            run(E.Validator, True), run(E.Validator, False)
            torch.cuda.synchronize()
            t = {(c, f): [] for c in ('device', 'host') for f in (False, True)}
            for _ in range(rounds):      # alternating windows
                for name, cls in (('device', E.DeviceValidator), ('host', E.Validator)):
                    for flag in (False, True):
                        t[name, flag].append(window(lambda: run(cls, flag))[0])
            m = np.array(run(E.DeviceValidator, True).results()['confusion_matrix'])
            assert m.tolist() == run(E.Validator, True).results()['confusion_matrix']
            rows.append({'B': B, 'nq': nq, 'nc': nc, 'labels_per_image': per_image, 'conf': conf, 'matched': int(m[:nc, :nc].sum()),
                         'background_misses': int(m[nc].sum()), 'false_positives': int(m[:nc, nc].sum()),
                         'device_update_ms': [round(x, 4) for x in t['device', False]],
                         'device_update_confusion_ms': [round(x, 4) for x in t['device', True]],
                         'host_update_ms': [round(x, 3) for x in t['host', False]],
                         'host_update_confusion_ms': [round(x, 3) for x in t['host', True]]})
    return rows


def synthetic_run(nc, images=548, nq=300, per_image=70, batch=16, seed=3):
    """What DeviceValidator.update leaves behind for a run of `images` images, made directly: every row live, distinct-ish scores,
    hits rarer at higher IoU thresholds (about 10 % at 0.5, so hits stay below the labels of a class), host-side labels."""
    g = torch.Generator().manual_seed(seed)
    rng = np.random.default_rng(seed)
    out = []
    for first in range(0, images, batch):
        B = min(batch, images - first)
        predn = torch.rand(B, nq, 6, generator=g)
        predn[..., 5] = torch.randint(0, nc, (B, nq), generator=g).float()
        hit = torch.rand(B, nq, 1, generator=g) < torch.linspace(0.1, 0.02, 10) * (0.5 + predn[..., 4:5])
        out.append((predn.cuda(), hit.to(torch.uint8).cuda(), torch.full((B,), nq, dtype=torch.int32).cuda(),
                    rng.integers(0, nc, B * per_image).astype(np.float32), (np.arange(B + 1) * per_image).astype(np.int32)))
    return out


def bench_metrics(rounds, kernel_only=False):
    from tamtr_amd import engine as E
    rows = []
    for nc in (10, 80):
        run = synthetic_run(nc)

        def validator(device_metrics):
            v = E.DeviceValidator(640, 0.001, 0.7, nc=nc, device_metrics=device_metrics)
            v.batches, v.seen = list(run), sum(b[0].shape[0] for b in run)
            return v

        host, device = validator(False), validator(True)

        def results(v):
            v._reduced = v._reduced_dev = None       # results() keeps its reduction: time it afresh
            return v.results()

        for _ in range(3):
            results(device)
        if kernel_only:
            t, n = window(lambda: results(device))
            rows.append({'nc': nc, 'device_results_ms': round(t, 3), 'iters': n})
            continue
        results(host)
        th, td = [], []
        for _ in range(rounds):      # alternating windows
            th.append(window(lambda: results(host))[0])
            td.append(window(lambda: results(device))[0])
        a, b = results(host), results(device)
        n_rows = sum(int(b_[2].sum()) for b_ in run)
        rows.append({'images': host.seen, 'rows': n_rows, 'labels': sum(len(b_[3]) for b_ in run), 'nc': nc,
                     'mAP50_host': a['mAP50'], 'mAP50_device': b['mAP50'], 'mAP50-95_host': a['mAP50-95'], 'mAP50-95_device': b['mAP50-95'],
                     'host_results_ms': [round(t, 3) for t in th], 'device_results_ms': [round(t, 3) for t in td],
                     'host_copy_bytes': sum(b_[0].numel() * 4 + b_[1].numel() + b_[2].numel() * 4 for b_ in run),
                     'device_copy_bytes': 8 * 3011 * nc})
    return rows


def coco_run(nc, images=548, nq=300, per_image=70, batch=16):
    """(y, batch dict) per batch at VisDrone-val scale: clustered predictions, and as labels 70 of each image's own predicted boxes with
    their predicted class."""
    out = []
    for k, first in enumerate(range(0, images, batch)):
        B = min(batch, images - first)
        y = synthetic_preds(B, nq, nc, seed=k)
        g = torch.Generator().manual_seed(1000 + k)
        pick = torch.stack([torch.randperm(nq, generator=g)[:per_image] for _ in range(B)])
        boxes = torch.gather(y[..., :4], 1, pick[..., None].expand(B, per_image, 4)).reshape(-1, 4).clamp(0.005, 0.995)
        cls = torch.gather(y[..., 4:].argmax(-1), 1, pick).reshape(-1, 1).float()
        out.append((y.cuda(), {'cls': cls, 'bboxes': boxes, 'batch_idx': torch.arange(B).repeat_interleave(per_image).float(),
                               'ori_shape': [(540 + 20 * i, 960 - 10 * i) for i in range(B)]}))
    return out


def bench_coco(rounds, kernel_only=False):
    from tamtr_amd import engine as E
    rows = []
    conf, iou = 0.001, 0.7
    for nc in (10, 80):
        run = coco_run(nc)

        def update(coco):
            v = E.DeviceValidator(640, conf, iou, coco=coco)
            v.update(*run[0])
            return v

        def whole(coco=True):
            v = E.DeviceValidator(640, conf, iou, coco=coco)
            for y, b in run:
                v.update(y, b)
            return v

        def results(v):
            v._reduced = v._reduced_dev = None       # results() keeps its reduction: time it afresh
            return v.results()

        for _ in range(5):
            update(True), update(False)
        dv, plain = whole(), whole(False)
        for _ in range(2):
            results(dv), results(plain)
        if kernel_only:
            tu, n = window(lambda: update(True))
            tr, m = window(lambda: results(dv))
            rows.append({'nc': nc, 'device_update_coco_ms': round(tu, 4), 'update_iters': n, 'device_results_coco_ms': round(tr, 3), 'results_iters': m})
            continue
        t = {k: [] for k in ('update', 'update_coco', 'results', 'results_coco')}
        for _ in range(rounds):      # alternating windows
            t['update'].append(window(lambda: update(False))[0])
            t['update_coco'].append(window(lambda: update(True))[0])
            t['results'].append(window(lambda: results(plain))[0])
            t['results_coco'].append(window(lambda: results(dv))[0])
        got = results(dv)['coco']
        predn, _, image, _, _ = dv._reduce()
        images, first = [], 0
        for (y, b), (pn, _, cn, _, _) in zip(run, dv.batches):
            pn, cn = pn.cpu(), cn.cpu()
            for i in range(y.shape[0]):
                h, w = b['ori_shape'][i]
                mine = b['batch_idx'] == i
                tbox = E.xywh2xyxy(b['bboxes'][mine])
                tbox[..., [0, 2]] *= w
                tbox[..., [1, 3]] *= h
                images.append((pn[i, :cn[i]].numpy(), torch.cat((b['cls'][mine], tbox), 1).numpy()))
        t0 = time.perf_counter()
        want = E.coco_evaluate(images, nc)['summary']
        host_s = time.perf_counter() - t0
        err = max(abs(got[k] - want[k]) for k in E.COCO_KEYS)
        assert err <= 1e-12, (got, want)
        rows.append({'images': len(images), 'rows': int(len(predn)), 'labels': sum(len(b['cls']) for _, b in run), 'nc': nc,
                     **{k: round(got[k], 6) for k in E.COCO_KEYS}, 'device_vs_host_max_err': err,
                     'device_update_ms': [round(x, 4) for x in t['update']], 'device_update_coco_ms': [round(x, 4) for x in t['update_coco']],
                     'device_results_ms': [round(x, 3) for x in t['results']], 'device_results_coco_ms': [round(x, 3) for x in t['results_coco']],
                     'host_coco_evaluate_s_one_call': round(host_s, 2), 'copy_gains_bytes': 8 * 80 * nc * 3 + 16 * nc,
                     'precision_array_bytes_left_on_device': 8 * 10 * 101 * nc * 4 * 3})
    return rows


def bench_update(rounds, kernel_only=False):
    from tamtr_amd import engine as E
    rows = []
    B, nq, conf, iou = 16, 300, 0.001, 0.7
    for nc in (10, 80):
        for per_image in (50, 500):
            y = synthetic_preds(B, nq, nc).cuda()
            batch = synthetic_labels(B, per_image, nc)

            def host():
                v = E.Validator(640, conf, iou)
                v.update(y, batch)

            def device():
                v = E.DeviceValidator(640, conf, iou)
                v.update(y, batch)
                return v

            for _ in range(5):
                device()
            if kernel_only:
                t, n = window(device)
                rows.append({'nc': nc, 'labels_per_image': per_image, 'device_update_ms': round(t, 4), 'iters': n})
                continue
            for _ in range(2):
                host()
            torch.cuda.synchronize()
            th, td = [], []
            for _ in range(rounds):      # alternating windows
                th.append(window(host)[0])
                td.append(window(device)[0])
            kept = float(device().batches[0][2].float().mean())
            rows.append({'B': B, 'nq': nq, 'nc': nc, 'labels_per_image': per_image, 'conf': conf, 'iou': iou, 'kept_per_image': round(kept, 1),
                         'host_update_ms': [round(t, 3) for t in th], 'device_update_ms': [round(t, 4) for t in td],
                         'speedup_worst_over_best': round(min(th) / max(td), 1)})
    return rows


def bench_validate(n_images, batch=16):
    from PIL import Image
    from tamtr_amd import data as D, engine as E
    from tamtr_amd.model import RTDETRDetectionWorldModel
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests', 'golden'))
    from weights import fill_state
    rng = np.random.default_rng(0)
    names = [f'c{i}' for i in range(10)]
    tf = D.TextFeatures.synthetic(names)
    rows = []
    with tempfile.TemporaryDirectory() as d:
        os.makedirs(os.path.join(d, 'images')), os.makedirs(os.path.join(d, 'labels'))
        for i in range(n_images):
            h, w = ((1080, 1920), (540, 960), (1500, 2000), (640, 640))[i % 4]
            Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(os.path.join(d, 'images', f'{i:04d}.jpg'), quality=90)
            lab = [f'{rng.integers(0, 10)} {rng.uniform(0.2, 0.8):.5f} {rng.uniform(0.2, 0.8):.5f} {rng.uniform(0.02, 0.2):.5f} {rng.uniform(0.02, 0.2):.5f}'
                   for _ in range(50)]
            with open(os.path.join(d, 'labels', f'{i:04d}.txt'), 'w') as f:
                f.write('\n'.join(lab))
        ds = D.PromptDetDataset(os.path.join(d, 'images'), names, 640, augment=False)
        for dtype in (None, torch.bfloat16):
            torch.manual_seed(0)
            model = RTDETRDetectionWorldModel(nc=len(names))
            model.load_state_dict(fill_state(model.state_dict(), 78))
            model = model.cuda().eval()
            model.set_text_features(tf.encode(names)[None].cuda())
            model.autocast_dtype = dtype
            row = {'imgsz': 640, 'batch': batch, 'dtype': 'bf16' if dtype else 'fp32', 'images': n_images, 'conf': 1e-5}
            for on_device in (False, True, False, True):   # alternating; the first pair warms kernels, libraries and the loader up
                loader = D.build_dataloader(ds, batch, 8, shuffle=False)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = E.validate(model, (D.preprocess_batch(b, None, 'cuda') for b in loader), imgsz=640, conf=1e-5, iou=0.7,
                                 autocast_dtype=dtype, on_device=on_device)   # conf: the seeded weights score below 5e-4
                torch.cuda.synchronize()
                key = 'device' if on_device else 'host'
                row[key + '_s'] = round(time.perf_counter() - t0, 3)
                row[key + '_images_per_s'] = round(res['seen'] / (time.perf_counter() - t0), 1)
            rows.append(row)
            del model
            torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=64)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--kernel-only', action='store_true')
    ap.add_argument('--skip-validate', action='store_true')
    ap.add_argument('--confusion', action='store_true', help='measurement (c): update with and without the confusion matrix')
    ap.add_argument('--metrics', action='store_true', help='measurement (d): results() on the host path and with device_metrics=True')
    ap.add_argument('--coco', action='store_true', help='measurement (e): update and results() with and without coco=True, and the host rule')
    args = ap.parse_args()
    import tamtr_amd  # noqa: F401
    assert torch.cuda.is_available(), 'val_bench needs an MI355X'
    print(torch.cuda.get_device_name(0), 'torch', torch.__version__)
    if args.coco:
        if args.kernel_only:
            print(json.dumps({'device_coco_only': bench_coco(0, True)}))
            return
        print(f'(e) COCO evaluation: update and results() with and without coco=True ({args.rounds} alternating windows of >= 1 s each, device '
              'events); engine.coco_evaluate (our numpy rule, not pycocotools) timed once on the same rows')
        for r in bench_coco(args.rounds):
            print(json.dumps(r))
        return
    if args.metrics:
        if args.kernel_only:
            print(json.dumps({'device_results_only': bench_metrics(0, True)}))
            return
        print(f'(d) DeviceValidator.results(): host reduction vs device_metrics=True ({args.rounds} alternating windows of >= 1 s each, device events)')
        for r in bench_metrics(args.rounds):
            print(json.dumps(r))
        return
    if args.kernel_only:
        print(json.dumps({'device_update_only': (bench_confusion if args.confusion else bench_update)(0, True)}))
        return
    if args.confusion:
        print(f'(c) update with and without the confusion matrix on one batch ({args.rounds} alternating windows of >= 1 s each, device events)')
        for r in bench_confusion(args.rounds):
            print(json.dumps(r))
        return
    print(f'(a) Validator.update vs DeviceValidator.update on one batch ({args.rounds} alternating windows of >= 1 s each, device events)')
    for r in bench_update(args.rounds):
        print(json.dumps(r))
    if not args.skip_validate:
        print(f'(b) validate end to end, {args.images} synthetic JPEGs with 50 labels each, second pass of each path timed')
        for r in bench_validate(args.images):
            print(json.dumps(r))


if __name__ == '__main__':
    main()
