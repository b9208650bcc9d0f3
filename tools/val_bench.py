#!/usr/bin/env python3
"""Validator measurements (profiles/r06_val.txt):

  (a) one batch, B = 16, nq = 300, nc = 10 and 80, conf 0.001, about 50 and about 500 labels per image: engine.Validator.update (the
      per-image host loop) against engine.DeviceValidator.update (one HIP launch), on the same batch, ALTERNATING windows of >= 1 s
      each after warm-up, device events around every window;
  (b) engine.validate end to end at 640 x 640, batch 16, fp32 and bf16, host against device path, from synthetic JPEG files with
      labels: seconds for the pass (second pass timed) and images/s.

  (c) --confusion: the shapes of (a); DeviceValidator.update with and without confusion=True, and
      Validator.update with and without it for scale, ALTERNATING windows as in (a).

    python tools/val_bench.py [--images 64] [--rounds 3] [--kernel-only] [--confusion]
--kernel-only runs only the device loop of (a) - with --confusion the loop with confusion=True - for a `rocprofv3 --kernel-trace --stats`
run of its own.
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
    args = ap.parse_args()
    import tamtr_amd  # noqa: F401
    assert torch.cuda.is_available(), 'val_bench needs an MI355X'
    print(torch.cuda.get_device_name(0), 'torch', torch.__version__)
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
