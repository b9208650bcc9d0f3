#!/usr/bin/env python3
"""Validate a checkpoint on a YOLO-format dataset (the reference's valTAMTR.py flow): mAP50 / mAP50-95 / precision / recall.

    python tools/val.py --data dataset.yaml --text-feats clip_vitb32.npz --weights runs/train/TAMTR/best.pt [--split val] [--save-json]

Postprocess and label matching run on the device (engine.DeviceValidator, one HIP launch per batch); --host-postprocess goes back to the
per-image host loop.  --save-json writes the reference's predictions.json into the run folder <project>/<name> (name, name2, ...).
--confusion adds the reference's confusion matrix (one more launch per batch on the device path, engine.ConfusionMatrix on the host path)
and writes confusion_matrix.csv and confusion_matrix_normalized.csv (columns divided by their sums) into the run folder: row = predicted,
column = true, header row and first column = the class names and `background`.
--curves writes the reference's four curve plots as tables, PR_curve.csv (precision over recall at IoU 0.5), P_curve.csv, R_curve.csv and
F1_curve.csv (over confidence), into the run folder: first column = the 1000-point grid, then one column per class that has labels, last
column `all classes` = their mean.  --device-metrics also reduces AP and the curves on the device (engine.DeviceValidator(device_metrics=True):
the rows of the run never come to the host).
--coco adds the COCO-protocol numbers (AP, AP50, AP75, AP / AR by object size, AR at the cuts of --coco-max-dets, default 1 10 100): the
step the reference leaves to save_json + dataset/yolo2coco.py + pycocotools.  One more launch per batch on the device path
(csrc/cocoeval.hip), engine.coco_evaluate with --host-postprocess; the twelve lines are printed in pycocotools' wording (to stderr; the
JSON result line stays the last line of stdout) and coco_metrics.json is written into the run folder.  Every image of the split is
evaluated, also one without labels.
--augment validates with test-time augmentation (tamtr_amd.tta: the reference's three scaled / mirrored views, or --tta-scales / --tta-flips,
merged on the device into one prediction tensor per image before the validator sees it); everything above rides along unchanged.
"""
import argparse
import csv
import json
import os
import sys

import torch
import yaml

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--data', required=True)
    ap.add_argument('--text-feats', help='.npz {texts, feats} or a torch-saved {text: vector}; or give --clip-weights and --clip-vocab')
    ap.add_argument('--clip-weights', help='CLIP ViT-B/32 checkpoint (state_dict or TorchScript archive): class names are encoded here')
    ap.add_argument('--clip-vocab', help="CLIP's BPE merges file (bpe_simple_vocab_16e6.txt.gz), with --clip-weights")
    ap.add_argument('--weights', required=True)
    ap.add_argument('--split', default='val')
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--imgsz', type=int, default=640)
    ap.add_argument('--workers', type=int, default=8)
    ap.add_argument('--dtype', default='bf16', choices=['bf16', 'fp32'])
    ap.add_argument('--conf', type=float, default=0.001)
    ap.add_argument('--iou', type=float, default=0.7)
    ap.add_argument('--raw', action='store_true', help='use the raw weights instead of the EMA copy')
    ap.add_argument('--no-fuse', action='store_true', help='keep BatchNorm layers separate (valTAMTR.py fuses, nn/autobackend.py:115)')
    ap.add_argument('--host-postprocess', action='store_true', help='the per-image host loop (engine.Validator); no per-class table, no JSON')
    ap.add_argument('--save-json', action='store_true', help="write predictions.json (the reference's save_json=True)")
    ap.add_argument('--confusion', action='store_true', help='write confusion_matrix.csv and confusion_matrix_normalized.csv')
    ap.add_argument('--curves', action='store_true', help='write PR_curve.csv, P_curve.csv, R_curve.csv and F1_curve.csv')
    ap.add_argument('--device-metrics', action='store_true', help='reduce AP and the curves on the device too (not with --host-postprocess)')
    ap.add_argument('--coco', action='store_true', help='COCO-protocol AP / AR by object size; writes coco_metrics.json')
    ap.add_argument('--coco-max-dets', type=int, nargs='+', default=[1, 10, 100], help='ascending cuts, at most 4 (VisDrone: 1 10 100 500)')
    ap.add_argument('--project', default='runs/val')
    ap.add_argument('--name', default='TAMTR')
    ap.add_argument('--augment', action='store_true', help='test-time augmentation: scaled / mirrored views merged on the device')
    ap.add_argument('--tta-scales', type=float, nargs='+', default=None, help='with --augment: one scale per view (default 1 0.83 0.67)')
    ap.add_argument('--tta-flips', type=int, nargs='+', default=None, choices=[0, 1], help='with --augment: 1 mirrors a view left-right (default 0 1 0)')
    args = ap.parse_args()
    if (args.tta_scales or args.tta_flips) and not args.augment:
        ap.error('--tta-scales / --tta-flips need --augment')
    if (args.text_feats is None) == (args.clip_weights is None and args.clip_vocab is None) or (args.clip_weights is None) != (args.clip_vocab is None):
        ap.error('give either --text-feats, or --clip-weights together with --clip-vocab (not both, not neither)')
    if args.save_json and args.host_postprocess:
        ap.error('--save-json needs the device path (drop --host-postprocess)')
    if args.device_metrics and args.host_postprocess:
        ap.error('--device-metrics needs the device path (drop --host-postprocess)')
    if args.coco and (not 1 <= len(args.coco_max_dets) <= 4 or args.coco_max_dets[0] < 1
                      or any(b <= a for a, b in zip(args.coco_max_dets, args.coco_max_dets[1:]))):
        ap.error('--coco-max-dets takes 1 to 4 ascending positive integers')

    import tamtr_amd  # noqa: F401
    from tamtr_amd import data as D, engine as E
    from tamtr_amd.model import RTDETRDetectionWorldModel
    from tamtr_amd.tta import views_from_cli
    dev = torch.device('cuda', 0)
    with open(args.data) as f:
        spec = yaml.safe_load(f)
    root = spec.get('path', os.path.dirname(os.path.abspath(args.data)))
    names = spec['names'] if isinstance(spec['names'], dict) else dict(enumerate(spec['names']))
    tf = D.TextFeatures.from_args(args.text_feats, args.clip_weights, args.clip_vocab, dev)
    ds = D.PromptDetDataset(os.path.normpath(os.path.join(root, spec[args.split])), names, args.imgsz, augment=False)
    loader = D.build_dataloader(ds, args.batch, args.workers, shuffle=False)
    model = RTDETRDetectionWorldModel(nc=len(names)).to(dev)
    ck = torch.load(args.weights, map_location=dev)
    model.load_state_dict(ck['model' if args.raw else 'ema'])
    model.set_text_features(tf.encode([v.split('/')[0] for v in names.values()])[None].to(dev))
    model.eval()
    model.autocast_dtype = torch.bfloat16 if args.dtype == 'bf16' else None    # predict() opens its own autocast region from this
    if not args.no_fuse:
        model.fuse()
    save_dir = None
    if args.save_json or args.confusion or args.curves or args.coco:
        from tamtr_amd.predict import increment_path
        save_dir = str(increment_path(os.path.join(args.project, args.name), mkdir=True))
    short = {k: v.split('/')[0] for k, v in names.items()}
    res = E.validate(model, (D.preprocess_batch(b, None, dev) for b in loader), imgsz=args.imgsz, conf=args.conf, iou=args.iou,
                     autocast_dtype=torch.bfloat16 if args.dtype == 'bf16' else None, on_device=not args.host_postprocess,
                     save_json=save_dir if args.save_json else None, names=short, confusion=args.confusion,
                     device_metrics=args.device_metrics, curves=args.curves, coco=args.coco, coco_max_dets=tuple(args.coco_max_dets),
                     augment=args.augment, tta_views=views_from_cli(args.tta_scales, args.tta_flips))
    if save_dir is not None:
        res['save_dir'] = save_dir
    if args.confusion:
        res['confusion_csv'], res['confusion_normalized_csv'] = write_confusion(res['confusion_matrix'], [short[k] for k in sorted(short)], save_dir)
    if args.curves:
        res['curves_csv'] = write_curves(res.pop('curves'), short, save_dir)
    if args.coco:
        res['coco_json'] = write_coco(res['coco'], save_dir)
        print('\n'.join(coco_lines(res['coco'])), file=sys.stderr)
    print(json.dumps(res))


COCO_LINES = (('AP', 'Average Precision', '0.50:0.95', '   all', -1), ('AP50', 'Average Precision', '0.50', '   all', -1),
              ('AP75', 'Average Precision', '0.75', '   all', -1), ('APs', 'Average Precision', '0.50:0.95', ' small', -1),
              ('APm', 'Average Precision', '0.50:0.95', 'medium', -1), ('APl', 'Average Precision', '0.50:0.95', ' large', -1),
              ('AR1', 'Average Recall', '0.50:0.95', '   all', 0), ('AR10', 'Average Recall', '0.50:0.95', '   all', 1),
              ('AR100', 'Average Recall', '0.50:0.95', '   all', 2), ('ARs', 'Average Recall', '0.50:0.95', ' small', -1),
              ('ARm', 'Average Recall', '0.50:0.95', 'medium', -1), ('ARl', 'Average Recall', '0.50:0.95', ' large', -1))


def coco_lines(coco):
    """The twelve numbers in the wording of pycocotools' COCOeval.summarize.  maxDets is the cut the number was taken at (the keys AR1,
    AR10, AR100 name the first three cuts of max_dets whatever their values; a cut max_dets does not have prints as maxDets= -1)."""
    md = coco['max_dets']
    out = []
    for key, title, iou, area, cut in COCO_LINES:
        m = md[cut] if cut < len(md) else -1
        out.append(f' {title:<18} ({"AP" if title.endswith("Precision") else "AR"}) @[ IoU={iou:<9} | area={area} | maxDets={m:>3d} ] = {coco[key]:0.3f}')
    return out


def write_coco(coco, save_dir):
    """coco_metrics.json: the 'coco' dict of results() (twelve numbers, max_dets, per_class) as it is."""
    path = os.path.join(save_dir, 'coco_metrics.json')
    with open(path, 'w') as f:
        json.dump(coco, f, indent=1)
    return path


CURVE_FILES = {'PR_curve.csv': ('pr', 'recall'), 'P_curve.csv': ('p', 'confidence'), 'R_curve.csv': ('r', 'confidence'),
               'F1_curve.csv': ('f1', 'confidence')}


def write_curves(curves, names, save_dir):
    """The reference's PR / P / R / F1 plots (utils/metrics.py:894-996) as CSV: the grid, one column per class that has labels (named by
    `names[class]`), and their mean as `all classes` (PR_curve: the mean of the classes that also have predictions).  curves: the 'curves' dict of results(curves=True); {} writes the headers only."""
    classes = curves.get('classes', [])
    px = curves.get('px', [])
    paths = []
    for fname, (key, axis) in CURVE_FILES.items():
        rows = curves.get(key, [])
        paths.append(os.path.join(save_dir, fname))
        with open(paths[-1], 'w', newline='') as f:
            w = csv.writer(f)
            w.writerow([axis] + [names[c] for c in classes] + ['all classes'])
            # the reference's PR plot averages the classes that have predictions too (its prec_values has no other rows)
            mean_of = [k for k, ok in enumerate(curves.get('valid', [])) if ok or key != 'pr']
            for g, x in enumerate(px):
                col = [row[g] for row in rows]
                mean = sum(col[k] for k in mean_of) / len(mean_of) if mean_of else float('nan')    # the mean of no class, as numpy names it
                w.writerow([repr(float(x))] + [repr(float(v)) for v in col] + [repr(mean)])
    return paths


def write_confusion(matrix, names, save_dir):
    """The two tables of the reference's confusion-matrix plot as CSV: counts, and columns divided by (column sum + 1e-9)."""
    ticks = list(names) + ['background']
    total = [sum(col) + 1e-9 for col in zip(*matrix)] if matrix else []
    tables = {'confusion_matrix.csv': matrix, 'confusion_matrix_normalized.csv': [[v / t for v, t in zip(row, total)] for row in matrix]}
    paths = []
    for fname, rows in tables.items():
        paths.append(os.path.join(save_dir, fname))
        with open(paths[-1], 'w', newline='') as f:
            w = csv.writer(f)
            w.writerow(['predicted / true'] + ticks)
            for tick, row in zip(ticks, rows):
                w.writerow([tick] + list(row))
    return paths


if __name__ == '__main__':
    main()
