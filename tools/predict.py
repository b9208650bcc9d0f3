#!/usr/bin/env python3
"""Run a checkpoint on images (the reference's predictTAMTR.py flow): boxes per image, optional annotated copies and YOLO-format
label files under an incremented --project/--name folder; one JSON line at the end.

    python tools/predict.py --weights runs/train/TAMTR/best.pt --text-feats clip_vitb32.npz --data dataset.yaml \
        --source images/ --conf 0.4 --iou 0.6 --batch 4 --save [--save-txt --save-conf]

Instead of --text-feats, --clip-weights ViT-B-32.pt --clip-vocab bpe_simple_vocab_16e6.txt.gz encodes the class names with the package's
own CLIP text tower (tamtr_amd.text), so any name works, not only those of a table.
--augment predicts with test-time augmentation (tamtr_amd.tta): the reference's three views (scales 1 0.83 0.67, the second mirrored), or
--tta-scales / --tta-flips, merged on the device; the JSON line then carries 'tta' under ms_per_image and 'tta_dropped'.
--slice 640 [--slice-overlap 0.2] [--no-slice-full] [--slice-match ios] predicts large frames in slices (tamtr_amd.slicing): overlapping
windows of the full-resolution frame, cut and resized on the device, next to the whole-frame view, merged on the device; the JSON line
then carries 'slice' under ms_per_image, 'views_per_image' and 'slice_dropped'.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description='TAM-TR prediction on images (one HIP postprocess launch per batch)')
    ap.add_argument('--weights', required=True, help="checkpoint written by training ({'model', 'ema', ...} state_dicts)")
    ap.add_argument('--raw', action='store_true', help='use the raw weights instead of the EMA copy')
    ap.add_argument('--text-feats', help='.npz {texts, feats} or a torch-saved {text: vector}; or give --clip-weights and --clip-vocab')
    ap.add_argument('--clip-weights', help='CLIP ViT-B/32 checkpoint (state_dict or TorchScript archive): class names are encoded here')
    ap.add_argument('--clip-vocab', help="CLIP's BPE merges file (bpe_simple_vocab_16e6.txt.gz), with --clip-weights")
    g = ap.add_mutually_exclusive_group(required=True)
    g.add_argument('--data', help="dataset yaml whose 'names' are the classes")
    g.add_argument('--names', help='comma-separated class names')
    ap.add_argument('--source', required=True, help='an image file, a directory of images, or a list file')
    ap.add_argument('--imgsz', type=int, default=640)
    ap.add_argument('--batch', type=int, default=4)
    ap.add_argument('--conf', type=float, default=0.25)
    ap.add_argument('--iou', type=float, default=0.7)
    ap.add_argument('--classes', type=int, nargs='+', default=None, help='keep only these class ids')
    ap.add_argument('--single-cls', action='store_true', help='class-agnostic NMS')
    ap.add_argument('--save', action='store_true', help='write annotated images')
    ap.add_argument('--save-txt', action='store_true', help='write labels/<stem>.txt: cls x y w h (normalised)')
    ap.add_argument('--save-conf', action='store_true', help='append the score to every label line')
    ap.add_argument('--project', default='runs/predict')
    ap.add_argument('--name', default='TAMTR')
    ap.add_argument('--exist-ok', action='store_true', help='reuse --project/--name instead of incrementing it')
    ap.add_argument('--dtype', default='bf16', choices=['bf16', 'fp32'])
    ap.add_argument('--augment', action='store_true', help='test-time augmentation: scaled / mirrored views merged on the device')
    ap.add_argument('--tta-scales', type=float, nargs='+', default=None, help='with --augment: one scale per view (default 1 0.83 0.67)')
    ap.add_argument('--tta-flips', type=int, nargs='+', default=None, choices=[0, 1], help='with --augment: 1 mirrors a view left-right (default 0 1 0)')
    ap.add_argument('--slice', type=int, nargs='+', default=None, metavar='PX', help='sliced prediction: window size in pixels of the original frame (one value, or height width)')
    ap.add_argument('--slice-overlap', type=float, default=0.2, help='with --slice: overlap of neighbouring windows as a fraction of the window')
    ap.add_argument('--no-slice-full', action='store_true', help='with --slice: leave out the whole-frame view')
    ap.add_argument('--slice-match', default='iou', choices=['iou', 'ios'], help='with --slice: the merge suppresses on IoU or on intersection over the smaller box')
    args = ap.parse_args(argv)
    if args.slice is not None and (len(args.slice) > 2 or args.augment):
        ap.error('--slice takes one size or height width, and does not combine with --augment')
    if (args.tta_scales or args.tta_flips) and not args.augment:
        ap.error('--tta-scales / --tta-flips need --augment')
    if (args.text_feats is None) == (args.clip_weights is None and args.clip_vocab is None) or (args.clip_weights is None) != (args.clip_vocab is None):
        ap.error('give either --text-feats, or --clip-weights together with --clip-vocab (not both, not neither)')
    return args


def load_names(args):
    if args.names:
        return dict(enumerate(n.strip() for n in args.names.split(',')))
    import yaml
    with open(args.data) as f:
        names = yaml.safe_load(f)['names']
    return names if isinstance(names, dict) else dict(enumerate(names))


def main(argv=None):
    args = parse_args(argv)
    import torch
    import tamtr_amd  # noqa: F401
    from tamtr_amd import data as D
    from tamtr_amd.model import RTDETRDetectionWorldModel
    from tamtr_amd.predict import Predictor, increment_path
    from tamtr_amd.slicing import slice_windows
    from tamtr_amd.tta import views_from_cli

    dev = torch.device('cuda', 0)
    names = load_names(args)
    model = RTDETRDetectionWorldModel(nc=len(names)).to(dev)
    ck = torch.load(args.weights, map_location=dev)
    model.load_state_dict(ck['model' if args.raw else 'ema'])
    pred = Predictor(model, names, D.TextFeatures.from_args(args.text_feats, args.clip_weights, args.clip_vocab, dev), imgsz=args.imgsz, conf=args.conf, iou=args.iou,
                     classes=args.classes, single_cls=args.single_cls, batch=args.batch, dtype=args.dtype, augment=args.augment,
                     tta_views=views_from_cli(args.tta_scales, args.tta_flips),
                     slice=None if args.slice is None else args.slice[0] if len(args.slice) == 1 else tuple(args.slice),
                     slice_overlap=args.slice_overlap, slice_full=not args.no_slice_full, slice_match=args.slice_match)
    save_dir = increment_path(os.path.join(args.project, args.name), exist_ok=args.exist_ok)
    if args.save or args.save_txt:
        (save_dir / 'labels' if args.save_txt else save_dir).mkdir(parents=True, exist_ok=True)
    n_img = n_det = n_views = 0
    t0 = time.perf_counter()
    for det in pred.predict(args.source):
        n_img += 1
        n_det += len(det)
        if pred.slice:
            n_views += len(slice_windows(det.orig_shape[0], det.orig_shape[1], pred.slice, pred.slice_overlap, pred.slice_full))
        stem = os.path.splitext(os.path.basename(det.path))[0]
        if args.save_txt:
            det.save_txt(save_dir / 'labels' / f'{stem}.txt', save_conf=args.save_conf)
        if args.save:
            det.save(save_dir / os.path.basename(det.path))
    wall = time.perf_counter() - t0
    sp = pred.speed()
    tta = {'tta': round(sp['tta'], 3)} if args.augment else {'slice': round(sp['slice'], 3)} if pred.slice else {}
    print(json.dumps({'images': n_img, 'detections': n_det, 'save_dir': str(save_dir) if (args.save or args.save_txt) else None,
                      'ms_per_image': {'load': round(sp['load'], 3), 'forward': round(sp['h2d'] + sp['forward'], 3), **tta,
                                       'postprocess': round(sp['postprocess'] + sp['d2h'], 3)},
                      **({'augment': True, 'tta_dropped': pred.tta_dropped} if args.augment else {}),
                      **({'slice': list(pred.slice), 'slice_match': pred.slice_match, 'views_per_image': round(n_views / max(n_img, 1), 3),
                          'slice_dropped': pred.slice_dropped} if pred.slice else {}),
                      'wall_s': round(wall, 3), 'dtype': args.dtype, 'imgsz': args.imgsz, 'batch': args.batch}))


if __name__ == '__main__':
    main()
