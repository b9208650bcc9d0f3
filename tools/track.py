#!/usr/bin/env python3
"""Track objects through image sequences (the reference's model.track flow with ByteTrack or BoT-SORT): per frame the boxes of the confirmed
tracks with their ids; optional annotated copies, YOLO-format label files with the id appended, and one VisDrone-MOT result file per
sequence, under an incremented --project/--name folder; one JSON line at the end.  With --gt the tracks are scored on the device
as they are made (CLEAR-MOT and identity metrics, tam-tr_amd/csrc/mot.hip): a table per sequence and over all, and mot_metrics.json;
--hota scores them by HOTA as well (tam-tr_amd/csrc/hota.hip): its tables next to the others and a `hota` key in mot_metrics.json.
--track-map scores them by track-mAP, the score VisDrone-MOT ranks by (tam-tr_amd/csrc/trackmap.hip): AP over whole tracks at
--track-map-iou (default 0.25 0.5 0.75), a table per sequence and over all, and a `track_map` key in mot_metrics.json.

    python tools/track.py --weights runs/train/TAMTR/best.pt --text-feats clip_vitb32.npz --data dataset.yaml \
        --source sequences/ [--tracker bytetrack.yaml | --tracker botsort.yaml [--gmc none] [--reid on]] --conf 0.1 --batch 4 --save-mot [--save --save-txt --save-conf] [--gt annotations/]

--source is a directory of frames (one sequence, frames in sorted order) or a directory of sequence directories (the VisDrone-MOT
`sequences/<name>/` layout); the tracker is reset for every sequence.  --save-mot writes <save_dir>/<sequence>.txt with lines
`frame,id,left,top,width,height,score,category,-1,-1`, frames 1-based.  --tracker takes the reference's bytetrack.yaml or botsort.yaml (track.tracker_from_yaml); BoT-SORT runs on
the device as well: the tracker rule (XYWH filter, warped track states) in the tracker launch, and the camera-motion warps
(gmc_method: sparseOptFlow, the reference's default) estimated from each batch's uploaded frames in at most four more launches
(tam-tr_amd/csrc/gmc.hip).  --gmc overrides the yaml's gmc_method: `none` runs identity warps.  --reid overrides the yaml's with_reid:
`on` adds BoT-SORT's appearance association with the decoder's per-query hidden state as the embedding of a detection (gathered
and compared on the device; how well those embeddings tell identities apart with trained weights has not been measured).
--gt is a directory of VisDrone-MOT annotation files <sequence>.txt (track.read_mot states how categories become classes and kinds);
a sequence without a file there is tracked but not scored.
--streams S tracks the sequence directories S at a time, as S streams of one batch (Predictor.track_streams: one forward and one
tracker launch, one workgroup per stream, for --batch frames of every stream); the files written are the same per-sequence ones.
--gt does not go with it here: write the tracks with --save-mot and score them with tools/mot_eval.py --streams S, which stacks the
evaluators the same way (Predictor.track_streams takes gt and stacked evaluators itself).
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description='TAM-TR multi-object tracking on image sequences (one HIP tracker launch per batch)')
    ap.add_argument('--weights', required=True, help="checkpoint written by training ({'model', 'ema', ...} state_dicts)")
    ap.add_argument('--raw', action='store_true', help='use the raw weights instead of the EMA copy')
    ap.add_argument('--text-feats', help='.npz {texts, feats} or a torch-saved {text: vector}; or give --clip-weights and --clip-vocab')
    ap.add_argument('--clip-weights', help='CLIP ViT-B/32 checkpoint (state_dict or TorchScript archive): class names are encoded here')
    ap.add_argument('--clip-vocab', help="CLIP's BPE merges file (bpe_simple_vocab_16e6.txt.gz), with --clip-weights")
    g = ap.add_mutually_exclusive_group(required=True)
    g.add_argument('--data', help="dataset yaml whose 'names' are the classes")
    g.add_argument('--names', help='comma-separated class names')
    ap.add_argument('--source', required=True, help='a directory of frames, or a directory of sequence directories')
    ap.add_argument('--tracker', help="tracker yaml with the reference's keys (cfg/trackers/bytetrack.yaml or botsort.yaml); default: "
                    "bytetrack.yaml's values")
    ap.add_argument('--gmc', choices=['sparseOptFlow', 'none'], help="with a botsort.yaml: override its gmc_method (sparseOptFlow = warps "
                    "estimated on the device from the frames, none = identity warps)")
    ap.add_argument('--reid', choices=['on', 'off'], help="with a botsort.yaml: override its with_reid (on = appearance association on the "
                    "decoder's query embeddings, next to IoU; off = IoU only)")
    ap.add_argument('--capacity', type=int, default=1024, help='tracks the device table holds')
    ap.add_argument('--imgsz', type=int, default=640)
    ap.add_argument('--batch', type=int, default=4, help='frames per forward; with --streams: frames of every stream per forward')
    ap.add_argument('--streams', type=int, help='track the sequence directories S at a time, one tracker per stream in one launch')
    ap.add_argument('--conf', type=float, default=0.1, help='keep it at or below track_low_thresh so the second association has input')
    ap.add_argument('--iou', type=float, default=0.7)
    ap.add_argument('--classes', type=int, nargs='+', default=None, help='keep only these class ids')
    ap.add_argument('--single-cls', action='store_true', help='class-agnostic NMS')
    ap.add_argument('--save', action='store_true', help='write annotated frames (id:<n> name score)')
    ap.add_argument('--save-txt', action='store_true', help='write labels/<sequence>/<stem>.txt: cls x y w h [conf] id')
    ap.add_argument('--save-conf', action='store_true', help='put the score before the id on every label line')
    ap.add_argument('--save-mot', action='store_true', help='write <sequence>.txt in the VisDrone-MOT result format')
    ap.add_argument('--gt', help='directory of VisDrone-MOT annotations <sequence>.txt: score the tracks (MOTA, MOTP, IDF1 ...)')
    ap.add_argument('--hota', action='store_true', help='with --gt: HOTA, DetA, AssA ... as well')
    ap.add_argument('--track-map', action='store_true', help='with --gt: track-mAP (AP over whole tracks by spatio-temporal IoU) as well')
    ap.add_argument('--track-map-iou', type=float, nargs='+', default=[0.25, 0.5, 0.75], help='the thresholds of --track-map (1 to 10)')
    ap.add_argument('--mot-iou', type=float, default=0.5, help='IoU a track needs with a ground truth to match it, with --gt')
    ap.add_argument('--project', default='runs/track')
    ap.add_argument('--name', default='TAMTR')
    ap.add_argument('--exist-ok', action='store_true', help='reuse --project/--name instead of incrementing it')
    ap.add_argument('--dtype', default='bf16', choices=['bf16', 'fp32'])
    args = ap.parse_args(argv)
    if (args.text_feats is None) == (args.clip_weights is None and args.clip_vocab is None) or (args.clip_weights is None) != (args.clip_vocab is None):
        ap.error('give either --text-feats, or --clip-weights together with --clip-vocab (not both, not neither)')
    if args.reid and not args.tracker:
        ap.error('--reid overrides a botsort.yaml: give --tracker')
    if args.streams is not None and args.streams < 1:
        ap.error('--streams must be positive')
    if args.streams is not None and args.gt:
        ap.error('--gt does not go with --streams here: write the tracks with --save-mot and score them S sequences at a time with '
                 'tools/mot_eval.py --streams S')
    return args


def list_sequences(source, is_image):
    """-> [(name, directory)]: the sub-directories of `source` that hold frames, sorted; `source` itself when it holds frames."""
    source = os.path.abspath(source)
    if not os.path.isdir(source):
        raise FileNotFoundError(f'{source} is not a directory')
    if any(is_image(os.path.join(source, f)) for f in os.listdir(source)):
        return [(os.path.basename(source.rstrip(os.sep)), source)]
    seqs = [(d, os.path.join(source, d)) for d in sorted(os.listdir(source)) if os.path.isdir(os.path.join(source, d))]
    if not seqs:
        raise FileNotFoundError(f'no frames and no sequence directories in {source}')
    return seqs


def main(argv=None):
    args = parse_args(argv)
    import torch
    import tamtr_amd  # noqa: F401
    from tamtr_amd import data as D
    from tamtr_amd.model import RTDETRDetectionWorldModel
    from tamtr_amd.predict import Predictor, increment_path, is_image_file
    from tamtr_amd import engine
    from tamtr_amd.track import ByteTracker, HotaEvaluator, MotEvaluator, TrackMapEvaluator, read_mot, tracker_from_yaml, write_mot
    from predict import load_names

    dev = torch.device('cuda', 0)
    names = load_names(args)
    model = RTDETRDetectionWorldModel(nc=len(names)).to(dev)
    ck = torch.load(args.weights, map_location=dev)
    model.load_state_dict(ck['model' if args.raw else 'ema'])
    pred = Predictor(model, names, D.TextFeatures.from_args(args.text_feats, args.clip_weights, args.clip_vocab, dev), imgsz=args.imgsz, conf=args.conf,
                     iou=args.iou, classes=args.classes, single_cls=args.single_cls, batch=args.batch, dtype=args.dtype)
    def make_tracker(streams=None):
        if args.tracker:
            over = {**({'gmc_method': args.gmc} if args.gmc else {}), **({'with_reid': args.reid == 'on'} if args.reid else {})}
            return tracker_from_yaml(args.tracker, dev, capacity=args.capacity, reid_dim=model.model[-1].hidden_dim, streams=streams, **over)
        return ByteTracker(dev, capacity=args.capacity, streams=streams)

    tracker = make_tracker() if args.streams is None else None
    save_dir = increment_path(os.path.join(args.project, args.name), exist_ok=args.exist_ok)
    saving = args.save or args.save_txt or args.save_mot or bool(args.gt)
    evaluator = MotEvaluator(dev, len(names), iou=args.mot_iou) if args.gt else None
    hota = HotaEvaluator(dev, len(names), iou=args.mot_iou) if args.gt and args.hota else None
    tmap = TrackMapEvaluator(dev, len(names), thresholds=args.track_map_iou, iou=args.mot_iou) if args.gt and args.track_map else None
    evaluators = [e for e in (evaluator, hota, tmap) if e is not None]
    scored, per_seq = engine.mot_new_counts(len(names)), {}
    tscored, tper_seq = engine.track_map_new_counts(len(names), args.track_map_iou), {}
    hscored, hper_seq = engine.hota_new_counts(len(names)), {}
    class_names = list(names.values()) if isinstance(names, dict) else list(names)
    if saving:
        save_dir.mkdir(parents=True, exist_ok=True)
    n_img = n_rows = n_ids = 0
    t0 = time.perf_counter()
    seqs = list_sequences(args.source, is_image_file)

    def keep(name, det, frames, ids):      # one frame's files and counts
        nonlocal n_img, n_rows
        n_img += 1
        stem = os.path.splitext(os.path.basename(det.path))[0]
        if det.id is not None:
            n_rows += len(det)
            ids.update(det.id.tolist())
        if args.save_txt:
            det.save_txt(save_dir / 'labels' / name / f'{stem}.txt', save_conf=args.save_conf)
        if args.save:
            det.save(save_dir / name / os.path.basename(det.path))
        det.orig_img = None
        frames.append(det)

    groups = [seqs[g:g + args.streams] for g in range(0, len(seqs), args.streams)] if args.streams else []
    trackers = {}      # --streams: one stacked tracker per group size (the last group may be smaller)
    for group in groups:
        frames, ids = [[] for _ in group], [set() for _ in group]
        if len(group) not in trackers:
            trackers[len(group)] = make_tracker(len(group))
        for s, det in pred.track_streams([folder for _, folder in group], tracker=trackers[len(group)], frames_per_stream=args.batch):
            keep(group[s][0], det, frames[s], ids[s])
        n_ids += sum(len(i) for i in ids)
        for (name, _), fr in zip(group, frames):
            if args.save_mot:
                write_mot(save_dir / f'{name}.txt', fr)
    for name, folder in [] if args.streams else seqs:
        frames, ids = [], set()
        gt_file = os.path.join(args.gt, name + '.txt') if args.gt else None
        gt = read_mot(gt_file) if gt_file and os.path.exists(gt_file) else None
        for det in pred.track(folder, tracker=tracker, gt=gt, evaluator=(evaluator if len(evaluators) == 1 else evaluators) if gt is not None else None):     # persist=False: a fresh tracker
            keep(name, det, frames, ids)
        n_ids += len(ids)
        if args.save_mot:
            write_mot(save_dir / f'{name}.txt', frames)
        if gt is not None:
            run = evaluator.counts()
            counts = {k: run[k] - scored[k] for k in run}
            scored = engine.mot_add_counts(scored, counts)
            per_seq[name] = engine.mot_summary(counts, class_names)
            print(engine.mot_table(per_seq[name], name))
            if hota is not None:
                run = hota.counts()
                counts = {k: run[k] - hscored[k] for k in run}
                hscored = engine.hota_add_counts(hscored, counts)
                hper_seq[name] = engine.hota_summary(counts, class_names)
                print(engine.hota_table(hper_seq[name], name))
            if tmap is not None:
                counts = engine.track_map_since(tmap.counts(), tscored)
                tscored = engine.track_map_add_counts(tscored, counts)
                tper_seq[name] = engine.track_map_summary(counts, class_names)
                print(engine.track_map_table(tper_seq[name], name))
    wall = time.perf_counter() - t0
    sp = pred.speed()
    extra = {}
    if args.gt:
        overall = engine.mot_summary(scored, class_names)
        print(engine.mot_table(overall, 'OVERALL'))
        metrics = {'iou': args.mot_iou, 'sequences': per_seq, 'overall': overall}
        if hota is not None:
            metrics['hota'] = {'sequences': hper_seq, 'overall': engine.hota_summary(hscored, class_names)}
            print(engine.hota_table(metrics['hota']['overall'], 'OVERALL'))
        if tmap is not None:      # the overall numbers are the evaluator's own accumulation, on the device
            metrics['track_map'] = {'sequences': tper_seq, 'overall': tmap.results(class_names)}
            print(engine.track_map_table(metrics['track_map']['overall'], 'OVERALL'))
        with open(save_dir / 'mot_metrics.json', 'w') as fh:
            json.dump(metrics, fh, indent=1)
        extra = {'mot': {k: overall['all'][k] for k in ('MOTA', 'MOTP', 'IDF1', 'IDSW', 'FP', 'FN')}, 'mot_ms_per_image': round(sp.get('mot', 0.0), 4),
                 'scored_sequences': len(per_seq)}
        if hota is not None:
            extra['hota'] = {k: metrics['hota']['overall']['all'][k] for k in ('HOTA', 'DetA', 'AssA', 'LocA')}
            extra['hota_ms_per_image'] = round(sp.get('hota', 0.0), 4)
        if tmap is not None:
            extra['track_map'] = {k: metrics['track_map']['overall']['all'][k] for k in ('AP', 'AP_thr', 'AR_thr')}
            extra['tmap_ms_per_image'] = round(sp.get('tmap', 0.0), 4)
    print(json.dumps({**extra, 'sequences': len(seqs), 'images': n_img, 'track_rows': n_rows, 'ids': n_ids, 'save_dir': str(save_dir) if saving else None,
                      'ms_per_image': {'load': round(sp['load'], 3), 'forward': round(sp['h2d'] + sp['forward'], 3),
                                       'postprocess': round(sp['postprocess'], 3), 'track': round(sp['track'], 4), 'd2h': round(sp['d2h'], 3)},
                      'wall_s': round(wall, 3), 'dtype': args.dtype, 'imgsz': args.imgsz, 'batch': args.batch,
                      **({'streams': args.streams} if args.streams else {})}))


if __name__ == '__main__':
    main()
