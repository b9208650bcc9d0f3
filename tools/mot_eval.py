#!/usr/bin/env python3
"""Score VisDrone-MOT result files against annotation files: CLEAR-MOT (MOTA, MOTP, FP, FN, IDSW, Frag, MT / PT / ML) and identity
(IDF1, IDP, IDR) metrics per class, per sequence and over all sequences.  The rule is written out in tam-tr_amd/csrc/mot.hip.

    python tools/mot_eval.py --gt annotations/ --results runs/track/TAMTR/ --names pedestrian,people,... [--host] [--batch 4]

Every `<sequence>.txt` of --results (as tools/track.py --save-mot writes them) is scored against `<sequence>.txt` of --gt.  By default the
frames go through the device path in batches (track.MotEvaluator: one launch per batch, one per sequence); --host runs the numpy
statement of the same rule (engine.mot_evaluate) and needs no GPU.  The tables are printed, then one JSON line.  --hota adds the HOTA
tables (HOTA, DetA, AssA ... per class; the rule is written out in tam-tr_amd/csrc/hota.hip) and a `hota` key to the JSON line, through
the same path: track.HotaEvaluator on the device, engine.hota_evaluate with --host.  --track-map adds track-mAP, the score VisDrone-MOT
ranks by (AP over whole tracks at --track-map-iou, default 0.25 0.5 0.75; the rule is written out in tam-tr_amd/csrc/trackmap.hip), with
the scores of the result files: track.TrackMapEvaluator on the device, engine.track_map_evaluate with --host; a `track_map` key.
--streams S scores the sequences S at a time through stacked evaluators (track.MotEvaluator / HotaEvaluator built with streams=S: one
update launch for --batch frames of every stream, one workgroup per stream) and prints the same tables and the same JSON line.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description='MOT metrics of VisDrone-MOT result files')
    ap.add_argument('--gt', required=True, help='directory of annotation files <sequence>.txt')
    ap.add_argument('--results', required=True, help='directory of result files <sequence>.txt')
    ap.add_argument('--names', required=True, help='comma-separated class names; their number is nc')
    ap.add_argument('--iou', type=float, default=0.5)
    ap.add_argument('--host', action='store_true', help='the numpy path (no GPU)')
    ap.add_argument('--hota', action='store_true', help='score by HOTA as well')
    ap.add_argument('--track-map', action='store_true', help='score by track-mAP as well, with the scores of the result files')
    ap.add_argument('--track-map-iou', type=float, nargs='+', default=[0.25, 0.5, 0.75], help='the spatio-temporal IoU thresholds of track-mAP (1 to 10)')
    ap.add_argument('--batch', type=int, default=4, help='frames per launch on the device path')
    ap.add_argument('--gt-capacity', type=int, default=1024)
    ap.add_argument('--track-capacity', type=int, default=4096)
    ap.add_argument('--rows', type=int, default=300, help='rows per frame the device path is sized for (nq = ng)')
    ap.add_argument('--streams', type=int, default=None, help='score the sequences S at a time through stacked evaluators (device path)')
    args = ap.parse_args(argv)
    if args.streams is not None:
        if args.streams < 1:
            ap.error(f'--streams must be a positive number of sequences to score at once, got {args.streams}')
        if args.host:
            ap.error('--streams stacks evaluator states on the device; --host is the numpy path, which scores one sequence at a time')
        if args.track_map:
            ap.error('--streams does not take --track-map: track.TrackMapEvaluator holds one sequence (its run table appends the tracks in '
                     'the order the sequences end)')
    return args


def score_streams(args, seqs, load, nc, dev):
    """The device path S sequences at a time -> {name: (MOT counts, HOTA counts or None)}.  Group by group: every launch takes
    --batch frames of every stream, frame-major; a stream past its last frame (or a group with fewer than S sequences) keeps its images as
    no frames; the streams whose last frame a batch holds are ended right after it, in one call.  A sequence's counts are its stream's
    totals after the group minus those before it."""
    import numpy as np
    from tamtr_amd import engine
    from tamtr_amd.track import HotaEvaluator, MotEvaluator, pack_track_rows
    S, F = args.streams, args.batch
    kw = dict(iou=args.iou, gt_capacity=args.gt_capacity, track_capacity=args.track_capacity, nq=args.rows, ng=args.rows, streams=S)
    evs = [MotEvaluator(dev, nc, **kw)] + ([HotaEvaluator(dev, nc, **kw)] if args.hota else [])
    prev = [[engine.mot_new_counts(nc) for _ in range(S)]] + ([[engine.hota_new_counts(nc) for _ in range(S)]] if args.hota else [])
    empty, out = np.zeros((0, 6), np.float32), {}
    for i in range(0, len(seqs), S):
        group = seqs[i:i + S]
        data = [load(name) for name in group]
        for k in range(0, max(len(gt) for gt, _ in data), F):
            at = [(k + j // S, j % S) for j in range(F * S)]
            live = [s < len(data) and n < len(data[s][0]) for n, s in at]
            rows = pack_track_rows([data[s][1][n] if a else empty for (n, s), a in zip(at, live)], evs[0].nq, dev)
            ending = [s for s, (gt, _) in enumerate(data) if gt and (len(gt) - 1) // F == k // F]
            for ev in evs:
                ev.update(*rows, [data[s][0][n] if a else None for (n, s), a in zip(at, live)])
                if ending:
                    ev.end_sequence(ending)
        for s, name in enumerate(group):
            got = []
            for e, ev in enumerate(evs):
                run = ev.stream_counts(s)
                got.append({key: run[key] - prev[e][s][key] for key in run})
                prev[e][s] = run
            out[name] = (got[0], got[1] if args.hota else None)
    return out


def main(argv=None):
    args = parse_args(argv)
    import numpy as np
    import tamtr_amd  # noqa: F401
    from tamtr_amd import engine
    from tamtr_amd.track import read_mot
    names = [n.strip() for n in args.names.split(',')]
    nc = len(names)
    seqs = sorted(f[:-4] for f in os.listdir(args.results) if f.endswith('.txt') and os.path.exists(os.path.join(args.gt, f)))
    if not seqs:
        raise FileNotFoundError(f'no <sequence>.txt of {args.results} has an annotation file in {args.gt}')

    def load(name):
        res = read_mot(os.path.join(args.results, name + '.txt'), gt=False, scores=args.track_map)
        gt = read_mot(os.path.join(args.gt, name + '.txt'), frames=len(res))
        return gt, res + [np.zeros((0, 7 if args.track_map else 6), np.float32)] * (len(gt) - len(res))

    stacked = None
    if args.streams is not None:
        import torch
        stacked = score_streams(args, seqs, load, nc, torch.device('cuda', 0))
    elif not args.host:
        import torch
        from tamtr_amd.track import HotaEvaluator, MotEvaluator, TrackMapEvaluator, pack_track_rows
        dev = torch.device('cuda', 0)
        ev = MotEvaluator(dev, nc, iou=args.iou, gt_capacity=args.gt_capacity, track_capacity=args.track_capacity, nq=args.rows, ng=args.rows)
        hev = HotaEvaluator(dev, nc, iou=args.iou, gt_capacity=args.gt_capacity, track_capacity=args.track_capacity, nq=args.rows,
                            ng=args.rows) if args.hota else None
        tev = TrackMapEvaluator(dev, nc, thresholds=args.track_map_iou, iou=args.iou, gt_capacity=args.gt_capacity,
                                track_capacity=args.track_capacity, nq=args.rows, ng=args.rows) if args.track_map else None
    total, per_seq = engine.mot_new_counts(nc), {}
    htotal, hper_seq = engine.hota_new_counts(nc), {}
    ttotal, tper_seq = engine.track_map_new_counts(nc, args.track_map_iou), {}
    for name in seqs:
        gt, res = load(name) if stacked is None else (None, None)      # the stacked path loaded its groups itself
        if stacked is not None:
            counts, hcounts = stacked[name]
        elif args.host:
            counts = engine.mot_evaluate([list(zip(gt, res))], nc, iou=args.iou)
            hcounts = engine.hota_evaluate([list(zip(gt, res))], nc, iou=args.iou) if args.hota else None
            tcounts = engine.track_map_evaluate([list(zip(gt, res))], nc, iou=args.iou, thresholds=args.track_map_iou) if args.track_map else None
        else:
            for i in range(0, len(gt), args.batch):
                rows = pack_track_rows(res[i:i + args.batch], ev.nq, dev)
                ev.update(*rows, gt[i:i + args.batch])
                if args.hota:
                    hev.update(*rows, gt[i:i + args.batch])
                if args.track_map:
                    tev.update(*rows, gt[i:i + args.batch])
            ev.end_sequence()
            run = ev.counts()
            counts = {k: run[k] - total[k] for k in run}
            if args.hota:
                hev.end_sequence()
                run = hev.counts()
                hcounts = {k: run[k] - htotal[k] for k in run}
            if args.track_map:
                tev.end_sequence()
                tcounts = engine.track_map_since(tev.counts(), ttotal)
        total = engine.mot_add_counts(total, counts)
        per_seq[name] = engine.mot_summary(counts, names)
        print(engine.mot_table(per_seq[name], name))
        if args.hota:
            htotal = engine.hota_add_counts(htotal, hcounts)
            hper_seq[name] = engine.hota_summary(hcounts, names)
            print(engine.hota_table(hper_seq[name], name))
        if args.track_map:
            ttotal = engine.track_map_add_counts(ttotal, tcounts)
            tper_seq[name] = engine.track_map_summary(tcounts, names)
            print(engine.track_map_table(tper_seq[name], name))
    overall = engine.mot_summary(total, names)
    print(engine.mot_table(overall, 'OVERALL'))
    extra = {}
    if args.hota:
        extra['hota'] = {'per_sequence': hper_seq, 'overall': engine.hota_summary(htotal, names)}
        print(engine.hota_table(extra['hota']['overall'], 'OVERALL'))
    if args.track_map:      # on the device path the overall numbers are the evaluator's own accumulation
        extra['track_map'] = {'per_sequence': tper_seq, 'overall': engine.track_map_summary(ttotal, names) if args.host else tev.results(names)}
        print(engine.track_map_table(extra['track_map']['overall'], 'OVERALL'))
    print(json.dumps({'sequences': len(seqs), 'path': 'host' if args.host else 'device', 'iou': args.iou, 'per_sequence': per_seq, 'overall': overall,
                      **extra}))


if __name__ == '__main__':
    main()
