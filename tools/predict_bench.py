#!/usr/bin/env python3
"""Predictor measurements (profiles/r05_predict.txt):

  (a) postprocess of one batch, B = 16, nq = 300, nc = 10 and 80: ops.detect_postprocess (one HIP launch) against the per-image
      torch path that RTDETRPredictor.postprocess implies (models/rtdetrworld/predict.py:34-78), run on the device with the
      project's host NMS (engine.nms); device events around a >= 1 s window after warm-up;
  (b) the predictor end to end at 640 x 640, bf16, batch 4 and 16, from synthetic JPEG files: images/s and ms/image split into
      load (waiting for decode + resize), H2D, forward, postprocess and D2H (device events).

  (c) --track: the tracker on a seeded synthetic sequence (tests/bytetrack_np.make_scene), per frame: the device path (one
      tamtr_bytetrack_update launch per batch of 4 frames, device events) against a host path on the same detections - one
      device-to-host copy of the batch's detections plus the numpy twin tests/bytetrack_np.py per frame (host clock).  The host side
      is numpy with scipy's assignment, NOT the reference's tracker with `lap`.  With --botsort as well: the same scene seen by a
      panning camera (tests/botsort_np.camera_path), the camera's warps on the device, one tamtr_botsort_update launch per batch
      against the twin tests/botsort_np.py.
  (c*) --track --streams S [--botsort]: the scenes of (c) in S copies with different seeds, tracked by ONE stacked launch per batch
      (one workgroup per stream, tamtr_*_update_streams) next to S single-tracker launches in sequence; ms per launch, and the two
      paths' tables compared bit for bit.
  (c') --gmc: BoT-SORT with its camera-motion estimate on a seeded 640 x 640 sequence (tests/gmc_np.make_frames, 8 frames, batches of
      4, 60 boxes that sit in the scene): the estimate's launches (csrc/gmc.hip) and the tracker launch that reads their warps, device
      events around each, median and 10th / 90th percentile over repeated passes after a warm-up pass, per frame; against a host path
      that makes one copy of the batch and runs the numpy statements tests/gmc_np.py (in fp32) and tests/botsort_np.py (host clock).

  (d) --mot: the MOT evaluation on a seeded synthetic sequence (200 frames, about 100 ground-truth rows per frame, 300 ground-truth
      ids, 600 track ids, nq = 300, batches of 4): the update launch per batch and the end-of-sequence launch (device events around
      each launch, rows already on the device as the tracker leaves them; median and 10th / 90th percentile over repeated passes after
      a warm-up pass), the update as MotEvaluator.update runs it (with the ground truth's upload), and the host path on the same rows:
      the batch's device-to-host copy plus engine.mot_evaluate (numpy and scipy; host clock).
  (e) --hota: the HOTA launches on the same sequence, the same way: the update launch per batch next to the MOT update launch, the
      three end-of-sequence launches, and the host path (the batches' copies plus engine.hota_evaluate).
  (f) --track-map: the track-mAP launches on the same sequence with a seeded score per row: the update launch per batch next to the
      HOTA update launch, the six end-of-sequence launches, the run's accumulation, and the host path (the batches' copies plus
      engine.track_map_evaluate).
  (d*) --mot --streams S / --hota --streams S: the sequence of (d) in S copies with different seeds, scored by ONE stacked update
      launch per batch (one workgroup per stream, tamtr_mot_update_streams / tamtr_hota_update_streams) next to S single-evaluator
      launches in sequence on the same rows, and the end of the S sequences likewise; ms per launch, and the two forms' counts
      compared stream by stream.

  (g) --tta: test-time augmentation at 640 x 640, B = 4, the reference's three views (canvases 640, 576 and 448 at gs 64), nq = 300,
      nc = 10 and 80, in one run (device events, >= 1 s window after warm-up): the three ops.tta_view launches next to their torch
      composition (flip / F.interpolate / F.pad on the device); the ops.tta_merge launch on 900 candidates per image followed by
      ops.detect_postprocess on its 512 rows, next to the torch composition (de-augment, torch.cat, then the per-image host loop of
      (a) with engine.nms), and next to the existing ops.detect_postprocess on one view's 300 rows.

  (h) --slice: sliced prediction of ONE frame of 1500 x 2000 (13 views) and of 2160 x 3840 (33 views) at 640-pixel slices, overlap 0.2,
      imgsz 640, nq = 300, nc = 10: the ops.slice_views launch (device events) next to the same views made on the host
      (data.resize_linear_u8 per window on the predictor's worker threads, host clock) plus the upload of the V stretched inputs
      (to_model_input); the upload of the original frame next to that upload; the ops.slice_merge launch on V * 300 candidates next
      to a torch composition (map and concatenate on the device, then the per-image host loop of (a) with engine.nms).

    python tools/predict_bench.py [--images 64] [--kernel-only] [--track [--botsort [--reid]] [--streams S]] [--gmc] [--mot [--streams S]]
                                  [--hota [--streams S]] [--track-map] [--tta] [--slice]
--kernel-only runs only the kernel loop of (a), for a `rocprofv3 --kernel-trace --stats` run of its own.
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


def synthetic_preds(B, nq, nc, seed=0):
    g = torch.Generator().manual_seed(seed)
    centres = torch.cat([torch.rand(B, 12, 2, generator=g) * 0.8 + 0.1, torch.rand(B, 12, 2, generator=g) * 0.2 + 0.02], -1)
    pick = torch.gather(centres, 1, torch.randint(0, 12, (B, nq, 1), generator=g).expand(B, nq, 4))
    xy = pick[..., :2] + torch.randn(B, nq, 2, generator=g) * 0.01               # clustered: NMS has work to do
    wh = pick[..., 2:] * (0.85 + 0.3 * torch.rand(B, nq, 2, generator=g))
    scores = torch.sigmoid(torch.randn(B, nq, nc, generator=g) * 2 - 2)
    return torch.cat([xy, wh, scores], -1)


def host_loop(y, hw, conf, iou, max_wh=7680):
    """The reference's per-image loop on device tensors, NMS through engine.nms (one IoU matrix to the host per image)."""
    from tamtr_amd.engine import nms, xywh2xyxy
    nd = y.shape[-1]
    bboxes, scores = y.split((4, nd - 4), dim=-1)
    outs = []
    for i, bbox in enumerate(bboxes):
        bbox = xywh2xyxy(bbox)
        score, cls = scores[i].max(-1, keepdim=True)
        idx = score.squeeze(-1) > conf
        pred = torch.cat([bbox, score, cls.to(bbox.dtype)], dim=-1)[idx]
        oi = nms(pred[:, :4] + pred[:, 5:6] * max_wh, pred[:, 4], iou)
        out = pred[oi]
        oh, ow = hw[i]
        out[..., [0, 2]] *= ow
        out[..., [1, 3]] *= oh
        outs.append(out.cpu())
    return outs


def timed(fn, min_s=1.0, warmup=5, chunk=20):
    """Mean ms per call over chunks of `chunk` calls, each chunk bracketed by device events, until >= min_s has passed."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    total_ms, n, t0 = 0.0, 0, time.perf_counter()
    while time.perf_counter() - t0 < min_s:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(chunk):
            fn()
        e1.record()
        e1.synchronize()
        total_ms += e0.elapsed_time(e1)
        n += chunk
    return total_ms / n, n


def bench_postprocess(kernel_only=False):
    from tamtr_amd import ops
    rows = []
    B, nq, conf, iou = 16, 300, 0.25, 0.7
    for nc in (10, 80):
        y = synthetic_preds(B, nq, nc).cuda()
        hw = [(540 + 20 * i, 960 - 10 * i) for i in range(B)]
        hw_dev = torch.tensor(hw, dtype=torch.int32, device='cuda')

        def kernel():
            return ops.detect_postprocess(y, hw_dev, conf, iou)

        def kernel_with_copy():   # what the predictor does: the call plus one device-to-host copy of its outputs
            o, k, c = kernel()
            return torch.cat([o.view(-1), k.view(torch.float32).view(-1), c.view(torch.float32)]).cpu()

        t_k, n_k = timed(kernel)
        if kernel_only:
            rows.append({'nc': nc, 'kernel_ms': t_k, 'iters': n_k})
            continue
        t_kc, _ = timed(kernel_with_copy)
        t_h, n_h = timed(lambda: host_loop(y, hw, conf, iou))
        _, _, counts = kernel()
        rows.append({'B': B, 'nq': nq, 'nc': nc, 'conf': conf, 'iou': iou, 'kept_per_image': round(float(counts.float().mean()), 1),
                     'kernel_ms': round(t_k, 4), 'kernel_plus_d2h_ms': round(t_kc, 4), 'host_loop_ms': round(t_h, 3),
                     'speedup_vs_host_loop': round(t_h / t_kc, 1), 'iters': [n_k, n_h]})
    return rows


def bench_predictor(n_images, batches, conf=1e-5):
    """conf: the seeded weights score below 5e-4, so the reference's 0.25 would leave the postprocess nothing to do."""
    from PIL import Image
    from tamtr_amd import data as D
    from tamtr_amd.model import RTDETRDetectionWorldModel
    from tamtr_amd.predict import Predictor
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests', 'golden'))
    from weights import fill_state
    rng = np.random.default_rng(0)
    names = {i: f'c{i}' for i in range(10)}
    tf = D.TextFeatures.synthetic(list(names.values()))
    rows = []
    with tempfile.TemporaryDirectory() as d:
        for i in range(n_images):
            h, w = ((1080, 1920), (540, 960), (1500, 2000), (640, 640))[i % 4]
            Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(os.path.join(d, f'{i:04d}.jpg'), quality=90)
        for batch in batches:
            torch.manual_seed(0)
            model = RTDETRDetectionWorldModel(nc=len(names))
            model.load_state_dict(fill_state(model.state_dict(), 78))
            pred = Predictor(model.cuda(), names, tf, imgsz=640, conf=conf, iou=0.7, batch=batch, dtype='bf16')
            for _ in pred.predict(d):   # warm-up pass: kernels, libraries, tail-batch shapes
                pass
            pred.times = {k: 0.0 for k in pred.times}
            pred.seen = 0
            t0 = time.perf_counter()
            n_det = sum(len(det) for det in pred.predict(d))
            wall = time.perf_counter() - t0
            sp = pred.speed()
            rows.append({'imgsz': 640, 'dtype': 'bf16', 'batch': batch, 'conf': conf, 'images': pred.seen, 'detections': n_det,
                         'images_per_s': round(pred.seen / wall, 1), 'ms_per_image': {k: round(v, 3) for k, v in sp.items()},
                         'workers': pred.workers})
            del pred, model
            torch.cuda.empty_cache()
    return rows


def bench_track(n_obj, frames=240, B=4, nq=300, capacity=1024, botsort=False):
    """-> one row: ms per frame of the tracker launch (device events) and of the host path (copy + numpy twin, host clock)."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests'))
    import bytetrack_np as T
    import botsort_np as BS
    from tamtr_amd.track import BotSort, ByteTracker
    scene = T.make_scene(1, n_obj=n_obj, frames=frames, fp_every=3, gaps=[(o, 20 + 7 * o, 5 + 10 * (o % 4)) for o in range(min(n_obj, 8))])
    if botsort:
        warps = BS.camera_path(1, frames, jumps={frames // 2: (40.0, 25.0)})
        scene = BS.through_camera(scene, warps)
        warps_d = torch.from_numpy(warps).cuda()
    out = np.zeros((frames, nq, 6), np.float32)
    for i, f in enumerate(scene):
        out[i, :len(f)] = f
    out_d = torch.from_numpy(out).cuda()
    cnt_d = torch.tensor([len(f) for f in scene], dtype=torch.int32).cuda()
    trk = (BotSort if botsort else ByteTracker)('cuda', capacity=capacity, nq=nq)

    def device_pass():
        trk.reset()
        for i in range(0, frames, B):
            res = trk.update(out_d[i:i + B], cnt_d[i:i + B], warps=warps_d[i:i + B]) if botsort else trk.update(out_d[i:i + B], cnt_d[i:i + B])
        return res

    t_dev, n_dev = timed(device_pass, min_s=1.0, warmup=2, chunk=2)
    sd = trk.state_dict()
    trk.check_overflow(sd['hdr'][3])

    def host_pass():
        twin = BS.BotSortNp(capacity=capacity) if botsort else T.ByteTrackNp(capacity=capacity)
        rows = 0
        for i in range(0, frames, B):
            o, c = out_d[i:i + B].cpu().numpy(), cnt_d[i:i + B].cpu().numpy()      # the copy the reference makes per frame, here per batch
            for b in range(len(c)):
                rows += len(twin.update(o[b, :c[b]], warps[i + b]) if botsort else twin.update(o[b, :c[b]]))
        return twin, rows

    host_pass()
    t0 = time.perf_counter()
    twin, rows = host_pass()
    t_host = (time.perf_counter() - t0) * 1e3
    assert np.array_equal(sd['hdr'], twin.state['hdr']), (sd['hdr'], twin.state['hdr'])     # the two paths tracked the same thing
    return {'tracker': 'botsort' if botsort else 'bytetrack', 'objects': n_obj, 'frames': frames, 'frames_per_launch': B, 'nq': nq, 'capacity': capacity,
            'detections_per_frame': round(float(np.mean([len(f) for f in scene])), 1), 'track_rows': rows, 'ids': int(sd['hdr'][1]) - 1,
            'device_launch_ms_per_frame': round(t_dev / frames, 4), 'host_copy_plus_numpy_twin_ms_per_frame': round(t_host / frames, 3),
            'device_passes_timed': n_dev}


def bench_track_streams(n_obj, S, frames=240, F=4, nq=300, capacity=1024, botsort=False, rounds=7):
    """-> one row: ms per launch of ONE stacked launch for S streams (tamtr_*_update_streams, F frames of every stream, one workgroup
    per stream) next to the S single-tracker launches that track the same streams one after another, on bench_track's scene in S
    copies with different seeds.  Both are whole passes over the sequence between device events, taken in turn `rounds` times after a
    warm-up pass of each: median and 10th / 90th percentile.  The two paths must leave the same tables, bit for bit."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests'))
    import bytetrack_np as T
    import botsort_np as BS
    from tamtr_amd.track import BotSort, ByteTracker
    out = np.zeros((frames, S, nq, 6), np.float32)
    cnt = np.zeros((frames, S), np.int32)
    warps = np.zeros((frames, S, 2, 3))
    for s in range(S):
        scene = T.make_scene(1 + s, n_obj=n_obj, frames=frames, fp_every=3, gaps=[(o, 20 + 7 * o, 5 + 10 * (o % 4)) for o in range(min(n_obj, 8))])
        if botsort:
            warps[:, s] = BS.camera_path(1 + s, frames, jumps={frames // 2: (40.0, 25.0)})
            scene = BS.through_camera(scene, warps[:, s])
        for i, f in enumerate(scene):
            out[i, s, :len(f)] = f
            cnt[i, s] = len(f)
    out_d, cnt_d, warps_d = torch.from_numpy(out).cuda(), torch.from_numpy(cnt).cuda(), torch.from_numpy(warps).cuda()
    # frame-major batches for the stack; one contiguous sequence per stream for the single trackers
    so, sc, sw = (t.transpose(0, 1).contiguous() for t in (out_d, cnt_d, warps_d))
    kind = BotSort if botsort else ByteTracker
    kw = {'gmc_method': 'none'} if botsort else {}
    stack = kind('cuda', capacity=capacity, nq=nq, streams=S, **kw)
    singles = [kind('cuda', capacity=capacity, nq=nq, **kw) for _ in range(S)]

    def upd(trk, o, c, w):
        return trk.update(o, c, warps=w) if botsort else trk.update(o, c)

    def stacked_pass():
        stack.reset()
        for i in range(0, frames, F):
            upd(stack, out_d[i:i + F].flatten(0, 1), cnt_d[i:i + F].flatten(0, 1), warps_d[i:i + F].flatten(0, 1))

    def sequential_pass():
        for t in singles:
            t.reset()
        for i in range(0, frames, F):
            for s, t in enumerate(singles):
                upd(t, so[s, i:i + F], sc[s, i:i + F], sw[s, i:i + F])

    def one(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    one(stacked_pass), one(sequential_pass)
    t_stack, t_seq = [], []
    for _ in range(rounds):
        t_stack.append(one(stacked_pass))
        t_seq.append(one(sequential_pass))
    sd = stack.state_dict()
    stack.check_overflow(sd['hdr'][:, 3])
    same = all(np.array_equal(sd[k][s], v) for s, t in enumerate(singles) for k, v in t.state_dict().items())
    assert same, 'the stacked launch and the single-tracker launches left different tables'
    n = -(-frames // F)
    pct = lambda v: [round(float(x) / n, 4) for x in np.percentile(v, [50, 10, 90])]   # noqa: E731
    return {'tracker': 'botsort' if botsort else 'bytetrack', 'objects': n_obj, 'streams': S, 'frames_per_stream_per_launch': F, 'frames': frames,
            'nq': nq, 'capacity': capacity, 'ids_per_stream': (sd['hdr'][:, 1] - 1).tolist(), 'same_tables_bit_for_bit': same,
            'stacked_launch_ms_p50_p10_p90': pct(t_stack), 'sequential_single_launches_ms_p50_p10_p90': pct(t_seq),
            'stacked_ms_per_stream_frame': round(float(np.median(t_stack)) / (frames * S), 4), 'rounds': rounds}


def bench_track_reid(n_obj, frames=240, B=4, nq=300, capacity=1024, dim=256, rounds=3):
    """-> one row: ms per frame of the BoT-SORT launch with ReID (tamtr_botsort_reid_update, feature rows ready), of the gather that
    makes those rows (tamtr_reid_rows, from an fp32 embedding of all nq queries) and of the plain BoT-SORT launch, on bench_track's
    scene with one seeded feature axis per object (tests/botsort_reid_np.object_features) at D = dim; the three are timed in turn,
    `rounds` times, in this process, and the median round is reported; a fourth pass runs the ReID launch with proximity_thresh = -1, which
    leaves the feature updates and removes the gated pairs' dot products.  The numpy twin says how many pairs passed the gate."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests'))
    import botsort_np as BS
    import botsort_reid_np as R
    from tamtr_amd import ops
    from tamtr_amd.track import BotSort
    scene, who = R.make_scene(1, n_obj=n_obj, frames=frames, fp_every=3, gaps=[(o, 20 + 7 * o, 5 + 10 * (o % 4)) for o in range(min(n_obj, 8))])
    warps = BS.camera_path(1, frames, jumps={frames // 2: (40.0, 25.0)})
    scene = BS.through_camera(scene, warps)
    feats = R.object_features(1, who, n_obj, dim)
    rng = np.random.default_rng(1)
    out, embed, keep = np.zeros((frames, nq, 6), np.float32), rng.normal(size=(frames, nq, dim)).astype(np.float32), np.zeros((frames, nq), np.int32)
    for i, (f, ft) in enumerate(zip(scene, feats)):
        out[i, :len(f)] = f
        keep[i] = rng.permutation(nq)
        embed[i, keep[i, :len(f)]] = ft
    out_d, embed_d, keep_d, warps_d = (torch.from_numpy(a).cuda() for a in (out, embed, keep, warps))
    cnt_d = torch.tensor([len(f) for f in scene], dtype=torch.int32).cuda()
    plain, reid = BotSort('cuda', capacity=capacity, nq=nq, gmc_method='none'), BotSort('cuda', capacity=capacity, nq=nq, gmc_method='none', with_reid=True,
                                                                                         reid_dim=dim)
    feat_d = torch.cat([ops.reid_rows(embed_d[i:i + B], keep_d[i:i + B], cnt_d[i:i + B]) for i in range(0, frames, B)])

    def plain_pass():
        plain.reset()
        for i in range(0, frames, B):
            plain.update(out_d[i:i + B], cnt_d[i:i + B], warps=warps_d[i:i + B])

    def reid_pass():
        reid.reset()
        for i in range(0, frames, B):
            ops.botsort_reid_update(out_d[i:i + B], cnt_d[i:i + B], feat_d[i:i + B], reid.state, capacity, warps_d[i:i + B], reid.track_high_thresh,
                                    reid.track_low_thresh, reid.new_track_thresh, reid.match_thresh, reid.max_time_lost, reid.proximity_thresh,
                                    reid.appearance_thresh, reid.workspace)

    def reid_pass_ungated():      # proximity_thresh = -1: no pair passes the gate, so no embedding distance is computed; the matches (and with
        reid.reset()              # them the feature updates) are plain BoT-SORT's
        for i in range(0, frames, B):
            ops.botsort_reid_update(out_d[i:i + B], cnt_d[i:i + B], feat_d[i:i + B], reid.state, capacity, warps_d[i:i + B], reid.track_high_thresh,
                                    reid.track_low_thresh, reid.new_track_thresh, reid.match_thresh, reid.max_time_lost, -1.0,
                                    reid.appearance_thresh, reid.workspace)

    def gather_pass():
        for i in range(0, frames, B):
            ops.reid_rows(embed_d[i:i + B], keep_d[i:i + B], cnt_d[i:i + B])

    t = {'plain': [], 'reid': [], 'reid_ungated': [], 'gather': []}
    for _ in range(rounds):
        for k, fn in (('plain', plain_pass), ('reid_ungated', reid_pass_ungated), ('reid', reid_pass), ('gather', gather_pass)):
            t[k].append(timed(fn, min_s=0.7, warmup=1, chunk=2)[0] / frames)
    sd = reid.state_dict()
    reid.check_overflow(sd['hdr'][3])
    twin = R.BotSortReidNp(dim, capacity=capacity)
    rows = sum(len(twin.update(f, w, ft)) for f, w, ft in zip(scene, warps, feats))
    ev = twin.events
    med = lambda v: round(float(np.median(v)), 4)      # noqa: E731
    return {'tracker': 'botsort+reid', 'objects': n_obj, 'frames': frames, 'frames_per_launch': B, 'nq': nq, 'capacity': capacity, 'D': dim,
            'detections_per_frame': round(float(np.mean([len(f) for f in scene])), 1), 'track_rows': rows, 'ids': int(sd['hdr'][1]) - 1,
            'same_header_as_the_numpy_twin': bool(np.array_equal(sd['hdr'], twin.state['hdr'])), 'gated_pairs_per_frame': round((ev['pairs'] - ev['prox_masked']) / frames, 1), 'cost_pairs_per_frame': round(ev['pairs'] / frames, 1),
            'feature_updates_per_frame': round((ev['match1'] + ev['match2'] + ev['match_unconfirmed']) / frames, 1),
            'reid_launch_ms_per_frame': med(t['reid']), 'reid_launch_without_gated_pairs_ms_per_frame': med(t['reid_ungated']), 'gather_ms_per_frame': med(t['gather']), 'plain_botsort_launch_ms_per_frame': med(t['plain']),
            'rounds_ms_per_frame': {k: [round(x, 4) for x in v] for k, v in t.items()}}


def bench_gmc(frames=8, S=640, B=4, nq=300, n_obj=60, repeats=7):
    """-> one row: ms per frame of the camera-motion estimate's launches and of the BoT-SORT tracker launch that reads its warps
    (device events, median and 10th / 90th percentile over `repeats` passes after one warm-up pass), and of a host path that makes
    one copy of the batch and runs the numpy statements (tests/gmc_np.py, tests/botsort_np.py; host clock, one pass)."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests'))
    import botsort_np as BS
    import gmc_np as G
    from tamtr_amd.track import BotSort
    imgs, truth = G.make_frames(1, S, frames, G.random_motions(2, frames - 1, S=S))
    rng = np.random.default_rng(3)
    pos, dets = rng.uniform(60, S - 100, (n_obj, 2)), []
    for t in range(frames):      # boxes that sit in the scene: they move as the camera's warp says
        pos = pos @ truth[t][:, :2].T + truth[t][:, 2]
        dets.append(np.concatenate([pos, pos + 24, np.full((n_obj, 1), 0.9), np.zeros((n_obj, 1))], 1).astype(np.float32))
    out = np.zeros((frames, nq, 6), np.float32)
    out[:, :n_obj] = np.stack(dets)
    out_d, cnt_d = torch.from_numpy(out).cuda(), torch.full((frames,), n_obj, dtype=torch.int32).cuda()
    fr_d, scale = torch.from_numpy(imgs).cuda(), torch.ones(frames, 2, dtype=torch.float64).cuda()
    trk = BotSort('cuda', nq=nq)
    pct = lambda v: [round(float(np.percentile(v, q)) / B, 4) for q in (50, 10, 90)]   # noqa: E731  per frame
    event = lambda: torch.cuda.Event(enable_timing=True)   # noqa: E731
    gmc, track = [], []
    for rep in range(repeats + 1):
        trk.reset()
        evs = []
        for i in range(0, frames, B):
            e = [event(), event(), event()]
            e[0].record()
            w = trk.estimate_warps(fr_d[i:i + B], cnt_d[i:i + B], scale[i:i + B])
            e[1].record()
            trk.update(out_d[i:i + B], cnt_d[i:i + B], warps=w)
            e[2].record()
            evs.append(e)
        torch.cuda.synchronize()
        if rep:      # the first pass is the warm-up
            gmc += [e[0].elapsed_time(e[1]) for e in evs]
            track += [e[1].elapsed_time(e[2]) for e in evs]
    sd = trk.state_dict()
    t0 = time.perf_counter()
    est, twin, errs = G.GmcNp(np.float32), BS.BotSortNp(capacity=1024), []
    for i in range(0, frames, B):
        f, o, c = fr_d[i:i + B].cpu().numpy(), out_d[i:i + B].cpu().numpy(), cnt_d[i:i + B].cpu().numpy()      # one copy of the batch
        w, _ = est.estimate(f, c)
        for b in range(len(c)):
            twin.update(o[b, :c[b]], w[b])
            errs.append(G.corner_error(w[b], truth[i + b], S, S))
    t_host = (time.perf_counter() - t0) * 1e3
    return {'frames': frames, 'size': S, 'same_tracker_header_on_both_paths': bool(np.array_equal(sd['hdr'], twin.state['hdr'])), 'frames_per_launch': B, 'detections_per_frame': n_obj, 'ids': int(sd['hdr'][1]) - 1,
            'last_batch_stats_keypoints_tracked_inliers_used': trk.last_stats.cpu().tolist(),
            'twin_corner_error_px_max': round(max(errs), 3),
            'gmc_launches_ms_per_frame_p50_p10_p90': pct(gmc), 'botsort_launch_ms_per_frame_p50_p10_p90': pct(track),
            'host_copy_plus_numpy_twins_ms_per_frame': round(t_host / frames, 1), 'passes_timed': repeats}


def mot_scene(frames=200, n_obj=300, nc=10, seed=2):
    """-> per frame (gt [m, 7], tracks [k, 6]): objects live about a third of the sequence (about 100 per frame), every one has two
    track ids (it changes half way), 5 % misses, loose boxes, strays, three distractors and a region per frame."""
    rng = np.random.default_rng(seed)
    start = rng.integers(-frames // 6, frames - frames // 6, n_obj)
    life = rng.integers(frames // 4, frames // 2, n_obj)
    pos, vel = rng.uniform([0, 0], [1800, 1000], (n_obj, 2)), rng.uniform(-2, 2, (n_obj, 2))
    size, cls = rng.uniform(30, 90, (n_obj, 2)), rng.integers(0, nc, n_obj)
    out = []
    for f in range(frames):
        gt, trk = [], []
        for o in np.flatnonzero((start <= f) & (f < start + life)):
            p = pos[o] + vel[o] * f
            box = np.array([p[0], p[1], p[0] + size[o, 0], p[1] + size[o, 1]])
            gt.append([*box, o + 1, cls[o], 0])
            if rng.random() > 0.05:
                jit = rng.normal(0, 0.03, 4) * np.tile(size[o], 2) * (5 if rng.random() < 0.1 else 1)
                trk.append([*(box + jit), 2 * o + 1 + (f - start[o] > life[o] // 2), cls[o]])
        for k in range(3):
            d = [1900 + 70 * k, 50 + f, 1950 + 70 * k, 110 + f]
            gt.append([*d, 0, 0, 1])
            trk.append([*(np.array(d) + rng.normal(0, 1, 4)), 700 + k, rng.integers(0, nc)])
        gt.append([1900, 600, 2200, 900, 0, 0, 2])
        trk.append([1950 + rng.uniform(0, 100), 650, 2100, 800, 710, 0])
        for k in range(5):
            p = rng.uniform([0, 1100], [1800, 1150], 2)
            trk.append([p[0], p[1], p[0] + 40, p[1] + 40, 720 + (5 * f + k) % 200, rng.integers(0, nc)])
        out.append((np.asarray(gt, np.float32).reshape(-1, 7), np.asarray(trk, np.float32).reshape(-1, 6)))
    return out


def bench_mot(frames=200, B=4, nq=300, nc=10, repeats=7):
    from tamtr_amd import engine, ops
    from tamtr_amd.track import MotEvaluator, pack_track_rows
    scene = mot_scene(frames, nc=nc)
    gts, trks = [g for g, _ in scene], [t for _, t in scene]
    tracks_d, tc_d = pack_track_rows(trks, nq, 'cuda')
    ev = MotEvaluator('cuda', nc, nq=nq, ng=300)
    pct = lambda v: [round(float(np.percentile(v, q)), 4) for q in (50, 10, 90)]   # noqa: E731
    event = lambda: torch.cuda.Event(enable_timing=True)   # noqa: E731
    upd, end, full = [], [], []
    for rep in range(repeats + 1):
        pairs, ends = [], []
        for with_upload in (False, True):
            ev.reset()
            for i in range(0, frames, B):
                if not with_upload:
                    gt_d, gc_d = ev.upload(gts[i:i + B])
                e0, e1 = event(), event()
                e0.record()
                if with_upload:
                    ev.update(tracks_d[i:i + B], tc_d[i:i + B], gts[i:i + B])
                else:
                    ops.mot_update(tracks_d[i:i + B], tc_d[i:i + B], gt_d, gc_d, ev.state, nc, ev.gt_capacity, ev.track_capacity, ev.iou, ev.workspace)
                e1.record()
                pairs.append((with_upload, e0, e1))
            e2, e3 = event(), event()
            e2.record()
            ev.end_sequence()
            e3.record()
            ends.append((e2, e3))
        torch.cuda.synchronize()
        if rep:      # the first pass is the warm-up
            upd += [a.elapsed_time(b) for w, a, b in pairs if not w]
            full += [a.elapsed_time(b) for w, a, b in pairs if w]
            end += [a.elapsed_time(b) for a, b in ends]
    dev_counts = ev.counts()      # the evaluator holds the last pass only: reset() came before it

    def host_pass():
        rows = []
        for i in range(0, frames, B):
            t, c = tracks_d[i:i + B].cpu().numpy(), tc_d[i:i + B].cpu().numpy()      # the copy a host evaluation needs, per batch
            rows += [t[b, :c[b]][:, [0, 1, 2, 3, 4, 6]] for b in range(len(c))]
        return engine.mot_evaluate([list(zip(gts, rows))], nc)

    host_pass()
    t_host = []
    for _ in range(3):
        t0 = time.perf_counter()
        host_counts = host_pass()
        t_host.append((time.perf_counter() - t0) * 1e3)
    assert all(np.array_equal(dev_counts[k], host_counts[k]) for k in engine.MOT_COUNT_KEYS), 'the two paths counted different things'
    s = engine.mot_summary(dev_counts)['all']
    return {'frames': frames, 'frames_per_launch': B, 'nq': nq, 'nc': nc, 'gt_rows_per_frame': round(float(np.mean([len(g) for g in gts])), 1),
            'track_rows_per_frame': round(float(np.mean([len(t) for t in trks])), 1), 'gt_ids': s['gt_ids'],
            'track_ids': len({int(i) for t in trks for i in t[:, 4]}), 'MOTA': round(s['MOTA'], 4), 'IDF1': round(s['IDF1'], 4), 'IDSW': s['IDSW'],
            'update_launch_ms_per_batch_p50_p10_p90': pct(upd), 'update_with_gt_upload_ms_per_batch_p50_p10_p90': pct(full),
            'end_sequence_launch_ms_p50_p10_p90': pct(end),
            'host_copy_plus_numpy_twin_ms_per_sequence_p50_min_max': [round(float(np.median(t_host)), 1), round(min(t_host), 1), round(max(t_host), 1)],
            'host_ms_per_batch': round(float(np.median(t_host)) / (frames / B), 3), 'passes_timed': repeats}


def bench_hota(frames=200, B=4, nq=300, nc=10, repeats=7):
    """The HOTA launches on bench_mot's sequence: the update launch per batch (alone, and as HotaEvaluator.update runs it with the ground
    truth's upload), the MOT update launch on the same batches next to it, the three end-of-sequence launches, and the host path on
    the same rows: the batches' device-to-host copies plus engine.hota_evaluate."""
    from tamtr_amd import engine, ops
    from tamtr_amd.track import HotaEvaluator, MotEvaluator, pack_track_rows
    scene = mot_scene(frames, nc=nc)
    gts, trks = [g for g, _ in scene], [t for _, t in scene]
    tracks_d, tc_d = pack_track_rows(trks, nq, 'cuda')
    ev, mot = HotaEvaluator('cuda', nc, nq=nq, ng=300), MotEvaluator('cuda', nc, nq=nq, ng=300)
    pct = lambda v: [round(float(np.percentile(v, q)), 4) for q in (50, 10, 90)]   # noqa: E731
    event = lambda: torch.cuda.Event(enable_timing=True)   # noqa: E731
    upd, end, full, mupd = [], [], [], []
    for rep in range(repeats + 1):
        pairs, ends = [], []
        for mode in ('mot', 'launch', 'upload'):      # a HOTA pass comes last: its counts are read below
            ev.reset(), mot.reset()
            for i in range(0, frames, B):
                if mode != 'upload':
                    gt_d, gc_d = (mot if mode == 'mot' else ev).upload(gts[i:i + B])
                e0, e1 = event(), event()
                e0.record()
                if mode == 'upload':
                    ev.update(tracks_d[i:i + B], tc_d[i:i + B], gts[i:i + B])
                elif mode == 'launch':
                    ops.hota_update(tracks_d[i:i + B], tc_d[i:i + B], gt_d, gc_d, ev.state, nc, ev.caps, ev.iou, ev.workspace)
                else:
                    ops.mot_update(tracks_d[i:i + B], tc_d[i:i + B], gt_d, gc_d, mot.state, nc, mot.gt_capacity, mot.track_capacity, mot.iou, mot.workspace)
                e1.record()
                pairs.append((mode, e0, e1))
            if mode == 'mot':
                continue
            e2, e3 = event(), event()
            e2.record()
            ev.end_sequence()
            e3.record()
            ends.append((e2, e3))
        torch.cuda.synchronize()
        if rep:      # the first pass is the warm-up
            upd += [a.elapsed_time(b) for w, a, b in pairs if w == 'launch']
            full += [a.elapsed_time(b) for w, a, b in pairs if w == 'upload']
            mupd += [a.elapsed_time(b) for w, a, b in pairs if w == 'mot']
            end += [a.elapsed_time(b) for a, b in ends]
    dev_counts = ev.counts()      # the evaluator holds the last ended pass only: reset() came before it
    hdr = ev.state['hdr'].cpu().tolist()

    def host_pass():
        rows = []
        for i in range(0, frames, B):
            t, c = tracks_d[i:i + B].cpu().numpy(), tc_d[i:i + B].cpu().numpy()      # the copy a host evaluation needs, per batch
            rows += [t[b, :c[b]][:, [0, 1, 2, 3, 4, 6]] for b in range(len(c))]
        return engine.hota_evaluate([list(zip(gts, rows))], nc)

    host_pass()
    t_host = []
    for _ in range(3):
        t0 = time.perf_counter()
        host_counts = host_pass()
        t_host.append((time.perf_counter() - t0) * 1e3)
    assert all(np.array_equal(dev_counts[k], host_counts[k]) for k in ('TP', 'FN', 'FP', 'gt_dets', 'trk_dets')), 'the two paths counted different things'
    assert all(np.allclose(dev_counts[k], host_counts[k], rtol=1e-9, atol=0) for k in engine.HOTA_SUM_KEYS), 'the two paths summed different things'
    s = engine.hota_summary(dev_counts)['all']
    n_batches = frames / B
    dev_seq = float(np.median(upd)) * n_batches + float(np.median(end))
    return {'frames': frames, 'frames_per_launch': B, 'nq': nq, 'nc': nc, 'gt_rows_per_frame': round(float(np.mean([len(g) for g in gts])), 1),
            'track_rows_per_frame': round(float(np.mean([len(t) for t in trks])), 1), 'HOTA': round(s['HOTA'], 4), 'DetA': round(s['DetA'], 4),
            'AssA': round(s['AssA'], 4), 'header_after_the_run': hdr[:8],
            'hota_update_launch_ms_per_batch_p50_p10_p90': pct(upd), 'hota_update_with_gt_upload_ms_per_batch_p50_p10_p90': pct(full),
            'mot_update_launch_ms_per_batch_p50_p10_p90': pct(mupd), 'end_sequence_3_launches_ms_p50_p10_p90': pct(end),
            'device_ms_per_sequence': round(dev_seq, 2),
            'host_copy_plus_numpy_twin_ms_per_sequence_p50_min_max': [round(float(np.median(t_host)), 1), round(min(t_host), 1), round(max(t_host), 1)],
            'host_ms_per_batch': round(float(np.median(t_host)) / n_batches, 3), 'passes_timed': repeats}


def bench_eval_streams(kind, S, frames=200, F=4, nq=300, nc=10, rounds=7):
    """-> one row: ONE stacked update launch for S streams (tamtr_<kind>_update_streams: F frames of every stream, one workgroup per
    stream) next to the S single-evaluator launches that score the same streams one after another, on mot_scene in S copies with
    different seeds; likewise the end of the S sequences (one launch set with the stream as a grid dimension next to S in sequence).
    The ground truth is uploaded once, before anything is timed, so the rows are the same for both forms and every timed span holds
    launches only.  A pass is all the update launches of the sequences between device events, then their end between two more; the
    two forms take turns `rounds` times after a warm-up pass of each: median and 10th / 90th percentile, per launch.  The two forms
    must count the same."""
    from tamtr_amd import ops
    from tamtr_amd.track import HotaEvaluator, MotEvaluator, pack_track_rows
    make = MotEvaluator if kind == 'mot' else HotaEvaluator
    scenes = [mot_scene(frames, nc=nc, seed=2 + s) for s in range(S)]
    stack = make('cuda', nc, nq=nq, ng=300, streams=S)
    singles = [make('cuda', nc, nq=nq, ng=300) for _ in range(S)]
    starts = range(0, frames, F)
    # frame-major batches for the stack, one contiguous sequence per stream for the single evaluators
    fm = [pack_track_rows([scenes[s][f][1] for f in range(i, min(i + F, frames)) for s in range(S)], nq, 'cuda') + stack.upload(
        [scenes[s][f][0] for f in range(i, min(i + F, frames)) for s in range(S)]) for i in starts]
    per = [[pack_track_rows([t for _, t in scenes[s][i:i + F]], nq, 'cuda') + ev.upload([g for g, _ in scenes[s][i:i + F]]) for i in starts]
           for s, ev in enumerate(singles)]
    gt_used = torch.tensor([len(r) for r in stack.rows], dtype=torch.int32).cuda()
    assert [len(r) for r in stack.rows] == [len(ev.rows) for ev in singles]

    def update(ev, tracks, tc, gt, gc, active=None):
        if kind == 'mot':
            ops.mot_update(tracks, tc, gt, gc, ev.state, nc, *ev.caps, ev.iou, ev.workspace, ev.streams, active)
        else:
            ops.hota_update(tracks, tc, gt, gc, ev.state, nc, ev.caps, ev.iou, ev.workspace, ev.streams, active)

    def end(ev):
        used = gt_used if ev.streams else len(ev.rows)
        if kind == 'mot':
            ops.mot_end_sequence(ev.state, nc, *ev.caps, used, ev.workspace, ev.streams)
        else:
            ops.hota_end_sequence(ev.state, nc, ev.caps, ev.nq, ev.ng, ev.workspace, streams=ev.streams)

    def one(evs, batches_of):
        for ev in evs:
            for v in ev.state.values():
                v.zero_()
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        for k in range(len(starts)):
            for j, ev in enumerate(evs):
                update(ev, *batches_of[j][k])
        e[1].record()
        for ev in evs:
            end(ev)
        e[2].record()
        e[2].synchronize()
        return e[0].elapsed_time(e[1]) / len(starts), e[1].elapsed_time(e[2])

    one([stack], [fm]), one(singles, per)
    t_stack, t_seq = [], []
    for _ in range(rounds):
        t_stack.append(one([stack], [fm]))
        t_seq.append(one(singles, per))
    ints =[k for k, v in singles[0].counts().items() if v.dtype.kind == 'i']
    for s, ev in enumerate(singles):
        a, b = stack.stream_counts(s), ev.counts()
        assert all(np.array_equal(a[k], b[k]) if k in ints else np.allclose(a[k], b[k], rtol=1e-9, atol=0) for k in b), f'stream {s} counted differently'
    pct = lambda v: [round(float(x), 4) for x in np.percentile(v, [50, 10, 90])]   # noqa: E731
    up_stack, up_seq = [u for u, _ in t_stack], [u for u, _ in t_seq]
    return {'evaluator': kind, 'streams': S, 'frames_per_stream_per_launch': F, 'frames': frames, 'nq': nq, 'nc': nc,
            'gt_rows_per_frame': round(float(np.mean([len(g) for sc in scenes for g, _ in sc])), 1),
            'track_rows_per_frame': round(float(np.mean([len(t) for sc in scenes for _, t in sc])), 1), 'same_counts_per_stream': True,
            'stacked_update_launch_ms_p50_p10_p90': pct(up_stack), 'sequential_single_update_launches_ms_p50_p10_p90': pct(up_seq),
            'update_sequential_over_stacked': round(float(np.median(up_seq) / np.median(up_stack)), 2),
            'stacked_end_ms_p50_p10_p90': pct([x for _, x in t_stack]), 'sequential_single_ends_ms_p50_p10_p90': pct([x for _, x in t_seq]),
            'rounds': rounds}


def bench_trackmap(frames=200, B=4, nq=300, nc=10, repeats=7):
    """The track-mAP launches on bench_mot's sequence with a seeded score per row: the update launch per batch (alone, and as
    TrackMapEvaluator.update runs it with the ground truth's upload), the HOTA update launch on the same batches as the yardstick (it
    does the same steps 1 and 2 and pair-table work), the six end-of-sequence launches, the run's accumulation, and the host path on
    the same rows: the batches' device-to-host copies plus engine.track_map_evaluate and track_map_summary."""
    from tamtr_amd import engine, ops
    from tamtr_amd.track import HotaEvaluator, TrackMapEvaluator, pack_track_rows
    rng = np.random.default_rng(17)
    scene = mot_scene(frames, nc=nc)
    gts = [g for g, _ in scene]
    trks = [np.concatenate([t, rng.uniform(0.05, 1.0, (len(t), 1)).astype(np.float32)], 1) for _, t in scene]
    tracks_d, tc_d = pack_track_rows(trks, nq, 'cuda')
    ev, hota = TrackMapEvaluator('cuda', nc, nq=nq, ng=300), HotaEvaluator('cuda', nc, nq=nq, ng=300)
    pct = lambda v: [round(float(np.percentile(v, q)), 4) for q in (50, 10, 90)]   # noqa: E731
    event = lambda: torch.cuda.Event(enable_timing=True)   # noqa: E731
    upd, end, full, hupd, acc = [], [], [], [], []
    for rep in range(repeats + 1):
        pairs, ends = [], []
        for mode in ('hota', 'launch', 'upload'):      # a track-mAP pass comes last: its counts are read below
            ev.reset(), hota.reset()
            for i in range(0, frames, B):
                if mode != 'upload':
                    gt_d, gc_d = (hota if mode == 'hota' else ev).upload(gts[i:i + B])
                e0, e1 = event(), event()
                e0.record()
                if mode == 'upload':
                    ev.update(tracks_d[i:i + B], tc_d[i:i + B], gts[i:i + B])
                elif mode == 'launch':
                    ops.trackmap_update(tracks_d[i:i + B], tc_d[i:i + B], gt_d, gc_d, ev.state, nc, ev.caps, ev.iou, ev.workspace)
                else:
                    ops.hota_update(tracks_d[i:i + B], tc_d[i:i + B], gt_d, gc_d, hota.state, nc, hota.caps, hota.iou, hota.workspace)
                e1.record()
                pairs.append((mode, e0, e1))
            if mode == 'hota':
                continue
            e2, e3, e4 = event(), event(), event()
            e2.record()
            ev.end_sequence()
            e3.record()
            ops.trackmap_accumulate(ev.state, nc, ev.caps, len(ev.thresholds))
            e4.record()
            ends.append((e2, e3, e4))
        torch.cuda.synchronize()
        if rep:      # the first pass is the warm-up
            upd += [a.elapsed_time(b) for w, a, b in pairs if w == 'launch']
            full += [a.elapsed_time(b) for w, a, b in pairs if w == 'upload']
            hupd += [a.elapsed_time(b) for w, a, b in pairs if w == 'hota']
            end += [a.elapsed_time(b) for a, b, _ in ends]
            acc += [b.elapsed_time(c) for _, b, c in ends]
    dev_counts, dev_res = ev.counts(), ev.results()      # the evaluator holds the last ended pass only: reset() came before it
    hdr = ev.state['hdr'].cpu().tolist()

    def host_pass():
        rows = []
        for i in range(0, frames, B):
            t, c = tracks_d[i:i + B].cpu().numpy(), tc_d[i:i + B].cpu().numpy()      # the copy a host evaluation needs, per batch
            rows += [t[b, :c[b]][:, [0, 1, 2, 3, 4, 6, 5]] for b in range(len(c))]
        counts = engine.track_map_evaluate([list(zip(gts, rows))], nc)
        return counts, engine.track_map_summary(counts)

    host_pass()
    t_host = []
    for _ in range(3):
        t0 = time.perf_counter()
        host_counts, host_res = host_pass()
        t_host.append((time.perf_counter() - t0) * 1e3)
    assert all(np.array_equal(dev_counts[k], host_counts[k]) for k in ('cls', 'bits', 'gt_tracks')), 'the two paths matched different things'
    assert np.allclose(dev_counts['score'], host_counts['score'], rtol=1e-9, atol=0), 'the two paths scored different things'
    assert np.allclose(dev_res['all']['AP_thr'], host_res['all']['AP_thr'], rtol=1e-9, atol=0), 'the two paths accumulated different things'
    n_batches = frames / B
    dev_seq = float(np.median(upd)) * n_batches + float(np.median(end))
    return {'frames': frames, 'frames_per_launch': B, 'nq': nq, 'nc': nc, 'gt_rows_per_frame': round(float(np.mean([len(g) for g in gts])), 1),
            'track_rows_per_frame': round(float(np.mean([len(t) for t in trks])), 1), 'tracks': dev_res['all']['tracks'],
            'gt_tracks': dev_res['all']['gt_tracks'], 'AP': round(dev_res['all']['AP'], 4), 'AP_thr': [round(v, 4) for v in dev_res['all']['AP_thr']],
            'header_after_the_run': hdr[:8],
            'tmap_update_launch_ms_per_batch_p50_p10_p90': pct(upd), 'tmap_update_with_gt_upload_ms_per_batch_p50_p10_p90': pct(full),
            'hota_update_launch_ms_per_batch_p50_p10_p90': pct(hupd), 'end_sequence_6_launches_ms_p50_p10_p90': pct(end),
            'accumulate_ms_p50_p10_p90': pct(acc), 'tmap_update_launch_ms_per_frame': round(float(np.median(upd)) / B, 4),
            'device_ms_per_sequence': round(dev_seq, 2),
            'host_copy_plus_numpy_twin_ms_per_sequence_p50_min_max': [round(float(np.median(t_host)), 1), round(min(t_host), 1), round(max(t_host), 1)],
            'host_ms_per_batch': round(float(np.median(t_host)) / n_batches, 3), 'passes_timed': repeats}


def bench_tta(B=4, S=640, nq=300, conf=0.25, iou=0.7):
    import torch.nn.functional as F
    from tamtr_amd import ops, tta
    views = tta.DEFAULT_VIEWS
    x = torch.rand(B, 3, S, S, generator=torch.Generator().manual_seed(0)).cuda()
    canvases = [ops.tta_view_sizes(S, S, r, tta.GS) for r, _ in views]

    def view_kernels():
        return [ops.tta_view(x, r, f, tta.GS) for r, f in views]

    def view_torch():
        out = []
        for (r, f), ((sh, sw), (hp, wp)) in zip(views, canvases):
            v = x.flip(3) if f else x
            v = v if r == 1.0 else F.interpolate(v, size=(sh, sw), mode='bilinear', align_corners=False)
            out.append(F.pad(v, [0, wp - sw, 0, hp - sh], value=0.447))
        return out

    t_vk, n_vk = timed(view_kernels)
    t_vt, n_vt = timed(view_torch)
    bytes_moved = 4 * B * 3 * sum(S * S + hp * wp for _, (hp, wp) in canvases)      # every view reads the input once and writes its canvas
    rows = [{'what': 'views', 'B': B, 'size': S, 'canvases': [c[1] for c in canvases], 'kernels_ms': round(t_vk, 4), 'torch_ms': round(t_vt, 4),
             'speedup_vs_torch': round(t_vt / t_vk, 2), 'kernels_GB_per_s': round(bytes_moved / t_vk / 1e6, 1), 'iters': [n_vk, n_vt]}]
    hw = [(540 + 20 * i, 960 - 10 * i) for i in range(B)]
    hw_dev = torch.tensor(hw, dtype=torch.int32, device='cuda')
    table = ops.tta_view_factors(views, (S, S), tta.GS)
    for nc in (10, 80):
        ys = [synthetic_preds(B, nq, nc, seed=v).cuda() for v in range(len(views))]

        def merge():
            return ops.tta_merge(ys, views, conf, iou, size=(S, S), gs=tta.GS)

        def merge_and_postprocess():
            return ops.detect_postprocess(merge()[0], hw_dev, conf, iou)

        def merge_postprocess_copy():   # what the predictor does: both launches plus one device-to-host copy of the outputs
            o, k, c = merge_and_postprocess()
            return torch.cat([o.view(-1), k.view(torch.float32).view(-1), c.view(torch.float32)]).cpu()

        def torch_composition():        # de-augment and concatenate on the device, then the per-image host loop of (a)
            parts = []
            for y, (kx, ky, f) in zip(ys, table):
                cx = y[..., 0:1] * kx
                parts.append(torch.cat([1 - cx if f else cx, y[..., 1:2] * ky, y[..., 2:3] * kx, y[..., 3:4] * ky, y[..., 4:]], -1))
            return host_loop(torch.cat(parts, 1), hw, conf, iou)

        t_m, n_m = timed(merge)
        t_mp, _ = timed(merge_and_postprocess)
        t_mpc, _ = timed(merge_postprocess_copy)
        t_one, _ = timed(lambda: ops.detect_postprocess(ys[0], hw_dev, conf, iou))
        t_h, n_h = timed(torch_composition)
        _, _, counts, dropped = merge()
        rows.append({'what': 'merge', 'B': B, 'V': len(views), 'nq': nq, 'nc': nc, 'conf': conf, 'iou': iou,
                     'merged_per_image': round(float(counts.float().mean()), 1), 'dropped': int(dropped.sum()), 'merge_ms': round(t_m, 4),
                     'merge_plus_postprocess_ms': round(t_mp, 4), 'merge_postprocess_d2h_ms': round(t_mpc, 4),
                     'detect_postprocess_nq300_ms': round(t_one, 4), 'torch_cat_host_loop_ms': round(t_h, 3),
                     'speedup_vs_torch': round(t_h / t_mpc, 1), 'iters': [n_m, n_h]})
    return rows


def host_timed(fn, min_s=1.0, warmup=2):
    """Median ms per call on the host clock (the call synchronises itself where it uses the device), until >= min_s has passed."""
    for _ in range(warmup):
        fn()
    ts, t0 = [], time.perf_counter()
    while time.perf_counter() - t0 < min_s or len(ts) < 3:
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return float(np.median(ts)), len(ts)


def bench_slice(S=640, sl=640, overlap=0.2, nq=300, nc=10, conf=0.25, iou=0.7):
    from concurrent.futures import ThreadPoolExecutor
    from tamtr_amd import data as D, ops, slicing
    from tamtr_amd.predict import _pinned_copy, allowed_cpus, letterbox_scalefill, to_model_input
    dev = torch.device('cuda', 0)
    rows = []
    for h, w in ((1500, 2000), (2160, 3840)):
        im = np.random.default_rng(h).integers(0, 256, (h, w, 3), dtype=np.uint8)
        wins = slicing.slice_windows(h, w, sl, overlap)
        V = len(wins)
        src = torch.from_numpy(im).cuda()
        out = torch.empty(V, 3, S, S, device='cuda')
        t_views, n_views = timed(lambda: ops.slice_views(src, wins, S, out=out))
        crop_bytes = 3 * sum((x1 - x0) * (y1 - y0) for x0, y0, x1, y1 in wins.tolist())

        def upload_orig():
            t = _pinned_copy(im).to(dev, non_blocking=True)
            torch.cuda.synchronize()
            return t

        with ThreadPoolExecutor(max_workers=allowed_cpus()) as pool:
            def host_views():
                return np.stack(list(pool.map(lambda q: letterbox_scalefill(np.ascontiguousarray(im[q[1]:q[3], q[0]:q[2]]), S), wins.tolist())))

            t_hv, _ = host_timed(host_views)
            stretched = host_views()

        def upload_views():
            x = to_model_input(stretched, dev)
            torch.cuda.synchronize()
            return x

        t_uo, _ = host_timed(upload_orig)
        t_uv, _ = host_timed(upload_views)
        assert torch.equal(upload_views(), ops.slice_views(src, wins, S))      # the two paths make the same network inputs
        y = synthetic_preds(V, nq, nc, seed=h).cuda()
        off, hws = [0, V], [(h, w)]
        fac = torch.from_numpy(ops.slice_view_factors(wins, off, hws)).cuda()[:, None, :]

        def merge():
            return ops.slice_merge(y, off, wins, hws, conf, iou)

        def merge_postprocess_copy():   # what the predictor does: both launches plus one device-to-host copy of the outputs
            o, k, c = ops.detect_postprocess(merge()[0], hws, conf, iou)
            return torch.cat([o.view(-1), k.view(torch.float32).view(-1), c.view(torch.float32)]).cpu()

        def torch_composition():        # map and concatenate on the device, then the per-image host loop of (a)
            m = torch.cat([y[..., 0:1] * fac[..., 2:3] + fac[..., 0:1], y[..., 1:2] * fac[..., 3:4] + fac[..., 1:2], y[..., 2:3] * fac[..., 2:3],
                           y[..., 3:4] * fac[..., 3:4], y[..., 4:]], -1)
            return host_loop(m.reshape(1, V * nq, 4 + nc), hws, conf, iou)

        t_m, n_m = timed(merge)
        t_mpc, _ = timed(merge_postprocess_copy)
        t_h, n_h = timed(torch_composition)
        _, _, counts, dropped, overflow = merge()
        passing = int((y[..., 4:].max(-1).values > conf).sum())
        rows.append({'frame': [h, w], 'slice': sl, 'overlap': overlap, 'imgsz': S, 'views': V, 'nq': nq, 'nc': nc,
                     'slice_views_ms': round(t_views, 4), 'slice_views_GB_per_s': round((crop_bytes + 4 * V * 3 * S * S) / t_views / 1e6, 1),
                     'host_views_ms': round(t_hv, 2), 'host_workers': allowed_cpus(), 'upload_original_ms': round(t_uo, 3),
                     'upload_V_inputs_ms': round(t_uv, 3), 'device_path_ms': round(t_uo + t_views, 3), 'host_path_ms': round(t_hv + t_uv, 3),
                     'candidates': V * nq, 'passing': passing, 'merged': int(counts[0]), 'dropped': int(dropped[0]), 'overflow': int(overflow[0]),
                     'slice_merge_ms': round(t_m, 4), 'merge_postprocess_d2h_ms': round(t_mpc, 4), 'torch_map_cat_host_loop_ms': round(t_h, 3),
                     'speedup_vs_torch': round(t_h / t_mpc, 1), 'iters': [n_views, n_m, n_h]})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=64)
    ap.add_argument('--kernel-only', action='store_true')
    ap.add_argument('--track', action='store_true', help='only (c): the tracker launch against copy + numpy twin')
    ap.add_argument('--botsort', action='store_true', help='with --track: the BoT-SORT form of the launch, with warps on the device')
    ap.add_argument('--streams', type=int, help='with --track [--botsort]: S streams in one stacked launch (one workgroup per stream) next to S '
                    'single-tracker launches in sequence, on S copies of the scenes with different seeds; with --mot or --hota: the same for '
                    'the stacked evaluator launches')
    ap.add_argument('--reid', action='store_true', help='with --track --botsort: the ReID launch and the feature gather next to the plain BoT-SORT '
                    'launch on the same scene, D = 256')
    ap.add_argument('--gmc', action='store_true', help="only (c'): BoT-SORT's camera-motion estimate and tracker launch on a 640 x 640 sequence")
    ap.add_argument('--mot', action='store_true', help='only (d): the MOT evaluation launches against copy + numpy twin')
    ap.add_argument('--hota', action='store_true', help='only (e): the HOTA launches against copy + numpy twin, on the sequence of --mot')
    ap.add_argument('--track-map', action='store_true', help='only (f): the track-mAP launches against copy + numpy twin, on the sequence of --hota '
                    'with scores added, next to the HOTA update launch')
    ap.add_argument('--tta', action='store_true', help='only (g): the test-time-augmentation view and merge launches against their torch compositions')
    ap.add_argument('--slice', action='store_true', help='only (h): the sliced-prediction view and merge launches against the host views and a torch composition')
    args = ap.parse_args()
    import tamtr_amd  # noqa: F401
    assert torch.cuda.is_available(), 'predict_bench needs an MI355X'
    print(torch.cuda.get_device_name(0), 'torch', torch.__version__)
    if args.streams is not None and (not (args.track or args.mot or args.hota) or args.streams < 1 or args.reid):
        ap.error('--streams S (S >= 1) goes with --track [--botsort], --mot or --hota')
    if (args.mot or args.hota) and args.streams:
        kind = 'mot' if args.mot else 'hota'
        print(f'(d*) {args.streams} streams: one stacked {kind} update launch per 4 frames of every stream vs {args.streams} single-evaluator launches '
              'in sequence, and the end of the sequences likewise (device events around whole passes, taken in turn)')
        print(json.dumps(bench_eval_streams(kind, args.streams)))
        return
    if args.track and args.streams:
        print(f'(c*) {args.streams} streams: one stacked launch per 4 frames of every stream vs {args.streams} single-tracker launches in sequence '
              '(device events around whole passes, taken in turn)')
        for n_obj in (24, 100):
            print(json.dumps(bench_track_streams(n_obj, args.streams, botsort=args.botsort)))
        return
    if args.track:
        print('(c) tracker per frame: one launch per 4 frames (device events) vs device-to-host copy + numpy twin (host clock; numpy and scipy, not the reference with lap)')
        for n_obj in (24, 100):
            print(json.dumps(bench_track(n_obj, botsort=args.botsort)))
        if args.botsort and args.reid:
            print('(c+) BoT-SORT with ReID per frame: the ReID launch (rows ready), the gather of the rows and the plain launch, timed in turn (device events)')
            for n_obj in (24, 100):
                print(json.dumps(bench_track_reid(n_obj)))
        return
    if args.gmc:
        print("(c') BoT-SORT with camera-motion compensation, per frame: the estimate's launches and the tracker launch per 4 frames (device events) vs one "
              'copy of the batch + the numpy statements (host clock)')
        print(json.dumps(bench_gmc()))
        return
    if args.mot:
        print('(d) MOT evaluation: update launch per batch of 4 frames and end-of-sequence launch (device events) vs device-to-host copy + numpy twin (host clock)')
        print(json.dumps(bench_mot()))
        return
    if args.hota:
        print('(e) HOTA: update launch per batch of 4 frames and the end-of-sequence launches (device events) vs device-to-host copy + numpy twin (host clock)')
        print(json.dumps(bench_hota()))
        return
    if args.track_map:
        print('(f) track-mAP: update launch per batch of 4 frames, the end-of-sequence launches and the accumulation (device events) vs device-to-host '
              'copy + numpy twin (host clock)')
        print(json.dumps(bench_trackmap()))
        return
    if args.tta:
        print('(g) test-time augmentation, one batch of 4 at 640 x 640, three views (device events, >= 1 s window after 5 warm-up calls)')
        for r in bench_tta():
            print(json.dumps(r))
        return
    if args.slice:
        print('(h) sliced prediction of one frame, 640-pixel slices at overlap 0.2 plus the whole frame, imgsz 640 (device events, >= 1 s window after '
              '5 warm-up calls; host paths on the host clock, median)')
        for r in bench_slice():
            print(json.dumps(r))
        return
    if args.kernel_only:
        print(json.dumps({'postprocess_kernel_only': bench_postprocess(True)}))
        return
    print('(a) postprocess of one batch (device events, >= 1 s window after 5 warm-up calls)')
    for r in bench_postprocess():
        print(json.dumps(r))
    print(f'(b) predictor end to end, {args.images} synthetic JPEGs (1920x1080 / 960x540 / 2000x1500 / 640x640), second pass timed')
    for r in bench_predictor(args.images, (4, 16)):
        print(json.dumps(r))


if __name__ == '__main__':
    main()
