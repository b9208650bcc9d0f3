"""Batched image prediction (the reference's predictTAMTR.py / RTDETRPredictor flow): files -> scale-filled batches -> fused
eval forward -> ops.detect_postprocess (one HIP launch per batch: class max, confidence / class filter, class-aware NMS,
scaling to the original size) -> one device-to-host copy per batch -> Detections.

    from tamtr_amd.predict import Predictor
    for det in Predictor(model, names, text_features, conf=0.4, iou=0.6).predict('images/'):
        det.save_txt(...); det.save(...)
"""
import os
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np
import torch

from . import data as D, ops


# ------------------------------------------------------------------------------------------------ files
def is_image_file(path):
    return os.path.isfile(path) and str(path).rsplit('.', 1)[-1].lower() in D.IMG_FORMATS


def list_sources(source):
    """One image file, a directory (recursive) or a list file -> sorted image paths.  An image is recognised by its extension
    before data.list_images, which reads any other existing file as a list of paths."""
    if isinstance(source, (str, os.PathLike)) and is_image_file(str(source)):
        return [str(source)]
    return D.list_images(source)


def increment_path(path, exist_ok=False, sep='', mkdir=False):
    """runs/predict/TAMTR -> runs/predict/TAMTR2, TAMTR3, ... when it exists (ultralytics/utils/files.py:85-117)."""
    path = Path(path)
    if path.exists() and not exist_ok:
        path, suffix = (path.with_suffix(''), path.suffix) if path.is_file() else (path, '')
        for n in range(2, 9999):
            p = f'{path}{sep}{n}{suffix}'
            if not os.path.exists(p):
                break
        path = Path(p)
    if mkdir:
        path.mkdir(parents=True, exist_ok=True)
    return path


def allowed_cpus(cap=16):
    """CPUs this process may run on (not the machine's count), at most `cap`."""
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    return max(1, min(cap, n))


def letterbox_scalefill(im, imgsz):
    """LetterBox(imgsz, auto=False, scaleFill=True) (models/rtdetrworld/predict.py:80-92): a plain cv2 INTER_LINEAR resize to
    imgsz x imgsz, no padding; an image already at that size is returned as it is."""
    h, w = im.shape[:2]
    return im if (h, w) == (imgsz, imgsz) else D.resize_linear_u8(im, imgsz, imgsz)


def load_image(path, imgsz):
    """-> (original RGB u8 [h, w, 3], network input u8 [imgsz, imgsz, 3])."""
    im = D.decode_image(path)
    return im, letterbox_scalefill(im, imgsz)


def load_original(path, imgsz=None):
    """-> (original RGB u8 [h, w, 3], None): the loader of sliced prediction, whose network inputs are cut on the device."""
    return D.decode_image(path), None


def stream_batches(files_per_stream, frames_per_stream=1):
    """The batches of Predictor.track_streams: S file lists (one sequence each) -> [(paths [F * S], active [F * S])] with
    F = frames_per_stream, frame-major: entry f * S + s of batch k is frame k * F + f of stream s.  A stream that has no such frame
    (it ended, or it is empty) keeps its entry: active is False there and the path is the batch's first active one, an image that is
    loaded anyway (padding; its result is dropped).  Batches run until the longest stream ends.  Pure: touches no file."""
    files = [list(f) for f in files_per_stream]
    S, F = len(files), int(frames_per_stream)
    if S < 1:
        raise ValueError('track_streams needs at least one source')
    if F < 1:
        raise ValueError(f'frames_per_stream must be positive, got {frames_per_stream!r}')
    batches = []
    for k in range(0, max(len(f) for f in files), F):
        at = [(k + i // S, i % S) for i in range(F * S)]
        active = [n < len(files[s]) for n, s in at]
        pad = next(files[s][n] for (n, s), a in zip(at, active) if a)
        batches.append(([files[s][n] if a else pad for (n, s), a in zip(at, active)], active))
    return batches


def _as_list(evaluator):
    """One evaluator, a list / tuple of them or None -> a list."""
    return list(evaluator) if isinstance(evaluator, (list, tuple)) else [] if evaluator is None else [evaluator]


def _pad_gt(gt, n):
    """A sequence's per-frame ground truth for n frames: cut to them, missing frames empty."""
    gt = list(gt)[:n]
    return gt + [np.zeros((0, 7), np.float32)] * (n - len(gt))


def sequence_records(files, batch, gt=None):
    """What Predictor's batch loop runs on for ONE sequence: [(paths, active, gt_frames, ending)] per batch, plain chunks of `batch`
    files - no padding (active is None) and the last chunk may be short.  gt_frames: the chunk's slice of `gt` (_pad_gt), or None
    without gt; ending is empty: track() ends the sequence after the last frame.  Pure: touches no file."""
    gt = None if gt is None else _pad_gt(gt, len(files))
    return [(files[i:i + batch], None, None if gt is None else gt[i:i + batch], []) for i in range(0, len(files), batch)]


def stream_records(files_per_stream, frames_per_stream=1, gt=None):
    """The same for S sequences at once, over stream_batches: active is its mask; gt_frames (gt: S entries, a sequence's frames or
    None for a stream that is not scored) holds None for padding and for unscored streams, which are no frames to the evaluators;
    ending: the scored streams whose last frame lies in this batch."""
    files = [list(f) for f in files_per_stream]
    S, F = len(files), int(frames_per_stream)
    gts = None if gt is None else [None if g is None else _pad_gt(g, len(f)) for g, f in zip(gt, files)]
    records = []
    for k, (paths, active) in enumerate(stream_batches(files, frames_per_stream)):
        frames, ending = None, []
        if gts is not None:      # image f * S + s is frame k * F + f of stream s
            frames = [gts[i % S][k * F + i // S] if active[i] and gts[i % S] is not None else None for i in range(len(paths))]
            ending = [s for s, g in enumerate(gts) if g and (len(g) - 1) // F == k]
        records.append((paths, active, frames, ending))
    return records


def to_model_input(ims_u8, device, keep_u8=False):
    """u8 [B, S, S, 3] host batch -> f32 [B, 3, S, S] / 255 on the device (engine/predictor.py:111-129: RGB, CHW, float, / 255).
    keep_u8: -> (that, the u8 batch as it was uploaded), which BoT-SORT's camera-motion estimate reads."""
    t = torch.from_numpy(ims_u8)
    if device.type == 'cuda':
        t = t.pin_memory().to(device, non_blocking=True)
    x = t.permute(0, 3, 1, 2).contiguous().float() / 255
    return (x, t) if keep_u8 else x


def _pinned_copy(a):
    """A host u8 array -> a pinned tensor holding its values (one copy; the array may be read-only, as a decoded image is)."""
    t = torch.empty(a.shape, dtype=torch.uint8, pin_memory=True)
    t.numpy()[...] = a
    return t


# ------------------------------------------------------------------------------------------------ results
class Detections:
    """The boxes of one image (engine/results.py Results + Boxes, detection only): boxes f32 [n, 6] on the host, x1 y1 x2 y2 in
    pixels of the original image, score, class.  id: i64 [n] track ids from Predictor.track, else None."""

    def __init__(self, path, orig_shape, names, boxes, orig_img=None, id=None):
        self.path, self.orig_shape, self.names = path, tuple(orig_shape), names
        self.boxes = boxes
        self.orig_img = orig_img
        self.id = id

    def __len__(self):
        return len(self.boxes)

    @property
    def xyxy(self):
        return self.boxes[:, :4]

    @property
    def conf(self):
        return self.boxes[:, 4]

    @property
    def cls(self):
        return self.boxes[:, 5]

    @property
    def xywhn(self):
        """xyxy2xywh (utils/ops.py:336-356), then / (w, h) of the original image (engine/results.py:436-441)."""
        x = self.xyxy
        y = torch.empty_like(x)
        y[:, 0] = (x[:, 0] + x[:, 2]) / 2
        y[:, 1] = (x[:, 1] + x[:, 3]) / 2
        y[:, 2] = x[:, 2] - x[:, 0]
        y[:, 3] = x[:, 3] - x[:, 1]
        y[:, [0, 2]] /= self.orig_shape[1]
        y[:, [1, 3]] /= self.orig_shape[0]
        return y

    def save_txt(self, txt_file, save_conf=False):
        """`cls x y w h [conf] [id]` per box, '%g'-formatted, appended; no file when there is no box (engine/results.py:278-311)."""
        if not len(self):
            return
        texts = []
        ids = [None] * len(self) if self.id is None else self.id.tolist()
        for c, xywhn, conf, tid in zip(self.cls.tolist(), self.xywhn.tolist(), self.conf.tolist(), ids):
            line = (int(c), *xywhn) + (conf,) * save_conf + (() if tid is None else (int(tid),))
            texts.append(('%g ' * len(line)).rstrip() % line)
        Path(txt_file).parent.mkdir(parents=True, exist_ok=True)
        with open(txt_file, 'a') as f:
            f.writelines(t + '\n' for t in texts)

    def save(self, path, line_width=None):
        """An annotated copy of the original image (boxes and `name score` labels, `id:<n> name score` with track ids; drawn with PIL)."""
        from PIL import Image, ImageDraw
        im = Image.fromarray(self.orig_img if self.orig_img is not None else D.decode_image(self.path))
        draw = ImageDraw.Draw(im)
        lw = line_width or max(round(sum(im.size) / 2 * 0.003), 2)
        ids = [None] * len(self) if self.id is None else self.id.tolist()
        for (x1, y1, x2, y2), conf, c, tid in zip(self.xyxy.tolist(), self.conf.tolist(), self.cls.tolist(), ids):
            color = _COLORS[int(c) % len(_COLORS)]
            draw.rectangle((x1, y1, x2, y2), outline=color, width=lw)
            label = ('' if tid is None else f'id:{int(tid)} ') + f'{self.names.get(int(c), int(c))} {conf:.2f}'
            l, t, r, b = draw.textbbox((x1, y1), label)
            top = y1 - (b - t) - 2 if y1 - (b - t) - 2 >= 0 else y1
            draw.rectangle((x1, top, x1 + (r - l) + 2, top + (b - t) + 2), fill=color)
            draw.text((x1 + 1, top), label, fill=(255, 255, 255))
        Path(path).parent.mkdir(parents=True, exist_ok=True)
        im.save(path)


_COLORS = [(255, 56, 56), (255, 157, 151), (255, 112, 31), (255, 178, 29), (207, 210, 49), (72, 249, 10), (146, 204, 23), (61, 219, 134),
           (26, 147, 52), (0, 212, 187), (44, 153, 168), (0, 194, 255), (52, 69, 147), (100, 115, 255), (0, 24, 236), (132, 56, 255),
           (82, 0, 133), (203, 56, 255), (255, 149, 200), (255, 55, 199)]


# ------------------------------------------------------------------------------------------------ the predictor
class Predictor:
    """model: RTDETRDetectionWorldModel on the GPU; names: {id: name} or a list; text_features: data.TextFeatures (encodes the
    names, first synonym of a 'a/b' entry) or a ready [nc, d] tensor.  Defaults are the reference's (cfg/default.yaml:47-49,68).
    keep_raw=True keeps the last batch's model input (`last_img`) and raw eval output (`last_y`) for inspection.
    augment=True: test-time augmentation (the reference's `augment`, cfg/default.yaml:66; tta.py): the forward runs on tta_views
    (default tta.DEFAULT_VIEWS: the reference's three scales and flips) and ops.tta_merge leaves one prediction tensor of at most
    tta_max_out rows per image, which the postprocess takes as it takes the model's.  `tta_dropped` sums the merged rows that did not
    fit (it rides in the batch's one device-to-host copy), times gains 'tta' (the view launches and the merge, taken out of
    'forward'), and keep_raw then keeps the merged tensor as `last_y` and the per-view inputs / raw outputs as `last_views` /
    `last_ys`.  track() and track_streams() refuse it: a merged row is no single decoder query.
    slice=int | (h, w): sliced prediction for large frames (slicing.py): the loader hands over the original frame only, the frames are
    uploaded as they are, overlapping windows of `slice` pixels (slicing.slice_windows with slice_overlap; slice_full adds the whole
    frame as view 0) are cut and resized to imgsz on the device, the model runs on all views in chunks of `batch`, and ops.slice_merge
    (slice_match 'iou' or 'ios', the predictor's conf / iou / classes / single_cls) leaves one prediction tensor of at most
    slice_max_out rows per frame, which the postprocess takes as it takes the model's.  `slice_dropped` sums the merged rows that did
    not fit; candidates beyond the merge's table raise slicing.SliceOverflow; times gains 'slice' (the view launches and the merge,
    taken out of 'forward'); keep_raw keeps the merged tensor as `last_y` and all views / their raw outputs as `last_views` /
    `last_ys`.  track() and track_streams() refuse it for augment's reason, and slice together with augment is refused."""

    def __init__(self, model, names, text_features, imgsz=640, conf=0.25, iou=0.7, classes=None, single_cls=False, batch=4, dtype='bf16',
                 keep_raw=False, workers=None, augment=False, tta_views=None, tta_max_out=512, slice=None, slice_overlap=0.2, slice_full=True,
                 slice_match='iou', slice_max_out=512):
        if dtype not in ('bf16', 'fp32'):
            raise ValueError(f"dtype must be 'bf16' or 'fp32', got {dtype!r}")
        self.names = names if isinstance(names, dict) else dict(enumerate(names))
        self.imgsz, self.conf, self.iou, self.single_cls, self.batch = int(imgsz), float(conf), float(iou), bool(single_cls), int(batch)
        self.classes = None if classes is None else [int(c) for c in ([classes] if isinstance(classes, int) else classes)]
        self.autocast_dtype = torch.bfloat16 if dtype == 'bf16' else None
        self.keep_raw = keep_raw
        self.workers = workers or allowed_cpus()
        self.device = next(model.parameters()).device
        if self.device.type != 'cuda':
            raise ops._lib.TamtrHipError('Predictor needs the model on an MI355X; there is no CPU path')
        if isinstance(text_features, D.TextFeatures):
            tf = text_features.encode([str(v).split('/')[0] for v in self.names.values()])
        else:
            tf = torch.as_tensor(text_features, dtype=torch.float32)
        model.eval()
        model.fuse()   # what AutoBackend(fuse=True) does; a no-op once fused
        model.set_text_features(tf.reshape(1, len(self.names), -1).to(self.device))
        model.autocast_dtype = self.autocast_dtype
        self.model = model
        self.times = {'load': 0.0, 'h2d': 0.0, 'forward': 0.0, 'postprocess': 0.0, 'track': 0.0, 'd2h': 0.0}   # ms, summed over batches
        self.seen = 0
        self.tracker = None
        self.last_img = self.last_y = None
        self.augment, self.tta_max_out, self.tta_dropped = bool(augment), int(tta_max_out), 0
        self.last_views = self.last_ys = None
        if self.augment:
            from . import tta
            self.tta_views = tta.check_views(tta.DEFAULT_VIEWS if tta_views is None else tta_views)
            self.times['tta'] = 0.0
        self.slice, self.slice_dropped = None, 0
        if slice is not None:
            from . import slicing
            if self.augment:
                raise ValueError('slice and augment cannot be combined: each replaces the forward by views and a merge of its own')
            if slice_match not in ops.SLICE_MATCH:
                raise ValueError(f"slice_match must be 'iou' or 'ios', got {slice_match!r}")
            self.slice = slicing.check_slice(slice)
            self.slice_overlap, self.slice_full, self.slice_match, self.slice_max_out = float(slice_overlap), bool(slice_full), slice_match, int(slice_max_out)
            slicing.slice_windows(self.slice[0], self.slice[1], self.slice, self.slice_overlap, self.slice_full)      # checks the overlap now
            self.times['slice'] = 0.0

    @torch.no_grad()
    def run_batch(self, ims, tracker=None, gt_frames=None, evaluator=None, active=None):
        """Network inputs u8 [B, S, S, 3] (host) + original (h, w) per image -> host (out [B, nq, 6], keep [B, nq], counts [B]).
        With slice set, the first entry is instead the list of the B original frames u8 [h, w, 3] (host), and nq is slice_max_out.
        With a tracker (track.ByteTracker or track.BotSort) the batch's frames also go through one tracker launch, and its rows ride in the same copy:
        -> host (out, keep, counts, tracks [B, nq, 8], tcounts [B]).  With gt_frames (B host arrays [m, 7]) and an evaluator
        (track.MotEvaluator, track.HotaEvaluator or track.TrackMapEvaluator, or a list of them) as well, one more launch per evaluator
        scores the tracker's rows where they lie; each evaluator's header rides in the same copy and its time goes under its own key
        of times ('mot', 'hota', 'tmap').
        active (track_streams; B host booleans): the images that are padding have their counts set to 0 on the device before the
        estimator and the tracker see them - such an image reaches neither.  There the evaluators are stacked ones (streams=S) and a
        gt_frames[i] of None keeps image i out of the score."""
        arr, hw = ims
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
        ev[0].record()
        gmc = getattr(tracker, 'gmc_method', None) == 'sparseOptFlow'      # a track.BotSort that estimates its warps from the frames
        reid = bool(getattr(tracker, 'with_reid', False))                  # a track.BotSort that takes the decoder's query embeddings
        ev_tta = []
        if self.slice:      # the original frames go up as they are; views, forwards in chunks of `batch`, one merge launch
            from . import slicing
            origs = [_pinned_copy(o).to(self.device, non_blocking=True) for o in arr]
            ev[1].record()
            wins = [slicing.slice_windows(h0, w0, self.slice, self.slice_overlap, self.slice_full) for h0, w0 in hw]
            y, _, _, dropped, overflow, views, ys = slicing.sliced_forward(self.model, origs, wins, self.imgsz, self.batch, None, self.conf, self.iou,
                                                                           self.classes, self.single_cls, self.slice_match, self.slice_max_out,
                                                                           self.autocast_dtype, keep=True, events=ev_tta)
            img = u8 = None      # there is no one network input; a tracker, which would read u8, is refused
        else:
            img, u8 = to_model_input(arr, self.device, keep_u8=True)
            ev[1].record()
            if self.augment:      # views, one forward per canvas size, one merge launch: y is the merged tensor
                from . import tta
                y, _, _, dropped, views, ys = tta.tta_forward(self.model, img, None, self.tta_views, self.conf, self.iou, self.classes,
                                                              self.single_cls, self.tta_max_out, self.autocast_dtype, keep=True, events=ev_tta)
            else:
                with torch.autocast('cuda', dtype=self.autocast_dtype or torch.bfloat16, enabled=self.autocast_dtype is not None):
                    preds = self.model(img)
                y = preds[0] if isinstance(preds, (list, tuple)) else preds
        ev[2].record()
        out, keep, counts = ops.detect_postprocess(y, hw, self.conf, self.iou, self.classes, self.single_cls)
        ev[3].record()
        if active is not None:      # the counts mask
            counts = counts * torch.as_tensor(active, dtype=torch.int32).to(self.device, non_blocking=True)
        # one device-to-host copy for all the outputs
        parts = {'out': out, 'keep': keep, 'counts': counts}
        if self.augment:
            parts['dropped'] = dropped
        if self.slice:
            parts.update(dropped=dropped, overflow=overflow)
        evaluators = _as_list(evaluator) if tracker is not None and gt_frames is not None else []
        ev_eval = []
        ev_gmc = None
        if tracker is not None:
            if gmc:      # the warps stay on the device; the tracker launch reads them there
                H, W = float(arr.shape[1]), float(arr.shape[2])
                warps = tracker.estimate_warps(u8, counts, [[w0 / W, h0 / H] for h0, w0 in np.asarray(hw).reshape(-1, 2).tolist()])
                ev_gmc = torch.cuda.Event(enable_timing=True)
                ev_gmc.record()
                tracks, tcounts = tracker.update(out, counts, warps=warps, **self._reid_operands(reid, keep))
            else:
                tracks, tcounts = tracker.update(out, counts, **self._reid_operands(reid, keep))
            parts.update(tracks=tracks, tcounts=tcounts, hdr=tracker.state['hdr'])      # hdr: 8 words, per stream of a stacked tracker
            for i, e in enumerate(evaluators):
                ev_eval.append(torch.cuda.Event(enable_timing=True))
                ev_eval[-1].record()
                e.update(tracks, tcounts, gt_frames)
                parts['ehdr', i] = e.state['hdr']
        ev[4].record()
        host = {k: torch.from_numpy(a) for k, a in ops._lib.to_host(parts, pinned=True, record=ev[5]).items()}
        ev[5].synchronize()
        spans = [('h2d', ev[0], ev[1]), ('forward', ev[1], ev[2]), ('postprocess', ev[2], ev[3]), ('track', ev_gmc or ev[3], (ev_eval + [ev[4]])[0]),
                 ('d2h', ev[4], ev[5])] + ([('gmc', ev[3], ev_gmc)] if ev_gmc is not None else [])
        for i, e in enumerate(evaluators):
            spans.append((e.times_key, ev_eval[i], (ev_eval + [ev[4]])[i + 1]))
        if self.augment:
            spans[1] = ('forward', ev_tta[1], ev_tta[2])
            spans += [('tta', ev[1], ev_tta[1]), ('tta', ev_tta[2], ev[2])]
            self.tta_dropped += int(host['dropped'].sum())
        if self.slice:
            spans[1] = ('forward', ev_tta[1], ev_tta[2])
            spans += [('slice', ev[1], ev_tta[1]), ('slice', ev_tta[2], ev[2])]
            self.slice_dropped += int(host['dropped'].sum())
        for k, a, b in spans:
            self.times[k] = self.times.get(k, 0.0) + a.elapsed_time(b)
        if self.keep_raw:
            self.last_img, self.last_y = img, y
            if self.augment or self.slice:
                self.last_views, self.last_ys = views, ys
        if self.slice:
            from .slicing import check_overflow
            check_overflow(host['overflow'], self.conf)
        res = host['out'], host['keep'], host['counts']
        if tracker is None:
            return res
        tracker.check_overflow(host['hdr'].view(-1, 8)[:, 3])
        for i, e in enumerate(evaluators):
            e.check_overflow(host['ehdr', i].view(-1))
        return res + (host['tracks'], host['tcounts'])

    def _reid_operands(self, reid, keep):
        """For a BotSort with ReID: the decoder's per-query hidden state of this forward (head.keep_query_embed) and the source query
        of every kept row, both where they lie on the device; the gather (ops.reid_rows) runs inside tracker.update, under 'track'."""
        if not reid:
            return {}
        embed = self.model.model[-1].last_query_embed
        if embed is None:
            raise RuntimeError('the tracker has with_reid on and the decoder kept no query embedding: set head.keep_query_embed (track() does)')
        return {'embed': embed, 'keep': keep}

    def predict(self, source):
        """Yields one Detections per image, in the sorted order of list_sources(source)."""
        for _, det in self._run(sequence_records(list_sources(source), self.batch)):
            yield det

    def track(self, source, tracker=None, persist=False, gt=None, evaluator=None):
        """The sorted files of `source` as ONE sequence (the reference's model.track): the batches of predict, then one tracker launch
        per batch.  Yields one Detections per frame whose boxes are the track rows (x1 y1 x2 y2 from the filter, score, cls) and
        whose `id` holds the track ids; a frame for which the tracker returned nothing keeps its plain detections and id None
        (trackers/track.py:46-50).  tracker: a track.ByteTracker or track.BotSort, a bytetrack.yaml or botsort.yaml path
        (track.tracker_from_yaml), or None for ByteTrack's defaults; persist=True keeps the tracker (and its tracks) of the previous
        call.  A BotSort estimates its camera-motion warps from the uploaded frames of each batch (unless its gmc_method is none), and
        speed() then has a 'gmc' entry for those launches.  A BotSort with ReID (with_reid=True, or a yaml with `with_reid: True`,
        which is built with reid_dim = the decoder's hidden size) takes the decoder's per-query hidden state as the embedding of a
        detection: the decoder keeps it for the run (head.keep_query_embed, switched back afterwards), the tracker gathers the kept
        rows on the device; nothing more is copied to the host.
        gt + evaluator: the sequence's ground truth, one array [m, 7] (x1 y1 x2 y2 id cls kind, track.read_mot) per frame in file order
        (missing frames are empty), and a track.MotEvaluator, track.HotaEvaluator or track.TrackMapEvaluator, or a list / tuple of them:
        every batch's rows are scored on the device right after the tracker's launch, by each evaluator in turn (a frame without track
        rows is an empty track set, as write_mot has it), the sequence is ended after the last frame, and speed() has an entry per
        evaluator ('mot', 'hota', 'tmap'); each evaluator's results() then holds the metrics.  Without both, nothing changes."""
        self._refuse_augment('track')      # when track() is called, not at the first frame
        return self._track_source(source, tracker, persist, gt, evaluator)

    def _track_source(self, source, tracker, persist, gt, evaluator):
        self._install_tracker(tracker, persist)
        files = list_sources(source)
        if getattr(self.tracker, 'with_reid', False):
            yield from self._with_query_embed(self._track(files, gt, evaluator))
        else:
            yield from self._track(files, gt, evaluator)

    def track_streams(self, sources, tracker=None, frames_per_stream=1, persist=False, gt=None, evaluator=None):
        """S sequences at once, one tracker per sequence (the reference's model.track on a batch of streams, trackers/track.py:33-53):
        `sources` is a list of S sources - each a directory, a list file or a list of paths, each a sequence of its own.  Every
        batch holds `frames_per_stream` frames of every stream, frame-major (stream_batches), and gets one forward, one
        detect_postprocess, the counts mask, at most four estimator launches, one tracker launch (one workgroup per stream) and one
        device-to-host copy.  Yields (stream_index, Detections) as track() yields Detections, in frame order within a stream, until
        the longest stream ends; a stream that has ended keeps its place in the batch as padding, which reaches neither the tracker
        nor the estimator and is never yielded.  tracker: a yaml path, None for ByteTrack's defaults, or a track.ByteTracker /
        track.BotSort built with streams=len(sources) (any other `streams` raises ValueError); persist as in track().  BoT-SORT's
        camera-motion estimate and ReID work as in track(), per stream.
        gt + evaluator: `gt` is a list of S entries, each the sequence's per-frame arrays as track() takes them or None for "do not
        score this stream"; `evaluator` is a track.MotEvaluator and / or track.HotaEvaluator built with streams=S, or a list of them
        (anything else raises ValueError: another S, an evaluator without streams, a TrackMapEvaluator, which holds one sequence).
        Every batch's rows are then scored on the device right after the tracker's launch, one launch per evaluator with one
        workgroup per stream; the evaluators' headers ride in the batch's one device-to-host copy and speed() has an entry per
        evaluator ('mot', 'hota').  A stream is ended right after the batch that holds its last frame, all streams ending there in
        one call; stream_counts(s) and results() then hold the metrics.  Without both, nothing changes.
        The arguments are checked when this is called, before the first frame is asked for."""
        self._refuse_augment('track_streams')
        sources = list(sources) if isinstance(sources, (list, tuple)) else None
        if not sources:
            raise ValueError('track_streams needs a non-empty list of sources, one per stream')
        S = len(sources)
        evaluators = _as_list(evaluator)
        for e in evaluators:
            if getattr(e, 'times_key', None) not in ('mot', 'hota') or getattr(e, 'streams', None) != S:
                raise ValueError(f'track_streams scores {S} sources with a MotEvaluator / HotaEvaluator built with streams={S}, got '
                                 f'{type(e).__name__} with streams={getattr(e, "streams", None)!r} (a TrackMapEvaluator holds one sequence)')
        if gt is not None:
            gt = list(gt) if isinstance(gt, (list, tuple)) else None
            if gt is None or len(gt) != S:
                raise ValueError(f'gt must be a list of {S} entries, one per source (per-frame arrays, or None for a stream that is not scored)')
        self._install_tracker(tracker, persist, streams=S)
        evaluators = evaluators if gt is not None else []
        records = stream_records([list_sources(src) for src in sources], frames_per_stream, gt if evaluators else None)
        self._prune_times(evaluators)
        frames = self._run(records, self.tracker, evaluators, S)
        return self._with_query_embed(frames) if getattr(self.tracker, 'with_reid', False) else frames

    def _refuse_augment(self, what):
        if getattr(self, 'slice', None):
            raise ValueError(f'{what}() does not take a predictor with slice set: a merged row is no single decoder query of one forward, so the '
                             'tracker\'s row-to-query identity (ReID) would not hold; build a Predictor without slice for tracking')
        if getattr(self, 'augment', False):      # (an object that never ran __init__ has no augment: the argument checks still work on it)
            raise ValueError(f'{what}() does not take a predictor with augment=True: a merged row is no single decoder query, so the tracker\'s '
                             'row-to-query identity (ReID) would not hold; build a Predictor without augment for tracking')

    def _install_tracker(self, tracker, persist, streams=None):
        """self.tracker for a run of track() (streams=None) or track_streams() (streams=S): the given instance, reset unless persist;
        else the previous call's with persist, when it has these streams; else a new one from the yaml path or ByteTrack's defaults."""
        from .track import ByteTracker, tracker_from_yaml
        if isinstance(tracker, ByteTracker):
            if streams is not None and tracker.streams != streams:
                raise ValueError(f'the tracker was built with streams={tracker.streams!r}, {streams} sources need streams={streams}')
            self.tracker = tracker
            if not persist:
                tracker.reset()
        elif not persist or (self.tracker is None if streams is None else getattr(self.tracker, 'streams', None) != streams):
            kw = {} if streams is None else {'streams': streams}
            head = self.model.model[-1]
            self.tracker = tracker_from_yaml(tracker, self.device, reid_dim=head.hidden_dim, **kw) if tracker else ByteTracker(self.device, **kw)

    def _prune_times(self, evaluators):
        """An evaluator's key of times exists only while a run is scored by it, the estimator's only while a BotSort run is in progress."""
        for k in {'mot', 'hota', 'tmap'} - {e.times_key for e in evaluators}:
            self.times.pop(k, None)
        if getattr(self.tracker, 'gmc_method', None) != 'sparseOptFlow':
            self.times.pop('gmc', None)

    def _with_query_embed(self, frames):
        head = self.model.model[-1]
        if self.tracker.reid_dim != head.hidden_dim:
            raise ValueError(f'the tracker was built with reid_dim {self.tracker.reid_dim}, the decoder\'s query embedding has {head.hidden_dim}')
        was, head.keep_query_embed = head.keep_query_embed, True
        try:
            yield from frames
        finally:
            head.keep_query_embed = was

    def _track(self, files, gt, evaluator):
        evaluators = _as_list(evaluator) if gt is not None else []
        self._prune_times(evaluators)
        for _, det in self._run(sequence_records(files, self.batch, gt if evaluators else None), self.tracker, evaluators):
            yield det
        for e in evaluators:
            e.end_sequence()

    def _run(self, records, tracker=None, evaluators=(), S=1):
        """The batch loop of predict, track and track_streams over sequence_records / stream_records: yields (stream index, Detections)
        for every image that is not padding.  The next batch decodes while this one runs on the GPU."""
        load = load_original if self.slice else load_image      # sliced prediction: the host makes no stretched network input
        with ThreadPoolExecutor(max_workers=self.workers) as pool:
            def submit(k):      # a padding entry shares its path's load
                paths = records[k][0] if k < len(records) else []
                jobs = {f: pool.submit(load, f, self.imgsz) for f in dict.fromkeys(paths)}
                return [jobs[f] for f in paths]
            pending = submit(0)
            for k, (paths, active, gt_frames, ending) in enumerate(records):
                t0 = time.perf_counter()
                loaded = [f.result() for f in pending]
                self.times['load'] += (time.perf_counter() - t0) * 1e3
                pending = submit(k + 1)
                origs = [o for o, _ in loaded]
                hw = [o.shape[:2] for o in origs]
                ims = (origs if self.slice else np.stack([r for _, r in loaded]), hw)
                more = {} if active is None else {'active': active}
                res = self.run_batch(ims, tracker, **more) if gt_frames is None else self.run_batch(ims, tracker, gt_frames, evaluators, **more)
                for e in evaluators if ending else []:
                    e.end_sequence(ending)
                out, counts = res[0], res[2]
                live = [True] * len(paths) if active is None else active
                self.seen += sum(live)
                for i, path in enumerate(paths):
                    if not live[i]:
                        continue
                    n, nt = int(counts[i]), int(res[4][i]) if tracker is not None else 0
                    if nt:
                        rows = res[3][i, :nt]
                        yield i % S, Detections(path, hw[i], self.names, rows[:, [0, 1, 2, 3, 5, 6]].clone(), orig_img=origs[i], id=rows[:, 4].long())
                    else:
                        yield i % S, Detections(path, hw[i], self.names, out[i, :n].clone(), orig_img=origs[i])

    def __call__(self, source):
        return list(self.predict(source))

    def speed(self):
        """ms per image of each phase so far (load = waiting for decoded + resized images; the rest from device events)."""
        return {k: v / max(self.seen, 1) for k, v in self.times.items()}
