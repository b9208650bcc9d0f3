"""ByteTrack multi-object tracking on the device (the reference's ultralytics/trackers: track.py, byte_tracker.py, basetrack.py,
utils/kalman_filter.py, utils/matching.py, cfg/trackers/bytetrack.yaml): one HIP launch per predictor batch, state in device buffers.

    from tamtr_amd.track import ByteTracker
    tracker = ByteTracker(device)                       # or ByteTracker.from_yaml('bytetrack.yaml', device)
    tracks, tcounts = tracker.update(out, counts)       # the outputs of ops.detect_postprocess, frames in order; no synchronisation

`Predictor.track(source)` (predict.py) drives it and yields Detections with ids; tools/track.py is the command line.

BotSort is the reference's other tracker (trackers/bot_sort.py, cfg/trackers/botsort.yaml) on the same table and launch: the XYWH
filter and one camera-motion warp per frame applied to the track states.  The warps are estimated on the device from the frames of
the batch (csrc/gmc.hip states that rule, which is the project's own), or come from the caller:

    tracker = BotSort(device)                           # or tracker_from_yaml('botsort.yaml', device)
    tracks, tcounts = tracker.update(out, counts, frames=u8, scale=s)   # u8 [B, H, W, 3] on the device, s [B, 2] = (w0 / W, h0 / H)
    tracks, tcounts = tracker.update(out, counts, warps=w)      # w f64 [B, 2, 3] in original pixels, device or host
    tracks, tcounts = tracker.update(out, counts)               # identity warps (the reference without an image)

BotSort(device, with_reid=True, reid_dim=D) adds the appearance half of BoT-SORT (the reference writes the rule out and ships no
encoder for it): every detection comes with a D-vector, either gathered from a per-query embedding by detect_postprocess's `keep`
(the decoder's hidden state is such an embedding: head.keep_query_embed) or handed in ready:

    tracks, tcounts = tracker.update(out, counts, frames=u8, scale=s, embed=e, keep=keep)   # e f32 | bf16 [B, nqm, D]
    tracks, tcounts = tracker.update(out, counts, feats=f)                                   # f f32 [B, nq, D], rows aligned with out

Several streams at once (the reference keeps one tracker per image of the batch, trackers/track.py:33-53): streams=S stacks S
trackers' tables and still takes one launch per batch, one workgroup per stream.  A batch then holds F frames of every stream,
frame-major (image f * S + s is the f-th frame of stream s); a stream without a frame at some position keeps its image with
counts 0.  `Predictor.track_streams(sources)` drives it.

    tracker = ByteTracker(device, streams=4)            # BotSort(device, streams=4), tracker_from_yaml(path, device, streams=4)
    tracks, tcounts = tracker.update(out, counts)       # out [F * 4, nq, 6]
    tracker.reset(stream=2)                             # stream 2 starts over; the others are untouched

MOT evaluation next to it (CLEAR-MOT and identity metrics; the rule is written out in csrc/mot.hip, engine.mot_evaluate states it in
numpy): one more launch per batch on the rows the tracker left on the device, one launch per sequence for the reduction.

    ev = MotEvaluator(device, nc)
    ev.update(tracks, tcounts, gt_frames)               # gt_frames: B host arrays [m, 7] (read_mot); no synchronisation
    ev.end_sequence()
    ev.results(names)                                   # synchronises: {'all': row, 'per_class': [...]}, MOTA / MOTP / IDF1 ...

HotaEvaluator has the same methods and scores the same rows by HOTA (the rule is written out in csrc/hota.hip, engine.hota_evaluate
states it in numpy): one launch per batch, three per sequence.  `Predictor.track(..., evaluator=[mot, hota])` feeds both.

Several streams scored at once, next to the stacked trackers: streams=S keeps one evaluator state per stream in stacked tensors, and
the update is still one launch per batch, one workgroup per stream, on the tracker's frame-major rows.

    ev = MotEvaluator(device, nc, streams=4)            # HotaEvaluator(device, nc, streams=4)
    ev.update(tracks, tcounts, gt_frames)               # gt_frames[f * 4 + s]: frame f of stream s, or None for "not a frame"
    ev.end_sequence([1, 3])                             # streams 1 and 3 end, in one launch set; None ends every open stream
    ev.stream_counts(1), ev.counts(), ev.results()      # one stream's totals; the run's totals over all streams

`Predictor.track_streams(sources, gt=[...], evaluator=[mot, hota])` drives them; tools/mot_eval.py --streams S scores result files so.
"""
import numpy as np
import torch

from . import ops

# state values of a slot (meta[:, 0]) and the columns of meta and hdr; csrc/track.hip states the table
FREE, TRACKED, LOST, REMOVED = 0, 1, 2, 3
META_COLS = ('state', 'is_activated', 'track_id', 'frame_id', 'start_frame', 'tracklet_len', 'idx', 'flags')
HDR_FRAME, HDR_NEXT_ID, HDR_LIVE, HDR_OVERFLOW = 0, 1, 2, 3
YAML_KEYS = ('track_high_thresh', 'track_low_thresh', 'new_track_thresh', 'track_buffer', 'match_thresh')


class TrackerOverflow(RuntimeError):
    pass


class MotOverflow(RuntimeError):
    pass


class HotaOverflow(RuntimeError):
    pass


class TrackMapOverflow(RuntimeError):
    pass


def read_tracker_yaml(path):
    """The keys of the reference's cfg/trackers/bytetrack.yaml -> ByteTracker's constructor arguments; any other tracker_type raises.
    tracker_from_yaml reads either of the reference's tracker files and builds ByteTracker or BotSort."""
    import yaml
    with open(path) as f:
        cfg = yaml.safe_load(f) or {}
    kind = cfg.get('tracker_type', 'bytetrack')
    if kind != 'bytetrack':
        raise ValueError(f"tracker_type {kind!r} is not supported: only 'bytetrack' is built (BoT-SORT needs optical flow on the host)")
    return {k: cfg[k] for k in YAML_KEYS if k in cfg}


def check_streams(streams):
    """streams=None (one tracker) or a positive int -> itself; anything else raises ValueError.  Touches no device."""
    if streams is not None and (isinstance(streams, bool) or not isinstance(streams, int) or streams < 1):
        raise ValueError(f'streams must be None (one tracker) or a positive int (one tracker per stream), got {streams!r}')
    return streams


class _Stacked:
    """What a tracker and an evaluator built with streams=S share: `state`, a dict of device tensors that each gain a leading S."""
    _noun = streams = None

    @property
    def _lead(self):
        """The leading dimension of every state tensor: none without streams, (S,) for a stack."""
        return () if self.streams is None else (self.streams,)

    def _stream(self, stream):
        if self.streams is None or isinstance(stream, bool) or not isinstance(stream, (int, np.integer)) or not 0 <= stream < self.streams:
            raise ValueError(f'stream must be in 0 .. {self.streams - 1}, got {stream!r}' if self.streams else
                             f'stream={stream!r} was given to {self._noun} built without streams')
        return int(stream)

    def stream_state(self, s):
        """Stream s's state as views state[k][s]: contiguous, so the ops without streams take them as they are."""
        s = self._stream(s)
        return {k: v[s] for k, v in self.state.items()}


class ByteTracker(_Stacked):
    """One tracker = one slot table of `capacity` tracks on `device` (ids start at 1).  nq is the number of rows per frame the
    workspace is sized for; a batch with more rows gets a larger workspace on its first use.
    streams=S: S trackers, one per stream, in one stacked table (every state tensor gains a leading S) and one launch; update()
    then takes the frame-major batch (image f * S + s is the f-th frame of stream s) and every stream's ids start at 1."""
    _noun = 'a tracker'

    def __init__(self, device, track_high_thresh=0.5, track_low_thresh=0.1, new_track_thresh=0.6, track_buffer=30, match_thresh=0.8,
                 frame_rate=30, capacity=1024, nq=300, streams=None):
        self.streams = check_streams(streams)
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise ops._lib.TamtrHipError('ByteTracker needs an MI355X; there is no CPU path')
        self.track_high_thresh, self.track_low_thresh = float(track_high_thresh), float(track_low_thresh)
        self.new_track_thresh, self.match_thresh = float(new_track_thresh), float(match_thresh)
        self.track_buffer, self.frame_rate = int(track_buffer), frame_rate
        self.max_time_lost = int(frame_rate / 30.0 * track_buffer)      # byte_tracker.py:234
        self.capacity, self.nq = int(capacity), int(nq)
        if self.capacity < 1 or self.nq < 1:
            raise ValueError(f'capacity and nq must be positive, got {capacity} and {nq}')
        self.workspace = torch.empty(self._ws_bytes(), device=self.device, dtype=torch.uint8)
        self.state = {k: torch.zeros(self._lead + (self.capacity,) + tail, device=self.device, dtype=dt) for k, dt, tail in ops.TRACK_STATE_SPEC}
        self.state['hdr'] = torch.zeros(self._lead + (8,), device=self.device, dtype=torch.int32)
        self._fresh_hdr = torch.tensor([0, 1, 0, 0, 0, 0, 0, 0], dtype=torch.int32).to(self.device)
        self.reset()

    @classmethod
    def from_yaml(cls, path, device, **kw):
        return cls(device, **{**read_tracker_yaml(path), **kw})

    def reset(self, stream=None):
        """Forget every track; the next id is 1 again.  stream=s: of that stream's tracker alone.  No synchronisation."""
        if stream is None:
            self.state['meta'].zero_()
            self.state['hdr'].copy_(self._fresh_hdr)
        else:
            s = self._stream(stream)
            self.state['meta'][s].zero_()
            self.state['hdr'][s].copy_(self._fresh_hdr)

    def _ws_bytes(self):
        return ops.bytetrack_workspace_bytes(self.capacity, self.nq, *self._lead)

    def _grow(self, out):
        """A batch with more rows per frame than the workspace was sized for gets a larger workspace."""
        if out.dim() == 3 and out.shape[1] > self.nq:
            self.nq = out.shape[1]
            self.workspace = torch.empty(self._ws_bytes(), device=self.device, dtype=torch.uint8)

    def update(self, out, counts):
        """out f32 [B, nq, 6], counts i32 [B] on the device (ops.detect_postprocess) -> tracks f32 [B, nq, 8] (x1 y1 x2 y2 id score
        cls idx, zero after the count), tcounts i32 [B], on the device.  The B frames are consumed in order in one launch; with
        streams=S they are F frames of each stream, frame-major, and every stream's are consumed in order by its own tracker."""
        self._grow(out)
        return ops.bytetrack_update(out, counts, self.state, self.capacity, self.track_high_thresh, self.track_low_thresh,
                                    self.new_track_thresh, self.match_thresh, self.max_time_lost, self.workspace, streams=self.streams)

    def check_overflow(self, overflow):
        """Raise when the header's overflow count (read by the caller, e.g. from the predictor's packed copy) is not zero.  With
        streams=S it is the column hdr[:, 3], and the message names the streams that overflowed."""
        if self.streams is not None:
            over = np.asarray(overflow).reshape(-1).astype(np.int64)
            if over.any():
                which = ', '.join(f'stream {i}: {n}' for i, n in enumerate(over.tolist()) if n)
                raise TrackerOverflow(f'new tracks found no free slot ({which}): each stream\'s table holds {self.capacity} tracks; '
                                      'build the tracker with a larger capacity')
            return
        if int(overflow):
            raise TrackerOverflow(f'{int(overflow)} new tracks found no free slot: the table holds {self.capacity} tracks; '
                                  'build the tracker with a larger capacity')

    def state_dict(self):
        """The whole table as host numpy arrays (synchronises): mean, cov, meta, sc, hdr."""
        return {k: v.cpu().numpy().copy() for k, v in self.state.items()}

    def load_state_dict(self, sd):
        """Place the tracker in the state of a state_dict() (same capacity): a resumable stream, and `persist` across calls."""
        for k, v in self.state.items():
            a = np.asarray(sd[k])
            if a.shape != tuple(v.shape):
                raise ValueError(f'state {k!r} has shape {a.shape}, this tracker (capacity {self.capacity}) needs {tuple(v.shape)}')
            v.copy_(torch.from_numpy(np.ascontiguousarray(a)).to(v.dtype))
        self.check_overflow(np.asarray(sd['hdr'])[..., HDR_OVERFLOW])


BOTSORT_YAML_KEYS = YAML_KEYS + ('gmc_method', 'proximity_thresh', 'appearance_thresh', 'with_reid')
GMC_BUILT = ('sparseOptFlow', 'none')      # what `gmc_method` may name; the reference's orb, sift and ecc (utils/gmc.py) are not built


class BotSort(ByteTracker):
    """BoT-SORT on the device (the reference's trackers/bot_sort.py, cfg/trackers/botsort.yaml): ByteTracker's table, launch and
    methods with the XYWH Kalman filter, `vw = vh = 0` before a lost track is predicted, and each frame's 2x3 camera-motion warp
    applied to the track states between the prediction and the first association (csrc/track.hip states the rule; it is pinned to
    the reference's BOTSORT by tests/golden/botsort.npz).

    gmc_method 'sparseOptFlow' (the default, as in botsort.yaml) estimates the warps on the device from the frames handed to
    update(): grid keypoints, pyramidal Lucas-Kanade and a similarity fit, at most four launches (csrc/gmc.hip writes the rule out;
    it is the project's own, not OpenCV's, whose role it takes).  The estimator keeps the previous tracked frame on the device
    across batches; reset() forgets it.  'none' (or None) never estimates: every warp is the identity unless update() is given
    warps.  'orb', 'sift' and 'ecc' raise ValueError.
    proximity_thresh and appearance_thresh gate ReID embeddings, which the reference itself does not build ("Haven't supported
    BoT-SORT(reid) yet"): with with_reid off its get_dists is ByteTrack's fused IoU distance, the constructor keeps the two
    thresholds and the launch does not read them.
    with_reid=True needs reid_dim=D, the length of the embedding update() will be given per detection (embed + keep, or feats):
    the table gains state['feat'] f32 [capacity, D], the tracks' smoothed features, and update() launches the ReID instantiation
    of the kernel (ops.botsort_reid_update; csrc/track.hip states the rule, tests/golden/botsort_reid.npz pins it to the
    reference's BOTSORT run with a stub encoder).  Which embedding separates identities, and how well, is the caller's matter:
    nothing here has been measured with trained weights.  A feature row of zero norm is outside the contract."""

    def __init__(self, device, gmc_method='sparseOptFlow', proximity_thresh=0.5, appearance_thresh=0.25, with_reid=False, reid_dim=None,
                 streams=None, **kw):
        method = 'none' if gmc_method is None else str(gmc_method)
        if method not in GMC_BUILT:
            raise ValueError(f"gmc_method {gmc_method!r} is not built: 'sparseOptFlow' (estimated on the device) and 'none' are; the "
                             "reference's orb, sift and ecc run OpenCV on the host")
        if with_reid and reid_dim is None:
            raise ValueError('with_reid=True needs reid_dim=D, the length of the embedding each detection comes with (the reference '
                             'has no ReID encoder for BoT-SORT; update() takes embed + keep, or feats)')
        if reid_dim is not None and not with_reid:
            raise ValueError(f'reid_dim={reid_dim!r} has no meaning with with_reid off')
        if with_reid and not 1 <= int(reid_dim) <= ops.REID_MAX_D:
            raise ValueError(f'reid_dim must be in 1 .. {ops.REID_MAX_D} with with_reid on, got {reid_dim!r}')
        self.gmc_method, self.with_reid = method, bool(with_reid)
        self.reid_dim = int(reid_dim) if with_reid else None
        self.proximity_thresh, self.appearance_thresh = float(proximity_thresh), float(appearance_thresh)
        self.last_warps = self.last_stats = None
        self.gmc, self.gmc_hw, self.gmc_workspace = None, None, None      # the estimator's state, made for the first frames' size
        super().__init__(device, **kw, **({} if streams is None else {'streams': streams}))
        if self.with_reid:
            self.state['feat'] = torch.zeros(self._lead + (self.capacity, self.reid_dim), device=self.device, dtype=torch.float32)

    def _ws_bytes(self):
        return (ops.botsort_reid_workspace_bytes if self.with_reid else ops.bytetrack_workspace_bytes)(self.capacity, self.nq, *self._lead)

    def reset(self, stream=None):
        """Forget every track and the estimator's previous frame (stream=s: that stream's alone).  state['feat'] is left as it is: a
        slot's row is read only while the slot holds a track, and a new track overwrites it.  No synchronisation."""
        super().reset(stream)
        if self.gmc is not None:
            (self.gmc['hdr'] if stream is None else self.gmc['hdr'][stream]).zero_()

    def estimate_warps(self, frames, counts, scale=None):
        """frames u8 [B, H, W, 3] on the device (the network input as uploaded), counts i32 [B], scale [B, 2] = (w0 / W, h0 / H) or
        None for ones -> warps f64 [B, 2, 3] on the device (ops.gmc_estimate); last_stats keeps i32 [B, 4] (keypoints, tracked,
        inliers, used).  Frames of another size than the last start a new sequence for the estimator (with streams=S: for every
        stream's, and pairing runs per stream over the frame-major batch)."""
        B, H, W = int(frames.shape[0]), int(frames.shape[1]), int(frames.shape[2])
        if self.gmc_hw != (H, W):
            self.gmc, self.gmc_hw = ops.gmc_state(H, W, self.device, self.streams), (H, W)
        need = ops.gmc_workspace_bytes(B, H, W)
        if self.gmc_workspace is None or self.gmc_workspace.numel() < need:
            self.gmc_workspace = torch.empty(need, device=self.device, dtype=torch.uint8)
        if scale is None:
            scale = np.ones((B, 2))
        warps, self.last_stats = ops.gmc_estimate(frames, counts, scale, self.gmc, self.gmc_workspace, streams=self.streams)
        return warps

    def update(self, out, counts, frames=None, scale=None, warps=None, embed=None, keep=None, feats=None):
        """As ByteTracker.update.  With `frames` (and gmc_method 'sparseOptFlow') the warps are estimated first (estimate_warps) and
        read by the tracker launch where they lie; with `warps` (f64 [B, 2, 3], device tensor, host tensor or array; a host one goes
        up in one copy) nothing is estimated; with neither every warp is the identity, as in the reference when no image is given.
        The warp of a frame without detections is not applied.  last_warps keeps the device tensor.
        With ReID on, either `embed` (f32 | bf16 [B, nqm, D], one vector per query) with `keep` (i32 [B, nq], detect_postprocess's)
        - the rows are gathered and normalised on the device (ops.reid_rows) - or `feats` (f32 [B, nq, D], ready rows aligned with
        `out`, from any other encoder; they go through the same double normalisation).  With ReID off neither may be given."""
        given = embed is not None or keep is not None or feats is not None
        if not self.with_reid and given:
            raise ValueError('embed / keep / feats were given to a tracker built with with_reid off')
        if self.with_reid:
            if feats is not None and (embed is not None or keep is not None):
                raise ValueError('with_reid: give either embed with keep, or feats, not both')
            if feats is None and (embed is None or keep is None):
                raise ValueError('with_reid is on: update() needs embed with keep (gathered by ops.reid_rows), or feats')
            src = feats if feats is not None else embed
            if not torch.is_tensor(src) or src.dim() != 3 or src.shape[-1] != self.reid_dim:
                got = tuple(src.shape) if torch.is_tensor(src) else type(src).__name__
                raise ValueError(f'with_reid: the embedding must be a tensor [B, n, {self.reid_dim}] (reid_dim), got {got}')
        self._grow(out)
        if warps is None and frames is not None and self.gmc_method == 'sparseOptFlow':
            warps = self.estimate_warps(frames, counts, scale)
        elif warps is not None and not (torch.is_tensor(warps) and warps.is_cuda):
            warps = torch.as_tensor(np.asarray(warps, np.float64)).to(self.device, non_blocking=True)
        self.last_warps = warps
        if self.with_reid:
            if feats is not None:      # ready rows: row j of frame b is its own source
                keep = torch.arange(feats.shape[1], device=feats.device, dtype=torch.int32).expand(feats.shape[0], -1)
                embed = feats
            feat = ops.reid_rows(embed, keep, counts)
            return ops.botsort_reid_update(out, counts, feat, self.state, self.capacity, warps, self.track_high_thresh, self.track_low_thresh,
                                           self.new_track_thresh, self.match_thresh, self.max_time_lost, self.proximity_thresh,
                                           self.appearance_thresh, self.workspace, streams=self.streams)
        return ops.botsort_update(out, counts, self.state, self.capacity, warps, self.track_high_thresh, self.track_low_thresh,
                                  self.new_track_thresh, self.match_thresh, self.max_time_lost, self.workspace, streams=self.streams)

    def state_dict(self):
        """ByteTracker's table (with ReID on it includes feat f32 [capacity, D]) plus the estimator's state (gmc_pyr, gmc_kp, gmc_hdr,
        gmc_hw) once it exists (synchronises).  load_state_dict refuses a feat of another D."""
        sd = super().state_dict()
        if self.gmc is not None:
            sd.update({'gmc_' + k: v.cpu().numpy().copy() for k, v in self.gmc.items()})
            sd['gmc_hw'] = np.asarray(self.gmc_hw, np.int64)
        return sd

    def load_state_dict(self, sd):
        if ('feat' in sd) != self.with_reid:
            raise ValueError("the state has a 'feat' table and this tracker was built with with_reid off" if 'feat' in sd else
                             f"the state has no 'feat' table: this tracker was built with with_reid on (reid_dim {self.reid_dim})")
        super().load_state_dict(sd)
        self.gmc, self.gmc_hw = None, None
        if 'gmc_hw' in sd:
            H, W = (int(v) for v in np.asarray(sd['gmc_hw']))
            self.gmc, self.gmc_hw = ops.gmc_state(H, W, self.device, self.streams), (H, W)
            for k, v in self.gmc.items():
                a = np.asarray(sd['gmc_' + k])
                if a.shape != tuple(v.shape):
                    raise ValueError(f'state gmc_{k} has shape {a.shape}, frames of {H} x {W} need {tuple(v.shape)}')
                v.copy_(torch.from_numpy(np.ascontiguousarray(a)).to(v.dtype))


def tracker_from_yaml(path, device, **kw):
    """A tracker yaml with the reference's keys (cfg/trackers/bytetrack.yaml or botsort.yaml) -> ByteTracker or BotSort, by its
    `tracker_type`; keyword arguments override the file (e.g. gmc_method='none', with_reid=True, reid_dim=256) or go to the
    constructor as they are (streams=S: one tracker per stream)."""
    import yaml
    check_streams(kw.get('streams'))
    with open(path) as f:
        cfg = yaml.safe_load(f) or {}
    kind = cfg.get('tracker_type', 'bytetrack')
    if kind == 'bytetrack':      # which has no use for a gmc_method or a reid_dim
        if kw.get('with_reid'):
            raise ValueError("with_reid is BoT-SORT's: the yaml's tracker_type is 'bytetrack'")
        return ByteTracker(device, **{**{k: cfg[k] for k in YAML_KEYS if k in cfg},
                                      **{k: v for k, v in kw.items() if k not in ('gmc_method', 'reid_dim', 'with_reid')}})
    if kind == 'botsort':      # with_reid: True needs reid_dim from the caller; with it off a reid_dim is dropped
        args = {**{k: cfg[k] for k in BOTSORT_YAML_KEYS if k in cfg}, **kw}
        if not args.get('with_reid'):
            args.pop('reid_dim', None)
        return BotSort(device, **args)
    raise ValueError(f"tracker_type {kind!r} is not supported: 'bytetrack' and 'botsort' are built")


def write_mot(path, frames):
    """VisDrone-MOT result file: `frame,id,left,top,width,height,score,category,-1,-1` per track, frames 1-based.  `frames` is one
    Detections per frame of the sequence, in order; frames whose `id` is None (no track) write nothing."""
    lines = []
    for f, det in enumerate(frames, 1):
        if det.id is None:
            continue
        for (x1, y1, x2, y2, score, cls), tid in zip(det.boxes.tolist(), det.id.tolist()):
            lines.append('%d,%d,%.2f,%.2f,%.2f,%.2f,%.4f,%d,-1,-1\n' % (f, tid, x1, y1, x2 - x1, y2 - y1, score, int(cls)))
    with open(path, 'w') as fh:
        fh.writelines(lines)
    return len(lines)


# ------------------------------------------------------------------------------------------------ MOT evaluation
MOT_HDR_FRAME, MOT_HDR_OVER_GT, MOT_HDR_OVER_TRK, MOT_HDR_OVER_ROWS = 0, 1, 2, 3
# VisDrone-MOT annotation categories: 0 ignored region, 1 .. 10 the classes, 11 others
VISDRONE_CATEGORIES = {0: (0, 2), **{c: (c - 1, 0) for c in range(1, 11)}, 11: (0, 1)}


HDR_OVER_FRAME = ('gt identities beyond gt_capacity', 'track ids beyond track_capacity', 'rows beyond ng / nq per frame')


def pack_gt(gt_frames, ng, nc, rows):
    """The ground truth of a batch as one host buffer, pure numpy: B host arrays [m, 7] (or None) -> f32 [B * ng * 7 + 2 B]: the rows
    gt [B, ng, 7], then the counts and the active words as i32 [B] each (view the tail as int32).  rows: one (class, id) -> dense row
    map per stream, updated in place; image i belongs to stream i % len(rows) (frame-major), and the identities of its kind-0 rows are
    replaced by their dense rows, handed out per stream in order of appearance.  None marks an image that is no frame of its stream:
    active word 0, count 0, no row handed out.  Rows beyond ng are left out and the true count is kept (the device counts them)."""
    B, S = len(gt_frames), len(rows)
    n = B * ng * 7
    buf = np.zeros(n + 2 * B, np.float32)
    gt, cnt, act = buf[:n].reshape(B, ng, 7), buf[n:n + B].view(np.int32), buf[n + B:].view(np.int32)
    for b, g in enumerate(gt_frames):
        if g is None:
            continue
        g = np.array(g, np.float32).reshape(-1, 7)
        table = rows[b % S]
        for i in np.flatnonzero((g[:, 6] == 0) & (g[:, 5] >= 0) & (g[:, 5] < nc)):
            g[i, 4] = table.setdefault((int(g[i, 5]), int(g[i, 4])), len(table))
        cnt[b], act[b] = len(g), 1
        gt[b, :min(len(g), ng)] = g[:ng]
    return buf


class _SequenceEvaluator(_Stacked):
    """What the tracking evaluators share: the state on `device`, the ground truth's way up, one update launch per batch and the
    bookkeeping of the sequence in progress.  A subclass names its host path, its state spec and capacities in ops, the offset of its
    overflow counters in hdr with what each counts and the exception they raise, and supplies _ws_bytes, _launch_update and
    _launch_end.
    streams=S (MotEvaluator and HotaEvaluator): one evaluator state per stream, stacked - every state tensor gains a leading S, `rows`
    and `open` are lists with an entry per stream - and still one update launch per batch, one workgroup per stream.  update() then
    takes the frame-major batch (image f * S + s is the f-th frame of stream s, as ByteTracker(streams=S) leaves it)."""
    host = spec = cap_names = hdr_over = over = overflow = None
    _noun = 'an evaluator'

    def __init__(self, device, nc, iou, caps, nq, ng, streams=None):
        self.streams = check_streams(streams)
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise ops._lib.TamtrHipError(f'{type(self).__name__} needs an MI355X; engine.{self.host} is the host path')
        self.nc, self.iou, self.nq, self.ng = int(nc), float(iou), int(nq), int(ng)
        self.caps = tuple(int(c) for c in caps)
        self.gt_capacity = self.caps[0]
        if min(self.nc, self.nq, self.ng, *self.caps) < 1:
            raise ValueError('nc, the capacities, nq and ng must be positive')
        self.workspace = torch.empty(self._ws_bytes(), device=self.device, dtype=torch.uint8)
        self.state = {k: torch.zeros(self._lead + shape(self.nc, self.caps), device=self.device, dtype=dt) for k, dt, shape in self.spec}
        self._fresh()

    def _fresh(self):
        self.rows, self.open = ({}, False) if self.streams is None else ([{} for _ in range(self.streams)], [False] * self.streams)

    def reset(self, stream=None):
        """Forget every count and the sequence in progress (stream=s: stream s's alone).  No synchronisation."""
        if stream is None:
            for v in self.state.values():
                v.zero_()
            self._fresh()
            return
        s = self._stream(stream)
        for v in self.state.values():
            v[s].zero_()
        self.rows[s], self.open[s] = {}, False

    def upload(self, gt_frames):
        """B host arrays [m, 7] -> gt f32 [B, ng, 7] and gcounts i32 [B] on the device, in one pinned copy (pack_gt makes the buffer);
        the ground-truth identities (class, id) of the kind-0 rows are replaced by their dense rows, handed out in order of
        appearance.  With streams=S the batch is frame-major, the rows are handed out per stream, None marks an image that is no
        frame of its stream, and the active words i32 [B] come third."""
        if self.streams is None and any(g is None for g in gt_frames):
            raise ValueError('a ground-truth frame of None (not a frame) belongs to an evaluator built with streams=S')
        B, ng = len(gt_frames), self.ng
        n = B * ng * 7
        buf = pack_gt(gt_frames, ng, self.nc, [self.rows] if self.streams is None else self.rows)
        dev = torch.from_numpy(buf).pin_memory().to(self.device, non_blocking=True)
        gt, words = dev[:n].view(B, ng, 7), dev[n:].view(torch.int32)
        return (gt, words[:B]) if self.streams is None else (gt, words[:B], words[B:])

    def update(self, tracks, tcounts, gt_frames):
        """tracks f32 [B, nq, 8], tcounts i32 [B] on the device (ByteTracker.update); gt_frames: B host arrays [m, 7] x1 y1 x2 y2 id
        cls kind.  The ground truth goes up in one copy (upload), one launch follows; nothing synchronises.  With streams=S the batch
        is frame-major and a gt_frames[i] of None marks image i as no frame of its stream (padding after its end, or a stream that
        is not scored): it counts nothing and its rows are not read."""
        B = tracks.shape[0]
        if len(gt_frames) != B:
            raise ValueError(f'{len(gt_frames)} ground-truth frames for a batch of {B}')
        if self.streams is not None and B % self.streams:
            raise ValueError(f'a batch of {B} images is no multiple of streams = {self.streams} (frame-major: image f * S + s)')
        if tracks.shape[1] > self.nq:
            self.nq = int(tracks.shape[1])
            self.workspace = torch.empty(self._ws_bytes(), device=self.device, dtype=torch.uint8)
        self._launch_update(tracks, tcounts, *self.upload(gt_frames))
        if self.streams is None:
            self.open = True
        else:
            for i, g in enumerate(gt_frames):
                if g is not None:
                    self.open[i % self.streams] = True

    def end_sequence(self, streams=None):
        """Reduce the sequence in progress (the class states the launches) and start a new one: ground-truth ids may be used again.
        No synchronisation.  With streams=S: None ends every open stream, an iterable of stream indices ends those - in one launch
        set either way, the others' state is untouched - and the ground-truth ids of an ended stream may be used again."""
        if self.streams is None:
            if streams is not None:
                raise ValueError(f'streams={streams!r} was given to an evaluator built without streams')
            self._launch_end()
            self.rows, self.open = {}, False
            return
        ending = [s for s in range(self.streams) if self.open[s]] if streams is None else sorted({self._stream(s) for s in streams})
        if not ending:
            return
        words = np.zeros((2, self.streams), np.int32)      # ending, then the dense rows handed out
        words[0, ending] = 1
        words[1] = [len(r) for r in self.rows]
        dev = torch.from_numpy(words).pin_memory().to(self.device, non_blocking=True)
        self._launch_end(dev[0], dev[1])
        for s in ending:
            self.rows[s], self.open[s] = {}, False

    def check_overflow(self, hdr, stream=None):
        """Raise when the header (read by the caller, e.g. from the predictor's packed copy) counts anything beyond a capacity.  With
        streams=S it is the stacked header [S, n] (flat or not), or stream `stream`'s own row, and the message names the streams that
        overflowed."""
        hdr = np.asarray(hdr).reshape(1 if self.streams is None or stream is not None else self.streams, -1)
        said = []
        for s, h in enumerate(hdr, stream or 0):
            over = [(int(h[self.hdr_over + i]), what) for i, what in enumerate(self.over)]
            if any(n for n, _ in over):
                said.append(('' if self.streams is None else f'stream {s}: ') + '; '.join(f'{n} {what}' for n, what in over if n))
        if said:
            raise self.overflow(' | '.join(said) + f' were left out (capacities {", ".join(self.cap_names)} = {self.caps}' +
                                ('' if self.streams is None else ' per stream') + f', ng {self.ng}, nq {self.nq}): build the evaluator with '
                                'larger capacities')

    def _ended(self, stream=None):
        if self.open if self.streams is None else (any(self.open) if stream is None else self.open[stream]):
            raise RuntimeError('a sequence is in progress: call end_sequence() before reading the results')

    def _host_state(self, keys, stream=None):
        """The named state tensors on the host as [S', ...] arrays (synchronises): every stream's, or stream `stream`'s alone (S' = 1)."""
        if stream is not None:
            stream = self._stream(stream)
        self._ended(stream)
        out = []
        for k in keys:
            a = self.state[k] if self.streams is None else self.state[k] if stream is None else self.state[k][stream]
            out.append(a.cpu().numpy().reshape((-1,) + tuple(self.state[k].shape[len(self._lead):])))
        return out

    def _run_counts(self, stream=None):
        """The totals as the host path's counts: per stream, then added in stream order (integers exactly, fp64 sums one add each)."""
        arrays = self._host_state(self.count_keys, stream)
        self.check_overflow(arrays[-1], stream)
        per = [self._counts_of(*(a[s] for a in arrays[:-1])) for s in range(len(arrays[0]))]
        out = per[0]
        for c in per[1:]:
            out = {k: out[k] + c[k] for k in out}
        return out

    def counts(self):
        """The run's counts as the host path returns them (synchronises; raises on overflow); with streams=S the totals of all
        streams."""
        return self._run_counts()

    def stream_counts(self, s):
        """Stream s's totals in the form of counts() (synchronises); a caller gets per-sequence numbers by differencing."""
        return self._run_counts(self._stream(s))


class MotEvaluator(_SequenceEvaluator):
    """CLEAR-MOT and identity counts of tracker rows against ground truth, kept on `device` (csrc/mot.hip states the rule and the
    state).  gt_capacity: ground-truth identities (class, id) per sequence; track_capacity: track ids are used as they are and must
    be below it; nq / ng: track / ground-truth rows per frame the workspace is sized for (a batch with wider track rows gets a larger
    workspace on its first use; ground-truth rows beyond ng are counted as overflow).  The end of a sequence is one launch."""
    times_key = 'mot'      # the key of Predictor.times this evaluator's launches go under
    host, spec, cap_names = 'mot_evaluate', ops.MOT_STATE_SPEC, ops.MOT_CAPS
    hdr_over, over, overflow = MOT_HDR_OVER_GT, HDR_OVER_FRAME, MotOverflow

    count_keys = ('counts', 'iou_sum', 'hdr')

    def __init__(self, device, nc, iou=0.5, gt_capacity=1024, track_capacity=4096, nq=300, ng=300, streams=None):
        super().__init__(device, nc, iou, (gt_capacity, track_capacity), nq, ng, streams)
        self.track_capacity = self.caps[1]

    def _ws_bytes(self):
        return ops.mot_workspace_bytes(self.nq, self.ng, self.nc, *self.caps, *self._lead)

    def _launch_update(self, tracks, tcounts, gt, gcounts, active=None):
        ops.mot_update(tracks, tcounts, gt, gcounts, self.state, self.nc, *self.caps, self.iou, self.workspace, self.streams, active)

    def _launch_end(self, ending=None, gt_used=None):
        ops.mot_end_sequence(self.state, self.nc, *self.caps, len(self.rows) if self.streams is None else gt_used, self.workspace,
                             self.streams, ending)

    def _counts_of(self, c, s):
        """One state's totals as engine.mot_evaluate returns them."""
        from .engine import MOT_COUNT_KEYS
        out = {k: c[:, i].astype(np.int64) for i, k in enumerate(MOT_COUNT_KEYS)}
        out['iou_sum'] = s.copy()
        return out

    def results(self, names=None):
        """engine.mot_summary of the sequences ended so far (synchronises; raises MotOverflow)."""
        from .engine import mot_summary
        return mot_summary(self.counts(), names)


# ------------------------------------------------------------------------------------------------ HOTA
HOTA_HDR_OVER = HDR_OVER_FRAME + ('pairs beyond log_capacity', 'frames beyond frame_capacity',
                                  'pairs that found no slot in pair_capacity')   # hdr[2:8]


class HotaEvaluator(_SequenceEvaluator):
    """HOTA counts of tracker rows against ground truth, kept on `device` (csrc/hota.hip states the rule and the state).  The methods
    are MotEvaluator's.  gt_capacity / track_capacity / nq / ng as there; pair_capacity: slots of the sparse pair table (distinct
    (ground truth, track) pairs with a positive IoU in a sequence; the table fills badly beyond about half); log_capacity: positive
    pairs logged over the frames of a sequence; frame_capacity: frames of a sequence.  The defaults hold a 2 000-frame sequence of
    100 rows a side several times over and take 85 MiB with the workspace.  The end of a sequence is the second pass and the
    reduction, three launches."""
    times_key = 'hota'
    host, spec, cap_names = 'hota_evaluate', ops.HOTA_STATE_SPEC, ops.HOTA_CAPS
    hdr_over, over, overflow = 2, HOTA_HDR_OVER, HotaOverflow

    count_keys = ('dets', 'tp_lvl', 'loc_lvl', 'ass', 'hdr')

    def __init__(self, device, nc, iou=0.5, gt_capacity=1024, track_capacity=4096, pair_capacity=1 << 18, log_capacity=1 << 20,
                 frame_capacity=4096, nq=300, ng=300, streams=None):
        super().__init__(device, nc, iou, (gt_capacity, track_capacity, pair_capacity, log_capacity, frame_capacity), nq, ng, streams)

    def _ws_bytes(self):
        return ops.hota_workspace_bytes(self.nq, self.ng, streams=self.streams)

    def _launch_update(self, tracks, tcounts, gt, gcounts, active=None):
        ops.hota_update(tracks, tcounts, gt, gcounts, self.state, self.nc, self.caps, self.iou, self.workspace, self.streams, active)

    def _launch_end(self, ending=None, gt_used=None):
        ops.hota_end_sequence(self.state, self.nc, self.caps, self.nq, self.ng, self.workspace, streams=self.streams, ending=ending)

    def _counts_of(self, dets, tp, loc, ass):
        """One state's totals as engine.hota_evaluate returns them."""
        above = lambda lvl: np.cumsum(lvl[:, ::-1], 1)[:, ::-1][:, 1:]   # noqa: E731  a pair at level k counts for every threshold a < k
        out = {'TP': above(tp.astype(np.int64)), 'loc_sum': above(loc), 'ass_sum': ass[0].copy(), 'assre_sum': ass[1].copy(),
               'asspr_sum': ass[2].copy(), 'gt_dets': dets[:, 0].astype(np.int64), 'trk_dets': dets[:, 1].astype(np.int64)}
        out['FN'], out['FP'] = out['gt_dets'][:, None] - out['TP'], out['trk_dets'][:, None] - out['TP']
        return out

    def results(self, names=None):
        """engine.hota_summary of the sequences ended so far (synchronises; raises HotaOverflow)."""
        from .engine import hota_summary
        return hota_summary(self.counts(), names)


# ------------------------------------------------------------------------------------------------ track-mAP
TRACKMAP_HDR_OVER = HDR_OVER_FRAME + ('pairs that found no slot in pair_capacity', 'tracks beyond row_capacity')   # hdr[2:7]


class TrackMapEvaluator(_SequenceEvaluator):
    """Track-mAP of tracker rows against ground truth, kept on `device` (csrc/trackmap.hip states the rule and the state): average
    precision over whole tracks, ranked by mean score and matched by spatio-temporal IoU at `thresholds` (1 to 10 values; the default
    is VisDrone-MOT's, np.linspace(0.5, 0.95, 10) gives TrackEval's).  The methods are MotEvaluator's.  gt_capacity / track_capacity /
    nq / ng as there; pair_capacity: slots of the sparse pair table (distinct (ground truth, track) pairs that intersect in a sequence;
    the table fills badly beyond about half); row_capacity: track identities of the whole run.  The end of a sequence matches its
    tracks and appends them to the run's table, six launches; track ids may be used again after it too."""
    times_key = 'tmap'
    host, spec, cap_names = 'track_map_evaluate', ops.TRACKMAP_STATE_SPEC, ops.TRACKMAP_CAPS
    hdr_over, over, overflow = 2, TRACKMAP_HDR_OVER, TrackMapOverflow

    def __init__(self, device, nc, thresholds=(0.25, 0.5, 0.75), iou=0.5, gt_capacity=1024, track_capacity=4096, pair_capacity=1 << 18,
                 row_capacity=1 << 16, nq=300, ng=300):
        from .engine import track_map_thresholds
        super().__init__(device, nc, iou, (gt_capacity, track_capacity, pair_capacity, row_capacity), nq, ng)
        self.thresholds = track_map_thresholds(thresholds)

    def _ws_bytes(self):
        return ops.trackmap_workspace_bytes(self.nq, self.ng, self.nc, self.caps)

    def _launch_update(self, tracks, tcounts, gt, gcounts):
        ops.trackmap_update(tracks, tcounts, gt, gcounts, self.state, self.nc, self.caps, self.iou, self.workspace)

    def _launch_end(self):
        ops.trackmap_end_sequence(self.state, self.nc, self.caps, self.thresholds, self.workspace)

    def _read(self, *keys):
        self._ended()
        hdr = self.state['hdr'].cpu().numpy()
        self.check_overflow(hdr)
        n = int(hdr[0])
        return n, [self.state[k][:n].cpu().numpy() if k != 'gt_tracks' else self.state[k].cpu().numpy() for k in keys]

    def counts(self):
        """The run's counts as engine.track_map_evaluate returns them (synchronises; raises TrackMapOverflow)."""
        _, (score, meta, gtt) = self._read('rscore', 'rmeta', 'gt_tracks')
        return {'score': score.copy(), 'cls': meta[:, 0].astype(np.int64), 'bits': meta[:, 1].astype(np.int32),
                'gt_tracks': gtt.astype(np.int64), 'thresholds': self.thresholds.copy()}

    def results(self, names=None):
        """engine.track_map_rows of the sequences ended so far, accumulated on the device (ops.trackmap_accumulate; synchronises;
        raises TrackMapOverflow)."""
        from .engine import track_map_rows
        n, (meta, gtt) = self._read('rmeta', 'gt_tracks')
        ap, ar = (x.cpu().numpy() for x in ops.trackmap_accumulate(self.state, self.nc, self.caps, len(self.thresholds)))
        return track_map_rows(ap, ar, gtt, np.bincount(meta[:, 0], minlength=self.nc)[:self.nc], self.thresholds, names)


def pack_track_rows(frames, nq, device):
    """Per-frame host rows [k, 6] (x1 y1 x2 y2 id cls, read_mot(gt=False)) or [k, 7] (with the score, read_mot(gt=False, scores=True)) ->
    tracks f32 [B, nq, 8] and tcounts i32 [B] on `device`, laid out as ByteTracker.update leaves them (the score in column 5, 1 for
    [k, 6] rows; idx = the row), in one copy.  A frame with more than nq rows keeps its count."""
    B = len(frames)
    buf = np.zeros(B * nq * 8 + B, np.float32)
    rows, cnt = buf[:B * nq * 8].reshape(B, nq, 8), buf[B * nq * 8:].view(np.int32)
    for b, f in enumerate(frames):
        f = np.asarray(f, np.float32)
        f = f.reshape(-1, 7 if f.ndim == 2 and f.shape[1] == 7 else 6)
        k = min(len(f), nq)
        rows[b, :k, :5], rows[b, :k, 5], rows[b, :k, 6], rows[b, :k, 7] = f[:k, :5], f[:k, 6] if f.shape[1] == 7 else 1.0, f[:k, 5], np.arange(k)
        cnt[b] = len(f)
    dev = torch.from_numpy(buf).to(device)
    return dev[:B * nq * 8].view(B, nq, 8), dev[B * nq * 8:].view(torch.int32)


def read_mot(path, gt=True, category_map=None, frames=None, scores=False):
    """A VisDrone-MOT file (`frame,id,left,top,width,height,score,category,truncation,occlusion`, frames 1-based) -> one fp32 array per
    frame 1 .. max(last frame in the file, `frames`).  gt=True: an annotation file -> [m, 7] x1 y1 x2 y2 id cls kind, where category 0
    (ignored region) gives kind 2, `score == 0` or category 11 (others) gives kind 1, and categories 1 .. 10 give classes 0 .. 9 with
    kind 0; category_map {category: (cls, kind)} replaces that table (a category it lacks is a distractor).  gt=False: a result file
    as write_mot writes it -> [k, 6] x1 y1 x2 y2 id cls, the category being the class; with scores=True [k, 7], the file's score last."""
    table = VISDRONE_CATEGORIES if category_map is None else category_map
    rows = {}
    with open(path) as fh:
        for line in fh:
            v = line.replace(',', ' ').split()
            if not v:
                continue
            f, tid, x, y, w, h, score, cat = int(float(v[0])), float(v[1]), *(float(e) for e in v[2:7]), int(float(v[7]))
            box = [x, y, x + w, y + h, tid]
            if gt:
                cls, kind = table.get(cat, (0, 1))
                if kind == 0 and score == 0:
                    kind = 1
                rows.setdefault(f, []).append(box + [cls, kind])
            else:
                rows.setdefault(f, []).append(box + [cat] + ([score] if scores else []))
    n = max(max(rows, default=0), frames or 0)
    return [np.asarray(rows.get(f, []), np.float32).reshape(-1, 7 if gt or scores else 6) for f in range(1, n + 1)]
