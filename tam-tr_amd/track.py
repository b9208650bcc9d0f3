"""ByteTrack multi-object tracking on the device (the reference's ultralytics/trackers: track.py, byte_tracker.py, basetrack.py,
utils/kalman_filter.py, utils/matching.py, cfg/trackers/bytetrack.yaml): one HIP launch per predictor batch, state in device buffers.

    from tamtr_amd.track import ByteTracker
    tracker = ByteTracker(device)                       # or ByteTracker.from_yaml('bytetrack.yaml', device)
    tracks, tcounts = tracker.update(out, counts)       # the outputs of ops.detect_postprocess, frames in order; no synchronisation

`Predictor.track(source)` (predict.py) drives it and yields Detections with ids; tools/track.py is the command line.
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


def read_tracker_yaml(path):
    """The keys of the reference's cfg/trackers/bytetrack.yaml -> constructor arguments.  Only `tracker_type: bytetrack` is built."""
    import yaml
    with open(path) as f:
        cfg = yaml.safe_load(f) or {}
    kind = cfg.get('tracker_type', 'bytetrack')
    if kind != 'bytetrack':
        raise ValueError(f"tracker_type {kind!r} is not supported: only 'bytetrack' is built (BoT-SORT needs optical flow on the host)")
    return {k: cfg[k] for k in YAML_KEYS if k in cfg}


class ByteTracker:
    """One tracker = one slot table of `capacity` tracks on `device` (ids start at 1).  nq is the number of rows per frame the
    workspace is sized for; a batch with more rows gets a larger workspace on its first use."""

    def __init__(self, device, track_high_thresh=0.5, track_low_thresh=0.1, new_track_thresh=0.6, track_buffer=30, match_thresh=0.8,
                 frame_rate=30, capacity=1024, nq=300):
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
        self.workspace = torch.empty(ops.bytetrack_workspace_bytes(self.capacity, self.nq), device=self.device, dtype=torch.uint8)
        self.state = {k: torch.zeros((self.capacity,) + tail, device=self.device, dtype=dt) for k, dt, tail in ops.TRACK_STATE_SPEC}
        self.state['hdr'] = torch.zeros(8, device=self.device, dtype=torch.int32)
        self._fresh_hdr = torch.tensor([0, 1, 0, 0, 0, 0, 0, 0], dtype=torch.int32).to(self.device)
        self.reset()

    @classmethod
    def from_yaml(cls, path, device, **kw):
        return cls(device, **{**read_tracker_yaml(path), **kw})

    def reset(self):
        """Forget every track; the next id is 1 again.  No synchronisation."""
        self.state['meta'].zero_()
        self.state['hdr'].copy_(self._fresh_hdr)

    def update(self, out, counts):
        """out f32 [B, nq, 6], counts i32 [B] on the device (ops.detect_postprocess) -> tracks f32 [B, nq, 8] (x1 y1 x2 y2 id score
        cls idx, zero after the count), tcounts i32 [B], on the device.  The B frames are consumed in order in one launch."""
        if out.dim() == 3 and out.shape[1] > self.nq:
            self.nq = out.shape[1]
            self.workspace = torch.empty(ops.bytetrack_workspace_bytes(self.capacity, self.nq), device=self.device, dtype=torch.uint8)
        return ops.bytetrack_update(out, counts, self.state, self.capacity, self.track_high_thresh, self.track_low_thresh,
                                    self.new_track_thresh, self.match_thresh, self.max_time_lost, self.workspace)

    def check_overflow(self, overflow):
        """Raise when the header's overflow count (read by the caller, e.g. from the predictor's packed copy) is not zero."""
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
        self.check_overflow(np.asarray(sd['hdr'])[HDR_OVERFLOW])


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
