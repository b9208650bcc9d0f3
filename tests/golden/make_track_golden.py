#!/usr/bin/env python3
"""Generate tests/golden/track.npz by running the *reference's* BYTETracker (ultralytics/trackers/byte_tracker.py) on the CPU over seeded
sequences.  Runs only where the reference is present; the import recipe is make_golden.py's.

    python tests/golden/make_track_golden.py

The reference solves its assignments with `lap`, which is not needed here: before ultralytics.trackers is imported a module named `lap`
goes into sys.modules whose lapjv builds the extended matrix lap builds for extend_cost=True and solves it with scipy
(tests/bytetrack_np.py: lapjv_extended).  BYTETracker.update is driven directly, with the two `continue`s of trackers/track.py:46-50
restated: a frame without detections does not reach the tracker.

What is stored (data only), per sequence s in `names`:
  {s}_cnt i32 [F], {s}_det f32 [sum cnt, 5] (x1 y1 x2 y2 score) and {s}_cls u8 [sum cnt]: the detections, frames concatenated;
  {s}_rcnt i32 [F], {s}_box f32 [sum rcnt, 4], {s}_id i16, {s}_idx i16: the returned rows (their score and cls are asserted to be those
  of detection idx, so they are not stored);
  {s}_fin_meta i32 [k, 7] (id, state, is_activated, frame_id, start_frame, tracklet_len, idx), {s}_fin_sc f32 [k, 2] (score, cls),
  {s}_fin_mean f64 [k, 8], {s}_fin_cov f64 [k, 8, 8]: every track of the final tracked and lost lists, by id.
The staged sequence starts from a table built from STrack objects made by hand, stored as staged_mean / _cov / _meta / _sc / _hdr in
the layout of ByteTracker.load_state_dict (capacity 64).

The numpy twin runs in lockstep and must agree on every frame; its counters then say which rules the sequences exercised, and the
generator asserts each of them, the distance of every score and cost from its threshold (> 1e-3) and of every assignment's optimum
from the runner-up (> 1e-6).  If an assertion fails, change the seed.
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as G  # noqa: E402
import bytetrack_np as T  # noqa: E402

CAP = 64
CROWD_SEED, TWINS_SEED = 14, 3       # seeds 11-13 of the crowd put a cost within 1e-3 of a threshold
CFG = dict(track_high_thresh=0.5, track_low_thresh=0.1, new_track_thresh=0.6, track_buffer=30, match_thresh=0.8)


def import_tracker():
    G._import_reference()
    lap = types.ModuleType('lap')
    lap.__version__ = '0.0-scipy'
    lap.lapjv = lambda cost, extend_cost=True, cost_limit=np.inf: T.lapjv_extended(cost, cost_limit)
    sys.modules['lap'] = lap
    from ultralytics.trackers import byte_tracker, basetrack
    from ultralytics.trackers.utils.kalman_filter import KalmanFilterXYAH
    return byte_tracker, basetrack, KalmanFilterXYAH


def crowd(seed):
    return T.make_scene(seed, n_obj=24, frames=90, p_low=0.15, fp_every=4, empty=(37,), gaps=[(0, 20, 3), (1, 30, 8), (2, 25, 40), (3, 50, 3)])


def twins(seed):
    """Pairs of near-coincident boxes of different classes; the second of a pair vanishes for a while."""
    rng = np.random.default_rng(seed)
    frames, pairs = 40, 4
    cx, cy = rng.uniform(200, 1700, pairs), rng.uniform(150, 900, pairs)
    vx, vy = rng.uniform(-3, 3, pairs), rng.uniform(-2, 2, pairs)
    w, h = rng.uniform(60, 110, pairs), rng.uniform(90, 150, pairs)
    off = rng.uniform(1.5, 3.0, (pairs, 2)) * rng.choice([-1, 1], (pairs, 2))
    out = []
    for f in range(frames):
        rows = []
        for p in range(pairs):
            for t in range(2):
                if t == 1 and (8 + 6 * p <= f < 14 + 6 * p):
                    continue
                j = rng.normal(0, 0.4, 4)
                x, y = cx[p] + vx[p] * f + t * off[p, 0] + j[0], cy[p] + vy[p] * f + t * off[p, 1] + j[1]
                ww, hh = w[p] + j[2], h[p] + j[3]
                s = rng.uniform(0.15, 0.45) if rng.random() < 0.12 else rng.uniform(0.65, 0.95)
                rows.append([x - ww / 2, y - hh / 2, x + ww / 2, y + hh / 2, s, 2 * p + t])
        if f % 5 == 3:
            x, y = rng.uniform(100, 1800), rng.uniform(100, 1000)
            rows.append([x - 30, y - 40, x + 30, y + 40, rng.uniform(0.65, 0.9), 9])
        a = np.array(rows, np.float32).reshape(-1, 6)
        out.append(a[rng.permutation(len(a))])
    return out


class Boxes:
    def __init__(self, d):
        self.xyxy, self.conf, self.cls = d[:, :4], d[:, 4], d[:, 5]


def ref_live(tracker):
    """{id: (state, activated, frame_id, start_frame, tracklet_len, idx, score, cls, mean, cov)} of the tracked and lost lists."""
    return {int(t.track_id): (int(t.state), int(t.is_activated), int(t.frame_id), int(t.start_frame), int(t.tracklet_len), int(t.idx),
                              np.float32(t.score), np.float32(t.cls), np.asarray(t.mean, np.float64), np.asarray(t.covariance, np.float64))
            for t in tracker.tracked_stracks + tracker.lost_stracks}


def same_live(a, b):
    assert set(a) == set(b), (sorted(a), sorted(b))
    for k in a:
        assert a[k][:6] == b[k][:6] and a[k][6] == b[k][6] and a[k][7] == b[k][7], (k, a[k][:8], b[k][:8])
        for u, v in ((a[k][8], b[k][8]), (a[k][9], b[k][9])):
            assert np.abs(u - v).max() <= 1e-6 * np.abs(u).max(), (k, u, v)


def run(name, frames, tracker, twin, d):
    cnt, rcnt, det, box, ids, idxs = [], [], [], [], [], []
    for f, fr in enumerate(frames):
        rows = np.zeros((0, 8), np.float32)
        if len(fr):
            rows = np.asarray(tracker.update(Boxes(fr)), np.float32).reshape(-1, 8)
        mine = twin.update(fr)
        assert sorted(zip(rows[:, 4], rows[:, 7])) == sorted(zip(mine[:, 4], mine[:, 7])), (name, f, rows[:, [4, 7]], mine[:, [4, 7]])
        o1, o2 = np.argsort(rows[:, 4]), np.argsort(mine[:, 4])
        assert np.allclose(rows[o1, :4], mine[o2, :4], rtol=1e-6, atol=5e-4) and np.array_equal(rows[o1, 5:7], mine[o2, 5:7]), (name, f)
        same_live(ref_live(tracker), twin.live())
        k = rows[:, 7].astype(int)
        assert np.array_equal(rows[:, 5:7], fr[k, 4:6]), 'a row does not carry the score and class of detection idx'
        cnt.append(len(fr)); rcnt.append(len(rows)); det.append(fr); box.append(rows[:, :4]); ids.append(rows[:, 4]); idxs.append(rows[:, 7])
    det = np.concatenate(det)
    d[f'{name}_cnt'], d[f'{name}_det'], d[f'{name}_cls'] = np.array(cnt, np.int32), det[:, :5], det[:, 5].astype(np.uint8)
    d[f'{name}_rcnt'], d[f'{name}_box'] = np.array(rcnt, np.int32), np.concatenate(box)
    d[f'{name}_id'], d[f'{name}_idx'] = np.concatenate(ids).astype(np.int16), np.concatenate(idxs).astype(np.int16)
    live = ref_live(tracker)
    keys = sorted(live)
    d[f'{name}_fin_meta'] = np.array([(k,) + live[k][:6] for k in keys], np.int32).reshape(-1, 7)
    d[f'{name}_fin_sc'] = np.array([live[k][6:8] for k in keys], np.float32).reshape(-1, 2)
    d[f'{name}_fin_mean'] = np.array([live[k][8] for k in keys]).reshape(-1, 8)
    d[f'{name}_fin_cov'] = np.array([live[k][9] for k in keys]).reshape(-1, 8, 8)
    print(f'{name}: {len(frames)} frames, {int(det.shape[0])} detections, {sum(rcnt)} rows, ids up to {int(twin.state["hdr"][T.H_NEXT]) - 1}, '
          f'margin {twin.margin:.3g}, threshold margin {twin.thr_margin:.3g}\n   {twin.events}')
    assert twin.margin > 1e-6, (name, 'an assignment is not unique enough', twin.margin)
    assert twin.thr_margin > 1e-3, (name, 'a score or cost is too close to its threshold', twin.thr_margin)
    return twin.events


def staged(bt, base, KF):
    """A table in which the TRACKED side of a duplicate pair goes: a young tracked track sits on an older lost one."""
    kf = KF()
    boxes = {1: (400, 300, 480, 420), 2: (402, 303, 482, 423), 3: (900, 500, 1000, 640), 4: (1300, 200, 1360, 330)}
    spec = {1: (bt.TrackState.Tracked, 10, 8, 2), 2: (bt.TrackState.Lost, 7, 1, 6), 3: (bt.TrackState.Tracked, 10, 2, 8),
            4: (bt.TrackState.Lost, 9, 3, 6)}        # state, frame_id, start_frame, tracklet_len
    st = T.new_state(CAP)
    tracked, lost = [], []
    for s, (tid, b) in enumerate(boxes.items()):
        t = bt.STrack(np.array(b + (0,), np.float64), np.float32(0.8), np.float32(tid % 3))
        t.kalman_filter = kf
        mean, cov = kf.initiate(t.convert_coords(t._tlwh))
        t.mean, t.covariance = np.asarray(mean, np.float64), np.asarray(cov, np.float64)
        t.state, t.frame_id, t.start_frame, t.tracklet_len = spec[tid]
        t.track_id, t.is_activated = tid, True
        (tracked if t.state == bt.TrackState.Tracked else lost).append(t)
        slot = 2 * s + 1                            # not the first slots: the table need not be dense
        st['mean'][slot], st['cov'][slot] = t.mean, t.covariance
        st['meta'][slot] = t.state, 1, tid, t.frame_id, t.start_frame, t.tracklet_len, 0, 0
        st['sc'][slot] = 0.8, tid % 3
    st['hdr'][:3] = 10, 5, 4
    tracker = bt.BYTETracker(types.SimpleNamespace(**CFG), frame_rate=30)
    tracker.tracked_stracks, tracker.lost_stracks, tracker.frame_id = tracked, lost, 10
    base.BaseTrack._count = 4
    rng = np.random.default_rng(5)
    frames = []
    for f in range(6):
        rows = [[400 + f, 300, 480 + f, 420, 0.9, 1], [900 + 2 * f, 500, 1000 + 2 * f, 640, 0.85, 0]]
        if f >= 2:
            rows.append([1300, 200 + f, 1360, 330 + f, 0.75, 1])
        if f == 3:
            rows.append([100, 100, 160, 190, 0.3, 2])
        a = np.array(rows, np.float32) + np.concatenate([rng.normal(0, 0.3, (len(rows), 4)), np.zeros((len(rows), 2))], 1).astype(np.float32)
        frames.append(a[rng.permutation(len(a))])
    return st, tracker, frames


def main():
    bt, base, KF = import_tracker()
    d, events = {}, {}
    for name, frames in (('crowd', crowd(CROWD_SEED)), ('twins', twins(TWINS_SEED))):
        tracker = bt.BYTETracker(types.SimpleNamespace(**CFG), frame_rate=30)
        ev = run(name, frames, tracker, T.ByteTrackNp(capacity=CAP, want_margin=True, **CFG), d)
        events = {k: events.get(k, 0) + v for k, v in ev.items()}
    st, tracker, frames = staged(bt, base, KF)
    for k, v in st.items():
        d[f'staged_{k}'] = v.copy()
    twin = T.ByteTrackNp(capacity=CAP, want_margin=True, **CFG)
    twin.state = st
    ev = run('staged', frames, tracker, twin, d)
    assert ev['dup_tracked_dropped'] >= 1, ev
    events = {k: events.get(k, 0) + v for k, v in ev.items()}
    for k in ('match1', 'match2', 'refind', 'aged_out', 'unconfirmed_removed', 'new_refused', 'dup_lost_dropped', 'dup_tracked_dropped',
              'empty_frame'):
        assert events[k] >= 1, ('the sequences never exercise', k, events)
    d['names'] = np.array(['crowd', 'twins', 'staged'])
    d['capacity'] = CAP
    G.save('track', d)


if __name__ == '__main__':
    main()
