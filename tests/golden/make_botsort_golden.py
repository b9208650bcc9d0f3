#!/usr/bin/env python3
"""Generate tests/golden/botsort.npz by running the *reference's* BOTSORT (ultralytics/trackers/bot_sort.py) on the CPU over seeded
sequences seen by a moving camera.  Runs only where the reference is present; the import recipe is make_track_golden.py's.

    python tests/golden/make_botsort_golden.py

utils/gmc.py imports cv2 at the top and this generator calls nothing of it: make_golden's import recipe registers an inert module of
that name, `lap` is replaced as in make_track_golden.py, and `tracker.gmc` is replaced by an object whose `apply` returns the next
prescribed warp.  BOTSORT.update(Boxes(frame), img=<dummy array>) is driven frame by frame, so the warp is applied on every frame that
reaches the tracker; a frame without detections does not reach it (trackers/track.py:46-47) and its warp is dropped.

Sequences (detections are world positions pushed through the camera's accumulated motion, the warps are the camera's):
  pan    a crowd under a camera that pans, rotates and zooms a little and jumps by about 50 px at frame JUMP
  aniso  a short one whose warps are no similarities (anisotropic R): ours are such in original pixels when sx != sy
  gaps   one with empty frames, the first frame among them

What is stored (data only), per sequence s in `names`: what track.npz stores ({s}_cnt, _det, _cls, _rcnt, _box, _id, _idx, _fin_meta,
_fin_sc, _fin_mean, _fin_cov; see make_track_golden.py) plus {s}_warp f64 [F, 2, 3].

The numpy twin (tests/botsort_np.py) runs in lockstep and must agree on every frame; the generator asserts the margins of
make_track_golden.py (scores and costs > 1e-3 from their thresholds, every assignment's optimum > 1e-6 from the runner-up) and that
the sequences exercise each rule counted below.  If an assertion fails, change the seed.
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as G  # noqa: E402
import make_track_golden as M  # noqa: E402
import bytetrack_np as T  # noqa: E402
import botsort_np as BS  # noqa: E402

CAP = 64
PAN_SEED, ANISO_SEED, GAPS_SEED = 37, 5, 8       # seeds 14-36 of the pan put a cost within 1e-3 of a threshold
JUMP, JUMP_BY = 45, (46.0, 31.0)
CFG = dict(M.CFG)
ARGS = dict(CFG, gmc_method='sparseOptFlow', proximity_thresh=0.5, appearance_thresh=0.25, with_reid=False)


class PrescribedGMC:
    def __init__(self, warps):
        self.warps, self.calls = [np.asarray(w, np.float64) for w in warps], 0

    def apply(self, img, dets=None):
        self.calls += 1
        return self.warps.pop(0).copy()


def sequences():
    pan = M.crowd(PAN_SEED)
    wp = BS.camera_path(PAN_SEED, len(pan), jumps={JUMP: JUMP_BY})
    an = T.make_scene(ANISO_SEED, n_obj=6, frames=13, fp_every=4, p_low=0.1)
    wa = BS.camera_path(ANISO_SEED, len(an), pan=(2.0, -1.0), aniso=0.004)
    gp = T.make_scene(GAPS_SEED, n_obj=6, frames=20, fp_every=5, p_low=0.1, empty=(0, 7, 8, 19))
    wg = BS.camera_path(GAPS_SEED, len(gp), pan=(-2.5, 1.0))
    return (('pan', BS.through_camera(pan, wp), wp), ('aniso', BS.through_camera(an, wa), wa), ('gaps', BS.through_camera(gp, wg), wg))


def run(name, frames, warps, tracker, twin, d):
    tracker.gmc = PrescribedGMC([w for fr, w in zip(frames, warps) if len(fr)])
    img = np.zeros((8, 8, 3), np.uint8)
    cnt, rcnt, det, box, ids, idxs = [], [], [], [], [], []
    for f, (fr, w) in enumerate(zip(frames, warps)):
        rows = np.zeros((0, 8), np.float32)
        if len(fr):
            rows = np.asarray(tracker.update(M.Boxes(fr), img=img), np.float32).reshape(-1, 8)
        mine = twin.update(fr, w)
        assert sorted(zip(rows[:, 4], rows[:, 7])) == sorted(zip(mine[:, 4], mine[:, 7])), (name, f, rows[:, [4, 7]], mine[:, [4, 7]])
        o1, o2 = np.argsort(rows[:, 4]), np.argsort(mine[:, 4])
        assert np.allclose(rows[o1, :4], mine[o2, :4], rtol=1e-6, atol=5e-4) and np.array_equal(rows[o1, 5:7], mine[o2, 5:7]), (name, f)
        M.same_live(M.ref_live(tracker), twin.live())
        k = rows[:, 7].astype(int)
        assert np.array_equal(rows[:, 5:7], fr[k, 4:6]), 'a row does not carry the score and class of detection idx'
        cnt.append(len(fr)); rcnt.append(len(rows)); det.append(fr); box.append(rows[:, :4]); ids.append(rows[:, 4]); idxs.append(rows[:, 7])
    assert not tracker.gmc.warps and tracker.gmc.calls == sum(len(fr) > 0 for fr in frames)
    det = np.concatenate(det)
    d[f'{name}_cnt'], d[f'{name}_det'], d[f'{name}_cls'] = np.array(cnt, np.int32), det[:, :5], det[:, 5].astype(np.uint8)
    d[f'{name}_rcnt'], d[f'{name}_box'] = np.array(rcnt, np.int32), np.concatenate(box)
    d[f'{name}_id'], d[f'{name}_idx'] = np.concatenate(ids).astype(np.int16), np.concatenate(idxs).astype(np.int16)
    d[f'{name}_warp'] = np.asarray(warps, np.float64)
    live = M.ref_live(tracker)
    keys = sorted(live)
    d[f'{name}_fin_meta'] = np.array([(k,) + live[k][:6] for k in keys], np.int32).reshape(-1, 7)
    d[f'{name}_fin_sc'] = np.array([live[k][6:8] for k in keys], np.float32).reshape(-1, 2)
    d[f'{name}_fin_mean'] = np.array([live[k][8] for k in keys]).reshape(-1, 8)
    d[f'{name}_fin_cov'] = np.array([live[k][9] for k in keys]).reshape(-1, 8, 8)
    print(f'{name}: {len(frames)} frames, {int(det.shape[0])} detections, {sum(rcnt)} rows, ids up to {int(twin.state["hdr"][T.H_NEXT]) - 1}, '
          f'margin {twin.margin:.3g}, threshold margin {twin.thr_margin:.3g}\n   {twin.events}')
    assert twin.margin > 1e-6, (name, 'an assignment is not unique enough: change the seed', twin.margin)
    assert twin.thr_margin > 1e-3, (name, 'a score or cost is too close to its threshold: change the seed', twin.thr_margin)
    return twin.events, [set(i.astype(int)) for i in ids]


def kept_across(ids, f):
    return ids[f - 1] & ids[f]


def main():
    M.import_tracker()
    from ultralytics.trackers import bot_sort
    assert bot_sort.BOTSORT(types.SimpleNamespace(**ARGS)).kalman_filter.__class__.__name__ == 'KalmanFilterXYWH'
    d, events, jump_gain = {}, {}, 0
    for name, frames, warps in sequences():
        tracker = bot_sort.BOTSORT(types.SimpleNamespace(**ARGS), frame_rate=30)
        ev, ids = run(name, frames, warps, tracker, BS.BotSortNp(capacity=CAP, want_margin=True, **CFG), d)
        events = {k: events.get(k, 0) + v for k, v in ev.items()}
        if name == 'pan':      # the same detections without compensation: the jump costs tracks
            blind = BS.BotSortNp(capacity=CAP, **CFG)
            bids = [set(blind.update(fr)[:, 4].astype(int)) for fr in frames]
            kept, bkept = kept_across(ids, JUMP), kept_across(bids, JUMP)
            print(f'   across the jump at frame {JUMP}: {len(kept)} of {len(ids[JUMP - 1])} ids kept, {len(bkept)} of {len(bids[JUMP - 1])} '
                  'with identity warps')
            jump_gain = len(kept) - len(bkept)
            assert len(kept) >= len(ids[JUMP - 1]) - 1, 'the compensated run loses tracks at the jump: change the seed'
    events['kept_across_jump'] = jump_gain
    for k in ('match1', 'match2', 'refind', 'aged_out', 'unconfirmed_removed', 'warp_unconfirmed', 'lost_zeroed_vw_vh', 'empty_frame',
              'kept_across_jump'):
        assert events[k] >= 1, ('the sequences never exercise', k, 'change the seed', events)
    d['names'] = np.array(['pan', 'aniso', 'gaps'])
    d['capacity'] = CAP
    d['jump'] = JUMP
    G.save('botsort', d)


if __name__ == '__main__':
    main()
