#!/usr/bin/env python3
"""Generate tests/golden/botsort_reid.npz by running the *reference's* BOTSORT (ultralytics/trackers/bot_sort.py) with with_reid on,
on the CPU.  Runs only where the reference is present; the import recipe is make_track_golden.py's.

    python tests/golden/make_botsort_reid_golden.py

The reference writes the appearance rule out (BOTrack.update_features, BOTSORT.init_track, BOTSORT.get_dists,
matching.embedding_distance) and leaves `self.encoder = None`.  After construction `tracker.encoder` is set to a stub whose
inference(img, dets) returns a fresh fp32 copy of the prescribed row of every detection in dets[:, 4], the detection index that
BYTETracker.update appends; `tracker.gmc` is make_botsort_golden.py's prescribed-warp object.  Nothing of the reference is changed.

Sequences (features: botsort_reid_np.object_features, fp16 values at D = 16, a fixed axis per object plus per-detection noise that
puts the halved cosine distance to the own track on both sides of appearance_thresh):
  crowd  12 objects for 90 frames under a camera that pans, rotates and zooms a little; gaps, low scores, false positives, one empty frame
  cross  pairs of same-size objects that overlap and turn back where they meet (botsort_reid_np.make_cross), camera at rest
  gaps   a short one with empty frames, the first frame among them

What is stored (data only), per sequence s in `names`: what botsort.npz stores ({s}_cnt, _det, _cls, _rcnt, _box, _id, _idx, _warp,
_fin_meta, _fin_sc, _fin_mean, _fin_cov; see make_track_golden.py) plus {s}_feat f16 [sum cnt, D] (the raw feature row of every
detection), {s}_obj i8 [sum cnt] (the object a detection shows, -1 = false positive) and {s}_fin_feat f32 [k, D] (the reference's
smooth_feat of every track of the final lists, by id); feat_bound = the largest distance seen between the fp32 and the fp64
statement of a smooth_feat.

The numpy twin (tests/botsort_reid_np.py) runs in lockstep, once with fp32 features as numpy computes them and once with fp64
features.  Asserted: the fp32 twin equals the reference on every frame (ids and idx exactly, boxes and filter states as in
make_botsort_golden.py, every live smooth_feat within the fp32-to-fp64 distance); the fp64 twin yields the same ids; every score, raw
IoU distance, e and final cost is more than 1e-3 from its threshold; with delta the largest difference of any cost entry between the
two runs, every assignment's optimum beats its runner-up by more than 100 * delta * (most matches in one assignment); each rule
counted at the end is exercised; on `cross` every object keeps one id, and the same detections without embeddings (BotSortNp) do
not.  If an assertion fails, change the seed.
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
import make_botsort_golden as MB  # noqa: E402
import bytetrack_np as T  # noqa: E402
import botsort_np as BS  # noqa: E402
import botsort_reid_np as R  # noqa: E402

CAP, D = 64, 16
CROWD_SEED, CROSS_SEED, GAPS_SEED = 2, 5, 1       # crowd 1 and 3, cross 2-4 put a cost within 1e-3 of a threshold
CFG = dict(M.CFG)
REID = dict(proximity_thresh=0.5, appearance_thresh=0.25)
ARGS = dict(CFG, gmc_method='sparseOptFlow', with_reid=True, **REID)


class PrescribedEncoder:
    """Stands where the reference would put a ReID model: inference(img, dets) -> the prescribed row of each detection index."""

    def __init__(self):
        self.rows, self.calls = None, 0

    def inference(self, img, dets):
        self.calls += 1
        return [np.array(self.rows[int(k)], np.float32) for k in dets[:, 4]]


def sequences():
    crowd, cw = R.make_scene(CROWD_SEED, n_obj=12, frames=90, p_low=0.15, fp_every=4, empty=(37,),
                             gaps=[(0, 20, 3), (1, 30, 8), (2, 25, 40), (3, 50, 3)])
    wp = BS.camera_path(CROWD_SEED, len(crowd))
    cross, xw = R.make_cross(CROSS_SEED)
    wx = np.tile(np.eye(2, 3), (len(cross), 1, 1))
    gp, gw = R.make_scene(GAPS_SEED, n_obj=6, frames=20, fp_every=5, p_low=0.1, empty=(0, 7, 8, 19))
    wg = BS.camera_path(GAPS_SEED, len(gp), pan=(-2.5, 1.0))
    return (('crowd', BS.through_camera(crowd, wp), wp, cw, R.object_features(CROWD_SEED, cw, 12, D)),
            ('cross', cross, wx, xw, R.object_features(CROSS_SEED, xw, 7, D)),
            ('gaps', BS.through_camera(gp, wg), wg, gw, R.object_features(GAPS_SEED, gw, 6, D)))


def ids_of_objects(rows_per_frame, who):
    """{object: set of the track ids its detections carried}, from the rows' idx column."""
    out = {}
    for rows, w in zip(rows_per_frame, who):
        for r in rows:
            o = int(w[int(r[7])])
            if o >= 0:
                out.setdefault(o, set()).add(int(r[4]))
    return out


def run(name, frames, warps, who, feats, tracker, d):
    twin = R.BotSortReidNp(D, capacity=CAP, want_margin=True, **REID, **CFG)
    twin64 = R.BotSortReidNp(D, capacity=CAP, dtype=np.float64, **REID, **CFG)
    tracker.gmc = MB.PrescribedGMC([w for fr, w in zip(frames, warps) if len(fr)])
    tracker.encoder = PrescribedEncoder()
    img = np.zeros((8, 8, 3), np.uint8)
    cnt, rcnt, det, box, ids, idxs, allrows = [], [], [], [], [], [], []
    ref_gap = bound = 0.0
    for f, (fr, w, ft) in enumerate(zip(frames, warps, feats)):
        rows = np.zeros((0, 8), np.float32)
        if len(fr):
            tracker.encoder.rows = ft
            rows = np.asarray(tracker.update(M.Boxes(fr), img=img), np.float32).reshape(-1, 8)
        mine, mine64 = twin.update(fr, w, ft), twin64.update(fr, w, ft)
        assert sorted(zip(rows[:, 4], rows[:, 7])) == sorted(zip(mine[:, 4], mine[:, 7])), (name, f, rows[:, [4, 7]], mine[:, [4, 7]])
        assert sorted(zip(mine64[:, 4], mine64[:, 7])) == sorted(zip(mine[:, 4], mine[:, 7])), (name, f, 'the fp64 features change an id')
        o1, o2 = np.argsort(rows[:, 4]), np.argsort(mine[:, 4])
        assert np.allclose(rows[o1, :4], mine[o2, :4], rtol=1e-6, atol=5e-4) and np.array_equal(rows[o1, 5:7], mine[o2, 5:7]), (name, f)
        M.same_live(M.ref_live(tracker), twin.live())
        lf, lf64 = twin.live_feat(), twin64.live_feat()
        assert set(lf) == set(lf64)
        for t in tracker.tracked_stracks + tracker.lost_stracks:
            assert t.smooth_feat.dtype == np.float32 and abs(float(np.linalg.norm(t.smooth_feat)) - 1) < 1e-6
            ref_gap = max(ref_gap, float(np.abs(t.smooth_feat - lf[int(t.track_id)]).max()))
        bound = max([bound] + [float(np.abs(lf[k] - lf64[k]).max()) for k in lf])
        k = rows[:, 7].astype(int)
        assert np.array_equal(rows[:, 5:7], fr[k, 4:6]), 'a row does not carry the score and class of detection idx'
        cnt.append(len(fr)); rcnt.append(len(rows)); det.append(fr); box.append(rows[:, :4]); ids.append(rows[:, 4]); idxs.append(rows[:, 7])
        allrows.append(rows)
    assert not tracker.gmc.warps and tracker.encoder.calls > 0
    assert ref_gap <= bound, (name, 'the reference smooth_feat is farther from the fp32 twin than the fp64 twin is', ref_gap, bound)
    assert len(twin.costs) == len(twin64.costs) and all(a.shape == b.shape for a, b in zip(twin.costs, twin64.costs))
    delta = max(float(np.abs(a - b).max()) for a, b in zip(twin.costs, twin64.costs) if a.size)
    need = 100 * delta * twin.max_matches
    det = np.concatenate(det)
    d[f'{name}_cnt'], d[f'{name}_det'], d[f'{name}_cls'] = np.array(cnt, np.int32), det[:, :5], det[:, 5].astype(np.uint8)
    d[f'{name}_rcnt'], d[f'{name}_box'] = np.array(rcnt, np.int32), np.concatenate(box)
    d[f'{name}_id'], d[f'{name}_idx'] = np.concatenate(ids).astype(np.int16), np.concatenate(idxs).astype(np.int16)
    d[f'{name}_warp'] = np.asarray(warps, np.float64)
    d[f'{name}_feat'] = np.concatenate(feats).astype(np.float16)
    assert np.array_equal(d[f'{name}_feat'].astype(np.float32), np.concatenate(feats)), 'the features are not fp16 values'
    d[f'{name}_obj'] = np.concatenate(who).astype(np.int8)
    live = M.ref_live(tracker)
    keys = sorted(live)
    sm = {int(t.track_id): t.smooth_feat for t in tracker.tracked_stracks + tracker.lost_stracks}
    d[f'{name}_fin_meta'] = np.array([(k,) + live[k][:6] for k in keys], np.int32).reshape(-1, 7)
    d[f'{name}_fin_sc'] = np.array([live[k][6:8] for k in keys], np.float32).reshape(-1, 2)
    d[f'{name}_fin_mean'] = np.array([live[k][8] for k in keys]).reshape(-1, 8)
    d[f'{name}_fin_cov'] = np.array([live[k][9] for k in keys]).reshape(-1, 8, 8)
    d[f'{name}_fin_feat'] = np.array([sm[k] for k in keys], np.float32).reshape(-1, D)
    print(f'{name}: {len(frames)} frames, {int(det.shape[0])} detections, {sum(rcnt)} rows, ids up to {int(twin.state["hdr"][T.H_NEXT]) - 1}\n'
          f'   margin {twin.margin:.3g} (needs > 100 * delta {delta:.3g} * matches {twin.max_matches} = {need:.3g}), threshold margin '
          f'{twin.thr_margin:.3g}\n   smooth_feat: reference to fp32 twin {ref_gap:.3g}, fp32 to fp64 twin {bound:.3g}\n   {twin.events}')
    assert delta > 0 and twin.margin > need, (name, 'an assignment is not unique enough: change the seed', twin.margin, need)
    assert min(twin.thr_margin, twin64.thr_margin) > 1e-3, (name, 'a score, distance or cost is too close to its threshold: change the seed',
                                                            twin.thr_margin, twin64.thr_margin)
    return twin.events, allrows, bound


def main():
    M.import_tracker()
    from ultralytics.trackers import bot_sort
    d, events, bound = {}, {}, 0.0
    for name, frames, warps, who, feats in sequences():
        tracker = bot_sort.BOTSORT(types.SimpleNamespace(**ARGS), frame_rate=30)
        assert tracker.encoder is None and tracker.kalman_filter.__class__.__name__ == 'KalmanFilterXYWH'
        ev, rows, b = run(name, frames, warps, who, feats, tracker, d)
        bound = max(bound, b)
        events = {k: (max if k == 'feat_updates_max' else lambda a, c: a + c)(events.get(k, 0), v) for k, v in ev.items()}
        if name == 'cross':      # every object keeps one id; the same detections without embeddings do not
            mine = ids_of_objects(rows, who)
            blind = BS.BotSortNp(capacity=CAP, **CFG)
            theirs = ids_of_objects([blind.update(fr) for fr in frames], who)
            print(f'   ids per object with ReID {sorted(len(v) for v in mine.values())}, IoU only {sorted(len(v) for v in theirs.values())}')
            assert all(len(v) == 1 for v in mine.values()), ('an id is lost at a crossing although the embeddings tell the objects apart', mine)
            assert any(len(v) > 1 for v in theirs.values()), ('IoU alone keeps every id: the crossing is too easy, change the seed', theirs)
    for k in ('emb_won', 'app_clipped', 'prox_masked', 'assign_differs', 'unconf_by_embedding', 'feat_match2', 'feat_reactivate', 'empty_frame',
              'match1', 'match2', 'refind', 'warped'):
        assert events[k] >= 1, ('the sequences never exercise', k, 'change the seed', events)
    assert events['feat_updates_max'] >= 10, events
    d['names'] = np.array(['crowd', 'cross', 'gaps'])
    d['capacity'], d['dim'], d['feat_bound'] = CAP, D, bound
    d['proximity_thresh'], d['appearance_thresh'] = REID['proximity_thresh'], REID['appearance_thresh']
    G.save('botsort_reid', d)
    assert os.path.getsize(os.path.join(HERE, 'botsort_reid.npz')) < 128 * 1024


if __name__ == '__main__':
    main()
