"""GPU: the frame filter the three tracking evaluators share (mot_frame_filter, csrc/mot_rule.h) seen through all three at once: on
the same frames MotEvaluator, HotaEvaluator and TrackMapEvaluator count the same surviving rows, those engine._mot_preprocess keeps,
and the same rows beyond a capacity.  All counts are integers and are equal."""
import numpy as np
import pytest
import torch

import mot_cases as MC

pytestmark = pytest.mark.gpu
NC, NQ, NG = 2, 80, 80


def _box(k, shift=0):
    x, y = 30 * (k % 10) + shift, 30 * (k // 10)
    return (x, y, x + 20, y + 20)


def _frames(extra_tracks=0):
    """Frame 0: 70 objects (classes alternate) each with a track 1 to 3 px aside (IoU >= 0.73, no other overlap), a region with two
    tracks inside, a distractor with a track on it, a ground truth and a track of class 5; `extra_tracks` more tracks far away at the
    end.  Frame 1: nothing.  Frame 2: the first three objects and their tracks and a lone track; no distractor."""
    gt = [MC.G(_box(k), 1 + k, k % 2) for k in range(70)]
    trk = [MC.T(_box(k, 1 + k % 3), 1 + k, k % 2) for k in range(70)]
    gt += [MC.G((1000, 0, 1200, 200), 90, 0, 2), MC.G((1000, 300, 1020, 320), 91, 0, 1), MC.G((1000, 400, 1020, 420), 92, 5)]
    trk += [MC.T((1010, 10, 1030, 30), 71, 0), MC.T((1100, 100, 1120, 120), 72, 1), MC.T((1001, 300, 1021, 320), 73, 1),
            MC.T((1000, 400, 1020, 420), 74, 5)]
    trk += [MC.T((2000 + 30 * i, 0, 2020 + 30 * i, 20), 75 + i, 0) for i in range(extra_tracks)]
    return [MC.frame(gt, trk), MC.frame(), MC.frame(gt[:3], trk[:3] + [MC.T((500, 500, 520, 520), 80, 1)])]


def _pack(frames):
    """Track rows as the tracker leaves them, [B, NQ, 8]; a frame with more than NQ rows keeps its count."""
    rows = np.zeros((len(frames), NQ, 8), np.float32)
    for b, (_, t) in enumerate(frames):
        rows[b, :min(len(t), NQ)] = MC.device_rows(t)[:NQ]
    return torch.from_numpy(rows).cuda(), torch.tensor([len(t) for _, t in frames], dtype=torch.int32).cuda()


def _evaluators(G, T):
    from tamtr_amd.track import HotaEvaluator, MotEvaluator, TrackMapEvaluator
    kw = dict(gt_capacity=G, track_capacity=T, nq=NQ, ng=NG)
    return (MotEvaluator('cuda', NC, **kw), HotaEvaluator('cuda', NC, pair_capacity=1 << 10, log_capacity=1 << 12, frame_capacity=8, **kw),
            TrackMapEvaluator('cuda', NC, pair_capacity=1 << 10, row_capacity=256, **kw))


def _run(frames, G, T):
    """All three on the frames in one launch each -> the evaluators, track-mAP's per-class sums before its end of the sequence, and the
    three (over gt, over track, over rows) triples."""
    evs = _evaluators(G, T)
    tracks, tc = _pack(frames)
    for ev in evs:
        ev.update(tracks, tc, [g for g, _ in frames])
    st = {k: v.cpu().numpy() for k, v in evs[2].state.items()}
    tm_trk = st['tframes'].sum(1)
    tm_gt = np.bincount(st['gstate'][:, 1][st['gstate'][:, 0] > 0] - 1, weights=st['gstate'][:, 0][st['gstate'][:, 0] > 0], minlength=NC)
    for ev in evs:
        ev.end_sequence()
    over = [ev.state['hdr'].cpu().numpy()[o:o + 3].tolist() for ev, o in zip(evs, (1, 2, 2))]
    return evs, tm_gt.astype(np.int64), tm_trk.astype(np.int64), over


def test_the_three_evaluators_see_the_same_rows():
    from tamtr_amd.engine import _mot_preprocess
    frames = _frames()
    assert len(frames[0][0]) == 73 and len(frames[0][1]) == 74          # beyond a wave's 64 lanes on both sides
    host = {'drop_region': np.zeros(NC, np.int64), 'drop_distractor': np.zeros(NC, np.int64)}
    gt_dets, trk_dets = np.zeros(NC, np.int64), np.zeros(NC, np.int64)
    for g, t in frames:
        _, gcls, _, tcls = _mot_preprocess(g, t, NC, 0.5, host)
        gt_dets += np.bincount(gcls, minlength=NC)
        trk_dets += np.bincount(tcls, minlength=NC)
    assert gt_dets.tolist() == [37, 36] and trk_dets.tolist() == [37, 37]  # 35 + 35 of frame 0; 2 + 1 and 2 + 2 of frame 2
    assert host['drop_region'].tolist() == [1, 1] and host['drop_distractor'].tolist() == [0, 1]
    (mot, hota, tmap), tm_gt, tm_trk, over = _run(frames, 128, 128)
    assert over == [[0, 0, 0]] * 3
    m, h = mot.counts(), hota.counts()
    tmap.counts()
    for name, got in (('mot', m), ('hota', h), ('track-mAP', {'gt_dets': tm_gt, 'trk_dets': tm_trk})):
        assert got['gt_dets'].tolist() == gt_dets.tolist() and got['trk_dets'].tolist() == trk_dets.tolist(), name
    assert m['drop_region'].tolist() == host['drop_region'].tolist() and m['drop_distractor'].tolist() == host['drop_distractor'].tolist()


def test_the_three_evaluators_leave_out_the_same_rows():
    """gt_capacity 64 for 70 identities, track_capacity 32 for ids up to 80, 82 track rows for nq = 80."""
    from tamtr_amd.track import HotaOverflow, MotOverflow, TrackMapOverflow
    G, T = 64, 32
    frames = _frames(extra_tracks=8)
    assert len(frames[0][1]) == 82
    # by counting: the dense rows 64 .. 69 of frame 0 (frame 2 uses rows 0 .. 2 again); of the 80 rows that fit, those with a class in
    # range and an id of 32 or more, which are counted before the region is looked at; 2 rows beyond nq
    over_trk = sum(int(((t[:NQ, 5] >= 0) & (t[:NQ, 5] < NC) & (t[:NQ, 4] >= T)).sum()) for _, t in frames)
    assert over_trk == (70 - 31) + 3 + 6 + 1
    want = [6, over_trk, 2]
    evs, _, _, over = _run(frames, G, T)                                  # nothing raises up to here
    assert over == [want] * 3
    for ev, exc in zip(evs, (MotOverflow, HotaOverflow, TrackMapOverflow)):
        with pytest.raises(exc):
            ev.counts()
