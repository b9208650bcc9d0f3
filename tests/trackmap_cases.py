"""Cases of track-mAP (csrc/trackmap.hip, engine.track_map_evaluate), shared by test_trackmap_host.py and test_gpu_trackmap.py:
hand-worked sequences with their expected rows and AP written as literals, the seeded sequences of mot_cases with a score per row, a
sequence of 300 track identities, and margins() - how far a case is from any decision that the last bits could flip.

A sequence is a list of frames (gt f32 [m, 7] x1 y1 x2 y2 id cls kind, tracks f32 [k, 7] x1 y1 x2 y2 id cls score); a case is a list of
sequences.  Thresholds are the default (0.25, 0.5, 0.75) throughout; bit a of a row = matched at threshold a."""
import numpy as np

import mot_cases as MC

THRESHOLDS = (0.25, 0.5, 0.75)
G = MC.G


def B(i, dx=0.0):
    """The i-th of a row of isolated 40 x 40 boxes, moved right by dx."""
    return (60.0 * i + dx, 0.0, 60.0 * i + 40.0 + dx, 40.0)


def T(box, tid, score, cls=0):
    return [*box, tid, cls, score]


def frame(gt=(), trk=()):
    return np.asarray(gt, np.float32).reshape(-1, 7), np.asarray(trk, np.float32).reshape(-1, 7)


def f32(x):
    return float(np.float32(x))


def with_scores(seq, seed):
    """mot_cases frames (tracks [k, 6]) with a seeded score per track row in [0.05, 1)."""
    rng = np.random.default_rng(seed)
    return [(g, np.concatenate([t, rng.uniform(0.05, 1.0, (len(t), 1)).astype(np.float32)], 1)) for g, t in seq]


def device_rows(trk):
    """Track rows [k, 7] (or [k, 6]: score 1) -> the tracker's 8 columns x1 y1 x2 y2 id score cls idx."""
    trk = np.asarray(trk, np.float32)
    trk = trk.reshape(-1, 7 if trk.ndim == 2 and trk.shape[1] == 7 else 6)
    out = np.zeros((len(trk), 8), np.float32)
    out[:, :5], out[:, 5], out[:, 6], out[:, 7] = trk[:, :5], trk[:, 6] if trk.shape[1] == 7 else 1.0, trk[:, 5], np.arange(len(trk))
    return out


# ------------------------------------------------------------------------------------------------ hand-worked cases
def _exact():
    # gt 1 and 2 on their boxes in three frames, tracks 1 and 2 exactly on them: IoU 1, matched at every threshold.
    return [[frame([G(B(0), 1), G(B(1), 2)], [T(B(0), 1, 0.9), T(B(1), 2, 0.8)])] * 3]


def _half():
    # gt 1 in four frames, track 1 exactly on it in the first two: inter 2 A, areas 4 A and 2 A: IoU = 2 / (6 - 2) = 0.5 exactly.
    g = [G(B(0), 1)]
    return [[frame(g, [T(B(0), 1, 0.9)])] * 2 + [frame(g)] * 2]


def _offset():
    # track 1 is gt 1 moved by half its width in both frames: inter 800 n, areas 1600 n each: IoU = 800 / 2400 = 1 / 3.
    return [[frame([G(B(0), 1)], [T(B(0, 20), 1, 0.9)])] * 2]


def _false_first():
    # track 2 (score 0.9) is nowhere near a ground truth, track 1 (0.5) is exactly on gt 1: rows fp, tp.  precision 0, 1 / 2; the
    # envelope is 1 / 2 everywhere: AP 0.5.
    return [[frame([G(B(0), 1)], [T(B(0), 1, 0.5), T(B(3), 2, 0.9)])] * 2]


def _greedy():
    # One frame, x ranges on a common y range: g1 = [50, 125], g2 = [0, 100], track A (0.9) = [0, 125], track B (0.6) = [-10, 49].
    # IoU(g1, A) = 75 / 125 = 0.6, IoU(g2, A) = 100 / 125 = 0.8, IoU(g2, B) = 49 / 110 = 0.445, B does not touch g1.  An assignment
    # would give A g1 and B g2; the protocol is greedy: A takes g2, its best, and B stays unmatched.  Rows tp, fp with 2 ground truths:
    # recall 0.5, 0.5, envelope 1, 0.5: the 51 recall points up to 0.5 read 1: AP 51 / 101.
    gt = [G((50, 0, 125, 40), 1), G((0, 0, 100, 40), 2)]
    return [[frame(gt, [T((-10, 0, 49, 40), 2, 0.6), T((0, 0, 125, 40), 1, 0.9)])]]


def _two_halves():
    # gt 1 in four frames; track 1 (0.9) on it in frames 1, 2 and track 2 (0.6) in frames 3, 4: IoU 0.5 each.  Track 1 takes the
    # ground truth at 0.25 and 0.5, track 2 is a false positive behind it: AP 1, 1, 0.
    g = [G(B(0), 1)]
    return [[frame(g, [T(B(0), 1, 0.9)])] * 2 + [frame(g, [T(B(0), 2, 0.6)])] * 2]


def _equal_iou():
    # One frame: g1 = [0, 40], g2 = [60, 100]; track 1 (0.9) = [20, 80] meets each on 20: IoU 800 / 3200 = 0.25 with both, exactly.
    # The later dense row, g2, wins the tie.  Track 2 (0.5) is exactly g2: at 0.25 its ground truth is taken (bits 110); had g1 won
    # it would read 111.
    return [[frame([G(B(0), 1), G(B(1), 2)], [T((20, 0, 80, 40), 1, 0.9), T(B(1), 2, 0.5)])]]


def _equal_score():
    # One frame: tracks 5 (exactly gt 1) and 3 (moved by half: IoU 1 / 3) both have score 0.7: the lower id, 3, goes first and takes
    # the ground truth at 0.25 (bits 001); track 5 gets it at 0.5 and 0.75 only (110).  Had 5 gone first the rows would read 111, 000.
    return [[frame([G(B(0), 1)], [T(B(0), 5, 0.7), T(B(0, 20), 3, 0.7)])]]


def _shortened():
    # gt 1 in four frames.  Track 1 is on it in frames 1, 2 (score 0.8); in frame 3 it lies inside an ignored region and in frame 4 on
    # a distractor (score 0.2): both rows are dropped, so its sums hold two frames: IoU = 2 / (4 + 2 - 2) = 0.5 and score 0.8 (four
    # frames would give 2 / (4 + 4 - 2) = 1 / 3 and 0.5).
    g = G(B(0), 1)
    return [[frame([g], [T(B(0), 1, 0.8)])] * 2 +
            [frame([g, G((300, 300, 500, 500), 8, 0, 2)], [T((320, 320, 360, 360), 1, 0.2)]),
             frame([g, G(B(5), 9, 0, 1)], [T(B(5), 1, 0.2)])]]


def _no_tracks_class():
    # nc 2: class 0 has gt 1 with its exact track; class 1 has gt 2 and no track: AP 0, and the mean over both classes is 0.5.
    return [[frame([G(B(0), 1, 0), G(B(1), 2, 1)], [T(B(0), 1, 0.9, 0)])] * 2]


def _no_gt_class():
    # nc 2: class 1 has a track and no ground truth: -1 throughout, left out of the `all` row.
    return [[frame([G(B(0), 1, 0)], [T(B(0), 1, 0.9, 0), T(B(2), 2, 0.8, 1)])] * 2]


def _class_change():
    # mot_cases' class change with scores: track 7 is class 0 on gt 1 in frames 1, 2 and class 1 on gt 2 in frames 3, 4: two
    # identities, each with IoU 2 / (4 + 2 - 2) = 0.5 (one identity over both classes would have IoU 2 / (4 + 4 - 2) = 1 / 3).
    g = [G(B(0), 1, 0), G(B(1), 2, 1)]
    return [[frame(g, [T(B(0), 7, 0.9, 0)])] * 2 + [frame(g, [T(B(1), 7, 0.6, 1)])] * 2]


def _interleaved():
    # Two sequences that both use gt ids 1, 2 and track ids 1, 2.  First: track 1 (0.9) on gt 1, track 2 (0.3) on nothing, gt 2 missed.
    # Second: track 1 (0.6) on gt 1, track 2 (0.5) on gt 2.  The run's order is 0.9 (first), 0.6, 0.5 (second), 0.3 (first): tp tp tp fp
    # with 4 ground truths: recall 0.25, 0.5, 0.75, 0.75, envelope 1, 1, 1, 0.75: the 76 recall points up to 0.75 read 1: AP 76 / 101.
    g = [G(B(0), 1), G(B(1), 2)]
    return [[frame(g, [T(B(0), 1, 0.9), T(B(3), 2, 0.3)])] * 2, [frame(g, [T(B(0), 1, 0.6), T(B(1), 2, 0.5)])] * 2]


def _rows(score, cls, bits, gt_tracks):
    return dict(score=[f32(s) for s in score], cls=cls, bits=bits, gt_tracks=gt_tracks)


# name: (sequences, nc, the run's rows, {row key: AP_thr}, {row key: AR_thr}); the `all` AP is the mean of AP_thr
HAND = {
    'exact': (_exact(), 1, _rows([0.9, 0.8], [0, 0], [7, 7], [2]), {'all': [1, 1, 1]}, {'all': [1, 1, 1]}),
    'half': (_half(), 1, _rows([0.9], [0], [3], [1]), {'all': [1, 1, 0]}, {'all': [1, 1, 0]}),
    'offset': (_offset(), 1, _rows([0.9], [0], [1], [1]), {'all': [1, 0, 0]}, {'all': [1, 0, 0]}),
    'false_first': (_false_first(), 1, _rows([0.9, 0.5], [0, 0], [0, 7], [1]), {'all': [0.5, 0.5, 0.5]}, {'all': [1, 1, 1]}),
    'greedy': (_greedy(), 1, _rows([0.9, 0.6], [0, 0], [7, 0], [2]), {'all': [51 / 101] * 3}, {'all': [0.5] * 3}),
    'two_halves': (_two_halves(), 1, _rows([0.9, 0.6], [0, 0], [3, 0], [1]), {'all': [1, 1, 0]}, {'all': [1, 1, 0]}),
    'equal_iou': (_equal_iou(), 1, _rows([0.9, 0.5], [0, 0], [1, 6], [2]), {'all': [51 / 101, 25.5 / 101, 25.5 / 101]}, {'all': [0.5] * 3}),
    'equal_score': (_equal_score(), 1, _rows([0.7, 0.7], [0, 0], [1, 6], [1]), {'all': [1, 0.5, 0.5]}, {'all': [1, 1, 1]}),
    'shortened': (_shortened(), 1, _rows([0.8], [0], [3], [1]), {'all': [1, 1, 0]}, {'all': [1, 1, 0]}),
    'no_tracks_class': (_no_tracks_class(), 2, _rows([0.9], [0], [7], [1, 1]), {'all': [0.5] * 3, 0: [1] * 3, 1: [0] * 3},
                        {'all': [0.5] * 3, 1: [0] * 3}),
    'no_gt_class': (_no_gt_class(), 2, _rows([0.9, 0.8], [0, 1], [7, 0], [1, 0]), {'all': [1] * 3, 0: [1] * 3, 1: [-1] * 3},
                    {'all': [1] * 3, 1: [-1] * 3}),
    'class_change': (_class_change(), 2, _rows([0.9, 0.6], [0, 1], [3, 3], [1, 1]), {'all': [1, 1, 0], 0: [1, 1, 0], 1: [1, 1, 0]},
                     {'all': [1, 1, 0]}),
    'interleaved': (_interleaved(), 1, _rows([0.9, 0.3, 0.6, 0.5], [0] * 4, [7, 0, 7, 7], [4]), {'all': [76 / 101] * 3}, {'all': [0.75] * 3}),
}
# the pair IoUs that hit a threshold exactly, by hand: left out of margins()' first value
EXACT_HITS = {'half': (0.5,), 'two_halves': (0.5,), 'equal_iou': (0.25,), 'shortened': (0.5,), 'class_change': (0.5,)}
# the cases that are about a tie: margins() does not apply
TIES = ('equal_iou', 'equal_score')


def check_expected(counts, summary, name):
    """The run's rows and the summary against HAND[name]'s literals (AP and AR within 1e-12: precision carries COCO's eps)."""
    _, nc, rows, ap, ar = HAND[name]
    assert counts['score'].tolist() == rows['score'], f'{name}: scores {counts["score"].tolist()} != {rows["score"]}'
    for k in ('cls', 'bits', 'gt_tracks'):
        assert [int(v) for v in counts[k]] == rows[k], f'{name}: {k} {list(counts[k])} != {rows[k]}'
    for what, want in (('AP_thr', ap), ('AR_thr', ar)):
        for key, vals in want.items():
            row = summary['all'] if key == 'all' else summary['per_class'][key]
            assert np.allclose(row[what], vals, rtol=0, atol=1e-12), f'{name} [{key}]: {what} {row[what]} != {vals}'
    assert abs(summary['all']['AP'] - float(np.mean(ap['all']))) <= 1e-12, f'{name}: AP {summary["all"]["AP"]}'
    assert summary['all']['gt_tracks'] == sum(rows['gt_tracks']) and summary['all']['tracks'] == len(rows['bits'])
    assert [r['tracks'] for r in summary['per_class']] == [rows['cls'].count(c) for c in range(nc)]


# ------------------------------------------------------------------------------------------------ seeded sequences
def many_tracks(n=100, frames=3, seed=9):
    """`frames` frames of n isolated boxes; gt i stays, the track on it has a fresh id in every frame: frames * n track identities in one
    class, each with IoU A / (frames A + A - A) = 1 / frames with its ground truth, and a seeded score."""
    rng = np.random.default_rng(seed)
    score = rng.uniform(0.05, 1.0, (frames, n))
    return [frame([G(B(i), 1 + i) for i in range(n)], [T(B(i), 1 + f * n + i, score[f, i]) for i in rng.permutation(n)]) for f in range(frames)]


_SEEDED = {}


def seeded_cases():
    """{name: (sequences, nc)}: mot_cases' three random sequences, the crowded and the cluster sequence, each with seeded scores, and
    many_tracks; made once."""
    if not _SEEDED:
        for s in MC.SEEDS:
            _SEEDED[f'seed{s}'] = ([with_scores(MC.random_cases()[s][0], 100 + s)], 2)
        _SEEDED['crowded'] = ([with_scores(MC.crowded_sequence(), 21)], 3)
        _SEEDED['cluster'] = ([with_scores(MC.cluster_sequence(), 22)], 1)
        _SEEDED['many_tracks'] = ([many_tracks()], 1)
    return _SEEDED


def margins(sequences, nc, exact=(), thresholds=THRESHOLDS):
    """(the smallest distance of any pair IoU from any threshold, the IoUs listed in `exact` left out; the smallest gap between the best
    and the second-best candidate at any greedy step; the smallest gap between two mean scores of a class), inf where there is none."""
    from tamtr_amd.engine import track_map_evaluate
    detail = []
    track_map_evaluate(sequences, nc, thresholds=thresholds, detail=detail)
    d_thr = d_cand = d_score = float('inf')
    for d in detail:
        for v in d['iou'].values():
            if v not in exact:
                d_thr = min([d_thr] + [abs(v - t) for t in thresholds])
        d_cand = min([d_cand] + d['gaps'])
        for c in range(nc):
            s = np.sort([m for t, m in d['mean'].items() if t[0] == c])
            if len(s) > 1:
                d_score = min(d_score, float(np.diff(s).min()))
    return d_thr, d_cand, d_score
