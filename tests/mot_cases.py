"""Cases of the MOT evaluation (csrc/mot.hip, engine.mot_evaluate), shared by test_mot_host.py and test_gpu_mot.py: hand-worked
sequences with their expected counts, literal() - the rule restated in plain Python loops with an exhaustive search in place of the
assignment solver - and a seeded generator of random sequences.

A sequence is a list of frames (gt f32 [m, 7] x1 y1 x2 y2 id cls kind, tracks f32 [k, 6] x1 y1 x2 y2 id cls); a case is a list of
sequences."""
import numpy as np

BOX_A, BOX_B, BOX_C = (0, 0, 10, 10), (50, 0, 60, 10), (100, 50, 110, 60)
COUNT_KEYS = ('TP', 'FN', 'FP', 'IDSW', 'gt_dets', 'trk_dets', 'Frag', 'MT', 'PT', 'ML', 'IDTP', 'gt_ids', 'drop_region', 'drop_distractor')


def G(box, gid, cls=0, kind=0):
    return [*box, gid, cls, kind]


def T(box, tid, cls=0):
    return [*box, tid, cls]


def frame(gt=(), trk=()):
    return np.asarray(gt, np.float32).reshape(-1, 7), np.asarray(trk, np.float32).reshape(-1, 6)


def device_rows(trk):
    """Track rows [k, 6] -> the tracker's 8 columns x1 y1 x2 y2 id score cls idx."""
    trk = np.asarray(trk, np.float32).reshape(-1, 6)
    out = np.zeros((len(trk), 8), np.float32)
    out[:, :5], out[:, 5], out[:, 6], out[:, 7] = trk[:, :5], 0.9, trk[:, 5], np.arange(len(trk))
    return out


# ------------------------------------------------------------------------------------------------ hand-worked cases
def _case_a():
    # gt 1 on BOX_A in six frames.  Frames 1, 2: track 1 on it (TP, IoU 1).  Frame 3: nothing (FN).  Frame 4: track 2 on it (TP, the
    # last-matched id 1 differs: IDSW; a new run after the gap: Frag 1).  Frame 5: track 2 again, and track 3 far away (FP).  Frame 6:
    # track 2 at (0, 0, 10, 20): inter 100, union 200, IoU exactly 0.5 qualifies (TP, + 0.5).  matched 5 of 6 = 0.83 > 0.8: MT.
    # pair[1, 1] = 2, pair[1, 2] = 3: IDTP 3, IDFN 6 - 3, IDFP 6 - 3.  MOTA = 1 - (1 + 1 + 1) / 6, MOTP = 4.5 / 5, IDF1 = 3 / (3 + 1.5 + 1.5).
    g = [G(BOX_A, 1)]
    return [[frame(g, [T(BOX_A, 1)]), frame(g, [T(BOX_A, 1)]), frame(g), frame(g, [T(BOX_A, 2)]),
             frame(g, [T(BOX_A, 2), T((100, 100, 110, 110), 3)]), frame(g, [T((0, 0, 10, 20), 2)])]]


def _case_b(first=True):
    # gt 1 (0, 0, 10, 10), gt 2 (4, 0, 14, 10).  Frame 1: tracks 1 and 2 exactly on them (gt 1 x track 2 has IoU 6 / 14: no pair).
    # Frame 2: track 1 (3, 0, 13, 10), track 2 (1, 0, 11, 10): keeping the ids gives 7/13 + 7/13, swapping gives 9/11 + 9/11 - the
    # larger sum - but the last-matched bonus keeps the ids.  All four pairs of frame 2 qualify: pair = [[2, 1], [1, 2]], IDTP 4.
    g = [G((0, 0, 10, 10), 1), G((4, 0, 14, 10), 2)]
    f1 = frame(g, [T((0, 0, 10, 10), 1), T((4, 0, 14, 10), 2)])
    f2 = frame(g, [T((3, 0, 13, 10), 1), T((1, 0, 11, 10), 2)])
    return [[f1, f2]] if first else [[f2]]


def _case_c():
    # One frame: gt 1 on BOX_A, a distractor, a region (100, 0, 200, 100).  Track 1 on the gt (TP); track 2 on the distractor (dropped
    # in step 2); track 3 inside the region (ioa 1: dropped in step 1); track 4 alone (FP); track 5 half inside the region (ioa
    # exactly 0.5 stays: FP).  trk_dets 3, IDTP 1, IDFP 2, MOTA = 1 - 2 / 1.
    gt = [G(BOX_A, 1), G((20, 0, 30, 10), 7, 0, 1), G((100, 0, 200, 100), 8, 0, 2)]
    trk = [T(BOX_A, 1), T((20, 0, 30, 10), 2), T((110, 10, 120, 20), 3), T((40, 0, 50, 10), 4), T((195, 0, 205, 10), 5)]
    return [[frame(gt, trk)]]


def _case_mt_pt():
    # gt 1: 10 frames, track 1 in the first 8: 8 / 10 is not > 0.8: PT.  gt 2: track 2 in the first 9: 0.9: MT.  No gap inside a run: Frag 0.
    return [[frame([G(BOX_A, 1), G(BOX_B, 2)], [T(BOX_A, 1)] * (f < 8) + [T(BOX_B, 2)] * (f < 9)) for f in range(10)]]


def _case_ml():
    # gt 1: 10 frames, matched in the fifth only: 0.1 < 0.2: ML.
    return [[frame([G(BOX_A, 1)], [T(BOX_A, 1)] * (f == 4)) for f in range(10)]]


def _case_absent():
    # gt 1 and track 1 in frames 1, 2, 4, 5; frame 3 has neither: two runs (Frag 1), the same id after the gap (no IDSW), 4 of 4: MT.
    on = frame([G(BOX_A, 1)], [T(BOX_A, 1)])
    return [[on, on, frame(), on, on]]


def _case_class_change():
    # nc 2.  gt 1 (class 0) on BOX_A and gt 2 (class 1) on BOX_B in four frames; track 7 is on BOX_A as class 0 in frames 1, 2 and on
    # BOX_B as class 1 in frames 3, 4: one identity per class, IDTP 2 in each (one identity over both classes would give 2 in all).
    g = [G(BOX_A, 1, 0), G(BOX_B, 2, 1)]
    return [[frame(g, [T(BOX_A, 7, 0)]), frame(g, [T(BOX_A, 7, 0)]), frame(g, [T(BOX_B, 7, 1)]), frame(g, [T(BOX_B, 7, 1)])]]


def _case_class_range():
    # nc 2, one frame.  gt 1 (class 0) on BOX_A with track 1 (class 0): TP.  gt 2 has class 5: out; track 2 (class 0) on it: FP.
    # Track 3 (class -1) on BOX_A: out.  gt 3 (class 1) on BOX_C with track 4 of class 2 (out) on it: FN.  A region of class 9 counts:
    # track 5 (class 1) inside it is dropped.
    gt = [G(BOX_A, 1, 0), G(BOX_B, 2, 5), G(BOX_C, 3, 1), G((300, 300, 400, 400), 4, 9, 2)]
    trk = [T(BOX_A, 1, 0), T(BOX_B, 2, 0), T(BOX_A, 3, -1), T(BOX_C, 4, 2), T((310, 310, 320, 320), 5, 1)]
    return [[frame(gt, trk)]]


def _case_no_gt():
    return [[frame([], [T(BOX_A, 1)]), frame([], [T(BOX_A, 1), T(BOX_B, 2)])]]


def _case_no_tracks():
    return [[frame([G(BOX_A, 1)]), frame([G(BOX_A, 1), G(BOX_B, 2)])]]


def _case_reuse():
    # Two sequences that both call their object 1: track 1 in the first, track 2 in the second.  Nothing carries over: no IDSW, and the
    # identity assignment is per sequence (2 + 2; one pair table over both would give 2).
    return [[frame([G(BOX_A, 1)], [T(BOX_A, 1)])] * 2, [frame([G(BOX_A, 1)], [T(BOX_A, 2)])] * 2]


def _all(**kw):
    return {'all': kw}


HAND = {
    'A': (_case_a(), 1, _all(TP=5, FN=1, FP=1, IDSW=1, Frag=1, MT=1, PT=0, ML=0, iou_sum=4.5, IDTP=3, IDFN=3, IDFP=3, MOTA=0.5, MOTP=0.9,
                             IDF1=0.5, gt_dets=6, trk_dets=6)),
    'B': (_case_b(), 1, _all(IDSW=0, TP=4, FN=0, FP=0, iou_sum=2 + 14 / 13, IDTP=4)),
    'B_frame2_alone': (_case_b(False), 1, _all(IDSW=0, TP=2, iou_sum=18 / 11, IDTP=2)),
    'C': (_case_c(), 1, _all(trk_dets=3, TP=1, FP=2, FN=0, IDFP=2, IDTP=1, MOTA=-1.0, drop_region=1, drop_distractor=1)),
    'mt_pt': (_case_mt_pt(), 1, _all(TP=17, FN=3, FP=0, MT=1, PT=1, ML=0, Frag=0, IDSW=0, IDTP=17, gt_dets=20, trk_dets=17, gt_ids=2)),
    'ml': (_case_ml(), 1, _all(TP=1, FN=9, MT=0, PT=0, ML=1, Frag=0, IDTP=1, MOTA=0.1)),
    'absent': (_case_absent(), 1, _all(TP=4, FN=0, FP=0, Frag=1, IDSW=0, MT=1, gt_dets=4, IDTP=4)),
    'class_change': (_case_class_change(), 2, {'all': dict(TP=4, FN=4, FP=0, IDTP=4, gt_dets=8, trk_dets=4),
                                               0: dict(TP=2, FN=2, IDTP=2, trk_dets=2, PT=1), 1: dict(TP=2, FN=2, IDTP=2, trk_dets=2, PT=1)}),
    'class_range': (_case_class_range(), 2, {'all': dict(TP=1, FP=1, FN=1, gt_dets=2, trk_dets=2, drop_region=1),
                                             0: dict(TP=1, FP=1, FN=0, gt_dets=1, trk_dets=2), 1: dict(TP=0, FP=0, FN=1, gt_dets=1, trk_dets=0, drop_region=1)}),
    'no_gt': (_case_no_gt(), 1, _all(TP=0, FN=0, FP=3, gt_dets=0, trk_dets=3, IDTP=0, IDFP=3, gt_ids=0)),
    'no_tracks': (_case_no_tracks(), 1, _all(TP=0, FN=3, FP=0, gt_dets=3, trk_dets=0, IDTP=0, IDFN=3, ML=2, MOTA=0.0, IDF1=0.0)),
    'two_sequences': (_case_a() + _case_c(), 1, _all(TP=6, FN=1, FP=3, IDSW=1, Frag=1, MT=2, iou_sum=5.5, IDTP=4, gt_dets=7, trk_dets=9)),
    'reuse': (_case_reuse(), 1, _all(TP=4, FN=0, FP=0, IDSW=0, IDTP=4, MT=2, gt_ids=2)),
}


# ------------------------------------------------------------------------------------------------ the rule in plain loops
def _iou(a, b):
    ax1, ay1, ax2, ay2 = (float(v) for v in a[:4])
    bx1, by1, bx2, by2 = (float(v) for v in b[:4])
    iw, ih = min(ax2, bx2) - max(ax1, bx1), min(ay2, by2) - max(ay1, by1)
    if iw <= 0 or ih <= 0:
        return 0.0, 0.0
    inter = iw * ih
    union = ((ax2 - ax1) * (ay2 - ay1) + (bx2 - bx1) * (by2 - by1)) - inter
    return (inter / union if union > 0 else 0.0), inter


def _best_matching(score):
    """Exhaustive search: the one-to-one matching of rows and columns with the largest total, over the pairs with a score > 0."""
    n = len(score)
    options = [[j for j, s in enumerate(row) if s > 0] for row in score]
    best = [-1.0, []]

    def walk(i, used, total, picked):
        if i == n:
            if total > best[0]:
                best[0], best[1] = total, list(picked)
            return
        walk(i + 1, used, total, picked)
        for j in options[i]:
            if j not in used:
                used.add(j)
                picked.append((i, j))
                walk(i + 1, used, total + score[i][j], picked)
                picked.pop()
                used.discard(j)

    walk(0, set(), 0.0, [])
    return best[1]


def literal(sequences, nc, iou=0.5):
    """The rule of csrc/mot.hip, step by step, one Python loop per sentence.  -> {key: list of nc numbers}."""
    out = {k: [0] * nc for k in COUNT_KEYS}
    out['iou_sum'] = [0.0] * nc
    for frames in sequences:
        last, present, matched, runs, prev_matched, pair = {}, {}, {}, {}, {}, {}
        for fid, (gt, trk) in enumerate(frames):
            gt = [[float(np.float32(v)) for v in r] for r in gt]
            trk = [[float(np.float32(v)) for v in r] for r in trk]
            trk = [t for t in trk if 0 <= t[5] < nc]
            kept = []
            for t in trk:                                        # 1. regions
                area = (t[2] - t[0]) * (t[3] - t[1])
                inside = any(area > 0 and _iou(t, r)[1] / area > 0.5 for r in gt if r[6] == 2)
                if inside:
                    out['drop_region'][int(t[5])] += 1
                else:
                    kept.append(t)
            trk = kept
            side = [g for g in gt if g[6] == 1 or (g[6] == 0 and 0 <= g[5] < nc)]
            score = [[_iou(g, t)[0] if _iou(g, t)[0] >= iou and (g[6] == 1 or int(g[5]) == int(t[5])) else 0.0 for t in trk] for g in side]
            gone = {j for i, j in _best_matching(score) if side[i][6] == 1}     # 2. distractors
            for j in gone:
                out['drop_distractor'][int(trk[j][5])] += 1
            trk = [t for j, t in enumerate(trk) if j not in gone]
            for c in range(nc):                                  # 3. and 4.
                gc = [g for g in side if g[6] == 0 and int(g[5]) == c]
                tc = [t for t in trk if int(t[5]) == c]
                score = []
                for g in gc:
                    key = (c, int(g[4]))
                    present[key] = present.get(key, 0) + 1
                    row = []
                    for t in tc:
                        v = _iou(g, t)[0]
                        if v >= iou:
                            pair[(key, int(t[4]))] = pair.get((key, int(t[4])), 0) + 1
                        row.append(0.0 if v < iou else v + 1000 if last.get(key) == int(t[4]) else v)
                    score.append(row)
                pairs = _best_matching(score)
                out['gt_dets'][c] += len(gc)
                out['trk_dets'][c] += len(tc)
                out['TP'][c] += len(pairs)
                out['FN'][c] += len(gc) - len(pairs)
                out['FP'][c] += len(tc) - len(pairs)
                for i, j in pairs:
                    key, tid = (c, int(gc[i][4])), int(tc[j][4])
                    out['iou_sum'][c] += _iou(gc[i], tc[j])[0]
                    if key in last and last[key] != tid:
                        out['IDSW'][c] += 1
                    last[key] = tid
                    matched[key] = matched.get(key, 0) + 1
                    if prev_matched.get(key) != fid - 1:
                        runs[key] = runs.get(key, 0) + 1
                    prev_matched[key] = fid
        for key, n in present.items():
            c, m = key[0], matched.get(key, 0)
            out['gt_ids'][c] += 1
            if m / n > 0.8:
                out['MT'][c] += 1
            elif m / n < 0.2:
                out['ML'][c] += 1
            else:
                out['PT'][c] += 1
            out['Frag'][c] += max(runs.get(key, 0) - 1, 0)
        for c in range(nc):
            gids = sorted({g for g, _ in pair if g[0] == c})
            tids = sorted({t for g, t in pair if g[0] == c})
            table = [[pair.get((g, t), 0) for t in tids] for g in gids]
            out['IDTP'][c] += sum(table[i][j] for i, j in _best_matching(table))
    return out


def same_counts(got, want, rtol, what=''):
    """Integer counts equal; iou_sum within rtol (relative)."""
    for k in COUNT_KEYS:
        assert [int(v) for v in got[k]] == [int(v) for v in want[k]], f'{what}: {k} {list(got[k])} != {list(want[k])}'
    for a, b in zip(got['iou_sum'], want['iou_sum']):
        assert abs(a - b) <= rtol * abs(b), f'{what}: iou_sum {a!r} vs {b!r}'


def check_expected(summary, expected, what=''):
    for key, want in expected.items():
        row = summary['all'] if key == 'all' else summary['per_class'][key]
        for k, v in want.items():
            assert row[k] == v if isinstance(v, int) else abs(row[k] - v) <= 1e-12, f'{what} [{key}]: {k} = {row[k]!r}, expected {v!r}'


# ------------------------------------------------------------------------------------------------ random sequences
SEEDS = (11, 12, 13)


def _distinct_scores(gt, trk, thr, what):
    """No two nonzero scores of a frame's assignments are equal: the qualifying IoUs of the frame are pairwise different (step 2's
    scores are these IoUs, step 3's are these IoUs, some plus 1000)."""
    v = [_iou(g, t)[0] for g in gt if g[6] != 2 for t in trk]
    v = [x for x in v if x >= thr]
    assert len(set(v)) == len(v), f'{what}: two equal qualifying IoUs'


def random_sequence(seed, frames=12, n_obj=6, nc=2, thr=0.5):
    """Objects move linearly; tracks are jittered copies of them with misses (a rate per object, so MT, PT and ML all occur), id
    changes, wrong classes and loose boxes; stray false positives; a distractor with a track on it; every third frame an ignored region
    with a track inside.  Coordinates come from continuous draws, so two matchings of equal total have probability zero."""
    rng = np.random.default_rng(seed)
    pos, vel = rng.uniform([50, 50], [500, 300], (n_obj, 2)), rng.uniform(-6, 6, (n_obj, 2))
    size, cls = rng.uniform(30, 70, (n_obj, 2)), rng.integers(0, nc, n_obj)
    miss = np.resize([0.0, 0.05, 0.5, 0.92, 0.25, 0.1], n_obj)
    tid, next_id = 10 + np.arange(n_obj), 100
    dpos, dvel = rng.uniform([600, 50], [800, 150], 2), rng.uniform(-3, 3, 2)
    out = []
    for f in range(frames):
        gt, trk = [], []
        for o in range(n_obj):
            if rng.random() < 0.1:
                continue
            p = pos[o] + vel[o] * f
            box = np.array([p[0], p[1], p[0] + size[o, 0], p[1] + size[o, 1]])
            gt.append([*box, o + 1, cls[o], 0])
            if rng.random() < 0.1:
                tid[o], next_id = next_id, next_id + 1
            if rng.random() < miss[o]:
                continue
            jit = rng.normal(0, 0.03, 4) * np.tile(size[o], 2) * (6 if rng.random() < 0.12 else 1)
            trk.append([*(box + jit), tid[o], cls[o] if rng.random() > 0.07 else (cls[o] + 1) % nc])
        if rng.random() < 0.4:
            p = rng.uniform([50, 400], [500, 500], 2)
            trk.append([p[0], p[1], p[0] + 40, p[1] + 50, 70 + f, rng.integers(0, nc)])
        d = dpos + dvel * f
        gt.append([d[0], d[1], d[0] + 50, d[1] + 40, 90, 0, 1])
        if rng.random() < 0.7:
            trk.append([*(np.array([d[0], d[1], d[0] + 50, d[1] + 40]) + rng.normal(0, 1.5, 4)), 50, rng.integers(0, nc)])
        if f % 3 == 0:
            gt.append([700, 400, 900, 580, 91, 0, 2])
            p = rng.uniform([710, 410], [820, 500], 2)
            trk.append([p[0], p[1], p[0] + 40, p[1] + 50, 60, rng.integers(0, nc)])
        order = rng.permutation(len(trk))
        fr = frame(gt, [trk[i] for i in order])
        _distinct_scores(fr[0], fr[1], thr, f'seed {seed} frame {f}')
        out.append(fr)
    return out


_RANDOM = {}


def random_cases():
    """{seed: (sequence, literal counts)} for SEEDS, computed once.  Asserts the condition on the set: every one of FN, FP, IDSW, Frag,
    MT, PT, ML, dropped-by-region and dropped-by-distractor is nonzero for some class of some seed."""
    if not _RANDOM:
        for s in SEEDS:
            seq = random_sequence(s)
            _RANDOM[s] = (seq, literal([seq], 2))
        for k in ('FN', 'FP', 'IDSW', 'Frag', 'MT', 'PT', 'ML', 'drop_region', 'drop_distractor'):
            assert any(v > 0 for _, (_, c) in _RANDOM.items() for v in c[k]), f'no seed of {SEEDS} produces a nonzero {k}'
    return _RANDOM


def crowded_sequence(frames=4, nc=3, seed=5):
    """A frame wider than a wavefront everywhere: 65 objects on a grid plus 6 distractors and a region = 72 ground-truth rows; 65
    jittered tracks plus strays = 70 rows, 72 in the last frame; gt ids from 100 and track ids from 200 (all above 64); some tracks
    trade ids from frame to frame."""
    rng = np.random.default_rng(seed)
    gx, gy = np.meshgrid(np.arange(13) * 70.0, np.arange(5) * 80.0)
    base = np.stack([gx.ravel() + 5, gy.ravel() + 5, gx.ravel() + 55, gy.ravel() + 65], 1)
    cls = rng.integers(0, nc, 65)
    tid = 200 + np.arange(65)
    out = []
    for f in range(frames):
        box = base + rng.normal(0, 1.0, (65, 4)) + 2.0 * f
        gt = [[*box[o], 100 + o, cls[o], 0] for o in range(65)]
        gt += [[1000 + 60 * k, 20, 1050 + 60 * k, 70, 300 + k, 0, 1] for k in range(6)]
        gt.append([1000, 200, 1300, 400, 310, 0, 2])
        if f:
            a, b = rng.choice(65, 2, replace=False)
            tid[a], tid[b] = tid[b], tid[a]
        keep = rng.random(65) > 0.08 if f < frames - 1 else np.ones(65, bool)
        trk = [[*(box[o] + rng.normal(0, 2.5, 4)), tid[o], cls[o]] for o in range(65) if keep[o]]
        for k in range(3):
            trk.append([*(np.array([1000 + 60 * k, 20, 1050 + 60 * k, 70]) + rng.normal(0, 1.0, 4)), 400 + k, rng.integers(0, nc)])
        trk.append([1100 + rng.uniform(0, 20), 250, 1150, 300 + rng.uniform(0, 20), 410, 1])
        while len(trk) < (72 if f == frames - 1 else 70):
            p = rng.uniform([0, 450], [900, 600], 2)
            trk.append([p[0], p[1], p[0] + 30, p[1] + 30, 420 + len(trk), rng.integers(0, nc)])
        fr = frame(gt, [trk[i] for i in rng.permutation(len(trk))])
        _distinct_scores(fr[0], fr[1], 0.5, f'crowded frame {f}')
        out.append(fr)
    return out


def cluster_sequence(frames=3, n=70, seed=6):
    """One connected component wider than a wavefront: 70 ground truths and 70 tracks, all jittered copies of one box, so every pair
    qualifies and the whole 70 x 70 problem reaches the assignment solver (nothing is an isolated pair); ids persist from frame to
    frame, so from the second frame on the last-matched bonus is in every row."""
    rng = np.random.default_rng(seed)
    base = np.array([100.0, 100.0, 220.0, 220.0])
    out = []
    for f in range(frames):
        gt = [[*(base + rng.uniform(-6, 6, 4)), 100 + i, 0, 0] for i in range(n)]
        trk = [[*(base + rng.uniform(-6, 6, 4)), 200 + i, 0] for i in range(n)]
        fr = frame(gt, [trk[i] for i in rng.permutation(n)])
        _distinct_scores(fr[0], fr[1], 0.5, f'cluster frame {f}')
        assert min(_iou(g, t)[0] for g in fr[0] for t in fr[1]) >= 0.5
        out.append(fr)
    return out
