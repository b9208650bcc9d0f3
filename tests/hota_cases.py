"""Cases of the HOTA evaluation (csrc/hota.hip, engine.hota_evaluate), shared by test_hota_host.py and test_gpu_hota.py: hand-worked
sequences with their expected values (worked on paper, written as literals), literal() - the rule restated in plain Python loops with
an exhaustive search in place of the assignment solver - and unique_optimum(), the condition under which device and numpy must pick
the same matching.  Sequences are those of mot_cases: a list of frames (gt f32 [m, 7], tracks f32 [k, 6])."""
import math

import numpy as np

import mot_cases as M
from mot_cases import BOX_A, BOX_B, G, T, frame

NA = 19
ALPHA = [float(a) for a in np.arange(0.05, 0.99, 0.05)]     # never k / 20: several differ in the last bit
EPS = float(np.finfo(float).eps)
INT_KEYS, SUM_KEYS = ('TP', 'FN', 'FP'), ('loc_sum', 'ass_sum', 'assre_sum', 'asspr_sum')
RATIOS = ('HOTA', 'DetA', 'AssA', 'DetRe', 'DetPr', 'AssRe', 'AssPr', 'LocA')


def upto(k, a, b):
    """A 19-vector: a at the first k thresholds (alpha <= 0.05 k), b above."""
    return [a] * k + [b] * (NA - k)


# ------------------------------------------------------------------------------------------------ hand-worked cases
def _case_perfect():
    # Two objects, two tracks exactly on them, three frames: every pair has S = 1, sim_iou = 1, pot = 3, gas = 3 / (3 + 3 - 3) = 1.
    g, t = [G(BOX_A, 1), G(BOX_B, 2)], [T(BOX_A, 5), T(BOX_B, 6)]
    return [[frame(g, t)] * 3]


def _case_id_switch():
    # One object, four frames, exact boxes; track 1 in frames 1, 2 and track 2 in frames 3, 4.  Every frame is a TP at every threshold:
    # TP 4, DetA 1.  Pair (g, 1): matched 2, gcount 4, tcount 2: 2 * 2 / (4 + 2 - 2) = 1; pair (g, 2) likewise: ass_sum 2, AssA 2 / 4.
    # assre_sum = 2 * (4 / 4) = 2: AssRe 0.5; asspr_sum = 2 * (4 / 2) = 4: AssPr 1.  HOTA = sqrt(1 * 0.5).
    g = [G(BOX_A, 1)]
    return [[frame(g, [T(BOX_A, 1)])] * 2 + [frame(g, [T(BOX_A, 2)])] * 2]


def _case_alignment():
    # One object on (0, 0, 10, 10), four frames.  Track 1 is exactly on it in frames 1 - 3.  Frame 4: track 1 at (0, 0, 10, 6), IoU 0.6,
    # and a new track 2 at (0, 0, 10, 9), IoU 0.9.
    # Pass 1.  Frames 1 - 3: sim_iou = 1 / (1 + 1 - 1) = 1.  Frame 4: rowsum 1.5; track 1: 0.6 / (1.5 + 0.6 - 0.6) = 0.4; track 2:
    # 0.9 / (1.5 + 0.9 - 0.9) = 0.6.  pot = 3.4 and 0.6; gcount 4, tcount 4 and 1.  gas = 3.4 / (8 - 3.4) = 0.739, 0.6 / (5 - 0.6) = 0.136.
    # Pass 2, frame 4: scores 0.739 * 0.6 = 0.443 for track 1 and 0.136 * 0.9 = 0.123 for track 2: track 1 is matched although track 2
    # fits the box better.  S = 0.6 passes the thresholds up to 0.6 (12 of them): TP 4 there and 3 above.  Matching on IoU alone takes
    # track 2 and has TP 4 up to 0.9 (18 thresholds).
    # trk_dets 5.  Up to 0.6: FN 0, FP 1, DetA 4 / 5; pair (g, 1) matched 4: 16 / (4 + 4 - 4) = 4, AssA 4 / 4 = 1.  Above: TP 3, FN 1, FP 2,
    # DetA 3 / 6; 9 / (4 + 4 - 3) = 1.8, AssA 1.8 / 3 = 0.6.  loc_sum 3.6 and 3.
    g = [G((0, 0, 10, 10), 1)]
    return [[frame(g, [T((0, 0, 10, 10), 1)])] * 3 + [frame(g, [T((0, 0, 10, 6), 1), T((0, 0, 10, 9), 2)])]]


def _case_low_iou():
    # One frame: (0, 0, 10, 10) against (0, 0, 8, 4): IoU 32 / 100, below the 0.5 of CLEAR but a TP at the 6 thresholds up to 0.30.
    return [[frame([G((0, 0, 10, 10), 1)], [T((0, 0, 8, 4), 1)])]]


def _case_exact():
    # One frame.  (0, 0, 10, 10) against (0, 0, 5, 5): IoU exactly 0.25, a TP up to 0.25 (5 thresholds).  (100, 0, 110, 10) against
    # (100, 0, 110, 5): exactly 0.5, a TP up to 0.5 (10 thresholds) - alpha - eps is what lets each pass its own threshold.
    return [[frame([G((0, 0, 10, 10), 1), G((100, 0, 110, 10), 2)], [T((0, 0, 5, 5), 1), T((100, 0, 110, 5), 2)])]]


ONE, ZERO = [1.0] * NA, [0.0] * NA
_perfect = dict(DetA_alpha=ONE, AssA_alpha=ONE, HOTA_alpha=ONE, LocA_alpha=ONE, DetRe_alpha=ONE, DetPr_alpha=ONE, AssRe_alpha=ONE, AssPr_alpha=ONE)

# name -> (sequences, nc, {row: {key: value}}): row 'all' or a class; a list is compared entry by entry, a float within 1e-12
HAND = {
    'perfect': (_case_perfect(), 1, {'all': dict(TP=[6] * NA, FN=[0] * NA, FP=[0] * NA, gt_dets=6, trk_dets=6, HOTA=1.0, **_perfect,
                                                 **{'HOTA(0)': 1.0, 'LocA(0)': 1.0, 'HOTALocA(0)': 1.0})}),
    'id_switch': (_case_id_switch(), 1, {'all': dict(TP=[4] * NA, DetA_alpha=ONE, AssA_alpha=[0.5] * NA, AssRe_alpha=[0.5] * NA, AssPr_alpha=ONE,
                                                     HOTA_alpha=[math.sqrt(0.5)] * NA, HOTA=math.sqrt(0.5), LocA_alpha=ONE)}),
    'alignment': (_case_alignment(), 1, {'all': dict(TP=upto(12, 4, 3), FN=upto(12, 0, 1), FP=upto(12, 1, 2), gt_dets=4, trk_dets=5,
                                                     DetA_alpha=upto(12, 0.8, 0.5), AssA_alpha=upto(12, 1.0, 1.8 / 3),
                                                     LocA_alpha=upto(12, 3.6 / 4, 1.0))}),
    'low_iou': (_case_low_iou(), 1, {'all': dict(TP=upto(6, 1, 0), FN=upto(6, 0, 1), FP=upto(6, 0, 1), DetA_alpha=upto(6, 1.0, 0.0),
                                                 AssA_alpha=upto(6, 1.0, 0.0), LocA_alpha=upto(6, 0.32, 1.0), HOTA_alpha=upto(6, 1.0, 0.0))}),
    'exact': (_case_exact(), 1, {'all': dict(TP=[2] * 5 + [1] * 5 + [0] * 9, LocA_alpha=[0.375] * 5 + [0.5] * 5 + [1.0] * 9,
                                             DetA_alpha=[1.0] * 5 + [1 / 3] * 5 + [0.0] * 9, AssA_alpha=[1.0] * 10 + [0.0] * 9)}),
    # a frame with both sides empty between matched frames changes nothing
    'absent': (M.HAND['absent'][0], 1, {'all': dict(TP=[4] * NA, gt_dets=4, trk_dets=4, **_perfect)}),
    # a side empty in the whole sequence: only gt_dets / trk_dets move; LocA of no TP is 1 by the max(1e-10, .) rule
    'no_gt': (M.HAND['no_gt'][0], 1, {'all': dict(TP=[0] * NA, FN=[0] * NA, FP=[3] * NA, gt_dets=0, trk_dets=3, DetA_alpha=ZERO, AssA_alpha=ZERO,
                                                  HOTA_alpha=ZERO, LocA_alpha=ONE, HOTA=0.0)}),
    'no_tracks': (M.HAND['no_tracks'][0], 1, {'all': dict(TP=[0] * NA, FN=[3] * NA, FP=[0] * NA, gt_dets=3, trk_dets=0, DetA_alpha=ZERO, HOTA=0.0)}),
    # mot_cases' class_change: track 7 is class 0 on gt 1 in frames 1, 2 and class 1 on gt 2 in frames 3, 4.  Per class: TP 2, FN 2, DetA
    # 2 / 4; the identity (class, 7) is present in 2 frames: 2 * 2 / (4 + 2 - 2) = 1, AssA 1 / 2 (one identity over both classes would be
    # present in 4: 4 / 6).  HOTA = sqrt(0.5 * 0.5).
    'class_change': (M.HAND['class_change'][0], 2, {0: dict(TP=[2] * NA, FN=[2] * NA, FP=[0] * NA, DetA_alpha=[0.5] * NA, AssA_alpha=[0.5] * NA, HOTA=0.5),
                                                    1: dict(TP=[2] * NA, FN=[2] * NA, FP=[0] * NA, DetA_alpha=[0.5] * NA, AssA_alpha=[0.5] * NA, HOTA=0.5),
                                                    'all': dict(TP=[4] * NA, FN=[4] * NA, DetA_alpha=[0.5] * NA, AssA_alpha=[0.5] * NA, HOTA=0.5)}),
    # mot_cases' class_range: classes outside [0, 2) leave; class 0 keeps gt 1 + track 1 (TP) and track 2 (FP); class 1 keeps gt 3 only
    # (its track is inside a region)
    'class_range': (M.HAND['class_range'][0], 2, {0: dict(TP=[1] * NA, FN=[0] * NA, FP=[1] * NA, gt_dets=1, trk_dets=2, AssA_alpha=ONE),
                                                  1: dict(TP=[0] * NA, FN=[1] * NA, FP=[0] * NA, gt_dets=1, trk_dets=0),
                                                  'all': dict(TP=[1] * NA, FN=[1] * NA, FP=[1] * NA, DetA_alpha=[1 / 3] * NA, AssA_alpha=ONE)}),
    # mot_cases' C: the region and the distractor take a track each first: trk_dets 3, one TP, two FP
    'region_distractor': (M.HAND['C'][0], 1, {'all': dict(TP=[1] * NA, FN=[0] * NA, FP=[2] * NA, gt_dets=1, trk_dets=3, DetA_alpha=[1 / 3] * NA,
                                                          AssA_alpha=ONE, HOTA=math.sqrt(1 / 3))}),
    # mot_cases' reuse: two sequences both call their object 1; each is perfect on its own (one pair table over both would give
    # gcount 4 and AssA 0.5)
    'reuse': (M.HAND['reuse'][0], 1, {'all': dict(TP=[4] * NA, gt_dets=4, trk_dets=4, **_perfect)}),
}


def check_expected(summary, expected, what=''):
    for key, want in expected.items():
        row = summary['all'] if key == 'all' else summary['per_class'][key]
        for k, v in want.items():
            got, v = (row[k], v) if isinstance(v, list) else ([row[k]], [v])
            assert len(got) == len(v), f'{what} [{key}]: {k} has {len(got)} entries'
            for a, (x, y) in enumerate(zip(got, v)):
                assert x == y if isinstance(y, int) else abs(x - y) <= 1e-12, f'{what} [{key}]: {k}[{a}] = {x!r}, expected {y!r}'


# ------------------------------------------------------------------------------------------------ the rule in plain loops
def _solve(score):
    """scipy's solver in place of the exhaustive search, for frames too wide for it -> the matched pairs with a positive score."""
    from scipy.optimize import linear_sum_assignment
    sc = np.asarray(score, np.float64).reshape(len(score), -1)
    return [(int(i), int(j)) for i, j in zip(*linear_sum_assignment(sc, maximize=True)) if sc[i, j] > 0] if sc.size else []


def _survivors(gt, trk, nc, iou, match=M._best_matching):
    """Steps 1 and 2 of the MOT rule, as mot_cases.literal has them -> (kind-0 rows in range, surviving track rows)."""
    gt = [[float(np.float32(v)) for v in r] for r in gt]
    trk = [[float(np.float32(v)) for v in r] for r in trk]
    trk = [t for t in trk if 0 <= t[5] < nc]
    kept = []
    for t in trk:
        area = (t[2] - t[0]) * (t[3] - t[1])
        if not any(area > 0 and M._iou(t, r)[1] / area > 0.5 for r in gt if r[6] == 2):
            kept.append(t)
    trk = kept
    side = [g for g in gt if g[6] == 1 or (g[6] == 0 and 0 <= g[5] < nc)]
    score = [[M._iou(g, t)[0] if M._iou(g, t)[0] >= iou and (g[6] == 1 or int(g[5]) == int(t[5])) else 0.0 for t in trk] for g in side]
    gone = {j for i, j in match(score) if side[i][6] == 1}
    return [g for g in side if g[6] == 0], [t for j, t in enumerate(trk) if j not in gone]


def scored_frames(frames, nc, iou=0.5, match=M._best_matching):
    """Pass 1 of the rule over one sequence -> ([(c, gt keys, track keys, S, score) per frame and class with both sides present],
    gcount, tcount, gt_dets, trk_dets); score = gas * S."""
    pot, gcount, tcount, kept = {}, {}, {}, []
    gt_dets, trk_dets = [0] * nc, [0] * nc
    for gt, trk in frames:
        gs, ts = _survivors(gt, trk, nc, iou, match)
        for c in range(nc):
            gc, tc = [g for g in gs if int(g[5]) == c], [t for t in ts if int(t[5]) == c]
            gk, tk = [(c, int(g[4])) for g in gc], [(c, int(t[4])) for t in tc]
            gt_dets[c] += len(gc)
            trk_dets[c] += len(tc)
            for k in gk:
                gcount[k] = gcount.get(k, 0) + 1
            for k in tk:
                tcount[k] = tcount.get(k, 0) + 1
            if not gc or not tc:
                continue
            S = [[M._iou(g, t)[0] for t in tc] for g in gc]
            for i in range(len(gc)):
                for j in range(len(tc)):
                    den = sum(S[i]) + sum(r[j] for r in S) - S[i][j]
                    if S[i][j] > 0:
                        pot[(gk[i], tk[j])] = pot.get((gk[i], tk[j]), 0.0) + (S[i][j] / den if den > EPS else 0.0)
            kept.append((c, gk, tk, S))
    out = []
    for c, gk, tk, S in kept:
        score = [[0.0] * len(tk) for _ in gk]
        for i in range(len(gk)):
            for j in range(len(tk)):
                if S[i][j] > 0:
                    p = pot[(gk[i], tk[j])]
                    score[i][j] = p / (gcount[gk[i]] + tcount[tk[j]] - p) * S[i][j]
        out.append((c, gk, tk, S, score))
    return out, gcount, tcount, gt_dets, trk_dets


def literal(sequences, nc, iou=0.5, match_on_iou=False):
    """The rule of csrc/hota.hip, one Python loop per sentence.  -> {key: nc lists of 19 numbers; gt_dets, trk_dets: nc numbers}.
    match_on_iou=True is the mutant that matches each frame on S alone."""
    out = {k: [[0] * NA for _ in range(nc)] for k in INT_KEYS}
    out.update({k: [[0.0] * NA for _ in range(nc)] for k in SUM_KEYS})
    out['gt_dets'], out['trk_dets'] = [0] * nc, [0] * nc
    for frames in sequences:
        scored, gcount, tcount, gd, td = scored_frames(frames, nc, iou)
        mc = {}
        for c, gk, tk, S, score in scored:
            for i, j in M._best_matching(S if match_on_iou else score):
                for a in range(NA):
                    if S[i][j] >= ALPHA[a] - EPS:
                        out['TP'][c][a] += 1
                        out['loc_sum'][c][a] += S[i][j]
                        mc.setdefault((gk[i], tk[j]), [0] * NA)[a] += 1
        for (g, t), m in mc.items():
            for a in range(NA):
                out['ass_sum'][g[0]][a] += m[a] * m[a] / max(1, gcount[g] + tcount[t] - m[a])
                out['assre_sum'][g[0]][a] += m[a] * m[a] / max(1, gcount[g])
                out['asspr_sum'][g[0]][a] += m[a] * m[a] / max(1, tcount[t])
        for c in range(nc):
            out['gt_dets'][c] += gd[c]
            out['trk_dets'][c] += td[c]
    for c in range(nc):
        out['FN'][c] = [out['gt_dets'][c] - v for v in out['TP'][c]]
        out['FP'][c] = [out['trk_dets'][c] - v for v in out['TP'][c]]
    return out


def same_counts(got, want, rtol, what=''):
    """Integer counts equal; the fp64 sums within rtol (relative)."""
    for k in INT_KEYS + ('gt_dets', 'trk_dets'):
        assert np.array_equal(np.asarray(got[k], np.int64), np.asarray(want[k], np.int64)), f'{what}: {k} {np.asarray(got[k]).tolist()} != {np.asarray(want[k]).tolist()}'
    for k in SUM_KEYS:
        a, b = np.asarray(got[k], np.float64), np.asarray(want[k], np.float64)
        assert a.shape == b.shape and (np.abs(a - b) <= rtol * np.abs(b)).all(), f'{what}: {k} {a.tolist()} vs {b.tolist()}'


def unique_optimum(frames, nc, iou=0.5, margin=1e-9):
    """Asserts, for every frame and class of the sequence, that forbidding any matched positive pair lowers the optimal total by at
    least `margin`: device and numpy differ in pot by about n * 2^-53 (the order of a sum), which then cannot change a matching.
    -> the smallest loss seen (inf when nothing is matched)."""
    from scipy.optimize import linear_sum_assignment
    worst = math.inf
    for f, (c, gk, tk, S, score) in enumerate(scored_frames(frames, nc, iou, _solve)[0]):
        sc = np.asarray(score, np.float64)
        r, cc = linear_sum_assignment(sc, maximize=True)
        best = sc[r, cc].sum()
        for i, j in zip(r, cc):
            if sc[i, j] > 0:
                alt = sc.copy()
                alt[i, j] = 0.0
                r2, c2 = linear_sum_assignment(alt, maximize=True)
                loss = best - alt[r2, c2].sum()
                assert loss >= margin, f'frame entry {f} class {c}: forbidding ({gk[i]}, {tk[j]}) loses only {loss!r}'
                worst = min(worst, loss)
    return worst
