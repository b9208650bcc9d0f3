"""numpy twin of BYTETracker.update (ultralytics/trackers/byte_tracker.py:238-351 with utils/kalman_filter.py:33-180 and
utils/matching.py:20-126) on the slot table that csrc/track.hip keeps: the rule restated, fp64 filters and fp32 costs.  Test
infrastructure only; the package never imports it.

The table (the arrays of ByteTracker.state_dict()):
  mean f64 [T, 8], cov f64 [T, 8, 8]
  meta i32 [T, 8]   state, is_activated, track_id, frame_id, start_frame, tracklet_len, idx, flags
  sc   f32 [T, 2]   score, cls
  hdr  i32 [8]      frame_id, next_id, live slots, overflow count, 0...
state: 0 free slot, 1 Tracked, 2 Lost, 3 Removed but still listed.  The reference takes a lost track that aged out from its lost
list only one update later (it filters with the removed list as it stood BEFORE the frame's removals, byte_tracker.py:344-346); in
between the track still takes part in the first association, where a match revives it, and in the duplicate removal.
flags: 1 = the mean still is the fp32 measurement it was initiated with (numpy then derives the first predict's process noise and the
first projection's std in fp32: `0.05 * np.float32` is fp32), 2 = the id is in the reference's removed list (such a track, revived and
lost again, leaves the lost list at once).  The reference clips that list to its last 999 entries; the table never forgets.

Every assignment is the optimum of lap.lapjv(cost, extend_cost=True, cost_limit=L): the partial matching that minimises
sum(c_ij - L).  `margin` is the smallest gap this tracker saw between an assignment's optimum and its best alternative.
"""
import numpy as np
from scipy.optimize import linear_sum_assignment

FREE, TRACKED, LOST, LIMBO = 0, 1, 2, 3
RAW, EVER_REMOVED = 1, 2
M_STATE, M_ACT, M_ID, M_FRAME, M_START, M_LEN, M_IDX, M_FLAGS = range(8)
H_FRAME, H_NEXT, H_LIVE, H_OVER = range(4)
f32 = np.float32
_BIG = 1e6


def new_state(T):
    hdr = np.zeros(8, np.int32)
    hdr[H_NEXT] = 1
    return {'mean': np.zeros((T, 8)), 'cov': np.zeros((T, 8, 8)), 'meta': np.zeros((T, 8), np.int32), 'sc': np.zeros((T, 2), f32),
            'hdr': hdr}


def lapjv_extended(cost, cost_limit):
    """What lap.lapjv(cost, extend_cost=True, cost_limit=L) solves: the n x m cost embedded in an (n + m)^2 matrix filled with L / 2,
    a zero block bottom-right; the real pairs of its optimum.  -> (opt, x [n], y [m]), -1 = unmatched."""
    cost = np.asarray(cost, np.float64)
    n, m = cost.shape
    ext = np.full((n + m, n + m), cost_limit / 2.0)
    ext[n:, m:] = 0.0
    ext[:n, :m] = cost
    r, c = linear_sum_assignment(ext)
    x, y = np.full(n, -1, np.int64), np.full(m, -1, np.int64)
    for i, j in zip(r, c):
        if i < n and j < m:
            x[i], y[j] = j, i
    return float(ext[r, c].sum()), x, y


def assign(cost, L, want_margin=False):
    """The same optimum with one private `unmatched` column of cost L per row (partial matchings and solutions correspond one to one).
    -> (x [n], margin): margin = best alternative - optimum, found by re-solving with each chosen pair forbidden."""
    cost = np.asarray(cost, np.float64)
    n, m = cost.shape
    ext = np.full((n, m + n), _BIG)
    ext[:, :m] = cost
    ext[np.arange(n), m + np.arange(n)] = L
    r, c = linear_sum_assignment(ext)
    x = np.where(c < m, c, -1)
    margin = np.inf
    if want_margin:
        opt = ext[r, c].sum()
        for i in range(n):
            e = ext.copy()
            e[i, c[i]] = _BIG
            r2, c2 = linear_sum_assignment(e)
            margin = min(margin, e[r2, c2].sum() - opt)
    return x, margin


def iou32(a, b):
    """bbox_ioa(a, b, iou=True) of utils/metrics.py:17-46 in fp32: a [n, 4], b [m, 4] tlbr -> [n, m]."""
    a, b = np.asarray(a, f32).reshape(-1, 4), np.asarray(b, f32).reshape(-1, 4)
    ax1, ay1, ax2, ay2 = a.T
    bx1, by1, bx2, by2 = b.T
    inter = (np.minimum(ax2[:, None], bx2) - np.maximum(ax1[:, None], bx1)).clip(0) * \
            (np.minimum(ay2[:, None], by2) - np.maximum(ay1[:, None], by1)).clip(0)
    area = (bx2 - bx1) * (by2 - by1)
    area = area + ((ax2 - ax1) * (ay2 - ay1))[:, None] - inter
    return inter / (area + f32(1e-7))


def det_tlbr32(d):
    """The tlbr an STrack without a mean reports: x1 y1 (x2 - x1) + x1 (y2 - y1) + y1 in fp32 (byte_tracker.py:48, 151-166)."""
    d = np.asarray(d, f32)
    w, h = d[:, 2] - d[:, 0], d[:, 3] - d[:, 1]
    return np.stack([d[:, 0], d[:, 1], w + d[:, 0], h + d[:, 1]], 1)


def det_xyah32(d):
    """convert_coords of a detection: fp32 throughout (byte_tracker.py:168-176)."""
    d = np.asarray(d, f32)
    w, h = d[2] - d[0], d[3] - d[1]
    return np.array([d[0] + w / f32(2), d[1] + h / f32(2), w / h, h], f32)


def mean_tlbr(mean):
    x, y, a, h = mean[:4]
    w = a * h
    x1, y1 = x - w / 2, y - h / 2
    return np.array([x1, y1, w + x1, h + y1])


# ---------------------------------------------------------------------------------------------------- the filter
def kf_initiate(z):
    h = f32(z[3])
    sp, sv = float(f32(0.1) * h), float(f32(0.0625) * h)
    mean = np.zeros(8)
    mean[:4] = z
    return mean, np.diag([sp * sp, sp * sp, 1e-2 * 1e-2, sp * sp, sv * sv, sv * sv, 1e-5 * 1e-5, sv * sv])


def kf_predict(mean, cov, raw):
    if raw:
        h = f32(mean[3])
        sp, sv = f32(1. / 20) * h, f32(1. / 160) * h
        q = np.array([sp * sp, sp * sp, f32(1e-2) * f32(1e-2), sp * sp, sv * sv, sv * sv, f32(1e-5) * f32(1e-5), sv * sv], f32).astype(np.float64)
    else:
        sp, sv = 1. / 20 * mean[3], 1. / 160 * mean[3]
        q = np.array([sp * sp, sp * sp, 1e-2 * 1e-2, sp * sp, sv * sv, sv * sv, 1e-5 * 1e-5, sv * sv])
    m = mean.copy()
    m[:4] = mean[:4] + mean[4:]
    A, B, C, D = cov[:4, :4], cov[:4, 4:], cov[4:, :4], cov[4:, 4:]
    p = np.empty((8, 8))
    p[:4, :4] = (A + C) + (B + D)
    p[:4, 4:] = B + D
    p[4:, :4] = C + D
    p[4:, 4:] = D
    p[np.arange(8), np.arange(8)] += q
    return m, p


def kf_update(mean, cov, z, raw):
    sp = float(f32(1. / 20) * f32(mean[3])) if raw else 1. / 20 * mean[3]
    S = cov[:4, :4] + np.diag([sp * sp, sp * sp, 1e-1 * 1e-1, sp * sp])
    Lc = np.linalg.cholesky(S)
    X = np.linalg.solve(Lc.T, np.linalg.solve(Lc, cov[:, :4].T))      # S X = (P H^T)^T
    K = X.T
    return mean + K @ (np.asarray(z, np.float64) - mean[:4]), cov - K @ (S @ K.T)


# ---------------------------------------------------------------------------------------------------- the tracker
class ByteTrackNp:
    def __init__(self, track_high_thresh=0.5, track_low_thresh=0.1, new_track_thresh=0.6, track_buffer=30, match_thresh=0.8,
                 frame_rate=30, capacity=1024, want_margin=False):
        self.high, self.low, self.new, self.match = track_high_thresh, track_low_thresh, new_track_thresh, match_thresh
        self.max_time_lost = int(frame_rate / 30.0 * track_buffer)
        self.T, self.want_margin = capacity, want_margin
        self.reset()

    def reset(self):
        self.state = new_state(self.T)
        self.margin = self.thr_margin = np.inf     # assignment optimum vs runner-up; |cost - threshold|, |score - threshold|
        self.events = dict.fromkeys(('match1', 'match2', 'refind', 'aged_out', 'unconfirmed_removed', 'new_refused', 'dup_lost_dropped',
                                     'dup_tracked_dropped', 'empty_frame', 'match_unconfirmed', 'revived', 'new'), 0)

    def _near(self, values, *thresholds):
        v = np.asarray(values, np.float64).reshape(-1)
        for t in thresholds:
            if v.size:
                self.thr_margin = min(self.thr_margin, float(np.abs(v - t).min()))

    def _assign(self, cost, L):
        n, m = cost.shape
        if n == 0 or m == 0:
            return np.full(n, -1, np.int64)
        self._near(cost, L)
        x, mg = assign(cost, L, self.want_margin)
        self.margin = min(self.margin, mg)
        return x

    def _tlbr32(self, slots):
        return np.array([mean_tlbr(self.state['mean'][s]) for s in slots], np.float64).reshape(-1, 4).astype(f32)

    def _matched(self, s, d, j, fid, keep_len):
        st = self.state
        meta = st['meta'][s]
        st['mean'][s], st['cov'][s] = kf_update(st['mean'][s], st['cov'][s], det_xyah32(d[j, :4]), meta[M_FLAGS] & RAW)
        meta[M_FLAGS] &= ~RAW
        meta[M_LEN] = meta[M_LEN] + 1 if keep_len else 0
        meta[M_STATE], meta[M_ACT], meta[M_FRAME], meta[M_IDX] = TRACKED, 1, fid, j
        st['sc'][s] = d[j, 4], d[j, 5]

    def update(self, det):
        """det f32 [n, 6] (x1 y1 x2 y2 score cls) -> rows f32 [k, 8] (x1 y1 x2 y2 id score cls idx), in slot order.  A frame without
        detections returns no rows and changes nothing (trackers/track.py:46-47)."""
        d = np.asarray(det, f32).reshape(-1, 6)
        if len(d) == 0:
            self.events['empty_frame'] += 1
            return np.zeros((0, 8), f32)
        st, ev = self.state, self.events
        mean, cov, meta, sc, hdr = st['mean'], st['cov'], st['meta'], st['sc'], st['hdr']
        hdr[H_FRAME] += 1
        fid = int(hdr[H_FRAME])
        score = d[:, 4]
        self._near(score, self.high, self.low, self.new)
        hi = [j for j in range(len(d)) if score[j] > f32(self.high)]
        lo = [j for j in range(len(d)) if score[j] > f32(self.low) and score[j] < f32(self.high)]
        dbox = det_tlbr32(d[:, :4])
        unconf = [s for s in range(self.T) if meta[s, M_STATE] == TRACKED and not meta[s, M_ACT]]
        pool = [s for s in range(self.T) if (meta[s, M_STATE] == TRACKED and meta[s, M_ACT]) or meta[s, M_STATE] in (LOST, LIMBO)]
        for s in pool:
            m = mean[s].copy()
            if meta[s, M_STATE] != TRACKED:
                m[7] = 0
            mean[s], cov[s] = kf_predict(m, cov[s], meta[s, M_FLAGS] & RAW)
            meta[s, M_FLAGS] &= ~RAW

        # first association: pool x high detections, fused distance
        iou = iou32(self._tlbr32(pool), dbox[hi])
        x = self._assign(f32(1) - (f32(1) - (f32(1) - iou)) * score[hi][None, :], self.match)
        used, newly_lost = set(), set()
        for i, j in enumerate(x):
            if j >= 0:
                s = pool[i]
                was = meta[s, M_STATE]
                ev['match1'] += 1
                ev['refind'] += was != TRACKED
                ev['revived'] += was == LIMBO
                self._matched(s, d, hi[j], fid, keep_len=was == TRACKED)
                used.add(hi[j])
        # second association: what is left of the pool in state Tracked x low detections, plain IoU distance, threshold 0.5
        rest = [s for i, s in enumerate(pool) if x[i] < 0 and meta[s, M_STATE] == TRACKED]
        x2 = self._assign(f32(1) - iou32(self._tlbr32(rest), dbox[lo]), 0.5)
        for i, j in enumerate(x2):
            s = rest[i]
            if j >= 0:
                ev['match2'] += 1
                self._matched(s, d, lo[j], fid, keep_len=True)
            elif meta[s, M_FLAGS] & EVER_REMOVED:
                meta[s, M_STATE] = FREE
            else:
                meta[s, M_STATE] = LOST
                newly_lost.add(s)
        # unconfirmed tracks x the high detections still free, fused distance, threshold 0.7
        left = [j for j in hi if j not in used]
        iou = iou32(self._tlbr32(unconf), dbox[left])
        x3 = self._assign(f32(1) - (f32(1) - (f32(1) - iou)) * score[left][None, :], 0.7)
        for i, j in enumerate(x3):
            if j >= 0:
                ev['match_unconfirmed'] += 1
                self._matched(unconf[i], d, left[j], fid, keep_len=True)
                used.add(left[j])
            else:
                ev['unconfirmed_removed'] += 1
                meta[unconf[i], M_STATE] = FREE
        # new tracks
        for j in left:
            if j in used:
                continue
            if score[j] < f32(self.new):
                ev['new_refused'] += 1
                continue
            free = np.flatnonzero(meta[:, M_STATE] == FREE)
            if not len(free):
                hdr[H_OVER] += 1
                continue
            s = free[0]
            mean[s], cov[s] = kf_initiate(det_xyah32(d[j, :4]))
            meta[s] = TRACKED, int(fid == 1), hdr[H_NEXT], fid, fid, 0, j, RAW
            sc[s] = d[j, 4], d[j, 5]
            hdr[H_NEXT] += 1
            ev['new'] += 1
        # lost tracks age out; one removed a frame ago leaves now
        for s in range(self.T):
            if meta[s, M_STATE] == LIMBO:
                meta[s, M_STATE] = FREE
            elif meta[s, M_STATE] == LOST and s not in newly_lost and fid - meta[s, M_FRAME] > self.max_time_lost:
                meta[s, M_STATE] = LIMBO
                meta[s, M_FLAGS] |= EVER_REMOVED
                ev['aged_out'] += 1
        # duplicates: tracked x lost, distance < 0.15; the younger side goes, the tracked side on equal age
        A = [s for s in range(self.T) if meta[s, M_STATE] == TRACKED]
        B = [s for s in range(self.T) if meta[s, M_STATE] in (LOST, LIMBO)]
        pd = f32(1) - iou32(self._tlbr32(A), self._tlbr32(B))
        self._near(pd, 0.15)
        drop = set()
        for p, q in zip(*np.where(pd < f32(0.15))):
            if meta[A[p], M_FRAME] - meta[A[p], M_START] > meta[B[q], M_FRAME] - meta[B[q], M_START]:
                drop.add(B[q])
            else:
                drop.add(A[p])
        for s in drop:
            ev['dup_lost_dropped' if meta[s, M_STATE] != TRACKED else 'dup_tracked_dropped'] += 1
            meta[s, M_STATE] = FREE
        hdr[H_LIVE] = int((meta[:, M_STATE] != FREE).sum())
        out = [s for s in range(self.T) if meta[s, M_STATE] == TRACKED and meta[s, M_ACT]]
        rows = np.zeros((len(out), 8), f32)
        for k, s in enumerate(out):
            rows[k, :4] = mean_tlbr(mean[s])
            rows[k, 4:] = meta[s, M_ID], sc[s, 0], sc[s, 1], meta[s, M_IDX]
        return rows

    def live(self):
        """The live tracks by id: {id: (state, activated, frame_id, start_frame, tracklet_len, idx, score, cls, mean, cov)}."""
        st = self.state
        return {int(m[M_ID]): (int(m[M_STATE]), int(m[M_ACT]), int(m[M_FRAME]), int(m[M_START]), int(m[M_LEN]), int(m[M_IDX]),
                               st['sc'][s, 0], st['sc'][s, 1], st['mean'][s].copy(), st['cov'][s].copy())
                for s, m in enumerate(st['meta']) if m[M_STATE] != FREE}


# ---------------------------------------------------------------------------------------------------- seeded scenes
def make_scene(seed, n_obj=10, frames=30, size=(1080, 1920), p_low=0.15, fp_every=5, empty=(), gaps=(), ncls=4):
    """A seeded sequence of detections: objects on straight lines with jitter, late starts, low-score frames, one-frame false
    positives and detection gaps [(object, first frame, length)].  -> list of f32 [n, 6], one per frame, rows shuffled."""
    rng = np.random.default_rng(seed)
    H, W = size
    cx, cy = rng.uniform(0.1 * W, 0.9 * W, n_obj), rng.uniform(0.1 * H, 0.9 * H, n_obj)
    vx, vy = rng.uniform(-4, 4, n_obj), rng.uniform(-3, 3, n_obj)
    w, h = rng.uniform(40, 120, n_obj), rng.uniform(60, 160, n_obj)
    cls = rng.integers(0, ncls, n_obj)
    start = np.where(rng.random(n_obj) < 0.3, rng.integers(1, max(2, frames // 3), n_obj), 0)
    out = []
    for f in range(frames):
        rows = []
        for o in range(n_obj):
            if f < start[o] or any(g[0] == o and g[1] <= f < g[1] + g[2] for g in gaps):
                continue
            j = rng.normal(0, 1.0, 4)
            x, y = cx[o] + vx[o] * f + j[0], cy[o] + vy[o] * f + j[1]
            ww, hh = w[o] + j[2], h[o] + j[3]
            s = rng.uniform(0.15, 0.45) if rng.random() < p_low else rng.uniform(0.65, 0.95)
            rows.append([x - ww / 2, y - hh / 2, x + ww / 2, y + hh / 2, s, cls[o]])
        if fp_every and f % fp_every == fp_every - 1:
            x, y = rng.uniform(0.05 * W, 0.95 * W), rng.uniform(0.05 * H, 0.95 * H)
            rows.append([x - 30, y - 40, x + 30, y + 40, rng.uniform(0.52, 0.58) if f % (2 * fp_every) == fp_every - 1 else rng.uniform(0.65, 0.9),
                         rng.integers(0, ncls)])
        rows = [] if f in empty else rows
        a = np.array(rows, f32).reshape(-1, 6)
        out.append(a[rng.permutation(len(a))])
    return out
