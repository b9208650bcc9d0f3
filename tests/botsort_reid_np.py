"""numpy twin of BOTSORT.update with with_reid on (ultralytics/trackers/bot_sort.py:55-64, 166-190 with utils/matching.py:84-105) on
the slot table that csrc/track.hip keeps: BotSortNp (tests/botsort_np.py) plus the appearance half of the rule.  The reference writes
that half out and ships no encoder ("Haven't supported BoT-SORT(reid) yet"); run with a stub encoder it is what this twin is held to
(tests/golden/make_botsort_reid_golden.py).  Test infrastructure only; the package never imports it.

The table gains feat [T, D], a track's smooth_feat.  update(det, warp, feats) takes one raw feature row per detection.

Where features enter
  Every detection that becomes a BOTrack gets a feature: init_track is called twice per frame, for the high set and for the low set
  (byte_tracker.py:264, 295), so a match of the second association updates a track's feature too.
update_features(feat) (bot_sort.py:55-64)
  feat /= norm(feat); curr = feat; smooth = feat if the track had none, else alpha * smooth + (1 - alpha) * feat; smooth /= norm(smooth).
  alpha = 0.9.  All of it is fp32: the stub returns fp32 rows and numpy 2 treats python scalars as weak, so 0.9 and 1 - 0.9 act as
  their fp32 values; norm is np.linalg.norm, sqrt(x.dot(x)) in fp32.
  A fresh detection's smooth IS the array feat (smooth = feat binds the same object), so the last step divides it again: a
  detection's curr_feat is its row normalised TWICE (`prepare`).  When a track takes a detection, update_features(new.curr_feat)
  divides that - already twice normalised - row by its norm once more before it is blended in.
When features update
  update and re_activate call update_features(new.curr_feat) before the filter update (bot_sort.py:75-85); a lost track keeps its
  smooth_feat; a new track IS its detection and keeps the detection's (twice normalised) row.
get_dists (bot_sort.py:176-190), used for the first association (match_thresh) and for the unconfirmed tracks (0.7)
  d = iou_distance (fp32); mask = d > proximity_thresh, on the raw fp32 distance before fuse_score, compared in fp32;
  d = fuse_score(d) (fp32); e = max(0, cdist(smooth, curr, 'cosine')) / 2 in fp64 from the fp32 rows, where cdist's cosine is
  1 - uv / (sqrt(uu) * sqrt(vv)) with the quotient clipped to [-1, 1]; e[e > appearance_thresh] = 1; e[mask] = 1;
  cost = minimum(d, e), an fp64 matrix.  The second association stays plain IoU distance at 0.5 (byte_tracker.py:298).  An empty
  side gives an empty matrix.
Project decision
  A feature row of zero norm is outside the contract: the reference divides by zero there.

`dtype=np.float64` runs the same rule with fp64 features (the fixture generator measures how far the costs of the two runs lie apart
and derives the margin an assignment must have from it).  The counters of `events` say which of the rules a sequence exercised.
"""
import numpy as np

import bytetrack_np as T
import botsort_np as BS
from bytetrack_np import (FREE, TRACKED, LOST, LIMBO, RAW, EVER_REMOVED, M_STATE, M_ACT, M_ID, M_FRAME, M_START, M_IDX, M_FLAGS,
                          H_FRAME, H_NEXT, H_LIVE, H_OVER, f32)

ALPHA = 0.9
REID_EVENTS = ('pairs', 'emb_won', 'app_clipped', 'prox_masked', 'assign_differs', 'unconf_by_embedding', 'feat_match2', 'feat_reactivate',
               'feat_updates_max')      # pairs - prox_masked = the pairs that pass the proximity gate and get an embedding distance


def prepare(rows, dtype=f32):
    """What a detection's curr_feat is once BOTrack.__init__ has run update_features on it: the row divided by its norm twice."""
    x = np.array(rows, dtype).reshape(len(rows), -1)
    for i in range(len(x)):
        x[i] /= np.linalg.norm(x[i])
        x[i] /= np.linalg.norm(x[i])
    return x


def update_features(smooth, curr, dtype=f32):
    """A track with smooth_feat `smooth` takes a detection whose curr_feat is `curr` -> the new smooth_feat."""
    feat = curr.astype(dtype) / np.linalg.norm(curr.astype(dtype))
    if dtype == f32:
        s = f32(ALPHA) * smooth + f32(1 - ALPHA) * feat
    else:
        s = ALPHA * smooth + (1 - ALPHA) * feat
    return (s / np.linalg.norm(s)).astype(dtype)


def embedding_distance(smooth, curr):
    """max(0, cdist(smooth, curr, 'cosine')) in fp64, written out: [n, D] x [m, D] -> [n, m]."""
    u, v = np.asarray(smooth, np.float64), np.asarray(curr, np.float64)
    cs = (u @ v.T) / (np.sqrt((u * u).sum(1))[:, None] * np.sqrt((v * v).sum(1))[None, :])
    return np.maximum(0.0, 1.0 - np.clip(cs, -1.0, 1.0))


class BotSortReidNp(BS.BotSortNp):
    def __init__(self, reid_dim, proximity_thresh=0.5, appearance_thresh=0.25, dtype=f32, **kw):
        self.D, self.prox, self.app, self.dtype = int(reid_dim), proximity_thresh, appearance_thresh, dtype
        super().__init__(**kw)

    def reset(self):
        super().reset()
        self.state['feat'] = np.zeros((self.T, self.D), self.dtype)
        self.events.update(dict.fromkeys(REID_EVENTS, 0))
        self.n_updates = np.zeros(self.T, np.int64)
        self.costs, self.max_matches = [], 0       # every get_dists matrix of the run; the most matches one assignment made

    def _dists(self, slots, dets, dbox, score, feats, limit):
        """get_dists for the tracks in `slots` x the detections `dets` -> (cost f64 [n, m], fused f32 [n, m])."""
        ev = self.events
        raw = f32(1) - T.iou32(self._tlbr32(slots), dbox[dets])
        fused = f32(1) - (f32(1) - raw) * score[dets][None, :]
        if raw.size == 0:
            return fused.astype(np.float64), fused
        mask = raw > f32(self.prox)
        e = embedding_distance(self.state['feat'][slots], feats[dets]) / 2.0
        self._near(raw, float(f32(self.prox)))
        self._near(e, self.app)
        ev['app_clipped'] += int(((e > self.app) & ~mask).sum())
        ev['prox_masked'] += int(mask.sum())
        ev['pairs'] += int(mask.size)
        e[e > self.app] = 1.0
        e[mask] = 1.0
        cost = np.minimum(fused, e)
        ev['emb_won'] += int((e < fused).sum())
        self.costs.append(cost.copy())
        if not np.array_equal(T.assign(cost, limit)[0], T.assign(fused, limit)[0]):
            ev['assign_differs'] += 1
        return cost, fused

    def _assign(self, cost, L):
        x = super()._assign(cost, L)
        self.max_matches = max(self.max_matches, int((np.asarray(x) >= 0).sum()))
        return x

    def _take(self, s, feats, j):
        self.state['feat'][s] = update_features(self.state['feat'][s], feats[j], self.dtype)
        self.n_updates[s] += 1
        self.events['feat_updates_max'] = max(self.events['feat_updates_max'], int(self.n_updates[s]))

    def update(self, det, warp=None, feats=None):
        """det f32 [n, 6] (x1 y1 x2 y2 score cls), warp f64 [2, 3] or None, feats [n, D] raw feature rows -> rows f32 [k, 8]
        (x1 y1 x2 y2 id score cls idx), in slot order.  A frame without detections returns no rows and changes nothing."""
        d = np.asarray(det, f32).reshape(-1, 6)
        if len(d) == 0:
            self.events['empty_frame'] += 1
            return np.zeros((0, 8), f32)
        feats = prepare(np.asarray(feats).reshape(len(d), self.D), self.dtype)
        H = np.eye(2, 3) if warp is None else np.asarray(warp, np.float64).reshape(2, 3)
        kf, st, ev = self.kf, self.state, self.events
        mean, cov, meta, sc, hdr = st['mean'], st['cov'], st['meta'], st['sc'], st['hdr']
        hdr[H_FRAME] += 1
        fid = int(hdr[H_FRAME])
        score = d[:, 4]
        self._near(score, self.high, self.low, self.new)
        hi = [j for j in range(len(d)) if score[j] > f32(self.high)]
        lo = [j for j in range(len(d)) if score[j] > f32(self.low) and score[j] < f32(self.high)]
        dbox = T.det_tlbr32(d[:, :4])
        unconf = [s for s in range(self.T) if meta[s, M_STATE] == TRACKED and not meta[s, M_ACT]]
        pool = [s for s in range(self.T) if (meta[s, M_STATE] == TRACKED and meta[s, M_ACT]) or meta[s, M_STATE] in (LOST, LIMBO)]
        for s in pool:
            m = mean[s].copy()
            if meta[s, M_STATE] != TRACKED:
                ev['lost_zeroed_vw_vh'] += bool(m[6] != 0 or m[7] != 0) and len(kf['zero']) == 2
                m[list(kf['zero'])] = 0
            mean[s], cov[s] = kf['predict'](m, cov[s], meta[s, M_FLAGS] & RAW)
            meta[s, M_FLAGS] &= ~RAW
        for s in (pool + unconf if self.with_image else []):
            mean[s], cov[s] = BS.gmc(mean[s], cov[s], H)
            meta[s, M_FLAGS] &= ~RAW
        moved = not np.array_equal(H, np.eye(2, 3))
        ev['warped'] += moved and len(pool) > 0
        ev['warp_unconfirmed'] += moved * len(unconf)

        # first association: pool x high detections, get_dists
        cost, _ = self._dists(pool, hi, dbox, score, feats, self.match)
        x = self._assign(cost, self.match)
        used, newly_lost = set(), set()
        for i, j in enumerate(x):
            if j >= 0:
                s = pool[i]
                was = meta[s, M_STATE]
                ev['match1'] += 1
                ev['refind'] += was != TRACKED
                ev['revived'] += was == LIMBO
                ev['feat_reactivate'] += was != TRACKED
                self._take(s, feats, hi[j])
                self._matched(s, d, hi[j], fid, keep_len=was == TRACKED)
                used.add(hi[j])
        # second association: what is left of the pool in state Tracked x low detections, plain IoU distance, threshold 0.5
        rest = [s for i, s in enumerate(pool) if x[i] < 0 and meta[s, M_STATE] == TRACKED]
        x2 = self._assign(f32(1) - T.iou32(self._tlbr32(rest), dbox[lo]), 0.5)
        for i, j in enumerate(x2):
            s = rest[i]
            if j >= 0:
                ev['match2'] += 1
                ev['feat_match2'] += 1
                self._take(s, feats, lo[j])
                self._matched(s, d, lo[j], fid, keep_len=True)
            elif meta[s, M_FLAGS] & EVER_REMOVED:
                meta[s, M_STATE] = FREE
            else:
                meta[s, M_STATE] = LOST
                newly_lost.add(s)
        # unconfirmed tracks x the high detections still free, get_dists, threshold 0.7
        left = [j for j in hi if j not in used]
        cost, fused = self._dists(unconf, left, dbox, score, feats, 0.7)
        x3 = self._assign(cost, 0.7)
        for i, j in enumerate(x3):
            if j >= 0:
                ev['match_unconfirmed'] += 1
                ev['unconf_by_embedding'] += bool(fused[i, j] > 0.7)
                self._take(unconf[i], feats, left[j])
                self._matched(unconf[i], d, left[j], fid, keep_len=True)
                used.add(left[j])
            else:
                ev['unconfirmed_removed'] += 1
                meta[unconf[i], M_STATE] = FREE
        # new tracks: the detection's row is the track's smooth_feat
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
            mean[s], cov[s] = kf['initiate'](kf['z'](d[j, :4]))
            meta[s] = TRACKED, int(fid == 1), hdr[H_NEXT], fid, fid, 0, j, RAW
            sc[s] = d[j, 4], d[j, 5]
            st['feat'][s] = feats[j]
            self.n_updates[s] = 0
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
        pd = f32(1) - T.iou32(self._tlbr32(A), self._tlbr32(B))
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
            rows[k, :4] = kf['tlbr'](mean[s])
            rows[k, 4:] = meta[s, M_ID], sc[s, 0], sc[s, 1], meta[s, M_IDX]
        return rows

    def live_feat(self):
        """{id: smooth_feat} of the live tracks."""
        return {int(m[M_ID]): self.state['feat'][s].copy() for s, m in enumerate(self.state['meta']) if m[M_STATE] != FREE}


# ---------------------------------------------------------------------------------------------------- seeded features and scenes
def object_features(seed, obj_of_det, n_obj, D=16, p_mid=0.06, p_far=0.06):
    """One raw feature row per detection, as fp16 values held in fp32: object o has a fixed unit vector (n_obj orthonormal axes of a
    seeded rotation; index n_obj serves every false positive), a detection's row is cos(t) * axis + sin(t) * n with n a unit vector
    in the complement of all axes, so rows of different objects stay near cosine 0 and t alone sets the distance to the own
    object: mostly small, sometimes about e = 0.12 (`mid`, under appearance_thresh 0.25), sometimes about e = 0.4 (`far`, above).
    obj_of_det: per frame, the object index of each detection (-1 = a false positive).  -> list of f32 [n, D]."""
    assert n_obj + 1 < D
    rng = np.random.default_rng(seed)
    Q = np.linalg.qr(rng.normal(size=(D, D)))[0]
    out = []
    for objs in obj_of_det:
        rows = np.zeros((len(objs), D))
        for i, o in enumerate(objs):
            r = rng.random()
            e = rng.uniform(0.36, 0.46) if r < p_far else rng.uniform(0.08, 0.16) if r < p_far + p_mid else rng.uniform(0.0005, 0.01)
            c = 1 - 2 * e
            n = Q[:, n_obj + 1:] @ rng.normal(size=D - n_obj - 1)
            rows[i] = rng.uniform(0.5, 2.0) * (c * Q[:, o if o >= 0 else n_obj] + np.sqrt(1 - c * c) * n / np.linalg.norm(n))
        out.append(rows.astype(np.float16).astype(f32))
    return out


def make_scene(seed, n_obj=12, frames=30, size=(1080, 1920), p_low=0.15, fp_every=5, empty=(), gaps=(), ncls=4):
    """bytetrack_np.make_scene's kind of sequence that also says which object a detection shows: objects on straight lines with
    jitter, late starts, low-score frames, one-frame false positives, detection gaps [(object, first frame, length)] and empty
    frames.  -> (list of f32 [n, 6], list of i64 [n]: the object of each row, -1 = a false positive), rows shuffled."""
    rng = np.random.default_rng(seed)
    H, W = size
    cx, cy = rng.uniform(0.1 * W, 0.9 * W, n_obj), rng.uniform(0.1 * H, 0.9 * H, n_obj)
    vx, vy = rng.uniform(-4, 4, n_obj), rng.uniform(-3, 3, n_obj)
    w, h = rng.uniform(40, 120, n_obj), rng.uniform(60, 160, n_obj)
    cls = rng.integers(0, ncls, n_obj)
    start = np.where(rng.random(n_obj) < 0.3, rng.integers(1, max(2, frames // 3), n_obj), 0)
    out, who = [], []
    for f in range(frames):
        rows, ids = [], []
        for o in range(n_obj):
            if f < start[o] or any(g[0] == o and g[1] <= f < g[1] + g[2] for g in gaps):
                continue
            j = rng.normal(0, 1.0, 4)
            x, y = cx[o] + vx[o] * f + j[0], cy[o] + vy[o] * f + j[1]
            ww, hh = w[o] + j[2], h[o] + j[3]
            s = rng.uniform(0.15, 0.45) if rng.random() < p_low else rng.uniform(0.65, 0.95)
            rows.append([x - ww / 2, y - hh / 2, x + ww / 2, y + hh / 2, s, cls[o]])
            ids.append(o)
        if fp_every and f % fp_every == fp_every - 1:
            x, y = rng.uniform(0.05 * W, 0.95 * W), rng.uniform(0.05 * H, 0.95 * H)
            rows.append([x - 30, y - 40, x + 30, y + 40, rng.uniform(0.52, 0.58) if f % (2 * fp_every) == fp_every - 1 else rng.uniform(0.65, 0.9),
                         rng.integers(0, ncls)])
            ids.append(-1)
        if f in empty:
            rows, ids = [], []
        a, k = np.array(rows, f32).reshape(-1, 6), rng.permutation(len(rows))
        out.append(a[k])
        who.append(np.asarray(ids, np.int64)[k])
    return out, who


def make_cross(seed, pairs=3, frames=40, late=(12, 13)):
    """Same-size objects in pairs that approach each other, coincide and turn back where they meet, under a camera at rest: a filter
    that extrapolates their motion expects them to pass through each other, so IoU alone exchanges their identities.  Object
    2 * pairs appears at frame late[0] and jumps by 0.31 of its width with a score of 0.55 at late[1]: its unconfirmed track meets a
    fused cost above 0.7 and keeps the detection through its embedding only.  -> (frames, objects) as make_scene."""
    rng = np.random.default_rng(seed)
    cx, cy = 300.0 + 450.0 * np.arange(pairs), rng.uniform(250, 800, pairs)
    w, h, v = rng.uniform(70, 90, pairs), rng.uniform(110, 140, pairs), rng.uniform(2.0, 3.0, pairs)
    fc = frames // 2 + rng.integers(-3, 4, pairs)
    out, who = [], []
    for f in range(frames):
        rows, ids = [], []
        for p in range(pairs):
            for t in range(2):
                j = rng.normal(0, 0.3, 2)
                x = cx[p] + (2 * t - 1) * v[p] * abs(f - fc[p]) + j[0]
                y = cy[p] + j[1]
                rows.append([x - w[p] / 2, y - h[p] / 2, x + w[p] / 2, y + h[p] / 2, rng.uniform(0.7, 0.95), p % 3])
                ids.append(2 * p + t)
        if f >= late[0]:
            x = 1700.0 + (31.0 if f >= late[1] else 0.0)
            rows.append([x - 50, 500.0, x + 50, 600.0, 0.55 if f == late[1] else 0.9, 1])
            ids.append(2 * pairs)
        a, k = np.array(rows, f32).reshape(-1, 6), rng.permutation(len(rows))
        out.append(a[k])
        who.append(np.asarray(ids, np.int64)[k])
    return out, who
