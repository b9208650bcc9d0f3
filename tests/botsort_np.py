"""numpy twin of BOTSORT.update (ultralytics/trackers/bot_sort.py with byte_tracker.py:81-97, 238-351 and
utils/kalman_filter.py:222-368) on the slot table that csrc/track.hip keeps: ByteTrackNp (tests/bytetrack_np.py) with the XYWH
filter, the changed prediction of lost tracks and the warp of the track states (multi_gmc).  Test infrastructure only; the package
never imports it.

What differs from ByteTrackNp:
  filter   state (x, y, w, h, vx, vy, vw, vh); the measurement is tlwh_to_xywh in fp32; every std is built from mean[2] and mean[3].
           A new track's mean AND covariance are fp32 arrays in the reference (every entry of initiate's std list is an fp32 scalar, so
           the squares are taken in fp32); while a mean still is that measurement (flag RAW) predict and project derive their stds and
           square them in fp32.
  predict  a pool track that is not Tracked gets mean[6] = mean[7] = 0 first (bot_sort.py:97-110).
  warp     after the pool's predict and before the first association, the frame's 2x3 warp H goes to every pool track and every
           unconfirmed track: with R = H[:, :2], t = H[:, 2]: mean = kron(I4, R) @ mean, mean[:2] += t, cov = R8 @ cov @ R8.T.  The
           result is an fp64 array, so a warped track is no longer RAW - also under the identity warp, which is what `warp=None`
           means here (the reference run with an image and GMC method none).
  costs    get_dists with with_reid off is the fused IoU distance ByteTrack uses; the tlbr of a mean is x - w/2, y - h/2, w + x1,
           h + y1.
`filter='xyah'` keeps ByteTrack's filter and prediction under the same flow: with identity warps it is ByteTrackNp up to the
rounding of the RAW rule, which guards the code the two share.
"""
import numpy as np

import bytetrack_np as T
from bytetrack_np import (FREE, TRACKED, LOST, LIMBO, RAW, EVER_REMOVED, M_STATE, M_ACT, M_ID, M_FRAME, M_START, M_LEN, M_IDX, M_FLAGS,
                          H_FRAME, H_NEXT, H_LIVE, H_OVER, f32)


def det_xywh32(d):
    """convert_coords of a detection (tlbr_to_tlwh, tlwh_to_xywh): fp32 throughout (bot_sort.py:112-121)."""
    d = np.asarray(d, f32)
    w, h = d[2] - d[0], d[3] - d[1]
    return np.array([d[0] + w / f32(2), d[1] + h / f32(2), w, h], f32)


def mean_tlbr_xywh(mean):
    x, y, w, h = mean[:4]
    x1, y1 = x - w / 2, y - h / 2
    return np.array([x1, y1, w + x1, h + y1])


# ---------------------------------------------------------------------------------------------------- KalmanFilterXYWH
def kf_initiate(z):
    w, h = f32(z[2]), f32(z[3])
    pw, ph, vw, vh = f32(0.1) * w, f32(0.1) * h, f32(0.0625) * w, f32(0.0625) * h
    mean = np.zeros(8)
    mean[:4] = z
    return mean, np.diag(np.array([pw * pw, ph * ph, pw * pw, ph * ph, vw * vw, vh * vh, vw * vw, vh * vh], f32).astype(np.float64))


def _stds(mean, raw):
    """(position std of w, of h, velocity std of w, of h)^2, in fp32 while the mean is the fp32 measurement."""
    if raw:
        w, h = f32(mean[2]), f32(mean[3])
        s = np.array([f32(1. / 20) * w, f32(1. / 20) * h, f32(1. / 160) * w, f32(1. / 160) * h], f32)
        return (s * s).astype(np.float64)
    s = np.array([1. / 20 * mean[2], 1. / 20 * mean[3], 1. / 160 * mean[2], 1. / 160 * mean[3]])
    return s * s


def kf_predict(mean, cov, raw):
    pw, ph, vw, vh = _stds(mean, raw)
    q = np.array([pw, ph, pw, ph, vw, vh, vw, vh])
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
    pw, ph, _, _ = _stds(mean, raw)
    S = cov[:4, :4] + np.diag([pw, ph, pw, ph])
    Lc = np.linalg.cholesky(S)
    X = np.linalg.solve(Lc.T, np.linalg.solve(Lc, cov[:, :4].T))      # S X = (P H^T)^T
    K = X.T
    return mean + K @ (np.asarray(z, np.float64) - mean[:4]), cov - K @ (S @ K.T)


def gmc(mean, cov, H):
    """STrack.multi_gmc for one track (byte_tracker.py:81-97)."""
    H = np.asarray(H, np.float64).reshape(2, 3)
    R8 = np.kron(np.eye(4), H[:, :2])
    m = R8.dot(mean)
    m[:2] += H[:, 2]
    return m, R8.dot(cov).dot(R8.T)


XYWH = dict(initiate=kf_initiate, predict=kf_predict, update=kf_update, z=det_xywh32, tlbr=mean_tlbr_xywh, zero=(6, 7))
XYAH = dict(initiate=T.kf_initiate, predict=T.kf_predict, update=T.kf_update, z=T.det_xyah32, tlbr=T.mean_tlbr, zero=(7,))


# ---------------------------------------------------------------------------------------------------- the tracker
class BotSortNp(T.ByteTrackNp):
    def __init__(self, filter='xywh', with_image=True, **kw):
        self.kf = {'xywh': XYWH, 'xyah': XYAH}[filter]
        self.with_image = with_image      # False: the reference called without an image, which skips multi_gmc altogether
        super().__init__(**kw)

    def reset(self):
        super().reset()
        self.events.update(dict.fromkeys(('warp_unconfirmed', 'lost_zeroed_vw_vh', 'warped'), 0))

    def _tlbr32(self, slots):
        return np.array([self.kf['tlbr'](self.state['mean'][s]) for s in slots], np.float64).reshape(-1, 4).astype(f32)

    def _matched(self, s, d, j, fid, keep_len):
        st = self.state
        meta = st['meta'][s]
        st['mean'][s], st['cov'][s] = self.kf['update'](st['mean'][s], st['cov'][s], self.kf['z'](d[j, :4]), meta[M_FLAGS] & RAW)
        meta[M_FLAGS] &= ~RAW
        meta[M_LEN] = meta[M_LEN] + 1 if keep_len else 0
        meta[M_STATE], meta[M_ACT], meta[M_FRAME], meta[M_IDX] = TRACKED, 1, fid, j
        st['sc'][s] = d[j, 4], d[j, 5]

    def update(self, det, warp=None):
        """det f32 [n, 6] (x1 y1 x2 y2 score cls), warp f64 [2, 3] or None for identity -> rows f32 [k, 8] (x1 y1 x2 y2 id score cls
        idx), in slot order.  A frame without detections returns no rows and changes nothing, its warp included."""
        d = np.asarray(det, f32).reshape(-1, 6)
        if len(d) == 0:
            self.events['empty_frame'] += 1
            return np.zeros((0, 8), f32)
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
            mean[s], cov[s] = gmc(mean[s], cov[s], H)
            meta[s, M_FLAGS] &= ~RAW
        moved = not np.array_equal(H, np.eye(2, 3))
        ev['warped'] += moved and len(pool) > 0
        ev['warp_unconfirmed'] += moved * len(unconf)

        # first association: pool x high detections, fused distance
        iou = T.iou32(self._tlbr32(pool), dbox[hi])
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
        x2 = self._assign(f32(1) - T.iou32(self._tlbr32(rest), dbox[lo]), 0.5)
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
        iou = T.iou32(self._tlbr32(unconf), dbox[left])
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
            mean[s], cov[s] = kf['initiate'](kf['z'](d[j, :4]))
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


# ---------------------------------------------------------------------------------------------------- seeded scenes under a moving camera
def camera_path(seed, frames, pan=(3.0, 1.5), rot_deg=0.15, scale=0.002, jumps=(), aniso=0.0, size=(1080, 1920)):
    """Frame-to-frame warps of a camera that pans steadily, rotates and zooms a little about the image centre and jumps:
    -> f64 [frames, 2, 3]; warp[f] maps frame f-1's pixel coordinates to frame f's (warp[0] is identity).  jumps: {frame: (dx, dy)};
    aniso stretches x against y (a warp that is no similarity, as ours are in original pixels when sx != sy)."""
    rng = np.random.default_rng(seed)
    Hh, W = size
    c = np.array([W / 2, Hh / 2])
    out = np.zeros((frames, 2, 3))
    out[0] = np.eye(2, 3)
    jumps = dict(jumps)
    for f in range(1, frames):
        a = np.deg2rad(rng.uniform(-rot_deg, rot_deg))
        s = 1 + rng.uniform(-scale, scale)
        R = s * np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]) @ np.diag([1 + aniso, 1 - aniso])
        t = np.array(pan) + rng.normal(0, 0.3, 2) + np.array(jumps.get(f, (0, 0)))
        out[f, :, :2] = R
        out[f, :, 2] = c - R @ c + t
    return out


def through_camera(scene, warps):
    """World-frame detections (bytetrack_np.make_scene) as the moving camera sees them: a box keeps its size, its centre goes through
    the accumulated warps.  -> list of f32 [n, 6]."""
    out, A = [], np.eye(3)
    for fr, H in zip(scene, warps):
        A = np.vstack([H, [0, 0, 1]]) @ A
        d = np.asarray(fr, np.float64).copy()
        if len(d):
            c = np.stack([(d[:, 0] + d[:, 2]) / 2, (d[:, 1] + d[:, 3]) / 2, np.ones(len(d))], 1) @ A[:2].T
            w, h = d[:, 2] - d[:, 0], d[:, 3] - d[:, 1]
            d[:, 0], d[:, 1], d[:, 2], d[:, 3] = c[:, 0] - w / 2, c[:, 1] - h / 2, c[:, 0] + w / 2, c[:, 1] + h / 2
        out.append(d.astype(f32))
    return out
