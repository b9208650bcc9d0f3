"""The numpy statement of the camera-motion estimate (csrc/gmc.hip, whose header writes the rule out): grey, pyramid and keypoints in
integer / fp32 numpy op by op, pyramidal LK written once with a `dtype` argument, the fit in fp64 in the kernel's operation order,
the pairing over a batch, and make_frames, which draws sequences with known frame-to-frame warps.  Test infrastructure only."""
import numpy as np

SLOTS, HYP, WIN, ITERS = 1024, 512, 10, 10
IDENTITY = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])


def n_levels(H, W):
    m, L = min(H, W) // 32, 1
    while L < 4 and (m >> L):
        L += 1
    return L


def grey(rgb):
    """u8 [H, W, 3] -> u8 [H, W]"""
    c = rgb.astype(np.int32)
    return ((77 * c[..., 0] + 150 * c[..., 1] + 29 * c[..., 2] + 128) >> 8).astype(np.uint8)


def pyr_down(img):
    p = np.pad(img.astype(np.int32), 2, mode='reflect')
    w = (1, 4, 6, 4, 1)
    H, W = img.shape
    rows = sum(w[i] * p[:, i:i + W] for i in range(5))
    full = sum(w[j] * rows[j:j + H] for j in range(5))
    return ((full[::2, ::2] + 128) >> 8).astype(np.uint8)


def pyramid(g0):
    out = [g0]
    for _ in range(n_levels(*g0.shape) - 1):
        out.append(pyr_down(out[-1]))
    return out


def corner_response(g0):
    """fp32 [H, W]: the smaller eigenvalue of the 3x3-summed structure tensor of the Sobel derivatives, 0 within 2 px of the border."""
    g = g0.astype(np.int32)
    H, W = g.shape
    gx, gy = np.zeros((H, W), np.int32), np.zeros((H, W), np.int32)
    gx[1:-1, 1:-1] = (g[:-2, 2:] + 2 * g[1:-1, 2:] + g[2:, 2:]) - (g[:-2, :-2] + 2 * g[1:-1, :-2] + g[2:, :-2])
    gy[1:-1, 1:-1] = (g[2:, :-2] + 2 * g[2:, 1:-1] + g[2:, 2:]) - (g[:-2, :-2] + 2 * g[:-2, 1:-1] + g[:-2, 2:])

    def box(v):
        return sum(v[j:H - 2 + j, i:W - 2 + i] for j in range(3) for i in range(3))
    a, b, c = (box(v).astype(np.float32) for v in (gx * gx, gx * gy, gy * gy))      # the sums are exact in int32 and in fp32
    tr, d = a + c, a - c
    t = np.float32(4.0) * b
    t = t * b
    inner = (tr - np.sqrt(d * d + t)) * np.float32(0.5)
    lam = np.zeros((H, W), np.float32)
    lam[2:-2, 2:-2] = inner[1:-1, 1:-1]
    return lam


def keypoints(lam):
    """i32 [1024]: per cell of the 32 x 32 grid the pixel index of its strongest pixel, -1 where none passes."""
    H, W = lam.shape
    thr = np.float32(0.01) * lam.max()
    kp = np.full(SLOTS, -1, np.int32)
    for cy in range(32):
        y0, y1 = (cy * H + 31) // 32, ((cy + 1) * H + 31) // 32
        for cx in range(32):
            x0, x1 = (cx * W + 31) // 32, ((cx + 1) * W + 31) // 32
            blk = lam[y0:y1, x0:x1]
            ok = (blk > 0) & (blk >= thr)
            if ok.any():
                i = int(np.argmax(np.where(ok, blk, np.float32(-1))))      # argmax: the first of equals = the lowest pixel index
                kp[cy * 32 + cx] = (y0 + i // (x1 - x0)) * W + x0 + i % (x1 - x0)
    return kp


def _bil(P, x, y, dt):
    h, w = P.shape
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = x - x0, y - y0
    with np.errstate(invalid='ignore'):
        ix = np.clip(np.nan_to_num(x0, nan=0.0, posinf=1e9, neginf=-1e9), -1, w).astype(np.int64)
        iy = np.clip(np.nan_to_num(y0, nan=0.0, posinf=1e9, neginf=-1e9), -1, h).astype(np.int64)
    xa, xb, ya, yb = np.clip(ix, 0, w - 1), np.clip(ix + 1, 0, w - 1), np.clip(iy, 0, h - 1), np.clip(iy + 1, 0, h - 1)
    a, b, c, d = (P[r, q].astype(dt) for r, q in ((ya, xa), (ya, xb), (yb, xa), (yb, xb)))
    top, bot = a + fx * (b - a), c + fx * (d - c)
    return top + fy * (bot - top)


def lk(prev_pyr, cur_pyr, kp, dtype=np.float64):
    """kp i32 [1024] on the previous frame -> pts dtype [1024, 4] (px py cx cy) and status i32 [1024] (0 empty, 1 lost, 2 tracked)."""
    dt = np.dtype(dtype).type
    H, W = prev_pyr[0].shape
    L = len(prev_pyr)
    live = kp >= 0
    k = np.where(live, kp, 0)
    px0, py0 = (k % W).astype(dt), (k // W).astype(dt)
    dx = (np.arange(441) % 21 - 10).astype(dt)[None]
    dy = (np.arange(441) // 21 - 10).astype(dt)[None]
    gx, gy = np.zeros(SLOTS, dt), np.zeros(SLOTS, dt)
    ok = np.ones(SLOTS, bool)
    one, half, four = dt(1), dt(0.5), dt(4)
    with np.errstate(all='ignore'):
        for l in range(L - 1, -1, -1):
            sc = dt(1.0 / (1 << l))
            P, C = prev_pyr[l], cur_pyr[l]
            x, y = (px0 * sc)[:, None] + dx, (py0 * sc)[:, None] + dy
            I = _bil(P, x, y, dt)
            Ix = (_bil(P, x + one, y, dt) - _bil(P, x - one, y, dt)) * half
            Iy = (_bil(P, x, y + one, dt) - _bil(P, x, y - one, dt)) * half
            gxx, gxy, gyy = (Ix * Ix).sum(1, dtype=dt), (Ix * Iy).sum(1, dtype=dt), (Iy * Iy).sum(1, dtype=dt)
            det = gxx * gyy - gxy * gxy
            tr, d = gxx + gyy, gxx - gyy
            t = four * gxy
            t = t * gxy
            lmin = (tr - np.sqrt(d * d + t)) * half
            ok &= (lmin / dt(441) >= one)
            vx, vy = np.zeros(SLOTS, dt), np.zeros(SLOTS, dt)
            for _ in range(ITERS):
                df = I - _bil(C, x + (gx + vx)[:, None], y + (gy + vy)[:, None], dt)
                bx, by = (df * Ix).sum(1, dtype=dt), (df * Iy).sum(1, dtype=dt)
                vx = vx + (gyy * bx - gxy * by) / det
                vy = vy + (gxx * by - gxy * bx) / det
            if l > 0:
                gx, gy = dt(2) * (gx + vx), dt(2) * (gy + vy)
            else:
                gx, gy = gx + vx, gy + vy
        cx, cy = px0 + gx, py0 + gy
        ok &= (cx >= 0) & (cx <= W - 1) & (cy >= 0) & (cy <= H - 1)
    pts = np.stack([px0, py0, cx, cy], 1)
    pts[~live] = 0
    return pts, np.where(live, np.where(ok, 2, 1), 0).astype(np.int32)


def _mix(x):
    x &= 0xffffffff
    x ^= x >> 16
    x = (x * 0x7feb352d) & 0xffffffff
    x ^= x >> 15
    x = (x * 0x846ca68b) & 0xffffffff
    x ^= x >> 16
    return x


def hypothesis(k, n):
    i = _mix((2 * k) * 0x9E3779B9 + n) % n
    j = _mix((2 * k + 1) * 0x9E3779B9 + n) % (n - 1)
    return i, j + (j >= i)


def _seqsum(v):
    return np.cumsum(v)[-1] if len(v) else np.float64(0)      # cumsum adds in index order, as the kernel's loop


def fit(src, dst):
    """src, dst f64 [n, 2] (already in original pixels) -> warp f64 [2, 3], chosen k (-1: none), inlier mask bool [n], used."""
    n = len(src)
    if n <= 4:
        return IDENTITY.copy(), -1, np.zeros(n, bool), 0
    X, Y, U, V = src[:, 0], src[:, 1], dst[:, 0], dst[:, 1]

    def model(k):
        i, j = hypothesis(k, n)
        dx, dy, ex, ey = X[j] - X[i], Y[j] - Y[i], U[j] - U[i], V[j] - V[i]
        den = dx * dx + dy * dy
        if not den > 0:
            return None
        a, b = (dx * ex + dy * ey) / den, (dx * ey - dy * ex) / den
        return a, b, U[i] - (a * X[i] - b * Y[i]), V[i] - (b * X[i] + a * Y[i])

    def inliers(m):
        a, b, tx, ty = m
        rx, ry = ((a * X - b * Y) + tx) - U, ((b * X + a * Y) + ty) - V
        return rx * rx + ry * ry <= 9.0
    best, bk = 0, 0
    for k in range(HYP):
        m = model(k)
        c = int(inliers(m).sum()) if m is not None else 0
        if k == 0 or c > best:
            best, bk = c, k
    if best == 0:
        return IDENTITY.copy(), bk, np.zeros(n, bool), 0
    m, out = model(bk), None
    for rnd, thr in enumerate((9.0, 1.0)):      # the winner's inliers at 3 px, then the refit's own at 1 px
        a, b, tx, ty = m
        rx, ry = ((a * X - b * Y) + tx) - U, ((b * X + a * Y) + ty) - V
        mask = rx * rx + ry * ry <= thr
        cnt = int(mask.sum())
        if cnt <= (4 if rnd else 0):
            break
        mx, my, mu, mv = (_seqsum(v[mask]) / cnt for v in (X, Y, U, V))
        x, y, u, v = X[mask] - mx, Y[mask] - my, U[mask] - mu, V[mask] - mv
        sxx, sa, sb = _seqsum(x * x + y * y), _seqsum(x * u + y * v), _seqsum(x * v - y * u)
        if not sxx > 0:
            break
        a, b = sa / sxx, sb / sxx
        m = (a, b, mu - (a * mx - b * my), mv - (b * mx + a * my))
        out = (np.array([[a, -b, m[2]], [b, a, m[3]]]), bk, mask, 1)
    return out if out is not None else (IDENTITY.copy(), bk, np.zeros(n, bool), 0)


def fit_pairs(pts, status, scale=(1.0, 1.0)):
    """The kernel's fit stage on LK's output: the tracked pairs in slot order, the warp scaled.  -> warp, (tracked, inliers, used), k, mask."""
    sel = status == 2
    p = pts[sel].astype(np.float64)
    sx, sy = float(scale[0]), float(scale[1])
    w, k, mask, used = fit(p[:, :2], p[:, 2:])      # in network pixels; out in original pixels as D W D^-1
    warp = np.array([[w[0, 0], (w[0, 1] * sx) / sy, w[0, 2] * sx], [(w[1, 0] * sy) / sx, w[1, 1], w[1, 2] * sy]])
    return warp, (int(sel.sum()), int(mask.sum()) if used else 0, used), k, mask


class GmcNp:
    """The whole estimate with its persistent state: estimate(frames u8 [B, H, W, 3], counts, scale [B, 2]) -> warps [B, 2, 3], stats [B, 4]."""

    def __init__(self, dtype=np.float64):
        self.dtype, self.prev = dtype, None      # prev: (pyramid, keypoint slots) of the last frame that reached the tracker

    def reset(self):
        self.prev = None

    def estimate(self, frames, counts, scale=None):
        B = len(frames)
        scale = np.ones((B, 2)) if scale is None else np.asarray(scale, np.float64)
        warps, stats = np.tile(IDENTITY, (B, 1, 1)), np.zeros((B, 4), np.int32)
        self.pairs = []
        for b in range(B):
            if counts[b] <= 0:
                self.pairs.append(None)
                continue
            pyr = pyramid(grey(frames[b]))
            cur = (pyr, keypoints(corner_response(pyr[0])))
            self.pairs.append(None if self.prev is None else self.prev[2])
            if self.prev is not None:
                pts, status = lk(self.prev[0], pyr, self.prev[1], self.dtype)
                warps[b], (tracked, inl, used), _, _ = fit_pairs(pts, status, scale[b])
                stats[b] = (int((status > 0).sum()), tracked, inl, used)
            self.prev = cur + (b,)
        if self.prev is not None and self.prev[2] != 'state':
            self.prev = self.prev[:2] + ('state',)
        return warps, stats


# ------------------------------------------------------------------------------------------------ drawn sequences
def similarity(tx, ty, deg=0.0, s=1.0, centre=(0.0, 0.0)):
    """The 2x3 warp x -> s R (x - c) + c + t."""
    c, si = s * np.cos(np.deg2rad(deg)), s * np.sin(np.deg2rad(deg))
    R = np.array([[c, -si], [si, c]])
    cc = np.asarray(centre, np.float64)
    return np.concatenate([R, (cc - R @ cc + (tx, ty))[:, None]], 1)


def _smooth(a, r):
    k = np.ones(2 * r + 1) / (2 * r + 1)
    for ax in (0, 1):
        a = np.apply_along_axis(lambda v: np.convolve(v, k, mode='same'), ax, a)
    return a


def _texture(rng, n):
    t = _smooth(rng.standard_normal((n, n)), 1) * 3.0 + _smooth(rng.standard_normal((n, n)), 4) * 9.0
    t = (t - t.mean()) / t.std()
    return np.clip(128 + 48 * t, 0, 255)


def _sample(img, x, y):
    h, w = img.shape
    x, y = np.clip(x, 0, w - 1.001), np.clip(y, 0, h - 1.001)
    x0, y0 = np.floor(x).astype(int), np.floor(y).astype(int)
    fx, fy = x - x0, y - y0
    return (img[y0, x0] * (1 - fx) + img[y0, x0 + 1] * fx) * (1 - fy) + (img[y0 + 1, x0] * (1 - fx) + img[y0 + 1, x0 + 1] * fx) * fy


def make_frames(seed, S, n, motions, movers=0):
    """n frames u8 [n, S, S, 3] of a seeded textured scene (smoothed noise at two scales) seen by a moving camera, and the true
    frame-to-frame warps f64 [n, 2, 3] (warp t maps frame t-1's pixels to frame t's; warp 0 is the identity).  motions: n - 1 warps
    (2x3).  The scene is resampled with fp64 bilinear interpolation.  movers: that many textured rectangles, together about a quarter
    of the frame, that move on their own, 4 to 7 px a frame in x and in y against the background: outliers."""
    rng = np.random.default_rng(seed)
    pad = S // 2
    scene = _texture(rng, S + 2 * pad)
    chans = np.stack([scene, np.roll(scene, 1, 0) * 0.5 + scene * 0.5, np.roll(scene, 1, 1) * 0.5 + scene * 0.5], -1)
    yy, xx = np.mgrid[0:S, 0:S].astype(np.float64)
    A = np.vstack([similarity(pad, pad), [0, 0, 1]])      # frame pixel -> scene pixel
    side = int(S * np.sqrt(0.25 / max(movers, 1)))
    boxes = [[rng.uniform(0.15 * S, 0.85 * S - side, 2), rng.uniform(4, 7, 2) * rng.choice([-1, 1], 2), _texture(rng, side)] for _ in range(movers)]
    frames, warps = np.zeros((n, S, S, 3), np.uint8), np.tile(IDENTITY, (n, 1, 1))
    for t in range(n):
        if t:
            M = np.vstack([np.asarray(motions[t - 1], np.float64), [0, 0, 1]])
            warps[t] = M[:2]
            A = A @ np.linalg.inv(M)
        sx, sy = A[0, 0] * xx + A[0, 1] * yy + A[0, 2], A[1, 0] * xx + A[1, 1] * yy + A[1, 2]
        img = np.stack([_sample(chans[..., c], sx, sy) for c in range(3)], -1)
        for box in boxes:      # a mover goes with the camera's warp and adds its own velocity: at least 4 px a frame off the background
            if t:
                box[0] = warps[t, :, :2] @ box[0] + warps[t, :, 2] + box[1]
            x0, y0 = (int(round(v)) for v in np.clip(box[0], 0, S - side))
            tex = box[2]
            img[y0:y0 + side, x0:x0 + side] = tex[..., None]
        frames[t] = np.clip(np.rint(img), 0, 255).astype(np.uint8)
    return frames, warps


def corner_error(warp, truth, H, W):
    """The largest distance between the images of the four frame corners under the two warps."""
    c = np.array([[0, 0, 1], [W - 1, 0, 1], [0, H - 1, 1], [W - 1, H - 1, 1]], np.float64).T
    return float(np.sqrt((((np.asarray(warp) - np.asarray(truth)) @ c) ** 2).sum(0)).max())


def random_motions(seed, n, max_t=12.0, max_deg=2.0, max_s=0.02, S=256):
    rng = np.random.default_rng(seed)
    return [similarity(*rng.uniform(-max_t, max_t, 2), rng.uniform(-max_deg, max_deg), 1 + rng.uniform(-max_s, max_s), centre=(S / 2, S / 2))
            for _ in range(n)]
