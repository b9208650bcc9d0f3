"""Shared by test_coco_host.py and test_gpu_coco.py: the hand-worked cases of the COCO protocol with their expected twelve numbers, and a
literal restatement of the rule (the walk over ground truths, step by step, in Python loops) that engine.coco_evaluate's vectorised
arg-max is checked against.

The twelve numbers are in the order AP, AP50, AP75, APs, APm, APl, AR1, AR10, AR100, ARs, ARm, ARl.  Boxes are x1 y1 x2 y2 in pixels; every
coordinate is a multiple of 1/4 below 512, so the normalised xywh labels of side 512 reproduce them exactly in fp32.
pr of a true positive with no false positive before it is 1 / (1 + 2.2e-16) = 1 - 2.2e-16, which the expected values below write as 1:
the bound is 1e-12."""
import numpy as np

F = np.float32
KEYS = ('AP', 'AP50', 'AP75', 'APs', 'APm', 'APl', 'AR1', 'AR10', 'AR100', 'ARs', 'ARm', 'ARl')
SIDE = 512
T = np.linspace(0.5, 0.95, 10)
R = np.linspace(0.0, 1.0, 101)
AREAS = ((0.0, 1e10), (0.0, 32.0 ** 2), (32.0 ** 2, 96.0 ** 2), (96.0 ** 2, 1e10))
NAN = float('nan')

# name -> (nc, max_dets, images, expected); images = [(dets [x1 y1 x2 y2 score cls], labels [cls x1 y1 x2 y2])]
HAND = {}

# A (from the issue).  Two ground truths of 1600 px^2 (medium), one detection equal to the first: tp = [1], rc = [0.5], pr = [1] at every
# threshold; precision is 1 at the 51 grid points <= 0.5 and 0 after: AP = 51/101; recall 0.5.  Nothing is small or large.
HAND['A'] = (1, (1, 10, 100), [([[0, 0, 40, 40, .9, 0]], [[0, 0, 0, 40, 40], [0, 100, 0, 140, 40]])],
             [51 / 101, 51 / 101, 51 / 101, -1, 51 / 101, -1, .5, .5, .5, -1, .5, -1])

# B (from the issue).  The first detection has IoU 0.77 with the first ground truth: a hit at 0.5 .. 0.75 (6 thresholds), where the second
# detection is then false: tp = [1, 1, 2], fp = [0, 1, 1], pr = [1, 1/2, 2/3] -> envelope [1, 2/3, 2/3]: 51 points of 1 and 50 of 2/3 =
# 253/303.  Above 0.77 it is false and the second detection hits: pr = [0, 1/2, 2/3] -> 2/3 everywhere.  In "large" its 7700 px^2 is outside
# the range, so there it is ignored instead of false: pr = [-, 1, 1] -> 1.
HAND['B'] = (1, (1, 10, 100), [([[0, 0, 100, 77, .9, 0], [0, 0, 100, 100, .8, 0], [200, 0, 300, 100, .7, 0]],
                                [[0, 0, 0, 100, 100], [0, 200, 0, 300, 100]])],
             [(6 * (253 / 303) + 4 * (2 / 3)) / 10, 253 / 303, 253 / 303, -1, -1, (6 * (253 / 303) + 4) / 10, .3, 1, 1, -1, -1, 1])

# An ignored ground truth is taken only when no non-ignored one qualifies.  Detection = the 1600 px^2 ground truth (IoU 1), and IoU
# 1000 / 1600 = 0.625 with the 1000 px^2 one.  "all": it takes the IoU-1 one at every threshold: tp = [1] of npig 2 -> 51/101, recall 0.5.
# "small": the big one is ignored there; at 0.5, 0.55, 0.6 the small one qualifies and is taken (a true positive: AP_t = 1, recall 1); from
# 0.65 on only the ignored one qualifies, the detection becomes ignored, no row counts: AP_t = 0, recall 0: APs = ARs = 0.3.
# "medium": the small one is ignored, the detection takes the big one everywhere: 1.
HAND['ignored_last'] = (1, (1, 10, 100), [([[0, 0, 40, 40, .9, 0]], [[0, 0, 0, 40, 25], [0, 0, 0, 40, 40]])],
                        [51 / 101, 51 / 101, 51 / 101, .3, 1, -1, .5, .5, .5, .3, 1, -1])

# IoU exactly 0.5 = 50 / ((50 + 100) - 50): a hit at 0.5 and at no other threshold.  One ground truth: AP_0.5 = 1, the other nine 0.
HAND['iou_half'] = (1, (1, 10, 100), [([[0, 0, 10, 5, .9, 0]], [[0, 0, 0, 10, 10]])], [.1, 1, 0, .1, -1, -1, .1, .1, .1, .1, -1, -1])

# Equal IoUs: the LATER ground truth wins.  Detection 1 has IoU 72.5 / 100 = 0.725 with both ground truths (hits at 0.5 .. 0.7); detection 2
# equals the FIRST ground truth and has IoU 0.45 with the second.  Detection 1 takes the second, so detection 2 finds the first free:
# at 0.5 .. 0.7 both hit (AP_t = 1, recall 1); from 0.75 on detection 1 is false and detection 2 hits: tp = [0, 1] of npig 2, rc = [0, 1/2],
# pr = [0, 1/2] -> 1/2 at the 51 grid points <= 1/2: AP_t = 51/202, recall 1/2.  AP = (5 + 5 * 51/202) / 10; AP75 = 51/202;
# AR10 = AR100 = (5 + 5/2) / 10.  Cut 1 keeps detection 1 only: recall 1/2 at five thresholds, 0 at five: AR1 = 1/4.
# (Were the earlier one taken, detection 2 would be false at 0.5 .. 0.7 too and AP50 would be 51/101.)
HAND['later_wins'] = (1, (1, 10, 100), [([[0, 0, 10, 10, .9, 0], [0, 0, 10, 7.25, .8, 0]], [[0, 0, 0, 10, 7.25], [0, 0, 2.75, 10, 10]])],
                      [(5 + 5 * 51 / 202) / 10, 1, 51 / 202, (5 + 5 * 51 / 202) / 10, -1, -1, .25, .75, .75, .75, -1, -1])

# 32 x 32 = 1024 px^2 is inside both [0, 1024] and [1024, 9216].
HAND['area_1024'] = (1, (1, 10, 100), [([[0, 0, 32, 32, .9, 0]], [[0, 0, 0, 32, 32]])], [1, 1, 1, 1, 1, -1, 1, 1, 1, 1, 1, -1])

# max_dets (1, 2) and three detections of one class: the third, equal to the second ground truth, is beyond the last cut, takes part in
# nothing and leaves that ground truth unmatched.  Cut 2: rows [false, hit]: pr = [0, 1/2] -> 1/2, rc = [0, 1/2]: 51 points of 1/2:
# AP = 51/202, recall 1/2.  Cut 1: the false one only: AR1 = 0.  The second cut is reported as "AR10", a third there is not: -1.
HAND['beyond_max_dets'] = (1, (1, 2), [([[50, 0, 60, 10, .9, 0], [0, 0, 10, 10, .8, 0], [20, 0, 30, 10, .7, 0]],
                                         [[0, 0, 0, 10, 10], [0, 20, 0, 30, 10]])],
                           [51 / 202, 51 / 202, 51 / 202, 51 / 202, -1, -1, 0, .5, -1, .5, -1, -1])

# Class 0: one ground truth, one exact detection: AP 1.  Class 1: a detection and no ground truth: npig 0, every entry -1, left out of
# every mean.  Class 2: a ground truth and no detection: recall 0 and AP 0, NOT -1.  Mean over classes 0 and 2: 1/2.
HAND['classes_without'] = (3, (1, 10, 100), [([[0, 0, 40, 40, .9, 0], [0, 0, 40, 40, .8, 1]], [[0, 0, 0, 40, 40], [2, 0, 0, 50, 50]])],
                           [.5, .5, .5, -1, .5, -1, .5, .5, .5, -1, .5, -1])

# The second image has no labels: its detection is a false positive, and with the higher score it comes first: pr = [0, 1/2] -> 1/2.
# Ranks are per image, so both rows are inside cut 1: recall 1 everywhere.
HAND['image_without_labels'] = (1, (1, 10, 100), [([[0, 0, 40, 40, .5, 0]], [[0, 0, 0, 40, 40]]), ([[0, 0, 40, 40, .9, 0]], [])],
                                [.5, .5, .5, -1, .5, -1, 1, 1, 1, -1, 1, -1])

# No live row in the whole run: the class has ground truth and no detection: 0, not -1.
HAND['no_rows'] = (1, (1, 10, 100), [([], [[0, 0, 0, 40, 40]])], [0, 0, 0, -1, 0, -1, 0, 0, 0, -1, 0, -1])

# Labels of class 5 and -1 and rows of class 7 and -3 with nc = 2 take part in nothing (they would otherwise add a missed ground truth
# and two false positives of higher score); class 1 has neither ground truth nor detection: -1.
HAND['out_of_range'] = (2, (1, 10, 100), [([[0, 0, 40, 40, .99, 7], [0, 0, 40, 40, .95, -3], [0, 0, 40, 40, .9, 0]],
                                           [[5, 0, 0, 40, 40], [0, 0, 0, 40, 40], [-1, 0, 0, 40, 40]])],
                        [1, 1, 1, -1, 1, -1, 1, 1, 1, -1, 1, -1])

# A NaN-score row takes part in nothing: not a false positive, and it does not take the ground truth.
HAND['nan_score'] = (1, (1, 10, 100), [([[0, 0, 40, 40, NAN, 0], [0, 0, 40, 40, .9, 0]], [[0, 0, 0, 40, 40]])],
                     [1, 1, 1, -1, 1, -1, 1, 1, 1, -1, 1, -1])


# Where COCO's greedy rule and the validator's `correct` table part: detection 2 overlaps the first ground truth best (9000 / 10500 = 0.857)
# but detection 1 (exact, more confident) holds it; its second choice has IoU 8500 / 11000 = 0.773.  COCO gives it that one at 0.5 .. 0.75;
# the `correct` table, which lets every detection claim only its best label, leaves it false at every threshold.
SECOND_CHOICE = [([[0, 0, 100, 100, .9, 0], [0, 10, 100, 105, .8, 0]], [[0, 0, 0, 100, 100], [0, 0, 20, 100, 120]])]


def arrays(images):
    """The hand case's images as (det f32 [n, 6], lab f32 [m, 5]) arrays."""
    return [(np.array(d, F).reshape(-1, 6), np.array(g, F).reshape(-1, 5)) for d, g in images]


def literal(images, nc, max_dets):
    """The rule of the issue, step by step: -> (precision [10, 101, nc, 4, M], recall [10, nc, 4, M], per image (bits [n, 4], rank [n]),
    npig [nc, 4]).  Python loops throughout; for small cases."""
    md = tuple(max_dets)
    rows = []                                       # (class, score, image, row, bits[4])
    npig = np.zeros((nc, 4), np.int64)
    matches = []
    for im, (det, lab) in enumerate(images):
        det, lab = np.asarray(det, F).reshape(-1, 6), np.asarray(lab, F).reshape(-1, 5)
        bits, rank = np.zeros((len(det), 4), np.int32), np.full(len(det), -1, np.int32)

        def cls_of(c):
            return int(np.trunc(c)) if c == c and 0 <= np.trunc(c) < nc else -1

        dcls = [cls_of(c) if s == s else -1 for c, s in zip(det[:, 5], det[:, 4])]
        gcls = [cls_of(c) for c in lab[:, 0]]
        box = lambda v: [float(x) for x in v]       # noqa: E731  (fp32 -> Python double)
        area = lambda b: (b[2] - b[0]) * (b[3] - b[1])   # noqa: E731

        def iou(d, g):
            iw, ih = min(d[2], g[2]) - max(d[0], g[0]), min(d[3], g[3]) - max(d[1], g[1])
            if iw <= 0 or ih <= 0:
                return 0.0
            i = iw * ih
            u = (area(d) + area(g)) - i
            return 0.0 if u <= 0 else i / u

        for k in range(nc):
            dk = sorted([i for i in range(len(det)) if dcls[i] == k], key=lambda i: -det[i, 4])    # sorted() is stable
            for r, i in enumerate(dk):
                rank[i] = r
            dk = dk[:md[-1]]
            gk = [j for j in range(len(lab)) if gcls[j] == k]
            for a, (lo, hi) in enumerate(AREAS):
                outside = lambda b: area(b) < lo or area(b) > hi    # noqa: E731
                ign = {j: outside(box(lab[j, 1:])) for j in gk}
                npig[k, a] += sum(not v for v in ign.values())
                order = [j for j in gk if not ign[j]] + [j for j in gk if ign[j]]
                for t in range(10):
                    taken = set()
                    for i in dk:
                        best, m = min(T[t], 1 - 1e-10), None
                        for j in order:
                            if j in taken:
                                continue
                            if m is not None and not ign[m] and ign[j]:
                                break
                            v = iou(box(det[i, :4]), box(lab[j, 1:]))
                            if v < best:
                                continue
                            best, m = v, j
                        if m is not None:
                            taken.add(m)
                            bits[i, a] |= (1 << t) | (int(ign[m]) << (16 + t))
                        elif outside(box(det[i, :4])):
                            bits[i, a] |= 1 << (16 + t)
            rows += [(k, float(det[i, 4]), im, i, rank[i], bits[i]) for i in range(len(det)) if dcls[i] == k]
        matches.append((bits, rank))
    precision, recall = -np.ones((10, 101, nc, 4, len(md))), -np.ones((10, nc, 4, len(md)))
    for k in range(nc):
        for a in range(4):
            if npig[k, a] == 0:
                continue
            for mi, cut in enumerate(md):
                sel = sorted([r for r in rows if r[0] == k and r[4] < cut], key=lambda r: -r[1])
                for t in range(10):
                    tp = fp = 0
                    rc, pr = [], []
                    for r in sel:
                        w = int(r[5][a])
                        matched, ignored = (w >> t) & 1, (w >> (16 + t)) & 1
                        tp += int(matched and not ignored)
                        fp += int(not matched and not ignored)
                        rc.append(tp / int(npig[k, a]))
                        pr.append(tp / ((fp + tp) + 2.220446049250313e-16))
                    for i in range(len(pr) - 2, -1, -1):
                        pr[i] = max(pr[i], pr[i + 1])
                    recall[t, k, a, mi] = rc[-1] if rc else 0.0
                    for ri, x in enumerate(R):
                        first = next((i for i, v in enumerate(rc) if v >= x), None)
                        precision[t, ri, k, a, mi] = pr[first] if first is not None else 0.0
    return precision, recall, matches, npig


def random_images(seed, n_images, nc, n_det, n_lab, levels=None):
    """Images in pixels with boxes of 8 .. 150 px on a 1/4 grid (exact ties of IoU happen): clustered detections, classes mostly right."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_images):
        m = int(rng.integers(0, n_lab + 1))
        xy = rng.integers(0, 1200, (m, 2)) / 4
        wh = np.exp(rng.uniform(np.log(8), np.log(150), (m, 2))).round()
        lab = np.concatenate([rng.integers(-1, nc + 1, (m, 1)), xy, xy + wh], 1).astype(F)
        n = int(rng.integers(0, n_det + 1))
        if m:
            src = rng.integers(0, m, n)
            jit = rng.integers(-2, 3, (n, 4)) * np.maximum(wh[src].min(1, keepdims=True) // 12, 1) / 2
            box = lab[src, 1:] + jit
            cls = np.where(rng.random(n) < 0.8, lab[src, 0], rng.integers(0, nc, n))
        else:
            box = np.concatenate([xy := rng.integers(0, 300, (n, 2)), xy + rng.integers(8, 100, (n, 2))], 1)
            cls = rng.integers(0, nc, n)
        score = rng.integers(1, levels, n) / levels if levels else rng.permutation(n) / max(n, 1) * 0.9 + 0.05
        order = np.argsort(-score, kind='stable')
        det = np.concatenate([box, score[:, None], cls[:, None]], 1).astype(F)[order]
        out.append((det, lab))
    return out


def sized_case(B, nq, nc, labels_per_image, seed, hw=None, imgsz=640, bf16=False, shuffle_labels=False):
    """test_val_host.make_case with the label sides drawn in PIXELS, log-uniform over 10 .. 200 px of the image the labels live in (hw[b],
    or imgsz square), so that the small, medium and large ranges all have ground truths whatever the image size.  y [B, nq, 4 + nc] fp32
    (every value on the bf16 grid when bf16) and host labels; detections cluster on the image's first 24 labels with the label's class
    four times out of five; the row maxima are pairwise distinct inside an image, also after rounding to bf16."""
    from test_val_host import to_bf16_grid
    rng = np.random.default_rng(seed)
    cls, boxes, bidx = [], [], []
    y = np.zeros((B, nq, 4 + nc), F)
    for b in range(B):
        L = labels_per_image[b % len(labels_per_image)]
        h, w = hw[b] if hw is not None else (imgsz, imgsz)
        side = np.exp(rng.uniform(np.log(10), np.log(200), (L, 2))) / np.array([w, h])
        lb = np.concatenate([rng.uniform(0.15, 0.85, (L, 2)), np.minimum(side, 0.28)], 1).astype(F)
        lc = rng.integers(0, nc, L).astype(F)
        cls.append(lc), boxes.append(lb), bidx.append(np.full(L, b, F))
        if L:
            src = rng.integers(0, min(L, 24), nq)
            ctr, want = lb[src], lc[src].astype(np.int64)
        else:
            ctr = np.concatenate([rng.uniform(0.2, 0.8, (nq, 2)), rng.uniform(0.05, 0.3, (nq, 2))], 1).astype(F)
            want = rng.integers(0, nc, nq)
        y[b, :, :2] = ctr[:, :2] + rng.normal(0, 0.03, (nq, 2)) * ctr[:, 2:]
        y[b, :, 2:4] = ctr[:, 2:] * rng.uniform(0.85, 1.15, (nq, 2))
        if bf16:    # distinct values of the bf16 grid in [2^-9, 1)
            grid = (np.arange(0x3b00, 0x3f80, dtype=np.uint32) << 16).view(F)
            top = rng.choice(grid, nq, replace=False)
        else:
            top = (rng.permutation(nq) + rng.uniform(0.1, 0.9, nq)) / nq * 0.97 + 0.002
        wrong = rng.random(nq) < 0.2
        want = np.where(wrong, rng.integers(0, nc, nq), want)
        y[b, :, 4:] = top[:, None] * rng.uniform(0.05, 0.45, (nq, nc))
        y[b, np.arange(nq), 4 + want] = top
    y = to_bf16_grid(y) if bf16 else y
    cls, boxes, bidx = np.concatenate(cls), np.concatenate(boxes), np.concatenate(bidx)
    if shuffle_labels and len(cls):
        p = rng.permutation(len(cls))
        cls, boxes, bidx = cls[p], boxes[p], bidx[p]
    import torch
    return y, torch.from_numpy(cls).view(-1, 1), torch.from_numpy(boxes), torch.from_numpy(bidx)


def to_xywh(lab):
    """Labels cls x1 y1 x2 y2 (pixels, multiples of 1/4 below SIDE) -> cls [m], normalised xywh [m, 4] of side SIDE, exact in fp32."""
    lab = np.asarray(lab, F).reshape(-1, 5)
    xy = lab[:, 1:]
    out = np.stack([(xy[:, 0] + xy[:, 2]) / 2, (xy[:, 1] + xy[:, 3]) / 2, xy[:, 2] - xy[:, 0], xy[:, 3] - xy[:, 1]], 1) / F(SIDE)
    return lab[:, 0].copy(), out.astype(F)
