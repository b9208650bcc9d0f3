#!/usr/bin/env python3
"""Generate tests/golden/confusion.npz by running the *reference's* ConfusionMatrix.process_batch (ultralytics/utils/metrics.py:801-877)
on the CPU over seeded single-image cases.  Runs only where the reference is present; the import recipe is make_golden.py's.

    python tests/golden/make_confusion_golden.py

What is stored (data only): per case k the detections `det{k}` f32 [N, 6] (xyxy, score, cls; absent for the `detections=None` form),
the labels `lab{k}` f32 [M, 5] (cls, xyxy), `nc{k}`, the validator's `conf{k}` and the reference's matrix `mx{k}` int64 [nc + 1, nc + 1];
`n` = number of cases and `kind{k}` (a short tag).  Every case is TIE-FREE: the generator asserts that no two candidate IoUs (> 0.45, score > 0.25) of a case
are equal, so the reference's answer does not depend on the order numpy's argsort gives equal keys.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402

NCS = (1, 3, 10)
SIZES = [(0, 7), (1, 1), (5, 0), (12, 9), (40, 60), (23, 31), (40, 17), (9, 60)]      # (detections, labels)


SHARED = [0, 0]


def boxes(rng, n):
    c = rng.uniform(60, 580, (n, 2))
    wh = rng.uniform(24, 160, (n, 2))
    return np.concatenate([c - wh / 2, c + wh / 2], 1).astype(np.float32)


def make_image(rng, nc, nd, nl, miss=False):
    """Labels anywhere in a 640-pixel image; most detections are jittered copies of one of the first few labels (so that several
    detections claim one label and one detection overlaps several labels), the rest lie anywhere; scores on both sides of 0.25;
    about a quarter of the classes differ from the label's.  miss: every detection is moved outside the image, so no pair passes."""
    lab = boxes(rng, nl)
    gc = rng.integers(0, nc, nl)
    det = boxes(rng, nd)
    dc = rng.integers(0, nc, nd)
    if nl and nd:
        src = rng.integers(0, min(nl, 8), nd)
        near = rng.random(nd) < 0.8
        jit = lab[src] + rng.normal(0, 6, (nd, 4)).astype(np.float32)
        det = np.where(near[:, None], jit, det).astype(np.float32)
        dc = np.where(near & (rng.random(nd) < 0.75), gc[src], dc)
    if miss:
        det = det + np.float32(2000)
    score = rng.uniform(0.03, 0.97, nd).astype(np.float32)
    return (np.concatenate([det, score[:, None], dc[:, None].astype(np.float32)], 1).astype(np.float32).reshape(nd, 6),
            np.concatenate([gc[:, None].astype(np.float32), lab], 1).astype(np.float32).reshape(nl, 5))


def assert_tie_free(box_iou, det, lab, conf=0.25, thr=0.45):
    d = torch.from_numpy(det)
    d = d[d[:, 4] > conf]
    iou = box_iou(torch.from_numpy(lab[:, 1:]), d[:, :4])
    v = iou[iou > thr].numpy()
    assert len(np.unique(v)) == len(v), 'two candidate IoUs are equal: choose another seed'
    SHARED[0] += int(((iou > thr).sum(1) > 1).sum())      # labels that several detections overlap
    SHARED[1] += int(((iou > thr).sum(0) > 1).sum())      # detections that overlap several labels
    return len(v)


def put(d, k, det, lab, nc, cm, conf, kind):
    if det is not None:
        d[f'det{k}'] = det
    d[f'lab{k}'], d[f'nc{k}'], d[f'conf{k}'], d[f'mx{k}'], d[f'kind{k}'] = lab, nc, conf, cm.matrix.astype(np.int64), kind


def main():
    G._import_reference()
    from ultralytics.utils.metrics import ConfusionMatrix, box_iou
    d, k = {}, 0
    passing = multi = 0
    for nc in NCS:
        for i, (nd, nl) in enumerate(SIZES):
            rng = np.random.default_rng(1000 * nc + i)
            det, lab = make_image(rng, nc, nd, nl)
            cm = ConfusionMatrix(nc=nc, conf=0.001)        # the validator's default: 0.25 applies
            assert cm.conf == 0.25 and cm.iou_thres == 0.45
            if nl:
                n = assert_tie_free(box_iou, det, lab)
                passing += n
                cm.process_batch(torch.from_numpy(det), torch.from_numpy(lab))
            put(d, k, det, lab, nc, cm, 0.001, f'image {nd}x{nl}')
            multi += int(cm.matrix[:nc, nc].sum() > 0)
            k += 1
        # no pair passes: every label is a background miss and, although detections pass the confidence, no false positive is counted
        rng = np.random.default_rng(1000 * nc + 50)
        det, lab = make_image(rng, nc, 15, 11, miss=True)
        cm = ConfusionMatrix(nc=nc, conf=0.001)
        assert assert_tie_free(box_iou, det, lab) == 0
        cm.process_batch(torch.from_numpy(det), torch.from_numpy(lab))
        assert cm.matrix[:nc].sum() == 0 and cm.matrix[nc].sum() == 11
        put(d, k, det, lab, nc, cm, 0.001, 'no pair passes')
        k += 1
        # the detections=None form (an image without detections): labels are the class vector
        _, lab = make_image(rng, nc, 0, 13)
        cm = ConfusionMatrix(nc=nc, conf=0.001)
        cm.process_batch(None, torch.from_numpy(lab[:, 0]))
        put(d, k, None, lab, nc, cm, 0.001, 'detections=None')
        k += 1
        # a non-default confidence is used as given
        rng = np.random.default_rng(1000 * nc + 60)
        det, lab = make_image(rng, nc, 30, 20)
        cm = ConfusionMatrix(nc=nc, conf=0.6)
        assert cm.conf == 0.6
        assert_tie_free(box_iou, det, lab, conf=0.6)
        cm.process_batch(torch.from_numpy(det), torch.from_numpy(lab))
        put(d, k, det, lab, nc, cm, 0.6, 'conf 0.6')
        k += 1
    d['n'] = k
    # a good share of pairs pass, false positives occur, labels are claimed by several detections and detections overlap several labels
    assert passing > 200 and multi >= 6 and SHARED[0] > 30 and SHARED[1] > 5, (passing, multi, SHARED)
    G.save('confusion', d)


if __name__ == '__main__':
    main()
