#!/usr/bin/env python3
"""Generate tests/golden/curves.npz by running the *reference's* ap_per_class and compute_ap (ultralytics/utils/metrics.py:999-1128) on the
CPU over seeded cases.  Runs only where the reference is present; the import recipe is make_golden.py's.

    python tests/golden/make_curves_golden.py

What is stored (data only): `n` = number of cases; per case k the inputs `tp{k}` bool [N, 10], `conf{k}` f32 [N], `pcls{k}` f32 [N],
`tcls{k}` f32 [M], `nc{k}`, and the reference's `ap{k}` [C, 10], `p{k}`, `r{k}`, `f1{k}` [C], `classes{k}` [C], `pcurve{k}`, `rcurve{k}`,
`f1curve{k}` [C, 1000] and `pr{k}` [C, 1000]: np.interp(x, mrec, mpre) of its compute_ap at the first threshold, which is what it
appends to `prec_values` when it plots - computed here from compute_ap's knots, dense over its classes (zero rows where a class has no
prediction), without calling its plotting.
Cases: nc in {1, 3, 10} x (predictions, labels) in SIZES.  With nc >= 3 class 1 has labels and no predictions and class 2 predictions and
no labels.  Hits are rarer at higher thresholds and never outnumber the class's labels (a label is matched once), so recall <= 1.
Every case is TIE-FREE in conf (asserted), so the reference's answer does not depend on the order numpy's argsort gives equal keys, and
the largest smoothed mean-F1 value exceeds the runner-up by more than 1e-9 (asserted), so rounding cannot move the operating point.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402

NCS = (1, 3, 10)
SIZES = [(0, 7), (1, 1), (5, 0), (37, 12), (600, 90), (4000, 300)]      # (predictions, labels)


def make_case(rng, nc, n, m):
    pcls = rng.integers(0, nc, n)
    tcls = rng.integers(0, nc, m)
    if nc >= 3:
        pcls[pcls == 1] = 0          # class 1: labels, no predictions
        tcls[tcls == 2] = 0          # class 2: predictions, no labels
    conf = ((rng.permutation(n) + rng.uniform(0.1, 0.9, n)) / max(n, 1) * 0.97 + 0.002).astype(np.float32)
    assert len(np.unique(conf)) == n, 'two confidences are equal: choose another seed'
    u = rng.random(n)
    tp = u[:, None] < np.linspace(0.7, 0.15, 10)[None, :] * (0.3 + 0.7 * conf[:, None])      # confident rows hit more often
    order = np.argsort(-conf)
    for c in range(nc):              # a label is matched at most once per threshold
        rows = order[pcls[order] == c]
        tp[rows] &= tp[rows].cumsum(0) <= int((tcls == c).sum())
    return tp, conf, pcls.astype(np.float32), tcls.astype(np.float32)


def main():
    G._import_reference()
    from ultralytics.utils.metrics import ap_per_class, compute_ap, smooth
    d, k, gaps = {}, 0, []
    for nc in NCS:
        for i, (n, m) in enumerate(SIZES):
            tp, conf, pcls, tcls = make_case(np.random.default_rng(7000 + 100 * nc + i), nc, n, m)
            with np.errstate(all='ignore'):
                _, _, p, r, f1, ap, classes, p_curve, r_curve, f1_curve, x, _ = ap_per_class(tp, conf, pcls, tcls, names={})
            assert np.array_equal(x, np.linspace(0, 1, 1000))
            order = np.argsort(-conf)
            pr = np.zeros((len(classes), 1000))
            for row, c in enumerate(classes):
                hit = tp[order][pcls[order] == c]
                n_l = int((tcls == c).sum())
                if len(hit) == 0 or n_l == 0:
                    continue
                tpc = hit.cumsum(0)
                fpc = (1 - hit).cumsum(0)
                a, mpre, mrec = compute_ap(tpc[:, 0] / (n_l + 1e-16), tpc[:, 0] / (tpc[:, 0] + fpc[:, 0]))
                assert a == ap[row, 0]
                pr[row] = np.interp(x, mrec, mpre)
            if len(classes) and f1_curve.any():
                top = np.sort(smooth(f1_curve.mean(0), 0.1))
                gaps.append(top[-1] - top[-2])
                assert gaps[-1] > 1e-9, ('the operating point is not unique: choose another seed', nc, n, m, gaps[-1])
            d[f'tp{k}'], d[f'conf{k}'], d[f'pcls{k}'], d[f'tcls{k}'], d[f'nc{k}'] = tp, conf, pcls, tcls, nc
            d[f'ap{k}'], d[f'p{k}'], d[f'r{k}'], d[f'f1{k}'], d[f'classes{k}'] = ap, p, r, f1, classes
            d[f'pcurve{k}'], d[f'rcurve{k}'], d[f'f1curve{k}'], d[f'pr{k}'] = p_curve, r_curve, f1_curve, pr
            k += 1
    d['n'] = k
    print('smallest gap of the smoothed mean F1 between its maximum and the runner-up:', min(gaps))
    G.save('curves', d)


if __name__ == '__main__':
    main()
