"""CPU: engine.ap_per_class(curves=..., stable=...) against the reference's stored results (tests/golden/curves.npz) and against a loop
restatement with an explicit stable order; the C entry tamtr_val_ap_curves without a GPU; validate's argument check; the CLI's tables."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'curves.npz')
TOL = 1e-12      # about 2 000 fp64 roundings of values <= 1; the issue's bound, not a fitted one


def fixture_cases():
    d = np.load(GOLDEN)
    for k in range(int(d['n'])):
        yield k, {name: d[f'{name}{k}'] for name in ('tp', 'conf', 'pcls', 'tcls', 'nc', 'ap', 'p', 'r', 'f1', 'classes', 'pcurve', 'rcurve',
                                                     'f1curve', 'pr')}


def test_fixture_has_the_cases_the_kernel_needs():
    cases = [c for _, c in fixture_cases()]
    assert len(cases) == 18 and {int(c['nc']) for c in cases} == {1, 3, 10}
    assert {(len(c['conf']), len(c['tcls'])) for c in cases} == {(0, 7), (1, 1), (5, 0), (37, 12), (600, 90), (4000, 300)}
    assert all(len(np.unique(c['conf'])) == len(c['conf']) for c in cases)                      # tie-free
    big = [c for c in cases if int(c['nc']) == 10 and len(c['conf']) == 4000][0]
    assert 1 in big['classes'] and not (big['pcls'] == 1).any()                                 # labels, no predictions
    assert 2 not in big['classes'] and (big['pcls'] == 2).any()                                 # predictions, no labels


@pytest.mark.parametrize('stable', [False, True])
def test_curves_equal_the_reference(stable):
    from tamtr_amd import engine as E
    worst = 0.0
    for k, c in fixture_cases():
        with np.errstate(all='ignore'):        # the case without labels averages over no class, as the reference does
            tp, fp, p, r, f1, ap, classes, cv = E.ap_per_class(c['tp'], c['conf'], c['pcls'], c['tcls'], curves=True, stable=stable)
        assert np.array_equal(classes, c['classes'].astype(int)), k
        assert cv['px'].dtype == np.float64 and np.array_equal(cv['px'], np.linspace(0, 1, 1000))
        for got, want in ((p, c['p']), (r, c['r']), (f1, c['f1']), (ap, c['ap']), (cv['p'], c['pcurve']), (cv['r'], c['rcurve']),
                          (cv['f1'], c['f1curve']), (cv['pr'], c['pr'])):
            assert got.shape == want.shape and got.dtype == np.float64, k
            if got.size:
                worst = max(worst, float(np.abs(got - want).max()))
                assert np.abs(got - want).max() <= TOL, (k, float(np.abs(got - want).max()))
        n_pred = np.array([(c['pcls'] == x).sum() for x in classes], int)
        assert cv['valid'].dtype == bool and np.array_equal(cv['valid'], n_pred > 0)
        assert not cv['pr'][~cv['valid']].any() and not cv['p'][~cv['valid']].any()
    print('largest difference from the reference:', worst)


def test_defaults_return_the_old_tuple():
    from tamtr_amd import engine as E
    for k, c in fixture_cases():
        if len(c['tcls']) == 0:
            continue
        old = E.ap_per_class(c['tp'], c['conf'], c['pcls'], c['tcls'])
        new = E.ap_per_class(c['tp'], c['conf'], c['pcls'], c['tcls'], curves=True, stable=True)
        assert len(old) == 7 and len(new) == 8
        assert all(np.array_equal(a, b) for a, b in zip(old, new)), k      # tie-free input: the stable order is the default's


def ties_case(seed, n=900, m=120, nc=4):
    rng = np.random.default_rng(seed)
    conf = (rng.integers(1, 65, n) / 64).astype(np.float32)
    pcls, tcls = rng.integers(0, nc, n).astype(np.float32), rng.integers(0, nc + 1, m).astype(np.float32)
    tp = rng.random((n, 1)) < np.linspace(0.5, 0.1, 10)[None, :]
    return tp, conf, pcls, tcls


def loop_rule(tp, conf, pcls, tcls):
    """ap_per_class(stable=True, curves=True), restated with an explicit order: confidence descending, then input order."""
    from tamtr_amd import engine as E
    order = sorted(range(len(conf)), key=lambda i: (-float(conf[i]), i))
    classes = sorted(set(tcls.tolist()))
    px = np.linspace(0, 1, 1000)
    ap, pc, rc, pr = np.zeros((len(classes), 10)), np.zeros((len(classes), 1000)), np.zeros((len(classes), 1000)), np.zeros((len(classes), 1000))
    for row, c in enumerate(classes):
        rows = [i for i in order if pcls[i] == c]
        n = int((tcls == c).sum())
        if not rows or not n:
            continue
        hits = np.zeros(10)
        rec, pre = np.zeros((len(rows), 10)), np.zeros((len(rows), 10))
        for j, i in enumerate(rows):
            hits = hits + tp[i]
            rec[j], pre[j] = hits / (n + 1e-16), hits / (j + 1)
        score = np.array([conf[i] for i in rows], np.float64)
        rc[row], pc[row] = np.interp(-px, -score, rec[:, 0], left=0), np.interp(-px, -score, pre[:, 0], left=1)
        for t in range(10):
            ap[row, t], env, knots = E.compute_ap(rec[:, t], pre[:, t])
            if t == 0:
                pr[row] = np.interp(px, knots, env)
    return ap, pc, rc, pr


def test_stable_order_equals_the_loop_restatement_on_ties():
    from tamtr_amd import engine as E
    tp, conf, pcls, tcls = ties_case(5)
    assert len(np.unique(conf)) <= 64
    *_, ap, classes, cv = E.ap_per_class(tp, conf, pcls, tcls, curves=True, stable=True)
    want = loop_rule(tp, conf, pcls, tcls)
    for got, w in zip((ap, cv['p'], cv['r'], cv['pr']), want):
        assert np.array_equal(got, w)
    # and the order matters on such input: reversing the rows moves the curves
    rev = E.ap_per_class(tp[::-1], conf[::-1], pcls[::-1], tcls, curves=True, stable=True)
    assert not np.array_equal(rev[5], ap)


def test_validators_carry_the_curves_on_request():
    from tamtr_amd import engine as E
    from test_val_host import _fed_validators
    dv, hv = _fed_validators()
    assert 'curves' not in dv.results() and 'curves' not in hv.results()
    got, want = dv.results(curves=True), hv.results(curves=True)
    assert got['curves'] == want['curves'] and set(got['curves']) == {'px', 'p', 'r', 'f1', 'pr', 'valid', 'classes'}
    cv = got['curves']
    assert len(cv['px']) == 1000 and all(len(cv[k]) == len(cv['classes']) and len(cv[k][0]) == 1000 for k in ('p', 'r', 'f1', 'pr'))
    plain = dv.results()
    got.pop('curves')
    assert got == plain
    assert E.Validator(160).results(curves=True)['curves'] == {} and E.DeviceValidator(160).results(curves=True)['curves'] == {}


def test_validate_device_metrics_needs_the_device_path():
    from tamtr_amd import engine as E
    with pytest.raises(ValueError, match='device_metrics'):
        E.validate(torch.nn.Identity(), [], on_device=False, device_metrics=True)


# ------------------------------------------------------------------------------------------------ the C ABI without a GPU
def _lib():
    import tamtr_amd
    from tamtr_amd import _lib
    if not os.path.exists(tamtr_amd.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


def test_the_symbol_is_exported_and_the_abi_is_still_36():
    from tamtr_amd import _lib as L, ops
    h = _lib()
    assert L.ABI_VERSION == 36 and h.tamtr_abi_version() == 36
    assert 'tamtr_val_ap_curves' in L.EXPORTS and hasattr(h, 'tamtr_val_ap_curves')
    assert h.tamtr_val_ap_tile() == ops.VAL_AP_TILE
    with open(os.path.join(ROOT, 'include', 'tamtr_hip.h')) as f:
        text = f.read()
    assert 'int tamtr_val_ap_curves(' in text and 'utils/metrics.py:999-1029,1073-1127' in text


def test_val_ap_curves_arguments_are_checked_before_any_launch():
    h = _lib()
    z, one, odd = ctypes.c_void_p(0), ctypes.c_void_p(64), ctypes.c_void_p(68)   # non-null, never dereferenced (the checks come first)
    f = h.tamtr_val_ap_curves
    names = ('conf', 'correct', 'seg_off', 'lab_cls', 'px', 'grid', 'tpc', 'env', 'ap', 'p', 'r', 'pr', 'n_gt', 'n_pred')

    def call(N=100, nc=10, M=5, **kw):
        a = {k: kw.get(k, one) for k in names}
        return f(a['conf'], a['correct'], a['seg_off'], N, nc, a['lab_cls'], M, a['px'], a['grid'], a['tpc'], a['env'], a['ap'], a['p'], a['r'],
                 a['pr'], a['n_gt'], a['n_pred'], z)

    for k in names:
        assert call(**{k: z}) == -1, k
    assert call(N=0) == -1 and call(nc=0) == -1 and call(M=-1) == -1
    for k in ('px', 'grid', 'env', 'ap', 'p', 'r', 'pr'):                        # f64 operands: 8-byte aligned
        assert call(**{k: odd}) == -1, k
    for k in ('conf', 'seg_off', 'lab_cls', 'tpc', 'n_gt', 'n_pred'):            # f32 / i32 operands: 4-byte aligned
        assert call(**{k: ctypes.c_void_p(66)}) == -1, k
    assert call(nc=(1 << 20) + 1) == -2 and call(N=(1 << 30) + 1) == -2
    assert call(nc=(1 << 20) + 1, M=0, lab_cls=z) == -2                          # NULL labels are legal with M = 0: the next check answers
    assert call(nc=(1 << 20) + 1, ap=z) == -1


def test_val_ap_curves_refuses_cpu_tensors():
    import tamtr_amd.ops as ops
    from tamtr_amd import TamtrHipError
    batch = (torch.zeros(1, 5, 6), torch.zeros(1, 5, 10, dtype=torch.uint8), torch.zeros(1, dtype=torch.int32))
    with pytest.raises(TamtrHipError):
        ops.val_ap_curves([batch], np.zeros(3, np.float32), 3)
    with pytest.raises(TamtrHipError):
        ops.val_ap_curves([], np.zeros(3, np.float32), 3)


def test_val_ap_split_undoes_the_packing():
    import tamtr_amd.ops as ops
    nc = 3
    for buf in (np.arange(3011 * nc, dtype=np.float64), torch.arange(3011 * nc, dtype=torch.float64)):
        ap, p, r, pr, n_gt, n_pred = ops.val_ap_split(buf, nc)
        assert tuple(ap.shape) == (nc, 10) and tuple(p.shape) == tuple(r.shape) == tuple(pr.shape) == (nc, 1000)
        assert float(p[0, 0]) == 10 * nc and float(r[0, 0]) == 1010 * nc and float(pr[0, 0]) == 2010 * nc and float(pr[-1, -1]) == 3010 * nc - 1
        assert len(n_gt) == len(n_pred) == nc and 'int32' in str(n_gt.dtype)


# ------------------------------------------------------------------------------------------------ the CLI
def test_cli_curve_tables(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import val as V
    px = [0.0, 0.5, 1.0]
    curves = {'px': px, 'classes': [0, 2], 'valid': [True, False], 'p': [[1.0, 0.5, 0.25], [0.0, 0.0, 0.0]], 'r': [[0.1, 0.2, 0.3], [0.0, 0.0, 0.0]],
              'f1': [[0.2, 0.3, 0.4], [0.0, 0.0, 0.0]], 'pr': [[1.0, 0.75, 0.0], [0.0, 0.0, 0.0]]}
    paths = V.write_curves(curves, {0: 'car', 1: 'van', 2: 'bus'}, str(tmp_path))
    assert [os.path.basename(p) for p in paths] == ['PR_curve.csv', 'P_curve.csv', 'R_curve.csv', 'F1_curve.csv']
    tables = {os.path.basename(p): [line.split(',') for line in open(p).read().strip().splitlines()] for p in paths}
    assert tables['PR_curve.csv'][0] == ['recall', 'car', 'bus', 'all classes']
    assert all(tables[f][0] == ['confidence', 'car', 'bus', 'all classes'] for f in ('P_curve.csv', 'R_curve.csv', 'F1_curve.csv'))
    num = {f: np.array([[float(x) for x in row] for row in t[1:]]) for f, t in tables.items()}
    assert all(np.array_equal(a[:, 0], px) and a.shape == (3, 4) for a in num.values())
    assert np.array_equal(num['P_curve.csv'][:, 1:], [[1.0, 0.0, 0.5], [0.5, 0.0, 0.25], [0.25, 0.0, 0.125]])      # mean over both classes
    assert np.array_equal(num['PR_curve.csv'][:, 1:], [[1.0, 0.0, 1.0], [0.75, 0.0, 0.75], [0.0, 0.0, 0.0]])       # mean over the valid class
    empty = V.write_curves({}, {0: 'car'}, str(tmp_path))
    assert open(empty[0]).read().strip() == 'recall,all classes'
