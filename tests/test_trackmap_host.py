"""CPU: engine.track_map_evaluate / track_map_summary (the numpy statement of the track-mAP rule, csrc/trackmap.hip) against the
hand-worked literals of tests/trackmap_cases.py; the margins that keep every decision of the seeded cases away from the last bits; the C
ABI and the argument checks of ops.trackmap_*; read_mot / pack_track_rows with scores; tools/mot_eval.py --host --track-map.

Tolerances: rows (scores included), classes, bits and counts are equal to the literals; AP and AR are within 1e-12 of the hand values,
because precision carries COCO's eps in its denominator (1 / (1 + 2^-52) is not 1)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
import mot_cases as MC
import trackmap_cases as TC


def evaluate(sequences, nc, **kw):
    from tamtr_amd.engine import track_map_evaluate
    return track_map_evaluate(sequences, nc, **kw)


@pytest.mark.parametrize('name', sorted(TC.HAND))
def test_hand_cases_have_the_worked_values(name):
    from tamtr_amd.engine import track_map_summary
    sequences, nc = TC.HAND[name][:2]
    got = evaluate(sequences, nc)
    assert got['thresholds'].tolist() == list(TC.THRESHOLDS)
    TC.check_expected(got, track_map_summary(got), name)


def test_a_class_without_ground_truth_is_minus_one_and_left_out():
    from tamtr_amd.engine import track_map_summary, track_map_table
    s = track_map_summary(evaluate(*TC.HAND['no_gt_class'][:2]), ['a', 'b'])
    assert s['per_class'][1] == {'class': 'b', 'AP': -1.0, 'AP_thr': [-1.0] * 3, 'AR_thr': [-1.0] * 3, 'gt_tracks': 0, 'tracks': 1}
    assert abs(s['all']['AP'] - 1.0) <= 1e-12 and s['all']['tracks'] == 2 and s['thresholds'] == [0.25, 0.5, 0.75]
    lines = track_map_table(s, 'seq').splitlines()
    assert len(lines) == 4 and lines[0].split()[:3] == ['seq', 'AP', 'AP@0.25'] and lines[-1].split()[0] == 'all'
    empty = track_map_summary(evaluate([[TC.frame()] * 2], 2))
    assert empty['all']['AP'] == -1.0 and empty['all']['AP_thr'] == [-1.0] * 3 and empty['all']['tracks'] == 0


def test_counts_of_sequences_add():
    from tamtr_amd.engine import track_map_add_counts, track_map_new_counts, track_map_since, track_map_summary
    seqs = TC.HAND['interleaved'][0] + TC.HAND['greedy'][0] + TC.seeded_cases()['seed11'][0]
    whole = evaluate(seqs, 2)
    parts = track_map_new_counts(2)
    for s in seqs:
        before = parts
        parts = track_map_add_counts(parts, evaluate([s], 2))
        one = track_map_since(parts, before)
        assert one['score'].tolist() == evaluate([s], 2)['score'].tolist() and one['gt_tracks'].tolist() == evaluate([s], 2)['gt_tracks'].tolist()
    for k in ('score', 'cls', 'bits', 'gt_tracks'):
        assert parts[k].tolist() == whole[k].tolist(), k
    assert track_map_summary(parts) == track_map_summary(whole)
    with pytest.raises(ValueError, match='thresholds'):
        track_map_add_counts(parts, track_map_new_counts(2, (0.5,)))


def test_rows_without_a_score_have_score_one():
    seq = TC.HAND['false_first'][0][0]
    six = [(g, t[:, :6]) for g, t in seq]
    ones = [(g, np.concatenate([t[:, :6], np.ones((len(t), 1), np.float32)], 1)) for g, t in seq]
    a, b = evaluate([six], 1), evaluate([ones], 1)
    assert a['score'].tolist() == [1.0, 1.0] == b['score'].tolist() and a['bits'].tolist() == b['bits'].tolist() == [7, 0]   # equal scores: id order


def test_thresholds_are_checked_and_ten_are_allowed():
    from tamtr_amd.engine import track_map_summary
    for bad in ((), (0.0,), (1.5,), tuple(np.linspace(0.05, 0.95, 11))):
        with pytest.raises(ValueError, match='thresholds'):
            evaluate(TC.HAND['half'][0], 1, thresholds=bad)
    ten = evaluate(TC.HAND['half'][0], 1, thresholds=np.linspace(0.5, 0.95, 10))
    assert ten['bits'].tolist() == [1]                      # IoU 0.5 passes the first of TrackEval's thresholds only
    assert np.allclose(track_map_summary(ten)['all']['AP_thr'], [1] + [0] * 9, atol=1e-12)


@pytest.mark.parametrize('name', sorted(set(TC.HAND) - set(TC.TIES)) + sorted(TC.seeded_cases()))
def test_margins_keep_every_decision_away_from_the_last_bits(name):
    """1e-6 everywhere, so that the 1e-9 the device is allowed cannot flip a threshold test, a pick or the order of two tracks."""
    sequences, nc = (TC.HAND[name] if name in TC.HAND else TC.seeded_cases()[name])[:2]
    d_thr, d_cand, d_score = TC.margins(sequences, nc, TC.EXACT_HITS.get(name, ()))
    print(name, 'margins', d_thr, d_cand, d_score)
    assert d_thr >= 1e-6 and d_cand >= 1e-6 and d_score >= 1e-6


def test_margins_of_the_cluster_at_trackevals_ten_thresholds():
    d_thr, d_cand, d_score = TC.margins(*TC.seeded_cases()['cluster'], thresholds=np.linspace(0.5, 0.95, 10))
    print('cluster, ten thresholds: margins', d_thr, d_cand, d_score)
    assert d_thr >= 1e-6 and d_cand >= 1e-6 and d_score >= 1e-6


def test_seeded_cases_exercise_what_they_are_for():
    cases = TC.seeded_cases()
    many = evaluate(*cases['many_tracks'])
    assert len(many['score']) == 300 and many['gt_tracks'].tolist() == [100] and sorted(set(many['bits'].tolist())) == [0, 1]
    assert int((many['bits'] == 1).sum()) == 100             # every IoU is 1 / 3: the best-scored of each three matches at 0.25
    detail = []
    cluster = evaluate(*cases['cluster'], detail=detail)
    assert cluster['gt_tracks'].tolist() == [70] and len(detail[0]['iou']) == 4900     # one ground truth has 70 > 64 candidates
    crowded = evaluate(*cases['crowded'])
    assert len(crowded['score']) > 64 and len(set(crowded['cls'].tolist())) == 3
    for s in MC.SEEDS:
        c = evaluate(*cases[f'seed{s}'])
        assert 0 < int((c['bits'] & 1).sum()) < len(c['bits']) and len(set(c['bits'].tolist())) > 2, f'seed {s}: {c["bits"].tolist()}'


def test_read_mot_and_pack_track_rows_round_trip_the_scores(tmp_path):
    from tamtr_amd.predict import Detections
    from tamtr_amd.track import pack_track_rows, read_mot, write_mot
    rng = np.random.default_rng(3)
    frames = []
    for n in (3, 0, 2):
        boxes = np.concatenate([rng.uniform(0, 50, (n, 2)), rng.uniform(60, 100, (n, 2)), rng.uniform(0.1, 1, (n, 1)), rng.integers(0, 3, (n, 1))], 1)
        boxes = np.round(boxes.astype(np.float32), 2)
        boxes[:, 4] = np.round(boxes[:, 4], 4)
        frames.append(Detections(f'{len(frames)}.jpg', (100, 100), None, torch.from_numpy(boxes), id=torch.arange(1, n + 1) if n else None))
    write_mot(tmp_path / 'seq.txt', frames)
    plain, scored = read_mot(tmp_path / 'seq.txt', gt=False), read_mot(tmp_path / 'seq.txt', gt=False, scores=True)
    assert [r.shape for r in plain] == [(3, 6), (0, 6), (2, 6)] and [r.shape for r in scored] == [(3, 7), (0, 7), (2, 7)]
    for p, s, d in zip(plain, scored, frames):
        assert np.array_equal(p, s[:, :6])
        assert np.allclose(s[:, 6], d.boxes[:, 4].numpy(), atol=5e-5) and np.allclose(s[:, :4], d.boxes[:, :4].numpy(), atol=0.011)
    rows, cnt = pack_track_rows(scored, 4, 'cpu')
    assert cnt.tolist() == [3, 0, 2] and np.array_equal(rows[0, :3, 5].numpy(), scored[0][:, 6]) and np.array_equal(rows[2, :2, 6].numpy(), scored[2][:, 5])
    rows6, _ = pack_track_rows(plain, 4, 'cpu')
    assert rows6[0, :3, 5].tolist() == [1.0] * 3 and torch.equal(rows6[..., :5], rows[..., :5]) and torch.equal(rows6[..., 6:], rows[..., 6:])


def test_new_symbols_are_exported_and_the_abi_version_stays():
    from tamtr_amd import _lib, ops, track
    h = _lib.lib()
    for n in ('tamtr_trackmap_update', 'tamtr_trackmap_end_sequence', 'tamtr_trackmap_workspace_bytes'):
        assert n in _lib.EXPORTS and hasattr(h, n), n
    assert h.tamtr_abi_version() == 36 == _lib.ABI_VERSION
    assert [k for k, _, _ in ops.TRACKMAP_STATE_SPEC] == ['gstate', 'garea', 'tframes', 'tsum', 'pkey', 'pinter', 'rscore', 'rmeta', 'gt_tracks', 'hdr']
    assert issubclass(track.TrackMapOverflow, RuntimeError) and track.TrackMapEvaluator.times_key == 'tmap'
    assert all(callable(getattr(ops, f)) for f in ('trackmap_update', 'trackmap_end_sequence', 'trackmap_accumulate', 'trackmap_workspace_bytes'))
    assert h.tamtr_trackmap_workspace_bytes(0, 8, 2, 4, 8, 16) == 0 and h.tamtr_trackmap_workspace_bytes(8, 8, 2, 4, 8, 0) == 0
    assert h.tamtr_trackmap_workspace_bytes(8, 8, 5000, 4, 8, 16) == 0 and h.tamtr_trackmap_workspace_bytes(8, 8, 4096, 1 << 24, 1 << 24, 16) == 0
    assert ops.trackmap_workspace_bytes(8, 8, 2, (4, 8, 16, 32)) >= 16 * 64
    # state and workspace at the default capacities stay under 32 MiB
    caps = (1024, 4096, 1 << 18, 1 << 16)
    total = ops.trackmap_workspace_bytes(300, 300, 10, caps)
    for _, dt, shape in ops.TRACKMAP_STATE_SPEC:
        total += int(np.prod(shape(10, caps))) * torch.empty(0, dtype=dt).element_size()
    assert total < 32 << 20, total


def test_c_entries_check_their_arguments_before_any_launch():
    import ctypes
    from tamtr_amd import _lib
    h = _lib.lib()
    eps = 2.0 ** -52
    z, one = ctypes.c_void_p(0), ctypes.c_void_p(16)
    state, caps = (ctypes.c_void_p * 10)(*[16] * 10), (ctypes.c_int * 4)(4, 8, 16, 32)
    holed = (ctypes.c_void_p * 10)(*([16] * 9 + [0]))
    need = h.tamtr_trackmap_workspace_bytes(8, 8, 2, 4, 8, 16)
    ok = [one] * 4 + [2, 8, 8, 2, 0.5, state, caps, one, need, z]
    bad = lambda i, v: h.tamtr_trackmap_update(*(ok[:i] + [v] + ok[i + 1:]))     # noqa: E731
    assert bad(0, z) == -1 and bad(4, 0) == -1 and bad(8, 0.0) == -1 and bad(9, holed) == -1 and bad(9, z) == -1
    assert bad(10, (ctypes.c_int * 4)(4, 8, 0, 32)) == -1 and bad(12, 16) == -1 and bad(11, ctypes.c_void_p(8)) == -1
    assert bad(5, 4000) == -2 and bad(7, 5000) == -2                         # solver state beyond the LDS; more classes than are built
    thr = (ctypes.c_double * 3)(0.25, 0.5, 0.75)
    end = [thr, 3, eps, 2, state, caps, one, need, z]
    bad = lambda i, v: h.tamtr_trackmap_end_sequence(*(end[:i] + [v] + end[i + 1:]))     # noqa: E731
    assert bad(0, z) == -1 and bad(1, 0) == -1 and bad(1, 11) == -1 and bad(2, 0.0) == -1 and bad(4, holed) == -1 and bad(7, 16) == -1
    assert bad(3, 5000) == -2 and bad(5, (ctypes.c_int * 4)(4, 1 << 25, 16, 32)) == -2


def _state(nc=2, caps=(4, 8, 16, 32), device='cpu'):
    from tamtr_amd import ops
    return {k: torch.zeros(shape(nc, caps), dtype=dt, device=device) for k, dt, shape in ops.TRACKMAP_STATE_SPEC}


def test_ops_refuse_bad_arguments_and_cpu_tensors():
    from tamtr_amd import TamtrHipError, ops
    from tamtr_amd.track import TrackMapEvaluator
    with pytest.raises(TamtrHipError):
        TrackMapEvaluator('cpu', 2)
    caps = (4, 8, 16, 32)
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)     # noqa: E731
    good = lambda: [torch.zeros(1, 8, 8), i32(1), torch.zeros(1, 8, 7), i32(1)]     # noqa: E731
    with pytest.raises(TamtrHipError, match='MI355X'):       # everything is right but the device
        ops.trackmap_update(*good(), _state(), 2, caps)
    with pytest.raises(TamtrHipError, match='MI355X'):
        ops.trackmap_end_sequence(_state(), 2, caps, TC.THRESHOLDS)
    with pytest.raises(TamtrHipError, match='MI355X'):
        ops.trackmap_accumulate(_state(), 2, caps, 3)
    for i, v, what in ((0, torch.zeros(1, 8, 6), 'tracks'), (2, torch.zeros(2, 8, 7), 'gt'), (1, i32(2), 'tcounts'), (3, torch.zeros(1), 'int32'),
                       (0, torch.zeros(1, 8, 8, dtype=torch.float64), 'float32')):
        a = good()
        a[i] = v
        with pytest.raises(TamtrHipError, match=what):
            ops.trackmap_update(*a, _state(), 2, caps)
    with pytest.raises(TamtrHipError, match='capacities'):
        ops.trackmap_update(*good(), _state(), 2, (4, 8, 0, 32))
    with pytest.raises(TamtrHipError, match='capacities'):
        ops.trackmap_end_sequence(_state(), 2, caps[:3], TC.THRESHOLDS)
    with pytest.raises(TamtrHipError, match='iou'):
        ops.trackmap_update(*good(), _state(), 2, caps, iou=0.0)
    with pytest.raises(TamtrHipError, match='pkey'):         # a state built for other capacities
        ops.trackmap_update(*good(), _state(caps=(4, 8, 17, 32)), 2, caps)
    st = _state()
    st['rscore'] = st['rscore'].float()
    with pytest.raises(TamtrHipError, match='rscore'):
        ops.trackmap_end_sequence(st, 2, caps, TC.THRESHOLDS)
    for thr in ((), (0.0, 0.5), tuple(np.linspace(0.05, 0.95, 11))):
        with pytest.raises(TamtrHipError, match='thresholds'):
            ops.trackmap_end_sequence(_state(), 2, caps, thr)
    with pytest.raises(TamtrHipError, match='n_thresholds'):
        ops.trackmap_accumulate(_state(), 2, caps, 11)
    with pytest.raises(TamtrHipError, match='outside'):
        ops.trackmap_workspace_bytes(8, 8, 5000, caps)
    with pytest.raises(ValueError, match='thresholds'):
        from tamtr_amd.engine import track_map_thresholds
        track_map_thresholds((0.5, 2.0))


def write_case(folder, sequences):
    """Sequences with scored track rows as VisDrone-MOT annotation and result files (category c + 1 is class c in the annotations)."""
    (folder / 'gt').mkdir(parents=True)
    (folder / 'res').mkdir()
    for s, frames in enumerate(sequences):
        gl, tl = [], []
        for f, (gt, trk) in enumerate(frames, 1):
            for x1, y1, x2, y2, i, c, k in gt.tolist():
                gl.append('%d,%d,%g,%g,%g,%g,1,%d,0,0\n' % (f, i, x1, y1, x2 - x1, y2 - y1, 0 if k == 2 else 11 if k == 1 else int(c) + 1))
            for x1, y1, x2, y2, i, c, sc in trk.tolist():
                tl.append('%d,%d,%.2f,%.2f,%.2f,%.2f,%.4f,%d,-1,-1\n' % (f, i, x1, y1, x2 - x1, y2 - y1, sc, int(c)))
        (folder / 'gt' / f'seq{s}.txt').write_text(''.join(gl))
        (folder / 'res' / f'seq{s}.txt').write_text(''.join(tl))


def test_mot_eval_cli_host_path_with_track_map_in_a_child_process(tmp_path):
    write_case(tmp_path, TC.HAND['interleaved'][0])
    cmd = [sys.executable, os.path.join(ROOT, 'tools', 'mot_eval.py'), '--gt', str(tmp_path / 'gt'), '--results', str(tmp_path / 'res'),
           '--names', 'thing', '--host']
    plain = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    r = subprocess.run(cmd + ['--track-map'], capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert r.returncode == 0 and plain.returncode == 0, r.stderr[-3000:]
    res, old = json.loads(r.stdout.strip().splitlines()[-1]), json.loads(plain.stdout.strip().splitlines()[-1])
    same = lambda d: json.dumps(d, sort_keys=True)     # noqa: E731  (nan compares equal as text)
    assert 'track_map' not in old and 'AP@0.25' not in plain.stdout and same({k: v for k, v in res.items() if k != 'track_map'}) == same(old)
    tm = res['track_map']
    assert 'AP@0.25' in r.stdout and sorted(tm['per_sequence']) == ['seq0', 'seq1'] and tm['overall']['per_class'][0]['class'] == 'thing'
    assert np.allclose(tm['overall']['all']['AP_thr'], [76 / 101] * 3, atol=1e-12) and tm['overall']['all']['gt_tracks'] == 4
    assert np.allclose(tm['per_sequence']['seq0']['all']['AP_thr'], [51 / 101] * 3, atol=1e-12)      # tp, fp with two ground truths
    assert np.allclose(tm['per_sequence']['seq1']['all']['AP_thr'], [1] * 3, atol=1e-12)
