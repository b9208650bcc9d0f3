"""GPU: tamtr_hota_update / tamtr_hota_end_sequence (csrc/hota.hip) through track.HotaEvaluator against the numpy statement of the rule
(engine.hota_evaluate) and the hand-worked values of tests/hota_cases.py; Predictor.track with two evaluators and tools/track.py --hota.

Tolerances: integer counts (TP, FN, FP, gt_dets, trk_dets) are equal.  The fp64 sums are added with atomics on the device, so
reordering moves them by about n * 2^-53 of their value: 1e-9 relative, the tolerance tests/test_gpu_mot.py gives iou_sum for the same
reason.  The twin's matching is the device's because every sequence used holds hota_cases.unique_optimum (asserted in
test_hota_host.py and, for the sequences made here, below): forbidding any matched pair loses at least 1e-9 of the total, far more than
the last bits in which the two sides' pot differ."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
import hota_cases as HC
import mot_cases as MC
from test_gpu_mot import _gt_from, pack

pytestmark = pytest.mark.gpu
RTOL = 1e-9


def evaluator(nc, nq=8, ng=8, G=16, Tcap=32, P=256, L=1024, F=128, **kw):
    from tamtr_amd.track import HotaEvaluator
    return HotaEvaluator('cuda', nc, gt_capacity=G, track_capacity=Tcap, pair_capacity=P, log_capacity=L, frame_capacity=F, nq=nq, ng=ng, **kw)


def feed(ev, seq, B, end=True):
    """The frames of one sequence in groups of B (0: all in one launch; the last group may be shorter), then the end of the sequence."""
    for i in range(0, len(seq), B or len(seq)):
        chunk = seq[i:i + (B or len(seq))]
        tracks, tc = pack([t for _, t in chunk], ev.nq)
        ev.update(tracks, tc, [g for g, _ in chunk])
    if end:
        ev.end_sequence()


def run(ev, sequences, B):
    for seq in sequences:
        feed(ev, seq, B)
    return ev.counts()


_TWIN = {}


def twin(key, sequences, nc):
    """engine.hota_evaluate of the sequences, computed once per key and shared."""
    if key not in _TWIN:
        from tamtr_amd.engine import hota_evaluate
        _TWIN[key] = hota_evaluate(sequences, nc)
    return _TWIN[key]


def random_twin(seed):
    return twin(('seed', seed), [MC.random_cases()[seed][0]], 2)


def sequence_state_is_clear(ev):
    sd = {k: v.cpu().numpy() for k, v in ev.state.items()}
    return not any(sd[k].any() for k in ('gstate', 'tcount', 'pkey', 'ppot', 'phist')) and sd['hdr'].tolist() == [0] * 16


# ------------------------------------------------------------------------------------------------ hand-worked cases
@pytest.mark.parametrize('name', sorted(HC.HAND))
def test_hand_cases(name):
    sequences, nc, expected = HC.HAND[name]
    ev = evaluator(nc)
    got = run(ev, sequences, 4)
    HC.same_counts(got, twin(('hand', name), sequences, nc), RTOL, name)
    HC.check_expected(ev.results(), expected, name)
    assert sequence_state_is_clear(ev), 'the per-sequence state is not cleared'


# ------------------------------------------------------------------------------------------------ random sequences, every grouping
@pytest.mark.parametrize('seed', MC.SEEDS)
def test_random_sequence_in_every_grouping(seed):
    seq = MC.random_cases()[seed][0]
    want = random_twin(seed)
    assert len(seq) == 12 and len(seq) % 5 and want['TP'][:, 0].sum() > want['TP'][:, 18].sum() > 0
    got = {B: run(evaluator(2, nq=12, ng=12, G=32, Tcap=256), [seq], B) for B in (1, 4, 5, 0)}
    for B, c in got.items():
        HC.same_counts(c, want, RTOL, f'seed {seed} B {B}')
        HC.same_counts(c, got[1], RTOL, f'seed {seed} B {B} against B 1')


def test_crowded_sequence_crosses_the_wave_width():
    seq = MC.crowded_sequence()
    want = twin('crowded', [seq], 3)
    assert want['TP'][:, 0].sum() > 200
    for B in (1, 4):
        HC.same_counts(run(evaluator(3, nq=72, ng=72, G=128, Tcap=512, P=4096, L=8192), [seq], B), want, RTOL, f'crowded B {B}')


def test_dense_cluster_is_one_component_for_the_solver():
    """70 x 70 with every pair positive: nothing is an isolated pair, the whole frame goes through the solver, and the pair table and
    the log take 4900 pairs per frame."""
    seq = MC.cluster_sequence()
    want = twin('cluster', [seq], 1)
    assert want['TP'][0, 0] == 210 and want['gt_dets'][0] == 210
    for B in (1, 3):
        HC.same_counts(run(evaluator(1, nq=72, ng=72, G=128, Tcap=512, P=16384, L=16384), [seq], B), want, RTOL, f'cluster B {B}')


def long_sequence(n):
    """n frames: the seeded 12-frame sequences one after another, each with ids of its own (ground truth + 10 k, tracks + 150 k)."""
    out = []
    for k in range((n + 11) // 12):
        for g, t in MC.random_cases()[MC.SEEDS[k % 3]][0]:
            g, t = g.copy(), t.copy()
            g[:, 4] += 10 * k
            t[:, 4] += 150 * k
            out.append((g, t))
    assert all(len(set(t[:, 4].tolist())) == len(t) for _, t in out)
    return out[:n]


def test_more_frames_than_workgroups():
    """67 frames = the matching launch's workgroups + 3: the stride loop takes a second turn, and its tail leaves most groups idle."""
    from tamtr_amd import ops
    n = ops.HOTA_END_WORKGROUPS + 3
    seq = long_sequence(n)
    assert len(seq) == n and HC.unique_optimum(seq, 2) >= 1e-9
    want = twin('long', [seq], 2)
    assert want['TP'][:, 0].sum() > n
    for B in (4, 0):
        HC.same_counts(run(evaluator(2, nq=12, ng=12, G=128, Tcap=1024, P=1024, L=4096), [seq], B), want, RTOL, f'{n} frames B {B}')


def test_empty_frames_inside_a_batch():
    g, t = MC.frame([MC.G(MC.BOX_A, 1), MC.G(MC.BOX_B, 2)], [MC.T(MC.BOX_A, 1), MC.T(MC.BOX_B, 2), MC.T(MC.BOX_C, 3)])
    none_g, none_t = MC.frame()
    seq = [(g, t), (none_g, t), (g, none_t), (none_g, none_t), (g, t)]
    want = twin('empty', [seq], 1)
    assert want['TP'][0].tolist() == [4] * 19 and want['gt_dets'][0] == 6 and want['trk_dets'][0] == 9
    for B in (5, 2):
        HC.same_counts(run(evaluator(1), [seq], B), want, RTOL, f'empty frames B {B}')
    only_empty = run(evaluator(1), [[(none_g, none_t)] * 3], 3)
    assert not any(np.asarray(v).any() for v in only_empty.values())


# ------------------------------------------------------------------------------------------------ sequences, reset, evaluators
def test_two_sequences_then_results():
    from tamtr_amd.engine import hota_summary
    cases = MC.random_cases()
    seqs = [cases[s][0] for s in MC.SEEDS[:2]]
    ev = evaluator(2, nq=12, ng=12, G=32, Tcap=256)
    want = twin('two', seqs, 2)
    HC.same_counts(run(ev, seqs, 5), want, RTOL, 'two sequences')
    res, ref = ev.results(['a', 'b']), hota_summary(want, ['a', 'b'])
    assert res['per_class'][1]['class'] == 'b' and res['all']['TP'] == ref['all']['TP']
    for k in HC.RATIOS:
        assert abs(res['all'][k] - ref['all'][k]) <= RTOL and np.allclose(res['per_class'][0][k + '_alpha'], ref['per_class'][0][k + '_alpha'], rtol=RTOL, atol=0)
    feed(ev, seqs[0][:1], 1, end=False)
    with pytest.raises(RuntimeError, match='end_sequence'):
        ev.results()


def test_reset():
    seq = MC.random_cases()[MC.SEEDS[0]][0]
    ev = evaluator(2, nq=12, ng=12, G=32, Tcap=256)
    feed(ev, seq[:5], 5, end=False)      # a sequence left open
    ev.reset()
    assert all(not bool(v.any()) for v in ev.state.values())
    HC.same_counts(run(ev, [seq], 4), random_twin(MC.SEEDS[0]), RTOL, 'after reset')


def test_two_evaluators_used_alternately():
    cases = MC.random_cases()
    sa, sb = cases[MC.SEEDS[0]][0], cases[MC.SEEDS[1]][0]
    a, b = evaluator(2, nq=12, ng=12, G=32, Tcap=256), evaluator(2, nq=12, ng=12, G=32, Tcap=256)
    for i in range(0, 12, 3):
        for ev, seq in ((a, sa), (b, sb)):
            feed(ev, seq[i:i + 3], 3, end=False)
    a.end_sequence(), b.end_sequence()
    HC.same_counts(a.counts(), random_twin(MC.SEEDS[0]), RTOL, 'evaluator a')
    HC.same_counts(b.counts(), random_twin(MC.SEEDS[1]), RTOL, 'evaluator b')


def test_a_mot_evaluator_in_company_keeps_its_counts():
    from tamtr_amd.engine import mot_evaluate
    from tamtr_amd.track import MotEvaluator
    seq = MC.random_cases()[MC.SEEDS[2]][0]
    mot = MotEvaluator('cuda', 2, gt_capacity=32, track_capacity=256, nq=12, ng=12)
    hota = evaluator(2, nq=12, ng=12, G=32, Tcap=256)
    for i in range(0, 12, 4):
        tracks, tc = pack([t for _, t in seq[i:i + 4]], 12)
        gts = [g for g, _ in seq[i:i + 4]]
        mot.update(tracks, tc, gts)
        hota.update(tracks, tc, gts)
    mot.end_sequence(), hota.end_sequence()
    MC.same_counts(mot.counts(), mot_evaluate([seq], 2), RTOL, 'MOT next to HOTA')
    HC.same_counts(hota.counts(), random_twin(MC.SEEDS[2]), RTOL, 'HOTA next to MOT')
    assert hota.counts()['gt_dets'].tolist() == mot.counts()['gt_dets'].tolist()


# ------------------------------------------------------------------------------------------------ overflow
PAD = 77


def padded(ev):
    """Move the evaluator's state and workspace into tensors with a canary behind each -> a check that every canary is intact."""
    from tamtr_amd import ops
    big = {}
    for k, dt, shape in ops.HOTA_STATE_SPEC:
        sh = shape(ev.nc, ev.caps)
        big[k] = torch.full((sh[0] + 64,) + sh[1:], PAD, dtype=dt, device='cuda')
        big[k][:sh[0]] = 0
        ev.state[k] = big[k][:sh[0]]
    need = ops.hota_workspace_bytes(ev.nq, ev.ng)
    ws = torch.full((need + 4096,), PAD, dtype=torch.uint8, device='cuda')
    ev.workspace = ws[:need]

    def intact():
        torch.cuda.synchronize()
        for k, dt, shape in ops.HOTA_STATE_SPEC:
            assert bool((big[k][shape(ev.nc, ev.caps)[0]:] == PAD).all()), f'{k}: written past the table'
        assert bool((ws[need:] == PAD).all()), 'written past the workspace'
    return intact


def isolated(n, first_gt=1, first_trk=1):
    """One frame of n ground truths far apart, each with a track exactly on it."""
    boxes = [(60 * i, 0, 60 * i + 40, 40) for i in range(n)]
    return MC.frame([MC.G(boxes[i], first_gt + i) for i in range(n)], [MC.T(boxes[i], first_trk + i) for i in range(n)])


def test_ids_and_rows_beyond_capacity_are_counted_and_left_out():
    """gt_capacity 4 with 6 identities, track_capacity 8 with ids 3 .. 12, and a frame with more rows than ng.  What is inside the
    capacities is scored: 4 identities with tracks 3 .. 6 in both frames; track 7 is a false positive."""
    from tamtr_amd.track import HotaOverflow
    ev = evaluator(1, nq=12, ng=8, G=4, Tcap=8)
    intact = padded(ev)
    f1 = isolated(10, 101, 3)
    f1 = (f1[0][:6], f1[1])
    f2 = (np.concatenate([f1[0], np.asarray([MC.G((900, 0, 940, 40), 200 + i, 0, 1) for i in range(4)], np.float32)]), f1[1])     # 10 rows > ng
    feed(ev, [f1, f2], 2)
    intact()
    assert ev.state['hdr'].cpu().tolist() == [0, 0, 4, 10, 2, 0, 0, 0] + [0] * 8
    with pytest.raises(HotaOverflow, match='gt identities'):
        ev.results()
    assert ev.state['tp_lvl'].cpu()[0].tolist() == [0] * 19 + [8] and ev.state['dets'].cpu()[0].tolist() == [8, 10]


@pytest.mark.parametrize('what, caps, hdr', [
    ('log', dict(L=5), [0, 0, 0, 0, 0, 3, 0, 0]),            # 4 pairs per frame, two frames: the second keeps one
    ('frames', dict(F=2), [0, 0, 0, 0, 0, 0, 1, 0]),         # three frames
    ('pairs', dict(P=3), [0, 0, 0, 0, 0, 0, 0, 3]),          # 4 pairs: one finds no slot, in each of three frames
])
def test_log_frames_and_pair_table_beyond_capacity(what, caps, hdr):
    from tamtr_amd.track import HotaOverflow
    ev = evaluator(1, **caps)
    intact = padded(ev)
    n = 3 if what != 'log' else 2
    feed(ev, [isolated(4)] * n, 0)
    intact()
    assert ev.state['hdr'].cpu().tolist() == hdr + [0] * 8
    assert not any(bool(ev.state[k].any()) for k in ('gstate', 'tcount', 'pkey', 'ppot', 'phist'))
    with pytest.raises(HotaOverflow, match=what if what != 'log' else 'log_capacity'):
        ev.counts()
    ev.reset()
    HC.same_counts(run(ev, [[isolated(2)] * 2], 1), twin('iso2', [[isolated(2)] * 2], 1), RTOL, f'{what}: inside the capacity after reset')
    intact()


def test_header_check_raises_before_the_results_are_read():
    from tamtr_amd.track import HotaOverflow
    ev = evaluator(1, F=1)
    feed(ev, [isolated(2)] * 2, 2, end=False)
    with pytest.raises(HotaOverflow, match='frame_capacity'):
        ev.check_overflow(ev.state['hdr'].cpu().numpy())


# ------------------------------------------------------------------------------------------------ end to end
def test_predictor_track_with_two_evaluators(tmp_path):
    from test_gpu_predict import CONF, IMGSZ, NC, _images, _model, _text_feats
    from tamtr_amd.engine import hota_evaluate, mot_evaluate
    from tamtr_amd.predict import Predictor
    from tamtr_amd.track import ByteTracker, HotaEvaluator, MotEvaluator
    src = _images(tmp_path)
    names = {i: f'c{i}' for i in range(NC)}
    pred = Predictor(_model().cuda(), names, _text_feats(), imgsz=IMGSZ, conf=CONF, iou=0.7, batch=2, dtype='fp32')
    plain = list(pred.predict(str(src)))
    keys = set(pred.speed())
    scores = np.sort(np.concatenate([d.conf.numpy() for d in plain]))
    trk = ByteTracker('cuda', capacity=256, nq=300, track_high_thresh=float(scores[len(scores) // 2]) * 1.0001,
                      track_low_thresh=float(scores[len(scores) // 8]) * 1.0001, new_track_thresh=float(scores[len(scores) * 3 // 4]) * 1.0001)
    gt = _gt_from(plain, np.random.default_rng(8))
    mot, hota = MotEvaluator('cuda', NC, gt_capacity=64, track_capacity=4096), HotaEvaluator('cuda', NC, gt_capacity=64)
    got = list(pred.track(str(src), tracker=trk, gt=gt, evaluator=[mot, hota]))
    assert [d.path for d in got] == [d.path for d in plain]
    assert pred.speed()['mot'] > 0 and pred.speed()['hota'] > 0 and set(pred.speed()) == keys | {'mot', 'hota'}
    frames = []
    for d, g in zip(got, gt):
        rows = np.zeros((0, 6), np.float32) if d.id is None else np.concatenate([d.boxes.numpy()[:, :4], d.id.numpy()[:, None].astype(np.float32),
                                                                                  d.boxes.numpy()[:, 5:6]], 1)
        frames.append((g, rows))
    want = hota_evaluate([frames], NC)
    counts = hota.counts()
    print('end to end HOTA counts', {k: np.asarray(v).sum(0).tolist() for k, v in counts.items()})
    HC.same_counts(counts, want, RTOL, 'end to end')
    MC.same_counts(mot.counts(), mot_evaluate([frames], NC), RTOL, 'end to end, MOT in company')
    assert want['gt_dets'].sum() > 0 and want['trk_dets'].sum() > 0 and want['TP'][:, 0].sum() > 0
    # a single MotEvaluator has today's keys; no evaluator has none of them
    list(pred.track(str(src), tracker=trk, gt=gt, evaluator=MotEvaluator('cuda', NC, gt_capacity=64, track_capacity=4096)))
    assert set(pred.speed()) == keys | {'mot'}
    list(pred.track(str(src), tracker=trk))
    assert set(pred.speed()) == keys
    HC.same_counts(hota.counts(), want, RTOL, 'the evaluator was touched by a run that did not name it')


def test_track_cli_with_gt_and_hota_writes_both_tables(tmp_path):
    from PIL import Image
    from test_gpu_predict import CONF, IMGSZ, NC, _model, _text_feats
    rng = np.random.default_rng(4)
    (tmp_path / 'gt').mkdir()
    for seq, n in (('uav1', 3), ('uav2', 2)):
        (tmp_path / 'sequences' / seq).mkdir(parents=True)
        lines = []
        for i in range(n):
            Image.fromarray(rng.integers(0, 256, (96, 128, 3), dtype=np.uint8)).save(tmp_path / 'sequences' / seq / f'{i + 1:07d}.png')
            for k in range(4):
                x, y = rng.uniform(0, 80), rng.uniform(0, 50)
                lines.append('%d,%d,%.1f,%.1f,%.1f,%.1f,1,%d,0,0\n' % (i + 1, k + 1, x, y, rng.uniform(20, 48), rng.uniform(20, 46), 1 + k % NC))
            lines.append('%d,9,0,0,20,20,0,0,0,0\n' % (i + 1))
        (tmp_path / 'gt' / f'{seq}.txt').write_text(''.join(lines))
    sd = _model().state_dict()
    torch.save({'model': sd, 'ema': sd}, tmp_path / 'best.pt')
    names = [f'c{i}' for i in range(NC)]
    np.savez(tmp_path / 'feats.npz', texts=np.array(names), feats=_text_feats().numpy())
    (tmp_path / 'bytetrack.yaml').write_text('tracker_type: bytetrack\ntrack_high_thresh: 0.00004\ntrack_low_thresh: 0.00002\n'
                                             'new_track_thresh: 0.00005\ntrack_buffer: 30\nmatch_thresh: 0.8\n')
    cmd = [sys.executable, os.path.join(ROOT, 'tools', 'track.py'), '--weights', str(tmp_path / 'best.pt'), '--text-feats', str(tmp_path / 'feats.npz'),
           '--names', ','.join(names), '--source', str(tmp_path / 'sequences'), '--tracker', str(tmp_path / 'bytetrack.yaml'), '--imgsz', str(IMGSZ),
           '--batch', '2', '--conf', str(CONF), '--save-mot', '--gt', str(tmp_path / 'gt'), '--hota', '--project', str(tmp_path / 'runs'),
           '--name', 'TAMTR', '--dtype', 'fp32', '--capacity', '512']
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    m = json.loads((tmp_path / 'runs' / 'TAMTR' / 'mot_metrics.json').read_text())
    assert list(m) == ['iou', 'sequences', 'overall', 'hota'] and sorted(m['sequences']) == sorted(m['hota']['sequences']) == ['uav1', 'uav2']
    assert 'HOTA' in r.stdout and 'MOTA' in r.stdout and res['hota_ms_per_image'] > 0 and res['mot_ms_per_image'] > 0
    for seq in ('uav1', 'uav2'):
        a, h = m['sequences'][seq]['all'], m['hota']['sequences'][seq]['all']
        assert set(MC.COUNT_KEYS) <= set(a) and a['TP'] + a['FN'] == a['gt_dets']
        assert h['gt_dets'] == a['gt_dets'] and h['trk_dets'] == a['trk_dets']
        assert all(t + f == h['gt_dets'] for t, f in zip(h['TP'], h['FN']))
    o = m['hota']['overall']['all']
    assert o['TP'] == [sum(v) for v in zip(*(m['hota']['sequences'][s]['all']['TP'] for s in m['hota']['sequences']))]
    assert res['hota']['HOTA'] == o['HOTA'] and 0.0 <= o['HOTA'] <= 1.0
