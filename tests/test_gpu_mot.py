"""GPU: tamtr_mot_update / tamtr_mot_end_sequence (csrc/mot.hip) through track.MotEvaluator against the numpy statement of the rule
(engine.mot_evaluate) and the hand-worked counts of tests/mot_cases.py; Predictor.track with an evaluator and tools/track.py --gt.

Tolerances: integer counts are equal.  iou_sum is an fp64 sum of at most a few thousand terms in [0.5, 1] that the device adds with
atomics, so reordering moves it by at most about n * 2^-53 of its value: 1e-9 relative leaves three orders of margin and still catches
one missing term.  The twin's matching is the device's because every case has pairwise different scores inside a frame (asserted by
the generators of mot_cases.py), so each optimum is unique."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
import mot_cases as MC

pytestmark = pytest.mark.gpu
RTOL = 1e-9


def evaluator(nc, nq=8, ng=8, G=16, Tcap=32, **kw):
    from tamtr_amd.track import MotEvaluator
    return MotEvaluator('cuda', nc, gt_capacity=G, track_capacity=Tcap, nq=nq, ng=ng, **kw)


def pack(trks, nq):
    rows = np.zeros((len(trks), nq, 8), np.float32)
    for b, t in enumerate(trks):
        rows[b, :len(t)] = MC.device_rows(t)
    return torch.from_numpy(rows).cuda(), torch.tensor([len(t) for t in trks], dtype=torch.int32).cuda()


def feed(ev, seq, B):
    """The frames of one sequence in groups of B (the last may be shorter), then the end of the sequence."""
    for i in range(0, len(seq), B or len(seq)):
        chunk = seq[i:i + (B or len(seq))]
        tracks, tc = pack([t for _, t in chunk], ev.nq)
        ev.update(tracks, tc, [g for g, _ in chunk])
    ev.end_sequence()


def run(ev, sequences, B):
    for seq in sequences:
        feed(ev, seq, B)
    return ev.counts()


def twin(sequences, nc, **kw):
    from tamtr_amd.engine import mot_evaluate
    return mot_evaluate(sequences, nc, **kw)


_TWIN = {}


def random_twin(seed):
    if seed not in _TWIN:
        _TWIN[seed] = twin([MC.random_cases()[seed][0]], 2)
    return _TWIN[seed]


# ------------------------------------------------------------------------------------------------ hand-worked cases
@pytest.mark.parametrize('name', sorted(MC.HAND))
def test_hand_cases(name):
    sequences, nc, expected = MC.HAND[name]
    ev = evaluator(nc)
    got = run(ev, sequences, 4)
    MC.same_counts(got, twin(sequences, nc), RTOL, name)
    MC.check_expected(ev.results(), expected, name)
    sd = {k: v.cpu().numpy() for k, v in ev.state.items()}
    assert not sd['gstate'].any() and not sd['pair'].any() and sd['hdr'].tolist() == [0] * 8, 'the per-sequence state is not cleared'


# ------------------------------------------------------------------------------------------------ random sequences, every grouping
@pytest.mark.parametrize('seed', MC.SEEDS)
def test_random_sequence_in_every_grouping(seed):
    seq = MC.random_cases()[seed][0]
    want = random_twin(seed)
    assert len(seq) == 12 and len(seq) % 5
    got = {B: run(evaluator(2, nq=12, ng=12, G=32, Tcap=256), [seq], B) for B in (1, 4, 5, 0)}     # 0: the whole sequence in one launch
    for B, c in got.items():
        MC.same_counts(c, want, RTOL, f'seed {seed} B {B}')
        MC.same_counts(c, got[1], RTOL, f'seed {seed} B {B} against B 1')


def test_crowded_sequence_crosses_the_wave_width():
    seq = MC.crowded_sequence()
    assert max(len(g) for g, _ in seq) == 72 and max(len(t) for _, t in seq) == 72
    want = twin([seq], 3)
    assert want['IDSW'].sum() > 0 and want['drop_distractor'].sum() > 0 and want['TP'].sum() > 200
    for B in (1, 4):
        MC.same_counts(run(evaluator(3, nq=72, ng=72, G=128, Tcap=512), [seq], B), want, RTOL, f'crowded B {B}')


def test_dense_cluster_is_one_component_for_the_solver():
    """70 x 70 with every pair qualifying: no pair is isolated, so the whole problem goes through the solver, more columns than a
    wavefront, with the last-matched bonus in every row from the second frame on."""
    seq = MC.cluster_sequence()
    want = twin([seq], 1)
    assert want['TP'][0] == 210 and want['IDSW'][0] == 0 and want['IDTP'][0] == 210      # the bonus keeps all 70 ids in frames 2 and 3
    for B in (1, 3):
        MC.same_counts(run(evaluator(1, nq=72, ng=72, G=128, Tcap=512), [seq], B), want, RTOL, f'cluster B {B}')


def test_another_threshold():
    sequences, nc, _ = MC.HAND['B_frame2_alone']
    for thr in (0.6, 0.9):
        MC.same_counts(run(evaluator(nc, iou=thr), sequences, 1), twin(sequences, nc, iou=thr), RTOL, f'iou {thr}')


def test_empty_frames_inside_a_batch():
    g, t = MC.frame([MC.G(MC.BOX_A, 1), MC.G(MC.BOX_B, 2)], [MC.T(MC.BOX_A, 1), MC.T(MC.BOX_B, 2), MC.T(MC.BOX_C, 3)])
    none_g, none_t = MC.frame()
    seq = [(g, t), (none_g, t), (g, none_t), (none_g, none_t), (g, t)]
    want = twin([seq], 1)
    assert (want['TP'][0], want['FN'][0], want['FP'][0], want['Frag'][0]) == (4, 2, 5, 2)
    for B in (5, 2):
        MC.same_counts(run(evaluator(1), [seq], B), want, RTOL, f'empty frames B {B}')
    only_empty = run(evaluator(1), [[(none_g, none_t)] * 3], 3)
    assert not any(np.asarray(v).any() for v in only_empty.values())


# ------------------------------------------------------------------------------------------------ sequences, reset, two evaluators
def test_two_sequences_then_results():
    cases = MC.random_cases()
    seqs = [cases[s][0] for s in MC.SEEDS[:2]]
    ev = evaluator(2, nq=12, ng=12, G=32, Tcap=256)
    got = run(ev, seqs, 5)
    MC.same_counts(got, twin(seqs, 2), RTOL, 'two sequences')
    from tamtr_amd.engine import mot_summary
    res, want = ev.results(['a', 'b']), mot_summary(twin(seqs, 2), ['a', 'b'])
    assert res['all']['MOTA'] == want['all']['MOTA'] and res['per_class'][1]['class'] == 'b'
    assert abs(res['all']['MOTP'] - want['all']['MOTP']) <= RTOL and res['all']['IDF1'] == want['all']['IDF1']
    tracks, tc = pack([seqs[0][0][1]], ev.nq)
    ev.update(tracks, tc, [seqs[0][0][0]])
    with pytest.raises(RuntimeError, match='end_sequence'):
        ev.results()


def test_reset():
    seq = MC.random_cases()[MC.SEEDS[0]][0]
    ev = evaluator(2, nq=12, ng=12, G=32, Tcap=256)
    tracks, tc = pack([t for _, t in seq[:5]], ev.nq)
    ev.update(tracks, tc, [g for g, _ in seq[:5]])      # a sequence left open
    ev.reset()
    assert all(not bool(v.any()) for v in ev.state.values())
    MC.same_counts(run(ev, [seq], 4), random_twin(MC.SEEDS[0]), RTOL, 'after reset')


def test_two_evaluators_used_alternately():
    cases = MC.random_cases()
    sa, sb = cases[MC.SEEDS[0]][0], cases[MC.SEEDS[1]][0]
    a, b = evaluator(2, nq=12, ng=12, G=32, Tcap=256), evaluator(2, nq=12, ng=12, G=32, Tcap=256)
    for i in range(0, 12, 3):
        for ev, seq in ((a, sa), (b, sb)):
            tracks, tc = pack([t for _, t in seq[i:i + 3]], ev.nq)
            ev.update(tracks, tc, [g for g, _ in seq[i:i + 3]])
    a.end_sequence(), b.end_sequence()
    MC.same_counts(a.counts(), random_twin(MC.SEEDS[0]), RTOL, 'evaluator a')
    MC.same_counts(b.counts(), random_twin(MC.SEEDS[1]), RTOL, 'evaluator b')


# ------------------------------------------------------------------------------------------------ overflow
def test_overflow_is_counted_and_nothing_is_written_past_a_table():
    """gt_capacity 4 with 6 ground-truth identities, track_capacity 8 with track ids 3 .. 12, and one frame with more rows than ng: a
    bounds check by construction - what is beyond a capacity is counted and left out, results() raises, and the memory behind every
    state tensor and behind the workspace keeps its canary."""
    from tamtr_amd import ops
    from tamtr_amd.track import MotOverflow
    G_, T_, pad = 4, 8, 64
    ev = evaluator(1, nq=12, ng=8, G=G_, Tcap=T_)
    big = {}
    for k, dt, shape in ops.MOT_STATE_SPEC:
        sh = shape(1, (G_, T_))
        big[k] = torch.full((sh[0] + pad,) + sh[1:], 77, dtype=dt, device='cuda')
        big[k][:sh[0]] = 0
        ev.state[k] = big[k][:sh[0]]
    need = ops.mot_workspace_bytes(12, 8, 1, G_, T_)
    ws = torch.full((need + 4096,), 77, dtype=torch.uint8, device='cuda')
    ev.workspace = ws[:need]
    boxes = [(60 * i, 0, 60 * i + 40, 40) for i in range(10)]
    gt = [MC.G(boxes[i], 101 + i) for i in range(6)]
    trk = [MC.T(boxes[i], 3 + i) for i in range(10)]
    f1, f2 = MC.frame(gt, trk), MC.frame(gt + [MC.G((900, 0, 940, 40), 200 + i, 0, 1) for i in range(4)], trk)     # 10 rows > ng = 8
    tracks, tc = pack([f1[1], f2[1]], ev.nq)
    ev.update(tracks, tc, [f1[0], f2[0]])
    ev.end_sequence()
    torch.cuda.synchronize()
    hdr = ev.state['hdr'].cpu().numpy()
    assert hdr.tolist() == [0, 4, 10, 2, 0, 0, 0, 0]      # per frame 2 gt identities beyond 4 and ids 8 .. 12; 2 rows beyond ng
    for k, dt, shape in ops.MOT_STATE_SPEC:
        assert bool((big[k][shape(1, (G_, T_))[0]:] == 77).all()), f'{k}: written past the table'
    assert bool((ws[need:] == 77).all()), 'written past the workspace'
    with pytest.raises(MotOverflow):
        ev.results()
    # what is inside the capacities is scored: 4 identities with tracks 3 .. 6, in both frames; track 7 is a false positive
    c = ev.state['counts'].cpu().numpy()[0]
    assert c[:6].tolist() == [8, 0, 2, 0, 8, 10] and c[10] == 8


# ------------------------------------------------------------------------------------------------ end to end
def _gt_from(dets, rng):
    """Ground truth for the synthetic frames, made from a plain prediction run: the first six boxes of a frame, slightly moved, are
    objects; the seventh is a distractor."""
    out = []
    for d in dets:
        b = d.boxes.numpy()[:7].astype(np.float64)
        rows = [[*(r[:4] + rng.normal(0, 0.3, 4)), i + 1, r[5], 0 if i < 6 else 1] for i, r in enumerate(b)]
        out.append(np.asarray(rows, np.float32).reshape(-1, 7))
    return out


def test_predictor_track_with_an_evaluator(tmp_path):
    from test_gpu_predict import CONF, IMGSZ, NC, _images, _model, _text_feats
    from tamtr_amd.predict import Predictor
    from tamtr_amd.track import ByteTracker, MotEvaluator
    src = _images(tmp_path)
    names = {i: f'c{i}' for i in range(NC)}
    pred = Predictor(_model().cuda(), names, _text_feats(), imgsz=IMGSZ, conf=CONF, iou=0.7, batch=2, dtype='fp32')
    plain = list(pred.predict(str(src)))
    keys = set(pred.speed())
    scores = np.sort(np.concatenate([d.conf.numpy() for d in plain]))
    trk = ByteTracker('cuda', capacity=256, nq=300, track_high_thresh=float(scores[len(scores) // 2]) * 1.0001,
                      track_low_thresh=float(scores[len(scores) // 8]) * 1.0001, new_track_thresh=float(scores[len(scores) * 3 // 4]) * 1.0001)
    gt = _gt_from(plain, np.random.default_rng(8))
    ev = MotEvaluator('cuda', NC, gt_capacity=64, track_capacity=4096)
    got = list(pred.track(str(src), tracker=trk, gt=gt, evaluator=ev))
    assert [d.path for d in got] == [d.path for d in plain]
    assert pred.speed()['mot'] > 0 and set(pred.speed()) == keys | {'mot'}
    frames = []
    for d, g in zip(got, gt):
        rows = np.zeros((0, 6), np.float32) if d.id is None else np.concatenate([d.boxes.numpy()[:, :4], d.id.numpy()[:, None].astype(np.float32),
                                                                                  d.boxes.numpy()[:, 5:6]], 1)
        frames.append((g, rows))
    want = twin([frames], NC)
    counts = ev.counts()
    print('end to end counts', {k: int(np.sum(v)) for k, v in counts.items()})
    MC.same_counts(counts, want, RTOL, 'end to end')
    assert want['gt_dets'].sum() > 0 and want['trk_dets'].sum() > 0 and want['TP'].sum() > 0
    # without an evaluator nothing changes: the same keys as before
    again = list(pred.track(str(src), tracker=trk))
    assert set(pred.speed()) == keys and [d.path for d in again] == [d.path for d in got]
    MC.same_counts(ev.counts(), want, RTOL, 'the evaluator was touched by a run that did not name it')


def test_track_cli_with_gt_writes_the_metrics(tmp_path):
    """tools/track.py --gt on two sequence directories: mot_metrics.json holds a table per sequence and the overall one, consistent with
    each other, with the result files and with the annotations."""
    from PIL import Image
    from test_gpu_predict import CONF, IMGSZ, NC, _model, _text_feats
    rng = np.random.default_rng(4)
    (tmp_path / 'gt').mkdir()
    n_gt = {}
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
        n_gt[seq] = 4 * n
    sd = _model().state_dict()
    torch.save({'model': sd, 'ema': sd}, tmp_path / 'best.pt')
    names = [f'c{i}' for i in range(NC)]
    np.savez(tmp_path / 'feats.npz', texts=np.array(names), feats=_text_feats().numpy())
    (tmp_path / 'bytetrack.yaml').write_text('tracker_type: bytetrack\ntrack_high_thresh: 0.00004\ntrack_low_thresh: 0.00002\n'
                                             'new_track_thresh: 0.00005\ntrack_buffer: 30\nmatch_thresh: 0.8\n')
    cmd = [sys.executable, os.path.join(ROOT, 'tools', 'track.py'), '--weights', str(tmp_path / 'best.pt'), '--text-feats', str(tmp_path / 'feats.npz'),
           '--names', ','.join(names), '--source', str(tmp_path / 'sequences'), '--tracker', str(tmp_path / 'bytetrack.yaml'), '--imgsz', str(IMGSZ),
           '--batch', '2', '--conf', str(CONF), '--save-mot', '--gt', str(tmp_path / 'gt'), '--project', str(tmp_path / 'runs'), '--name', 'TAMTR',
           '--dtype', 'fp32', '--capacity', '512']
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    out = tmp_path / 'runs' / 'TAMTR'
    m = json.loads((out / 'mot_metrics.json').read_text())
    assert sorted(m['sequences']) == ['uav1', 'uav2'] and res['scored_sequences'] == 2 and 'OVERALL' in r.stdout
    assert set(res['ms_per_image']) == {'load', 'forward', 'postprocess', 'track', 'd2h'} and res['mot_ms_per_image'] > 0
    total_rows = 0
    for seq in ('uav1', 'uav2'):
        a = m['sequences'][seq]['all']
        rows = len((out / f'{seq}.txt').read_text().splitlines())
        assert a['gt_dets'] == n_gt[seq] and a['trk_dets'] + a['drop_region'] + a['drop_distractor'] == rows
        assert a['TP'] + a['FN'] == a['gt_dets'] and a['TP'] + a['FP'] == a['trk_dets']
        total_rows += rows
    o = m['overall']['all']
    for k in MC.COUNT_KEYS:
        assert o[k] == sum(m['sequences'][s]['all'][k] for s in m['sequences']), k
    assert total_rows == res['track_rows'] and res['mot']['FP'] == o['FP'] and res['mot']['FN'] == o['FN']
    assert o['MOTA'] == 1 - (o['FN'] + o['FP'] + o['IDSW']) / o['gt_dets'] == res['mot']['MOTA']
