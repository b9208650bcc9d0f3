"""GPU: tamtr_trackmap_update / tamtr_trackmap_end_sequence (csrc/trackmap.hip) and the run's accumulation through
track.TrackMapEvaluator against the numpy statement of the rule (engine.track_map_evaluate / track_map_summary) and the hand-worked
literals of tests/trackmap_cases.py; Predictor.track with three evaluators and tools/track.py --track-map.

Tolerances: a row's bits and class, gt_tracks, tracks and the -1 pattern are equal.  Scores, AP and AR are allowed 1e-9 relative, the
bound tests/test_gpu_mot.py and test_gpu_hota.py give fp64 sums; test_trackmap_host.py asserts margins of 1e-6 on every case used here,
so that bound cannot flip a threshold test, a pick or the order of two tracks.  Observed on the MI355X: equal bits
everywhere - every score, AP and AR of every test below has the statement's bits (the last test prints it)."""
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
from test_gpu_mot import _gt_from

pytestmark = pytest.mark.gpu
RTOL = 1e-9
UNEQUAL = []      # what differed from the statement in its last bits, for the line printed by the last test


def evaluator(nc, nq=8, ng=8, G=16, Tcap=32, P=256, R=256, **kw):
    from tamtr_amd.track import TrackMapEvaluator
    return TrackMapEvaluator('cuda', nc, gt_capacity=G, track_capacity=Tcap, pair_capacity=P, row_capacity=R, nq=nq, ng=ng, **kw)


def pack(trks, nq):
    rows = np.zeros((len(trks), nq, 8), np.float32)
    for b, t in enumerate(trks):
        rows[b, :len(t)] = TC.device_rows(t)
    return torch.from_numpy(rows).cuda(), torch.tensor([len(t) for t in trks], dtype=torch.int32).cuda()


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


def twin(key, sequences, nc, **kw):
    """engine.track_map_evaluate of the sequences and its summary, computed once per key and shared."""
    if key not in _TWIN:
        from tamtr_amd.engine import track_map_evaluate, track_map_summary
        c = track_map_evaluate(sequences, nc, **kw)
        _TWIN[key] = (c, track_map_summary(c))
    return _TWIN[key]


def seeded_twin(name):
    return twin(('seeded', name), *TC.seeded_cases()[name])


def same_counts(got, want, what):
    for k in ('cls', 'bits', 'gt_tracks'):
        assert got[k].tolist() == want[k].tolist(), f'{what}: {k} {got[k].tolist()} != {want[k].tolist()}'
    assert got['thresholds'].tolist() == want['thresholds'].tolist()
    assert got['score'].shape == want['score'].shape and np.allclose(got['score'], want['score'], rtol=RTOL, atol=0), f'{what}: scores'
    if got['score'].tolist() != want['score'].tolist():
        UNEQUAL.append(f'{what}: scores')


def same_summary(got, want, what):
    rows = [(got['all'], want['all'])] + list(zip(got['per_class'], want['per_class']))
    for g, w in rows:
        assert g['gt_tracks'] == w['gt_tracks'] and g['tracks'] == w['tracks'], f'{what}: {g} != {w}'
        for k in ('AP_thr', 'AR_thr'):
            assert [v == -1 for v in g[k]] == [v == -1 for v in w[k]], f'{what}: the -1 pattern of {k}'
            assert np.allclose(g[k], w[k], rtol=RTOL, atol=0), f'{what}: {k} {g[k]} != {w[k]}'
            if g[k] != w[k]:
                UNEQUAL.append(f'{what}: {k}')
        assert (g['AP'] == -1) == (w['AP'] == -1) and abs(g['AP'] - w['AP']) <= RTOL * abs(w['AP'])


def sequence_state_is_clear(ev):
    sd = {k: v.cpu().numpy() for k, v in ev.state.items()}
    return not any(sd[k].any() for k in ('gstate', 'garea', 'tframes', 'tsum', 'pkey', 'pinter')) and not sd['hdr'][2:].any()


# ------------------------------------------------------------------------------------------------ hand-worked cases
@pytest.mark.parametrize('name', sorted(TC.HAND))
def test_hand_cases_in_every_grouping(name):
    sequences, nc = TC.HAND[name][:2]
    want, wsum = twin(('hand', name), sequences, nc)
    got = {}
    for B in (1, 4, 5, 0):
        ev = evaluator(nc)
        got[B] = run(ev, sequences, B)
        same_counts(got[B], want, f'{name} B {B}')
        res = ev.results()
        same_summary(res, wsum, f'{name} B {B}')
        TC.check_expected(got[B], res, name)
        assert sequence_state_is_clear(ev), 'the per-sequence state is not cleared'
        assert ev.state['hdr'].cpu().tolist()[:2] == [len(want['score']), len(sequences)]
        assert got[B]['score'].tolist() == got[1]['score'].tolist(), f'{name}: B {B} and B 1 differ'


# ------------------------------------------------------------------------------------------------ seeded sequences
@pytest.mark.parametrize('seed', MC.SEEDS)
def test_random_sequence_in_every_grouping(seed):
    sequences, nc = TC.seeded_cases()[f'seed{seed}']
    want, wsum = seeded_twin(f'seed{seed}')
    assert len(sequences[0]) == 12 and len(want['score']) > 8
    got = {}
    for B in (1, 4, 5, 0):
        ev = evaluator(nc, nq=12, ng=12, G=32, Tcap=256)
        got[B] = run(ev, sequences, B)
        same_counts(got[B], want, f'seed {seed} B {B}')
        same_summary(ev.results(), wsum, f'seed {seed} B {B}')
        assert got[B]['score'].tolist() == got[1]['score'].tolist(), f'seed {seed}: B {B} and B 1 differ'


def test_ten_thresholds():
    """TrackEval's thresholds on the cluster, whose IoUs lie between them: ten waves per class in the matching launch, ten bits per row."""
    sequences, nc = TC.seeded_cases()['cluster']
    thr = np.linspace(0.5, 0.95, 10)
    want, wsum = twin('ten', sequences, nc, thresholds=thr)
    assert len(set(want['bits'].tolist())) >= 3 and want['bits'].max() == 1023 and (want['bits'] != 1023).any()
    ev = evaluator(nc, nq=72, ng=72, G=128, Tcap=512, P=16384, R=128, thresholds=thr)
    same_counts(run(ev, sequences, 3), want, 'ten thresholds')
    res = ev.results()
    same_summary(res, wsum, 'ten thresholds')
    assert len(res['all']['AP_thr']) == 10 and res['thresholds'] == thr.tolist()


def test_crowded_sequence_crosses_the_wave_width():
    sequences, nc = TC.seeded_cases()['crowded']
    want, wsum = seeded_twin('crowded')
    for B in (1, 4):
        ev = evaluator(nc, nq=72, ng=72, G=128, Tcap=512, P=4096, R=512)
        same_counts(run(ev, sequences, B), want, f'crowded B {B}')
        same_summary(ev.results(), wsum, f'crowded B {B}')


def test_dense_cluster_has_more_candidates_than_a_wave():
    """70 x 70 with every pair intersecting: every track has 70 candidates, more than the 64 lanes that stride over them."""
    sequences, nc = TC.seeded_cases()['cluster']
    want, wsum = seeded_twin('cluster')
    assert len(want['score']) == 70 and want['gt_tracks'].tolist() == [70] and int((want['bits'] & 1).sum()) > 35
    for B in (1, 3):
        ev = evaluator(nc, nq=72, ng=72, G=128, Tcap=512, P=16384, R=128)
        same_counts(run(ev, sequences, B), want, f'cluster B {B}')
        same_summary(ev.results(), wsum, f'cluster B {B}')


def test_more_tracks_than_a_workgroup_has_threads():
    """300 track identities in one class: the ranking launch takes two tiles of 256 and two workgroups for the class."""
    sequences, nc = TC.seeded_cases()['many_tracks']
    want, wsum = seeded_twin('many_tracks')
    assert len(want['score']) == 300 and (np.diff(want['score']) < 0).all()
    for B in (1, 0):
        ev = evaluator(nc, nq=100, ng=100, G=128, Tcap=512, P=2048, R=512)
        same_counts(run(ev, sequences, B), want, f'many tracks B {B}')
        same_summary(ev.results(), wsum, f'many tracks B {B}')


def test_empty_frames_inside_a_batch():
    g, t = TC.frame([TC.G(TC.B(0), 1), TC.G(TC.B(1), 2)], [TC.T(TC.B(0), 1, 0.9), TC.T(TC.B(1), 2, 0.8), TC.T(TC.B(2), 3, 0.7)])
    none_g, none_t = TC.frame()
    seq = [(g, t), (none_g, t), (g, none_t), (none_g, none_t), (g, t)]
    want, wsum = twin('empty', [seq], 1)
    assert want['bits'].tolist() == [3, 3, 0] and want['gt_tracks'].tolist() == [2]      # IoU 2 / (3 + 3 - 2) = 0.5
    for B in (5, 2):
        ev = evaluator(1)
        same_counts(run(ev, [seq], B), want, f'empty frames B {B}')
        same_summary(ev.results(), wsum, f'empty frames B {B}')
    ev = evaluator(2)
    only_empty = run(ev, [[(none_g, none_t)] * 3], 3)
    assert len(only_empty['score']) == 0 and not only_empty['gt_tracks'].any() and ev.state['hdr'].cpu().tolist() == [0, 1] + [0] * 14
    res = ev.results()
    assert res['all']['AP'] == -1.0 and res['per_class'][1]['AP_thr'] == [-1.0] * 3 and res['all']['tracks'] == 0


# ------------------------------------------------------------------------------------------------ sequences, reset, evaluators
def test_two_sequences_then_results():
    seqs = TC.seeded_cases()['seed11'][0] + TC.seeded_cases()['seed12'][0]
    ev = evaluator(2, nq=12, ng=12, G=32, Tcap=256)
    want, wsum = twin('two', seqs, 2)
    same_counts(run(ev, seqs, 5), want, 'two sequences')
    res = ev.results(['a', 'b'])
    same_summary(res, wsum, 'two sequences')
    assert res['per_class'][1]['class'] == 'b' and ev.state['hdr'].cpu().tolist()[:2] == [len(want['score']), 2]
    feed(ev, seqs[0][:1], 1, end=False)
    with pytest.raises(RuntimeError, match='end_sequence'):
        ev.results()
    with pytest.raises(RuntimeError, match='end_sequence'):
        ev.counts()


def test_reset():
    seq = TC.seeded_cases()['seed11'][0][0]
    ev = evaluator(2, nq=12, ng=12, G=32, Tcap=256)
    feed(ev, seq, 4)
    feed(ev, seq[:5], 5, end=False)      # a sequence left open
    ev.reset()
    assert all(not bool(v.any()) for v in ev.state.values())
    same_counts(run(ev, [seq], 4), seeded_twin('seed11')[0], 'after reset')


def test_two_evaluators_used_alternately():
    sa, sb = TC.seeded_cases()['seed11'][0][0], TC.seeded_cases()['seed12'][0][0]
    a, b = evaluator(2, nq=12, ng=12, G=32, Tcap=256), evaluator(2, nq=12, ng=12, G=32, Tcap=256)
    for i in range(0, 12, 3):
        for ev, seq in ((a, sa), (b, sb)):
            feed(ev, seq[i:i + 3], 3, end=False)
    a.end_sequence(), b.end_sequence()
    same_counts(a.counts(), seeded_twin('seed11')[0], 'evaluator a')
    same_counts(b.counts(), seeded_twin('seed12')[0], 'evaluator b')
    same_summary(a.results(), seeded_twin('seed11')[1], 'evaluator a')


def test_mot_and_hota_evaluators_in_company_keep_their_counts():
    import hota_cases as HC
    from tamtr_amd.engine import hota_evaluate, mot_evaluate
    from tamtr_amd.track import HotaEvaluator, MotEvaluator
    seq = TC.seeded_cases()['seed13'][0][0]
    plain = [(g, t[:, :6]) for g, t in seq]
    mot = MotEvaluator('cuda', 2, gt_capacity=32, track_capacity=256, nq=12, ng=12)
    hota = HotaEvaluator('cuda', 2, gt_capacity=32, track_capacity=256, pair_capacity=256, log_capacity=1024, frame_capacity=128, nq=12, ng=12)
    tmap = evaluator(2, nq=12, ng=12, G=32, Tcap=256)
    for i in range(0, 12, 4):
        tracks, tc = pack([t for _, t in seq[i:i + 4]], 12)
        gts = [g for g, _ in seq[i:i + 4]]
        for ev in (mot, tmap, hota):
            ev.update(tracks, tc, gts)
    for ev in (tmap, mot, hota):
        ev.end_sequence()
    MC.same_counts(mot.counts(), mot_evaluate([plain], 2), RTOL, 'MOT next to track-mAP')
    HC.same_counts(hota.counts(), hota_evaluate([plain], 2), RTOL, 'HOTA next to track-mAP')
    same_counts(tmap.counts(), seeded_twin('seed13')[0], 'track-mAP next to MOT and HOTA')


# ------------------------------------------------------------------------------------------------ overflow
PAD = 77


def padded(ev):
    """Move the evaluator's state and workspace into tensors with a canary behind each -> a check that every canary is intact."""
    from tamtr_amd import ops
    big = {}
    for k, dt, shape in ops.TRACKMAP_STATE_SPEC:
        sh = shape(ev.nc, ev.caps)
        big[k] = torch.full((sh[0] + 64,) + sh[1:], PAD, dtype=dt, device='cuda')
        big[k][:sh[0]] = 0
        ev.state[k] = big[k][:sh[0]]
    need = ops.trackmap_workspace_bytes(ev.nq, ev.ng, ev.nc, ev.caps)
    ws = torch.full((need + 4096,), PAD, dtype=torch.uint8, device='cuda')
    ev.workspace = ws[:need]

    def intact():
        torch.cuda.synchronize()
        for k, dt, shape in ops.TRACKMAP_STATE_SPEC:
            assert bool((big[k][shape(ev.nc, ev.caps)[0]:] == PAD).all()), f'{k}: written past the table'
        assert bool((ws[need:] == PAD).all()), 'written past the workspace'
    return intact


def isolated(n, first_gt=1, first_trk=1):
    """One frame of n ground truths far apart, each with a track exactly on it; the scores fall with the track id."""
    return TC.frame([TC.G(TC.B(i), first_gt + i) for i in range(n)], [TC.T(TC.B(i), first_trk + i, 0.9 - 0.05 * i) for i in range(n)])


def clean_after_reset(ev, intact, what):
    ev.reset()
    seqs = [[isolated(2)] * 2]
    want, wsum = twin('iso2', seqs, 1)
    same_counts(run(ev, seqs, 1), want, f'{what}: inside the capacity after reset')
    same_summary(ev.results(), wsum, f'{what}: after reset')
    intact()


def test_ids_and_rows_beyond_capacity_are_counted_and_left_out():
    """gt_capacity 4 with 6 identities, track_capacity 8 with ids 3 .. 12, and a frame with more rows than ng.  What is inside the
    capacities is scored: 4 identities with tracks 3 .. 6 in both frames; track 7 is a false positive behind them."""
    from tamtr_amd.track import TrackMapOverflow
    ev = evaluator(1, nq=12, ng=8, G=4, Tcap=8)
    intact = padded(ev)
    f1 = isolated(10, 101, 3)
    f1 = (f1[0][:6], f1[1])
    f2 = (np.concatenate([f1[0], np.asarray([TC.G((900, 0, 940, 40), 200 + i, 0, 1) for i in range(4)], np.float32)]), f1[1])     # 10 rows > ng
    feed(ev, [f1, f2], 2)
    intact()
    assert ev.state['hdr'].cpu().tolist() == [5, 1, 4, 10, 2, 0, 0] + [0] * 9
    with pytest.raises(TrackMapOverflow, match='gt identities'):
        ev.results()
    with pytest.raises(TrackMapOverflow, match='track ids'):
        ev.counts()
    assert ev.state['rmeta'].cpu()[:6].tolist() == [[0, 7]] * 4 + [[0, 0]] * 2 and ev.state['gt_tracks'].cpu().tolist() == [4]
    assert ev.state['rscore'].cpu()[:5].tolist() == [TC.f32(0.9 - 0.05 * i) for i in range(5)]
    clean_after_reset(ev, intact, 'ids and rows')


def test_track_rows_beyond_nq_are_counted_and_left_out():
    from tamtr_amd.track import TrackMapOverflow
    ev = evaluator(1, nq=3, ng=8)
    intact = padded(ev)
    g, t = isolated(4)
    tracks, _ = pack([t[:3]], 3)
    ev.update(tracks, torch.tensor([4], dtype=torch.int32).cuda(), [g])      # four rows announced, three fit
    ev.end_sequence()
    intact()
    assert ev.state['hdr'].cpu().tolist() == [3, 1, 0, 0, 1, 0, 0] + [0] * 9
    assert ev.state['rmeta'].cpu()[:4].tolist() == [[0, 7]] * 3 + [[0, 0]] and ev.state['gt_tracks'].cpu().tolist() == [4]
    with pytest.raises(TrackMapOverflow, match='nq'):
        ev.results()
    clean_after_reset(ev, intact, 'nq')


def test_pair_table_beyond_capacity():
    """4 pairs and 3 slots: one pair finds no slot, in each of three frames; the other three tracks are matched."""
    from tamtr_amd.track import TrackMapOverflow
    ev = evaluator(1, P=3)
    intact = padded(ev)
    feed(ev, [isolated(4)] * 3, 0)
    intact()
    assert ev.state['hdr'].cpu().tolist() == [4, 1, 0, 0, 0, 3, 0] + [0] * 9
    assert sorted(ev.state['rmeta'].cpu()[:4, 1].tolist()) == [0, 7, 7, 7] and sequence_state_is_clear_but_hdr(ev)
    with pytest.raises(TrackMapOverflow, match='pair_capacity'):
        ev.counts()
    clean_after_reset(ev, intact, 'pairs')


def sequence_state_is_clear_but_hdr(ev):
    return not any(bool(ev.state[k].any()) for k in ('gstate', 'garea', 'tframes', 'tsum', 'pkey', 'pinter'))


def test_run_table_beyond_capacity():
    """row_capacity 3 and two sequences of two tracks: the second sequence's better track fits, the other is counted."""
    from tamtr_amd.track import TrackMapOverflow
    ev = evaluator(1, R=3)
    intact = padded(ev)
    feed(ev, [isolated(2)] * 2, 2)
    assert ev.state['hdr'].cpu().tolist() == [2, 1] + [0] * 14
    feed(ev, [isolated(2, 1, 5)] * 2, 2)
    intact()
    assert ev.state['hdr'].cpu().tolist() == [3, 2, 0, 0, 0, 0, 1] + [0] * 9
    assert ev.state['rmeta'].cpu().tolist() == [[0, 7]] * 3 and ev.state['rscore'].cpu().tolist() == [TC.f32(0.9), TC.f32(0.85), TC.f32(0.9)]
    assert ev.state['gt_tracks'].cpu().tolist() == [4] and sequence_state_is_clear_but_hdr(ev)
    feed(ev, [isolated(1)], 1)                                   # a full table takes nothing more
    intact()
    assert ev.state['hdr'].cpu().tolist() == [3, 3, 0, 0, 0, 0, 2] + [0] * 9
    with pytest.raises(TrackMapOverflow, match='row_capacity'):
        ev.results()
    clean_after_reset(ev, intact, 'run rows')


def test_header_check_raises_before_the_results_are_read():
    from tamtr_amd.track import TrackMapOverflow
    ev = evaluator(1, Tcap=2)
    feed(ev, [isolated(2, 1, 1)] * 2, 2, end=False)              # track id 2 is beyond track_capacity 2
    with pytest.raises(TrackMapOverflow, match='track_capacity'):
        ev.check_overflow(ev.state['hdr'].cpu().numpy())


def test_bad_or_unsupported_operands_raise_before_any_launch():
    from tamtr_amd import TamtrHipError, ops
    ev = evaluator(1)
    g, t = isolated(2)
    tracks, tc = pack([t], ev.nq)
    gt, gc = ev.upload([g])
    before = {k: v.clone() for k, v in ev.state.items()}
    small = torch.empty(64, dtype=torch.uint8, device='cuda')
    with pytest.raises(TamtrHipError, match='workspace'):
        ops.trackmap_update(tracks, tc, gt, gc, ev.state, 1, ev.caps, 0.5, small)
    with pytest.raises(TamtrHipError, match='workspace'):
        ops.trackmap_end_sequence(ev.state, 1, ev.caps, TC.THRESHOLDS, small)
    with pytest.raises(TamtrHipError, match='gt'):
        ops.trackmap_update(tracks, tc, gt[:, :, :6], gc, ev.state, 1, ev.caps)
    with pytest.raises(TamtrHipError, match='float32'):
        ops.trackmap_update(tracks.double(), tc, gt, gc, ev.state, 1, ev.caps)
    with pytest.raises(TamtrHipError, match='MI355X'):
        ops.trackmap_update(tracks.cpu(), tc, gt, gc, ev.state, 1, ev.caps)
    with pytest.raises(TamtrHipError, match='tsum'):
        ops.trackmap_update(tracks, tc, gt, gc, {**ev.state, 'tsum': ev.state['tsum'][:, :, :1]}, 1, ev.caps)
    with pytest.raises(TamtrHipError, match='thresholds'):
        ops.trackmap_end_sequence(ev.state, 1, ev.caps, [0.5] * 11)
    with pytest.raises(TamtrHipError, match='outside'):          # more classes than the kernels are built for
        ops.trackmap_workspace_bytes(8, 8, 5000, ev.caps)
    wide = torch.zeros(1, 4000, 8, device='cuda')
    with pytest.raises(TamtrHipError, match='EUNSUP'):           # solver state beyond the LDS
        ops.trackmap_update(wide, tc, torch.zeros(1, 4000, 7, device='cuda'), gc, ev.state, 1, ev.caps)
    torch.cuda.synchronize()
    assert all(torch.equal(v, before[k]) for k, v in ev.state.items()), 'a refused call touched the state'


# ------------------------------------------------------------------------------------------------ end to end
def test_predictor_track_with_three_evaluators(tmp_path):
    import hota_cases as HC
    from test_gpu_predict import CONF, IMGSZ, NC, _images, _model, _text_feats
    from tamtr_amd.engine import hota_evaluate, mot_evaluate, track_map_evaluate, track_map_summary
    from tamtr_amd.predict import Predictor
    from tamtr_amd.track import ByteTracker, HotaEvaluator, MotEvaluator, TrackMapEvaluator
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
    tmap = TrackMapEvaluator('cuda', NC, gt_capacity=64, track_capacity=4096, pair_capacity=4096, row_capacity=4096)
    got = list(pred.track(str(src), tracker=trk, gt=gt, evaluator=[mot, hota, tmap]))
    assert [d.path for d in got] == [d.path for d in plain]
    assert pred.speed()['tmap'] > 0 and set(pred.speed()) == keys | {'mot', 'hota', 'tmap'}
    frames = []
    for d, g in zip(got, gt):
        b = d.boxes.numpy()
        rows = np.zeros((0, 7), np.float32) if d.id is None else np.concatenate([b[:, :4], d.id.numpy()[:, None].astype(np.float32), b[:, 5:6], b[:, 4:5]], 1)
        frames.append((g, rows))
    want = track_map_evaluate([frames], NC)
    counts = tmap.counts()
    print('end to end track-mAP', counts['bits'].tolist(), 'margins', TC.margins([frames], NC))
    same_counts(counts, want, 'end to end')
    same_summary(tmap.results(), track_map_summary(want), 'end to end')
    assert want['gt_tracks'].sum() > 0 and len(want['score']) > 0 and (want['bits'] & 1).any()
    six = [(g, t[:, :6]) for g, t in frames]
    MC.same_counts(mot.counts(), mot_evaluate([six], NC), RTOL, 'end to end, MOT in company')
    HC.same_counts(hota.counts(), hota_evaluate([six], NC), RTOL, 'end to end, HOTA in company')
    # without the evaluator the key is gone, and a run that does not name it leaves it alone
    list(pred.track(str(src), tracker=trk, gt=gt, evaluator=[mot, hota]))
    assert set(pred.speed()) == keys | {'mot', 'hota'}
    list(pred.track(str(src), tracker=trk))
    assert set(pred.speed()) == keys
    same_counts(tmap.counts(), want, 'the evaluator was touched by a run that did not name it')


def test_track_cli_with_gt_and_track_map_writes_the_key(tmp_path):
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
           '--batch', '2', '--conf', str(CONF), '--save-mot', '--gt', str(tmp_path / 'gt'), '--track-map', '--project', str(tmp_path / 'runs'),
           '--name', 'TAMTR', '--dtype', 'fp32', '--capacity', '512']
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    m = json.loads((tmp_path / 'runs' / 'TAMTR' / 'mot_metrics.json').read_text())
    assert list(m) == ['iou', 'sequences', 'overall', 'track_map'] and sorted(m['track_map']['sequences']) == ['uav1', 'uav2']
    assert 'AP@0.25' in r.stdout and 'AP@0.75' in r.stdout and 'MOTA' in r.stdout and res['tmap_ms_per_image'] > 0 and 'hota' not in res
    o = m['track_map']['overall']
    assert o['thresholds'] == [0.25, 0.5, 0.75] and res['track_map']['AP'] == o['all']['AP'] and len(o['per_class']) == NC
    assert o['all']['gt_tracks'] == sum(s['all']['gt_tracks'] for s in m['track_map']['sequences'].values()) > 0
    assert o['all']['tracks'] == sum(s['all']['tracks'] for s in m['track_map']['sequences'].values())
    assert all(-1.0 <= v <= 1.0 for v in o['all']['AP_thr'])


def test_zz_report_whether_the_bits_were_equal():
    """Not a check: prints what differed from the statement in its last bits over the tests above (nothing: equal bits)."""
    print('track-mAP, device against statement:', 'equal bits everywhere' if not UNEQUAL else f'{len(UNEQUAL)} differences: {UNEQUAL[:20]}')
