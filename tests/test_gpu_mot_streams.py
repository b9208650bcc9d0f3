"""GPU: several streams scored at once - tamtr_mot_update_streams / tamtr_mot_end_streams (csrc/mot.hip) and tamtr_hota_update_streams /
tamtr_hota_end_streams (csrc/hota.hip) through track.MotEvaluator(streams=S) / track.HotaEvaluator(streams=S): every stream of a
stack against the numpy statement of the rule on its own sequence (engine.mot_evaluate / engine.hota_evaluate) and against a single
evaluator fed alone; Predictor.track_streams with gt and both evaluators; tools/mot_eval.py --streams.

Tolerances, those of test_gpu_mot.py and test_gpu_hota.py for the same reason: integer counts and all integer state are equal;
iou_sum, loc_lvl and ass are fp64 sums the device adds with atomics within one stream, so reordering moves them by about n * 2^-53 of
their value: 1e-9 relative.  HOTA's ppot is plain in-order adds: bit-equal.  No sum is shared between streams, so nothing here is
looser than for one evaluator.  The twin's matching is the device's because every sequence has pairwise different scores inside a
frame (mot_cases' generators assert it) and holds hota_cases.unique_optimum (test_hota_host.py asserts it for the seeded sequences,
seeded() below for the prefixes made here).

What of HOTA's open state depends on the order in which threads arrive is compared as what it encodes: a pair's slot in the open-
addressing table is decided by atomicCAS when two new pairs of one frame probe the same slot, and a frame's log entries are appended
through an atomic counter.  So the table is compared as {pair: (pot, histogram)} and a frame's log as the set of its entries with
the slot replaced by the pair; every other tensor is compared where it lies."""
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
KINDS = ('mot', 'hota')
SAME = {'mot': MC.same_counts, 'hota': HC.same_counts}
MOT_SEQUENCE_STATE, HOTA_SEQUENCE_STATE = ('gstate', 'pair', 'hdr'), ('gstate', 'tcount', 'pkey', 'ppot', 'phist', 'hdr')


def evaluator(kind, nc, streams=None, nq=33, ng=33, G=32, Tcap=256, P=256, L=1024, F=128):
    from tamtr_amd.track import HotaEvaluator, MotEvaluator
    if kind == 'mot':
        return MotEvaluator('cuda', nc, gt_capacity=G, track_capacity=Tcap, nq=nq, ng=ng, streams=streams)
    return HotaEvaluator('cuda', nc, gt_capacity=G, track_capacity=Tcap, pair_capacity=P, log_capacity=L, frame_capacity=F, nq=nq, ng=ng,
                         streams=streams)


_TWIN = {}


def twin(kind, key, sequences, nc):
    """engine.mot_evaluate / engine.hota_evaluate of the sequences, computed once per key and shared."""
    if (kind, key) not in _TWIN:
        from tamtr_amd import engine
        _TWIN[kind, key] = (engine.mot_evaluate if kind == 'mot' else engine.hota_evaluate)(sequences, nc)
    return _TWIN[kind, key]


_CHECKED = set()


def seeded(seed, n=None):
    """The first n frames of a seeded sequence of mot_cases.  A prefix is a sequence of its own for HOTA (pot is a sum over the whole
    sequence), so its precondition is asserted here, once: forbidding any matched pair loses at least 1e-9 of a frame's total."""
    seq = MC.random_cases()[seed][0][:n]
    if n is not None and (seed, n) not in _CHECKED:
        assert HC.unique_optimum(seq, 2) >= 1e-9, f'seed {seed}, first {n} frames'
        _CHECKED.add((seed, n))
    return seq


DECOY = MC.frame([], [MC.T(MC.BOX_A, 1), MC.T(MC.BOX_B, 2)])[1]      # the track rows of an image that is no frame: counted if ever read


def batch(ev, streams, start, F):
    """Frames start .. start + F - 1 of every stream as one frame-major update.  An entry of a stream that is None, or a stream past
    its end, is an image that is no frame; it carries two decoy track rows."""
    S = len(streams)
    at = [(start + j // S, j % S) for j in range(F * S)]
    frames = [streams[s][n] if n < len(streams[s]) else None for n, s in at]
    tracks, tc = pack([DECOY if f is None else f[1] for f in frames], ev.nq)
    ev.update(tracks, tc, [None if f is None else f[0] for f in frames])


def feed(ev, streams, F):
    """All the streams, F frames of each per launch; the streams whose last frame a batch holds are ended right after it, in one call."""
    for k in range(0, max(len(s) for s in streams), F):
        batch(ev, streams, k, F)
        ending = [s for s, seq in enumerate(streams) if seq and (len(seq) - 1) // F == k // F]
        if ending:
            ev.end_sequence(ending)


def feed_single(ev, seq, F, end=True):
    for i in range(0, len(seq), F):
        chunk = [f for f in seq[i:i + F] if f is not None]
        if chunk:
            tracks, tc = pack([t for _, t in chunk], ev.nq)
            ev.update(tracks, tc, [g for g, _ in chunk])
    if end:
        ev.end_sequence()


def host(ev, s=None):
    return {k: (v if s is None else v[s]).cpu().numpy() for k, v in ev.state.items()}


def sequence_state_is_clear(kind, sd):
    return not any(sd[k].any() for k in (MOT_SEQUENCE_STATE if kind == 'mot' else HOTA_SEQUENCE_STATE))


def hota_open_state(sd):
    """What HOTA's open state encodes, free of the order threads arrived in: {pair: (pot, histogram)} and per frame (n, m, the set of
    (row, column, S, pair))."""
    used = np.flatnonzero(sd['pkey'])
    table = {int(sd['pkey'][i]): (float(sd['ppot'][i]), tuple(sd['phist'][i].tolist())) for i in used}
    assert not sd['ppot'][sd['pkey'] == 0].any() and not sd['phist'][sd['pkey'] == 0].any()
    log = np.ascontiguousarray(sd['log'])
    s_val, slot, ij = log.view(np.float64)[:, 0], log[:, 2], log[:, 3].copy().view(np.uint16).reshape(-1, 2)
    frames = []
    for first, n_entries, n, m in sd['fidx'][:int(sd['hdr'][0])].tolist():
        e = range(first, first + n_entries)
        frames.append((n, m, sorted((int(ij[i, 0]), int(ij[i, 1]), float(s_val[i]), int(sd['pkey'][slot[i]])) for i in e)))
    return table, frames


def same_state(kind, got, want, what):
    """Two states, tensor by tensor: integers equal, ppot bit-equal, the fp64 atomic sums within RTOL."""
    if kind == 'hota':
        assert hota_open_state(got) == hota_open_state(want), f'{what}: the pair table or the log differ'
    skip = ('pkey', 'ppot', 'phist', 'log', 'fidx') if kind == 'hota' else ()
    for k in want:
        if k in skip:
            continue
        a, b = got[k], want[k]
        if a.dtype.kind == 'f':
            assert (np.abs(a - b) <= RTOL * np.abs(b)).all(), f'{what}: {k}'
        else:
            assert np.array_equal(a, b), f'{what}: {k} {a.ravel()[:16]} vs {b.ravel()[:16]}'
    if kind == 'hota':      # the frames logged and the entries used are the first two words of hdr, compared above
        assert np.array_equal(got['fidx'][:int(want['hdr'][0]), 1:], want['fidx'][:int(want['hdr'][0]), 1:]), f'{what}: fidx'


# ------------------------------------------------------------------------------------------------ 1. ragged streams
def ragged():
    return [seeded(11), seeded(12, 7), seeded(13)]


@pytest.mark.parametrize('F', [1, 4, 5])
@pytest.mark.parametrize('kind', KINDS)
def test_ragged_streams_equal_evaluators_fed_alone(kind, F):
    """12, 7 and 12 frames; 5 divides neither 12 nor 7, so padding falls mid-batch and stream 1 ends while the others go on.  nq = ng =
    33: the single workspace is no multiple of 16 bytes, so every slice but the first starts on a rounded offset."""
    from tamtr_amd import ops
    assert ops.mot_workspace_bytes(33, 33, 2, 32, 256) % 16 != 0 and ops.hota_workspace_bytes(33, 33, 1) % 16 != 0
    streams = ragged()
    assert [len(s) for s in streams] == [12, 7, 12] and 12 % 5 and 7 % 5
    ev = evaluator(kind, 2, streams=3)
    assert ev.nq == ev.ng == 33
    feed(ev, streams, F)
    for s, seq in enumerate(streams):
        SAME[kind](ev.stream_counts(s), twin(kind, ('ragged', s), [seq], 2), RTOL, f'{kind} F {F} stream {s}')
        assert sequence_state_is_clear(kind, host(ev, s)), f'stream {s}: the per-sequence state is not cleared'
    SAME[kind](ev.counts(), twin(kind, 'ragged', streams, 2), RTOL, f'{kind} F {F} all streams')
    assert ev.open == [False] * 3 and ev.rows == [{}, {}, {}]


# ------------------------------------------------------------------------------------------------ 2. state isolation
@pytest.mark.parametrize('kind', KINDS)
def test_two_streams_with_the_same_ids_keep_their_own_state(kind):
    seq = seeded(11)
    stack, one = evaluator(kind, 2, streams=2), evaluator(kind, 2)
    for k in range(0, 12, 4):
        batch(stack, [seq, seq], k, 4)
    feed_single(one, seq, 4, end=False)
    want = host(one)
    assert want['hdr'][0] == 12 and not sequence_state_is_clear(kind, want)
    for s in range(2):
        same_state(kind, host(stack, s), want, f'{kind} open stream {s}')
    stack.end_sequence(), one.end_sequence()
    want = host(one)
    for s in range(2):
        same_state(kind, host(stack, s), want, f'{kind} ended stream {s}')
        SAME[kind](stack.stream_counts(s), one.counts(), RTOL, f'{kind} stream {s} against the single evaluator')
        assert sequence_state_is_clear(kind, host(stack, s))
    SAME[kind](stack.counts(), twin(kind, 'twice 11', [seq, seq], 2), RTOL, f'{kind} both streams')


def test_ids_reused_across_streams_are_different_identities():
    """mot_cases' reuse: both sequences call their object 1; stream 0 tracks it as 1, stream 1 as 2.  One state over both streams would
    see an id switch and one identity: IDSW 1, IDTP 2."""
    a, b = MC.HAND['reuse'][0]
    ev = evaluator('mot', 1, streams=2)
    feed(ev, [a, b], 2)
    total = ev.counts()
    MC.same_counts(total, twin('mot', 'reuse', [a, b], 1), RTOL, 'reuse')
    assert total['IDSW'].tolist() == [0] and total['IDTP'].tolist() == [4] and total['gt_ids'].tolist() == [2]
    assert [ev.stream_counts(s)['IDTP'].tolist() for s in range(2)] == [[2], [2]]
    hv = evaluator('hota', 1, streams=2)
    feed(hv, [a, b], 2)
    HC.same_counts(hv.counts(), twin('hota', 'reuse', [a, b], 1), RTOL, 'reuse')
    HC.check_expected(hv.results(), HC.HAND['reuse'][2], 'reuse')


# ------------------------------------------------------------------------------------------------ 3. wide next to tiny
@pytest.mark.parametrize('kind', KINDS)
def test_a_stream_wider_than_a_wave_next_to_a_tiny_one(kind):
    wide, tiny = MC.crowded_sequence(), MC.HAND['A'][0][0]
    assert max(len(g) for g, _ in wide) == 72 and max(len(t) for _, t in wide) == 72 and len(tiny) == 6
    ev = evaluator(kind, 3, streams=2, nq=72, ng=72, G=128, Tcap=512, P=4096, L=8192)
    feed(ev, [wide, tiny], 4)
    SAME[kind](ev.stream_counts(0), twin(kind, 'crowded', [wide], 3), RTOL, f'{kind} crowded stream')
    SAME[kind](ev.stream_counts(1), twin(kind, 'A of 3', [tiny], 3), RTOL, f'{kind} tiny stream')
    if kind == 'mot':
        assert ev.stream_counts(1)['TP'].tolist() == [5, 0, 0] and ev.stream_counts(0)['IDSW'].sum() > 0


# ------------------------------------------------------------------------------------------------ 4. partial end and restart
@pytest.mark.parametrize('kind', KINDS)
def test_one_stream_ends_and_starts_over_while_the_other_goes_on(kind):
    seq0, seq1a, seq1b = seeded(11), seeded(12, 6), seeded(13, 6)      # 1b reuses 1a's ground-truth ids 1 .. 6 and track ids
    assert {int(i) for g, _ in seq1a for i in g[:, 4]} & {int(i) for g, _ in seq1b for i in g[:, 4]}
    ev = evaluator(kind, 2, streams=2)
    for k in (0, 3):
        batch(ev, [seq0, seq1a], k, 3)
    keys = MOT_SEQUENCE_STATE if kind == 'mot' else HOTA_SEQUENCE_STATE + ('fidx', 'log')
    before = {k: ev.state[k][0].clone() for k in keys}
    assert any(bool(v.any()) for v in before.values()) and ev.open == [True, True]
    ev.end_sequence([1])
    assert ev.open == [True, False] and ev.rows[1] == {} and len(ev.rows[0]) > 0
    with pytest.raises(RuntimeError, match='end_sequence'):
        ev.results()
    with pytest.raises(RuntimeError, match='end_sequence'):
        ev.stream_counts(0)
    SAME[kind](ev.stream_counts(1), twin(kind, '12[:6]', [seq1a], 2), RTOL, f'{kind} stream 1 after its first sequence')
    for k, v in before.items():
        assert torch.equal(ev.state[k][0], v), f'{kind}: the end of stream 1 touched state[{k!r}] of stream 0'
    assert sequence_state_is_clear(kind, host(ev, 1))
    tail = [None] * 6
    for k in (6, 9):
        batch(ev, [seq0, tail + seq1b], k, 3)
    ev.end_sequence()
    SAME[kind](ev.stream_counts(0), twin(kind, ('ragged', 0), [seq0], 2), RTOL, f'{kind} stream 0')
    SAME[kind](ev.stream_counts(1), twin(kind, '12[:6] 13[:6]', [seq1a, seq1b], 2), RTOL, f'{kind} stream 1, two sequences')
    SAME[kind](ev.counts(), twin(kind, '11 12[:6] 13[:6]', [seq0, seq1a, seq1b], 2), RTOL, f'{kind} run')
    ev.results()
    ev.reset(stream=1)
    assert not any(bool(v[1].any()) for v in ev.state.values())
    SAME[kind](ev.counts(), twin(kind, ('ragged', 0), [seq0], 2), RTOL, f'{kind} after reset(stream=1)')


# ------------------------------------------------------------------------------------------------ 5. overflow is per stream
@pytest.mark.parametrize('kind', KINDS)
def test_an_overflowing_stream_leaves_its_neighbour_and_the_memory_around_alone(kind):
    """gt_capacity 4: stream 1 brings 6 ground-truth identities, stream 0 brings 2.  Canaries after every stacked tensor and after the
    workspace."""
    from tamtr_amd import ops
    from tamtr_amd.track import HotaOverflow, MotOverflow
    G_, S, pad = 4, 2, 64
    ev = evaluator(kind, 1, streams=S, nq=12, ng=12, G=G_, Tcap=32)
    big = {}
    for k, dt, shape in ev.spec:
        sh = shape(1, ev.caps)
        big[k] = torch.full((S * sh[0] + pad,) + sh[1:], 77, dtype=dt, device='cuda')
        big[k][:S * sh[0]] = 0
        ev.state[k] = big[k][:S * sh[0]].view((S,) + sh)
    need = ev._ws_bytes()
    assert need == (ops.mot_workspace_bytes(12, 12, 1, G_, 32, S) if kind == 'mot' else ops.hota_workspace_bytes(12, 12, streams=S))
    ws = torch.full((need + 4096,), 77, dtype=torch.uint8, device='cuda')
    ev.workspace = ws[:need]
    boxes = [(60 * i, 0, 60 * i + 40, 40) for i in range(6)]
    crowd = [MC.frame([MC.G(boxes[i], 101 + i) for i in range(6)], [MC.T(boxes[i], 3 + i) for i in range(6)])] * 2
    calm = MC.HAND['B'][0][0]
    feed(ev, [calm, crowd], 2)
    torch.cuda.synchronize()
    hdr = ev.state['hdr'].cpu().numpy()
    assert not hdr[0].any() and hdr[1, ev.hdr_over] == 4 and not hdr[1, ev.hdr_over + 1:].any()      # 2 identities beyond 4, in 2 frames
    for k in big:
        assert bool((big[k][S * ev.state[k].shape[1]:] == 77).all()), f'{k}: written past the stacked tensor'
    assert bool((ws[need:] == 77).all()), 'written past the workspace'
    with pytest.raises(MotOverflow if kind == 'mot' else HotaOverflow, match=r'^stream 1: 4 gt identities'):
        ev.counts()
    with pytest.raises(MotOverflow if kind == 'mot' else HotaOverflow, match='stream 1'):
        ev.stream_counts(1)
    SAME[kind](ev.stream_counts(0), twin(kind, 'B', [calm], 1), RTOL, f'{kind} stream 0 next to an overflowing stream')


# ------------------------------------------------------------------------------------------------ 6. inactive images
@pytest.mark.parametrize('kind', KINDS)
def test_inactive_images_are_not_frames_and_empty_frames_are(kind):
    """Stream 1: two matched frames, a whole batch of images that are no frames, two matched frames: one run, Frag 0 - were the
    inactive images frames, the run would break (hand case `absent`: Frag 1).  Stream 2 is `absent` itself, its empty frame active."""
    on, absent = MC.HAND['absent'][0][0][0], MC.HAND['absent'][0][0]
    busy = seeded(11)
    paused = [on, on, None, None, on, on]
    ev = evaluator(kind, 2, streams=3)
    for k in range(0, 12, 2):
        batch(ev, [busy, paused, absent], k, 2)
    frames = ev.state['hdr'][:, 0].cpu().tolist()
    assert frames == [12, 4, 5], f'frames counted per stream: {frames}'
    ev.end_sequence()
    SAME[kind](ev.stream_counts(0), twin(kind, ('ragged', 0), [busy], 2), RTOL, f'{kind} busy stream')
    SAME[kind](ev.stream_counts(1), twin(kind, 'on x 4', [[on] * 4], 2), RTOL, f'{kind} paused stream')
    SAME[kind](ev.stream_counts(2), twin(kind, 'absent of 2', [absent], 2), RTOL, f'{kind} stream with an empty frame')
    if kind == 'mot':
        assert ev.stream_counts(1)['Frag'].tolist() == [0, 0] and ev.stream_counts(2)['Frag'].tolist() == [1, 0]
        assert ev.stream_counts(1)['TP'].tolist() == [4, 0] and ev.stream_counts(1)['FP'].tolist() == [0, 0]      # no decoy row was read
    # a stream that never had a frame is not open and counts nothing
    ev2 = evaluator(kind, 2, streams=2)
    batch(ev2, [busy[:2], [None, None]], 0, 2)
    assert ev2.open == [True, False]
    ev2.end_sequence()
    assert not any(np.asarray(v).any() for v in ev2.stream_counts(1).values())


# ------------------------------------------------------------------------------------------------ 7. checks before any launch
def test_argument_checks_come_before_any_launch():
    """Every refusal leaves the state as it was: nothing was launched."""
    from tamtr_amd import TamtrHipError, ops
    from tamtr_amd.predict import Predictor
    mot, hota = evaluator('mot', 2, streams=2), evaluator('hota', 2, streams=2)
    seq = seeded(11)
    tracks, tc = pack([t for _, t in seq[:3]], 33)
    for ev in (mot, hota):
        with pytest.raises(ValueError, match='no multiple of streams = 2'):
            ev.update(tracks, tc, [g for g, _ in seq[:3]])
    gt = torch.zeros(4, 33, 7, device='cuda')
    cnt = torch.zeros(4, dtype=torch.int32, device='cuda')
    tracks, tc = pack([t for _, t in seq[:4]], 33)
    with pytest.raises(TamtrHipError, match='no multiple of streams = 3'):
        ops.mot_update(tracks, tc, gt, cnt, mot.state, 2, 32, 256, streams=3)
    with pytest.raises(TamtrHipError, match=r"state\['gstate'\]"):      # state without the leading S
        ops.mot_update(tracks, tc, gt, cnt, mot.stream_state(0), 2, 32, 256, streams=2)
    with pytest.raises(TamtrHipError, match=r"state\['gstate'\]"):      # a stack of another S
        ops.hota_update(tracks, tc, gt, cnt, hota.state, 2, hota.caps, streams=4)
    with pytest.raises(TamtrHipError, match=r"state\['gstate'\]"):
        ops.hota_end_sequence(hota.state, 2, hota.caps, 33, 33, streams=4)
    small = torch.empty(ops.mot_workspace_bytes(33, 33, 2, 32, 256), device='cuda', dtype=torch.uint8)
    with pytest.raises(TamtrHipError, match='workspace must be'):      # a workspace sized for one evaluator
        ops.mot_update(tracks, tc, gt, cnt, mot.state, 2, 32, 256, workspace=small, streams=2)
    with pytest.raises(TamtrHipError, match='active'):
        ops.mot_update(tracks, tc, gt, cnt, mot.state, 2, 32, 256, streams=2, active=cnt[:2])
    with pytest.raises(TamtrHipError, match='gt_used'):
        ops.mot_end_sequence(mot.state, 2, 32, 256, 3, streams=2)
    for ev in (mot, hota):
        with pytest.raises(ValueError, match='stream must be in 0 .. 1'):
            ev.end_sequence([2])
        with pytest.raises(ValueError, match='stream must be in 0 .. 1'):
            ev.stream_counts(True)
    with pytest.raises(ValueError, match='without streams'):
        evaluator('mot', 2).end_sequence([0])
    pred = Predictor.__new__(Predictor)      # no model: only what the checks read
    pred.tracker = None
    with pytest.raises(ValueError, match='streams=3'):      # three sources, evaluators of two streams
        pred.track_streams(['a', 'b', 'c'], gt=[[], [], []], evaluator=[mot, hota])
    torch.cuda.synchronize()
    assert not any(bool(v.any()) for ev in (mot, hota) for v in ev.state.values()) and mot.open == hota.open == [False, False]


# ------------------------------------------------------------------------------------------------ 8. end to end
class EachImageOnce(torch.nn.Module):
    """The detector, run once per distinct image: a later forward of the same pixels, in whatever batch, returns the first one's
    output.  The detector's output is not the same from run to run - on an MI355X two runs of Predictor.predict over these five
    images, same batch size, differed by 2e-5 to 6e-5 px in a box coordinate, as much as runs of different batch sizes - so
    Predictor.track and Predictor.track_streams never score the same rows as it stands: iou_sum came out 3.4710900858117246 against
    3.4710905018971494 (1.2e-7 relative) with every integer count equal.  That belongs to the detector; with one output per image the
    two runs track and score the same rows, and what is compared is the scoring."""

    def __init__(self, model):
        super().__init__()
        self.model, self.seen = model, {}

    def forward(self, x):
        ys = []
        for i in range(x.shape[0]):
            key = x[i].cpu().numpy().tobytes()
            if key not in self.seen:
                y = self.model(x[i:i + 1])
                self.seen[key] = (y[0] if isinstance(y, (list, tuple)) else y).clone()
            ys.append(self.seen[key])
        return torch.cat(ys, 0)


def test_predictor_track_streams_with_gt_and_both_evaluators(tmp_path):
    """Two directories of 3 and 2 images as two streams: every stream's counts equal those of Predictor.track on its directory with
    single evaluators, and the numpy twins on this run's own rows; a stream given gt=None contributes nothing."""
    from test_gpu_predict import CONF, IMGSZ, NC, _images, _model, _text_feats
    from tamtr_amd.engine import hota_evaluate, mot_evaluate
    from tamtr_amd.predict import Predictor
    from tamtr_amd.track import ByteTracker, HotaEvaluator, MotEvaluator
    src = _images(tmp_path)
    names = {i: f'c{i}' for i in range(NC)}
    pred = Predictor(_model().cuda(), names, _text_feats(), imgsz=IMGSZ, conf=CONF, iou=0.7, batch=2, dtype='fp32')
    pred.model = EachImageOnce(pred.model)
    plain = list(pred.predict(str(src)))
    keys = set(pred.speed())
    scores = np.sort(np.concatenate([d.conf.numpy() for d in plain]))
    kw = dict(track_high_thresh=float(scores[len(scores) // 2]) * 1.0001, track_low_thresh=float(scores[len(scores) // 8]) * 1.0001,
              new_track_thresh=float(scores[len(scores) * 3 // 4]) * 1.0001, match_thresh=0.8, track_buffer=30)
    gt_all = _gt_from(plain, np.random.default_rng(8))
    files = sorted(str(p) for p in src.iterdir())
    for s, group in enumerate((files[:3], files[3:])):
        (tmp_path / f'cam{s}').mkdir()
        for f in group:
            os.rename(f, tmp_path / f'cam{s}' / os.path.basename(f))
    sources, gt = [str(tmp_path / 'cam0'), str(tmp_path / 'cam1')], [gt_all[:3], gt_all[3:]]
    caps = dict(gt_capacity=64, track_capacity=4096)
    mot, hota = MotEvaluator('cuda', NC, streams=2, **caps), HotaEvaluator('cuda', NC, streams=2, **caps)
    with pytest.raises(ValueError, match='streams=2'):
        pred.track_streams(sources, gt=gt, evaluator=MotEvaluator('cuda', NC, **caps))
    trk = ByteTracker('cuda', capacity=256, nq=300, streams=2, **kw)
    got = [[], []]
    for s, det in pred.track_streams(sources, tracker=trk, frames_per_stream=2, gt=gt, evaluator=[mot, hota]):
        got[s].append(det)
    assert [len(g) for g in got] == [3, 2] and mot.open == hota.open == [False, False]
    assert pred.speed()['mot'] > 0 and pred.speed()['hota'] > 0 and set(pred.speed()) == keys | {'track', 'mot', 'hota'}
    for s in range(2):
        frames = []
        for d, g in zip(got[s], gt[s]):
            rows = np.zeros((0, 6), np.float32) if d.id is None else np.concatenate([d.boxes.numpy()[:, :4], d.id.numpy()[:, None].astype(np.float32),
                                                                                      d.boxes.numpy()[:, 5:6]], 1)
            frames.append((g, rows))
        want = mot_evaluate([frames], NC)
        print('stream', s, 'counts', {k: int(np.sum(v)) for k, v in want.items()})
        assert want['gt_dets'].sum() > 0 and want['trk_dets'].sum() > 0 and want['TP'].sum() > 0
        MC.same_counts(mot.stream_counts(s), want, RTOL, f'stream {s} against the twin on its own rows')
        HC.same_counts(hota.stream_counts(s), hota_evaluate([frames], NC), RTOL, f'stream {s} against the twin on its own rows')
        one_mot, one_hota = MotEvaluator('cuda', NC, **caps), HotaEvaluator('cuda', NC, **caps)
        alone = list(pred.track(sources[s], tracker=ByteTracker('cuda', capacity=256, nq=300, **kw), gt=gt[s], evaluator=[one_mot, one_hota]))
        assert len(alone) == len(got[s]) and all(torch.equal(a.boxes, d.boxes) for a, d in zip(alone, got[s])), 'the two runs tracked different rows'
        MC.same_counts(mot.stream_counts(s), one_mot.counts(), RTOL, f'stream {s} against Predictor.track')
        HC.same_counts(hota.stream_counts(s), one_hota.counts(), RTOL, f'stream {s} against Predictor.track')
    total = {k: v.copy() for k, v in mot.counts().items()}
    first = {k: v.copy() for k, v in mot.stream_counts(0).items()}
    # stream 1 is tracked but not scored: it contributes nothing, stream 0 counts its sequence once more
    list(pred.track_streams(sources, tracker=trk, frames_per_stream=2, gt=[gt[0], None], evaluator=[mot, hota]))
    MC.same_counts(mot.stream_counts(1), {k: total[k] - first[k] for k in total}, RTOL, 'a stream with gt=None was scored')
    MC.same_counts(mot.stream_counts(0), {k: 2 * first[k] for k in first}, RTOL, 'stream 0, scored twice')
    # without gt and evaluator nothing changes
    list(pred.track_streams(sources, tracker=trk, frames_per_stream=2))
    assert set(pred.speed()) == keys | {'track'}
    MC.same_counts(mot.stream_counts(0), {k: 2 * first[k] for k in first}, RTOL, 'the evaluator was touched by a run that did not name it')


# ------------------------------------------------------------------------------------------------ 9. tools/mot_eval.py --streams
def _same_json(a, b, what):
    if isinstance(a, dict):
        assert isinstance(b, dict) and sorted(a) == sorted(b), what
        for k in a:
            _same_json(a[k], b[k], f'{what}.{k}')
    elif isinstance(a, list):
        assert isinstance(b, list) and len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            _same_json(x, y, f'{what}[{i}]')
    elif isinstance(a, float) or isinstance(b, float):
        assert (a != a and b != b) or abs(a - b) <= RTOL * abs(b), f'{what}: {a!r} vs {b!r}'
    else:
        assert a == b, f'{what}: {a!r} vs {b!r}'


def test_mot_eval_cli_streams_in_a_child_process(tmp_path):
    """Three sequences, two at a time: the last group has one stream.  The numbers are those of the run without --streams and of --host."""
    from test_mot_host import write_case
    write_case(tmp_path, [HC.HAND['alignment'][0][0], MC.HAND['A'][0][0], HC.HAND['id_switch'][0][0]])
    cmd = [sys.executable, os.path.join(ROOT, 'tools', 'mot_eval.py'), '--gt', str(tmp_path / 'gt'), '--results', str(tmp_path / 'res'),
           '--names', 'thing', '--hota', '--batch', '2', '--rows', '16', '--gt-capacity', '32', '--track-capacity', '64']
    runs = {}
    for key, more in (('streams', ['--streams', '2']), ('single', []), ('host', ['--host'])):
        r = subprocess.run(cmd + more, capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
        assert r.returncode == 0, r.stderr[-3000:]
        runs[key] = (json.loads(r.stdout.strip().splitlines()[-1]), r.stdout.strip().splitlines()[:-1])
    res = runs['streams'][0]
    assert res['path'] == 'device' and res['sequences'] == 3 and sorted(res['per_sequence']) == ['seq0', 'seq1', 'seq2']
    HC.check_expected(res['hota']['per_sequence']['seq0'], HC.HAND['alignment'][2], 'seq0')
    MC.check_expected(res['per_sequence']['seq1'], MC.HAND['A'][2], 'seq1')
    HC.check_expected(res['hota']['per_sequence']['seq2'], HC.HAND['id_switch'][2], 'seq2')
    _same_json(res, runs['single'][0], 'against the run without --streams')
    _same_json({k: v for k, v in res.items() if k != 'path'}, {k: v for k, v in runs['host'][0].items() if k != 'path'}, 'against --host')
    first = lambda lines: [ln.split()[0] for ln in lines if ln.split() and ln.split()[0] in ('seq0', 'seq1', 'seq2', 'OVERALL')]     # noqa: E731
    assert first(runs['streams'][1]) == first(runs['single'][1]) and first(runs['streams'][1])[:2] == ['seq0', 'seq0']
