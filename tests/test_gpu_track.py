"""GPU: tamtr_bytetrack_update (csrc/track.hip) against the reference's BYTETracker (tests/golden/track.npz, made by
tests/golden/make_track_golden.py) and against the numpy twin (tests/bytetrack_np.py), and Predictor.track end to end.

Tolerances (derived, not tuned): ids, idx, counts, states and frame numbers are equal; scores and classes are copies, bit-equal; a box
is an fp64 mean cast to fp32, so two correct implementations differ by the final rounding: atol 5e-4 px (4 ulp of fp32 at 2048 px)
with rtol 1e-6; an fp64 mean / covariance entry is within 1e-6 x the largest absolute entry of its array (expected accumulation about
cond(S) * 2^-53 * frames = 2.5e5 * 1.1e-16 * 100 = 3e-9; a rule error moves these by 1e-2 or more)."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
import bytetrack_np as T

pytestmark = pytest.mark.gpu
CFG = dict(track_high_thresh=0.5, track_low_thresh=0.1, new_track_thresh=0.6, track_buffer=30, match_thresh=0.8)
_G = {}


def golden():
    if not _G:
        _G.update(np.load(os.path.join(ROOT, 'tests', 'golden', 'track.npz')))
    return _G


def sequence(name):
    """-> (frames: list of f32 [n, 6], rows: list of (box [k, 4], id [k], idx [k]))."""
    g = golden()
    det = np.concatenate([g[f'{name}_det'], g[f'{name}_cls'].astype(np.float32)[:, None]], 1)
    o = np.concatenate([[0], np.cumsum(g[f'{name}_cnt'])])
    r = np.concatenate([[0], np.cumsum(g[f'{name}_rcnt'])])
    frames = [det[o[i]:o[i + 1]] for i in range(len(o) - 1)]
    rows = [(g[f'{name}_box'][r[i]:r[i + 1]], g[f'{name}_id'][r[i]:r[i + 1]].astype(int), g[f'{name}_idx'][r[i]:r[i + 1]].astype(int))
            for i in range(len(r) - 1)]
    return frames, rows


def tracker(capacity=64, nq=32, **kw):
    from tamtr_amd.track import ByteTracker
    return ByteTracker('cuda', capacity=capacity, nq=nq, **{**CFG, **kw})


def pack(frames, nq):
    out = np.zeros((len(frames), nq, 6), np.float32)
    for i, f in enumerate(frames):
        out[i, :len(f)] = f
    return torch.from_numpy(out).cuda(), torch.tensor([len(f) for f in frames], dtype=torch.int32).cuda()


def run(trk, frames, B, nq):
    """The frames in groups of B (the last group may be shorter) -> per-frame rows f32 [k, 8] on the host."""
    rows = []
    for i in range(0, len(frames), B):
        out, counts = pack(frames[i:i + B], nq)
        tracks, tc = trk.update(out, counts)
        tracks, tc = tracks.cpu().numpy(), tc.cpu().numpy()
        for b in range(len(tc)):
            assert not tracks[b, tc[b]:].any(), 'rows after the count are not zero'
            rows.append(tracks[b, :tc[b]])
    return rows


def same_rows(got, frame, box, ids, idx, what):
    assert sorted(zip(got[:, 4].astype(int), got[:, 7].astype(int))) == sorted(zip(ids, idx)), f'{what}: (id, idx) pairs differ'
    o1, o2 = np.argsort(got[:, 4]), np.argsort(ids)
    np.testing.assert_allclose(got[o1, :4], box[o2], rtol=1e-6, atol=5e-4, err_msg=what)
    k = got[:, 7].astype(int)
    assert np.array_equal(got[:, 5:7], frame[k, 4:6]), f'{what}: score / cls are not those of detection idx'


def close64(a, b, what):
    assert np.abs(a - b).max() <= 1e-6 * np.abs(b).max(), f'{what}: {np.abs(a - b).max()} vs largest entry {np.abs(b).max()}'


def same_final(sd, name):
    """The table's live tracks = the reference's final tracked and lost lists."""
    g = golden()
    meta = sd['meta']
    live = {int(m[T.M_ID]): s for s, m in enumerate(meta) if m[T.M_STATE] != T.FREE}
    fm = g[f'{name}_fin_meta']
    assert sorted(live) == fm[:, 0].tolist()
    for k, row in enumerate(fm):
        s = live[int(row[0])]
        assert meta[s, [T.M_STATE, T.M_ACT, T.M_FRAME, T.M_START, T.M_LEN, T.M_IDX]].tolist() == row[1:].tolist(), f'{name} id {row[0]}'
        assert np.array_equal(sd['sc'][s], g[f'{name}_fin_sc'][k])
        close64(sd['mean'][s], g[f'{name}_fin_mean'][k], f'{name} id {row[0]} mean')
        close64(sd['cov'][s], g[f'{name}_fin_cov'][k], f'{name} id {row[0]} cov')


def same_table(sd, twin, what):
    """Kernel and twin keep the same table: slots, ids, counters equal; filters within the fp64 bound."""
    ts = twin.state
    assert np.array_equal(sd['hdr'], ts['hdr']), f'{what}: hdr {sd["hdr"]} vs {ts["hdr"]}'
    used = ts['meta'][:, T.M_STATE] != T.FREE
    assert np.array_equal(sd['meta'][:, T.M_STATE], ts['meta'][:, T.M_STATE]), f'{what}: slot states differ'
    assert np.array_equal(sd['meta'][used], ts['meta'][used]) and np.array_equal(sd['sc'][used], ts['sc'][used]), what
    for s in np.flatnonzero(used):
        close64(sd['mean'][s], ts['mean'][s], f'{what} slot {s} mean')
        close64(sd['cov'][s], ts['cov'][s], f'{what} slot {s} cov')


def against_twin(frames, B, nq, capacity=64, what='', **kw):
    trk = tracker(capacity, nq, **kw)
    twin = T.ByteTrackNp(capacity=capacity, want_margin=True, **{**CFG, **kw})
    got = run(trk, frames, B, nq)
    for f, fr in enumerate(frames):
        want = twin.update(fr)
        same_rows(got[f], fr, want[:, :4], want[:, 4].astype(int), want[:, 7].astype(int), f'{what} frame {f}')
    same_table(trk.state_dict(), twin, what)
    return trk, twin


# ------------------------------------------------------------------------------------------------ the reference's sequences
_B1 = {}


def b1(name, nq):
    if name not in _B1:
        trk = tracker(64, nq)
        _B1[name] = (run(trk, sequence(name)[0], 1, nq), trk.state_dict())
    return _B1[name]


@pytest.mark.parametrize('name,nq,B', [('crowd', 300, 1), ('crowd', 300, 4), ('twins', 32, 1), ('twins', 32, 3)])
def test_fixture_sequence_reproduces_the_reference(name, nq, B):
    frames, want = sequence(name)
    got, sd = b1(name, nq)
    if B > 1:   # grouped launches (the last group ends mid-group): identical to one frame per launch, bit for bit
        assert len(frames) % B, 'the last group must be a partial one'
        trk = tracker(64, nq)
        grouped = run(trk, frames, B, nq)
        assert all(np.array_equal(a, b) for a, b in zip(grouped, got)) and len(grouped) == len(got)
        sdB = trk.state_dict()
        live = sd['meta'][:, T.M_STATE] != T.FREE
        assert all(np.array_equal(sdB[k][live] if k != 'hdr' else sdB[k], sd[k][live] if k != 'hdr' else sd[k]) for k in sd)
        got, sd = grouped, sdB
    assert sum(len(r) for r in got) > 100
    for f, (box, ids, idx) in enumerate(want):
        same_rows(got[f], frames[f], box, ids, idx, f'{name} frame {f}')
    same_final(sd, name)


def test_staged_state_and_resume():
    g = golden()
    frames, want = sequence('staged')
    staged = {k: g[f'staged_{k}'] for k in ('mean', 'cov', 'meta', 'sc', 'hdr')}
    trk = tracker(int(g['capacity']), 32)
    trk.load_state_dict(staged)
    got = run(trk, frames, 2, 32)
    for f, (box, ids, idx) in enumerate(want):
        same_rows(got[f], frames[f], box, ids, idx, f'staged frame {f}')
    same_final(trk.state_dict(), 'staged')
    assert 1 not in [int(i) for r in got for i in r[:, 4]], 'the tracked side of the staged duplicate pair was not dropped'
    # state_dict() -> load_state_dict() -> continue = an uninterrupted run
    a = tracker(64, 32)
    a.load_state_dict(staged)
    head = run(a, frames[:3], 1, 32)
    b = tracker(64, 32)
    b.load_state_dict(a.state_dict())
    tail = run(b, frames[3:], 1, 32)
    whole = tracker(64, 32)
    whole.load_state_dict(staged)
    ref = run(whole, frames, 1, 32)
    assert all(np.array_equal(x, y) for x, y in zip(head + tail, ref))
    sa, sb = b.state_dict(), whole.state_dict()
    assert all(np.array_equal(sa[k], sb[k]) for k in sa)


# ------------------------------------------------------------------------------------------------ edge cases
def test_empty_frames_do_not_reach_the_tracker():
    scene = T.make_scene(101, n_obj=5, frames=6, fp_every=0, p_low=0.0)
    empty = np.zeros((0, 6), np.float32)
    trk = tracker()
    out, counts = pack([empty] * 3, 32)      # a batch whose every frame is empty
    tracks, tc = trk.update(out, counts)
    assert not tracks.cpu().numpy().any() and not tc.cpu().numpy().any()
    sd = trk.state_dict()
    assert sd['hdr'].tolist() == [0, 1, 0, 0, 0, 0, 0, 0] and not sd['meta'].any()
    against_twin([empty] + scene[:3] + [empty] + scene[3:], 4, 32, what='first frame empty')


def test_one_detection():
    d = np.array([[10, 20, 50, 100, 0.9, 3]], np.float32)
    trk, twin = against_twin([d, d + np.float32([1, 1, 1, 1, 0, 0]), d + np.float32([2, 2, 2, 2, -0.6, 0])], 1, 32, what='one detection')
    assert trk.state_dict()['hdr'][:3].tolist() == [3, 2, 1]


def test_all_scores_below_track_low_thresh():
    scene = T.make_scene(102, n_obj=6, frames=3, fp_every=0)
    for f in scene:
        f[:, 4] = 0.05
    trk, _ = against_twin(scene, 3, 32, what='low scores')
    assert trk.state_dict()['hdr'][:3].tolist() == [3, 1, 0]      # the frames count, nothing is tracked


def test_counts_equal_to_nq():
    rng = np.random.default_rng(7)
    nq = 32
    gx, gy = np.meshgrid(np.arange(8) * 120.0, np.arange(4) * 150.0)
    base = np.stack([gx.ravel() + 10, gy.ravel() + 10, gx.ravel() + 90, gy.ravel() + 120, rng.uniform(0.65, 0.95, nq), rng.integers(0, 3, nq)], 1)
    frames = [(base + np.concatenate([rng.normal(0, 0.5, (nq, 4)), np.zeros((nq, 2))], 1)).astype(np.float32)[rng.permutation(nq)] for _ in range(3)]
    trk, _ = against_twin(frames, 3, nq, what='full frame')
    assert trk.state_dict()['hdr'][2] == nq


def test_reset():
    scene = T.make_scene(103, n_obj=5, frames=4, fp_every=0, p_low=0.0)
    trk = tracker()
    run(trk, scene, 2, 32)
    assert trk.state_dict()['hdr'][1] > 1
    trk.reset()
    again = run(trk, scene, 2, 32)
    fresh = run(tracker(), scene, 2, 32)
    assert all(np.array_equal(a, b) for a, b in zip(again, fresh))
    assert min(int(r[:, 4].min()) for r in again if len(r)) == 1


def test_overflow_is_counted_and_nothing_is_written_past_the_table():
    """capacity 8, 12 objects: a bounds check by construction - the four tracks that find no slot are counted, the host raises, and
    the memory after every table and after the workspace keeps its canary."""
    from tamtr_amd import ops
    from tamtr_amd.track import TrackerOverflow
    cap, nq, pad = 8, 32, 64
    rng = np.random.default_rng(9)
    d = np.stack([np.arange(12) * 100.0, np.full(12, 50.0), np.arange(12) * 100.0 + 60, np.full(12, 150.0), rng.uniform(0.7, 0.9, 12),
                  np.zeros(12)], 1).astype(np.float32)
    big, state = {}, {}
    for k, dt, tail in ops.TRACK_STATE_SPEC:
        big[k] = torch.full((cap + pad,) + tail, 77, dtype=dt, device='cuda')
        big[k][:cap] = 0
        state[k] = big[k][:cap]
    big['hdr'] = torch.full((8 + pad,), 77, dtype=torch.int32, device='cuda')
    big['hdr'][:8] = torch.tensor([0, 1, 0, 0, 0, 0, 0, 0], dtype=torch.int32)
    state['hdr'] = big['hdr'][:8]
    need = ops.bytetrack_workspace_bytes(cap, nq)
    ws = torch.full((need + 4096,), 77, dtype=torch.uint8, device='cuda')
    out, counts = pack([d, d], nq)
    tracks, tc = ops.bytetrack_update(out, counts, state, cap, workspace=ws[:need], **{k: v for k, v in CFG.items() if k != 'track_buffer'})
    torch.cuda.synchronize()
    hdr = state['hdr'].cpu().numpy()
    assert hdr[T.H_OVER] == 8 and hdr[T.H_LIVE] == 8 and hdr[T.H_NEXT] == 9      # 4 refused in each of the two frames
    assert tc.tolist() == [8, 8]
    for k in big:
        tail = big[k][(8 if k == 'hdr' else cap):]
        assert bool((tail == 77).all()), f'{k}: written past the table'
    assert bool((ws[need:] == 77).all()), 'written past the workspace'
    with pytest.raises(TrackerOverflow):
        tracker(cap, nq).check_overflow(hdr[T.H_OVER])
    twin = T.ByteTrackNp(capacity=cap, **CFG)
    twin.update(d), twin.update(d)
    assert np.array_equal(twin.state['hdr'], hdr)


# ------------------------------------------------------------------------------------------------ fresh sequences
@pytest.mark.parametrize('seed,B', [(201, 1), (203, 4), (206, 7)])
def test_fresh_sequence_equals_the_twin(seed, B):
    """Seeds that are not in the fixture.  Precondition (checked on the CPU when the seeds were chosen, and again here): every
    assignment's optimum beats the runner-up by more than 1e-6 and no score or cost is within 1e-4 of a threshold."""
    scene = T.make_scene(seed, n_obj=12, frames=40, fp_every=3, gaps=[(0, 5, 3), (1, 8, 25), (2, 12, 6)])
    trk, twin = against_twin(scene, B, 64, what=f'seed {seed}', track_buffer=10)
    assert twin.margin > 1e-6 and twin.thr_margin > 1e-4, (twin.margin, twin.thr_margin)
    ev = twin.events
    assert ev['match2'] and ev['refind'] and ev['aged_out'] and ev['unconfirmed_removed'] and ev['new_refused'], ev


# ------------------------------------------------------------------------------------------------ end to end
def test_predictor_track_end_to_end(tmp_path):
    from test_gpu_predict import CONF, IMGSZ, NC, _images, _model, _text_feats
    from tamtr_amd.predict import Predictor
    src = _images(tmp_path)
    names = {i: f'c{i}' for i in range(NC)}
    pred = Predictor(_model().cuda(), names, _text_feats(), imgsz=IMGSZ, conf=CONF, iou=0.7, batch=2, dtype='fp32')
    plain = list(pred.predict(str(src)))
    assert all(d.id is None for d in plain) and sum(len(d) for d in plain) > 0
    # the seeded weights score below 5e-4: thresholds that split this run's own scores into high, low and ignored
    scores = np.sort(np.concatenate([d.conf.numpy() for d in plain]))
    kw = dict(track_high_thresh=float(scores[len(scores) // 2]) * 1.0001, track_low_thresh=float(scores[len(scores) // 8]) * 1.0001,
              new_track_thresh=float(scores[len(scores) * 3 // 4]) * 1.0001, match_thresh=0.8, track_buffer=30)
    trk = tracker(256, 300, **kw)
    twin = T.ByteTrackNp(capacity=256, want_margin=True, **kw)
    batches, run_batch = [], pred.run_batch

    def spy(ims, tracker=None):      # this run's own detections, as they left the device
        batches.append(run_batch(ims, tracker))
        return batches[-1]

    pred.run_batch = spy
    got = list(pred.track(str(src), tracker=trk))
    assert [d.path for d in got] == [d.path for d in plain]
    dets = [o[:int(c)].numpy() for res in batches for o, c in zip(res[0], res[2])]
    assert len(dets) == len(got)
    n_ids = 0
    for f, (det, raw) in enumerate(zip(got, dets)):
        want = twin.update(raw)
        if len(want) == 0:
            assert det.id is None and np.array_equal(det.boxes.numpy(), raw), f'frame {f}'
            continue
        assert det.id.dtype == torch.int64
        order, worder = np.argsort(det.id.numpy()), np.argsort(want[:, 4])
        assert np.array_equal(det.id.numpy()[order], want[worder, 4].astype(np.int64)), f'frame {f}: ids'
        idx = want[worder, 7].astype(int)
        assert np.array_equal(det.boxes.numpy()[order, 4:6], raw[idx, 4:6]), f'frame {f}: score / cls of detection idx'
        np.testing.assert_allclose(det.boxes.numpy()[order, :4], want[worder, :4], rtol=1e-6, atol=5e-4)
        n_ids += len(want)
        det.save_txt(tmp_path / 'labels' / f'{f}.txt', save_conf=True)
        assert np.array_equal(np.loadtxt(tmp_path / 'labels' / f'{f}.txt', ndmin=2)[:, 6], det.id.numpy())
    print('twin margin', twin.margin, 'threshold margin', twin.thr_margin, 'events', twin.events)
    assert twin.margin > 1e-6, 'precondition: this run has an assignment that is not unique'
    assert n_ids > 0 and pred.speed()['track'] > 0


def test_track_cli_runs_in_a_child_process(tmp_path):
    """tools/track.py on two sequence directories: labels with ids, one MOT file per sequence, ids restart with every sequence."""
    import json
    import subprocess
    from PIL import Image
    from test_gpu_predict import CONF, IMGSZ, NC, _model, _text_feats
    rng = np.random.default_rng(4)
    for seq, n in (('uav1', 3), ('uav2', 2)):
        (tmp_path / 'sequences' / seq).mkdir(parents=True)
        for i in range(n):
            Image.fromarray(rng.integers(0, 256, (96, 128, 3), dtype=np.uint8)).save(tmp_path / 'sequences' / seq / f'{i + 1:07d}.png')
    sd = _model().state_dict()
    torch.save({'model': sd, 'ema': sd}, tmp_path / 'best.pt')
    names = [f'c{i}' for i in range(NC)]
    np.savez(tmp_path / 'feats.npz', texts=np.array(names), feats=_text_feats().numpy())
    # the seeded weights score below 5e-4: thresholds in that range, in the reference's yaml keys
    (tmp_path / 'bytetrack.yaml').write_text('tracker_type: bytetrack\ntrack_high_thresh: 0.00004\ntrack_low_thresh: 0.00002\n'
                                             'new_track_thresh: 0.00005\ntrack_buffer: 30\nmatch_thresh: 0.8\n')
    cmd = [sys.executable, os.path.join(ROOT, 'tools', 'track.py'), '--weights', str(tmp_path / 'best.pt'), '--text-feats', str(tmp_path / 'feats.npz'),
           '--names', ','.join(names), '--source', str(tmp_path / 'sequences'), '--tracker', str(tmp_path / 'bytetrack.yaml'), '--imgsz', str(IMGSZ),
           '--batch', '2', '--conf', str(CONF), '--save-txt', '--save-conf', '--save-mot', '--save', '--project', str(tmp_path / 'runs'),
           '--name', 'TAMTR', '--dtype', 'fp32', '--capacity', '512']
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    out = tmp_path / 'runs' / 'TAMTR'
    assert res['sequences'] == 2 and res['images'] == 5 and res['track_rows'] > 0 and res['save_dir'] == str(out)
    assert set(res['ms_per_image']) == {'load', 'forward', 'postprocess', 'track', 'd2h'}
    total = 0
    for seq in ('uav1', 'uav2'):
        mot = [ln.split(',') for ln in (out / f'{seq}.txt').read_text().splitlines()]
        assert mot and all(len(ln) == 10 and ln[8:] == ['-1', '-1'] for ln in mot)
        assert mot[0][0] == '1' and min(int(ln[1]) for ln in mot) == 1        # frames are 1-based; every sequence starts at id 1
        first = np.loadtxt(out / 'labels' / seq / '0000001.txt', ndmin=2)
        assert first.shape[1] == 7 and sorted(first[:, 6].astype(int)) == sorted(int(ln[1]) for ln in mot if ln[0] == '1')
        assert (out / seq / '0000001.png').exists()
        total += len(mot)
    assert total == res['track_rows']
