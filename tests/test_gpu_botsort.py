"""GPU: tamtr_botsort_update (csrc/track.hip, the KF_XYWH form of the tracker kernel) against the reference's BOTSORT
(tests/golden/botsort.npz, made by tests/golden/make_botsort_golden.py) and against the numpy twin (tests/botsort_np.py).

Tolerances are test_gpu_track.py's (derived there): ids, idx, counts, states and frame numbers are equal; scores and classes are
copies, bit-equal; a box is an fp64 mean cast to fp32: atol 5e-4 px with rtol 1e-6; an fp64 mean / covariance entry is within 1e-6 x
the largest absolute entry of its array.  The warp adds two fp64 products and a sum per entry and frame, well inside that."""
import numpy as np
import pytest
import torch

import bytetrack_np as T
import botsort_np as BS
from test_botsort_host import CFG, G, sequence
from test_gpu_track import close64, pack, same_rows

pytestmark = pytest.mark.gpu


def tracker(capacity=64, nq=32, **kw):
    from tamtr_amd.track import BotSort
    return BotSort('cuda', capacity=capacity, nq=nq, **{**CFG, **kw})


def run(trk, frames, warps, B, nq, identity=False):
    """The frames in groups of B (the last group may be shorter) -> per-frame rows f32 [k, 8] on the host.  warps: f64 [F, 2, 3] or
    None; identity=True hands explicit identity warps instead."""
    rows = []
    for i in range(0, len(frames), B):
        out, counts = pack(frames[i:i + B], nq)
        w = None if warps is None else warps[i:i + B]
        if identity:
            w = np.tile(np.eye(2, 3), (len(counts), 1, 1))
        if B > 1 and w is not None:      # a device tensor is taken as it is, a host array goes up in one copy
            w = torch.from_numpy(np.ascontiguousarray(w)).cuda()
        tracks, tc = trk.update(out, counts, warps=w)
        tracks, tc = tracks.cpu().numpy(), tc.cpu().numpy()
        for b in range(len(tc)):
            assert not tracks[b, tc[b]:].any(), 'rows after the count are not zero'
            rows.append(tracks[b, :tc[b]])
    return rows


def same_final(sd, name):
    """The table's live tracks = the reference's final tracked and lost lists."""
    meta = sd['meta']
    live = {int(m[T.M_ID]): s for s, m in enumerate(meta) if m[T.M_STATE] != T.FREE}
    fm = G[f'{name}_fin_meta']
    assert sorted(live) == fm[:, 0].tolist()
    for k, row in enumerate(fm):
        s = live[int(row[0])]
        assert meta[s, [T.M_STATE, T.M_ACT, T.M_FRAME, T.M_START, T.M_LEN, T.M_IDX]].tolist() == row[1:].tolist(), f'{name} id {row[0]}'
        assert np.array_equal(sd['sc'][s], G[f'{name}_fin_sc'][k])
        close64(sd['mean'][s], G[f'{name}_fin_mean'][k], f'{name} id {row[0]} mean')
        close64(sd['cov'][s], G[f'{name}_fin_cov'][k], f'{name} id {row[0]} cov')


def same_table(sd, twin, what):
    ts = twin.state
    assert np.array_equal(sd['hdr'], ts['hdr']), f'{what}: hdr {sd["hdr"]} vs {ts["hdr"]}'
    used = ts['meta'][:, T.M_STATE] != T.FREE
    assert np.array_equal(sd['meta'][:, T.M_STATE], ts['meta'][:, T.M_STATE]), f'{what}: slot states differ'
    assert np.array_equal(sd['meta'][used], ts['meta'][used]) and np.array_equal(sd['sc'][used], ts['sc'][used]), what
    for s in np.flatnonzero(used):
        close64(sd['mean'][s], ts['mean'][s], f'{what} slot {s} mean')
        close64(sd['cov'][s], ts['cov'][s], f'{what} slot {s} cov')


# ------------------------------------------------------------------------------------------------ the reference's sequences
_B1 = {}


def b1(name, nq):
    if name not in _B1:
        trk = tracker(64, nq)
        frames, _, warps = sequence(name)
        _B1[name] = (run(trk, frames, warps, 1, nq), trk.state_dict())
    return _B1[name]


@pytest.mark.parametrize('name,nq,B', [('pan', 300, 1), ('pan', 300, 4), ('aniso', 32, 1), ('aniso', 32, 3), ('gaps', 32, 1), ('gaps', 32, 3)])
def test_fixture_sequence_reproduces_the_reference(name, nq, B):
    frames, want, warps = sequence(name)
    got, sd = b1(name, nq)
    if B > 1:   # grouped launches (the last group ends mid-group): identical to one frame per launch, bit for bit
        assert len(frames) % B, 'the last group must be a partial one'
        trk = tracker(64, nq)
        grouped = run(trk, frames, warps, B, nq)
        assert all(np.array_equal(a, b) for a, b in zip(grouped, got)) and len(grouped) == len(got)
        sdB = trk.state_dict()
        live = sd['meta'][:, T.M_STATE] != T.FREE
        assert all(np.array_equal(sdB[k][live] if k != 'hdr' else sdB[k], sd[k][live] if k != 'hdr' else sd[k]) for k in sd)
        assert tuple(trk.last_warps.shape) == (len(frames) % B, 2, 3) and trk.last_warps.is_cuda
        got, sd = grouped, sdB
    assert sum(len(r) for r in got) > 50
    assert [len(r) for r in got] == G[f'{name}_rcnt'].tolist()
    for f, (box, ids, idx) in enumerate(want):
        same_rows(got[f], frames[f], box, ids, idx, f'{name} frame {f}')
    same_final(sd, name)


def test_explicit_identity_warps_equal_none():
    frames, _, _ = sequence('gaps')
    a, b = tracker(), tracker()
    ra, rb = run(a, frames, None, 3, 32), run(b, frames, None, 3, 32, identity=True)
    assert all(np.array_equal(x, y) for x, y in zip(ra, rb))
    sa, sb = a.state_dict(), b.state_dict()
    assert all(np.array_equal(sa[k], sb[k]) for k in sa)
    assert a.last_warps is None and b.last_warps is not None
    assert sum(len(r) for r in ra) > 50


def test_warps_matter_and_the_jump_is_survived():
    """The pan sequence up to its jump: with the camera's warps the ids the reference keeps across the jump are kept, with identity
    warps most of them are lost there."""
    frames, want, warps = sequence('pan')
    J = int(G['jump'])
    good = run(tracker(64, 300), frames[:J + 1], warps[:J + 1], 4, 300)
    blind = run(tracker(64, 300), frames[:J + 1], None, 4, 300)
    ids = lambda r: set(r[:, 4].astype(int))      # noqa: E731
    kept, bkept = ids(good[J - 1]) & ids(good[J]), ids(blind[J - 1]) & ids(blind[J])
    assert kept == set(want[J - 1][1]) & set(want[J][1]) and len(kept) >= len(want[J - 1][1]) - 1
    assert len(bkept) < len(kept) // 2, (len(kept), len(bkept))


def test_bytetrack_is_unchanged():
    """ByteTracker on its own fixture through the kernel that now has two forms (the full set stays in test_gpu_track.py)."""
    import test_gpu_track as A
    frames, want = A.sequence('twins')
    trk = A.tracker(64, 32)
    got = A.run(trk, frames, 3, 32)
    for f, (box, ids, idx) in enumerate(want):
        same_rows(got[f], frames[f], box, ids, idx, f'twins frame {f}')
    A.same_final(trk.state_dict(), 'twins')


def test_resume_in_the_middle_of_the_pan():
    frames, _, warps = sequence('pan')
    cut, end = 43, 50      # the cut lies before the jump, the tail crosses it
    a = tracker(64, 300)
    head = run(a, frames[:cut], warps[:cut], 4, 300)
    b = tracker(64, 300)
    b.load_state_dict(a.state_dict())
    tail = run(b, frames[cut:end], warps[cut:end], 4, 300)
    whole = tracker(64, 300)
    ref = run(whole, frames[:cut], warps[:cut], 4, 300) + run(whole, frames[cut:end], warps[cut:end], 4, 300)
    assert all(np.array_equal(x, y) for x, y in zip(head + tail, ref)) and len(ref) == end
    sa, sb = b.state_dict(), whole.state_dict()
    assert all(np.array_equal(sa[k], sb[k]) for k in sa)


# ------------------------------------------------------------------------------------------------ fresh sequences, bookkeeping
@pytest.mark.parametrize('seed,B', [(301, 1), (303, 5)])
def test_fresh_sequence_equals_the_twin(seed, B):
    """Seeds that are not in the fixture, under a camera with non-similarity warps.  Precondition (checked on the CPU when the
    seeds were chosen, and again here): every assignment's optimum beats the runner-up by more than 1e-6 and no score or cost is
    within 1e-4 of a threshold."""
    scene = T.make_scene(seed, n_obj=10, frames=32, fp_every=3, gaps=[(0, 5, 3), (1, 8, 20), (2, 12, 6)], empty=(9,))
    warps = BS.camera_path(seed, len(scene), pan=(4.0, -2.0), aniso=0.003, jumps={20: (30.0, -20.0)})
    frames = BS.through_camera(scene, warps)
    trk = tracker(64, 64, track_buffer=10)
    twin = BS.BotSortNp(capacity=64, want_margin=True, **{**CFG, 'track_buffer': 10})
    got = run(trk, frames, warps, B, 64)
    for f, fr in enumerate(frames):
        want = twin.update(fr, warps[f])
        same_rows(got[f], fr, want[:, :4], want[:, 4].astype(int), want[:, 7].astype(int), f'seed {seed} frame {f}')
    same_table(trk.state_dict(), twin, f'seed {seed}')
    assert twin.margin > 1e-6 and twin.thr_margin > 1e-4, (twin.margin, twin.thr_margin)
    ev = twin.events
    assert ev['match2'] and ev['refind'] and ev['aged_out'] and ev['unconfirmed_removed'] and ev['warp_unconfirmed'] and ev['lost_zeroed_vw_vh'], ev


def test_overflow_and_reset_at_capacity_4():
    from tamtr_amd.track import TrackerOverflow
    rng = np.random.default_rng(9)
    d = np.stack([np.arange(7) * 100.0, np.full(7, 50.0), np.arange(7) * 100.0 + 60, np.full(7, 150.0), rng.uniform(0.7, 0.9, 7),
                  np.zeros(7)], 1).astype(np.float32)
    w = np.array([[[1.0, 0.0, 2.0], [0.0, 1.0, -1.0]]] * 2)
    trk = tracker(4, 32)
    twin = BS.BotSortNp(capacity=4, **CFG)
    got = run(trk, [d, d + np.float32([2, -1, 2, -1, 0, 0])], w, 2, 32)
    want = [twin.update(d, w[0]), twin.update(d + np.float32([2, -1, 2, -1, 0, 0]), w[1])]
    sd = trk.state_dict()
    assert sd['hdr'][:4].tolist() == [2, 5, 4, 6] and np.array_equal(sd['hdr'], twin.state['hdr'])      # 3 refused in each of the two frames
    assert [len(r) for r in got] == [4, 4] == [len(r) for r in want]
    with pytest.raises(TrackerOverflow):
        trk.check_overflow(sd['hdr'][T.H_OVER])
    trk.reset()
    again = run(trk, [d[:3], d[:3]], w, 2, 32)
    fresh = run(tracker(4, 32), [d[:3], d[:3]], w, 2, 32)
    assert all(np.array_equal(a, b) for a, b in zip(again, fresh)) and sorted(again[1][:, 4].astype(int)) == [1, 2, 3]
    assert trk.state_dict()['hdr'][:4].tolist() == [2, 4, 3, 0]


# ------------------------------------------------------------------------------------------------ end to end
def test_predictor_track_with_a_botsort_yaml(tmp_path):
    """Predictor.track(tracker='botsort.yaml') builds a BotSort (track.tracker_from_yaml); with gmc_method none in the yaml it runs
    identity warps, and this run's own detections through the twin give the same ids and boxes.  The helper is test_gpu_track.py's.
    (The run with estimated warps, on drawn frames, is tests/test_gpu_gmc.py's.)"""
    from test_gpu_predict import CONF, IMGSZ, NC, _images, _model, _text_feats
    from tamtr_amd.predict import Predictor
    from tamtr_amd.track import BotSort
    src = _images(tmp_path)
    names = {i: f'c{i}' for i in range(NC)}
    pred = Predictor(_model().cuda(), names, _text_feats(), imgsz=IMGSZ, conf=CONF, iou=0.7, batch=2, dtype='fp32')
    plain = list(pred.predict(str(src)))
    # the seeded weights score below 5e-4: thresholds that split this run's own scores into high, low and ignored
    scores = np.sort(np.concatenate([d.conf.numpy() for d in plain]))
    kw = dict(track_high_thresh=float(scores[len(scores) // 2]) * 1.0001, track_low_thresh=float(scores[len(scores) // 8]) * 1.0001,
              new_track_thresh=float(scores[len(scores) * 3 // 4]) * 1.0001, match_thresh=0.8, track_buffer=30)
    kw = {k: float(f'{v:.10e}') for k, v in kw.items()}      # what the yaml below carries
    y = tmp_path / 'botsort.yaml'
    y.write_text('tracker_type: botsort\n' + ''.join(f'{k}: {v:.10e}\n' for k, v in kw.items()) +
                 'gmc_method: none\nproximity_thresh: 0.5\nappearance_thresh: 0.25\nwith_reid: False\n')
    twin = BS.BotSortNp(capacity=1024, want_margin=True, **kw)
    batches, run_batch = [], pred.run_batch

    def spy(ims, tracker=None):      # this run's own detections, as they left the device
        batches.append(run_batch(ims, tracker))
        return batches[-1]

    pred.run_batch = spy
    got = list(pred.track(str(src), tracker=str(y)))
    assert type(pred.tracker) is BotSort and pred.tracker.gmc_method == 'none'
    assert [d.path for d in got] == [d.path for d in plain]
    dets = [o[:int(c)].numpy() for res in batches for o, c in zip(res[0], res[2])]
    n_ids = 0
    for f, (det, raw) in enumerate(zip(got, dets)):
        want = twin.update(raw)
        if len(want) == 0:
            assert det.id is None and np.array_equal(det.boxes.numpy(), raw), f'frame {f}'
            continue
        order, worder = np.argsort(det.id.numpy()), np.argsort(want[:, 4])
        assert np.array_equal(det.id.numpy()[order], want[worder, 4].astype(np.int64)), f'frame {f}: ids'
        assert np.array_equal(det.boxes.numpy()[order, 4:6], raw[want[worder, 7].astype(int), 4:6]), f'frame {f}: score / cls of detection idx'
        np.testing.assert_allclose(det.boxes.numpy()[order, :4], want[worder, :4], rtol=1e-6, atol=5e-4)
        n_ids += len(want)
    assert twin.margin > 1e-6, 'precondition: this run has an assignment that is not unique'
    assert n_ids > 0 and pred.speed()['track'] > 0


def test_track_cli_with_the_references_botsort_yaml(tmp_path):
    """tools/track.py --tracker botsort.yaml in a child process, with the yaml as the reference ships it (gmc_method: sparseOptFlow,
    estimated on the device from the frames); --gmc none overrides it, which tests/test_botsort_host.py checks on tracker_from_yaml."""
    import json
    import os
    import subprocess
    import sys
    from PIL import Image
    from conftest import ROOT
    from test_gpu_predict import CONF, IMGSZ, NC, _model, _text_feats
    rng = np.random.default_rng(4)
    (tmp_path / 'uav1').mkdir()
    for i in range(3):
        Image.fromarray(rng.integers(0, 256, (96, 128, 3), dtype=np.uint8)).save(tmp_path / 'uav1' / f'{i + 1:07d}.png')
    sd = _model().state_dict()
    torch.save({'model': sd, 'ema': sd}, tmp_path / 'best.pt')
    names = [f'c{i}' for i in range(NC)]
    np.savez(tmp_path / 'feats.npz', texts=np.array(names), feats=_text_feats().numpy())
    (tmp_path / 'botsort.yaml').write_text('tracker_type: botsort\ntrack_high_thresh: 0.00004\ntrack_low_thresh: 0.00002\nnew_track_thresh: 0.00005\n'
                                           'track_buffer: 30\nmatch_thresh: 0.8\ngmc_method: sparseOptFlow\nproximity_thresh: 0.5\n'
                                           'appearance_thresh: 0.25\nwith_reid: False\n')
    cmd = [sys.executable, os.path.join(ROOT, 'tools', 'track.py'), '--weights', str(tmp_path / 'best.pt'), '--text-feats', str(tmp_path / 'feats.npz'),
           '--names', ','.join(names), '--source', str(tmp_path / 'uav1'), '--tracker', str(tmp_path / 'botsort.yaml'), '--imgsz', str(IMGSZ),
           '--batch', '2', '--conf', str(CONF), '--save-mot', '--project', str(tmp_path / 'runs'), '--name', 'TAMTR', '--dtype', 'fp32',
           '--capacity', '512']
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res['sequences'] == 1 and res['images'] == 3 and res['track_rows'] > 0
    mot = [ln.split(',') for ln in (tmp_path / 'runs' / 'TAMTR' / 'uav1.txt').read_text().splitlines()]
    assert len(mot) == res['track_rows'] and mot[0][0] == '1' and min(int(ln[1]) for ln in mot) == 1
