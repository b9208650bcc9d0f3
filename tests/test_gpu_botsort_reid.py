"""GPU: tamtr_reid_rows and tamtr_botsort_reid_update (csrc/track.hip, the ReID instantiation of the tracker kernel) against the
reference's BOTSORT run with a stub encoder (tests/golden/botsort_reid.npz, made by tests/golden/make_botsort_reid_golden.py) and
against the numpy twin (tests/botsort_reid_np.py), then through track.BotSort, Predictor.track and tools/track.py.

Tolerances: ids, idx, counts, states and frame numbers are equal; boxes and filter states as in test_gpu_botsort.py.  A feature row is
fp32 arithmetic whose sums run in another order than numpy's (csrc/track.hip writes the order down): it is held to FOUR TIMES the
distance between the numpy statement's own fp32 and fp64 runs on the same input, measured at run time - the rule of test_gpu_gmc.py.
The precondition of every comparison of ids with the twin is the fixture generator's: with delta the largest difference of a cost
entry between the twin's fp32 and fp64 runs, every assignment's optimum beats its runner-up by more than 100 * delta * (most matches
in one assignment), and no score, distance or cost lies within 1e-4 of its threshold."""
import numpy as np
import pytest
import torch

import bytetrack_np as T
import botsort_np as BS
import botsort_reid_np as R
from test_botsort_host import CFG
from test_botsort_reid_host import D, G, REID, ids_of_objects, sequence, twin, twin_run
from test_gpu_botsort import same_table
from test_gpu_botsort import tracker as plain_tracker
from test_gpu_track import close64, pack, same_rows

pytestmark = pytest.mark.gpu


def tracker(capacity=64, nq=32, dim=D, **kw):
    from tamtr_amd.track import BotSort
    return BotSort('cuda', capacity=capacity, nq=nq, with_reid=True, reid_dim=dim, gmc_method='none', **{**CFG, **REID, **kw})


def pack_feats(feats, nq, dim):
    out = np.zeros((len(feats), nq, dim), np.float32)
    for i, f in enumerate(feats):
        out[i, :len(f)] = f
    return torch.from_numpy(out).cuda()


def run(trk, frames, warps, feats, B, nq, reid=True):
    """The frames in groups of B (the last group may be shorter) -> per-frame rows f32 [k, 8] on the host."""
    rows = []
    dim = feats[0].shape[1]
    for i in range(0, len(frames), B):
        out, counts = pack(frames[i:i + B], nq)
        w = torch.from_numpy(np.ascontiguousarray(warps[i:i + B])).cuda()
        kw = dict(feats=pack_feats(feats[i:i + B], nq, dim)) if reid else {}
        tracks, tc = trk.update(out, counts, warps=w, **kw)
        tracks, tc = tracks.cpu().numpy(), tc.cpu().numpy()
        for b in range(len(tc)):
            assert not tracks[b, tc[b]:].any(), 'rows after the count are not zero'
            rows.append(tracks[b, :tc[b]])
    return rows


def feat_within_bound(sd, t32, t64, what):
    """The table's feature rows of the live slots against the fp64 twin, bound = 4 x |fp32 twin - fp64 twin|.  -> (err, bound)"""
    live = np.flatnonzero(t32.state['meta'][:, T.M_STATE] != T.FREE)
    assert len(live) and np.array_equal(sd['meta'][:, T.M_STATE], t32.state['meta'][:, T.M_STATE]), what
    bound = 4 * np.abs(t32.state['feat'][live].astype(np.float64) - t64.state['feat'][live]).max()
    err = np.abs(sd['feat'][live].astype(np.float64) - t64.state['feat'][live]).max()
    print(f'{what}: |device - twin64| {err:.3e} against the bound {bound:.3e}')
    assert 0 < bound < 4e-6 and err <= bound, (what, err, bound)
    return err, bound


# ------------------------------------------------------------------------------------------------ reid_rows
def reid_rows_np(embed, keep, counts, dtype):
    B, nq = keep.shape
    out = np.zeros((B, nq, embed.shape[2]), dtype)
    for b in range(B):
        if counts[b]:
            out[b, :counts[b]] = R.prepare(embed[b, keep[b, :counts[b]]], dtype)
    return out


@pytest.mark.parametrize('dt', ['f32', 'bf16'])
@pytest.mark.parametrize('B,nqm,nq,dim', [(2, 7, 5, 4), (3, 9, 9, 33), (1, 300, 300, 256)])
def test_reid_rows_against_numpy(B, nqm, nq, dim, dt):
    from tamtr_amd import ops
    rng = np.random.default_rng(B * 1000 + dim)
    e = torch.from_numpy((rng.normal(size=(B, nqm, dim)) * rng.uniform(0.1, 30, (B, nqm, 1))).astype(np.float32))
    if dt == 'bf16':
        e = e.to(torch.bfloat16)
    keep = np.stack([rng.permutation(nqm)[:nq] for _ in range(B)]).astype(np.int32)
    counts = np.array([nq, 0, nq // 2][:B], np.int32)
    got = ops.reid_rows(e.cuda(), torch.from_numpy(keep).cuda(), torch.from_numpy(counts).cuda()).cpu().numpy()
    src = e.float().numpy()
    w32, w64 = reid_rows_np(src, keep, counts, np.float32), reid_rows_np(src, keep, counts, np.float64)
    for b in range(B):
        assert not got[b, counts[b]:].any(), 'rows past the count are not zero'
    bound = 4 * np.abs(w32.astype(np.float64) - w64).max()
    err = np.abs(got.astype(np.float64) - w64).max()
    print(f'reid_rows {(B, nqm, nq, dim)} {dt}: |device - numpy64| {err:.3e} against the bound {bound:.3e}')
    assert 0 < bound < 2e-6 and err <= bound
    assert np.abs(np.linalg.norm(got[0].astype(np.float64), axis=1) - 1).max() < 1e-6


# ------------------------------------------------------------------------------------------------ the reference's sequences
_B1, _T64 = {}, {}


def b1(name):
    if name not in _B1:
        trk = tracker()
        frames, _, warps, feats, _ = sequence(name)
        _B1[name] = (run(trk, frames, warps, feats, 1, 32), trk.state_dict())
    return _B1[name]


def twin64_run(name):
    if name not in _T64:
        frames, _, warps, feats, _ = sequence(name)
        _T64[name] = twin(np.float64)
        for fr, w, ft in zip(frames, warps, feats):
            _T64[name].update(fr, w, ft)
    return _T64[name]


@pytest.mark.parametrize('name,B', [('crowd', 1), ('crowd', 4), ('crowd', 7), ('cross', 1), ('cross', 7), ('gaps', 1), ('gaps', 4), ('gaps', 7)])
def test_fixture_sequence_reproduces_the_reference(name, B):
    frames, want, warps, feats, who = sequence(name)
    got, sd = b1(name)
    if B > 1:   # grouped launches, across the empty frames: identical to one frame per launch, bit for bit, feat included
        trk = tracker()
        grouped = run(trk, frames, warps, feats, B, 32)
        assert all(np.array_equal(a, b) for a, b in zip(grouped, got)) and len(grouped) == len(got)
        sdB = trk.state_dict()
        live = sd['meta'][:, T.M_STATE] != T.FREE
        assert set(sd) == {'mean', 'cov', 'meta', 'sc', 'hdr', 'feat'}
        assert all(np.array_equal(sdB[k][live] if k != 'hdr' else sdB[k], sd[k][live] if k != 'hdr' else sd[k]) for k in sd)
        got, sd = grouped, sdB
    assert [len(r) for r in got] == G[f'{name}_rcnt'].tolist()
    for f, (box, ids, idx) in enumerate(want):
        same_rows(got[f], frames[f], box, ids, idx, f'{name} frame {f}')
    live = {int(m[T.M_ID]): s for s, m in enumerate(sd['meta']) if m[T.M_STATE] != T.FREE}
    fm = G[f'{name}_fin_meta']
    assert sorted(live) == fm[:, 0].tolist()
    for k, row in enumerate(fm):
        s = live[int(row[0])]
        assert sd['meta'][s, [T.M_STATE, T.M_ACT, T.M_FRAME, T.M_START, T.M_LEN, T.M_IDX]].tolist() == row[1:].tolist(), f'{name} id {row[0]}'
        assert np.array_equal(sd['sc'][s], G[f'{name}_fin_sc'][k])
        close64(sd['mean'][s], G[f'{name}_fin_mean'][k], f'{name} id {row[0]} mean')
        close64(sd['cov'][s], G[f'{name}_fin_cov'][k], f'{name} id {row[0]} cov')
    t32, t64 = twin_run(name)[0], twin64_run(name)
    feat_within_bound(sd, t32, t64, f'{name} B {B}')
    for k, row in enumerate(fm):      # and against the reference's own smooth_feat (which the fp32 twin reproduces to the bit)
        assert np.abs(sd['feat'][live[int(row[0])]] - G[f'{name}_fin_feat'][k]).max() <= 4 * float(G['feat_bound'])
    if name == 'cross':
        mine = ids_of_objects(got, who)
        assert all(len(v) == 1 for v in mine.values()) and len(mine) == 7


# ------------------------------------------------------------------------------------------------ fresh sequences
def fresh(seed, dim):
    scene, who = R.make_scene(seed, n_obj=12, frames=30, fp_every=3, gaps=[(0, 5, 3), (1, 8, 18), (2, 12, 6)], empty=(9,))
    warps = BS.camera_path(seed, len(scene), pan=(4.0, -2.0), aniso=0.003, jumps={20: (30.0, -20.0)})
    return BS.through_camera(scene, warps), warps, R.object_features(seed, who, 12, dim)


@pytest.mark.parametrize('seed,dim,B', [(402, 16, 1), (403, 16, 5), (404, 16, 7), (501, 256, 4)])
def test_fresh_sequence_equals_the_twin(seed, dim, B):
    """Seeds that are not in the fixture, under a camera with non-similarity warps and a jump; the precondition of the module
    docstring was checked on the CPU when the seeds were chosen, and is checked again here."""
    frames, warps, feats = fresh(seed, dim)
    kw = {**CFG, 'track_buffer': 10}
    trk = tracker(64, 64, dim, track_buffer=10)
    t32 = R.BotSortReidNp(dim, capacity=64, want_margin=True, **REID, **kw)
    t64 = R.BotSortReidNp(dim, capacity=64, dtype=np.float64, **REID, **kw)
    got = run(trk, frames, warps, feats, B, 64)
    for f, fr in enumerate(frames):
        want = t32.update(fr, warps[f], feats[f])
        t64.update(fr, warps[f], feats[f])
        same_rows(got[f], fr, want[:, :4], want[:, 4].astype(int), want[:, 7].astype(int), f'seed {seed} frame {f}')
    sd = trk.state_dict()
    same_table(sd, t32, f'seed {seed}')
    feat_within_bound(sd, t32, t64, f'seed {seed} D {dim}')
    delta = max(float(np.abs(a - b).max()) for a, b in zip(t32.costs, t64.costs) if a.size)
    assert t32.margin > 100 * delta * t32.max_matches and t32.thr_margin > 1e-4, (t32.margin, delta, t32.max_matches, t32.thr_margin)
    ev = t32.events
    assert ev['emb_won'] and ev['app_clipped'] and ev['feat_match2'] and ev['feat_reactivate'] and ev['match_unconfirmed'] and ev['empty_frame'], ev


# ------------------------------------------------------------------------------------------------ invariance
def test_no_embedding_can_pass_below_zero_and_the_tracker_is_plain_botsort():
    """appearance_thresh = -1: every e is set to 1, the cost is the fused IoU distance, and the rows and the whole table have the
    bits of tamtr_botsort_update on the same input; the feature table is maintained all the same."""
    frames, _, warps, feats, _ = sequence('crowd')
    a, b = tracker(appearance_thresh=-1.0), plain_tracker(64, 32, gmc_method='none')
    ra, rb = run(a, frames, warps, feats, 4, 32), run(b, frames, warps, feats, 4, 32, reid=False)
    assert all(np.array_equal(x, y) for x, y in zip(ra, rb)) and sum(len(r) for r in ra) > 500
    sa, sb = a.state_dict(), b.state_dict()
    assert set(sa) - set(sb) == {'feat'} and all(np.array_equal(sa[k], sb[k]) for k in sb)
    frames, _, warps, feats, _ = sequence('gaps')
    c = tracker(appearance_thresh=-1.0)
    rc = run(c, frames, warps, feats, 3, 32)
    t32, t64 = twin(want_margin=True, appearance_thresh=-1.0), twin(np.float64, appearance_thresh=-1.0)      # REID's value is overridden
    for f, fr in enumerate(frames):
        want = t32.update(fr, warps[f], feats[f])
        t64.update(fr, warps[f], feats[f])
        same_rows(rc[f], fr, want[:, :4], want[:, 4].astype(int), want[:, 7].astype(int), f'gaps frame {f}')
    assert t32.events['emb_won'] == 0 and t32.margin > 1e-6
    feat_within_bound(c.state_dict(), t32, t64, 'gaps without appearance')


# ------------------------------------------------------------------------------------------------ state
def test_resume_in_the_middle_of_the_crossing():
    frames, _, warps, feats, _ = sequence('cross')
    cut = 20
    a = tracker()
    head = run(a, frames[:cut], warps[:cut], feats[:cut], 4, 32)
    b = tracker()
    b.load_state_dict(a.state_dict())
    tail = run(b, frames[cut:], warps[cut:], feats[cut:], 4, 32)
    whole = tracker()
    ref = run(whole, frames[:cut], warps[:cut], feats[:cut], 4, 32) + run(whole, frames[cut:], warps[cut:], feats[cut:], 4, 32)
    assert all(np.array_equal(x, y) for x, y in zip(head + tail, ref)) and len(ref) == len(frames)
    sa, sb = b.state_dict(), whole.state_dict()
    assert 'feat' in sa and all(np.array_equal(sa[k], sb[k]) for k in sa)
    other = tracker(dim=8)
    with pytest.raises(ValueError, match='feat'):
        other.load_state_dict(sa)
    with pytest.raises(ValueError, match='feat'):
        plain_tracker(64, 32, gmc_method='none').load_state_dict(sa)


def test_overflow_and_reset_at_capacity_4():
    from tamtr_amd.track import TrackerOverflow
    rng = np.random.default_rng(9)
    d = np.stack([np.arange(7) * 100.0, np.full(7, 50.0), np.arange(7) * 100.0 + 60, np.full(7, 150.0), rng.uniform(0.7, 0.9, 7),
                  np.zeros(7)], 1).astype(np.float32)
    d2 = d + np.float32([2, -1, 2, -1, 0, 0])
    ft = rng.normal(size=(7, D)).astype(np.float16).astype(np.float32)
    w = np.tile(np.eye(2, 3), (2, 1, 1))
    trk = tracker(4, 32)
    tw = R.BotSortReidNp(D, capacity=4, **REID, **CFG)
    got = run(trk, [d, d2], w, [ft, ft], 2, 32)
    want = [tw.update(d, w[0], ft), tw.update(d2, w[1], ft)]
    sd = trk.state_dict()
    assert sd['hdr'][:4].tolist() == [2, 5, 4, 6] and np.array_equal(sd['hdr'], tw.state['hdr'])      # 3 refused in each of the two frames
    assert [len(r) for r in got] == [4, 4] == [len(r) for r in want]
    with pytest.raises(TrackerOverflow):
        trk.check_overflow(sd['hdr'][T.H_OVER])
    trk.reset()
    # after reset() the slots are taken again, by other detections: a reused slot carries the new track's feature, not the old one
    again = run(trk, [d[4:7]], w[:1], [ft[4:7]], 1, 32)
    sd2 = trk.state_dict()
    assert sorted(again[0][:, 4].astype(int)) == [1, 2, 3] and sd2['hdr'][:4].tolist() == [1, 4, 3, 0]
    new = R.prepare(ft[4:7])
    for r in again[0]:
        s = int(np.flatnonzero((sd2['meta'][:, T.M_ID] == int(r[4])) & (sd2['meta'][:, T.M_STATE] != T.FREE))[0])
        assert np.abs(sd2['feat'][s] - new[int(r[7])]).max() < 1e-6
        assert np.abs(sd2['feat'][s] - sd['feat'][s]).max() > 1e-2, 'the slot still carries the feature of the track before reset()'


# ------------------------------------------------------------------------------------------------ end to end
def decoder_outputs_keep_their_bits(model, head):
    """The switch changes no output bit.  Two predict() passes over the same files cannot show that: the trunk is not reproducible
    from one call to the next, switch or no switch (measured on MI355X at the parent commit, two eval forwards of this model on one
    input: token memory up to 5.4e-06 apart, y up to 2.4e-07 apart, with the switch off both times).  So the decoder runs on ONE token
    memory with the switch off, on, off and on: every output (y, boxes, scores, encoder picks) is equal bit for bit, and the kept
    tensor is the per-query hidden state [B, nq, hd]."""
    g = torch.Generator().manual_seed(1)
    img = torch.rand(2, 3, 128, 128, generator=g).cuda()
    with torch.no_grad():
        txt = model.txt_feats.to(img.device).float().repeat(2, 1, 1)
        feats, shapes = model.token_memory(img, txt, drop_scales=None)
        outs = []
        for flag in (False, True, False, True):
            head.keep_query_embed = flag
            y, x = head.decode(feats, shapes, txt.clone())
            outs.append([y.clone()] + [t.clone() for t in x[:4]])
            if flag:
                assert tuple(head.last_query_embed.shape) == (2, head.num_queries, head.hidden_dim)
            else:
                assert head.last_query_embed is None
    for o in outs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(outs[0], o)), 'an output of the decoder changes with keep_query_embed'
    assert head.training is False and outs[0][0].shape[1] == head.num_queries
    head.keep_query_embed = False


def test_predictor_track_with_reid_in_the_yaml(tmp_path):
    """Predictor.track(tracker='botsort.yaml' with with_reid: True) builds a BotSort with reid_dim = the decoder's hidden size, switches
    the decoder's query embedding on for the run and hands embed + keep to the tracker; this run's own out, keep and query embeddings
    through the twin give the same ids and boxes.  The decoder's outputs have the same bits with the switch on and off
    (decoder_outputs_keep_their_bits)."""
    from test_gpu_predict import CONF, IMGSZ, NC, _images, _model, _text_feats
    from tamtr_amd.predict import Predictor
    from tamtr_amd.track import BotSort
    src = _images(tmp_path)
    names = {i: f'c{i}' for i in range(NC)}
    pred = Predictor(_model().cuda(), names, _text_feats(), imgsz=IMGSZ, conf=CONF, iou=0.7, batch=2, dtype='fp32')
    head = pred.model.model[-1]
    assert head.keep_query_embed is False and head.last_query_embed is None
    plain = list(pred.predict(str(src)))
    assert head.last_query_embed is None
    decoder_outputs_keep_their_bits(pred.model, head)
    scores = np.sort(np.concatenate([d.conf.numpy() for d in plain]))
    kw = dict(track_high_thresh=float(scores[len(scores) // 2]) * 1.0001, track_low_thresh=float(scores[len(scores) // 8]) * 1.0001,
              new_track_thresh=float(scores[len(scores) * 3 // 4]) * 1.0001, match_thresh=0.8, track_buffer=30)
    kw = {k: float(f'{v:.10e}') for k, v in kw.items()}      # what the yaml below carries
    y = tmp_path / 'botsort.yaml'
    y.write_text('tracker_type: botsort\n' + ''.join(f'{k}: {v:.10e}\n' for k, v in kw.items()) +
                 'gmc_method: none\nproximity_thresh: 0.5\nappearance_thresh: 0.25\nwith_reid: True\n')
    dim = head.hidden_dim
    t32 = R.BotSortReidNp(dim, capacity=1024, want_margin=True, **REID, **kw)
    t64 = R.BotSortReidNp(dim, capacity=1024, dtype=np.float64, **REID, **kw)
    batches, run_batch = [], pred.run_batch

    def spy(ims, tracker=None):      # this run's own detections and embeddings, as they left the device
        res = run_batch(ims, tracker)
        batches.append(res + (head.last_query_embed.float().cpu().numpy(),))
        return res

    pred.run_batch = spy
    got = list(pred.track(str(src), tracker=str(y)))
    assert type(pred.tracker) is BotSort and pred.tracker.with_reid and pred.tracker.reid_dim == dim
    assert head.keep_query_embed is False, 'track() leaves the switch as it found it'
    assert [d.path for d in got] == [d.path for d in plain]
    dets = [(o[:int(c)].numpy(), e[k[:int(c)].numpy()]) for res in batches for o, k, c, e in zip(res[0], res[1], res[2], res[5])]
    n_ids = 0
    for f, (det, (raw, ft)) in enumerate(zip(got, dets)):
        want = t32.update(raw, None, ft)
        t64.update(raw, None, ft)
        if len(want) == 0:
            assert det.id is None and np.array_equal(det.boxes.numpy(), raw), f'frame {f}'
            continue
        order, worder = np.argsort(det.id.numpy()), np.argsort(want[:, 4])
        assert np.array_equal(det.id.numpy()[order], want[worder, 4].astype(np.int64)), f'frame {f}: ids'
        assert np.array_equal(det.boxes.numpy()[order, 4:6], raw[want[worder, 7].astype(int), 4:6]), f'frame {f}: score / cls of detection idx'
        np.testing.assert_allclose(det.boxes.numpy()[order, :4], want[worder, :4], rtol=1e-6, atol=5e-4)
        n_ids += len(want)
    delta = max([0.0] + [float(np.abs(a - b).max()) for a, b in zip(t32.costs, t64.costs) if a.size])
    print(f'end to end: margin {t32.margin:.3g}, delta {delta:.3g}, matches {t32.max_matches}, threshold margin {t32.thr_margin:.3g}')
    assert t32.margin > 100 * delta * t32.max_matches, 'precondition: this run has an assignment that is not unique enough'
    assert n_ids > 0 and pred.speed()['track'] > 0


def test_track_cli_with_reid_on(tmp_path):
    """tools/track.py --tracker botsort.yaml --reid on in a child process: the yaml says with_reid: False, the flag overrides it."""
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
           '--names', ','.join(names), '--source', str(tmp_path / 'uav1'), '--tracker', str(tmp_path / 'botsort.yaml'), '--reid', 'on', '--imgsz',
           str(IMGSZ), '--batch', '2', '--conf', str(CONF), '--save-txt', '--save-mot', '--project', str(tmp_path / 'runs'), '--name', 'TAMTR',
           '--dtype', 'bf16', '--capacity', '512']
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res['sequences'] == 1 and res['images'] == 3 and res['track_rows'] > 0
    labels = sorted(os.listdir(tmp_path / 'runs' / 'TAMTR' / 'labels' / 'uav1'))
    assert labels and all(f.endswith('.txt') for f in labels)
    mot = [ln.split(',') for ln in (tmp_path / 'runs' / 'TAMTR' / 'uav1.txt').read_text().splitlines()]
    assert len(mot) == res['track_rows'] and min(int(ln[1]) for ln in mot) == 1
