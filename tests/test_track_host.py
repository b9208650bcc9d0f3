"""CPU: the numpy twin of the tracker (tests/bytetrack_np.py) reproduces the reference's BYTETracker (tests/golden/track.npz, made by
tests/golden/make_track_golden.py), and the host side of tracking: Detections with ids, the MOT writer, the tracker yaml, the command
line and the argument checks of ops.bytetrack_update.  Tolerances as in test_gpu_track.py."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
import bytetrack_np as T

CFG = dict(track_high_thresh=0.5, track_low_thresh=0.1, new_track_thresh=0.6, track_buffer=30, match_thresh=0.8)
G = dict(np.load(os.path.join(ROOT, 'tests', 'golden', 'track.npz')))


def sequence(name):
    det = np.concatenate([G[f'{name}_det'], G[f'{name}_cls'].astype(np.float32)[:, None]], 1)
    o = np.concatenate([[0], np.cumsum(G[f'{name}_cnt'])])
    r = np.concatenate([[0], np.cumsum(G[f'{name}_rcnt'])])
    frames = [det[o[i]:o[i + 1]] for i in range(len(o) - 1)]
    rows = [(G[f'{name}_box'][r[i]:r[i + 1]], G[f'{name}_id'][r[i]:r[i + 1]].astype(int), G[f'{name}_idx'][r[i]:r[i + 1]].astype(int))
            for i in range(len(r) - 1)]
    return frames, rows


@pytest.mark.parametrize('name', ['crowd', 'twins', 'staged'])
def test_twin_reproduces_the_reference(name):
    frames, want = sequence(name)
    twin = T.ByteTrackNp(capacity=int(G['capacity']), want_margin=name != 'crowd', **CFG)
    if name == 'staged':
        twin.state = {k: G[f'staged_{k}'].copy() for k in ('mean', 'cov', 'meta', 'sc', 'hdr')}
    for f, (fr, (box, ids, idx)) in enumerate(zip(frames, want)):
        got = twin.update(fr)
        assert sorted(zip(got[:, 4].astype(int), got[:, 7].astype(int))) == sorted(zip(ids, idx)), f'{name} frame {f}'
        o1, o2 = np.argsort(got[:, 4]), np.argsort(ids)
        np.testing.assert_allclose(got[o1, :4], box[o2], rtol=1e-6, atol=5e-4)
        assert np.array_equal(got[:, 5:7], fr[got[:, 7].astype(int), 4:6])       # score and cls: copies of detection idx
    live = twin.live()
    fm = G[f'{name}_fin_meta']
    assert sorted(live) == fm[:, 0].tolist()
    for k, row in enumerate(fm):
        t = live[int(row[0])]
        assert list(t[:6]) == row[1:].tolist() and t[6] == G[f'{name}_fin_sc'][k, 0] and t[7] == G[f'{name}_fin_sc'][k, 1]
        for a, b in ((t[8], G[f'{name}_fin_mean'][k]), (t[9], G[f'{name}_fin_cov'][k])):
            assert np.abs(a - b).max() <= 1e-6 * np.abs(b).max()
    assert twin.thr_margin > 1e-3 and (name == 'crowd' or twin.margin > 1e-6)
    ev = twin.events
    if name == 'crowd':
        assert ev['match1'] and ev['match2'] and ev['refind'] and ev['aged_out'] and ev['unconfirmed_removed'] and ev['new_refused'] and ev['empty_frame']
    elif name == 'twins':
        assert ev['dup_lost_dropped'] and ev['match2'] and ev['unconfirmed_removed']
    else:
        assert ev['dup_tracked_dropped']


def test_twin_assignment_is_the_extended_lapjv_optimum():
    rng = np.random.default_rng(0)
    for n, m in ((1, 1), (3, 5), (6, 2), (7, 7)):
        cost = rng.uniform(0, 1, (n, m)).astype(np.float32)
        _, x, _ = T.lapjv_extended(cost, 0.6)
        x2, margin = T.assign(cost, 0.6, want_margin=True)
        assert np.array_equal(x, x2) and margin > 0


def test_fixture_is_small():
    assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'track.npz')) < 128 * 1024


# ------------------------------------------------------------------------------------------------ results and files
def test_save_txt_appends_the_id(tmp_path):
    from tamtr_amd.predict import Detections
    boxes = torch.tensor([[10., 20., 50., 80., 0.875, 3.], [0., 0., 200., 100., 0.5, 0.]])
    d = Detections('a.jpg', (100, 200), {0: 'x', 3: 'y'}, boxes, id=torch.tensor([7, 12]))
    f = tmp_path / 'labels' / 'a.txt'
    d.save_txt(f)
    assert f.read_text() == '3 0.15 0.5 0.2 0.6 7\n0 0.5 0.5 1 1 12\n'
    d.save_txt(f, save_conf=True)      # the id after the confidence (engine/results.py:305)
    assert f.read_text().splitlines()[2:] == ['3 0.15 0.5 0.2 0.6 0.875 7', '0 0.5 0.5 1 1 0.5 12']
    plain = Detections('a.jpg', (100, 200), {0: 'x', 3: 'y'}, boxes)
    assert plain.id is None
    g = tmp_path / 'labels' / 'b.txt'
    plain.save_txt(g, save_conf=True)
    assert g.read_text() == '3 0.15 0.5 0.2 0.6 0.875\n0 0.5 0.5 1 1 0.5\n'


def test_save_labels_carry_the_id(tmp_path):
    from PIL import Image
    from tamtr_amd.predict import Detections
    im = np.full((60, 120, 3), 128, np.uint8)
    box = torch.tensor([[10., 20., 50., 50., 0.9, 0.]])
    Detections('a.png', (60, 120), {0: 'car'}, box, orig_img=im).save(tmp_path / 'plain.png')
    Detections('a.png', (60, 120), {0: 'car'}, box, orig_img=im, id=torch.tensor([3])).save(tmp_path / 'ids.png')
    a, b = np.asarray(Image.open(tmp_path / 'plain.png')), np.asarray(Image.open(tmp_path / 'ids.png'))
    assert a.shape == b.shape == im.shape and (a != b).any()        # the label `id:3 car 0.90` is longer than `car 0.90`


def test_mot_writer(tmp_path):
    from tamtr_amd.predict import Detections
    from tamtr_amd.track import write_mot
    f1 = Detections('1.jpg', (100, 200), {}, torch.tensor([[10., 20., 50.5, 80., 0.875, 3.], [0., 0., 200., 100., 0.5, 0.]]), id=torch.tensor([2, 1]))
    f2 = Detections('2.jpg', (100, 200), {}, torch.tensor([[1., 2., 3., 4., 0.3, 1.]]))          # no track: nothing written
    f3 = Detections('3.jpg', (100, 200), {}, torch.tensor([[11., 21., 51., 81., 0.75, 3.]]), id=torch.tensor([2]))
    n = write_mot(tmp_path / 'seq.txt', [f1, f2, f3])
    assert n == 3
    assert (tmp_path / 'seq.txt').read_text().splitlines() == ['1,2,10.00,20.00,40.50,60.00,0.8750,3,-1,-1', '1,1,0.00,0.00,200.00,100.00,0.5000,0,-1,-1',
                                                               '3,2,11.00,21.00,40.00,60.00,0.7500,3,-1,-1']


def test_tracker_yaml(tmp_path):
    from tamtr_amd.track import read_tracker_yaml
    y = tmp_path / 'bytetrack.yaml'
    y.write_text('tracker_type: bytetrack  # tracker type\ntrack_high_thresh: 0.4\ntrack_low_thresh: 0.05\nnew_track_thresh: 0.7\n'
                 'track_buffer: 45\nmatch_thresh: 0.9\n# mot20: False\n')
    assert read_tracker_yaml(y) == dict(track_high_thresh=0.4, track_low_thresh=0.05, new_track_thresh=0.7, track_buffer=45, match_thresh=0.9)
    b = tmp_path / 'botsort.yaml'
    b.write_text('tracker_type: botsort\ntrack_high_thresh: 0.5\ngmc_method: sparseOptFlow\n')
    with pytest.raises(ValueError, match='bytetrack'):
        read_tracker_yaml(b)


def test_tracker_needs_a_gpu():
    from tamtr_amd import TamtrHipError
    from tamtr_amd.track import ByteTracker
    with pytest.raises(TamtrHipError):
        ByteTracker('cpu')


def test_track_cli_help_runs_without_a_gpu():
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'track.py'), '--help'], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    for flag in ('--weights', '--text-feats', '--source', '--tracker', '--save-txt', '--save-mot', '--capacity', '--project'):
        assert flag in r.stdout


def test_list_sequences(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    from track import list_sequences
    from tamtr_amd.predict import is_image_file
    from PIL import Image
    for p in ('seqs/uav2/0001.jpg', 'seqs/uav1/0001.jpg', 'seqs/uav1/0002.jpg'):
        (tmp_path / p).parent.mkdir(parents=True, exist_ok=True)
        Image.fromarray(np.zeros((8, 8, 3), np.uint8)).save(tmp_path / p)
    assert [n for n, _ in list_sequences(tmp_path / 'seqs', is_image_file)] == ['uav1', 'uav2']
    assert list_sequences(tmp_path / 'seqs' / 'uav1', is_image_file) == [('uav1', str(tmp_path / 'seqs' / 'uav1'))]


# ------------------------------------------------------------------------------------------------ the C ABI without a GPU
def _lib():
    import tamtr_amd
    from tamtr_amd import _lib
    if not os.path.exists(tamtr_amd.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib


def test_new_symbols_are_exported_and_the_abi_version_stays():
    L = _lib()
    assert 'tamtr_bytetrack_update' in L.EXPORTS and 'tamtr_bytetrack_workspace_bytes' in L.EXPORTS
    h = L.lib()
    assert h.tamtr_abi_version() == 36 == L.ABI_VERSION
    assert h.tamtr_bytetrack_workspace_bytes(64, 32) == 4 * (64 * 32 + 11 * 64 + 9 * 32)
    assert h.tamtr_bytetrack_workspace_bytes(0, 32) == 0


def test_bytetrack_c_entry_checks_its_arguments_before_any_launch():
    h = _lib().lib()
    z, one = ctypes.c_void_p(0), ctypes.c_void_p(16)
    need = h.tamtr_bytetrack_workspace_bytes(64, 32)

    def call(B=2, nq=32, T=64, ws=need, **p):
        a = {k: p.get(k, one) for k in ('out', 'counts', 'mean', 'cov', 'meta', 'sc', 'hdr', 'tracks', 'tcounts', 'workspace')}
        return h.tamtr_bytetrack_update(a['out'], a['counts'], B, nq, a['mean'], a['cov'], a['meta'], a['sc'], a['hdr'], T, 0.5, 0.1, 0.6, 0.8, 30,
                                        a['tracks'], a['tcounts'], a['workspace'], ws, z)

    for k in ('out', 'counts', 'mean', 'cov', 'meta', 'sc', 'hdr', 'tracks', 'tcounts', 'workspace'):
        assert call(**{k: z}) == -1, k
    assert call(B=0) == -1 and call(nq=0) == -1 and call(T=0) == -1 and call(ws=need - 1) == -1
    assert call(T=8192, ws=2 ** 31 - 1) == -2        # the solver's state would not fit into LDS


def test_bytetrack_update_checks_before_any_launch():
    from tamtr_amd import TamtrHipError, ops
    _lib()
    T_ = 16

    def state(cap=T_, **over):
        s = {k: torch.zeros((cap,) + tail, dtype=dt) for k, dt, tail in ops.TRACK_STATE_SPEC}
        s['hdr'] = torch.zeros(8, dtype=torch.int32)
        s.update(over)
        return s

    out, counts = torch.zeros(2, 32, 6), torch.zeros(2, dtype=torch.int32)
    bad = [(torch.zeros(2, 32, 5), counts, state()), (torch.zeros(32, 6), counts, state()), (out, torch.zeros(3, dtype=torch.int32), state()),
           (out.double(), counts, state()), (out, counts.long(), state()), (out, counts, state(cap=T_ + 1)),
           (out, counts, state(mean=torch.zeros(T_, 8))), (out, counts, state(hdr=torch.zeros(4, dtype=torch.int32))),
           (out, counts, {k: v for k, v in state().items() if k != 'cov'})]
    for o, c, s in bad:
        with pytest.raises(TamtrHipError, match='bytetrack_update'):
            ops.bytetrack_update(o, c, s, T_)
    with pytest.raises(TamtrHipError, match='CPU tensor'):       # everything right, but on the host
        ops.bytetrack_update(out, counts, state(), T_)


def test_package_does_not_import_the_oracle_or_the_twin():
    for f in ('track.py', 'predict.py'):
        s = open(os.path.join(ROOT, 'tam-tr_amd', f)).read()
        assert not re.search(r'^\s*(from|import)\s+(oracle|bytetrack_np)\b', s, flags=re.M), f
