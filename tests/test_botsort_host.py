"""CPU: the numpy twin of the BoT-SORT form of the tracker (tests/botsort_np.py) reproduces the reference's BOTSORT
(tests/golden/botsort.npz, made by tests/golden/make_botsort_golden.py), and the host side: the tracker yaml, the new symbol and
the argument checks of ops.botsort_update.  Tolerances as in test_gpu_track.py."""
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
import botsort_np as BS

CFG = dict(track_high_thresh=0.5, track_low_thresh=0.1, new_track_thresh=0.6, track_buffer=30, match_thresh=0.8)
G = dict(np.load(os.path.join(ROOT, 'tests', 'golden', 'botsort.npz')))
NAMES = ['pan', 'aniso', 'gaps']


def sequence(name, g=G):
    """-> (frames: list of f32 [n, 6], rows: list of (box [k, 4], id [k], idx [k]), warps f64 [F, 2, 3])."""
    det = np.concatenate([g[f'{name}_det'], g[f'{name}_cls'].astype(np.float32)[:, None]], 1)
    o = np.concatenate([[0], np.cumsum(g[f'{name}_cnt'])])
    r = np.concatenate([[0], np.cumsum(g[f'{name}_rcnt'])])
    frames = [det[o[i]:o[i + 1]] for i in range(len(o) - 1)]
    rows = [(g[f'{name}_box'][r[i]:r[i + 1]], g[f'{name}_id'][r[i]:r[i + 1]].astype(int), g[f'{name}_idx'][r[i]:r[i + 1]].astype(int))
            for i in range(len(r) - 1)]
    return frames, rows, g[f'{name}_warp']


def test_fixture_names_and_size():
    assert G['names'].tolist() == NAMES
    assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'botsort.npz')) < 128 * 1024
    assert all(G[f'{n}_warp'].shape == (len(G[f'{n}_cnt']), 2, 3) and G[f'{n}_warp'].dtype == np.float64 for n in NAMES)
    R = G['aniso_warp'][1, :, :2]
    assert abs(R[0] @ R[1]) > 1e-4 or abs(np.linalg.norm(R[0]) - np.linalg.norm(R[1])) > 1e-3, 'the aniso warps are similarities'


@pytest.mark.parametrize('name', NAMES)
def test_twin_reproduces_the_reference(name):
    frames, want, warps = sequence(name)
    twin = BS.BotSortNp(capacity=int(G['capacity']), want_margin=name != 'pan', **CFG)
    for f, (fr, (box, ids, idx)) in enumerate(zip(frames, want)):
        got = twin.update(fr, warps[f])
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
    assert twin.thr_margin > 1e-3 and (name == 'pan' or twin.margin > 1e-6)
    ev = twin.events
    if name == 'pan':
        assert ev['match1'] and ev['match2'] and ev['refind'] and ev['aged_out'] and ev['unconfirmed_removed'] and ev['empty_frame']
        assert ev['warp_unconfirmed'] and ev['lost_zeroed_vw_vh']
    elif name == 'gaps':
        assert ev['empty_frame'] == 4 and ev['warp_unconfirmed']


def test_the_jump_costs_tracks_without_the_warp():
    """The fixture's pan sequence jumps by about 50 px at frame `jump`: with the camera's warps every id survives it, with identity
    warps most are lost there - the sequence can tell a tracker that compensates from one that does not."""
    frames, want, warps = sequence('pan')
    J = int(G['jump'])
    kept = set(want[J - 1][1]) & set(want[J][1])
    blind = BS.BotSortNp(capacity=int(G['capacity']), **CFG)
    bids = [set(blind.update(fr)[:, 4].astype(int)) for fr in frames[:J + 1]]
    assert len(kept) >= len(want[J - 1][1]) - 1 and len(bids[J - 1] & bids[J]) < len(kept) // 2, (len(kept), len(bids[J - 1] & bids[J]))


def test_identity_warps_and_the_xyah_filter_are_bytetrack():
    """The flow the two twins share: BotSortNp with ByteTrack's filter is ByteTrackNp.  Without an image (multi_gmc skipped, as the
    reference does then) it is so bit for bit; with identity warps an unconfirmed track that went through the warp is an fp64 array,
    so its first projection's std is not derived in fp32, and the two agree up to that rounding."""
    scene = T.make_scene(206, n_obj=12, frames=40, fp_every=3, gaps=[(0, 5, 3), (1, 8, 25), (2, 12, 6)])
    kw = dict(capacity=64, track_buffer=10, **{k: v for k, v in CFG.items() if k != 'track_buffer'})
    a, b, c = T.ByteTrackNp(**kw), BS.BotSortNp(filter='xyah', **kw), BS.BotSortNp(filter='xyah', with_image=False, **kw)
    for f, fr in enumerate(scene):
        ra, rb, rc = a.update(fr), b.update(fr, np.eye(2, 3)), c.update(fr)
        assert np.array_equal(ra, rc), f'frame {f}'
        assert np.array_equal(ra[:, 4:], rb[:, 4:]), f'frame {f}'
        np.testing.assert_allclose(rb[:, :4], ra[:, :4], rtol=1e-6, atol=5e-4)
    for k in ('mean', 'cov', 'meta', 'sc', 'hdr'):
        assert np.array_equal(a.state[k], c.state[k]), k
    assert np.array_equal(a.state['meta'][:, :7], b.state['meta'][:, :7]) and np.array_equal(a.state['hdr'], b.state['hdr'])
    live = a.state['meta'][:, T.M_STATE] != T.FREE
    for k in ('mean', 'cov'):
        assert np.abs(a.state[k][live] - b.state[k][live]).max() <= 1e-6 * np.abs(a.state[k][live]).max()
    assert a.events['match2'] and a.events['refind'] and a.events['aged_out'] and a.events['unconfirmed_removed']


def test_warp_of_a_state_is_multi_gmc():
    """botsort_np.gmc against kron(I4, R) written out, on a non-similarity warp."""
    rng = np.random.default_rng(3)
    H = np.array([[1.01, -0.03, 12.5], [0.02, 0.97, -7.25]])
    m = rng.normal(0, 50, 8)
    A = rng.normal(0, 1, (8, 8))
    P = A @ A.T
    R8 = np.zeros((8, 8))
    for k in range(4):
        R8[2 * k:2 * k + 2, 2 * k:2 * k + 2] = H[:, :2]
    m2, P2 = BS.gmc(m, P, H)
    want = R8 @ m
    want[:2] += H[:, 2]
    assert np.allclose(m2, want, rtol=1e-14) and np.allclose(P2, R8 @ P @ R8.T, rtol=1e-13)
    m3, P3 = BS.gmc(m, P, np.eye(2, 3))
    assert np.array_equal(m3, m) and np.array_equal(P3, P)


# ------------------------------------------------------------------------------------------------ the tracker yaml
def test_tracker_from_yaml(tmp_path, monkeypatch):
    from tamtr_amd import track
    made = []
    monkeypatch.setattr(track.ByteTracker, '__init__', lambda self, device, **kw: made.append((type(self).__name__, kw)))
    y = tmp_path / 'bytetrack.yaml'
    y.write_text('tracker_type: bytetrack\ntrack_high_thresh: 0.4\ntrack_buffer: 45\n')
    b = tmp_path / 'botsort.yaml'
    b.write_text('tracker_type: botsort\ntrack_high_thresh: 0.5\ntrack_low_thresh: 0.1\nnew_track_thresh: 0.6\ntrack_buffer: 30\n'
                 'match_thresh: 0.8\ngmc_method: sparseOptFlow\nproximity_thresh: 0.5\nappearance_thresh: 0.25\nwith_reid: False\n')
    t = track.tracker_from_yaml(y, 'cuda', capacity=8)
    assert type(t) is track.ByteTracker and made[-1] == ('ByteTracker', dict(track_high_thresh=0.4, track_buffer=45, capacity=8))
    t = track.tracker_from_yaml(b, 'cuda', gmc_method='none', capacity=8)
    assert type(t) is track.BotSort and isinstance(t, track.ByteTracker) and t.gmc_method == 'none'
    assert (t.proximity_thresh, t.appearance_thresh, t.with_reid) == (0.5, 0.25, False)
    assert made[-1] == ('BotSort', dict(track_high_thresh=0.5, track_low_thresh=0.1, new_track_thresh=0.6, track_buffer=30, match_thresh=0.8,
                                        capacity=8))
    for method in ('orb', 'sift', 'ecc'):
        with pytest.raises(ValueError, match='sparseOptFlow'):   # the message names what is built
            track.BotSort('cuda', gmc_method=method)
    t = track.tracker_from_yaml(b, 'cuda')                       # the reference's own botsort.yaml, as it is
    assert type(t) is track.BotSort and t.gmc_method == 'sparseOptFlow' and track.BotSort('cuda').gmc_method == 'sparseOptFlow'
    with pytest.raises(ValueError, match='with_reid'):
        track.BotSort('cuda', with_reid=True)
    assert track.BotSort('cuda', gmc_method=None).gmc_method == 'none'
    (tmp_path / 'other.yaml').write_text('tracker_type: deepsort\n')
    with pytest.raises(ValueError, match='botsort'):
        track.tracker_from_yaml(tmp_path / 'other.yaml', 'cuda')
    with pytest.raises(ValueError, match='bytetrack'):           # read_tracker_yaml is ByteTracker.from_yaml's reader, as before
        track.read_tracker_yaml(b)


def test_botsort_needs_a_gpu():
    from tamtr_amd import TamtrHipError
    from tamtr_amd.track import BotSort
    with pytest.raises(TamtrHipError):
        BotSort('cpu')


def test_track_cli_help_names_gmc():
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'track.py'), '--help'], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert '--gmc' in r.stdout and 'botsort' in r.stdout


# ------------------------------------------------------------------------------------------------ the C ABI without a GPU
def _lib():
    import tamtr_amd
    from tamtr_amd import _lib
    if not os.path.exists(tamtr_amd.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib


def test_new_symbol_is_exported_and_the_abi_version_stays():
    L = _lib()
    new = ('tamtr_botsort_update', 'tamtr_gmc_estimate', 'tamtr_gmc_workspace_bytes', 'tamtr_gmc_workspace_offset', 'tamtr_gmc_state_bytes')
    assert all(n in L.EXPORTS for n in new)
    h = L.lib()
    assert h.tamtr_abi_version() == 36 == L.ABI_VERSION
    assert all(hasattr(h, n) for n in new)
    hdr = open(os.path.join(ROOT, 'include', 'tamtr_hip.h')).read()
    assert re.search(r'^int tamtr_botsort_update\(const float\* out, const int32_t\* counts, const double\* warps,', hdr, flags=re.M)


def test_botsort_c_entry_checks_its_arguments_before_any_launch():
    h = _lib().lib()
    z, one = ctypes.c_void_p(0), ctypes.c_void_p(16)
    need = h.tamtr_bytetrack_workspace_bytes(64, 32)

    def call(B=2, nq=32, T=64, ws=need, warps=z, **p):
        a = {k: p.get(k, one) for k in ('out', 'counts', 'mean', 'cov', 'meta', 'sc', 'hdr', 'tracks', 'tcounts', 'workspace')}
        return h.tamtr_botsort_update(a['out'], a['counts'], warps, B, nq, a['mean'], a['cov'], a['meta'], a['sc'], a['hdr'], T, 0.5, 0.1, 0.6,
                                      0.8, 30, a['tracks'], a['tcounts'], a['workspace'], ws, z)

    for k in ('out', 'counts', 'mean', 'cov', 'meta', 'sc', 'hdr', 'tracks', 'tcounts', 'workspace'):
        assert call(**{k: z}) == -1, k
        assert call(warps=one, **{k: z}) == -1, k
    assert call(B=0) == -1 and call(nq=0) == -1 and call(T=0) == -1 and call(ws=need - 1) == -1
    assert call(warps=ctypes.c_void_p(20)) == -1      # warps not 8-byte aligned
    assert call(T=8192, ws=2 ** 31 - 1) == -2         # the solver's state would not fit into LDS


def test_botsort_update_checks_before_any_launch():
    from tamtr_amd import TamtrHipError, ops
    _lib()
    T_ = 16

    def state(cap=T_, **over):
        s = {k: torch.zeros((cap,) + tail, dtype=dt) for k, dt, tail in ops.TRACK_STATE_SPEC}
        s['hdr'] = torch.zeros(8, dtype=torch.int32)
        s.update(over)
        return s

    out, counts, w = torch.zeros(2, 32, 6), torch.zeros(2, dtype=torch.int32), torch.zeros(2, 2, 3, dtype=torch.float64)
    bad = [(torch.zeros(2, 32, 5), counts, state(), w), (out, torch.zeros(3, dtype=torch.int32), state(), w), (out.double(), counts, state(), w),
           (out, counts.long(), state(), w), (out, counts, state(cap=T_ + 1), w), (out, counts, state(mean=torch.zeros(T_, 8)), w),
           (out, counts, state(), w.float()),                                       # warps: wrong dtype
           (out, counts, state(), torch.zeros(3, 2, 3, dtype=torch.float64)),       # wrong B
           (out, counts, state(), torch.zeros(2, 3, 3, dtype=torch.float64)),       # a 3x3 homography is not a 2x3 warp
           (out, counts, state(), np.zeros((2, 2, 3)))]                             # not a tensor
    for o, c, s, wp in bad:
        with pytest.raises(TamtrHipError, match='botsort_update'):
            ops.botsort_update(o, c, s, T_, wp)
    for wp in (w, None):
        with pytest.raises(TamtrHipError, match='CPU tensor'):       # everything right, but on the host
            ops.botsort_update(out, counts, state(), T_, wp)


def test_gmc_entries_check_their_arguments_before_any_launch():
    from tamtr_amd import TamtrHipError, ops
    h = _lib().lib()
    z, one = ctypes.c_void_p(0), ctypes.c_void_p(16)
    assert h.tamtr_gmc_workspace_bytes(2, 128, 128) > 2 * 128 * 128 * 5 and h.tamtr_gmc_state_bytes(128, 128) == 128 * 128 + 64 * 64 + 32 * 32
    assert h.tamtr_gmc_workspace_bytes(2, 124, 128) == -1 and h.tamtr_gmc_workspace_bytes(2, 128, 56) == -1 and h.tamtr_gmc_workspace_bytes(0, 128, 128) == -1
    offs = [h.tamtr_gmc_workspace_offset(2, 128, 128, i) for i in range(9)]
    assert offs[0] == 0 and offs == sorted(offs) and all(o % 16 == 0 for o in offs) and offs[8] == h.tamtr_gmc_workspace_bytes(2, 128, 128)
    need = offs[8]

    def call(B=2, H=128, W=128, ws=need, stages=15, **p):
        a = {k: p.get(k, one) for k in ('frames', 'counts', 'scale', 'pyr', 'kp', 'hdr', 'warps', 'stats', 'workspace')}
        return h.tamtr_gmc_estimate(a['frames'], a['counts'], a['scale'], B, H, W, a['pyr'], a['kp'], a['hdr'], a['warps'], a['stats'], a['workspace'],
                                    ws, stages, z)

    for k in ('frames', 'counts', 'scale', 'pyr', 'kp', 'hdr', 'warps', 'stats', 'workspace'):
        assert call(**{k: z}) == -1, k
    assert call(B=0) == -1 and call(H=124) == -1 and call(W=60) == -1 and call(H=56) == -1 and call(ws=need - 1) == -1
    assert call(stages=0) == -1 and call(stages=16) == -1 and call(warps=ctypes.c_void_p(20)) == -1 and call(workspace=ctypes.c_void_p(8)) == -1
    # the Python wrapper: dtype, H not a multiple of 8, a scale or a state of the wrong shape, CPU tensors - none reaches a launch
    fr, cnt, sc, st = torch.zeros(2, 64, 64, 3, dtype=torch.uint8), torch.ones(2, dtype=torch.int32), np.ones((2, 2)), ops.gmc_state(64, 64, 'cpu')
    for bad in (lambda: ops.gmc_estimate(fr.float(), cnt, sc, st), lambda: ops.gmc_estimate(fr[:, :60], cnt, sc, st),
                lambda: ops.gmc_estimate(fr, cnt.long(), sc, st), lambda: ops.gmc_estimate(fr, cnt, np.ones((3, 2)), st),
                lambda: ops.gmc_estimate(fr, cnt, sc, ops.gmc_state(128, 128, 'cpu')), lambda: ops.gmc_estimate(fr, cnt, sc, st),
                lambda: ops.gmc_estimate(fr, cnt, sc, st, stages=0)):
        with pytest.raises(TamtrHipError):
            bad()
    assert [lv[:2] for lv in ops.gmc_levels(640, 640)] == [(640, 640), (320, 320), (160, 160), (80, 80)] and len(ops.gmc_levels(72, 136)) == 2


def test_package_does_not_import_the_twins():
    for f in ('track.py', 'predict.py'):
        s = open(os.path.join(ROOT, 'tam-tr_amd', f)).read()
        assert not re.search(r'^\s*(from|import)\s+(oracle|bytetrack_np|botsort_np)\b', s, flags=re.M), f
