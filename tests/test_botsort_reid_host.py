"""CPU: the numpy twin of BoT-SORT with ReID (tests/botsort_reid_np.py) reproduces the reference's BOTSORT run with a stub encoder
(tests/golden/botsort_reid.npz, made by tests/golden/make_botsort_reid_golden.py), and the host side: the constructor and yaml rules,
the new symbols and the argument checks.  Box and filter tolerances as in test_gpu_track.py; a smooth_feat is held to the distance
between its fp32 and its fp64 statement that the generator measured (feat_bound)."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
import botsort_np as BS
import botsort_reid_np as R
from test_botsort_host import CFG, _lib
from test_botsort_host import sequence as _sequence

PATH = os.path.join(ROOT, 'tests', 'golden', 'botsort_reid.npz')
G = dict(np.load(PATH))
NAMES = ['crowd', 'cross', 'gaps']
D = int(G['dim'])
REID = dict(proximity_thresh=float(G['proximity_thresh']), appearance_thresh=float(G['appearance_thresh']))


def sequence(name):
    """-> (frames, rows, warps) as test_botsort_host.sequence, feats: list of f32 [n, D], who: list of int [n]."""
    frames, rows, warps = _sequence(name, G)
    o = np.concatenate([[0], np.cumsum(G[f'{name}_cnt'])])
    feats = [G[f'{name}_feat'][o[i]:o[i + 1]].astype(np.float32) for i in range(len(o) - 1)]
    who = [G[f'{name}_obj'][o[i]:o[i + 1]].astype(int) for i in range(len(o) - 1)]
    return frames, rows, warps, feats, who


def ids_of_objects(rows_per_frame, who):
    out = {}
    for rows, w in zip(rows_per_frame, who):
        for r in rows:
            if w[int(r[7])] >= 0:
                out.setdefault(int(w[int(r[7])]), set()).add(int(r[4]))
    return out


def twin(dtype=np.float32, **kw):
    return R.BotSortReidNp(D, capacity=int(G['capacity']), dtype=dtype, **{**REID, **CFG, **kw})


def test_fixture_names_and_size():
    assert G['names'].tolist() == NAMES and D == 16
    assert os.path.getsize(PATH) < 128 * 1024
    for n in NAMES:
        assert G[f'{n}_feat'].dtype == np.float16 and G[f'{n}_feat'].shape == (int(G[f'{n}_cnt'].sum()), D)
        assert G[f'{n}_fin_feat'].dtype == np.float32 and np.allclose(np.linalg.norm(G[f'{n}_fin_feat'], axis=1), 1, atol=1e-6)
    assert 0 < float(G['feat_bound']) < 1e-6


_RUNS = {}


def twin_run(name):
    """The fp32 twin over a fixture sequence, once: (twin, rows per frame)."""
    if name not in _RUNS:
        frames, _, warps, feats, _ = sequence(name)
        tw = twin(want_margin=name != 'crowd')
        _RUNS[name] = (tw, [tw.update(fr, w, ft) for fr, w, ft in zip(frames, warps, feats)])
    return _RUNS[name]


@pytest.mark.parametrize('name', NAMES)
def test_twin_reproduces_the_reference(name):
    frames, want, _, _, _ = sequence(name)
    tw, rows = twin_run(name)
    for f, (fr, got, (box, ids, idx)) in enumerate(zip(frames, rows, want)):
        assert sorted(zip(got[:, 4].astype(int), got[:, 7].astype(int))) == sorted(zip(ids, idx)), f'{name} frame {f}'
        o1, o2 = np.argsort(got[:, 4]), np.argsort(ids)
        np.testing.assert_allclose(got[o1, :4], box[o2], rtol=1e-6, atol=5e-4)
        assert np.array_equal(got[:, 5:7], fr[got[:, 7].astype(int), 4:6])
    live, lf = tw.live(), tw.live_feat()
    fm = G[f'{name}_fin_meta']
    assert sorted(live) == fm[:, 0].tolist()
    for k, row in enumerate(fm):
        t = live[int(row[0])]
        assert list(t[:6]) == row[1:].tolist() and t[6] == G[f'{name}_fin_sc'][k, 0] and t[7] == G[f'{name}_fin_sc'][k, 1]
        for a, b in ((t[8], G[f'{name}_fin_mean'][k]), (t[9], G[f'{name}_fin_cov'][k])):
            assert np.abs(a - b).max() <= 1e-6 * np.abs(b).max()
        assert np.abs(lf[int(row[0])] - G[f'{name}_fin_feat'][k]).max() <= float(G['feat_bound'])
    assert tw.thr_margin > 1e-3 and (name == 'crowd' or tw.margin > 1e-4)


def test_the_sequences_exercise_every_rule():
    ev = {}
    for name in NAMES:
        for k, v in twin_run(name)[0].events.items():
            ev[k] = max(ev.get(k, 0), v) if k == 'feat_updates_max' else ev.get(k, 0) + v
    for k in ('emb_won', 'app_clipped', 'prox_masked', 'assign_differs', 'unconf_by_embedding', 'feat_match2', 'feat_reactivate', 'empty_frame'):
        assert ev[k] >= 1, (k, ev)
    assert ev['feat_updates_max'] >= 10


def test_reid_keeps_the_ids_through_the_crossing_and_iou_alone_does_not():
    frames, want, _, _, who = sequence('cross')
    _, rows = twin_run('cross')
    mine = ids_of_objects(rows, who)
    assert len(mine) == 7 and all(len(v) == 1 for v in mine.values()), mine
    blind = BS.BotSortNp(capacity=int(G['capacity']), **CFG)
    theirs = ids_of_objects([blind.update(fr) for fr in frames], who)
    assert any(len(v) > 1 for v in theirs.values()), theirs


@pytest.mark.parametrize('name', NAMES)
def test_fp32_and_fp64_features_agree_on_every_id(name):
    frames, _, warps, feats, _ = sequence(name)
    _, rows = twin_run(name)
    t64 = twin(np.float64)
    for f, (fr, w, ft, got) in enumerate(zip(frames, warps, feats, rows)):
        r64 = t64.update(fr, w, ft)
        assert np.array_equal(r64[:, 4:], got[:, 4:]), f'{name} frame {f}'


def test_update_features_normalises_a_fresh_row_twice():
    x = np.array([[3.0, 4.0, 12.0, 1.5]], np.float32)
    once = x[0] / np.linalg.norm(x[0])
    assert np.array_equal(R.prepare(x)[0], once / np.linalg.norm(once))
    s = R.update_features(R.prepare(x)[0], R.prepare(x * 2)[0])
    assert s.dtype == np.float32 and abs(float(np.linalg.norm(s)) - 1) < 1e-6
    from scipy.spatial.distance import cdist
    rng = np.random.default_rng(0)
    a, b = rng.normal(size=(5, D)).astype(np.float32), rng.normal(size=(7, D)).astype(np.float32)
    np.testing.assert_allclose(R.embedding_distance(a, b), np.maximum(0.0, cdist(a, b, 'cosine')), rtol=0, atol=1e-15)


# ------------------------------------------------------------------------------------------------ constructor, yaml, update arguments
def test_constructor_and_yaml_rules(tmp_path, monkeypatch):
    from tamtr_amd import track
    made = []

    def init(self, device, **kw):
        made.append(kw)
        self.capacity, self.nq, self.device, self.state = kw.get('capacity', 1024), kw.get('nq', 300), 'cpu', {}

    monkeypatch.setattr(track.ByteTracker, '__init__', init)
    monkeypatch.setattr(track.ops, 'botsort_reid_workspace_bytes', lambda T_, nq: 64)
    with pytest.raises(ValueError, match=r'with_reid.*reid_dim'):
        track.BotSort('cuda', with_reid=True)
    with pytest.raises(ValueError, match='reid_dim'):
        track.BotSort('cuda', reid_dim=16)
    for bad in (0, 1025):
        with pytest.raises(ValueError, match='reid_dim'):
            track.BotSort('cuda', with_reid=True, reid_dim=bad)
    t = track.BotSort('cuda', with_reid=True, reid_dim=16, capacity=8)
    assert t.with_reid and t.reid_dim == 16 and made[-1] == dict(capacity=8)      # nothing new reaches ByteTracker.__init__
    assert tuple(t.state['feat'].shape) == (8, 16) and t.state['feat'].dtype == torch.float32
    off = track.BotSort('cuda', capacity=8)
    assert not off.with_reid and off.reid_dim is None and 'feat' not in off.state
    y = tmp_path / 'botsort.yaml'
    body = 'tracker_type: botsort\ntrack_high_thresh: 0.5\ngmc_method: none\nproximity_thresh: 0.4\nappearance_thresh: 0.2\nwith_reid: %s\n'
    y.write_text(body % 'True')
    with pytest.raises(ValueError, match=r'with_reid.*reid_dim'):
        track.tracker_from_yaml(y, 'cuda')
    t = track.tracker_from_yaml(y, 'cuda', reid_dim=32)
    assert t.with_reid and t.reid_dim == 32 and (t.proximity_thresh, t.appearance_thresh) == (0.4, 0.2)
    y.write_text(body % 'False')
    t = track.tracker_from_yaml(y, 'cuda', reid_dim=32)      # a caller that always offers its hidden size
    assert not t.with_reid and t.reid_dim is None
    assert track.tracker_from_yaml(y, 'cuda', with_reid=True, reid_dim=8).reid_dim == 8      # keywords override the file
    # update(): ReID on needs embed + keep or feats, ReID off takes neither; raised before anything touches a device
    out, counts = torch.zeros(1, 4, 6), torch.zeros(1, dtype=torch.int32)
    on = track.BotSort('cuda', with_reid=True, reid_dim=16, capacity=8)
    for kw in ({}, dict(embed=torch.zeros(1, 9, 16)), dict(keep=torch.zeros(1, 4, dtype=torch.int32)),
               dict(feats=torch.zeros(1, 4, 16), embed=torch.zeros(1, 9, 16), keep=torch.zeros(1, 4, dtype=torch.int32)),
               dict(feats=torch.zeros(1, 4, 8)), dict(feats=np.zeros((1, 4, 16), np.float32))):
        with pytest.raises(ValueError, match='with_reid'):
            on.update(out, counts, **kw)
    for kw in (dict(feats=torch.zeros(1, 4, 16)), dict(embed=torch.zeros(1, 9, 16), keep=torch.zeros(1, 4, dtype=torch.int32))):
        with pytest.raises(ValueError, match='with_reid off'):
            off.update(out, counts, **kw)
    with pytest.raises(ValueError, match='feat'):
        on.load_state_dict({'mean': 0})
    with pytest.raises(ValueError, match='feat'):
        off.load_state_dict({'feat': 0})


def test_track_cli_help_names_reid():
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'track.py'), '--help'], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert '--reid' in r.stdout


# ------------------------------------------------------------------------------------------------ the C ABI without a GPU
NEW = ('tamtr_reid_rows', 'tamtr_botsort_reid_update', 'tamtr_botsort_reid_workspace_bytes')


def test_new_symbols_are_exported_and_the_abi_version_stays():
    L = _lib()
    assert all(n in L.EXPORTS for n in NEW)
    h = L.lib()
    assert h.tamtr_abi_version() == 36 == L.ABI_VERSION
    assert all(hasattr(h, n) for n in NEW)
    hdr = open(os.path.join(ROOT, 'include', 'tamtr_hip.h')).read()
    assert re.search(r'^int tamtr_botsort_reid_update\(const float\* out, const int32_t\* counts, const double\* warps, const float\* feat,', hdr,
                     flags=re.M)
    assert re.search(r'^int tamtr_reid_rows\(const void\* embed, int dtype, const int32_t\* keep, const int32_t\* counts,', hdr, flags=re.M)
    assert 'thresh are not arguments' not in hdr


def test_reid_c_entries_check_their_arguments_before_any_launch():
    h = _lib().lib()
    z, one = ctypes.c_void_p(0), ctypes.c_void_p(16)
    need = h.tamtr_botsort_reid_workspace_bytes(64, 32)
    assert need > h.tamtr_bytetrack_workspace_bytes(64, 32) and h.tamtr_botsort_reid_workspace_bytes(0, 32) == 0
    ops_ = ('out', 'counts', 'feat', 'mean', 'cov', 'meta', 'sc', 'hdr', 'tfeat', 'tracks', 'tcounts', 'workspace')

    def call(B=2, nq=32, T_=64, D_=16, ws=need, warps=z, **p):
        a = {k: p.get(k, one) for k in ops_}
        return h.tamtr_botsort_reid_update(a['out'], a['counts'], warps, a['feat'], B, nq, a['mean'], a['cov'], a['meta'], a['sc'], a['hdr'],
                                           a['tfeat'], D_, T_, 0.5, 0.1, 0.6, 0.8, 30, 0.5, 0.25, a['tracks'], a['tcounts'], a['workspace'], ws, z)

    for k in ops_:
        assert call(**{k: z}) == -1, k
        assert call(warps=one, **{k: z}) == -1, k
    assert call(B=0) == -1 and call(nq=0) == -1 and call(T_=0) == -1 and call(D_=0) == -1 and call(D_=-3) == -1
    assert call(ws=need - 1) == -1 and call(ws=h.tamtr_bytetrack_workspace_bytes(64, 32)) == -1      # the plain tracker's size is too small
    assert call(warps=ctypes.c_void_p(20)) == -1 and call(workspace=ctypes.c_void_p(20)) == -1
    assert call(D_=1025) == -2 and call(T_=8192, ws=2 ** 31 - 1) == -2

    def rows(dtype=0, B=2, nqm=9, nq=5, D_=16, **p):
        a = {k: p.get(k, one) for k in ('embed', 'keep', 'counts', 'feat')}
        return h.tamtr_reid_rows(a['embed'], dtype, a['keep'], a['counts'], B, nqm, nq, D_, a['feat'], z)

    for k in ('embed', 'keep', 'counts', 'feat'):
        assert rows(**{k: z}) == -1, k
    assert rows(B=0) == -1 and rows(nqm=0) == -1 and rows(nq=0) == -1 and rows(D_=0) == -1
    assert rows(D_=1025) == -2 and rows(dtype=2) == -2


def test_ops_check_before_any_launch():
    from tamtr_amd import TamtrHipError, ops
    _lib()
    T_ = 16

    def state(cap=T_, dim=8, **over):
        s = {k: torch.zeros((cap,) + tail, dtype=dt) for k, dt, tail in ops.TRACK_STATE_SPEC}
        s['hdr'] = torch.zeros(8, dtype=torch.int32)
        s['feat'] = torch.zeros(cap, dim)
        s.update(over)
        return s

    out, counts, feat = torch.zeros(2, 32, 6), torch.zeros(2, dtype=torch.int32), torch.zeros(2, 32, 8)
    no_feat = state()
    del no_feat['feat']
    bad = [(out, counts, torch.zeros(2, 31, 8), state()), (out, counts, feat.double(), state()), (out, counts, feat, state(dim=9)),
           (out, counts, feat, no_feat), (out, counts, torch.zeros(2, 32, 1025), state(dim=1025)), (torch.zeros(2, 32, 5), counts, feat, state()),
           (out, counts.long(), feat, state()), (out, counts, feat, state(cap=T_ + 1)), (out, counts, np.zeros((2, 32, 8), np.float32), state())]
    for o, c, f, s in bad:
        with pytest.raises(TamtrHipError, match='botsort_reid_update'):
            ops.botsort_reid_update(o, c, f, s, T_)
    with pytest.raises(TamtrHipError, match='CPU tensor'):
        ops.botsort_reid_update(out, counts, feat, state(), T_)
    embed, keep = torch.zeros(2, 40, 8), torch.zeros(2, 32, dtype=torch.int32)
    for e, k, c in ((torch.zeros(2, 40), keep, counts), (embed, keep.long(), counts), (embed, torch.zeros(3, 32, dtype=torch.int32), counts),
                    (embed, keep, torch.zeros(3, dtype=torch.int32)), (torch.zeros(2, 40, 1025), keep, counts), (embed.half(), keep, counts)):
        with pytest.raises(TamtrHipError):
            ops.reid_rows(e, k, c)
    with pytest.raises(TamtrHipError, match='CPU tensor'):
        ops.reid_rows(embed, keep, counts)
    assert ops.botsort_reid_workspace_bytes(64, 32) > ops.bytetrack_workspace_bytes(64, 32)


def test_package_does_not_import_the_reid_twin():
    for f in ('track.py', 'predict.py', 'ops.py'):
        assert 'botsort_reid_np' not in open(os.path.join(ROOT, 'tam-tr_amd', f)).read()
