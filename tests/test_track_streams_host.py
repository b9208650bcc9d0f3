"""CPU: the host side of multi-stream tracking (one tracker per stream, one launch): the file-to-batch bookkeeping of
Predictor.track_streams, the argument checks of the constructors, of tracker_from_yaml, of track_streams, of the ops and of the C entry
points - all of which come before anything touches a device - and tools/track.py's --streams."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT


def _lib():
    import tamtr_amd
    from tamtr_amd import _lib
    if not os.path.exists(tamtr_amd.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib


# ------------------------------------------------------------------------------------------------ stream_batches
FILES = [['a0', 'a1', 'a2'], ['b0'], ['c0', 'c1'], []]      # streams of lengths 3, 1, 2 and 0


def test_stream_batches_one_frame_per_stream():
    from tamtr_amd.predict import stream_batches
    got = stream_batches(FILES, 1)
    assert [a for _, a in got] == [[True, True, True, False], [True, False, True, False], [True, False, False, False]]
    assert [p for p, _ in got] == [['a0', 'b0', 'c0', 'a0'], ['a1', 'a1', 'c1', 'a1'], ['a2'] * 4]


def test_stream_batches_two_frames_per_stream():
    from tamtr_amd.predict import stream_batches
    got = stream_batches(FILES, 2)
    assert len(got) == 2 and all(len(p) == len(a) == 2 * 4 for p, a in got)      # B = F * S, frame-major: entry f * S + s
    assert got[0] == (['a0', 'b0', 'c0', 'a0', 'a1', 'a0', 'c1', 'a0'], [True, True, True, False, True, False, True, False])
    assert got[1] == (['a2'] * 8, [True] + [False] * 7)


@pytest.mark.parametrize('F', [1, 2, 3, 5])
def test_stream_batches_keep_every_stream_in_order_and_pad_with_a_loaded_image(F):
    from tamtr_amd.predict import stream_batches
    S = len(FILES)
    per_stream = [[] for _ in FILES]
    for paths, active in stream_batches(FILES, F):
        assert len(paths) == len(active) == F * S and any(active)
        live = {p for p, a in zip(paths, active) if a}
        for i, (p, a) in enumerate(zip(paths, active)):
            if a:
                per_stream[i % S].append(p)
            else:
                assert p in live, 'padding must be an image the batch loads anyway'
    assert per_stream == FILES


def test_stream_batches_refuses_no_sources_and_no_frames():
    from tamtr_amd.predict import stream_batches
    with pytest.raises(ValueError, match='at least one source'):
        stream_batches([], 1)
    with pytest.raises(ValueError, match='frames_per_stream'):
        stream_batches(FILES, 0)
    assert stream_batches([[], []], 2) == []


# ------------------------------------------------------------------------------------------------ constructors, yaml, track_streams
@pytest.mark.parametrize('bad', [0, -2, True, 2.0, '2'])
def test_constructors_refuse_bad_streams_before_the_device(tmp_path, bad):
    """The device named here does not exist on a machine without a GPU: the ValueError has to come first."""
    from tamtr_amd.track import BotSort, ByteTracker, tracker_from_yaml
    for make in (lambda: ByteTracker('cuda', streams=bad), lambda: BotSort('cuda', streams=bad), lambda: BotSort('cuda', gmc_method='none', streams=bad)):
        with pytest.raises(ValueError, match='streams'):
            make()
    for kind in ('bytetrack', 'botsort'):
        (tmp_path / f'{kind}.yaml').write_text(f'tracker_type: {kind}\ntrack_buffer: 30\n')
        with pytest.raises(ValueError, match='streams'):
            tracker_from_yaml(str(tmp_path / f'{kind}.yaml'), 'cuda', streams=bad)


def _bare(cls, **attrs):
    obj = cls.__new__(cls)      # no device: only what the checks read
    for k, v in attrs.items():
        setattr(obj, k, v)
    return obj


def test_track_streams_checks_its_arguments_when_called():
    from tamtr_amd.predict import Predictor
    from tamtr_amd.track import ByteTracker
    pred = _bare(Predictor, tracker=None)
    for streams in (3, None, 1):      # two sources need streams=2
        with pytest.raises(ValueError, match='streams=2'):
            pred.track_streams(['a', 'b'], tracker=_bare(ByteTracker, streams=streams))
    for none in ([], (), 'a_directory', None):      # one source per stream, in a list
        with pytest.raises(ValueError, match='list of sources'):
            pred.track_streams(none)
    assert pred.tracker is None


def test_reset_and_stream_state_refuse_a_stream_that_is_not_there():
    from tamtr_amd.track import ByteTracker
    trk = _bare(ByteTracker, streams=3, state={})
    for bad in (3, -1, True, 1.0):
        with pytest.raises(ValueError, match='0 .. 2'):
            trk.reset(stream=bad)
        with pytest.raises(ValueError, match='0 .. 2'):
            trk.stream_state(bad)
    with pytest.raises(ValueError, match='without streams'):
        _bare(ByteTracker, streams=None, state={}).reset(stream=0)


def test_check_overflow_names_the_streams():
    from tamtr_amd.track import ByteTracker, TrackerOverflow
    trk = _bare(ByteTracker, streams=3, capacity=4)
    trk.check_overflow(np.zeros(3, np.int32))
    trk.check_overflow(torch.zeros(3, dtype=torch.int32))
    with pytest.raises(TrackerOverflow, match=r'\(stream 0: 5, stream 2: 1\)') as e:
        trk.check_overflow(torch.tensor([5, 0, 1], dtype=torch.int32))
    assert 'stream 1' not in str(e.value) and 'holds 4 tracks' in str(e.value)
    one = _bare(ByteTracker, streams=None, capacity=4)      # a single tracker's message is the one it had
    one.check_overflow(0)
    with pytest.raises(TrackerOverflow, match='^2 new tracks found no free slot'):
        one.check_overflow(np.int32(2))


# ------------------------------------------------------------------------------------------------ ops and the C entry points
def _state(S=None, cap=16, dim=None, **over):
    from tamtr_amd import ops
    lead = () if S is None else (S,)
    s = {k: torch.zeros(lead + (cap,) + tail, dtype=dt) for k, dt, tail in ops.TRACK_STATE_SPEC}
    s['hdr'] = torch.zeros(lead + (8,), dtype=torch.int32)
    if dim:
        s['feat'] = torch.zeros(lead + (cap, dim))
    s.update(over)
    return s


def test_ops_check_the_stream_dimension_before_any_launch():
    """CPU tensors: a call that passed every shape check would end at 'CPU tensor', so each message below is an earlier check's."""
    from tamtr_amd import TamtrHipError, ops
    _lib()
    out, counts = torch.zeros(4, 32, 6), torch.zeros(4, dtype=torch.int32)
    w, feat = torch.zeros(4, 2, 3, dtype=torch.float64), torch.zeros(4, 32, 8)
    for fn, extra in ((ops.bytetrack_update, ()), (ops.botsort_update, (w,))):
        with pytest.raises(TamtrHipError, match='no multiple of streams = 3'):
            fn(out, counts, _state(3), 16, *extra, streams=3)
        with pytest.raises(TamtrHipError, match=r"state\['mean'\].*\(2, 16, 8\).*streams 2"):      # a single tracker's table
            fn(out, counts, _state(), 16, *extra, streams=2)
        with pytest.raises(TamtrHipError, match=r"state\['hdr'\].*\(2, 8\)"):
            fn(out, counts, _state(2, hdr=torch.zeros(8, dtype=torch.int32)), 16, *extra, streams=2)
        with pytest.raises(TamtrHipError, match=r"state\['mean'\].*\(16, 8\)"):      # and a stacked one without streams
            fn(out, counts, _state(2), 16, *extra)
        for bad in (0, -1, True, 2.0):
            with pytest.raises(TamtrHipError, match='streams must be'):
                fn(out, counts, _state(2), 16, *extra, streams=bad)
        with pytest.raises(TamtrHipError, match='CPU tensor'):
            fn(out, counts, _state(2), 16, *extra, streams=2)
    with pytest.raises(TamtrHipError, match=r"state\['feat'\].*\(2, 16, 8\)"):
        ops.botsort_reid_update(out, counts, feat, _state(2, dim=8, feat=torch.zeros(16, 8)), 16, streams=2)
    with pytest.raises(TamtrHipError, match='no multiple of streams = 3'):
        ops.botsort_reid_update(out, counts, feat, _state(3, dim=8), 16, streams=3)
    with pytest.raises(TamtrHipError, match='CPU tensor'):
        ops.botsort_reid_update(out, counts, feat, _state(2, dim=8), 16, w, streams=2)
    # the estimator
    fr, cnt, sc = torch.zeros(4, 64, 64, 3, dtype=torch.uint8), torch.ones(4, dtype=torch.int32), np.ones((4, 2))
    st = ops.gmc_state(64, 64, 'cpu', streams=2)
    assert {k: tuple(v.shape) for k, v in st.items()} == {'pyr': (2, 64 * 64 + 32 * 32), 'kp': (2, 1024), 'hdr': (2, 4)}
    assert all(v.is_contiguous() and v[1].is_contiguous() for v in st.values())
    with pytest.raises(TamtrHipError, match='no multiple of streams = 3'):
        ops.gmc_estimate(fr, cnt, sc, ops.gmc_state(64, 64, 'cpu', streams=3), streams=3)
    with pytest.raises(TamtrHipError, match=r"state\['pyr'\].*streams=2"):
        ops.gmc_estimate(fr, cnt, sc, ops.gmc_state(64, 64, 'cpu'), streams=2)
    with pytest.raises(TamtrHipError, match=r"state\['pyr'\]"):
        ops.gmc_estimate(fr, cnt, sc, st)
    with pytest.raises(TamtrHipError, match='CPU tensor'):
        ops.gmc_estimate(fr, cnt, sc, st, streams=2)
    with pytest.raises(TamtrHipError, match='streams must be'):
        ops.gmc_state(64, 64, 'cpu', streams=0)


def test_workspace_of_a_stack_is_the_rounded_single_size_per_stream():
    from tamtr_amd import ops
    h = _lib().lib()
    for one, many, py in ((h.tamtr_bytetrack_workspace_bytes, h.tamtr_bytetrack_streams_workspace_bytes, ops.bytetrack_workspace_bytes),
                          (h.tamtr_botsort_reid_workspace_bytes, h.tamtr_botsort_reid_streams_workspace_bytes, ops.botsort_reid_workspace_bytes)):
        for T_, nq in ((64, 32), (5, 7), (1, 1), (1024, 300)):      # (1, 1): a single size that is no multiple of 16
            n = one(T_, nq)
            stride = (n + 15) // 16 * 16
            assert n > 0 and n % 4 == 0 and [many(S, T_, nq) for S in (1, 2, 3, 16)] == [S * stride for S in (1, 2, 3, 16)]
            assert py(T_, nq) == n and py(T_, nq, 3) == 3 * stride
        assert one(1, 1) % 16 and many(0, 64, 32) == 0 and many(2, 0, 32) == 0 and many(2, 64, 0) == 0
        assert many(1 << 20, 1024, 300) == 0      # beyond 2^31 - 1 bytes
    with pytest.raises(_lib().TamtrHipError, match='streams'):
        ops.bytetrack_workspace_bytes(1 << 20, 300, 1 << 10)


def test_c_entries_check_the_stream_dimension_before_any_launch():
    h = _lib().lib()
    z, one = ctypes.c_void_p(0), ctypes.c_void_p(16)
    T_, nq = 64, 32
    tabs = (one,) * 5
    rule = (0.5, 0.1, 0.6, 0.8, 30)

    def byte(B=4, S=2, ws=None):
        ws = h.tamtr_bytetrack_streams_workspace_bytes(max(S, 1), T_, nq) if ws is None else ws
        return h.tamtr_bytetrack_update_streams(one, one, B, S, nq, *tabs, T_, *rule, one, one, one, ws, z)

    def bot(B=4, S=2, ws=None, warps=z):
        ws = h.tamtr_bytetrack_streams_workspace_bytes(max(S, 1), T_, nq) if ws is None else ws
        return h.tamtr_botsort_update_streams(one, one, warps, B, S, nq, *tabs, T_, *rule, one, one, one, ws, z)

    def reid(B=4, S=2, ws=None, feat=one, tfeat=one):
        ws = h.tamtr_botsort_reid_streams_workspace_bytes(max(S, 1), T_, nq) if ws is None else ws
        return h.tamtr_botsort_reid_update_streams(one, one, z, feat, B, S, nq, *tabs, tfeat, 8, T_, *rule, 0.5, 0.25, one, one, one, ws, z)

    for call, single in ((byte, h.tamtr_bytetrack_workspace_bytes(T_, nq)), (bot, h.tamtr_bytetrack_workspace_bytes(T_, nq)),
                         (reid, h.tamtr_botsort_reid_workspace_bytes(T_, nq))):
        assert call(B=3) == -1 and call(B=5) == -1          # B % S
        assert call(S=0) == -1 and call(S=-1) == -1
        assert call(ws=single) == -1                        # a workspace sized for one tracker
        assert call(B=0) == -1
    assert bot(warps=ctypes.c_void_p(20)) == -1 and reid(feat=z) == -1 and reid(tfeat=z) == -1
    need = h.tamtr_gmc_workspace_bytes(4, 128, 128)

    def gmc(B=4, S=2, **p):
        a = {k: p.get(k, one) for k in ('frames', 'counts', 'scale', 'pyr', 'kp', 'hdr', 'warps', 'stats', 'workspace')}
        return h.tamtr_gmc_estimate_streams(a['frames'], a['counts'], a['scale'], B, S, 128, 128, a['pyr'], a['kp'], a['hdr'], a['warps'], a['stats'],
                                            a['workspace'], need, 15, z)

    assert gmc(S=3) == -1 and gmc(S=0) == -1 and gmc(S=8) == -1 and gmc(hdr=z) == -1


def test_new_symbols_are_declared_with_the_lines_they_replace():
    L = _lib()
    new = ('tamtr_bytetrack_update_streams', 'tamtr_botsort_update_streams', 'tamtr_botsort_reid_update_streams', 'tamtr_gmc_estimate_streams',
           'tamtr_bytetrack_streams_workspace_bytes', 'tamtr_botsort_reid_streams_workspace_bytes')
    h = L.lib()
    assert all(n in L.EXPORTS and hasattr(h, n) for n in new)
    hdr = open(os.path.join(ROOT, 'include', 'tamtr_hip.h')).read()
    assert all(f'int {n}(' in hdr for n in new) and 'trackers/track.py:33-53' in hdr
    assert h.tamtr_abi_version() == L.ABI_VERSION      # new symbols only, no signature changed


# ------------------------------------------------------------------------------------------------ tools/track.py
def test_track_cli_parses_streams_and_refuses_gt_with_it(capsys):
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import track as cli
    base = ['--weights', 'w.pt', '--text-feats', 'f.npz', '--names', 'a,b', '--source', 'seqs']
    assert cli.parse_args(base).streams is None
    a = cli.parse_args(base + ['--streams', '4', '--batch', '2', '--save-mot'])
    assert a.streams == 4 and a.batch == 2
    with pytest.raises(SystemExit):
        cli.parse_args(base + ['--streams', '2', '--gt', 'annotations'])
    assert 'tools/mot_eval.py' in capsys.readouterr().err
    with pytest.raises(SystemExit):
        cli.parse_args(base + ['--streams', '0'])
