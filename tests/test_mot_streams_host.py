"""CPU: the stream dimension of the MOT and HOTA evaluators without a GPU: the constructors' `streams` check, the pure ground-truth
packer (track.pack_gt), the new C entries (exported, declared, argument checks before any launch, workspace sizes), the argument
parsing of tools/mot_eval.py --streams, and Predictor.track_streams' checks of gt / evaluator at call time."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import hota_cases as HC
import mot_cases as MC

NEW = ('tamtr_mot_update_streams', 'tamtr_mot_end_streams', 'tamtr_mot_streams_workspace_bytes', 'tamtr_hota_update_streams',
       'tamtr_hota_end_streams', 'tamtr_hota_streams_workspace_bytes')


# ------------------------------------------------------------------------------------------------ constructors
@pytest.mark.parametrize('bad', [0, -1, True, 2.0, '2'])
def test_constructors_refuse_bad_streams_before_touching_a_device(bad):
    """'no_such_device' would raise RuntimeError from torch.device: the streams check comes first."""
    from tamtr_amd.track import HotaEvaluator, MotEvaluator, TrackMapEvaluator
    for cls in (MotEvaluator, HotaEvaluator):
        with pytest.raises(ValueError, match='streams'):
            cls('no_such_device', 2, streams=bad)
    with pytest.raises(TypeError):      # track-mAP stays single-sequence
        TrackMapEvaluator('no_such_device', 2, streams=2)


# ------------------------------------------------------------------------------------------------ the packer
def _views(buf, B, ng):
    n = B * ng * 7
    return buf[:n].reshape(B, ng, 7), buf[n:n + B].view(np.int32), buf[n + B:].view(np.int32)


def test_pack_gt_hands_out_dense_rows_per_stream_in_order_of_appearance():
    from tamtr_amd.track import pack_gt
    box = (0, 0, 10, 10)
    # frame-major, S = 2: images 0 and 2 are stream 0, images 1 and 3 stream 1.  (class 0, id 7) is in both streams.
    frames = [np.float32([MC.G(box, 7), MC.G(box, 3, 1), MC.G(box, 99, 0, 1)]),      # the distractor keeps its id
              np.float32([MC.G(box, 7), MC.G(box, 8)]),
              np.float32([MC.G(box, 3, 1), MC.G(box, 5), MC.G(box, 7), MC.G(box, 4, 6)]),      # class 6 is out of range: id kept
              np.float32([MC.G(box, 8), MC.G(box, 9)])]
    rows = [{}, {}]
    buf = pack_gt(frames, 4, 2, rows)
    assert buf.dtype == np.float32 and buf.shape == (4 * 4 * 7 + 2 * 4,)
    gt, cnt, act = _views(buf, 4, 4)
    assert rows == [{(0, 7): 0, (1, 3): 1, (0, 5): 2}, {(0, 7): 0, (0, 8): 1, (0, 9): 2}]
    assert gt[0, :3, 4].tolist() == [0, 1, 99] and gt[1, :2, 4].tolist() == [0, 1]
    assert gt[2, :4, 4].tolist() == [1, 2, 0, 4] and gt[3, :2, 4].tolist() == [1, 2]
    assert cnt.tolist() == [3, 2, 4, 2] and act.tolist() == [1, 1, 1, 1]
    assert not gt[1, 2:].any() and np.array_equal(gt[0, :3, :4], np.float32([box] * 3))
    # a second batch goes on where the maps stand; the caller's arrays are not written to
    again = pack_gt([np.float32([MC.G(box, 6)]), np.float32([MC.G(box, 7)])], 4, 2, rows)
    assert _views(again, 2, 4)[0][:, 0, 4].tolist() == [3, 0] and frames[0][0, 4] == 7


def test_pack_gt_none_is_an_inactive_image_and_wide_frames_keep_their_count():
    from tamtr_amd.track import pack_gt
    box = (0, 0, 10, 10)
    wide = np.float32([MC.G(box, 10 + i) for i in range(5)])
    rows = [{}, {}]
    gt, cnt, act = _views(pack_gt([None, wide, np.zeros((0, 7), np.float32), None], 3, 1, rows), 4, 3)
    assert act.tolist() == [0, 1, 1, 0] and cnt.tolist() == [0, 5, 0, 0]      # an empty frame is active; 5 rows > ng = 3 keep their count
    assert gt[1, :, 4].tolist() == [0, 1, 2] and not gt[0].any() and not gt[3].any()
    assert rows == [{}, {(0, 10 + i): i for i in range(5)}]      # rows are handed out to the whole frame, as the single evaluator does
    one = [{}]      # one map: every image is the same stream's
    gt, cnt, act = _views(pack_gt([wide[:2], wide[1:3]], 3, 1, one), 2, 3)
    assert gt[0, :2, 4].tolist() == [0, 1] and gt[1, :2, 4].tolist() == [1, 2] and act.tolist() == [1, 1]


# ------------------------------------------------------------------------------------------------ C ABI
def test_new_symbols_are_exported_declared_and_the_abi_version_stays():
    from tamtr_amd import _lib
    h = _lib.lib()
    header = open(os.path.join(ROOT, 'include', 'tamtr_hip.h')).read()
    for n in NEW:
        assert n in _lib.EXPORTS and hasattr(h, n), n
        assert re.search(r'^int\s+%s\s*\(' % n, header, flags=re.M), f'{n} is not declared in tamtr_hip.h'
    assert h.tamtr_abi_version() == 36 == _lib.ABI_VERSION


def test_stream_workspaces_are_s_slices_rounded_to_16_and_zero_past_2_31():
    from tamtr_amd import _lib
    h = _lib.lib()
    for sizes in ((33, 33, 2, 32, 256), (8, 8, 1, 16, 32), (300, 300, 10, 1024, 4096)):
        one = h.tamtr_mot_workspace_bytes(*sizes)
        for S in (1, 3, 16):
            n = h.tamtr_mot_streams_workspace_bytes(S, *sizes)
            assert n >= S * one and n == S * ((one + 15) // 16 * 16), (sizes, S)
    for sizes in ((33, 33, 1), (300, 300, 64), (8, 8, 2)):
        one = h.tamtr_hota_workspace_bytes(*sizes)
        for S in (1, 3, 16):
            n = h.tamtr_hota_streams_workspace_bytes(S, *sizes)
            assert n >= S * one and n == S * ((one + 15) // 16 * 16), (sizes, S)
    assert h.tamtr_mot_streams_workspace_bytes(0, 8, 8, 1, 16, 32) == 0 and h.tamtr_hota_streams_workspace_bytes(0, 8, 8, 2) == 0
    assert h.tamtr_mot_streams_workspace_bytes(2, 0, 8, 1, 16, 32) == 0 and h.tamtr_hota_streams_workspace_bytes(2, 8, 0, 2) == 0
    # the largest S whose total stays within 2^31 - 1 bytes is the last one supported (both single sizes are multiples of 16 here)
    one = h.tamtr_mot_workspace_bytes(300, 300, 10, 1024, 4096)
    S = (2 ** 31 - 1) // one
    assert one % 16 == 0 and S == 1370 and h.tamtr_mot_streams_workspace_bytes(S, 300, 300, 10, 1024, 4096) == S * one
    assert h.tamtr_mot_streams_workspace_bytes(S + 1, 300, 300, 10, 1024, 4096) == 0
    one = h.tamtr_hota_workspace_bytes(300, 300, 64)
    S = (2 ** 31 - 1) // one
    assert one % 16 == 0 and S == 45 and h.tamtr_hota_streams_workspace_bytes(S, 300, 300, 64) == S * one
    assert h.tamtr_hota_streams_workspace_bytes(S + 1, 300, 300, 64) == 0


def test_stream_entries_check_their_arguments_before_any_launch():
    """TAMTR_EINVAL (-1) without a GPU: the non-null addresses are never dereferenced, every check comes first."""
    from tamtr_amd import _lib
    h = _lib.lib()
    z, one, odd = ctypes.c_void_p(0), ctypes.c_void_p(16), ctypes.c_void_p(8)
    need = h.tamtr_mot_streams_workspace_bytes(2, 8, 8, 1, 16, 32)
    #      tracks tcounts gt gcounts | B  S  nq ng nc thr | active gstate counts iou_sum pair hdr | G   T  | ws   bytes stream
    ok = [one] * 4 + [4, 2, 8, 8, 1, 0.5] + [z] + [one] * 5 + [16, 32, one, need, z]
    bad = lambda i, v: h.tamtr_mot_update_streams(*(ok[:i] + [v] + ok[i + 1:]))     # noqa: E731
    assert bad(5, 0) == -1 and bad(5, -2) == -1 and bad(5, 3) == -1 and bad(4, 5) == -1      # S < 1, B % S != 0
    assert all(bad(i, z) == -1 for i in (0, 1, 2, 3, 11, 12, 13, 14, 15, 18)), 'a NULL operand'
    assert bad(18, odd) == -1 and bad(19, need - 16) == -1 and bad(9, 0.0) == -1 and bad(6, 4000) == -2
    assert bad(19, h.tamtr_mot_workspace_bytes(8, 8, 1, 16, 32)) == -1      # a workspace sized for one evaluator
    #      nc S | ending gt_used gstate counts pair hdr | G   T  | ws   bytes stream
    end = [1, 2, z, one, one, one, one, one, 16, 32, one, need, z]
    bad = lambda i, v: h.tamtr_mot_end_streams(*(end[:i] + [v] + end[i + 1:]))     # noqa: E731
    assert bad(1, 0) == -1 and all(bad(i, z) == -1 for i in (3, 4, 5, 6, 7, 10)) and bad(10, odd) == -1 and bad(11, 16) == -1 and bad(0, 0) == -1

    state, caps = (ctypes.c_void_p * 12)(*[16] * 12), (ctypes.c_int * 5)(4, 8, 16, 32, 8)
    holed = (ctypes.c_void_p * 12)(*([16] * 11 + [0]))
    need = h.tamtr_hota_streams_workspace_bytes(2, 8, 8, 2)
    #      tracks tcounts gt gcounts | B  S  nq ng nc thr  eps | active state caps | ws  bytes stream
    ok = [one] * 4 + [4, 2, 8, 8, 2, 0.5, HC.EPS, z, state, caps, one, need, z]
    bad = lambda i, v: h.tamtr_hota_update_streams(*(ok[:i] + [v] + ok[i + 1:]))     # noqa: E731
    assert bad(5, 0) == -1 and bad(5, 3) == -1 and bad(4, 3) == -1
    assert all(bad(i, z) == -1 for i in (0, 1, 2, 3, 12, 13, 14)) and bad(12, holed) == -1 and bad(14, odd) == -1 and bad(15, 16) == -1
    alpha = (ctypes.c_double * 19)(*HC.ALPHA)
    #      alpha eps nc S ending nq ng workgroups state caps ws bytes stream
    end = [alpha, HC.EPS, 2, 2, z, 8, 8, 2, state, caps, one, need, z]
    bad = lambda i, v: h.tamtr_hota_end_streams(*(end[:i] + [v] + end[i + 1:]))     # noqa: E731
    assert bad(3, 0) == -1 and bad(0, z) == -1 and bad(8, holed) == -1 and bad(10, z) == -1 and bad(10, odd) == -1 and bad(11, 16) == -1
    assert bad(7, 0) == -1 and bad(7, 2000) == -2


def test_ops_know_the_leading_s():
    """The shape checks of ops come before the device is looked at: CPU tensors get as far as the refusal of the device."""
    import torch
    from tamtr_amd import TamtrHipError, ops
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)     # noqa: E731
    mot = lambda lead: {k: torch.zeros(lead + sh(2, (16, 32)), dtype=dt) for k, dt, sh in ops.MOT_STATE_SPEC}     # noqa: E731
    hota = lambda lead: {k: torch.zeros(lead + sh(2, (4, 8, 16, 32, 8)), dtype=dt) for k, dt, sh in ops.HOTA_STATE_SPEC}     # noqa: E731
    rows = lambda B: [torch.zeros(B, 8, 8), i32(B), torch.zeros(B, 8, 7), i32(B)]     # noqa: E731
    for bad in (0, -1, True, 2.0, '2'):
        with pytest.raises(TamtrHipError, match='streams'):
            ops.mot_update(*rows(4), mot((2,)), 2, 16, 32, streams=bad)
        with pytest.raises(TamtrHipError, match='streams'):
            ops.hota_workspace_bytes(8, 8, streams=bad)
    with pytest.raises(TamtrHipError, match='no multiple of streams = 2'):
        ops.mot_update(*rows(3), mot((2,)), 2, 16, 32, streams=2)
    with pytest.raises(TamtrHipError, match='no multiple of streams = 2'):
        ops.hota_update(*rows(3), hota((2,)), 2, (4, 8, 16, 32, 8), streams=2)
    with pytest.raises(TamtrHipError, match=r"state\['gstate'\].*\(2, 16, 8\)"):      # a single state where a stack is due
        ops.mot_update(*rows(4), mot(()), 2, 16, 32, streams=2)
    with pytest.raises(TamtrHipError, match=r"state\['gstate'\].*\(3, 4, 2\)"):      # a stack of another S
        ops.hota_update(*rows(6), hota((2,)), 2, (4, 8, 16, 32, 8), streams=3)
    with pytest.raises(TamtrHipError, match=r"state\['gstate'\]"):      # a stack where a single state is due
        ops.mot_end_sequence(mot((2,)), 2, 16, 32, 0)
    with pytest.raises(TamtrHipError, match='active'):
        ops.mot_update(*rows(4), mot((2,)), 2, 16, 32, streams=2, active=i32(3))
    with pytest.raises(TamtrHipError, match='active'):
        ops.hota_update(*rows(4), hota(()), 2, (4, 8, 16, 32, 8), active=i32(4))
    with pytest.raises(TamtrHipError, match='gt_used'):
        ops.mot_end_sequence(mot((2,)), 2, 16, 32, i32(3), streams=2)
    with pytest.raises(TamtrHipError, match='ending'):
        ops.hota_end_sequence(hota((2,)), 2, (4, 8, 16, 32, 8), 8, 8, streams=2, ending=torch.zeros(2))
    with pytest.raises(TamtrHipError, match='MI355X'):      # everything is right but the device
        ops.mot_update(*rows(4), mot((2,)), 2, 16, 32, streams=2, active=i32(4))
    with pytest.raises(TamtrHipError, match='MI355X'):
        ops.hota_end_sequence(hota((2,)), 2, (4, 8, 16, 32, 8), 8, 8, streams=2, ending=i32(2))
    assert ops.mot_workspace_bytes(8, 8, 1, 16, 32, streams=3) >= 3 * ops.mot_workspace_bytes(8, 8, 1, 16, 32)
    assert ops.hota_end_workgroups() == 64 == ops.hota_end_workgroups(16) and ops.hota_end_workgroups(32) == 32 and ops.hota_end_workgroups(5000) == 1
    with pytest.raises(TamtrHipError, match='1371 streams'):
        ops.mot_workspace_bytes(300, 300, 10, 1024, 4096, streams=1371)


# ------------------------------------------------------------------------------------------------ tools/mot_eval.py
def _mot_eval():
    spec = importlib.util.spec_from_file_location('mot_eval_cli', os.path.join(ROOT, 'tools', 'mot_eval.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_mot_eval_streams_argument_parsing(capsys):
    cli = _mot_eval()
    base = ['--gt', 'g', '--results', 'r', '--names', 'a,b']
    a = cli.parse_args(base + ['--streams', '3', '--hota', '--batch', '2'])
    assert a.streams == 3 and a.hota and a.batch == 2 and cli.parse_args(base).streams is None
    for more, why in ((['--streams', '2', '--host'], 'numpy path'), (['--streams', '2', '--track-map'], 'holds one sequence'),
                      (['--streams', '0'], 'positive'), (['--streams', '-3'], 'positive')):
        with pytest.raises(SystemExit):
            cli.parse_args(base + more)
        assert why in capsys.readouterr().err, more


# ------------------------------------------------------------------------------------------------ Predictor.track_streams
def _bare(cls, **attrs):
    obj = cls.__new__(cls)      # no device: only what the checks read
    for k, v in attrs.items():
        setattr(obj, k, v)
    return obj


def test_track_streams_checks_gt_and_evaluators_when_it_is_called():
    from tamtr_amd.predict import Predictor
    from tamtr_amd.track import HotaEvaluator, MotEvaluator, TrackMapEvaluator
    pred = _bare(Predictor, tracker=None)
    gt = [[], []]
    for ev in (_bare(MotEvaluator, streams=3), _bare(HotaEvaluator, streams=None), _bare(MotEvaluator, streams=1), _bare(TrackMapEvaluator),
               [_bare(MotEvaluator, streams=2), _bare(HotaEvaluator, streams=3)], object()):
        with pytest.raises(ValueError, match='streams=2'):
            pred.track_streams(['a', 'b'], gt=gt, evaluator=ev)
    with pytest.raises(ValueError, match='TrackMapEvaluator'):
        pred.track_streams(['a', 'b'], gt=gt, evaluator=_bare(TrackMapEvaluator, streams=2))
    good = [_bare(MotEvaluator, streams=2), _bare(HotaEvaluator, streams=2)]
    for bad in ([[]], [[], [], []], 'annotations', {0: []}):
        with pytest.raises(ValueError, match='list of 2 entries'):
            pred.track_streams(['a', 'b'], gt=bad, evaluator=good)
    assert pred.tracker is None
