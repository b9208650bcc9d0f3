"""CPU: engine.mot_evaluate / mot_summary (the numpy statement of the MOT evaluation rule, csrc/mot.hip) against literal(), the rule in
plain loops (tests/mot_cases.py), and against the hand-worked counts; read_mot / write_mot; the C ABI; tools/mot_eval.py --host.

Tolerances: integer counts are equal.  iou_sum: both sides add the same fp64 IoUs, at most a few dozen terms in [0.5, 1], in orders
that may differ by class: 1e-12 relative (the reordering bound is n * 2^-53 = 4e-15)."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
import mot_cases as MC


def evaluate(sequences, nc, **kw):
    from tamtr_amd.engine import mot_evaluate
    return mot_evaluate(sequences, nc, **kw)


@pytest.mark.parametrize('name', sorted(MC.HAND))
def test_hand_cases_have_the_worked_counts_and_equal_the_literal_rule(name):
    from tamtr_amd.engine import mot_summary
    sequences, nc, expected = MC.HAND[name]
    got = evaluate(sequences, nc)
    MC.same_counts(got, MC.literal(sequences, nc), 1e-12, name)
    MC.check_expected(mot_summary(got), expected, name)


@pytest.mark.parametrize('seed', MC.SEEDS)
def test_random_sequences_equal_the_literal_rule(seed):
    seq, want = MC.random_cases()[seed]       # building the cases asserts their coverage condition
    MC.same_counts(evaluate([seq], 2), want, 1e-12, f'seed {seed}')


def test_random_sequences_add_up():
    from tamtr_amd.engine import mot_add_counts
    cases = MC.random_cases()
    both = evaluate([cases[s][0] for s in MC.SEEDS[:2]], 2)
    one, two = (evaluate([cases[s][0]], 2) for s in MC.SEEDS[:2])
    MC.same_counts(both, mot_add_counts(one, two), 1e-12, 'two sequences')


def test_crowded_sequence_is_well_formed():
    seq = MC.crowded_sequence()
    assert all(len(g) == 72 and (g[:, 6] == 0).sum() == 65 for g, _ in seq) and [len(t) for _, t in seq] == [70, 70, 70, 72]
    assert min(g[g[:, 6] == 0, 4].min() for g, _ in seq) > 64 and min(t[:, 4].min() for _, t in seq) > 64
    c = evaluate([seq], 3)
    assert c['IDSW'].sum() > 0 and c['FN'].sum() > 0 and c['FP'].sum() > 0 and c['drop_distractor'].sum() > 0 and c['drop_region'].sum() > 0


def _matches(fr):
    """(gt id, track id) of the IoU-only assignment of one frame of one class."""
    from scipy.optimize import linear_sum_assignment
    from tamtr_amd.engine import mot_iou_matrix
    g, t = fr
    m, _ = mot_iou_matrix(g[:, :4], t[:, :4])
    r, c = linear_sum_assignment(np.where(m >= 0.5, m, 0.0), maximize=True)
    return [(g[i, 4], t[j, 4]) for i, j in zip(r, c)]


def test_cluster_sequence_is_one_component():
    seq = MC.cluster_sequence()
    c = evaluate([seq], 1)
    assert len(seq) == 3 and all(len(g) == 70 and len(t) == 70 for g, t in seq)
    assert (c['TP'][0], c['FN'][0], c['FP'][0], c['gt_ids'][0], c['MT'][0]) == (210, 0, 0, 70, 70)
    assert c['IDSW'][0] == 0 and c['IDTP'][0] == 210      # the last-matched bonus keeps all 70 ids although the IoUs are redrawn every frame
    alone = evaluate([seq[1:2]], 1)                       # without a frame before it, a frame is matched on IoU alone
    first = {(int(g), int(t)) for g, t in _matches(seq[0])}
    assert alone['TP'][0] == 70 and {(int(g), int(t)) for g, t in _matches(seq[1])} != first


def test_another_threshold():
    sequences, nc, _ = MC.HAND['B_frame2_alone']      # IoUs 7/13 and 9/11
    assert evaluate(sequences, nc, iou=0.6)['TP'].tolist() == [2] and evaluate(sequences, nc, iou=0.9)['TP'].tolist() == [0]
    MC.same_counts(evaluate(sequences, nc, iou=0.6), MC.literal(sequences, nc, 0.6), 1e-12)


def test_summary_formulas_and_nan_rules():
    from tamtr_amd.engine import mot_new_counts, mot_summary
    c = mot_new_counts(3)
    for k, v in dict(TP=[6, 0, 0], FN=[2, 0, 3], FP=[1, 2, 0], IDSW=[1, 0, 0], gt_dets=[8, 0, 3], trk_dets=[7, 2, 0], IDTP=[4, 0, 0]).items():
        c[k][:] = v
    c['iou_sum'][:] = [4.5, 0, 0]
    s = mot_summary(c, names=['car', 'bus', 'van'])
    a, b, v = s['per_class']
    assert (a['class'], b['class'], v['class'], s['all']['class']) == ('car', 'bus', 'van', 'all')
    assert a['MOTA'] == 1 - 4 / 8 and a['MOTP'] == 4.5 / 6 and a['Recall'] == 6 / 8 and a['Precision'] == 6 / 7
    assert (a['IDFN'], a['IDFP']) == (4, 3) and a['IDF1'] == 4 / (4 + 1.5 + 2) and a['IDP'] == 4 / 7 and a['IDR'] == 4 / 8
    # no ground truth: everything over gt_dets is nan; precision is 0 / 2
    assert math.isnan(b['MOTA']) and math.isnan(b['Recall']) and math.isnan(b['IDR']) and math.isnan(b['MOTP']) and b['Precision'] == 0.0
    assert b['IDF1'] == 0.0 and b['IDP'] == 0.0
    # no tracks: precision and IDP are nan, MOTA is 0
    assert v['MOTA'] == 0.0 and math.isnan(v['Precision']) and math.isnan(v['IDP']) and v['IDF1'] == 0.0 and math.isnan(v['MOTP'])
    t = s['all']
    assert (t['TP'], t['FN'], t['FP'], t['gt_dets'], t['trk_dets'], t['IDTP']) == (6, 5, 3, 11, 9, 4)
    assert t['MOTA'] == 1 - 9 / 11 and t['IDF1'] == 4 / (4 + 2.5 + 3.5)
    empty = mot_summary(mot_new_counts(1))['all']
    assert all(math.isnan(empty[k]) for k in ('MOTA', 'MOTP', 'Recall', 'Precision', 'IDF1', 'IDP', 'IDR'))


ANNOTATION = ('1,1,10,20,30,40,1,4,0,0\n'        # car -> class 3
              '1,2,100,20,30,40,0,1,0,0\n'       # score 0 -> distractor
              '1,3,200,20,30,40,1,11,0,0\n'      # others -> distractor
              '1,4,300,300,100,100,0,0,0,0\n'    # ignored region
              '3,1,12,22,30,40,1,10,0,0\n')      # frame 2 is empty; motor -> class 9


def test_read_mot_kinds_and_category_map(tmp_path):
    from tamtr_amd.track import read_mot
    (tmp_path / 'gt.txt').write_text(ANNOTATION)
    fr = read_mot(tmp_path / 'gt.txt')
    assert len(fr) == 3 and [len(f) for f in fr] == [4, 0, 1] and all(f.dtype == np.float32 and f.shape[1] == 7 for f in fr)
    assert fr[0].tolist() == [[10, 20, 40, 60, 1, 3, 0], [100, 20, 130, 60, 2, 0, 1], [200, 20, 230, 60, 3, 0, 1], [300, 300, 400, 400, 4, 0, 2]]
    assert fr[2].tolist() == [[12, 22, 42, 62, 1, 9, 0]]
    assert len(read_mot(tmp_path / 'gt.txt', frames=5)) == 5
    mapped = read_mot(tmp_path / 'gt.txt', category_map={4: (0, 0), 10: (0, 0), 0: (0, 2)})
    assert mapped[0][:, 5:].tolist() == [[0, 0], [0, 1], [0, 1], [0, 2]] and mapped[2][0, 5:].tolist() == [0, 0]


def test_write_mot_read_mot_round_trip(tmp_path):
    from tamtr_amd.predict import Detections
    from tamtr_amd.track import read_mot, write_mot
    rows = [np.array([[10.25, 20.5, 40.75, 60.0, 0.9, 3], [1, 2, 3.5, 4.5, 0.5, 0]], np.float32), np.zeros((0, 6), np.float32),
            np.array([[5, 6, 50, 60, 0.7, 1]], np.float32)]
    ids = [[7, 9], None, [7]]
    dets = [Detections(f'{i}.png', (100, 100), {}, torch.from_numpy(r), id=None if t is None else torch.tensor(t)) for i, (r, t) in enumerate(zip(rows, ids))]
    assert write_mot(tmp_path / 'res.txt', dets) == 3
    back = read_mot(tmp_path / 'res.txt', gt=False)
    assert [f.shape for f in back] == [(2, 6), (0, 6), (1, 6)]
    for f, r, t in zip(back, rows, ids):
        if t is not None:
            assert np.array_equal(f[:, :4], r[:, :4]) and f[:, 4].tolist() == t and np.array_equal(f[:, 5], r[:, 5])


def test_new_symbols_are_exported_and_the_abi_version_stays():
    from tamtr_amd import _lib, ops, track
    h = _lib.lib()
    for n in ('tamtr_mot_update', 'tamtr_mot_end_sequence', 'tamtr_mot_workspace_bytes'):
        assert n in _lib.EXPORTS and hasattr(h, n), n
    assert h.tamtr_abi_version() == 36 == _lib.ABI_VERSION
    assert [k for k, _, _ in ops.MOT_STATE_SPEC] == ['gstate', 'counts', 'iou_sum', 'pair', 'hdr']
    assert issubclass(track.MotOverflow, RuntimeError) and callable(ops.mot_update) and callable(ops.mot_end_sequence)
    assert h.tamtr_mot_workspace_bytes(0, 8, 1, 4, 8) == 0 and h.tamtr_mot_workspace_bytes(8, 8, 1, 4, 8) >= 8 * 64 + 4 * 64
    assert ops.mot_workspace_bytes(300, 300, 10, 1024, 4096) >= 8 * 300 * 300


def test_c_entries_check_their_arguments_before_any_launch():
    import ctypes
    from tamtr_amd import _lib
    h = _lib.lib()
    z, one = ctypes.c_void_p(0), ctypes.c_void_p(16)
    need = h.tamtr_mot_workspace_bytes(8, 8, 2, 4, 8)
    ok = [one] * 4 + [2, 8, 8, 2, 0.5] + [one] * 5 + [4, 8, one, need, z]
    bad = lambda i, v: h.tamtr_mot_update(*(ok[:i] + [v] + ok[i + 1:]))     # noqa: E731
    assert bad(0, z) == -1 and bad(4, 0) == -1 and bad(8, 0.0) == -1 and bad(17, need - 1) == -1 and bad(16, ctypes.c_void_p(8)) == -1
    assert bad(5, 4000) == -2                                               # solver state beyond the LDS
    assert h.tamtr_mot_end_sequence(2, one, one, one, z, 4, 8, 0, one, need, z) == -1
    assert h.tamtr_mot_end_sequence(2, one, one, one, one, 4, 8, 0, one, 16, z) == -1


def test_cpu_tensors_are_refused():
    from tamtr_amd import TamtrHipError, ops
    from tamtr_amd.track import MotEvaluator
    with pytest.raises(TamtrHipError):
        MotEvaluator('cpu', 2)
    state = {k: torch.zeros(shape(2, (4, 8)), dtype=dt) for k, dt, shape in ops.MOT_STATE_SPEC}
    with pytest.raises(TamtrHipError):
        ops.mot_update(torch.zeros(1, 8, 8), torch.zeros(1, dtype=torch.int32), torch.zeros(1, 8, 7), torch.zeros(1, dtype=torch.int32), state, 2, 4, 8)
    with pytest.raises(TamtrHipError, match='tracks'):
        ops.mot_update(torch.zeros(1, 8, 6), torch.zeros(1, dtype=torch.int32), torch.zeros(1, 8, 7), torch.zeros(1, dtype=torch.int32), state, 2, 4, 8)


def write_case(folder, sequences):
    """The sequences of a hand case as VisDrone-MOT annotation and result files; kinds through a category map 1 -> class 0."""
    (folder / 'gt').mkdir(parents=True)
    (folder / 'res').mkdir()
    for s, frames in enumerate(sequences):
        gl, tl = [], []
        for f, (gt, trk) in enumerate(frames, 1):
            for x1, y1, x2, y2, i, c, k in gt.tolist():
                cat = 0 if k == 2 else 11 if k == 1 else int(c) + 1
                gl.append('%d,%d,%g,%g,%g,%g,1,%d,0,0\n' % (f, i, x1, y1, x2 - x1, y2 - y1, cat))
            for x1, y1, x2, y2, i, c in trk.tolist():
                tl.append('%d,%d,%.2f,%.2f,%.2f,%.2f,0.9,%d,-1,-1\n' % (f, i, x1, y1, x2 - x1, y2 - y1, int(c)))
        (folder / 'gt' / f'seq{s}.txt').write_text(''.join(gl))
        (folder / 'res' / f'seq{s}.txt').write_text(''.join(tl))


def test_mot_eval_cli_host_path_in_a_child_process(tmp_path):
    sequences, nc, expected = MC.HAND['two_sequences']
    write_case(tmp_path, sequences)
    cmd = [sys.executable, os.path.join(ROOT, 'tools', 'mot_eval.py'), '--gt', str(tmp_path / 'gt'), '--results', str(tmp_path / 'res'),
           '--names', 'thing', '--host']
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res['sequences'] == 2 and res['path'] == 'host' and sorted(res['per_sequence']) == ['seq0', 'seq1']
    MC.check_expected(res['overall'], expected, 'mot_eval --host')
    MC.check_expected(res['per_sequence']['seq0'], MC.HAND['A'][2], 'mot_eval --host seq0')
    assert res['overall']['per_class'][0]['class'] == 'thing'
