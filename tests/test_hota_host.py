"""CPU: engine.hota_evaluate / hota_summary (the numpy statement of the HOTA rule, csrc/hota.hip) against the hand-worked values and
against literal(), the rule in plain loops (tests/hota_cases.py); the C ABI and the argument checks of ops.hota_*; tools/mot_eval.py
--host --hota.

Tolerances: integer counts are equal.  The fp64 sums: both sides add the same terms, a few dozen at most, in orders that may differ
(numpy sums a row pairwise, the loops in order), and pot carries the same reordering into gas: 1e-12 relative (the bound is a few
n * 2^-53 = 1e-14).  unique_optimum() holds on every sequence used, so no matching can depend on those last bits."""
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
from test_mot_host import write_case


def evaluate(sequences, nc, **kw):
    from tamtr_amd.engine import hota_evaluate
    return hota_evaluate(sequences, nc, **kw)


@pytest.mark.parametrize('name', sorted(HC.HAND))
def test_hand_cases_have_the_worked_values_and_equal_the_literal_rule(name):
    from tamtr_amd.engine import hota_summary
    sequences, nc, expected = HC.HAND[name]
    got = evaluate(sequences, nc)
    HC.same_counts(got, HC.literal(sequences, nc), 1e-12, name)
    HC.check_expected(hota_summary(got), expected, name)


def test_thresholds_are_numpys_not_k_over_20():
    from tamtr_amd import engine
    assert engine.HOTA_ALPHA.tolist() == HC.ALPHA and len(HC.ALPHA) == 19 and engine.HOTA_EPS == HC.EPS == 2.0 ** -52
    assert 0.7500000000000001 in HC.ALPHA and 0.9500000000000001 in HC.ALPHA and 0.75 not in HC.ALPHA and HC.ALPHA[4] == 0.25


@pytest.mark.parametrize('seed', MC.SEEDS)
def test_random_sequences_equal_the_literal_rule_and_mot_evaluates_dets(seed):
    from tamtr_amd.engine import mot_evaluate
    seq = MC.random_cases()[seed][0]
    assert HC.unique_optimum(seq, 2) >= 1e-9
    got = evaluate([seq], 2)
    HC.same_counts(got, HC.literal([seq], 2), 1e-12, f'seed {seed}')
    mot = mot_evaluate([seq], 2)
    assert got['gt_dets'].tolist() == mot['gt_dets'].tolist() and got['trk_dets'].tolist() == mot['trk_dets'].tolist()
    # HOTA sees more than CLEAR does: pairs below IoU 0.5 are TPs at the low thresholds
    assert (got['TP'][:, 0] >= got['TP'][:, 9]).all() and got['TP'].sum() > 0 and (np.diff(got['TP'], axis=1) <= 0).all()


def test_wide_sequences_have_a_unique_optimum_with_the_real_preprocessing():
    assert HC.unique_optimum(MC.crowded_sequence(), 3) >= 1e-9
    assert HC.unique_optimum(MC.cluster_sequence(), 1) >= 1e-9


def test_counts_of_sequences_add():
    from tamtr_amd.engine import hota_add_counts, hota_new_counts
    cases = MC.random_cases()
    both = evaluate([cases[s][0] for s in MC.SEEDS[:2]], 2)
    one, two = (evaluate([cases[s][0]], 2) for s in MC.SEEDS[:2])
    HC.same_counts(both, hota_add_counts(one, two), 1e-12, 'two sequences')
    HC.same_counts(hota_add_counts(hota_new_counts(2), one), one, 0.0, 'zero + one')
    assert evaluate([], 2)['TP'].shape == (2, 19)


def test_matching_on_iou_alone_fails_the_alignment_case(monkeypatch):
    from tamtr_amd import engine
    sequences, nc, expected = HC.HAND['alignment']
    assert HC.literal(sequences, nc, match_on_iou=True)['TP'][0] == HC.upto(18, 4, 3)
    monkeypatch.setattr(engine, '_hota_assign', lambda score, S: engine._mot_assign(S))
    mutant = engine.hota_evaluate(sequences, nc)
    assert mutant['TP'][0].tolist() == HC.upto(18, 4, 3)
    with pytest.raises(AssertionError):
        HC.check_expected(engine.hota_summary(mutant), expected, 'mutant')


def test_summary_formulas_and_zero_denominators():
    from tamtr_amd.engine import HOTA_RATIOS, hota_new_counts, hota_summary, hota_table
    s = hota_summary(hota_new_counts(2), ['a', 'b'])
    for r in s['per_class'] + [s['all']]:
        assert r['LocA'] == 1.0 and r['LocA_alpha'] == [1.0] * 19 and r['LocA(0)'] == 1.0
        assert all(r[k] == 0.0 and r[k + '_alpha'] == [0.0] * 19 for k in HOTA_RATIOS if k != 'LocA')
        assert r['HOTA(0)'] == 0.0 and r['HOTALocA(0)'] == 0.0 and r['gt_dets'] == 0
    assert [r['class'] for r in s['per_class']] == ['a', 'b'] and s['all']['class'] == 'all'
    c = hota_new_counts(2)
    c['TP'][0], c['FN'][0], c['FP'][0] = 6, 2, 4
    c['loc_sum'][0], c['ass_sum'][0], c['assre_sum'][0], c['asspr_sum'][0] = 4.5, 3.0, 4.5, 6.0
    c['TP'][1, 0], c['FN'][1, 0], c['ass_sum'][1, 0], c['loc_sum'][1, 0] = 2, 2, 1.0, 2.0
    c['gt_dets'][:], c['trk_dets'][:] = (8, 4), (10, 2)
    s = hota_summary(c)
    r = s['per_class'][0]
    want = dict(DetA=0.5, DetRe=0.75, DetPr=0.6, AssA=0.5, AssRe=0.75, AssPr=1.0, LocA=0.75, HOTA=0.5)
    assert all(r[k + '_alpha'] == [v] * 19 and abs(r[k] - v) < 1e-15 for k, v in want.items()), r
    assert r['HOTA(0)'] == 0.5 and r['LocA(0)'] == 0.75 and r['HOTALocA(0)'] == 0.5 * 0.75 and r['class'] == 0
    a = s['all']      # counts sum over classes, then the ratios: (6 + 2) / (8 + 4 + 4) at the first threshold
    assert a['DetA_alpha'][0] == 0.5 and a['AssA_alpha'][0] == 0.5 and a['DetA_alpha'][1] == 0.5 and a['gt_dets'] == 12 and a['TP'][0] == 8
    assert abs(a['HOTA'] - np.mean([0.5] * 19)) < 1e-15
    lines = hota_table(s, 'seq').splitlines()
    assert len(lines) == 4 and lines[0].split()[:4] == ['seq', 'HOTA', 'DetA', 'AssA'] and lines[-1].split()[0] == 'all'


def test_new_symbols_are_exported_and_the_abi_version_stays():
    from tamtr_amd import _lib, ops, track
    h = _lib.lib()
    for n in ('tamtr_hota_update', 'tamtr_hota_end_sequence', 'tamtr_hota_workspace_bytes'):
        assert n in _lib.EXPORTS and hasattr(h, n), n
    assert h.tamtr_abi_version() == 36 == _lib.ABI_VERSION
    assert [k for k, _, _ in ops.HOTA_STATE_SPEC] == ['gstate', 'tcount', 'pkey', 'ppot', 'phist', 'fidx', 'log', 'dets', 'tp_lvl', 'loc_lvl', 'ass', 'hdr']
    assert issubclass(track.HotaOverflow, RuntimeError) and callable(ops.hota_update) and callable(ops.hota_end_sequence)
    assert h.tamtr_hota_workspace_bytes(0, 8, 1) == 0 and h.tamtr_hota_workspace_bytes(8, 8, 0) == 0
    assert ops.hota_workspace_bytes(8, 8, 4) >= 4 * 8 * 64 and ops.HOTA_END_WORKGROUPS >= 1
    # state, log and workspace at the default capacities stay under 128 MiB, and no tensor of the state has a [19, G, T] shape
    caps = (1024, 4096, 1 << 18, 1 << 20, 4096)
    total = ops.hota_workspace_bytes(300, 300)
    for _, dt, shape in ops.HOTA_STATE_SPEC:
        total += int(np.prod(shape(10, caps))) * torch.empty(0, dtype=dt).element_size()
    assert total < 128 << 20, total


def test_c_entries_check_their_arguments_before_any_launch():
    import ctypes
    from tamtr_amd import _lib
    h = _lib.lib()
    z, one = ctypes.c_void_p(0), ctypes.c_void_p(16)
    state, caps = (ctypes.c_void_p * 12)(*[16] * 12), (ctypes.c_int * 5)(4, 8, 16, 32, 8)
    holed = (ctypes.c_void_p * 12)(*([16] * 11 + [0]))
    need = h.tamtr_hota_workspace_bytes(8, 8, 2)
    ok = [one] * 4 + [2, 8, 8, 2, 0.5, HC.EPS, state, caps, one, need, z]
    bad = lambda i, v: h.tamtr_hota_update(*(ok[:i] + [v] + ok[i + 1:]))     # noqa: E731
    assert bad(0, z) == -1 and bad(4, 0) == -1 and bad(8, 0.0) == -1 and bad(9, 0.0) == -1 and bad(10, holed) == -1 and bad(10, z) == -1
    assert bad(11, (ctypes.c_int * 5)(4, 8, 0, 32, 8)) == -1 and bad(13, 16) == -1 and bad(12, ctypes.c_void_p(8)) == -1
    assert bad(5, 4000) == -2                                               # solver state beyond the LDS
    alpha = (ctypes.c_double * 19)(*HC.ALPHA)
    end = [alpha, HC.EPS, 2, 8, 8, 2, state, caps, one, need, z]
    bad = lambda i, v: h.tamtr_hota_end_sequence(*(end[:i] + [v] + end[i + 1:]))     # noqa: E731
    assert bad(0, z) == -1 and bad(5, 0) == -1 and bad(6, holed) == -1 and bad(9, 16) == -1 and bad(5, 2000) == -2


def _state(nc=2, caps=(4, 8, 16, 32, 8), device='cpu'):
    from tamtr_amd import ops
    return {k: torch.zeros(shape(nc, caps), dtype=dt, device=device) for k, dt, shape in ops.HOTA_STATE_SPEC}


def test_ops_refuse_bad_arguments_and_cpu_tensors():
    from tamtr_amd import TamtrHipError, ops
    from tamtr_amd.track import HotaEvaluator
    with pytest.raises(TamtrHipError):
        HotaEvaluator('cpu', 2)
    caps = (4, 8, 16, 32, 8)
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)     # noqa: E731
    good = lambda: [torch.zeros(1, 8, 8), i32(1), torch.zeros(1, 8, 7), i32(1)]     # noqa: E731
    with pytest.raises(TamtrHipError, match='MI355X'):       # everything is right but the device
        ops.hota_update(*good(), _state(), 2, caps)
    with pytest.raises(TamtrHipError, match='MI355X'):
        ops.hota_end_sequence(_state(), 2, caps, 8, 8)
    for i, v, what in ((0, torch.zeros(1, 8, 6), 'tracks'), (2, torch.zeros(2, 8, 7), 'gt'), (1, i32(2), 'tcounts'), (3, torch.zeros(1), 'int32'),
                       (0, torch.zeros(1, 8, 8, dtype=torch.float64), 'float32')):
        a = good()
        a[i] = v
        with pytest.raises(TamtrHipError, match=what):
            ops.hota_update(*a, _state(), 2, caps)
    with pytest.raises(TamtrHipError, match='capacities'):
        ops.hota_update(*good(), _state(), 2, (4, 8, 0, 32, 8))
    with pytest.raises(TamtrHipError, match='capacities'):
        ops.hota_end_sequence(_state(), 2, caps[:4], 8, 8)
    with pytest.raises(TamtrHipError, match='iou'):
        ops.hota_update(*good(), _state(), 2, caps, iou=0.0)
    with pytest.raises(TamtrHipError, match='pkey'):         # a state built for other capacities
        ops.hota_update(*good(), _state(caps=(4, 8, 17, 32, 8)), 2, caps)
    st = _state()
    st['pkey'] = st['pkey'].to(torch.int32)
    with pytest.raises(TamtrHipError, match='pkey'):
        ops.hota_end_sequence(st, 2, caps, 8, 8)
    with pytest.raises(TamtrHipError, match='workgroups'):
        ops.hota_end_sequence(_state(), 2, caps, 8, 8, workgroups=0)
    with pytest.raises(TamtrHipError, match='outside'):
        ops.hota_workspace_bytes(4000, 4000, 4096)


def test_mot_eval_cli_host_path_with_hota_in_a_child_process(tmp_path):
    sequences = HC.HAND['alignment'][0] + HC.HAND['id_switch'][0]
    write_case(tmp_path, sequences)
    cmd = [sys.executable, os.path.join(ROOT, 'tools', 'mot_eval.py'), '--gt', str(tmp_path / 'gt'), '--results', str(tmp_path / 'res'),
           '--names', 'thing', '--host']
    plain = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    r = subprocess.run(cmd + ['--hota'], capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert r.returncode == 0 and plain.returncode == 0, r.stderr[-3000:]
    res, old = json.loads(r.stdout.strip().splitlines()[-1]), json.loads(plain.stdout.strip().splitlines()[-1])
    same = lambda d: json.dumps(d, sort_keys=True)     # noqa: E731  (nan compares equal as text)
    assert 'hota' not in old and 'HOTA' not in plain.stdout and same({k: v for k, v in res.items() if k != 'hota'}) == same(old)
    HC.check_expected(res['hota']['per_sequence']['seq0'], HC.HAND['alignment'][2], 'mot_eval --host --hota seq0')
    HC.check_expected(res['hota']['per_sequence']['seq1'], HC.HAND['id_switch'][2], 'mot_eval --host --hota seq1')
    assert res['hota']['overall']['all']['TP'] == [8] * 12 + [7] * 7 and res['hota']['overall']['per_class'][0]['class'] == 'thing'
