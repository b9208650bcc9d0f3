"""CPU: engine.ConfusionMatrix - the host statement of the rule of csrc/confusion.hip - against the reference's matrices (fixture
tests/golden/confusion.npz, tie-free inputs), hand-worked cases for the rule's quirks and this project's tie rules, a literal
sequential restatement of the reference on random tie-free images; the threshold rounding of ops.val_confusion, the argument checks
of tamtr_val_confusion, the host Validator's key and the CLI flag."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT

F = np.float32


def CM(*a, **k):
    from tamtr_amd import engine as E
    return E.ConfusionMatrix(*a, **k)


def det_rows(boxes, scores, classes):
    return torch.tensor([list(b) + [s, c] for b, s, c in zip(boxes, scores, classes)], dtype=torch.float32).reshape(-1, 6)


def lab_rows(classes, boxes):
    return torch.tensor([[c] + list(b) for c, b in zip(classes, boxes)], dtype=torch.float32).reshape(-1, 5)


# ------------------------------------------------------------------------------------------------ the reference's matrices
def test_engine_confusion_matrix_reproduces_every_reference_matrix():
    z = np.load(os.path.join(GOLDEN, 'confusion.npz'), allow_pickle=False)
    n, kinds, counted = int(z['n']), set(), 0
    assert n >= 30
    for k in range(n):
        cm = CM(int(z[f'nc{k}']), float(z[f'conf{k}']))
        lab = torch.from_numpy(z[f'lab{k}'])
        if f'det{k}' not in z:
            cm.process_batch(None, lab[:, 0])
        elif len(lab):                                   # the validator calls process_batch only inside `if nl:`
            cm.process_batch(torch.from_numpy(z[f'det{k}']), lab)
        assert cm.matrix.dtype == np.int64
        np.testing.assert_array_equal(cm.matrix, z[f'mx{k}'], err_msg=f'case {k} ({z[f"kind{k}"]}, nc {z[f"nc{k}"]})')
        kinds.add(str(z[f'kind{k}']).split()[0])
        counted += int(z[f'mx{k}'][:-1, :-1].sum())
    assert kinds == {'image', 'no', 'detections=None', 'conf'} and counted > 100
    assert {int(z[f'nc{k}']) for k in range(n)} == {1, 3, 10}


# ------------------------------------------------------------------------------------------------ hand-worked cases
A, B_, C = (0, 0, 10, 10), (100, 100, 110, 110), (200, 200, 210, 210)


def test_no_false_positives_without_a_match():
    """Three confident detections, none on the label: the label is a background miss and NO detection is counted (`if n:`)."""
    cm = CM(3)
    cm.process_batch(det_rows([B_, C, C], [0.9, 0.8, 0.7], [0, 1, 2]), lab_rows([2], [A]))
    want = np.zeros((4, 4), np.int64)
    want[3, 2] = 1
    np.testing.assert_array_equal(cm.matrix, want)
    # one match in the image switches the false positives on
    cm = CM(3)
    cm.process_batch(det_rows([A, C, C], [0.9, 0.8, 0.2], [1, 1, 2]), lab_rows([2, 0], [A, B_]))
    want = np.zeros((4, 4), np.int64)
    want[1, 2] = 1          # label 0 (class 2) matched by detection 0 (class 1): a cross-class match
    want[3, 0] = 1          # label 1 missed
    want[1, 3] = 1          # detection 1 passes the confidence and matches nothing; detection 2 (0.2) does not take part
    np.testing.assert_array_equal(cm.matrix, want)
    np.testing.assert_array_equal(cm.tp_fp()[0], [0, 0, 0])
    np.testing.assert_array_equal(cm.tp_fp()[1], [0, 2, 0])


def test_an_image_without_labels_counts_nothing_and_one_without_detections_counts_every_label():
    from tamtr_amd import engine as E
    nq, nc = 4, 3
    y = np.zeros((2, nq, 4 + nc), F)
    y[0, :, :4] = [0.5, 0.5, 0.2, 0.2]
    y[0, :, 4] = [0.9, 0.8, 0.7, 0.6]                       # image 0: confident detections, no labels
    y[1, :, :4] = [0.5, 0.5, 0.2, 0.2]                      # image 1: nothing above the validator's conf, three labels
    batch = {'cls': torch.tensor([[2.], [2.], [0.]]), 'bboxes': torch.tensor([[0.5, 0.5, 0.2, 0.2]] * 3), 'batch_idx': torch.tensor([1., 1., 1.])}
    v = E.Validator(100, 0.001, 0.7, confusion=True)
    v.update(torch.from_numpy(y), batch)
    want = np.zeros((4, 4), np.int64)
    want[3, 2], want[3, 0] = 2, 1
    res = v.results()
    assert res['confusion_matrix'] == want.tolist() and v.nc == 3 and res['seen'] == 2
    assert 'confusion_matrix' not in E.Validator(100).results()
    cm = CM(3)
    cm.process_batch(None, torch.tensor([2., 2., 0.]))
    np.testing.assert_array_equal(cm.matrix, want)


def test_both_tie_rules():
    # L: one detection, two identical labels of different classes -> the LOWER label index takes it
    cm = CM(3)
    cm.process_batch(det_rows([A], [0.9], [0]), lab_rows([1, 2], [A, A]))
    want = np.zeros((4, 4), np.int64)
    want[0, 1], want[3, 2] = 1, 1
    np.testing.assert_array_equal(cm.matrix, want)
    cm = CM(3)
    cm.process_batch(det_rows([A], [0.9], [0]), lab_rows([2, 1], [A, A]))
    np.testing.assert_array_equal(cm.matrix, want.T[[0, 2, 1, 3]][:, [0, 2, 1, 3]].T)      # classes 1 and 2 swapped
    # D: two identical detections of different classes on one label -> the LOWER row wins, the other is a false positive; the more
    # confident row does not win on confidence
    cm = CM(3)
    cm.process_batch(det_rows([A, A], [0.5, 0.9], [1, 2]), lab_rows([0], [A]))
    want = np.zeros((4, 4), np.int64)
    want[1, 0], want[2, 3] = 1, 1
    np.testing.assert_array_equal(cm.matrix, want)
    # without a tie the higher IoU wins whatever the row: detection 1 fits better
    cm = CM(3)
    cm.process_batch(det_rows([(0, 0, 10, 8), A], [0.9, 0.5], [1, 2]), lab_rows([0], [A]))
    want = np.zeros((4, 4), np.int64)
    want[2, 0], want[1, 3] = 1, 1
    np.testing.assert_array_equal(cm.matrix, want)


def test_a_detection_that_loses_its_label_does_not_fall_back_to_its_second_choice():
    """Detection 1's best label is 0, which detection 0 takes with a higher IoU; label 1, which detection 1 also overlaps above the
    threshold, stays unmatched (the reference's first np.unique keeps one label per detection)."""
    cm = CM(1)
    cm.process_batch(det_rows([A, (0, 1, 10, 10.5)], [0.9, 0.9], [0, 0]), lab_rows([0, 0], [A, (0, 2, 10, 12)]))
    from tamtr_amd import engine as E
    iou = E.box_iou(torch.tensor([A, (0, 2, 10, 12)], dtype=torch.float32), torch.tensor([(0, 1, 10, 10.5)], dtype=torch.float32))
    assert iou[0, 0] > iou[1, 0] > 0.45
    np.testing.assert_array_equal(cm.matrix, [[1, 1], [1, 0]])


def test_nan_boxes_never_match():
    nan = float('nan')
    cm = CM(2)
    cm.process_batch(det_rows([(nan, 0, 10, 10), A], [0.9, 0.9], [0, 1]), lab_rows([0, 1], [A, (0, 0, nan, 10)]))
    want = np.zeros((3, 3), np.int64)
    want[1, 0] = 1          # detection 1 takes label 0
    want[2, 1] = 1          # the NaN label is a miss
    want[0, 2] = 1          # the NaN detection is a false positive (the image has a match)
    np.testing.assert_array_equal(cm.matrix, want)
    cm = CM(2)
    cm.process_batch(det_rows([A], [nan], [0]), lab_rows([0], [A]))       # a NaN score fails `> conf`
    np.testing.assert_array_equal(cm.matrix, [[0, 0, 0], [0, 0, 0], [1, 0, 0]])


def test_classes_truncate_and_out_of_range_classes_are_counted_nowhere():
    cm = CM(2)
    cm.process_batch(det_rows([A, B_, C], [0.9, 0.9, 0.9], [1.9, 2.0, -0.5]),
                     lab_rows([0.7, 2.0, -1.0, float('nan'), 1.2], [A, B_, C, C, C]))
    # labels 1, 2, 3 (classes 2, -1, NaN) and detection 1 (class 2) are removed first and appear nowhere
    want = np.zeros((3, 3), np.int64)
    want[1, 0] = 1          # label 0 (0.7 -> 0) matched by detection 0 (1.9 -> 1)
    want[0, 1] = 1          # label 4 (1.2 -> 1) matched by detection 2 (-0.5 -> 0, as `.int()` truncates towards zero)
    np.testing.assert_array_equal(cm.matrix, want)
    cm = CM(2)
    cm.process_batch(None, torch.tensor([0.0, 1.99, 2.0, -1.0, float('inf')]))
    np.testing.assert_array_equal(cm.matrix[2], [1, 1, 0])


def test_cm_conf_default_rule():
    from tamtr_amd import engine as E
    assert CM(1, None).conf == 0.25 and CM(1, 0.001).conf == 0.25 and CM(1).conf == 0.25
    assert CM(1, 0.3).conf == 0.3 and CM(1, 0.0011).conf == 0.0011 and CM(1, 0.25, 0.6).iou_thres == 0.6
    assert E.cm_conf(None) == E.cm_conf(0.001) == 0.25 and E.cm_conf(0.5) == 0.5
    with pytest.raises(ValueError):
        CM(1, 0.25, -0.1)
    d, l = det_rows([A], [0.25], [0]), lab_rows([0], [A])
    cm = CM(1, 0.001)
    cm.process_batch(d, l)                       # 0.25 does not exceed 0.25
    np.testing.assert_array_equal(cm.matrix, [[0, 0], [1, 0]])
    cm = CM(1, 0.2)
    cm.process_batch(d, l)
    np.testing.assert_array_equal(cm.matrix, [[1, 0], [0, 0]])


def test_normalized_divides_columns():
    cm = CM(2)
    cm.matrix[:] = [[3, 0, 1], [1, 0, 0], [0, 0, 0]]
    n = cm.normalized()
    np.testing.assert_allclose(n, [[0.75, 0, 1], [0.25, 0, 0], [0, 0, 0]], rtol=1e-8)      # the 1e-9 in the divisor
    assert n[0, 0] == 3 / (4 + 1e-9) and n[0, 1] == 0.0


# ------------------------------------------------------------------------------------------------ thresholds at the fp32 boundary
@pytest.mark.parametrize('thr,lab,det', [(0.45, (0, 0, 20, 10), (0, 0, 9, 10)), (0.6, (0, 0, 50, 10), (0, 0, 30, 10))])
def test_an_iou_equal_to_the_fp32_threshold_is_not_a_candidate(thr, lab, det):
    """inter / union = 90 / 200 and 300 / 500 round to float32(0.45) and float32(0.6).  float32(0.45) < 0.45 < float32(0.6)... the second
    lies ABOVE 0.6 in double, yet torch compares an fp32 tensor with the fp32 nearest to the Python scalar, so neither pair qualifies;
    ops.val_confusion hands the kernel exactly that fp32."""
    from tamtr_amd import engine as E, ops
    iou = E.box_iou(torch.tensor([lab], dtype=torch.float32), torch.tensor([det], dtype=torch.float32))
    assert iou.dtype == torch.float32 and iou.item() == float(F(thr))
    assert not bool((iou > thr).item())
    assert ops._f32_nearest(thr) == float(F(thr))
    for x in (np.nextafter(F(thr), F(0)), F(thr), np.nextafter(F(thr), F(1))):
        assert bool((torch.tensor([x]) > thr).item()) == bool(x > F(ops._f32_nearest(thr)))      # the kernel's comparison
    cm = CM(1, 0.25, thr)
    cm.process_batch(det_rows([det], [0.9], [0]), lab_rows([0], [lab]))
    np.testing.assert_array_equal(cm.matrix, [[0, 0], [1, 0]])
    cm = CM(1, 0.25, float(np.nextafter(F(thr), F(0))))
    cm.process_batch(det_rows([det], [0.9], [0]), lab_rows([0], [lab]))
    np.testing.assert_array_equal(cm.matrix, [[1, 0], [0, 0]])
    for c in (0.25, 0.001, 0.6):
        for x in (np.nextafter(F(c), F(0)), F(c), np.nextafter(F(c), F(1))):
            assert bool((torch.tensor([x]) > c).item()) == bool(x > F(ops._f32_nearest(c)))


# ------------------------------------------------------------------------------------------------ the reference, literally
def random_image(rng, nc, nd, nl):
    """[nd, 6] and [nl, 5] fp32: detections mostly jittered copies of the first few labels, scores on both sides of 0.25."""
    def boxes(n):
        c, wh = rng.uniform(60, 580, (n, 2)), rng.uniform(24, 160, (n, 2))
        return np.concatenate([c - wh / 2, c + wh / 2], 1)
    lab, det = boxes(nl), boxes(nd)
    gc, dc = rng.integers(0, nc, nl), rng.integers(0, nc, nd)
    if nl and nd:
        src = rng.integers(0, min(nl, 6), nd)
        near = rng.random(nd) < 0.8
        det = np.where(near[:, None], lab[src] + rng.normal(0, 6, (nd, 4)), det)
        dc = np.where(near & (rng.random(nd) < 0.7), gc[src], dc)
    return (torch.from_numpy(np.concatenate([det, rng.uniform(0.03, 0.97, (nd, 1)), dc[:, None]], 1).astype(F)),
            torch.from_numpy(np.concatenate([gc[:, None], lab], 1).astype(F)))


def literal_reference(det, lab, nc, conf, thr):
    """ConfusionMatrix.process_batch (utils/metrics.py:849-877) step by step in Python loops: sort the candidate pairs by descending IoU,
    keep the first pair of every detection, then the first pair of every label; count labels, then - only if a pair is left - the
    detections.  Returns (matrix, tie_free)."""
    from tamtr_amd import engine as E
    m = np.zeros((nc + 1, nc + 1), np.int64)
    det = det[det[:, 4] > conf]
    iou = E.box_iou(lab[:, 1:], det[:, :4])
    pairs = [(float(iou[i, j]), i, j) for i in range(lab.shape[0]) for j in range(det.shape[0]) if bool(iou[i, j] > thr)]
    tie_free = len({p[0] for p in pairs}) == len(pairs)
    pairs.sort(key=lambda p: -p[0])
    per_det, seen = [], set()
    for p in pairs:
        if p[2] not in seen:
            seen.add(p[2])
            per_det.append(p)
    matches, seen = [], set()
    for p in per_det:
        if p[1] not in seen:
            seen.add(p[1])
            matches.append(p)
    for i in range(lab.shape[0]):
        mine = [p for p in matches if p[1] == i]
        if len(mine) == 1:
            m[int(det[mine[0][2], 5]), int(lab[i, 0])] += 1
        else:
            m[nc, int(lab[i, 0])] += 1
    if matches:
        for j in range(det.shape[0]):
            if not any(p[2] == j for p in matches):
                m[int(det[j, 5]), nc] += 1
    return m, tie_free


def test_vectorised_class_equals_the_literal_sequential_reference_on_random_images():
    rng = np.random.default_rng(2024)
    images = matched = fps = shared = 0
    for k in range(300):
        nc = (1, 3, 10)[k % 3]
        nd, nl = int(rng.integers(0, 41)), int(rng.integers(1, 61))
        conf, thr = ((0.25, 0.45), (0.5, 0.3), (0.1, 0.6))[(k // 3) % 3]
        det, lab = random_image(rng, nc, nd, nl)
        want, tie_free = literal_reference(det, lab, nc, conf, thr)
        assert tie_free                                # random fp32 IoUs: a tie would be a bug of the generator
        cm = CM(nc, conf, thr)
        cm.process_batch(det, lab)
        np.testing.assert_array_equal(cm.matrix, want, err_msg=f'image {k}')
        assert cm.matrix[:, :nc].sum() == nl           # every label is counted exactly once
        images += 1
        matched += int(want[:nc, :nc].sum())
        fps += int(want[:nc, nc].sum())
        shared += int(want[nc, :nc].sum() > 0 and want[:nc, nc].sum() > 0)
    assert images == 300 and matched > 1000 and fps > 500 and shared > 100


# ------------------------------------------------------------------------------------------------ the validator's flow, for the GPU suite
def confusion_rule(predn, counts, cls, bboxes, batch_idx, ori_hw, imgsz, nc, conf, iou_thres=0.45, matrix=None):
    """engine.ConfusionMatrix called as engine.Validator.update calls it, on the matching op's outputs (predn [B, nq, 6], counts [B])
    and the batch's labels -> the matrix after this batch, int64 [nc + 1, nc + 1].  matrix: an earlier ConfusionMatrix to go on with."""
    from tamtr_amd import engine as E
    cm = CM(nc, conf, iou_thres) if matrix is None else matrix
    predn, counts = torch.as_tensor(predn).float().cpu(), torch.as_tensor(counts).cpu()
    cls, bboxes, batch_idx = torch.as_tensor(cls).float().cpu(), torch.as_tensor(bboxes).float().cpu(), torch.as_tensor(batch_idx).float().cpu()
    for si in range(predn.shape[0]):
        idx = batch_idx.view(-1) == si
        c, bbox = cls.view(-1, 1)[idx], bboxes.view(-1, 4)[idx]
        shape = (imgsz, imgsz) if ori_hw is None else ori_hw[si]
        npr = int(counts[si])
        if npr == 0:
            if c.shape[0]:
                cm.process_batch(None, c.squeeze(-1))
            continue
        if c.shape[0]:
            tbox = E.xywh2xyxy(bbox)
            tbox[..., [0, 2]] *= shape[1]
            tbox[..., [1, 3]] *= shape[0]
            cm.process_batch(predn[si, :npr], torch.cat((c, tbox), 1))
    return cm


def test_validator_confusion_is_the_rule_applied_to_its_own_detections():
    from tamtr_amd import engine as E
    from test_val_host import make_case, orig_shapes, val_rule
    y, cls, boxes, bidx = make_case(3, 64, 10, (0, 9, 37), 5)
    y[2, :, 4:] *= F(2.0 ** -13)                        # image 2: nothing above the validator's conf, 37 labels
    hw = orig_shapes(3, 5)
    batch = {'cls': cls, 'bboxes': boxes, 'batch_idx': bidx, 'ori_shape': hw}
    v, plain = E.Validator(160, 0.001, 0.7, confusion=True), E.Validator(160, 0.001, 0.7)
    for _ in range(2):
        v.update(torch.from_numpy(y), batch)
        plain.update(torch.from_numpy(y), batch)
    predn, _, counts = val_rule(y, cls, boxes, bidx, hw, 160, 0.001, 0.7)
    want = confusion_rule(predn, counts, cls, boxes, bidx, hw, 160, 10, 0.001).matrix
    res = v.results()
    got = np.array(res.pop('confusion_matrix'))
    np.testing.assert_array_equal(got, 2 * want)
    assert got[10, :10].sum() >= 2 * 37 and got[:10, :10].sum() > 0 and got[:, :10].sum() == 2 * (9 + 37)
    assert res == plain.results()                       # nothing else moves
    assert all(isinstance(x, int) for row in v.results()['confusion_matrix'] for x in row)


# ------------------------------------------------------------------------------------------------ the C ABI without a GPU
def _lib():
    import tamtr_amd
    from tamtr_amd import _lib
    if not os.path.exists(tamtr_amd.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


def test_the_symbol_is_exported_and_the_abi_is_still_36():
    from tamtr_amd import _lib as L
    h = _lib()
    assert L.ABI_VERSION == 36 and h.tamtr_abi_version() == 36
    assert 'tamtr_val_confusion' in L.EXPORTS and hasattr(h, 'tamtr_val_confusion')
    with open(os.path.join(ROOT, 'include', 'tamtr_hip.h')) as f:
        assert 'int tamtr_val_confusion(' in f.read()


def test_val_confusion_arguments_are_checked_before_any_launch():
    h = _lib()
    z, one = ctypes.c_void_p(0), ctypes.c_void_p(16)   # one: non-null, never dereferenced (the checks come first)
    f = h.tamtr_val_confusion

    def call(predn=one, counts=one, B=2, nq=300, nc=10, lab_cls=one, lab_box=one, lab_off=one, M=5, scale=one, conf=0.25, thr=0.45, matrix=one):
        return f(predn, counts, B, nq, nc, lab_cls, lab_box, lab_off, M, scale, conf, thr, matrix, z)

    for k in ('predn', 'counts', 'lab_off', 'scale', 'matrix', 'lab_cls', 'lab_box'):
        assert call(**{k: z}) == -1, k
    assert call(B=0) == -1 and call(nq=0) == -1 and call(nc=0) == -1 and call(M=-1) == -1
    assert call(thr=-0.1) == -1 and call(thr=float('nan')) == -1
    assert call(nq=513) == -2
    assert call(nq=513, M=0, lab_cls=z, lab_box=z) == -2        # NULL label pointers are legal with M = 0: the next check answers
    assert call(nq=513, matrix=z) == -1


def test_val_confusion_refuses_cpu_tensors():
    import tamtr_amd.ops as ops
    from tamtr_amd import TamtrHipError
    labels = (torch.zeros(0), torch.zeros(0, 4), torch.zeros(2, dtype=torch.int32), torch.ones(1, 4))
    with pytest.raises(TamtrHipError):
        ops.val_confusion(torch.zeros(1, 5, 6), torch.zeros(1, dtype=torch.int32), labels, 3, 0.25, 0.45, torch.zeros(4, 4, dtype=torch.int32))


def test_val_cli_help_lists_the_flag():
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'val.py'), '--help'], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert '--confusion' in r.stdout


def test_cli_tables_have_names_and_background(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import val as V
    paths = V.write_confusion([[3, 0, 1], [1, 0, 0], [0, 2, 0]], ['car', 'van'], str(tmp_path))
    assert [os.path.basename(p) for p in paths] == ['confusion_matrix.csv', 'confusion_matrix_normalized.csv']
    rows = [line.split(',') for line in open(paths[0]).read().strip().splitlines()]
    assert rows[0][1:] == ['car', 'van', 'background'] and [r[0] for r in rows[1:]] == ['car', 'van', 'background']
    assert [[int(x) for x in r[1:]] for r in rows[1:]] == [[3, 0, 1], [1, 0, 0], [0, 2, 0]]
    norm = [[float(x) for x in line.split(',')[1:]] for line in open(paths[1]).read().strip().splitlines()[1:]]
    cm = CM(2)
    cm.matrix[:] = [[3, 0, 1], [1, 0, 0], [0, 2, 0]]
    np.testing.assert_allclose(norm, cm.normalized(), rtol=1e-12)
