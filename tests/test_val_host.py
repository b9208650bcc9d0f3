"""CPU: the validator's rule restated in vectorised numpy (what the GPU suite, test_gpu_val.py, checks csrc/valmatch.hip against),
proved equal to engine.postprocess + engine.process_batch on CPU fp32; our tie rules pinned by hand; the argument checks of
tamtr_val_postprocess_match; DeviceValidator's reduce path."""
import ctypes
import itertools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

F = np.float32
IOUV = np.array([0.5, 0.55, 0.6, 0.65, 0.7, 0.75, 0.8, 0.85, 0.9, 0.95], dtype=np.float32)


# ------------------------------------------------------------------------------------------------ the restated rule
def group_labels(cls, bboxes, batch_idx, B):
    """Labels grouped by image with a stable sort (file order inside an image) -> lab_cls [M], lab_box [M, 4], lab_off [B + 1]."""
    bi = np.asarray(batch_idx, F).reshape(-1)
    order = np.argsort(bi, kind='stable')
    off = np.searchsorted(bi[order], np.arange(B + 1, dtype=F))
    order = order[off[0]:off[B]]
    return np.asarray(cls, F).reshape(-1)[order], np.asarray(bboxes, F).reshape(-1, 4)[order], (off - off[0]).astype(np.int32)


def pair_iou(a, b, eps):
    """[N, 4] x [M, 4] xyxy -> [N, M] in fp32: inter / (((area_a + area_b) - inter) + eps); eps None: no addition (the NMS form)."""
    w = np.maximum(F(0), np.minimum(a[:, None, 2], b[None, :, 2]) - np.maximum(a[:, None, 0], b[None, :, 0]))
    h = np.maximum(F(0), np.minimum(a[:, None, 3], b[None, :, 3]) - np.maximum(a[:, None, 1], b[None, :, 1]))
    inter = w * h
    union = ((a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1]))[:, None] + ((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]))[None, :] - inter
    with np.errstate(invalid='ignore', divide='ignore'):
        return inter / (union if eps is None else union + F(eps))


def val_rule(y, cls, bboxes, batch_idx, ori_hw, imgsz, conf, iou, single_cls=False, max_wh=7680, diag=None):
    """The rule of csrc/valmatch.hip in numpy fp32 -> predn f32 [B, nq, 6], correct u8 [B, nq, 10], counts i32 [B].
    diag (a dict): filled with the input conditions under which engine.Validator is DEFINED to give the same result -
    'equal_scores' (rows of one image with equal scores), 'nms_at_thr' (NMS IoUs equal to float32(iou)), 'iou_ties' (detections with
    two same-class labels at equal IoU >= 0.5)."""
    y = np.asarray(y, F)
    B, nq, _ = y.shape
    lab_cls, lab_box, lab_off = group_labels(cls, bboxes, batch_idx, B)
    predn, correct, counts = np.zeros((B, nq, 6), F), np.zeros((B, nq, 10), np.uint8), np.zeros(B, np.int32)
    if diag is not None:
        diag.update(equal_scores=0, nms_at_thr=0, iou_ties=0)
    at_thr = []
    for b in range(B):
        box = y[b, :, :4] * F(imgsz)
        half = box[:, 2:] / F(2)
        xyxy = np.concatenate([box[:, :2] - half, box[:, :2] + half], 1)
        sc = y[b, :, 4:]
        c = np.argmax(sc, 1)                                    # numpy's argmax: the first NaN, else the first maximum (torch.max)
        score = sc[np.arange(nq), c]
        order = np.argsort(-np.where(np.isnan(score), F(np.inf), score), kind='stable')      # descending, stable, NaN first
        rows = order[score > conf]                              # the UNSORTED mask on the SORTED rows
        sb = xyxy[rows] + (c[rows].astype(F) * F(0 if single_cls else max_wh))[:, None]
        m = pair_iou(sb, sb, None)
        sup = m.astype(np.float64) > iou                        # torchvision: float IoU against the double threshold
        alive, keep = np.ones(len(rows), bool), []
        for i in range(len(rows)):
            if alive[i]:
                keep.append(i)
                alive[i + 1:] &= ~sup[i, i + 1:]
        q = rows[np.asarray(keep, np.int64)]
        n = len(q)
        h0, w0 = (imgsz, imgsz) if ori_hw is None else ori_hw[b]
        s4 = np.array([F(w0 / imgsz), F(h0 / imgsz)] * 2, F)
        det = xyxy[q] * s4
        dcls = np.zeros(n, F) if single_cls else c[q].astype(F)
        predn[b, :n, :4], predn[b, :n, 4], predn[b, :n, 5], counts[b] = det, score[q], dcls, n
        lc, lb = lab_cls[lab_off[b]:lab_off[b + 1]], lab_box[lab_off[b]:lab_off[b + 1]]
        if diag is not None:
            diag['equal_scores'] += nq - len(np.unique(np.where(np.isnan(score), F(np.inf), score)))
            hit = np.nonzero(np.triu(m == F(iou), 1))[1]
            diag['nms_at_thr'] += len(hit)
            at_thr += [(b, int(j)) for j in rows[hit]]
        if n == 0 or len(lc) == 0:
            continue
        lh = lb[:, 2:] / F(2)
        tb = np.concatenate([lb[:, :2] - lh, lb[:, :2] + lh], 1) * np.array([F(w0), F(h0)] * 2, F)
        v = pair_iou(tb, det, 1e-7)                             # [labels, detections]
        with np.errstate(invalid='ignore'):
            v = np.where((lc[:, None] == dcls[None, :]) & (v >= F(0.5)), v, F(-1))
        bestl = np.argmax(v, 0)                                 # the first maximum: the LOWER label index among equal IoUs
        best = v[bestl, np.arange(n)]
        if diag is not None:
            diag['iou_ties'] += int((((v == best[None, :]) & (best[None, :] >= F(0.5))).sum(0) > 1).sum())
        for t, thr in enumerate(IOUV):
            ok = np.nonzero(best >= thr)[0]                     # ascending detection = descending confidence
            first = ok[np.unique(bestl[ok], return_index=True)[1]]   # each label goes to its first claimant
            correct[b, first, t] = 1
    if diag is not None:
        diag['_at_thr_rows'] = at_thr
    return predn, correct, counts


def settle_case(y, cls, bboxes, batch_idx, ori_hw, imgsz, conf, iou, single_cls=False, bf16=False):
    """Part of the generator: boxes on a coarse grid (bf16 inputs; any input after the shift by cls * 7680, whose fp32 spacing reaches
    1/16 px) give IoUs that are ratios of small integers, and some of them ARE float32(iou).  Widen the later box of every such pair
    by one step of its grid until no NMS IoU equals float32(iou).  Looks at the inputs only (val_rule's diag), never at the kernel."""
    for _ in range(50):
        diag = {}
        val_rule(y, cls, bboxes, batch_idx, ori_hw, imgsz, conf, iou, single_cls, diag=diag)
        rows = diag.pop('_at_thr_rows')
        if not rows:
            return diag
        for b, q in set(rows):
            w = y[b, q, 2:3].view(np.uint32)
            w += 0x10000 if bf16 else 0x40          # one bf16 step / 64 fp32 steps: scores and order are untouched
    raise AssertionError('generator: could not move the NMS IoUs off the threshold')


def engine_rule(y, cls, bboxes, batch_idx, ori_hw, imgsz, conf, iou, single_cls=False):
    """engine.postprocess + engine.process_batch exactly as engine.Validator.update strings them together, on CPU fp32, in the
    kernel's output form."""
    from tamtr_amd import engine as E
    y = torch.as_tensor(y).float().cpu()
    B, nq, _ = y.shape
    predn_o, correct_o, counts_o = torch.zeros(B, nq, 6), torch.zeros(B, nq, 10, dtype=torch.uint8), torch.zeros(B, dtype=torch.int32)
    cls, bboxes, batch_idx = torch.as_tensor(cls).float(), torch.as_tensor(bboxes).float(), torch.as_tensor(batch_idx).float()
    for si, pred in enumerate(E.postprocess(y, imgsz, conf, iou, single_cls)):
        idx = batch_idx.view(-1) == si
        c, bbox = cls.view(-1, 1)[idx], bboxes.view(-1, 4)[idx]
        shape = (imgsz, imgsz) if ori_hw is None else ori_hw[si]
        n = pred.shape[0]
        if n == 0:
            continue
        if single_cls:
            pred[:, 5] = 0
        predn = pred.clone()
        predn[..., [0, 2]] *= shape[1] / imgsz
        predn[..., [1, 3]] *= shape[0] / imgsz
        predn_o[si, :n], counts_o[si] = predn, n
        if c.shape[0]:
            tbox = E.xywh2xyxy(bbox)
            tbox[..., [0, 2]] *= shape[1]
            tbox[..., [1, 3]] *= shape[0]
            correct_o[si, :n] = E.process_batch(predn.float(), torch.cat((c, tbox), 1), E.IOUV).to(torch.uint8)
    return predn_o.numpy(), correct_o.numpy(), counts_o.numpy()


# ------------------------------------------------------------------------------------------------ inputs
def to_bf16_grid(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.bfloat16).float().numpy()


def make_case(B, nq, nc, labels_per_image, seed, bf16=False, shuffle_labels=False):
    """y [B, nq, 4 + nc] fp32 (every value on the bf16 grid when bf16) and host labels.  Detections cluster on the image's first
    labels (NMS suppresses, several detections claim one label); the row maxima are pairwise distinct inside an image by
    construction, also after rounding to bf16."""
    rng = np.random.default_rng(seed)
    cls, boxes, bidx = [], [], []
    y = np.zeros((B, nq, 4 + nc), F)
    for b in range(B):
        L = labels_per_image[b % len(labels_per_image)]
        lb = np.concatenate([rng.uniform(0.15, 0.85, (L, 2)), rng.uniform(0.04, 0.3, (L, 2))], 1).astype(F)
        lc = rng.integers(0, nc, L).astype(F)
        cls.append(lc), boxes.append(lb), bidx.append(np.full(L, b, F))
        if L:
            src = rng.integers(0, min(L, 24), nq)
            ctr, want = lb[src], lc[src].astype(np.int64)
        else:
            ctr = np.concatenate([rng.uniform(0.2, 0.8, (nq, 2)), rng.uniform(0.05, 0.3, (nq, 2))], 1).astype(F)
            want = rng.integers(0, nc, nq)
        y[b, :, :2] = ctr[:, :2] + rng.normal(0, 0.006, (nq, 2))
        y[b, :, 2:4] = ctr[:, 2:] * rng.uniform(0.85, 1.15, (nq, 2))
        if bf16:    # distinct values of the bf16 grid in [2^-9, 1)
            grid = (np.arange(0x3b00, 0x3f80, dtype=np.uint32) << 16).view(F)
            top = rng.choice(grid, nq, replace=False)
        else:
            top = (rng.permutation(nq) + rng.uniform(0.1, 0.9, nq)) / nq * 0.97 + 0.002
        wrong = rng.random(nq) < 0.2
        want = np.where(wrong, rng.integers(0, nc, nq), want)
        y[b, :, 4:] = top[:, None] * rng.uniform(0.05, 0.45, (nq, nc))
        y[b, np.arange(nq), 4 + want] = top
    y = to_bf16_grid(y) if bf16 else y
    cls, boxes, bidx = np.concatenate(cls), np.concatenate(boxes), np.concatenate(bidx)
    if shuffle_labels and len(cls):
        p = rng.permutation(len(cls))
        cls, boxes, bidx = cls[p], boxes[p], bidx[p]
    return y, torch.from_numpy(cls).view(-1, 1), torch.from_numpy(boxes), torch.from_numpy(bidx)


def orig_shapes(B, seed):
    rng = np.random.default_rng(seed + 7)
    return [(int(h), int(w)) for h, w in zip(rng.integers(200, 1500, B), rng.integers(200, 2000, B))]


def assert_conditions(diag):
    """Conditions on the INPUTS under which engine.Validator's result is defined (no unspecified sort order is exercised, and numpy's
    fp32 threshold equals torchvision's double one).  A violation is a bug of the generator."""
    assert {k: v for k, v in diag.items() if not k.startswith('_')} == {'equal_scores': 0, 'nms_at_thr': 0, 'iou_ties': 0}, diag


# ------------------------------------------------------------------------------------------------ tests of the rule
@pytest.mark.parametrize('conf,iou,single_cls,with_shape', list(itertools.product((0.001, 0.3), (0.45, 0.7), (False, True), (False, True))))
def test_restated_rule_equals_the_engine(conf, iou, single_cls, with_shape):
    total = matched = suppressed = 0
    for seed, (B, nq, nc, lpi) in enumerate([(3, 64, 10, (0, 1, 37)), (2, 300, 4, (60, 9)), (2, 100, 1, (5, 200))]):
        y, cls, boxes, bidx = make_case(B, nq, nc, lpi, seed, shuffle_labels=seed == 1)
        hw = orig_shapes(B, seed) if with_shape else None
        diag = {}
        got = val_rule(y, cls, boxes, bidx, hw, 160, conf, iou, single_cls, diag=diag)
        assert_conditions(diag)
        want = engine_rule(y, cls, boxes, bidx, hw, 160, conf, iou, single_cls)
        for g, w, what in zip(got, want, ('predn', 'correct', 'counts')):
            np.testing.assert_array_equal(g, w, err_msg=f'{what} seed {seed}')
        total += int(got[2].sum())
        matched += int(got[1].sum())
        suppressed += int(((y[:, :, 4:].max(-1) > conf).sum(1) - got[2]).sum())
    assert total > 0 and matched > 0 and suppressed > 0     # the cases exercise NMS and the matching


def test_confidence_quirk_bites_at_conf_03():
    """At conf 0.3 the unsorted mask keeps rows whose own score is below conf and drops rows above it."""
    y, cls, boxes, bidx = make_case(1, 64, 10, (5,), 3)
    predn, _, counts = val_rule(y, cls, boxes, bidx, None, 160, 0.3, 2.0)     # iou 2: nothing is suppressed
    kept = predn[0, :counts[0], 4]
    score = y[0, :, 4:].max(-1)
    assert counts[0] == (score > 0.3).sum() and (kept <= 0.3).any() and kept.min() < np.sort(score)[::-1][counts[0] - 1]


def test_engine_validator_stats_are_the_rule():
    """engine.Validator.update itself (not our re-stringing of its pieces) accumulates the rule's rows."""
    from tamtr_amd import engine as E
    y, cls, boxes, bidx = make_case(3, 64, 10, (0, 1, 37), 5)
    hw = orig_shapes(3, 5)
    v = E.Validator(160, 0.3, 0.7)
    v.update(torch.from_numpy(y), {'cls': cls, 'bboxes': boxes, 'batch_idx': bidx, 'ori_shape': hw})
    predn, correct, counts = val_rule(y, cls, boxes, bidx, hw, 160, 0.3, 0.7)
    live = np.arange(64)[None, :] < counts[:, None]
    np.testing.assert_array_equal(torch.cat([s[0] for s in v.stats]).numpy(), correct[live].astype(bool))
    np.testing.assert_array_equal(torch.cat([s[1] for s in v.stats]).numpy(), predn[live][:, 4])
    np.testing.assert_array_equal(torch.cat([s[2] for s in v.stats]).numpy(), predn[live][:, 5])


def tie_case():
    """One image, imgsz 100, native 100 x 100.  Queries 0 and 1: the same box and the same score (0.9, class 0), far apart from
    queries 2, 3 (class 1, scores 0.8 / 0.8, boxes shifted so that both overlap label 2 and do not suppress each other at iou 0.7).
    Labels 0 and 1 are duplicates of query 0's box (class 0); label 2 (class 1) lies between queries 2 and 3."""
    y = np.zeros((1, 4, 6), F)
    y[0, 0] = y[0, 1] = [0.25, 0.25, 0.2, 0.2, 0.9, 0.1]
    y[0, 2] = [0.70, 0.70, 0.2, 0.2, 0.1, 0.8]
    y[0, 3] = [0.72, 0.70, 0.2, 0.2, 0.1, 0.8]
    cls = torch.tensor([[0.], [0.], [1.]])
    boxes = torch.tensor([[0.25, 0.25, 0.2, 0.2], [0.25, 0.25, 0.2, 0.2], [0.71, 0.70, 0.2, 0.2]])
    return y, cls, boxes, torch.zeros(3)


def test_tie_rules_are_pinned_by_hand():
    y, cls, boxes, bidx = tie_case()
    diag = {}
    predn, correct, counts = val_rule(y, cls, boxes, bidx, None, 100, 0.001, 0.7, diag=diag)
    assert diag['equal_scores'] == 2 and diag['iou_ties'] == 1            # the inputs DO tie
    # equal scores keep ascending query order: query 0 first and query 1 (IoU 1 with it) suppressed; query 2 before query 3, which it
    # suppresses (2 px apart on 20 px boxes: IoU 18 / 22 = 0.818 > 0.7)
    assert counts.tolist() == [2]
    np.testing.assert_array_equal(predn[0, :2, 4:], np.array([[0.9, 0], [0.8, 1]], F))
    np.testing.assert_allclose(predn[0, :2, :4], [[15, 15, 35, 35], [60, 60, 80, 80]], rtol=0, atol=1e-4)
    # detection 0 has labels 0 and 1 at equal IoU 1: the lower index takes it; detection 1 matches label 2 (1 px apart) at IoU 19 / 21
    want = np.zeros((4, 10), np.uint8)
    want[0, :] = 1
    want[1, :9] = 1           # 0.905 >= 0.5 .. 0.9
    np.testing.assert_array_equal(correct[0], want)
    # at iou 0.85 query 3 survives NMS and claims label 2 as well (1 px to the other side): the earlier row of equal score keeps it
    predn, correct, counts = val_rule(y, cls, boxes, bidx, None, 100, 0.001, 0.85)
    assert counts.tolist() == [3] and predn[0, :3, 4].tolist() == [F(0.9), F(0.8), F(0.8)]
    assert predn[0, 1, 0] < predn[0, 2, 0]                                  # query 2 before query 3
    want[2, :] = 0
    np.testing.assert_array_equal(correct[0], want)
    # a second label of class 0 elsewhere does not let the suppressed duplicate in; swapping labels 0 and 1 changes nothing visible
    p2 = val_rule(y, cls[[1, 0, 2]], boxes[[1, 0, 2]], bidx, None, 100, 0.001, 0.85)
    np.testing.assert_array_equal(p2[1], correct)


def test_most_confident_claimant_wins_not_the_best_iou():
    y = np.zeros((1, 2, 5), F)
    y[0, 0] = [0.52, 0.5, 0.2, 0.2, 0.9]      # IoU 0.818 with the label, more confident
    y[0, 1] = [0.50, 0.5, 0.2, 0.2, 0.6]      # IoU 1 with the label
    _, correct, counts = val_rule(y, torch.zeros(1, 1), torch.tensor([[0.5, 0.5, 0.2, 0.2]]), torch.zeros(1), None, 100, 0.001, 0.9)
    assert counts.tolist() == [2]
    assert correct[0, 0].tolist() == [1] * 7 + [0] * 3 and correct[0, 1].tolist() == [0] * 7 + [1] * 3


def test_iouv_constants_are_torch_linspace():
    from tamtr_amd import engine as E
    np.testing.assert_array_equal(E.IOUV.numpy(), IOUV)


# ------------------------------------------------------------------------------------------------ the C ABI without a GPU
def _lib():
    import tamtr_amd
    from tamtr_amd import _lib
    if not os.path.exists(tamtr_amd.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


def test_abi_is_36_and_exports_the_symbol():
    from tamtr_amd import _lib as L
    h = _lib()
    assert L.ABI_VERSION == 36 and h.tamtr_abi_version() == 36
    assert 'tamtr_val_postprocess_match' in L.EXPORTS and hasattr(h, 'tamtr_val_postprocess_match')
    with open(os.path.join(ROOT, 'include', 'tamtr_hip.h')) as f:
        assert 'int tamtr_val_postprocess_match(' in f.read()


def test_val_postprocess_match_arguments_are_checked_before_any_launch():
    h = _lib()
    z, one = ctypes.c_void_p(0), ctypes.c_void_p(16)   # one: non-null, never dereferenced (the checks come first)
    f = h.tamtr_val_postprocess_match

    def call(preds=one, dtype=0, B=2, nq=300, nd=14, lab_cls=one, lab_box=one, lab_off=one, M=5, scale=one, predn=one, correct=one, counts=one):
        return f(preds, dtype, B, nq, nd, 640.0, 0.001, 0.7, 0, 7680.0, lab_cls, lab_box, lab_off, M, scale, predn, correct, counts, z)

    for k in ('preds', 'lab_off', 'scale', 'predn', 'correct', 'counts', 'lab_cls', 'lab_box'):
        assert call(**{k: z}) == -1, k
    assert call(nd=4) == -1 and call(B=0) == -1 and call(nq=0) == -1 and call(M=-1) == -1 and call(dtype=2) == -1
    assert call(nq=513) == -2 and call(nq=513, dtype=1) == -2
    assert call(nq=513, M=0, lab_cls=z, lab_box=z) == -2        # NULL label pointers are legal with M = 0: the next check answers
    assert call(nq=513, preds=z) == -1


def test_val_postprocess_match_refuses_cpu_tensors():
    import tamtr_amd.ops as ops
    from tamtr_amd import TamtrHipError
    with pytest.raises(TamtrHipError):
        ops.val_postprocess_match(torch.zeros(1, 300, 14), torch.zeros(0, 1), torch.zeros(0, 4), torch.zeros(0), None, 640, 0.001, 0.7)


def test_val_cli_help_runs_without_a_gpu():
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'val.py'), '--help'], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    for flag in ('--host-postprocess', '--save-json', '--project', '--name'):
        assert flag in r.stdout


# ------------------------------------------------------------------------------------------------ DeviceValidator's reduce path
def _fed_validators(save_json=False):
    """A DeviceValidator fed hand-made per-batch outputs (the restated rule's, as CPU tensors) and a Validator fed the same inputs."""
    from tamtr_amd import engine as E
    dv, hv = E.DeviceValidator(160, 0.001, 0.7, save_json=save_json, class_map=list(range(1, 11))), E.Validator(160, 0.001, 0.7)
    for k, B in enumerate((3, 3, 2)):       # a tail batch of another size
        y, cls, boxes, bidx = make_case(B, 64, 10, (0, 1, 37), 20 + k)
        hw = orig_shapes(B, k)
        predn, correct, counts = val_rule(y, cls, boxes, bidx, hw, 160, 0.001, 0.7)
        lab_cls, _, lab_off = group_labels(cls, boxes, bidx, B)
        dv.batches.append((torch.from_numpy(predn), torch.from_numpy(correct), torch.from_numpy(counts), lab_cls, lab_off))
        dv.seen += B
        dv.files.extend(f'/data/images/{k}_{i:03d}.jpg' for i in range(B))
        hv.update(torch.from_numpy(y), {'cls': cls, 'bboxes': boxes, 'batch_idx': bidx, 'ori_shape': hw})
    return dv, hv


def test_device_validator_reduce_equals_validator():
    dv, hv = _fed_validators()
    got, want = dv.results(), hv.results()
    per_class = got.pop('per_class')
    assert got == want and want['mAP50'] > 0
    tcls = np.concatenate([b[3] for b in dv.batches])
    assert [r['class'] for r in per_class] == sorted(set(tcls.astype(int).tolist()))
    assert sum(r['instances'] for r in per_class) == len(tcls)
    assert all(1 <= r['images'] <= min(r['instances'], dv.seen) for r in per_class)
    for key in ('precision', 'recall', 'mAP50', 'mAP50-95'):
        assert np.mean([r[key] for r in per_class]) == pytest.approx(want[key], rel=1e-12, abs=1e-15)


def test_device_validator_reduces_device_style_labels_and_the_matrix():
    """A batch whose labels are tensors - a slice lab_off[0] .. lab_off[B] of a larger upload, as the device path returns them - rides in
    the one copy with a confusion matrix set by hand, next to batches with host labels."""
    dv, hv = _fed_validators()
    B = 3
    y, cls, boxes, bidx = make_case(B, 64, 10, (5, 0, 12), 31)
    hw = orig_shapes(B, 31)
    predn, correct, counts = val_rule(y, cls, boxes, bidx, hw, 160, 0.001, 0.7)
    lab_cls, _, lab_off = group_labels(cls, boxes, bidx, B)
    big = np.concatenate([np.array([7, 7], F), lab_cls, np.array([3], F)])      # rows outside the slice belong to no image
    dv.batches.insert(1, (torch.from_numpy(predn), torch.from_numpy(correct), torch.from_numpy(counts), torch.from_numpy(big),
                          torch.from_numpy(lab_off + 2)))
    dv.seen += B
    hv.stats, hv.seen = [], 0
    for k, Bk in ((0, 3), (None, B), (1, 3), (2, 2)):      # the host validator sees the same batches in the same order
        if k is None:
            hv.update(torch.from_numpy(y), {'cls': cls, 'bboxes': boxes, 'batch_idx': bidx, 'ori_shape': hw})
        else:
            yk, ck, bk, ik = make_case(Bk, 64, 10, (0, 1, 37), 20 + k)
            hv.update(torch.from_numpy(yk), {'cls': ck, 'bboxes': bk, 'batch_idx': ik, 'ori_shape': orig_shapes(Bk, k)})
    matrix = torch.arange(121, dtype=torch.int32).reshape(11, 11)
    dv.confusion, dv._matrix = True, matrix.clone()
    got, want = dv.results(), hv.results()
    per_class = got.pop('per_class')
    assert got.pop('confusion_matrix') == matrix.tolist()
    assert got == want and want['mAP50'] > 0 and want['seen'] == 11
    tcls, timage = dv._reduce()[3:]
    assert len(tcls) == len(timage) == sum(r['instances'] for r in per_class) == 3 * 38 - 37 + 17
    assert np.array_equal(tcls[38:55], lab_cls) and np.array_equal(timage[38:55], 3 + np.repeat(np.arange(B), np.diff(lab_off)))


def test_device_validator_without_detections_or_labels():
    from tamtr_amd import engine as E
    dv = E.DeviceValidator(160)
    assert dv.results() == {**E.Validator(160).results(), 'per_class': []}
    dv.batches.append((torch.zeros(2, 8, 6), torch.zeros(2, 8, 10, dtype=torch.uint8), torch.zeros(2, dtype=torch.int32),
                       np.array([1, 1, 4], F), np.array([0, 3, 3], np.int32)))
    dv.seen = 2
    assert dv.results() == {'precision': 0.0, 'recall': 0.0, 'mAP50': 0.0, 'mAP50-95': 0.0, 'seen': 2, 'per_class': []}


def test_json_records_have_the_reference_format(tmp_path):
    dv, _ = _fed_validators(save_json=True)
    dv.results()
    path = dv.write_json(str(tmp_path))
    assert os.path.basename(path) == 'predictions.json'
    with open(path) as f:
        rows = json.load(f)
    counts = np.concatenate([b[2].numpy() for b in dv.batches])
    assert len(rows) == counts.sum() == len(dv.jdict)
    predn = np.concatenate([b[0].numpy()[np.arange(64)[None, :] < b[2].numpy()[:, None]] for b in dv.batches])
    stems = np.repeat([os.path.basename(f)[:-4] for f in dv.files], counts)
    for r, p, stem in zip(rows, predn.tolist(), stems):
        assert set(r) == {'image_id', 'category_id', 'bbox', 'score'}
        assert r['image_id'] == stem and r['category_id'] == int(p[5]) + 1 and r['score'] == round(p[4], 5)
        x1, y1, x2, y2 = p[:4]
        assert r['bbox'] == pytest.approx([x1, y1, x2 - x1, y2 - y1], abs=2e-3)
        assert all(round(x, 3) == x for x in r['bbox'])
