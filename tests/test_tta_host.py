"""CPU: test-time augmentation's host side (tam-tr_amd/tta.py, the two CLIs), the two rules the GPU suite (test_gpu_tta.py) checks
the kernels of csrc/tta.hip against, and the argument checks of tamtr_tta_view / tamtr_tta_merge without a GPU."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT
from test_gpu_predict import make_preds
from test_predict_host import reference_postprocess

SIZE = (256, 256)
VIEWS = ((1.0, False), (0.83, True), (0.67, False))


def view_outputs(B, V, nq, nc, seed, dtype=torch.float32):
    """V eval-output-like tensors [B, nq, 4 + nc]: make_preds' edge images, another draw per view."""
    return [make_preds(B, nq, nc, seed=seed + 31 * v).to(dtype) for v in range(V)]


def assert_merge_then_postprocess_is_postprocess_of_the_concatenation(ys, views, size, conf, iou, classes=None, single_cls=False, max_out=512):
    """The claim the design rests on, exact in rows, counts and order; -> (merge_host's outputs, the concatenation's postprocess)."""
    from tamtr_amd import tta
    ym, src, counts, dropped = tta.merge_host(ys, views, conf, iou, classes, single_cls, max_out=max_out, size=size)
    assert dropped.tolist() == [0] * len(dropped), 'a condition of the test: max_out holds every survivor'
    cat = tta.deaugment_host(ys, tta.tta_view_factors(views, size) if size is not None else views)
    hw = [(480 + 10 * b, 640 - 7 * b) for b in range(len(ym))]
    mo, mk, mc = reference_postprocess(ym, hw, conf, iou, classes, single_cls)
    co, ck, cc = reference_postprocess(cat, hw, conf, iou, classes, single_cls)
    assert torch.equal(mc, cc) and torch.equal(mc, counts)
    for b, n in enumerate(cc.tolist()):
        assert torch.equal(mo[b, :n], co[b, :n]), f'image {b}: rows'
        assert mk[b, :n].tolist() == list(range(n)), f'image {b}: the merged rows are already in NMS order and all survive'
        assert torch.equal(src[b, :n], ck[b, :n]), f'image {b}: source candidates'
        assert torch.equal(ym[b, :n], cat[b, ck[b, :n].long()]) and not ym[b, n:].any() and (src[b, n:] == -1).all()
    return (ym, src, counts, dropped), (co, ck, cc)


# ------------------------------------------------------------------------------------------------ the view rule
@pytest.mark.parametrize('ratio,flip', [(0.83, True), (0.67, False)])
def test_view_host_is_flip_interpolate_pad(ratio, flip):
    from tamtr_amd import tta
    x = torch.rand(2, 3, 128, 128, generator=torch.Generator().manual_seed(1))
    got = tta.view_host(x, ratio, flip)
    sh, sw = int(128 * ratio), int(128 * ratio)
    want = F.pad(F.interpolate(x.flip(3) if flip else x, size=(sh, sw), mode='bilinear', align_corners=False), [0, 128 - sw, 0, 128 - sh],
                 value=0.447)
    assert got.shape == (2, 3, 128, 128) and torch.equal(got, want)
    assert (got[:, :, sh:] == torch.tensor(0.447)).all() and (got[:, :, :, sw:] == torch.tensor(0.447)).all()


def test_canvas_sizes_follow_scale_img():
    from tamtr_amd import tta
    assert [tta.tta_view_sizes(128, 128, r, 64)[1] for r in (1.0, 0.83, 0.67)] == [(128, 128)] * 3
    assert [tta.tta_view_sizes(256, 256, r, 64)[1] for r in (1.0, 0.83, 0.67)] == [(256, 256), (256, 256), (192, 192)]
    assert tta.tta_view_sizes(256, 256, 0.83, 64)[0] == (212, 212) and tta.tta_view_sizes(96, 160, 0.75, 64) == ((72, 120), (128, 128))
    assert tta.tta_view_sizes(640, 640, 0.67, 32)[1] == (448, 448)      # the reference's canvas at its stride
    assert tta.view_host(torch.zeros(1, 3, 256, 256), 0.67, False).shape == (1, 3, 192, 192)
    assert tta.GS == 64 and tta.DEFAULT_VIEWS == VIEWS


def test_view_factors_of_ratio_one_are_exactly_one():
    from tamtr_amd import tta
    for size in ((128, 128), (256, 256), (640, 640), (192, 320)):
        assert tta.tta_view_factors([(1.0, False), (1.0, True)], size) == [(1.0, 1.0, False), (1.0, 1.0, True)]
    (kx, ky, flip), = tta.tta_view_factors([(0.67, True)], (256, 256))
    assert flip and kx == ky == float(torch.tensor(192 / (0.67 * 256), dtype=torch.float64).float())
    y = torch.rand(1, 5, 7, generator=torch.Generator().manual_seed(2))
    assert torch.equal(tta.deaugment_host([y], [(1.0, 1.0, False)]), y)      # view 0 passes through bit for bit


def test_views_are_checked():
    from tamtr_amd import tta
    assert tta.views_from_cli(None, None) is None
    assert tta.views_from_cli([1, 0.5], [0, 1]) == ((1.0, False), (0.5, True)) and tta.views_from_cli([1, 0.5], None) == ((1.0, False), (0.5, False))
    for bad in ((), ((0.0, False),), ((-1.0, True),)):
        with pytest.raises(ValueError):
            tta.check_views(bad)
    with pytest.raises(ValueError):
        tta.views_from_cli([1, 0.5], [0])


# ------------------------------------------------------------------------------------------------ the merge rule
def test_merge_then_postprocess_equals_postprocess_of_the_concatenation():
    ys = view_outputs(6, 3, 300, 10, seed=3)      # every edge image of make_preds: ties, a NaN score, nothing above conf, one box
    assert ys[0][2].isnan().any()
    for conf, iou in ((0.25, 0.7), (0.4, 0.45)):
        # max_out: 900 holds whatever survives; 512, the kernel's, holds the second case (the zero-width boxes of image 2 never suppress)
        (_, _, counts, _), _ = assert_merge_then_postprocess_is_postprocess_of_the_concatenation(ys, VIEWS, SIZE, conf, iou,
                                                                                                 max_out=900 if conf == 0.25 else 512)
        assert counts[3] == 0 and counts.sum() > 20


def test_merge_with_a_class_filter_and_single_cls():
    ys = view_outputs(3, 3, 300, 10, seed=5)
    (_, _, counts, _), (co, _, _) = assert_merge_then_postprocess_is_postprocess_of_the_concatenation(ys, VIEWS, SIZE, 0.25, 0.6, classes=[1, 3, 7],
                                                                                                     single_cls=True)
    assert counts.sum() > 0 and set(co[..., 5].unique().tolist()) <= {0.0, 1.0, 3.0, 7.0}


def test_identical_rows_in_two_views_tie_by_candidate_index():
    """Identity views (the Ensemble merge): a row and its copy in the next view have IoU 1 and equal scores; the lower candidate stays."""
    y = make_preds(2, 37, 4, seed=9)
    views = [(1.0, 1.0, False)] * 3
    ys = [y, y.clone(), make_preds(2, 37, 4, seed=10)]
    (ym, src, counts, _), _ = assert_merge_then_postprocess_is_postprocess_of_the_concatenation(ys, views, None, 0.1, 0.7)
    for b in range(2):
        s = src[b, :counts[b]]
        assert counts[b] > 0 and not ((s >= 37) & (s < 74)).any()      # no survivor comes from the copy


def test_merge_with_max_out_16_reports_what_it_dropped():
    from tamtr_amd import tta
    ys = view_outputs(3, 3, 300, 10, seed=3)
    ym, src, counts, dropped = tta.merge_host(ys, VIEWS, 0.25, 0.7, max_out=16, size=SIZE)
    cat = tta.deaugment_host(ys, tta.tta_view_factors(VIEWS, SIZE))
    _, ck, cc = reference_postprocess(cat, [(1, 1)] * 3, 0.25, 0.7)
    assert (cc > 16).all(), 'a condition of the test: every image overflows'
    assert torch.equal(dropped, cc - 16) and counts.tolist() == [16] * 3 and ym.shape == (3, 16, 14)
    for b in range(3):
        assert torch.equal(src[b], ck[b, :16]) and torch.equal(ym[b], cat[b, ck[b, :16].long()])      # the 16 top-scoring survivors


# ------------------------------------------------------------------------------------------------ the C ABI without a GPU
def _lib():
    import tamtr_amd
    from tamtr_amd import _lib
    if not os.path.exists(tamtr_amd.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


def test_symbols_are_exported_and_declared_and_the_abi_version_stays():
    from tamtr_amd import _lib as L
    h = _lib()
    header = open(os.path.join(ROOT, 'include', 'tamtr_hip.h')).read()
    for name in ('tamtr_tta_view', 'tamtr_tta_merge'):
        assert name in L.EXPORTS and hasattr(h, name) and f'int {name}(' in header
    assert h.tamtr_abi_version() == 36 == L.ABI_VERSION


def test_merge_arguments_are_checked_before_any_launch():
    h = _lib()
    z, one = ctypes.c_void_p(0), ctypes.c_void_p(16)      # one: non-null, never dereferenced (the checks come first)
    f = h.tamtr_tta_merge

    def call(V=3, dtype=0, B=2, nq=300, nd=14, views=one, classes=z, n_classes=0, max_out=512, ym=one, src=one, counts=one, dropped=one,
             ys='all', null_view=None):
        arr = (ctypes.c_void_p * max(V, 1))(*[0 if v == null_view else 16 for v in range(max(V, 1))])
        ys = ctypes.cast(arr, ctypes.c_void_p) if ys == 'all' else ys
        return f(ys, V, dtype, B, nq, nd, views, 0.25, 0.7, 0, 7680.0, classes, n_classes, max_out, ym, src, counts, dropped, z)

    for k in ('views', 'ym', 'src', 'counts', 'dropped', 'ys'):
        assert call(**{k: z}) == -1, k
    assert call(null_view=1) == -1
    assert call(V=0) == -1 and call(V=-1) == -1 and call(nd=4) == -1 and call(B=0) == -1 and call(nq=0) == -1
    assert call(n_classes=-1) == -1 and call(dtype=2) == -1 and call(max_out=0) == -1
    assert call(max_out=513) == -2 and call(V=4, nq=513) == -2 and call(V=1, nq=2049) == -2 and call(V=7, nq=300, dtype=1) == -2
    assert call(V=17, nq=2) == -2      # the pointer table of a launch holds 16 views
    assert call(max_out=513, ym=z) == -1


def test_view_arguments_are_checked_before_any_launch():
    h = _lib()
    z, one = ctypes.c_void_p(0), ctypes.c_void_p(16)
    f = h.tamtr_tta_view

    def call(x=one, out=one, B=2, H=128, W=128, sh=106, sw=106, Hp=128, Wp=128, flip=1):
        return f(x, out, B, H, W, sh, sw, Hp, Wp, flip, z)

    assert call(x=z) == -1 and call(out=z) == -1
    assert call(B=0) == -1 and call(H=0) == -1 and call(W=0) == -1 and call(sh=0) == -1 and call(sw=0) == -1
    assert call(Hp=105) == -1 and call(Wp=105) == -1 and call(flip=2) == -1 and call(flip=-1) == -1
    assert call(B=65536) == -2 and call(Hp=65536) == -2 and call(B=65536, x=z) == -1


def test_ops_refuse_cpu_tensors_and_bad_arguments():
    import tamtr_amd.ops as ops
    from tamtr_amd import TamtrHipError
    with pytest.raises(TamtrHipError):
        ops.tta_view(torch.zeros(1, 3, 64, 64), 0.83, True)
    with pytest.raises(TamtrHipError):
        ops.tta_merge([torch.zeros(1, 300, 14)] * 3, VIEWS, 0.25, 0.7, size=SIZE)
    with pytest.raises(TamtrHipError):
        ops.tta_merge([], VIEWS, 0.25, 0.7, size=SIZE)
    with pytest.raises(TamtrHipError):
        ops.tta_view_sizes(128, 128, 0.0)


# ------------------------------------------------------------------------------------------------ the CLIs
@pytest.mark.parametrize('tool', ['predict.py', 'val.py'])
def test_cli_help_lists_augment_without_a_gpu(tool):
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', tool), '--help'], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    for flag in ('--augment', '--tta-scales', '--tta-flips'):
        assert flag in r.stdout
