"""CPU: sliced prediction's host side (tam-tr_amd/slicing.py): the window grid, and the two rules the GPU suite (test_gpu_slice.py)
checks the kernels of csrc/slice.hip against - views_host and merge_host - on hand-made rows; the argument checks of tamtr_slice_views /
tamtr_slice_merge without a GPU."""
import ctypes

import numpy as np
import pytest
import torch

from test_gpu_predict import make_preds

HW = (100, 100)      # the hand-made rows live in a frame of 100 x 100 pixels
FULL = (0, 0, 100, 100)


def rows_of(*rows, nc=2):
    """[(cx, cy, w, h, score, cls)] -> one view's output [1, n, 4 + nc]."""
    y = torch.zeros(1, len(rows), 4 + nc)
    for k, (cx, cy, w, h, s, c) in enumerate(rows):
        y[0, k, :4] = torch.tensor([cx, cy, w, h])
        y[0, k, 4 + c] = s
    return y


def in_window(box, win, hw=HW):
    """A frame-normalised (cx, cy, w, h) box as the view of window `win` sees it (normalised to the window; exact for these numbers)."""
    x0, y0, x1, y1 = win
    cx, cy, w, h = box
    return ((cx * hw[1] - x0) / (x1 - x0), (cy * hw[0] - y0) / (y1 - y0), w * hw[1] / (x1 - x0), h * hw[0] / (y1 - y0))


# ------------------------------------------------------------------------------------------------ the grid
@pytest.mark.parametrize('h,w,sl,overlap', [(1500, 2000, 640, 0.2), (2160, 3840, 640, 0.2), (97, 131, 32, 0.25), (700, 300, (256, 128), 0.0),
                                            (640, 641, 640, 0.5), (100, 3000, 640, 0.2)])
def test_windows_cover_the_frame_and_overlap(h, w, sl, overlap):
    from tamtr_amd.slicing import check_slice, slice_windows
    sh, sw = check_slice(sl)
    wins = slice_windows(h, w, sl, overlap, full=False)
    assert wins.dtype == np.int32 and wins.shape[1] == 4
    covered = np.zeros((h, w), bool)
    for x0, y0, x1, y1 in wins.tolist():
        assert 0 <= x0 < x1 <= w and 0 <= y0 < y1 <= h
        assert (y1 - y0, x1 - x0) == (min(sh, h), min(sw, w))
        covered[y0:y1, x0:x1] = True
    assert covered.all()
    xs, ys = sorted(set(wins[:, 0].tolist())), sorted(set(wins[:, 1].tolist()))
    assert len(wins) == len(xs) * len(ys)      # a full grid
    assert all(a + min(sw, w) - b >= int(overlap * sw) for a, b in zip(xs, xs[1:]))
    assert all(a + min(sh, h) - b >= int(overlap * sh) for a, b in zip(ys, ys[1:]))
    full = slice_windows(h, w, sl, overlap, full=True)
    assert full[0].tolist() == [0, 0, w, h] and np.array_equal(full[1:], wins)


def test_the_issue_s_example_and_a_small_frame():
    from tamtr_amd.slicing import slice_windows
    wins = slice_windows(1500, 2000, 640, 0.2)
    assert len(wins) == 1 + 3 * 4 and wins[0].tolist() == [0, 0, 2000, 1500]
    assert sorted(set(wins[1:, 0].tolist())) == [0, 512, 1024, 1360] and sorted(set(wins[1:, 1].tolist())) == [0, 512, 860]
    assert wins[1:5, 1].tolist() == [0] * 4      # rows first
    for full in (True, False):      # a frame smaller than the slice, or equal to it: one view, never listed twice
        assert slice_windows(300, 500, 640, 0.2, full).tolist() == [[0, 0, 500, 300]]
        assert slice_windows(640, 640, 640, 0.2, full).tolist() == [[0, 0, 640, 640]]
    assert slice_windows(300, 1000, 640, 0.2).tolist() == [[0, 0, 1000, 300], [0, 0, 640, 300], [360, 0, 1000, 300]]
    assert len(slice_windows(2160, 3840, 640, 0.2)) == 1 + 4 * 8


def test_bad_grid_arguments_raise():
    from tamtr_amd.slicing import slice_windows
    for bad in ((0, 10, 4, 0.2), (10, -1, 4, 0.2), (10, 10, 0, 0.2), (10, 10, (4, 0), 0.2), (10, 10, 4, 1.0), (10, 10, 4, -0.1), (10, 10, None, 0.2),
                (10, 10, 2.5, 0.2)):
        with pytest.raises(ValueError):
            slice_windows(*bad)


# ------------------------------------------------------------------------------------------------ the view rule
def test_full_window_view_is_the_plain_predictors_input():
    from tamtr_amd.predict import letterbox_scalefill
    from tamtr_amd.slicing import views_host
    im = np.random.default_rng(1).integers(0, 256, (97, 131, 3), dtype=np.uint8)
    got = views_host(im, [(0, 0, 131, 97), (10, 20, 42, 52)], 32)
    assert got.shape == (2, 3, 32, 32) and got.dtype == torch.float32
    want = torch.from_numpy(letterbox_scalefill(im, 32)).permute(2, 0, 1).float() * torch.tensor(1 / 255, dtype=torch.float32)
    assert torch.equal(got[0], want)
    crop = torch.from_numpy(im[20:52, 10:42].copy()).permute(2, 0, 1).float() * torch.tensor(1 / 255, dtype=torch.float32)
    assert torch.equal(got[1], crop)      # a window already at imgsz is a copy
    assert float((got[0] * 255 - torch.from_numpy(letterbox_scalefill(im, 32)).permute(2, 0, 1)).abs().max()) < 1e-4      # it is `/ 255`


def test_view_factors_are_rounded_once_and_the_whole_frame_is_the_identity():
    from tamtr_amd.slicing import map_host, slice_view_factors
    f = slice_view_factors([(0, 0, 131, 97), (13, 7, 45, 39)], [0, 2], [(97, 131)])
    assert f.dtype == np.float32 and f[0].tolist() == [0.0, 0.0, 1.0, 1.0]
    assert f[1].tolist() == [float(np.float32(13 / 131)), float(np.float32(7 / 97)), float(np.float32(32 / 131)), float(np.float32(32 / 97))]
    y = torch.rand(1, 5, 7, generator=torch.Generator().manual_seed(2))
    assert torch.equal(map_host(y, [0, 1], [(0, 0, 131, 97)], [(97, 131)]), y)
    for bad_off in ([0, 1], [1, 2], [0, 0, 2]):
        with pytest.raises(Exception):
            slice_view_factors([(0, 0, 4, 4), (0, 0, 2, 2)], bad_off, [(4, 4)] * (len(bad_off) - 1))


# ------------------------------------------------------------------------------------------------ the merge rule on hand-made rows
def test_an_object_seen_by_two_windows_and_the_full_view_comes_out_once():
    from tamtr_amd.slicing import merge_host
    wins = [FULL, (0, 0, 64, 64), (36, 0, 100, 64)]
    obj = (0.5, 0.25, 0.125, 0.125)      # inside both windows: x 43.75 .. 56.25, y 18.75 .. 31.25
    y = torch.cat([rows_of((*obj, 0.6, 1), (0.9, 0.9, 0.05, 0.05, 0.5, 0)),      # the full view: the object, and something else
                   rows_of((*in_window(obj, wins[1]), 0.8, 1), (0.1, 0.1, 0.05, 0.05, 0.01, 0)),
                   rows_of((*in_window(obj, wins[2]), 0.7, 1), (0.1, 0.1, 0.05, 0.05, 0.01, 0))])
    ym, src, counts, dropped, overflow = merge_host(y, [0, 3], wins, [HW], 0.25, 0.7)
    assert counts.tolist() == [2] and dropped.tolist() == [0] and overflow.tolist() == [0]
    assert src[0, :3].tolist() == [2, 1, -1]      # the first window's row (the highest score), then the other object
    assert torch.allclose(ym[0, 0, :4], torch.tensor(obj), atol=1e-6) and ym[0, 0, 5] == 0.8 and not ym[0, 2:].any()
    assert ym.shape == (1, 512, 6) and src.dtype == counts.dtype == dropped.dtype == overflow.dtype == torch.int32


def test_a_truncated_box_survives_iou_and_is_removed_by_ios():
    from tamtr_amd.slicing import merge_host
    wins = [FULL, (0, 0, 64, 64)]
    whole = (0.64, 0.3, 0.4, 0.2)      # x 44 .. 84: the window ends at x = 64 and sees the left half, x 44 .. 64
    y = torch.cat([rows_of((*whole, 0.9, 0)), rows_of((*in_window((0.54, 0.3, 0.2, 0.2), wins[1]), 0.8, 0))])
    for match, kept in (('iou', [0, 1]), ('ios', [0])):      # IoU 0.5 <= 0.7; IoS 1 > 0.7
        ym, src, counts, _, _ = merge_host(y, [0, 2], wins, [HW], 0.25, 0.7, match=match)
        assert src[0, :counts[0]].tolist() == kept, match
    with pytest.raises(ValueError):
        merge_host(y, [0, 2], wins, [HW], 0.25, 0.7, match='giou')


def test_equal_scores_keep_the_lower_candidate_and_the_options_work():
    from tamtr_amd.slicing import merge_host
    wins = [FULL, FULL]
    a, b = (0.3, 0.3, 0.2, 0.2), (0.31, 0.3, 0.2, 0.2)      # IoU about 0.9
    y = torch.cat([rows_of((*b, 0.5, 0), (0.7, 0.7, 0.1, 0.1, 0.4, 1)), rows_of((*a, 0.5, 0), (*a, 0.45, 1))])
    ym, src, counts, _, _ = merge_host(y, [0, 2], wins, [HW], 0.25, 0.7)
    assert src[0, :counts[0]].tolist() == [0, 3, 1]      # 0 and 2 tie at 0.5: the lower stays; class 1 is not touched by class 0
    _, src, counts, _, _ = merge_host(y, [0, 2], wins, [HW], 0.25, 0.7, single_cls=True)
    assert src[0, :counts[0]].tolist() == [0, 1]      # class-agnostic: candidate 3 falls to candidate 0
    _, src, counts, _, _ = merge_host(y, [0, 2], wins, [HW], 0.25, 0.7, classes=[1])
    assert src[0, :counts[0]].tolist() == [3, 1]
    _, src, counts, _, _ = merge_host(y, [0, 2], wins, [HW], 0.25, 0.7, classes=[])
    assert counts.tolist() == [0] and (src == -1).all()
    # two frames: the second frame's candidates are numbered from its own first view
    _, src, counts, _, _ = merge_host(y, [0, 1, 2], wins, [HW, HW], 0.25, 0.7)
    assert counts.tolist() == [2, 2] and src[0, :2].tolist() == [0, 1] and src[1, :2].tolist() == [0, 1]


def test_max_out_sets_dropped_and_max_cand_sets_overflow():
    from tamtr_amd.slicing import merge_host
    rows = [(0.1 + 0.2 * k, 0.5, 0.05, 0.05, 0.3 + 0.1 * k, 0) for k in range(4)]      # four separate boxes, ascending scores
    y = torch.cat([rows_of(*rows[:2]), rows_of(*rows[2:])])
    ym, src, counts, dropped, overflow = merge_host(y, [0, 2], [FULL, FULL], [HW], 0.25, 0.7, max_out=3)
    assert counts.tolist() == [3] and dropped.tolist() == [1] and overflow.tolist() == [0] and src[0].tolist() == [3, 2, 1] and ym.shape == (1, 3, 6)
    ym, src, counts, dropped, overflow = merge_host(y, [0, 2], [FULL, FULL], [HW], 0.25, 0.7, max_cand=2)
    assert counts.tolist() == [2] and dropped.tolist() == [0] and overflow.tolist() == [2]
    assert src[0, :3].tolist() == [1, 0, -1]      # the two highest indices - the two best scores - were left out


def test_check_overflow_names_conf():
    from tamtr_amd.slicing import SliceOverflow, check_overflow
    check_overflow(np.zeros(3, np.int32), 0.25)
    with pytest.raises(SliceOverflow, match='conf'):
        check_overflow(np.array([0, 7], np.int32), 0.25)


@pytest.mark.parametrize('classes,single_cls', [(None, False), ([1, 3, 7], True)])
def test_one_whole_frame_view_per_image_is_the_tta_merge_of_the_identity_view(classes, single_cls):
    from tamtr_amd import slicing, tta
    y = make_preds(6, 60, 10, seed=5)
    hws = [(480 + 10 * b, 640 - 7 * b) for b in range(6)]
    wins = [(0, 0, w, h) for h, w in hws]
    got = slicing.merge_host(y, list(range(7)), wins, hws, 0.25, 0.7, classes, single_cls, max_out=4)
    want = tta.merge_host([y], [(1.0, 1.0, False)], 0.25, 0.7, classes, single_cls, max_out=4)
    assert int(want[2].sum()) > 8 and int(want[3].sum()) > 0 and got[4].tolist() == [0] * 6
    for g, w, name in zip(got, want, ('ym', 'src', 'counts', 'dropped')):
        assert g.dtype == w.dtype and torch.equal(g, w), name


# ------------------------------------------------------------------------------------------------ the C ABI without a GPU
def abi_argument_checks():
    """Every refusal comes before any launch: the non-null addresses are never dereferenced, the window and offset tables are host
    arrays."""
    from tamtr_amd import _lib
    h = _lib.lib()
    z, one = ctypes.c_void_p(0), ctypes.c_void_p(16)

    def views(wins, src=one, out=one, hh=97, ww=131, S=32, V=None):
        arr = (ctypes.c_int32 * (4 * len(wins)))(*[int(t) for w in wins for t in w])
        return h.tamtr_slice_views(src, hh, ww, ctypes.cast(arr, ctypes.c_void_p), len(wins) if V is None else V, S, out, z)

    ok = (0, 0, 131, 97)
    assert views([ok], src=z) == -1 and views([ok], out=z) == -1 and h.tamtr_slice_views(one, 97, 131, z, 1, 32, one, z) == -1
    assert views([ok], V=0) == -1 and views([ok], S=0) == -1 and views([ok], hh=0) == -1 and views([ok], ww=0) == -1
    for bad in ((0, 0, 132, 97), (0, 0, 131, 98), (-1, 0, 10, 10), (0, -1, 10, 10), (5, 0, 5, 10), (0, 9, 10, 9), (20, 0, 10, 10)):
        assert views([ok, bad]) == -1, bad
    assert views([ok] * 65) == -2 and views([ok], S=65536) == -2
    assert views([ok] * 64 + [(0, 0, 132, 97)]) == -1      # every window is checked, also beyond the table: invalid before unsupported

    def merge(off, y=one, N=None, nq=40, nd=7, views=one, match=0, dtype=0, max_out=8, outs=(one,) * 5, n_classes=0):
        arr = (ctypes.c_int32 * len(off))(*off)
        return h.tamtr_slice_merge(y, dtype, off[-1] if N is None else N, len(off) - 1, nq, nd, ctypes.cast(arr, ctypes.c_void_p), views, match, 0.25,
                                   0.7, 0, 7680.0, z, n_classes, max_out, *outs, z)

    assert merge([0, 1, 5], y=z) == -1 and merge([0, 1, 5], views=z) == -1
    for k in range(5):
        assert merge([0, 1, 5], outs=tuple(z if i == k else one for i in range(5))) == -1
    assert h.tamtr_slice_merge(one, 0, 5, 2, 40, 7, z, one, 0, 0.25, 0.7, 0, 7680.0, z, 0, 8, one, one, one, one, one, z) == -1
    assert merge([0, 1, 5], nd=4) == -1 and merge([0, 1, 5], nq=0) == -1 and merge([0, 1, 5], max_out=0) == -1 and merge([0, 1, 5], n_classes=-1) == -1
    assert merge([0, 1, 5], match=2) == -1 and merge([0, 1, 5], dtype=5) == -1
    assert merge([1, 2, 5]) == -1 and merge([0, 1, 5], N=6) == -1 and merge([0, 3, 3]) == -1 and merge([0, 4, 3, 5]) == -1
    assert merge([0, 1, 66]) == -2      # 65 views in one frame
    assert merge([0, 1, 5], nq=513) == -2 and merge([0, 1, 5], max_out=513) == -2 and merge(list(range(257))) == -2


def test_abi_argument_checks_without_a_gpu():
    abi_argument_checks()
