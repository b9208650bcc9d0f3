"""Sliced prediction for large frames (drone imagery: frames of 2000 x 1500 to 4K, objects a few dozen pixels across): overlapping
windows are cut out of the full-resolution frame on the device and resized to the network's input (ops.slice_views, one launch per
frame), the model runs on every window and on the whole frame, every view's boxes are mapped back to the frame and merged by the
ordinary NMS rule (ops.slice_merge, one launch per batch) into an ordinary prediction tensor [B, max_out, 4 + nc] that
detect_postprocess consumes unchanged.  views_host and merge_host state the two rules on the CPU; the GPU suite checks the kernels of
csrc/slice.hip against them bit for bit.

The reference has no such mode: its predictor stretches the whole frame to imgsz (models/rtdetrworld/predict.py:80-92), which is what
the whole-frame view (view 0) still is.
"""
import numpy as np
import torch

from . import ops
from .ops import SLICE_MAX_CAND, SLICE_MAX_VIEWS, slice_view_factors
from .tta import _eval_forward, _event_marker, merge_images_host


# ------------------------------------------------------------------------------------------------ the grid
def check_slice(slice_hw):
    """None | int | (h, w) -> None | (h, w) as positive ints."""
    if slice_hw is None:
        return None
    try:
        sh, sw = (slice_hw, slice_hw) if isinstance(slice_hw, (int, float, np.integer)) else tuple(slice_hw)
    except (TypeError, ValueError):
        sh = sw = False
    if isinstance(sh, bool) or isinstance(sw, bool) or int(sh) != sh or int(sw) != sw or sh < 1 or sw < 1:
        raise ValueError(f'slice must be a positive int or (h, w) of positive ints, got {slice_hw!r}')
    return int(sh), int(sw)


def _axis_starts(n, size, overlap):
    """Window starts along an axis of n pixels -> (starts, window length): steps of size - int(overlap * size) until a window reaches
    the far edge; the window that would cross it is shifted back to end there.  An axis shorter than the window is spanned by one."""
    if n <= size:
        return [0], n
    step = size - int(overlap * size)
    starts, s = [], 0
    while s + size < n:
        starts.append(s)
        s += step
    starts.append(n - size)
    return starts, size


def slice_windows(h, w, slice_hw, overlap=0.2, full=True):
    """The usual sliced-inference grid over a frame of h x w pixels -> i32 numpy [V, 4], x0 y0 x1 y1 per window, rows first.  Windows
    are slice_hw = int | (h, w) large (the frame's extent on an axis where the frame is smaller) and neighbours overlap by at least
    int(overlap * slice).  full=True: the whole frame (0, 0, w, h) is view 0, and a grid window equal to it is not listed twice."""
    sl = check_slice(slice_hw)
    if sl is None or isinstance(h, bool) or isinstance(w, bool) or int(h) != h or int(w) != w or h < 1 or w < 1:
        raise ValueError(f'slice_windows needs a positive frame and slice size, got frame {(h, w)!r}, slice {slice_hw!r}')
    overlap = float(overlap)
    if not 0 <= overlap < 1:
        raise ValueError(f'overlap must lie in [0, 1), got {overlap!r}')
    h, w = int(h), int(w)
    ys, wh = _axis_starts(h, sl[0], overlap)
    xs, ww = _axis_starts(w, sl[1], overlap)
    whole = (0, 0, w, h)
    grid = [(x, y, x + ww, y + wh) for y in ys for x in xs]
    wins = ([whole] + [g for g in grid if g != whole]) if full else grid
    return np.asarray(wins, dtype=np.int32).reshape(-1, 4)


# ------------------------------------------------------------------------------------------------ the two rules on the host
def views_host(orig_u8, windows, imgsz):
    """Original RGB frame u8 [h, w, 3] (numpy) and windows [V, 4] -> f32 [V, 3, imgsz, imgsz]: predict.letterbox_scalefill
    (data.resize_linear_u8; a crop already at imgsz is taken as it is) and to_model_input (CHW, float, / 255) applied to every crop.
    `/ 255` is what torch makes of it on the device, where to_model_input runs: a multiplication by float(1 / 255) (division by a
    host scalar), so a view has the bits of the plain predictor's input."""
    from .predict import letterbox_scalefill
    crops = [letterbox_scalefill(np.ascontiguousarray(orig_u8[y0:y1, x0:x1]), imgsz) for x0, y0, x1, y1 in np.asarray(windows).reshape(-1, 4).tolist()]
    x = torch.from_numpy(np.stack(crops)).permute(0, 3, 1, 2).contiguous().float()
    return x * torch.tensor(1.0 / 255.0, dtype=torch.float32)


def map_host(y, view_off, windows, hws):
    """y [N, nq, 4 + nc] -> the same rows in fp32 with every view's boxes mapped to its frame: cx' = cx kx + ox, cy' = cy ky + oy,
    w' = w kx, h' = h ky, every operation rounded on its own (slice_view_factors gives ox oy kx ky)."""
    y = y.detach().cpu().float().clone()
    f = torch.from_numpy(slice_view_factors(windows, view_off, hws))[:, None, :]      # [N, 1, 4]
    y[..., 0] = y[..., 0] * f[..., 2] + f[..., 0]
    y[..., 1] = y[..., 1] * f[..., 3] + f[..., 1]
    y[..., 2] = y[..., 2] * f[..., 2]
    y[..., 3] = y[..., 3] * f[..., 3]
    return y


def merge_host(y, view_off, windows, hws, conf, iou, classes=None, single_cls=False, match='iou', max_out=512, max_cand=SLICE_MAX_CAND,
               max_wh=7680.):
    """The rule of ops.slice_merge on the CPU in fp32, with its arguments: frame b's candidates are the mapped rows of its views
    view_off[b] .. view_off[b + 1] - 1 in order (candidate i = v_local * nq + q); class max, `score > conf`, the class filter; the
    first max_cand passing candidates in ascending i go on and the others are counted in overflow; class-aware greedy NMS on `match`
    (equal scores: the lower candidate first), the first max_out survivors: map_host, then tta.merge_rows_host per frame.
    -> (ym [B, max_out, 4 + nc], src i32 [B, max_out], counts, dropped, overflow i32 [B])."""
    if match not in ops.SLICE_MATCH:
        raise ValueError(f"match must be 'iou' or 'ios', got {match!r}")
    y = torch.cat(list(y)) if isinstance(y, (list, tuple)) else y
    rows = map_host(y, view_off, windows, hws)
    off, nd = [int(o) for o in view_off], rows.shape[2]
    return merge_images_host([rows[a:b].reshape(-1, nd) for a, b in zip(off, off[1:])], nd, conf, iou, classes, single_cls, match, max_out,
                             max_cand, max_wh)


def check_overflow(overflow, conf):
    """Raise when a frame's passing candidates did not fit the merge's table (the counts are read by the caller, e.g. from the
    predictor's packed copy)."""
    over = np.asarray(overflow).reshape(-1).astype(np.int64)
    if over.any():
        which = ', '.join(f'frame {i}: {n}' for i, n in enumerate(over.tolist()) if n)
        raise SliceOverflow(f'candidates above conf were left out of the sliced merge ({which}): its table holds {SLICE_MAX_CAND} per frame; '
                            f'raise conf (now {conf}) or use fewer or larger slices')


class SliceOverflow(RuntimeError):
    pass


# ------------------------------------------------------------------------------------------------ the forward
@torch.no_grad()
def sliced_forward(model, origs_dev, windows_per_frame, imgsz, batch, txt_feats=None, conf=0.25, iou=0.7, classes=None, single_cls=False,
                   match='iou', max_out=512, autocast_dtype=None, keep=False, events=None):
    """origs_dev: B original frames u8 [h, w, 3] on the GPU (sizes may differ); windows_per_frame: B arrays [V_b, 4] (slice_windows)
    -> (ym, src, counts, dropped, overflow) of ops.slice_merge over the model's eval outputs on all N = sum V_b views.  One
    ops.slice_views launch per frame writes its views into one [N, 3, imgsz, imgsz] tensor; the views go through the model in chunks
    of at most `batch` (the forward shapes of plain prediction; the last chunk may be short; txt_feats [1, nc, d], when given, is
    expanded per chunk); one merge launch.  conf / iou / classes / single_cls are the ones the following postprocess uses.
    keep=True: -> (ym, src, counts, dropped, overflow, views [N, 3, imgsz, imgsz], raw outputs [N, nq, 4 + nc]).  events: a list that
    receives four CUDA events - before and after the view launches, before and after the merge.  Nothing synchronises."""
    wins = [np.asarray(w, dtype=np.int32).reshape(-1, 4) for w in windows_per_frame]
    if len(wins) != len(origs_dev) or not wins or any(not 1 <= len(w) <= SLICE_MAX_VIEWS for w in wins):
        raise ValueError(f'sliced_forward needs one window list of 1 .. {SLICE_MAX_VIEWS} windows per frame, got {[len(w) for w in wins]} for '
                         f'{len(origs_dev)} frames (use larger slices or less overlap)')
    off = np.concatenate([[0], np.cumsum([len(w) for w in wins])]).tolist()
    N, batch = off[-1], max(int(batch), 1)
    mark = _event_marker(events)
    mark()
    x = torch.empty(N, 3, imgsz, imgsz, device=origs_dev[0].device, dtype=torch.float32)
    for b, (o, w) in enumerate(zip(origs_dev, wins)):
        ops.slice_views(o, w, imgsz, out=x[off[b]:off[b + 1]])
    mark()
    ys = []
    for k in range(0, N, batch):
        xc = x[k:k + batch]
        ys.append(_eval_forward(model, xc, None if txt_feats is None else txt_feats.expand(len(xc), -1, -1), autocast_dtype))
    y = ys[0] if len(ys) == 1 else torch.cat(ys)
    mark()
    merged = ops.slice_merge(y, off, np.concatenate(wins), [tuple(o.shape[:2]) for o in origs_dev], conf, iou, classes, single_cls, match,
                             max_out=max_out)
    mark()
    return merged + (x, y) if keep else merged
