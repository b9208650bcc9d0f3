"""Test-time augmentation for predict and validate (the reference's `augment`: DetectionModel._predict_augment, nn/tasks.py:272-295):
the model runs on a few scaled / mirrored views of the batch (ops.tta_view, one launch per view), every view's boxes are brought back
to the input's frame and the views are merged by the ordinary NMS rule (ops.tta_merge, one launch per batch) into an ordinary
prediction tensor [B, max_out, 4 + nc] that detect_postprocess, val_postprocess_match, the confusion matrix, COCO and save_json
consume unchanged.  view_host and merge_host state the two rules in torch on the CPU; the GPU suite checks the kernels against them.

_clip_augmented (tasks.py:297-306) cuts the tails of YOLO's anchor layers and has no counterpart for a query decoder.
"""
import torch
import torch.nn.functional as F

from . import ops
from .ops import tta_view_factors, tta_view_sizes

DEFAULT_VIEWS = ((1.0, False), (0.83, True), (0.67, False))      # the reference's scales and flips (tasks.py:275-276)
GS = 64      # not the stride 32: cpam.hip rejects odd maps, as the reference's CPAM does, so every level must stay even
PAD_VALUE = 0.447      # scale_img's (imagenet mean)


def check_views(views):
    """-> ((ratio, flip), ...) as floats and bools; at least one view, every ratio positive."""
    views = tuple((float(r), bool(f)) for r, f in views)
    if not views or any(not r > 0 for r, _ in views):
        raise ValueError(f'tta views must be a non-empty sequence of (ratio > 0, flip), got {views!r}')
    return views


def views_from_cli(scales, flips):
    """--tta-scales / --tta-flips -> views; None for both keeps the defaults."""
    if scales is None and flips is None:
        return None
    scales = [r for r, _ in DEFAULT_VIEWS] if scales is None else list(scales)
    flips = [0] * len(scales) if flips is None else list(flips)
    if len(scales) != len(flips):
        raise ValueError(f'--tta-scales has {len(scales)} entries and --tta-flips has {len(flips)}')
    return check_views(zip(scales, flips))


# ------------------------------------------------------------------------------------------------ the two rules on the host
def view_host(x, ratio, flip, gs=GS):
    """scale_img(x.flip(3) if flip else x, ratio, gs) (utils/torch_utils.py:316-327) with the canvas of tta_view_sizes: flip,
    F.interpolate (bilinear, align_corners=False), F.pad with 0.447.  Ratio 1 is not resampled."""
    (sh, sw), (Hp, Wp) = tta_view_sizes(x.shape[2], x.shape[3], ratio, gs)
    x = x.flip(3) if flip else x
    if (sh, sw) != tuple(x.shape[2:]):
        x = F.interpolate(x, size=(sh, sw), mode='bilinear', align_corners=False)
    return F.pad(x, [0, Wp - sw, 0, Hp - sh], value=PAD_VALUE)


def deaugment_host(ys, table):
    """V outputs [B, nq, 4 + nc] and [(kx, ky, flip)] -> the concatenation [B, V * nq, 4 + nc] of the de-augmented rows in fp32:
    cx' = cx kx, then 1 - cx' when flip; cy' = cy ky; w' = w kx; h' = h ky (descale, then de-flip: _descale_pred, tasks.py:286-295)."""
    rows = []
    for y, (kx, ky, flip) in zip(ys, table):
        y = y.detach().cpu().float().clone()
        kx, ky = torch.tensor(kx, dtype=torch.float32), torch.tensor(ky, dtype=torch.float32)
        y[..., 0] = y[..., 0] * kx
        if flip:
            y[..., 0] = 1 - y[..., 0]
        y[..., 1] = y[..., 1] * ky
        y[..., 2] = y[..., 2] * kx
        y[..., 3] = y[..., 3] * ky
        rows.append(y)
    return torch.cat(rows, 1)


def nms_host(boxes, scores, thr, match='iou'):
    """torchvision.ops.nms as its CPU kernel computes it (fp32, no eps, the fp32 overlap compared with the double threshold), the scores
    sorted descending and stable, with the overlap of `match`: 'iou', or 'ios' = inter / min(area_i, area_j) -> indices into boxes, in
    keep order."""
    order = scores.sort(descending=True, stable=True).indices
    x1, y1, x2, y2 = boxes[order].unbind(1)
    areas = (x2 - x1) * (y2 - y1)
    n = len(order)
    later = torch.arange(n)
    suppressed = torch.zeros(n, dtype=torch.bool)
    zero = torch.zeros((), dtype=torch.float32)
    keep = []
    for i in range(n):
        if suppressed[i]:
            continue
        keep.append(i)
        xx1 = torch.where(x1[i] < x1, x1, x1[i])      # std::max(ix1, x1[j])
        yy1 = torch.where(y1[i] < y1, y1, y1[i])
        xx2 = torch.where(x2 < x2[i], x2, x2[i])      # std::min(ix2, x2[j])
        yy2 = torch.where(y2 < y2[i], y2, y2[i])
        dx, dy = xx2 - xx1, yy2 - yy1
        inter = torch.where(zero < dx, dx, zero) * torch.where(zero < dy, dy, zero)
        if match == 'iou':
            ovr = inter / ((areas[i] + areas) - inter)
        else:
            ovr = inter / torch.where(areas < areas[i], areas, areas[i])      # std::min(area_i, area_j)
        suppressed |= (ovr.double() > thr) & (later > i)
    return order[torch.as_tensor(keep, dtype=torch.long)]


_nms_host = nms_host


def merge_rows_host(cat, conf, iou, classes, single_cls, match, max_out, max_cand, max_wh):
    """The merge rule of ops.tta_merge and ops.slice_merge for ONE image: cat [N, 4 + nc], its candidates' de-augmented / mapped rows in
    fp32 -> class max, `score > conf`, the class filter; the first max_cand passing candidates in ascending order go on (None: all);
    class-aware greedy NMS on `match` (equal scores: the lower candidate first); the first max_out survivors.
    -> (their rows, their candidates i32, their number, the survivors that did not fit, the passing candidates beyond max_cand)."""
    bbox, scores = cat[:, :4], cat[:, 4:]
    dw, dh = bbox[:, 2] / 2, bbox[:, 3] / 2
    xyxy = torch.stack([bbox[:, 0] - dw, bbox[:, 1] - dh, bbox[:, 0] + dw, bbox[:, 1] + dh], 1)
    score, cls = scores.max(-1)
    ok = score > conf
    if classes is not None:
        ok = (cls[:, None] == torch.as_tensor(classes, dtype=torch.long).reshape(-1)).any(1) & ok
    cand = ok.nonzero().view(-1)
    overflow = 0 if max_cand is None else max(len(cand) - max_cand, 0)
    cand = cand[:max_cand]
    shifted = xyxy[cand] + cls[cand, None].float() * (0 if single_cls else max_wh)
    kept = cand[nms_host(shifted, score[cand], iou, match)]
    n = min(len(kept), max_out)
    return cat[kept[:n]], kept[:n].to(torch.int32), n, len(kept) - n, overflow


def merge_images_host(images, nd, conf, iou, classes, single_cls, match, max_out, max_cand, max_wh):
    """merge_rows_host over the images' rows [N_b, nd], padded as the kernels pad: -> (ym [B, max_out, nd] with zero rows after the
    count, src i32 [B, max_out] with -1 after it, counts, dropped, overflow i32 [B])."""
    B = len(images)
    ym = torch.zeros(B, max_out, nd)
    src = torch.full((B, max_out), -1, dtype=torch.int32)
    counts, dropped, overflow = (torch.zeros(B, dtype=torch.int32) for _ in range(3))
    for b, cat in enumerate(images):
        rows, cand, n, dropped[b], overflow[b] = merge_rows_host(cat, conf, iou, classes, single_cls, match, max_out, max_cand, max_wh)
        ym[b, :n], src[b, :n], counts[b] = rows, cand, n
    return ym, src, counts, dropped, overflow


def merge_host(ys, views, conf, iou, classes=None, single_cls=False, max_wh=7680., max_out=512, size=None, gs=GS):
    """The rule of ops.tta_merge on the CPU in fp32, with its arguments: the concatenation of the de-augmented rows, then merge_rows_host
    per image (IoU, no candidate limit).
    -> (ym [B, max_out, 4 + nc], src i32 [B, max_out], counts i32 [B], dropped i32 [B])."""
    views = list(views)
    table = tta_view_factors(views, size, gs) if size is not None else [(float(kx), float(ky), bool(f)) for kx, ky, f in views]
    cat = deaugment_host(ys, table)
    return merge_images_host(cat, cat.shape[2], conf, iou, classes, single_cls, 'iou', max_out, None, max_wh)[:4]


# ------------------------------------------------------------------------------------------------ the forward
def _event_marker(events):
    """-> mark(): appends a recorded CUDA timing event to `events` (a list, or None: nothing happens)."""
    def mark():
        if events is not None:
            events.append(torch.cuda.Event(enable_timing=True))
            events[-1].record()
    return mark


def _eval_forward(model, x, txt_feats, autocast_dtype):
    """The model's eval output [len(x), nq, 4 + nc] on x (and txt_feats, when given), under autocast when autocast_dtype is set."""
    with torch.autocast('cuda', dtype=autocast_dtype or torch.bfloat16, enabled=autocast_dtype is not None):
        preds = model(x) if txt_feats is None else model(x, txt_feats=txt_feats)
    return preds[0] if isinstance(preds, (list, tuple)) else preds


@torch.no_grad()
def tta_forward(model, img, txt_feats=None, views=DEFAULT_VIEWS, conf=0.25, iou=0.7, classes=None, single_cls=False, max_out=512,
                autocast_dtype=None, keep=False, events=None):
    """img f32 [B, 3, H, W] on the GPU (already / 255) -> (ym, src, counts, dropped) of ops.tta_merge over the model's eval outputs
    on `views`.  Views whose canvases have the same size go through ONE forward, stacked along the batch (txt_feats [B, nc, d], when
    given, repeated to match); other sizes get a forward each.  conf / iou / classes / single_cls are the ones the following
    postprocess uses.  keep=True: -> (ym, src, counts, dropped, view tensors, per-view raw outputs).  events: a list that receives four
    CUDA events - before and after the view launches, before and after the merge - for a caller that times the phases.
    Nothing synchronises."""
    views = check_views(views)
    B, _, H, W = img.shape
    mark = _event_marker(events)
    mark()
    xs = [ops.tta_view(img, r, f, GS) for r, f in views]
    mark()
    groups = {}
    for k, x in enumerate(xs):
        groups.setdefault(tuple(x.shape[2:]), []).append(k)
    ys = [None] * len(views)
    for ks in groups.values():
        x = xs[ks[0]] if len(ks) == 1 else torch.cat([xs[k] for k in ks])
        y = _eval_forward(model, x, txt_feats if txt_feats is None or len(ks) == 1 else txt_feats.repeat(len(ks), 1, 1), autocast_dtype)
        for k, part in zip(ks, y.split(B)):
            ys[k] = part
    mark()
    merged = ops.tta_merge(ys, views, conf, iou, classes, single_cls, max_out=max_out, size=(H, W), gs=GS)
    mark()
    return merged + (xs, ys) if keep else merged
