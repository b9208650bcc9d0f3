"""Train / validate harness around the hot path: the pieces of the reference's engine that decide numbers.

  build_optimizer      ultralytics/engine/trainer.py:624-681   (three parameter groups: biases, norm weights, decayed weights)
  lr schedule, warm-up ultralytics/engine/trainer.py:276-279,330-340
  train_step           ultralytics/engine/trainer.py:343-357,471-479   (autocast forward, backward, clip 0.1, step, EMA)
  ModelEMA             ultralytics/utils/torch_utils.py:392-419
  postprocess          ultralytics/models/rtdetrworld/val.py:102-128  (conf filter, class-offset NMS; torchvision is not in the
                       image: the greedy NMS is restated here)
  match_predictions    ultralytics/engine/validator.py:208-247, models/yolo/detect/val.py:169-183
  ap_per_class, compute_ap, smooth, box_iou   ultralytics/utils/metrics.py:49-68,941-946,999-1029,1032-1128
  Validator            models/rtdetrworld/val.py:130-173 + models/yolo/detect/val.py get_stats

  fit                  ultralytics/engine/trainer.py:262-281,285-420 (the epoch loop: warm-up, step, schedule, EMA validation,
                       last / best checkpoints) over data.py's loaders

Host-side PyTorch / numpy by design (the reference's is too).  Batches arrive as tensors (img, txt_feats, cls, bboxes, batch_idx
[, ori_shape]) - from data.py's loaders or synthetic; the CLIP text encoder stays out of scope (precomputed table, data.py).
"""
import json
import math
import os
import time
from copy import deepcopy

import numpy as np
import torch
import torch.nn as nn


# ------------------------------------------------------------------------------------------------ training side
def build_optimizer(model, name='AdamW', lr=0.001, momentum=0.9, decay=1e-5, iterations=1e5):
    """Parameter groups exactly as the reference: [0] every '*bias*' (no decay), then weights with decay, then weights of
    normalisation layers (no decay).  name='auto' picks SGD(0.01) above 10 000 iterations, else AdamW(lr = 0.002*5/(4+nc))."""
    g = [], [], []
    norms = tuple(v for k, v in nn.__dict__.items() if 'Norm' in k)
    if name == 'auto':
        nc = getattr(model, 'nc', 10)
        lr_fit = round(0.002 * 5 / (4 + nc), 6)
        name, lr, momentum = ('SGD', 0.01, 0.9) if iterations > 10000 else ('AdamW', lr_fit, 0.9)
    for module_name, module in model.named_modules():
        for param_name, param in module.named_parameters(recurse=False):
            fullname = f'{module_name}.{param_name}' if module_name else param_name
            if 'bias' in fullname:
                g[2].append(param)
            elif isinstance(module, norms):
                g[1].append(param)
            else:
                g[0].append(param)
    if name in ('Adam', 'Adamax', 'AdamW', 'NAdam', 'RAdam'):
        opt = getattr(torch.optim, name)(g[2], lr=lr, betas=(momentum, 0.999), weight_decay=0.0)
    elif name == 'RMSProp':
        opt = torch.optim.RMSprop(g[2], lr=lr, momentum=momentum)
    elif name == 'SGD':
        opt = torch.optim.SGD(g[2], lr=lr, momentum=momentum, nesterov=True)
    else:
        raise NotImplementedError(f"Optimizer '{name}' not found in [Adam, AdamW, NAdam, RAdam, RMSProp, SGD, auto]")
    opt.add_param_group({'params': g[0], 'weight_decay': decay})
    opt.add_param_group({'params': g[1], 'weight_decay': 0.0})
    return opt


def linear_lr(epochs, lrf):
    """lf(epoch): 1 -> lrf linearly (trainer.py:278)."""
    return lambda x: (1 - x / epochs) * (1.0 - lrf) + lrf


def warmup(optimizer, ni, nw, lf_epoch, warmup_bias_lr=0.0, warmup_momentum=0.8, momentum=0.937):
    """Linear warm-up of lr (bias group from warmup_bias_lr, others from 0) and momentum over the first nw iterations
    (trainer.py:330-340; group 0 is the bias group)."""
    if ni > nw:
        return
    for j, x in enumerate(optimizer.param_groups):
        x['lr'] = float(np.interp(ni, [0, nw], [warmup_bias_lr if j == 0 else 0.0, x['initial_lr'] * lf_epoch]))
        if 'momentum' in x:
            x['momentum'] = float(np.interp(ni, [0, nw], [warmup_momentum, momentum]))


class ModelEMA:
    """EMA of every floating-point state_dict entry, decay ramp d(n) = decay * (1 - exp(-n / tau))."""

    def __init__(self, model, decay=0.9999, tau=2000, updates=0):
        self.ema = deepcopy(model).eval()
        self.updates = updates
        self.decay = lambda x: decay * (1 - math.exp(-x / tau))
        for p in self.ema.parameters():
            p.requires_grad_(False)
        self.enabled = True
        self._pairs = None      # (key, ema tensors, model tensors): walking two 1 200-entry state_dicts costs ~10 ms of host time per step

    def _tensors(self, model):
        first = next(model.parameters())
        key = (id(model), first.data_ptr(), len(model._modules))
        if self._pairs is None or self._pairs[0] != key:
            msd = model.state_dict()
            dst, src = [], []
            for k, v in self.ema.state_dict().items():
                if v.dtype.is_floating_point:
                    dst.append(v)
                    src.append(msd[k].detach())
            self._pairs = (key, dst, src)
        return self._pairs[1], self._pairs[2]

    @torch.no_grad()
    def update(self, model):
        if not self.enabled:
            return
        self.updates += 1
        d = self.decay(self.updates)
        dst, src = self._tensors(model)        # (parameters and buffers are updated in place, so the aliases stay valid)
        torch._foreach_mul_(dst, d)            # v = d * v + (1 - d) * m, a few multi-tensor kernels instead of 2 per tensor
        torch._foreach_add_(dst, src, alpha=1 - d)


class FusedOptimStep:
    """The reference's optimizer_step (ultralytics/engine/trainer.py:471-479): clip_grad_norm_(max_norm) -> optimizer.step() ->
    ema.update(model), for torch.optim.AdamW on the GPU, as four kernel launches over a device table that is built once
    (csrc/optim.hip tamtr_optim_step).  torch spends 9.4 ms of host time per step on the same work (grouping ~750 tensors into lists for
    its multi-tensor kernels, three times over: profiles/r04_host_phases.txt), and the host is this step's critical path.

    The optimizer object stays the owner of its state: `optimizer.state[p]` holds exp_avg / exp_avg_sq / step tensors as torch.optim.AdamW
    would have created them (state_dict() / load_state_dict() work; the step counts are 0-d views of one flat tensor), `param_groups`
    is read every step (warm-up and schedules change lr), the EMA object keeps its `updates` counter and decay ramp.
    Same arithmetic as torch's fused AdamW kernel and as ModelEMA.update (fp32); the gradient norm stays on the device.

        stepper = FusedOptimStep.create(model, optimizer, ema, max_norm=0.1)     # None when the combination is not served
        ...backward...;  stepper.step()        # instead of clip_grad_norm_ + optimizer.step() + ema.update(model)
    """

    @staticmethod
    def create(model, optimizer, ema=None, max_norm=0.1, shadows=False):
        """shadows=True: the update kernel also stores every new parameter value rounded to bf16 (`p._tamtr_bf16`, ops.bf16_of): the compute
        copies that bf16 autocast would cast out of the fp32 masters at every use in the next step.  They follow the masters as long as the
        masters are changed by THIS object's step() (or by load_state_dict on the model: a hook refreshes them); ops.bf16_of re-checks the
        tensor version on every use and falls back to a cast, so a stale copy is never read on the eager path - recorded graphs read the
        shadows' memory directly, so re-capture (model.capture_static_part) after switching shadows on or off."""
        ps = [p for g in optimizer.param_groups for p in g['params']]
        ok = (type(optimizer) is torch.optim.AdamW and len(optimizer.param_groups) <= 4 and ps
              and all(p.is_cuda and p.dtype == torch.float32 and (p.is_contiguous() or p.is_contiguous(memory_format=torch.channels_last)) for p in ps)
              and not any(g.get('amsgrad') or g.get('maximize') or g.get('capturable') or g.get('differentiable') for g in optimizer.param_groups))
        if not ok:
            return None
        st = FusedOptimStep(model, optimizer, ema, max_norm, shadows)
        if shadows:
            st._build()          # the copies exist before the first forward (and before a graph capture records their addresses)
        return st

    def __init__(self, model, optimizer, ema=None, max_norm=0.1, shadows=False):
        self.model, self.opt, self.ema, self.max_norm = model, optimizer, ema, float(max_norm)
        self.use_shadows = bool(shadows)
        self.shadows = []        # (parameter, bf16 copy) pairs
        self._key = None
        self._hook = None

    def refresh_shadows(self):
        """Re-derive every bf16 copy from its master (after the masters were changed by anything but step())."""
        with torch.no_grad():
            if self.shadows:
                torch._foreach_copy_([s for _, s in self.shadows], [p for p, _ in self.shadows])
            for p, s in self.shadows:
                s._tamtr_version = p._version

    def drop_shadows(self):
        for p, s in self.shadows:
            s._tamtr_version = -1     # (a recorded graph that still reads this copy re-derives it before every replay: graphs.GraphedPart.__call__)
            if hasattr(p, '_tamtr_bf16'):
                del p._tamtr_bf16
        self.shadows = []
        if self._hook is not None:
            self._hook.remove()
            self._hook = None

    def _state_key(self):
        first = self.opt.param_groups[0]['params'][0]
        st = self.opt.state.get(first, {})
        e = None if self.ema is None else next(self.ema.ema.parameters()).data_ptr()
        return (first.data_ptr(), st['exp_avg'].data_ptr() if 'exp_avg' in st else 0, e, sum(len(g['params']) for g in self.opt.param_groups))

    @torch.no_grad()
    def _build(self):
        from . import _lib
        dev = self.opt.param_groups[0]['params'][0].device
        entries = []                                   # (tensor, group, has_adam)
        for gi, g in enumerate(self.opt.param_groups):
            entries += [(p, gi, True) for p in g['params']]
        opt_ptrs = {p.data_ptr() for p, _, _ in entries}
        ema_of = {}
        if self.ema is not None:
            msd, esd = self.model.state_dict(), self.ema.ema.state_dict()
            by_ptr = {v.data_ptr(): k for k, v in msd.items() if v.dtype.is_floating_point}
            for p, _, _ in entries:
                k = by_ptr.get(p.data_ptr())
                if k is not None:
                    ema_of[id(p)] = esd[k]
            for k, v in msd.items():   # floating-point buffers (BatchNorm statistics) and parameters outside the optimizer: EMA only
                if v.dtype.is_floating_point and v.is_cuda and v.data_ptr() not in opt_ptrs:
                    entries.append((v, 0, False))
                    ema_of[id(v)] = esd[k]
        n = len(entries)
        steps = torch.zeros(n, device=dev, dtype=torch.float32)
        P, M, V, E, SH, numel, group = [], [], [], [], [], [], []
        old_sh = {id(p): s for p, s in self.shadows}
        self.shadows = []
        for i, (t, gi, adam) in enumerate(entries):
            sh = None
            if adam and self.use_shadows:
                sh = old_sh.get(id(t))
                if sh is None or sh.shape != t.shape or sh.stride() != t.stride() or sh.device != t.device:
                    sh = torch.empty_like(t, dtype=torch.bfloat16, memory_format=torch.preserve_format)
                t._tamtr_bf16 = sh
                self.shadows.append((t, sh))
            SH.append(sh.data_ptr() if sh is not None else 0)
            m = v = None
            if adam:
                st = self.opt.state[t]
                if 'exp_avg' not in st:               # what torch.optim.AdamW._init_group creates on its first step
                    st['exp_avg'] = torch.zeros_like(t, memory_format=torch.preserve_format)
                    st['exp_avg_sq'] = torch.zeros_like(t, memory_format=torch.preserve_format)
                elif 'step' in st:
                    steps[i] = float(st['step'])
                st['step'] = steps[i]                 # 0-d view: state_dict() / load_state_dict() see an ordinary step tensor
                m, v = st['exp_avg'], st['exp_avg_sq']
                if m.stride() != t.stride() or v.stride() != t.stride():
                    raise ValueError('FusedOptimStep: optimizer state with other strides than its parameter')
            e = ema_of.get(id(t))
            if e is not None and (e.stride() != t.stride() or e.dtype != torch.float32):
                raise ValueError('FusedOptimStep: EMA copy with another layout than the model tensor')
            P.append(t.data_ptr()); M.append(m.data_ptr() if m is not None else 0); V.append(v.data_ptr() if v is not None else 0)
            E.append(e.data_ptr() if e is not None else 0); numel.append(t.numel()); group.append(gi)
        chunk = _lib.lib().tamtr_optim_chunk()
        ct, co = [], []
        for i, nel in enumerate(numel):
            for off in range(0, nel, chunk):
                ct.append(i); co.append(off)
        I64 = lambda x: torch.tensor(x, dtype=torch.int64, device=dev)   # noqa: E731
        self.refresh_shadows()
        if self.use_shadows and self._hook is None and hasattr(self.model, 'register_load_state_dict_post_hook'):
            self._hook = self.model.register_load_state_dict_post_hook(lambda *_: self.refresh_shadows())
        self.tab = {'p': I64(P), 'm': I64(M), 'v': I64(V), 'e': I64(E), 'sh': I64(SH) if self.use_shadows else None, 'numel': I64(numel), 'group': torch.tensor(group, dtype=torch.uint8, device=dev),
                    'ct': torch.tensor(ct, dtype=torch.int32, device=dev), 'co': I64(co), 'step': steps,
                    'partial': torch.empty(len(ct), device=dev, dtype=torch.float32), 'norm': torch.zeros(2, device=dev, dtype=torch.float32)}
        self.entries, self.n, self.nchunks, self.dev = entries, n, len(ct), dev
        self.strides = [t.stride() for t, _, _ in entries]
        self.adam = [a for _, _, a in entries]
        self._key = self._state_key()

    @torch.no_grad()
    def step(self):
        """clip + AdamW + EMA on the current stream; returns the device tensor [grad norm, clip coefficient] (no host read-back)."""
        import ctypes
        from . import _lib
        from .hostio import stager
        if self._key is None or self._key != self._state_key():   # first step, or state / EMA tensors were replaced (load_state_dict)
            self._build()
        ptrs = [0] * self.n
        for i, (t, _, adam) in enumerate(self.entries):
            if adam:
                g = t.grad
                if g is not None:
                    if g.stride() != self.strides[i] or g.dtype != torch.float32:   # (never on this path: AccumulateGrad keeps the parameter's layout)
                        g = torch.empty_like(t, memory_format=torch.preserve_format).copy_(g)
                        t.grad = g
                    ptrs[i] = g.data_ptr()
        gptr = stager().h2d(torch.tensor(ptrs, dtype=torch.int64), self.dev)
        groups = self.opt.param_groups
        ng = len(groups)
        lr = (ctypes.c_float * ng)(*[float(g['lr']) for g in groups])
        wd = (ctypes.c_float * ng)(*[float(g['weight_decay']) for g in groups])
        b1, b2 = groups[0]['betas']
        if any(g['betas'] != groups[0]['betas'] or g['eps'] != groups[0]['eps'] for g in groups):
            raise ValueError('FusedOptimStep: parameter groups must share betas and eps')
        do_ema, d = 0, 0.0
        if self.ema is not None and self.ema.enabled:
            self.ema.updates += 1
            do_ema, d = 1, self.ema.decay(self.ema.updates)
        T = self.tab
        P = _lib.ptr
        _lib.call('tamtr_optim_step', P(T['p']), P(T['m']), P(T['v']), P(T['e']), P(T['sh']), P(T['step']), P(T['numel']), P(T['group']), P(T['ct']), P(T['co']),
                  P(gptr), self.n, self.nchunks, P(T['partial']), P(T['norm']), ctypes.cast(lr, ctypes.c_void_p), ctypes.cast(wd, ctypes.c_void_p), ng,
                  float(b1), float(b2), float(groups[0]['eps']), self.max_norm, float(d), do_ema, _lib.stream_ptr())
        if self.shadows:   # the kernel rewrote the copy of every tensor that had a gradient; anything else that changed under us is re-derived
            stale = []
            k = 0
            for i, (t, _, adam) in enumerate(self.entries):
                if not adam:
                    continue
                s = self.shadows[k][1]
                k += 1
                if s._tamtr_version != t._version:
                    if ptrs[i]:
                        s._tamtr_version = t._version
                    else:
                        stale.append((t, s))
            if stale:
                torch._foreach_copy_([s for _, s in stale], [t for t, _ in stale])
                for t, s in stale:
                    s._tamtr_version = t._version
        return T['norm']


def train_step(model, batch, optimizer, ema=None, max_norm=0.1):
    """One optimisation step as the reference trainer runs it for RT-DETR models (bf16 autocast replaces the fp16 scaler)."""
    loss, items = model(batch)
    loss.backward()
    torch.nn.utils.clip_grad_norm_([p for p in model.parameters() if p.grad is not None], max_norm=max_norm)
    optimizer.step()
    optimizer.zero_grad(set_to_none=True)
    if ema is not None:
        ema.update(model)
    return loss.detach(), items   # (the three torch calls; engine.fit and bench.py run them as FusedOptimStep on the GPU)


# ------------------------------------------------------------------------------------------------ validation side
def xywh2xyxy(b):
    half = b[..., 2:] / 2
    return torch.cat([b[..., :2] - half, b[..., :2] + half], -1)


def box_iou(box1, box2, eps=1e-7):
    """[N,4] x [M,4] xyxy -> [N,M]."""
    (a1, a2), (b1, b2) = box1.unsqueeze(1).chunk(2, 2), box2.unsqueeze(0).chunk(2, 2)
    inter = (torch.min(a2, b2) - torch.max(a1, b1)).clamp_(0).prod(2)
    return inter / ((a2 - a1).prod(2) + (b2 - b1).prod(2) - inter + eps)


def nms(boxes, scores, iou_thres):
    """Greedy NMS (torchvision.ops.nms semantics: keep in descending score order, suppress IoU > thres); <= a few hundred boxes."""
    order = scores.argsort(descending=True)
    if order.numel() == 0:
        return order
    iou = box_iou(boxes[order], boxes[order], eps=0.0).cpu().numpy()
    alive = np.ones(len(order), dtype=bool)
    keep = []
    for i in range(len(order)):
        if alive[i]:
            keep.append(i)
            alive &= ~(iou[i] > iou_thres)
            alive[i] = False
    return order[torch.as_tensor(keep, dtype=torch.long, device=order.device)]


def postprocess(preds, imgsz, conf=0.001, iou=0.7, single_cls=False, max_wh=7680):
    """Eval output [B, nq, 4 + nc] (xywh in 0..1, sigmoid scores) -> list of [n, 6] (xyxy pixels, conf, cls), conf-sorted and
    class-aware NMS'ed, as RTDETRValidator.postprocess."""
    y = preds[0] if isinstance(preds, (list, tuple)) else preds
    nd = y.shape[-1]
    bboxes, scores = y.split((4, nd - 4), dim=-1)
    bboxes = bboxes * imgsz
    out = []
    for i, bbox in enumerate(bboxes):
        bbox = xywh2xyxy(bbox)
        score, cls = scores[i].max(-1)
        pred = torch.cat([bbox, score[..., None], cls[..., None].to(bbox.dtype)], -1)
        order = score.argsort(descending=True)
        pred = pred[order][score > conf]  # the reference applies the UNSORTED confidence mask to the sorted rows (val.py:113-121): kept
        c = pred[:, 5:6] * (0 if single_cls else max_wh)
        out.append(pred[nms(pred[:, :4] + c, pred[:, 4], iou)])
    return out


IOUV = torch.linspace(0.5, 0.95, 10)


def match_predictions(pred_classes, true_classes, iou, iouv=IOUV):
    """correct[N, 10]: detection n is a true positive at IoU threshold t (one detection per label, best IoU first)."""
    correct = np.zeros((pred_classes.shape[0], iouv.shape[0])).astype(bool)
    correct_class = true_classes[:, None] == pred_classes
    iou = (iou * correct_class).cpu().numpy()
    for i, threshold in enumerate(iouv.cpu().tolist()):
        matches = np.array(np.nonzero(iou >= threshold)).T
        if matches.shape[0]:
            if matches.shape[0] > 1:
                matches = matches[iou[matches[:, 0], matches[:, 1]].argsort()[::-1]]
                matches = matches[np.unique(matches[:, 1], return_index=True)[1]]
                matches = matches[np.unique(matches[:, 0], return_index=True)[1]]
            correct[matches[:, 1].astype(int), i] = True
    return torch.tensor(correct, dtype=torch.bool, device=pred_classes.device)


def process_batch(detections, labels, iouv=IOUV):
    """detections [N, 6] xyxy conf cls; labels [M, 5] cls xyxy."""
    return match_predictions(detections[:, 5], labels[:, 0], box_iou(labels[:, 1:], detections[:, :4]), iouv)


def smooth(y, f=0.05):
    """Centred moving average of y over an odd window of about 2*f*len(y) samples; beyond the ends y is held at y[0] / y[-1].
    (metrics.py:941-946 does the same with a padded convolution; here a running sum.)"""
    win = round(len(y) * f * 2) // 2 + 1
    half = win // 2
    held = np.concatenate((np.full(half, y[0]), y, np.full(half, y[-1])))
    run = np.concatenate(([0.0], np.cumsum(held)))
    return (run[win:win + len(held) - win + 1] - run[:len(held) - win + 1]) / win


_AP_GRID = np.linspace(0.0, 1.0, 101)   # COCO's 101 recall samples


def compute_ap(recall, precision):
    """Area under the precision envelope sampled on the 101-point recall grid (metrics.py:999-1029).  recall, precision: the
    cumulative curves of one class at one IoU threshold, in descending-confidence order.  Returns (ap, envelope, recall knots)."""
    knots_r = np.empty(len(recall) + 2)
    knots_p = np.empty(len(precision) + 2)
    knots_r[0], knots_r[1:-1], knots_r[-1] = 0.0, recall, 1.0
    knots_p[0], knots_p[1:-1], knots_p[-1] = 1.0, precision, 0.0
    envelope = np.maximum.accumulate(knots_p[::-1])[::-1]        # best precision attainable at recall >= r
    y = np.interp(_AP_GRID, knots_r, envelope)
    h = _AP_GRID[1] - _AP_GRID[0]
    area = h * (y.sum() - 0.5 * (y[0] + y[-1]))                   # trapezoid rule on the uniform grid
    return area, envelope, knots_r


def _curves_of_class(hit, score, n_gt, grid, eps):
    """hit [n, T] bool (descending score), score [n]: recall / precision of the first IoU threshold resampled on `grid` (confidence
    axis), the AP of every threshold, and the first threshold's precision envelope resampled on `grid` (recall axis)."""
    tp_run = hit.cumsum(0)
    fp_run = (1 - hit).cumsum(0)
    recall = tp_run / (n_gt + eps)
    precision = tp_run / (tp_run + fp_run)
    r_grid = np.interp(-grid, -score, recall[:, 0], left=0)          # confidence decreases along the arrays: negate to interpolate
    p_grid = np.interp(-grid, -score, precision[:, 0], left=1)
    per_t = [compute_ap(recall[:, t], precision[:, t]) for t in range(hit.shape[1])]
    ap = np.array([a for a, _, _ in per_t])
    _, envelope, knots_r = per_t[0]
    return r_grid, p_grid, ap, np.interp(grid, knots_r, envelope)


def operating_point(p_curve, r_curve, n_gt, eps=1e-16):
    """-> tp, fp, p, r, f1 at the one confidence that maximises the smoothed mean F1 over classes, and f1_curve (metrics.py:1113-1126).
    p_curve, r_curve [classes, 1000] over confidence, n_gt [classes]: shared by ap_per_class and the device path of DeviceValidator."""
    f1_curve = 2 * p_curve * r_curve / (p_curve + r_curve + eps)
    best = smooth(f1_curve.mean(0), 0.1).argmax()                       # one operating confidence for all classes
    p, r, f1 = p_curve[:, best], r_curve[:, best], f1_curve[:, best]
    tpn = (r * n_gt).round()
    fpn = (tpn / (p + eps) - tpn).round()
    return tpn, fpn, p, r, f1, f1_curve


def ap_per_class(tp, conf, pred_cls, target_cls, eps=1e-16, curves=False, stable=False):
    """-> tp, fp, p, r, f1 (at the max-F1 confidence), ap [nc, 10], unique_classes   (metrics.py:1032-1128; its plots are the curves below).
    Classes are the ones that have ground truth; a class nobody predicted keeps zero curves.
    curves: an eighth element, a dict of float64 arrays whose rows follow the returned classes: 'px' = linspace(0, 1, 1000); 'p', 'r',
    'f1' [classes, 1000] over confidence (the reference's P_curve, R_curve, F1_curve); 'pr' [classes, 1000], the precision envelope of the
    first IoU threshold over recall px (its PR_curve, `prec_values`); 'valid' bool [classes]: the class has labels and predictions.  The
    reference appends prec_values for valid classes only, so its rows lose their class; here the rows are dense, zero where not valid.
    stable: predictions of equal confidence keep their input order (image order, then row order) instead of the order numpy's default
    argsort happens to give them.  The two agree when no two confidences are equal; csrc/metrics.hip implements the stable order."""
    order = np.argsort(-conf, kind='stable') if stable else np.argsort(-conf)
    tp, conf, pred_cls = tp[order], conf[order], pred_cls[order]
    classes, n_gt = np.unique(target_cls, return_counts=True)
    grid = np.linspace(0, 1, 1000)
    ap = np.zeros((len(classes), tp.shape[1]))
    p_curve, r_curve = np.zeros((len(classes), grid.size)), np.zeros((len(classes), grid.size))
    pr_curve, valid = np.zeros((len(classes), grid.size)), np.zeros(len(classes), bool)
    for row, (c, n) in enumerate(zip(classes, n_gt)):
        mine = pred_cls == c
        if n == 0 or not mine.any():
            continue
        r_curve[row], p_curve[row], ap[row], pr_curve[row] = _curves_of_class(tp[mine], conf[mine], n, grid, eps)
        valid[row] = True
    tpn, fpn, p, r, f1, f1_curve = operating_point(p_curve, r_curve, n_gt, eps)
    out = (tpn, fpn, p, r, f1, ap, classes.astype(int))
    if curves:
        out += ({'px': grid, 'p': p_curve, 'r': r_curve, 'f1': f1_curve, 'pr': pr_curve, 'valid': valid},)
    return out


def curves_as_lists(curves, classes):
    """The curves dict of ap_per_class as nested lists plus 'classes': what results(curves=True) carries under 'curves'."""
    return {**{k: np.asarray(v).tolist() for k, v in curves.items()}, 'classes': [int(c) for c in classes]}


# ------------------------------------------------------------------------------------------------ COCO-protocol evaluation
COCO_T = np.linspace(0.5, 0.95, 10)          # IoU thresholds
COCO_R = np.linspace(0.0, 1.0, 101)          # recall grid
COCO_AREAS = ((0.0, 1e10), (0.0, 32.0 ** 2), (32.0 ** 2, 96.0 ** 2), (96.0 ** 2, 1e10))   # all, small, medium, large; inclusive at both ends
COCO_KEYS = ('AP', 'AP50', 'AP75', 'APs', 'APm', 'APl', 'AR1', 'AR10', 'AR100', 'ARs', 'ARm', 'ARl')


def coco_cuts(max_dets):
    """max_dets as a tuple of ints, checked: 1 to 4 positive entries, strictly ascending."""
    md = tuple(int(m) for m in max_dets)
    if not 1 <= len(md) <= 4 or md[0] < 1 or any(b <= a for a, b in zip(md, md[1:])):
        raise ValueError(f'coco: max_dets must be 1 to 4 ascending positive integers, got {tuple(max_dets)}')
    return md


def _coco_match_image(det, lab, nc, cut):
    """One image.  det f32 [n, 6] (x1 y1 x2 y2 score cls, any order), lab f32 [m, 5] (cls x1 y1 x2 y2).  -> bits i32 [n, 4] (per size range:
    bit t = matched at threshold t, bit 16 + t = ignored), rank i32 [n] (rank among the image's participating rows of the class in stable
    descending score order, -1: takes part in nothing), npig i64 [nc, 4].  The statement of csrc/cocoeval.hip's matching rule."""
    n = det.shape[0]
    bits, rank, npig = np.zeros((n, 4), np.int32), np.full(n, -1, np.int32), np.zeros((nc, 4), np.int64)
    dcl_f, gcl_f = np.trunc(det[:, 5]), np.trunc(lab[:, 0])
    d_ok = (dcl_f >= 0) & (dcl_f < nc) & ~np.isnan(det[:, 4])         # NaN classes fail both comparisons
    g_ok = (gcl_f >= 0) & (gcl_f < nc)
    dbox, gbox = det[:, :4].astype(np.float64), lab[:, 1:5].astype(np.float64)
    darea = (dbox[:, 2] - dbox[:, 0]) * (dbox[:, 3] - dbox[:, 1])
    garea = (gbox[:, 2] - gbox[:, 0]) * (gbox[:, 3] - gbox[:, 1])
    thr = np.minimum(COCO_T, 1 - 1e-10)
    for k in np.unique(np.concatenate([dcl_f[d_ok], gcl_f[g_ok]])).astype(int):
        di = np.nonzero(d_ok & (dcl_f == k))[0]
        di = di[np.argsort(-det[di, 4], kind='stable')]               # COCO's mergesort on -score
        rank[di] = np.arange(len(di))
        di = di[:cut]                                                   # later ones take part in nothing and consume no ground truth
        gi = np.nonzero(g_ok & (gcl_f == k))[0]
        for a, (lo, hi) in enumerate(COCO_AREAS):
            g_ign = (garea[gi] < lo) | (garea[gi] > hi)
            npig[k, a] += int((~g_ign).sum())
            go = gi[np.argsort(g_ign, kind='stable')]                  # non-ignored first, file order inside each group
            g_ign = np.sort(g_ign, kind='stable')
            d_out = (darea[di] < lo) | (darea[di] > hi)
            if len(go) and len(di):
                iw = np.minimum(dbox[di, None, 2], gbox[None, go, 2]) - np.maximum(dbox[di, None, 0], gbox[None, go, 0])
                ih = np.minimum(dbox[di, None, 3], gbox[None, go, 3]) - np.maximum(dbox[di, None, 1], gbox[None, go, 1])
                inter = iw * ih
                union = (darea[di, None] + garea[None, go]) - inter
                with np.errstate(divide='ignore', invalid='ignore'):
                    iou = np.where((iw > 0) & (ih > 0) & (union > 0), inter / union, 0.0)
            else:
                iou = np.zeros((len(di), len(go)))
            top = iou.max(1) if len(go) else np.zeros(len(di))
            for t in range(10):
                taken = np.zeros(len(go), bool)
                for j in np.nonzero(top >= thr[t])[0]:                  # (the others have no ground truth to walk to: unmatched)
                    # the walk over `go` with best = thr, "skip when iou < best", "stop at the first ignored one once a non-ignored one is
                    # held": the arg-max of (non-ignored, IoU, position) over the unmatched ones with IoU >= thr (a NaN IoU never qualifies)
                    cand = ~taken & (iou[j] >= thr[t])
                    if cand.any():
                        pool = cand & ~g_ign if (cand & ~g_ign).any() else cand
                        m = np.nonzero(pool & (iou[j] == iou[j][pool].max()))[0][-1]           # equal IoUs: the later one
                        taken[m] = True
                        bits[di[j], a] |= (1 << t) | (int(g_ign[m]) << (16 + t))
                unmatched = (bits[di, a] & (1 << t)) == 0
                bits[di[unmatched & d_out], a] |= 1 << (16 + t)           # an unmatched detection outside the range is ignored
    return bits, rank, npig


def coco_accumulate(score, cls, bits, rank, npig, nc, max_dets):
    """The run's rows (image order, then row order): score [n], cls [n], bits [n, 4], rank [n] and npig [nc, 4] -> precision f64
    [10, 101, nc, 4, M], recall f64 [10, nc, 4, M].  The statement of csrc/cocoeval.hip's accumulation rule."""
    md = coco_cuts(max_dets)
    precision = -np.ones((10, 101, nc, 4, len(md)))
    recall = -np.ones((10, nc, 4, len(md)))
    cls_i = np.trunc(np.where(rank >= 0, cls, -1)).astype(np.int64)
    tbit = 1 << np.arange(10)
    for k in range(nc):
        mine = np.nonzero((rank >= 0) & (cls_i == k))[0]
        for a in range(4):
            n_gt = int(npig[k, a])
            if n_gt == 0:
                continue
            for mi, cut in enumerate(md):
                rows = mine[rank[mine] < cut]
                rows = rows[np.argsort(-score[rows], kind='stable')]
                w = bits[rows, a].astype(np.int64)
                matched, ignored = (w[:, None] & tbit) != 0, ((w[:, None] >> 16) & tbit) != 0
                tp = (matched & ~ignored).cumsum(0).astype(np.float64)          # [n, 10]
                fp = (~matched & ~ignored).cumsum(0).astype(np.float64)
                rc = tp / n_gt
                pr = tp / ((fp + tp) + 2.220446049250313e-16)
                pr = np.maximum.accumulate(pr[::-1], axis=0)[::-1]
                for t in range(10):
                    recall[t, k, a, mi] = rc[-1, t] if len(rows) else 0.0
                    at = np.searchsorted(rc[:, t], COCO_R, side='left')
                    ok = at < len(rows)
                    q = np.zeros(101)
                    q[ok] = pr[at[ok], t]
                    precision[t, :, k, a, mi] = q
    return precision, recall


def coco_summary(ap_tkam, recall, max_dets, npig=None, names=None):
    """The twelve COCO numbers and the per-class rows from ap_tkam and recall (f64 [10, nc, 4, M]; ap_tkam = the mean of precision over the
    recall grid, -1 where the class has no ground truth in the range) - the host and the device path both end in these lines.  Each number
    is the mean over the entries > -1, or -1 when there are none; the cut is the last of max_dets unless it is named (AR1 / AR10 / AR100 =
    the first three cuts, -1 for a cut max_dets does not have)."""
    md = coco_cuts(max_dets)
    ap_tkam, recall = np.asarray(ap_tkam, np.float64), np.asarray(recall, np.float64)

    def mean(x):
        x = x[x > -1]
        return float(x.mean()) if x.size else -1.0

    out = {'AP': mean(ap_tkam[:, :, 0, -1]), 'AP50': mean(ap_tkam[0, :, 0, -1]), 'AP75': mean(ap_tkam[5, :, 0, -1]),
           'APs': mean(ap_tkam[:, :, 1, -1]), 'APm': mean(ap_tkam[:, :, 2, -1]), 'APl': mean(ap_tkam[:, :, 3, -1])}
    for i, key in enumerate(('AR1', 'AR10', 'AR100')):
        out[key] = mean(recall[:, :, 0, i]) if i < len(md) else -1.0
    out.update({'ARs': mean(recall[:, :, 1, -1]), 'ARm': mean(recall[:, :, 2, -1]), 'ARl': mean(recall[:, :, 3, -1]), 'max_dets': list(md)})
    per_class = []
    for k in range(ap_tkam.shape[1]):
        row = {'class': names[k] if names is not None else k, 'AP': mean(ap_tkam[:, k, 0, -1]), 'AP50': mean(ap_tkam[0, k, 0, -1]),
               'APs': mean(ap_tkam[:, k, 1, -1]), 'APm': mean(ap_tkam[:, k, 2, -1]), 'APl': mean(ap_tkam[:, k, 3, -1])}
        if npig is not None:
            row.update({'npig': int(npig[k, 0]), 'npig_s': int(npig[k, 1]), 'npig_m': int(npig[k, 2]), 'npig_l': int(npig[k, 3])})
        per_class.append(row)
    out['per_class'] = per_class
    return out


def coco_evaluate(images, nc, max_dets=(1, 10, 100), names=None, return_matches=False):
    """COCO-protocol bbox evaluation (pycocotools' COCOeval evaluate + accumulate + summarize with iscrowd = 0, restated; the rule is
    written out in csrc/cocoeval.hip, whose checker this is, and the host Validator's path).  images: per image (det [n, 6] x1 y1 x2 y2
    score cls in native pixels, labels [m, 5] cls x1 y1 x2 y2), arrays or tensors; EVERY image is evaluated, also one without labels
    (its detections are false positives).  All arithmetic is fp64 on the fp32 values.
    -> {'precision' f64 [10, 101, nc, 4, M], 'recall', 'ap_tkam' f64 [10, nc, 4, M], 'npig' i64 [nc, 4], 'summary': coco_summary's dict}
    and, with return_matches, 'matches': per image (bits i32 [n, 4], rank i32 [n]) in the image's row order."""
    md, nc = coco_cuts(max_dets), int(nc)
    as_np = lambda x, w: (x.detach().float().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x, np.float32)).reshape(-1, w)  # noqa: E731
    npig, matches, score, cls = np.zeros((nc, 4), np.int64), [], [], []
    for det, lab in images:
        det, lab = as_np(det, 6), as_np(lab, 5)
        b, r, g = _coco_match_image(det, lab, nc, md[-1])
        npig += g
        matches.append((b, r))
        score.append(det[:, 4])
        cls.append(det[:, 5])
    cat = lambda xs, shape, dt: np.concatenate(xs) if xs else np.zeros(shape, dt)   # noqa: E731
    precision, recall = coco_accumulate(cat(score, (0,), np.float32), cat(cls, (0,), np.float32), cat([m[0] for m in matches], (0, 4), np.int32),
                                        cat([m[1] for m in matches], (0,), np.int32), npig, nc, md)
    ap_tkam = np.where(precision[:, 0] > -1, precision.sum(1) / 101.0, -1.0)
    out = {'precision': precision, 'recall': recall, 'ap_tkam': ap_tkam, 'npig': npig, 'summary': coco_summary(ap_tkam, recall, md, npig, names)}
    if return_matches:
        out['matches'] = matches
    return out


# ------------------------------------------------------------------------------------------------ MOT evaluation
# the columns of the per-class count table, on the host and on the device (csrc/mot.hip keeps them as i32 [nc, 16])
MOT_COUNT_KEYS = ('TP', 'FN', 'FP', 'IDSW', 'gt_dets', 'trk_dets', 'Frag', 'MT', 'PT', 'ML', 'IDTP', 'gt_ids', 'drop_region', 'drop_distractor')


def mot_iou_matrix(a, b):
    """fp64 IoU of boxes a [n, 4] and b [m, 4] (x1 y1 x2 y2), op by op as csrc/mot.hip: 0 where iw <= 0, ih <= 0 or union <= 0."""
    a, b = np.asarray(a, np.float64).reshape(-1, 4), np.asarray(b, np.float64).reshape(-1, 4)
    iw = np.minimum(a[:, None, 2], b[None, :, 2]) - np.maximum(a[:, None, 0], b[None, :, 0])
    ih = np.minimum(a[:, None, 3], b[None, :, 3]) - np.maximum(a[:, None, 1], b[None, :, 1])
    inter = iw * ih
    area_a, area_b = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1]), (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    union = (area_a[:, None] + area_b[None, :]) - inter
    ok = (iw > 0) & (ih > 0) & (union > 0)
    return np.where(ok, inter / np.where(ok, union, 1.0), 0.0), np.where((iw > 0) & (ih > 0), inter, 0.0)


def _mot_assign(score):
    """The (row, column) pairs of the assignment that maximises the total score, those with a score > 0."""
    from scipy.optimize import linear_sum_assignment
    if score.size == 0:
        return []
    r, c = linear_sum_assignment(score, maximize=True)
    return [(int(i), int(j)) for i, j in zip(r, c) if score[i, j] > 0]


def mot_new_counts(nc):
    c = {k: np.zeros(int(nc), np.int64) for k in MOT_COUNT_KEYS}
    c['iou_sum'] = np.zeros(int(nc), np.float64)
    return c


def _mot_preprocess(gt, trk, nc, thr, out=None):
    """Steps 1 (regions) and 2 (distractors) of the MOT rule on one frame, shared by mot_evaluate, hota_evaluate and track_map_evaluate.
    -> (kind-0 rows [n, 7], their classes, surviving track rows [k, 6] - [k, 7] when they came with a score -, their classes); the dropped
    rows are counted into out."""
    f32 = lambda x, w: np.asarray(x, np.float32).reshape(-1, w)   # noqa: E731
    trk = np.asarray(trk, np.float32)
    gt, trk = f32(gt, 7), f32(trk, 7 if trk.ndim == 2 and trk.shape[1] == 7 else 6)   # a seventh column (the score) rides along
    kind = gt[:, 6]
    in_range = lambda c: (c >= 0) & (c < nc)   # noqa: E731
    trk = trk[in_range(trk[:, 5])]
    tcls = trk[:, 5].astype(np.int64)
    # 1. regions
    reg = gt[kind == 2]
    if len(reg) and len(trk):
        _, inter = mot_iou_matrix(trk[:, :4], reg[:, :4])
        area = (trk[:, 2].astype(np.float64) - trk[:, 0]) * (trk[:, 3].astype(np.float64) - trk[:, 1])
        ioa = np.where(area[:, None] > 0, inter / np.where(area > 0, area, 1.0)[:, None], 0.0)
        drop = (ioa > 0.5).any(1)
        if out is not None:
            np.add.at(out['drop_region'], tcls[drop], 1)
        trk, tcls = trk[~drop], tcls[~drop]
    # 2. distractors
    g = gt[((kind == 0) & in_range(gt[:, 5])) | (kind == 1)]
    if (g[:, 6] == 1).any() and len(trk):
        m, _ = mot_iou_matrix(g[:, :4], trk[:, :4])
        agree = (g[:, 6] == 1)[:, None] | (g[:, 5].astype(np.int64)[:, None] == tcls[None, :])
        drop = np.zeros(len(trk), bool)
        for i, j in _mot_assign(np.where((m >= thr) & agree, m, 0.0)):
            drop[j] |= g[i, 6] == 1
        if out is not None:
            np.add.at(out['drop_distractor'], tcls[drop], 1)
        trk, tcls = trk[~drop], tcls[~drop]
    g = g[g[:, 6] == 0]
    return g, g[:, 5].astype(np.int64), trk, tcls


def mot_evaluate(sequences, nc, iou=0.5):
    """CLEAR-MOT and identity counts of tracker output against ground truth (TrackEval's CLEAR and Identity definitions, restated; the
    rule is written out in csrc/mot.hip, whose checker this is, and this is the path for a machine without a GPU).
    sequences: a list of sequences, each a list of frames in order, each frame (gt [m, 7] x1 y1 x2 y2 id cls kind, tracks [k, 6]
    x1 y1 x2 y2 id cls); kind 0 object, 1 distractor, 2 ignored region.  All arithmetic is fp64 on the fp32 values.  A ground truth
    (and a track) identity is the pair (class, id).  -> {key: i64 [nc] for key in MOT_COUNT_KEYS, 'iou_sum': f64 [nc]}; counts of
    several sequences add, and mot_summary turns them into MOTA / MOTP / IDF1 ..."""
    nc, thr = int(nc), float(iou)
    out = mot_new_counts(nc)
    for frames in sequences:
        last, present, matched, runs, last_frame, pair = {}, {}, {}, {}, {}, {}
        for fid, (gt, trk) in enumerate(frames, 1):
            g, gcls, trk, tcls = _mot_preprocess(gt, trk, nc, thr, out)
            # 3. CLEAR matching and 4. pair counts, per class
            for c in range(nc):
                gc, tc = g[gcls == c], trk[tcls == c]
                gid, tid = [(c, int(i)) for i in gc[:, 4]], [int(i) for i in tc[:, 4]]
                out['gt_dets'][c] += len(gc)
                out['trk_dets'][c] += len(tc)
                for k in gid:
                    present[k] = present.get(k, 0) + 1
                m, _ = mot_iou_matrix(gc[:, :4], tc[:, :4])
                q = m >= thr
                keeps = np.array([[last.get(k) == t for t in tid] for k in gid], bool).reshape(m.shape)
                pairs = _mot_assign(np.where(q & keeps, m + 1000.0, np.where(q, m, 0.0)))
                out['TP'][c] += len(pairs)
                out['FN'][c] += len(gc) - len(pairs)
                out['FP'][c] += len(tc) - len(pairs)
                for i, j in pairs:
                    k = gid[i]
                    out['iou_sum'][c] += m[i, j]
                    out['IDSW'][c] += k in last and last[k] != tid[j]
                    last[k] = tid[j]
                    runs[k] = runs.get(k, 0) + (last_frame.get(k) != fid - 1)
                    matched[k] = matched.get(k, 0) + 1
                    last_frame[k] = fid
                for i, j in zip(*np.nonzero(q)):
                    pair[(gid[i], tid[j])] = pair.get((gid[i], tid[j]), 0) + 1
        # the sequence's reduction
        for k, n in present.items():
            c, ratio = k[0], matched.get(k, 0) / n
            out['gt_ids'][c] += 1
            out['MT' if ratio > 0.8 else 'ML' if ratio < 0.2 else 'PT'][c] += 1
            out['Frag'][c] += max(runs.get(k, 0) - 1, 0)
        for c in range(nc):
            rows = sorted({g for g, _ in pair if g[0] == c})
            cols = sorted({t for g, t in pair if g[0] == c})
            tab = np.zeros((len(rows), len(cols)), np.int64)
            for (g, t), v in pair.items():
                if g[0] == c:
                    tab[rows.index(g), cols.index(t)] = v
            out['IDTP'][c] += sum(int(tab[i, j]) for i, j in _mot_assign(tab))
    return out


def mot_summary(counts, names=None):
    """Per-class rows and an 'all' row of summed counts from mot_evaluate's (or MotEvaluator's) counts.  A ratio whose denominator is 0
    is nan.  -> {'all': row, 'per_class': [row, ...]}; a row holds every count, IDFN / IDFP, and MOTA MOTP Recall Precision IDF1 IDP IDR."""
    def row(c, label):
        div = lambda a, b: float(a) / float(b) if b else float('nan')   # noqa: E731
        r = {'class': label, **{k: int(c[k]) for k in MOT_COUNT_KEYS}, 'iou_sum': float(c['iou_sum'])}
        r['IDFN'], r['IDFP'] = r['gt_dets'] - r['IDTP'], r['trk_dets'] - r['IDTP']
        r['MOTA'] = 1.0 - div(r['FN'] + r['FP'] + r['IDSW'], r['gt_dets'])
        r['MOTP'] = div(r['iou_sum'], r['TP'])
        r['Recall'], r['Precision'] = div(r['TP'], r['gt_dets']), div(r['TP'], r['trk_dets'])
        r['IDF1'] = div(r['IDTP'], r['IDTP'] + 0.5 * r['IDFP'] + 0.5 * r['IDFN'])
        r['IDP'], r['IDR'] = div(r['IDTP'], r['trk_dets']), div(r['IDTP'], r['gt_dets'])
        return r

    keys = MOT_COUNT_KEYS + ('iou_sum',)
    nc = len(np.atleast_1d(counts['TP']))
    per = [row({k: np.atleast_1d(counts[k])[c] for k in keys}, names[c] if names is not None else c) for c in range(nc)]
    return {'all': row({k: np.atleast_1d(counts[k]).sum() for k in keys}, 'all'), 'per_class': per}


def mot_table(summary, title=''):
    """mot_summary's rows as the table every MOT benchmark prints (percentages for the ratios)."""
    cols = ('MOTA', 'MOTP', 'IDF1', 'IDP', 'IDR', 'Recall', 'Precision')
    ints = ('gt_ids', 'MT', 'PT', 'ML', 'TP', 'FP', 'FN', 'IDSW', 'Frag')
    lines = [f'{title or "class":>16s}' + ''.join(f'{c:>8s}' for c in cols) + ''.join(f'{c:>8s}' for c in ints)]
    for r in summary['per_class'] + [summary['all']]:
        lines.append(f'{str(r["class"]):>16s}' + ''.join(f'{100 * r[c]:8.2f}' for c in cols) + ''.join(f'{r[c]:8d}' for c in ints))
    return '\n'.join(lines)


def mot_add_counts(a, b):
    """Counts of several sequences (or runs) add."""
    return {k: a[k] + b[k] for k in a}


# ------------------------------------------------------------------------------------------------ HOTA
# the 19 localisation thresholds and the slack of every threshold comparison, as TrackEval makes them (never k / 20: several differ in the last bit)
HOTA_ALPHA = np.arange(0.05, 0.99, 0.05)
HOTA_EPS = float(np.finfo(float).eps)
HOTA_INT_KEYS, HOTA_SUM_KEYS = ('TP', 'FN', 'FP'), ('loc_sum', 'ass_sum', 'assre_sum', 'asspr_sum')
HOTA_RATIOS = ('HOTA', 'DetA', 'AssA', 'DetRe', 'DetPr', 'AssRe', 'AssPr', 'LocA')


def hota_new_counts(nc):
    na = len(HOTA_ALPHA)
    c = {k: np.zeros((int(nc), na), np.int64) for k in HOTA_INT_KEYS}
    c.update({k: np.zeros((int(nc), na), np.float64) for k in HOTA_SUM_KEYS})
    c.update({k: np.zeros(int(nc), np.int64) for k in ('gt_dets', 'trk_dets')})
    return c


def hota_add_counts(a, b):
    """Counts of several sequences (or runs) add: TrackEval's combine_sequences weights the per-sequence ratios by TP, which is this."""
    return {k: a[k] + b[k] for k in a}


def hota_evaluate(sequences, nc, iou=0.5):
    """HOTA counts of tracker output against ground truth (TrackEval's HOTA.eval_sequence, restated; the rule is written out in
    csrc/hota.hip, whose checker this is, and this is the path for a machine without a GPU).  Arguments as mot_evaluate; `iou` is the
    threshold of the region / distractor preprocessing, which is mot_evaluate's.  -> {'TP' 'FN' 'FP': i64 [nc, 19], 'loc_sum' 'ass_sum'
    'assre_sum' 'asspr_sum': f64 [nc, 19], 'gt_dets' 'trk_dets': i64 [nc]}; counts of several sequences add (hota_add_counts) and
    hota_summary turns them into HOTA / DetA / AssA ..."""
    nc, thr = int(nc), float(iou)
    out = hota_new_counts(nc)
    for frames in sequences:
        pot, gcount, tcount, kept = {}, {}, {}, []
        # pass 1: the global alignment score needs the whole sequence
        for gt, trk in frames:
            g, gcls, trk, tcls = _mot_preprocess(gt, trk, nc, thr)
            for c in range(nc):
                gc, tc = g[gcls == c], trk[tcls == c]
                gid, tid = [(c, int(i)) for i in gc[:, 4]], [(c, int(i)) for i in tc[:, 4]]
                out['gt_dets'][c] += len(gc)
                out['trk_dets'][c] += len(tc)
                for k in gid:
                    gcount[k] = gcount.get(k, 0) + 1
                for k in tid:
                    tcount[k] = tcount.get(k, 0) + 1
                if not len(gc) or not len(tc):
                    continue
                S, _ = mot_iou_matrix(gc[:, :4], tc[:, :4])
                den = (S.sum(1)[:, None] + S.sum(0)[None, :]) - S
                ok = den > HOTA_EPS
                sim = np.where(ok, S / np.where(ok, den, 1.0), 0.0)
                for i, j in zip(*np.nonzero(S)):
                    pot[(gid[i], tid[j])] = pot.get((gid[i], tid[j]), 0.0) + sim[i, j]
                kept.append((c, gid, tid, S))
        # pass 2: one assignment per frame and class, weighted by the alignment score
        mc = {}
        for c, gid, tid, S in kept:
            gas = np.zeros_like(S)
            for i, j in zip(*np.nonzero(S)):
                p = pot[(gid[i], tid[j])]
                gas[i, j] = p / ((gcount[gid[i]] + tcount[tid[j]]) - p)
            for i, j in _hota_assign(gas * S, S):
                hit = S[i, j] >= HOTA_ALPHA - HOTA_EPS
                out['TP'][c] += hit
                out['loc_sum'][c] += np.where(hit, S[i, j], 0.0)
                k = (gid[i], tid[j])
                mc[k] = mc.get(k, 0) + hit.astype(np.int64)
        for (gk, tk), m in mc.items():
            sq = (m * m).astype(np.float64)
            out['ass_sum'][gk[0]] += sq / np.maximum(1, gcount[gk] + tcount[tk] - m)
            out['assre_sum'][gk[0]] += sq / max(1, gcount[gk])
            out['asspr_sum'][gk[0]] += sq / max(1, tcount[tk])
    out['FN'], out['FP'] = out['gt_dets'][:, None] - out['TP'], out['trk_dets'][:, None] - out['TP']
    return out


def _hota_assign(score, S):
    """The matched pairs of pass 2; hota_evaluate's one call of the solver, so that a test can put another rule in its place."""
    return _mot_assign(score)


def hota_summary(counts, names=None):
    """Per-class rows and an 'all' row of summed counts (TrackEval's combine_classes_det_averaged) from hota_evaluate's (or
    HotaEvaluator's) counts.  A row holds, for each of HOTA DetA AssA DetRe DetPr AssRe AssPr LocA, the mean over the 19 thresholds under
    its name and the 19 values under `<name>_alpha`; 'HOTA(0)', 'LocA(0)' and 'HOTALocA(0)' (the first threshold, and their product);
    TP / FN / FP per threshold; gt_dets and trk_dets.  A zero denominator gives 0 (LocA: 1), as TrackEval's max(1, .) does."""
    def row(c, label):
        tp, fn, fp = (np.asarray(c[k], np.float64) for k in HOTA_INT_KEYS)
        v = {'DetA': tp / np.maximum(1.0, tp + fn + fp), 'DetRe': tp / np.maximum(1.0, tp + fn), 'DetPr': tp / np.maximum(1.0, tp + fp),
             'AssA': c['ass_sum'] / np.maximum(1.0, tp), 'AssRe': c['assre_sum'] / np.maximum(1.0, tp),
             'AssPr': c['asspr_sum'] / np.maximum(1.0, tp), 'LocA': np.maximum(1e-10, c['loc_sum']) / np.maximum(1e-10, tp)}
        v['HOTA'] = np.sqrt(v['DetA'] * v['AssA'])
        r = {'class': label, 'gt_dets': int(c['gt_dets']), 'trk_dets': int(c['trk_dets']), **{k: [int(x) for x in c[k]] for k in HOTA_INT_KEYS}}
        for k in HOTA_RATIOS:
            r[k], r[k + '_alpha'] = float(np.mean(v[k])), [float(x) for x in v[k]]
        r['HOTA(0)'], r['LocA(0)'] = float(v['HOTA'][0]), float(v['LocA'][0])
        r['HOTALocA(0)'] = r['HOTA(0)'] * r['LocA(0)']
        return r

    nc = len(np.atleast_1d(counts['gt_dets']))
    per = [row({k: np.asarray(v)[c] for k, v in counts.items()}, names[c] if names is not None else c) for c in range(nc)]
    return {'all': row({k: np.asarray(v).sum(0) for k, v in counts.items()}, 'all'), 'per_class': per}


def hota_table(summary, title=''):
    """hota_summary's rows as TrackEval prints them (percentages)."""
    cols = HOTA_RATIOS + ('HOTA(0)', 'LocA(0)', 'HOTALocA(0)')
    lines = [f'{title or "class":>16s}' + ''.join(f'{c:>12s}' if '(' in c else f'{c:>8s}' for c in cols) + f'{"gt_dets":>9s}{"trk_dets":>9s}']
    for r in summary['per_class'] + [summary['all']]:
        lines.append(f'{str(r["class"]):>16s}' + ''.join(f'{100 * r[c]:12.2f}' if '(' in c else f'{100 * r[c]:8.2f}' for c in cols) +
                     f'{r["gt_dets"]:9d}{r["trk_dets"]:9d}')
    return '\n'.join(lines)


# ------------------------------------------------------------------------------------------------ track-mAP
TRACK_MAP_THRESHOLDS = (0.25, 0.5, 0.75)     # VisDrone-MOT's; np.linspace(0.5, 0.95, 10) gives TrackEval's


def track_map_thresholds(thresholds):
    """The thresholds as an f64 array, checked: 1 to 10 values in (0, 1]."""
    thr = np.asarray(thresholds, np.float64).reshape(-1)
    if not 1 <= len(thr) <= 10 or not np.all((thr > 0) & (thr <= 1)):
        raise ValueError(f'track-mAP: 1 to 10 thresholds in (0, 1] are needed, got {thresholds}')
    return thr


def track_map_new_counts(nc, thresholds=TRACK_MAP_THRESHOLDS):
    return {'score': np.zeros(0, np.float64), 'cls': np.zeros(0, np.int64), 'bits': np.zeros(0, np.int32),
            'gt_tracks': np.zeros(int(nc), np.int64), 'thresholds': track_map_thresholds(thresholds)}


def track_map_add_counts(a, b):
    """Counts of several sequences (or runs) add: the rows are concatenated in order and gt_tracks add."""
    if not np.array_equal(a['thresholds'], b['thresholds']):
        raise ValueError('track-mAP: the counts were made with different thresholds')
    out = {k: np.concatenate([a[k], b[k]]) for k in ('score', 'cls', 'bits')}
    out.update({'gt_tracks': a['gt_tracks'] + b['gt_tracks'], 'thresholds': a['thresholds']})
    return out


def track_map_since(run, before):
    """The counts that `run` holds beyond `before`, an earlier reading of the same run: what the sequences ended in between added."""
    n = len(before['score'])
    out = {k: run[k][n:] for k in ('score', 'cls', 'bits')}
    out.update({'gt_tracks': run['gt_tracks'] - before['gt_tracks'], 'thresholds': run['thresholds']})
    return out


def track_map_evaluate(sequences, nc, iou=0.5, thresholds=TRACK_MAP_THRESHOLDS, detail=None):
    """Track-mAP counts of tracker output against ground truth (TrackEval's TrackMAP for boxes, restated, with no area or time ranges and
    no cap on tracks; the rule is written out in csrc/trackmap.hip, whose checker this is, and this is the path for a machine without a
    GPU).  Arguments as mot_evaluate; a track row may carry a seventh column, its score ([k, 6] rows have score 1); `iou` is the
    threshold of the region / distractor preprocessing, which is mot_evaluate's.  A ground-truth identity's dense row is its place in
    the order of first appearance within the sequence.
    -> {'score' f64 [n], 'cls' i64 [n], 'bits' i32 [n]: one row per track identity of the run (sequences in order, classes in order,
    then score descending and id ascending), bit a = matched at thresholds[a]; 'gt_tracks' i64 [nc]; 'thresholds' f64}.  Counts of
    several sequences add (track_map_add_counts) and track_map_summary turns them into AP / AR.
    detail: a list that receives, per sequence, {'iou': {(dense row, (cls, id)): IoU}, 'mean': {(cls, id): score}, 'gaps': [best minus
    second-best IoU of every greedy step with two candidates]} - what tests/trackmap_cases.margins reads."""
    nc, thr, ts = int(nc), float(iou), track_map_thresholds(thresholds)
    out = track_map_new_counts(nc, ts)
    score, cls, bits = [], [], []
    for frames in sequences:
        rows, garea, tarea, tscore, tframes, inter = {}, {}, {}, {}, {}, {}
        for gt, trk in frames:
            g, gcls, trk, tcls = _mot_preprocess(gt, trk, nc, thr)
            sc = trk[:, 6].astype(np.float64) if trk.shape[1] == 7 else np.ones(len(trk))
            area = lambda b: (b[:, 2].astype(np.float64) - b[:, 0]) * (b[:, 3].astype(np.float64) - b[:, 1])   # noqa: E731
            ga, ta = area(g), area(trk)
            gid = [rows.setdefault((int(c), int(i)), len(rows)) for c, i in zip(gcls, g[:, 4])]
            tid = [(int(c), int(i)) for c, i in zip(tcls, trk[:, 4])]
            for k, a in zip(gid, ga):
                garea[k] = garea.get(k, 0.0) + a
            for k, a, s in zip(tid, ta, sc):
                tarea[k], tscore[k], tframes[k] = tarea.get(k, 0.0) + a, tscore.get(k, 0.0) + s, tframes.get(k, 0) + 1
            _, it = mot_iou_matrix(g[:, :4], trk[:, :4])
            for i, j in zip(*np.nonzero((it > 0) & (gcls[:, None] == tcls[None, :]))):
                inter[(gid[i], tid[j])] = inter.get((gid[i], tid[j]), 0.0) + it[i, j]
        ious = {}
        for (g, t), v in inter.items():
            union = (garea[g] + tarea[t]) - v
            ious[(g, t)] = v / union if union > 0 else 0.0
        mean = {t: tscore[t] / tframes[t] for t in tscore}
        gaps = []
        for c in range(nc):
            gts = sorted(r for (k, _), r in rows.items() if k == c)
            order = sorted((t for t in mean if t[0] == c), key=lambda t: (-mean[t], t[1]))
            word = np.zeros(len(order), np.int32)
            for a, th in enumerate(ts):
                taken = set()
                for n, t in enumerate(order):
                    best, choice = min(th, 1 - 1e-10), None
                    for g in gts:
                        v = ious.get((g, t), 0.0)
                        if g not in taken and v >= best - HOTA_EPS:
                            best, choice = v, g
                    if detail is not None:
                        cand = sorted((ious.get((g, t), 0.0) for g in gts if g not in taken), reverse=True)
                        if len(cand) > 1 and cand[1] > 0:
                            gaps.append(cand[0] - cand[1])
                    if choice is not None:
                        taken.add(choice)
                        word[n] |= 1 << a
            score += [mean[t] for t in order]
            cls += [c] * len(order)
            bits += word.tolist()
            out['gt_tracks'][c] += len(gts)
        if detail is not None:
            detail.append({'iou': ious, 'mean': mean, 'gaps': gaps})
    out.update({'score': np.asarray(score, np.float64), 'cls': np.asarray(cls, np.int64), 'bits': np.asarray(bits, np.int32)})
    return out


def track_map_accumulate(counts):
    """The run's AP and AR per threshold and class from track_map_evaluate's counts: coco_accumulate on one range and one cut.
    -> ap, ar f64 [n_thresholds, nc]; -1 for a class without ground truth."""
    n, nc, nt = len(counts['score']), len(counts['gt_tracks']), len(counts['thresholds'])
    bits, npig = np.zeros((n, 4), np.int32), np.zeros((nc, 4), np.int64)
    bits[:, 0], npig[:, 0] = counts['bits'], counts['gt_tracks']
    precision, recall = coco_accumulate(np.asarray(counts['score'], np.float64), np.asarray(counts['cls'], np.float64), bits, np.zeros(n, np.int32),
                                        npig, nc, (1,))
    ap = np.where(precision[:, 0] > -1, precision.sum(1) / 101.0, -1.0)
    return ap[:nt, :, 0, 0].copy(), recall[:nt, :, 0, 0].copy()


def track_map_rows(ap, ar, gt_tracks, tracks, thresholds, names=None):
    """ap, ar f64 [n_thresholds, nc] (-1 without ground truth), gt_tracks and tracks [nc] -> {'all': row, 'per_class': [row, ...],
    'thresholds'}: a row holds AP (the mean over the thresholds), AP_thr and AR_thr (lists), gt_tracks and tracks; the 'all' row holds the
    means over the classes that have ground truth (-1 when none has) and the summed counts.  The host and the device path both end here."""
    ap, ar = np.asarray(ap, np.float64), np.asarray(ar, np.float64)
    has = np.asarray(gt_tracks) > 0
    per = [{'class': names[c] if names is not None else c, 'AP': float(ap[:, c].mean()) if has[c] else -1.0,
            'AP_thr': [float(x) for x in ap[:, c]], 'AR_thr': [float(x) for x in ar[:, c]], 'gt_tracks': int(gt_tracks[c]),
            'tracks': int(tracks[c])} for c in range(ap.shape[1])]
    mean = lambda x: [float(v) for v in x[:, has].mean(1)] if has.any() else [-1.0] * x.shape[0]   # noqa: E731
    row = {'class': 'all', 'AP': float(np.mean([r['AP'] for r, h in zip(per, has) if h])) if has.any() else -1.0, 'AP_thr': mean(ap),
           'AR_thr': mean(ar), 'gt_tracks': int(np.sum(gt_tracks)), 'tracks': int(np.sum(tracks))}
    return {'all': row, 'per_class': per, 'thresholds': [float(t) for t in thresholds]}


def track_map_summary(counts, names=None):
    """Per-class rows and an 'all' row (track_map_rows) from track_map_evaluate's (or TrackMapEvaluator's) counts."""
    ap, ar = track_map_accumulate(counts)
    nc = len(counts['gt_tracks'])
    return track_map_rows(ap, ar, counts['gt_tracks'], np.bincount(np.asarray(counts['cls'], np.int64), minlength=nc)[:nc], counts['thresholds'], names)


def track_map_table(summary, title=''):
    """track_map_summary's rows as a table (percentages; a class without ground truth shows -100)."""
    ts = summary['thresholds']
    lines = [f'{title or "class":>16s}{"AP":>8s}' + ''.join(f'{"AP@%.2f" % t:>9s}' for t in ts) + ''.join(f'{"AR@%.2f" % t:>9s}' for t in ts) +
             f'{"gt_tracks":>10s}{"tracks":>8s}']
    for r in summary['per_class'] + [summary['all']]:
        lines.append(f'{str(r["class"]):>16s}{100 * r["AP"]:8.2f}' + ''.join(f'{100 * v:9.2f}' for v in r['AP_thr'] + r['AR_thr']) +
                     f'{r["gt_tracks"]:10d}{r["tracks"]:8d}')
    return '\n'.join(lines)


def cm_conf(conf):
    """The confusion matrix's confidence threshold from the validator's: 0.25 when that is None or the default 0.001 (metrics.py:818)."""
    return 0.25 if conf in (None, 0.001) else conf


def _int_classes(c, nc):
    """`.int()` of a float class vector with the range check done in float -> (indices int64, in-range mask).  NaN, +-inf and anything
    that truncates outside [0, nc) is out of range."""
    t = torch.trunc(c.float())
    ok = (t >= 0) & (t < nc)
    return t[ok].long().numpy(), ok


class ConfusionMatrix:
    """The reference's detection ConfusionMatrix (utils/metrics.py:801-888) on CPU tensors, vectorised; the statement of the rule that
    csrc/confusion.hip implements, its checker, and the host validator's path.  matrix int64 [nc + 1, nc + 1]: row = predicted,
    column = true, index nc = background.
    Per image: the detections with score > conf take part; IoU = box_iou(labels, detections), class-agnostic; a pair is a candidate when
    iou > iou_thres; L(d) = the candidate label of highest IoU of detection d; D(l) = among the detections with L(d) == l the one of
    highest IoU.  A label with a D(l) counts at [cls(D(l)), gc(l)], every other label at [nc, gc(l)]; a passing detection that is
    nobody's D(l) counts at [cls(d), nc] - but ONLY IF the image has at least one matched pair (the reference's `if n:`, kept on
    purpose).  The caller skips images without labels, as the reference does, so their detections are counted nowhere.
    Where the reference leaves the order of equal IoUs to numpy's argsort, this project defines it: the LOWER label index wins in L, the
    LOWER detection row wins in D.  A label or detection whose class is outside [0, nc) is removed first and counted nowhere (the
    reference would index out of range)."""

    def __init__(self, nc, conf=0.25, iou_thres=0.45):
        if not iou_thres >= 0:
            raise ValueError('ConfusionMatrix: iou_thres must be >= 0')
        self.nc, self.conf, self.iou_thres = int(nc), cm_conf(conf), iou_thres
        self.matrix = np.zeros((self.nc + 1, self.nc + 1), dtype=np.int64)

    def process_batch(self, detections, labels):
        """detections [N, 6] xyxy conf cls and labels [M, 5] cls xyxy of one image; or detections None and labels [M] classes (an image
        without detections: every label is a background miss)."""
        nc = self.nc
        if detections is None:
            gc, _ = _int_classes(labels.detach().cpu().reshape(-1), nc)
            np.add.at(self.matrix[nc], gc, 1)
            return
        det, lab = detections.detach().float().cpu(), labels.detach().float().cpu()
        det = det[det[:, 4] > self.conf]
        dc, ok = _int_classes(det[:, 5], nc)
        det = det[ok]
        gc, ok = _int_classes(lab[:, 0], nc)
        lab = lab[ok]
        nl, nd = lab.shape[0], det.shape[0]
        has, D = np.zeros(nl, bool), np.zeros(nl, np.int64)
        if nl and nd:
            iou = box_iou(lab[:, 1:], det[:, :4])
            v = torch.where(iou > self.iou_thres, iou, torch.full_like(iou, -1.0)).numpy()      # [nl, nd]; NaN fails the comparison
            L = v.argmax(0)                               # the first maximum: the LOWER label index among equal IoUs
            best = v[L, np.arange(nd)]
            claim = np.full((nl, nd), -1.0, np.float32)   # claim[l, d] = iou(l, d) where L(d) == l
            mine = best > -1.0
            claim[L[mine], np.nonzero(mine)[0]] = best[mine]
            D = claim.argmax(1)                           # the first maximum: the LOWER detection row among equal IoUs
            has = claim[np.arange(nl), D] > -1.0
        np.add.at(self.matrix, (dc[D[has]], gc[has]), 1)
        np.add.at(self.matrix[nc], gc[~has], 1)
        if has.any():
            free = np.ones(nd, bool)
            free[D[has]] = False
            np.add.at(self.matrix[:, nc], dc[free], 1)

    def tp_fp(self):
        """True and false positives per class (background dropped)."""
        tp = self.matrix.diagonal()
        return tp[:-1], (self.matrix.sum(1) - tp)[:-1]

    def normalized(self):
        """Every column divided by its sum + 1e-9, as the reference's plot normalises."""
        return self.matrix / (self.matrix.sum(0).reshape(1, -1) + 1e-9)


class Validator:
    """Accumulates (correct, conf, pred_cls, target_cls) over batches and reduces to mp, mr, mAP50, mAP50-95.
    confusion: also keep the reference's confusion matrix (ConfusionMatrix above, called where RTDETRValidator.update_metrics calls it);
    results() then carries 'confusion_matrix'.  nc: its class count, taken from the first prediction when None.
    coco: also keep every image's native-space rows and labels; results() then carries 'coco', the COCO-protocol numbers of
    coco_evaluate (AP, AP50, AP75, APs, APm, APl, AR1, AR10, AR100, ARs, ARm, ARl, max_dets, per_class) with the cuts coco_max_dets."""

    def __init__(self, imgsz=640, conf=0.001, iou=0.7, single_cls=False, confusion=False, nc=None, coco=False, coco_max_dets=(1, 10, 100)):
        self.imgsz, self.conf, self.iou, self.single_cls = imgsz, conf, iou, single_cls
        self.stats, self.seen = [], 0
        self.confusion, self.nc, self.confusion_matrix = confusion, nc, None
        self.coco, self.coco_max_dets, self._coco_images = coco, coco_cuts(coco_max_dets) if coco else tuple(coco_max_dets), []

    def _coco_image(self, pred, cls, bbox, shape):
        """(predn [n, 6], labelsn [m, 5]) of one image as numpy, computed as update() computes them."""
        predn = pred.clone()
        if self.single_cls:
            predn[:, 5] = 0
        predn[..., [0, 2]] *= shape[1] / self.imgsz
        predn[..., [1, 3]] *= shape[0] / self.imgsz
        tbox = xywh2xyxy(bbox)
        tbox[..., [0, 2]] *= shape[1]
        tbox[..., [1, 3]] *= shape[0]
        return predn.float().cpu().numpy(), torch.cat((cls, tbox), 1).cpu().numpy()

    @torch.no_grad()
    def update(self, preds, batch):
        y = preds[0] if isinstance(preds, (list, tuple)) else preds
        dev = y.device
        iouv = IOUV.to(dev)
        if self.confusion and self.confusion_matrix is None:
            self.nc = y.shape[-1] - 4 if self.nc is None else self.nc
            self.confusion_matrix = ConfusionMatrix(self.nc, self.conf)
        if self.coco and self.nc is None:
            self.nc = y.shape[-1] - 4
        for si, pred in enumerate(postprocess(preds, self.imgsz, self.conf, self.iou, self.single_cls)):
            idx = batch['batch_idx'].view(-1).to(dev) == si
            cls = batch['cls'].to(dev).view(-1, 1)[idx].float()
            bbox = batch['bboxes'].to(dev)[idx].float()
            shape = batch['ori_shape'][si] if 'ori_shape' in batch else (self.imgsz, self.imgsz)
            nl, npr = cls.shape[0], pred.shape[0]
            correct = torch.zeros(npr, iouv.numel(), dtype=torch.bool, device=dev)
            self.seen += 1
            if self.coco:
                self._coco_images.append(self._coco_image(pred, cls, bbox, shape))
            if npr == 0:
                if nl:
                    self.stats.append((correct, torch.zeros(0, device=dev), torch.zeros(0, device=dev), cls.squeeze(-1)))
                    if self.confusion:
                        self.confusion_matrix.process_batch(None, cls.squeeze(-1))
                continue
            if self.single_cls:
                pred[:, 5] = 0
            predn = pred.clone()
            predn[..., [0, 2]] *= shape[1] / self.imgsz
            predn[..., [1, 3]] *= shape[0] / self.imgsz
            if nl:
                tbox = xywh2xyxy(bbox)
                tbox[..., [0, 2]] *= shape[1]
                tbox[..., [1, 3]] *= shape[0]
                labelsn = torch.cat((cls, tbox), 1)
                correct = process_batch(predn.float(), labelsn, iouv)
                if self.confusion:
                    self.confusion_matrix.process_batch(predn, labelsn)
            self.stats.append((correct, pred[:, 4], pred[:, 5], cls.squeeze(-1)))

    def results(self, curves=False):
        """curves: the dict also carries 'curves' (ap_per_class's curves as nested lists, plus 'classes'; {} when there is nothing to reduce)."""
        extra = {}
        if self.confusion:
            extra['confusion_matrix'] = self.confusion_matrix.matrix.tolist() if self.confusion_matrix is not None else []
        if curves:
            extra['curves'] = {}
        if self.coco:
            extra['coco'] = coco_evaluate(self._coco_images, self.nc or 0, self.coco_max_dets)['summary']
        if not self.stats:
            return {'precision': 0.0, 'recall': 0.0, 'mAP50': 0.0, 'mAP50-95': 0.0, 'seen': self.seen, **extra}
        stats = [torch.cat(x, 0).cpu().numpy() for x in zip(*self.stats)]
        if not stats[0].any():
            return {'precision': 0.0, 'recall': 0.0, 'mAP50': 0.0, 'mAP50-95': 0.0, 'seen': self.seen, **extra}
        _, _, p, r, _, ap, classes, *cv = ap_per_class(*stats, curves=curves)
        if curves:
            extra['curves'] = curves_as_lists(cv[0], classes)
        return {'precision': float(p.mean()), 'recall': float(r.mean()), 'mAP50': float(ap[:, 0].mean()),
                'mAP50-95': float(ap.mean()), 'seen': self.seen, **extra}


_EMPTY = {'precision': 0.0, 'recall': 0.0, 'mAP50': 0.0, 'mAP50-95': 0.0}


def _cat(xs, shape, dt):
    return np.concatenate(xs) if xs else np.zeros(shape, dt)


def _batch_labels(lab_cls, lab_off, B, first):
    """One batch's labels grouped by image - host arrays, or the host copy of device ones, where lab_off[0] .. lab_off[B] may be a
    slice of a larger upload - with `first` the run's index of its first image -> target_cls [m], target_image [m]."""
    return lab_cls[lab_off[0]:lab_off[B]], first + np.repeat(np.arange(B), np.diff(lab_off[:B + 1]))


class DeviceValidator:
    """Validator with the per-image work on the device: update() is ops.val_postprocess_match (one launch per batch, csrc/valmatch.hip)
    plus list appends - no synchronisation; results() does one concatenation and one device-to-host copy for the whole run and feeds
    the same ap_per_class.  Its dict equals Validator's key for key (on the model output widened to fp32) and adds 'per_class':
    [{class, images, instances, precision, recall, mAP50, mAP50-95}] for the classes that have labels (the reference's print_results
    table).  save_json: also collect the reference's pred_to_json records (models/yolo/detect/val.py:231-242; the batch must carry
    'im_file'); class_map maps a class index to the record's category_id (default: the index).
    confusion: update() makes one more launch per batch (ops.val_confusion, csrc/confusion.hip) on the outputs and the uploaded labels
    of the first, adding into one device matrix - still nothing synchronises; results() then carries 'confusion_matrix' (nested lists
    of ints, equal to Validator's), which rides in the run's one device-to-host copy.  nc: its class count, from the first prediction
    when None.
    device_metrics: results() reduces on the device as well: ops.val_ap_curves (two stable sorts and one launch, csrc/metrics.hip) leaves
    AP per class and threshold and the P / R / PR curves in one packed buffer, and the run's one device-to-host copy carries that buffer
    (plus the confusion matrix and device-side labels) instead of every row: 8 * (3010 * nc) + 8 * nc bytes, whatever the number of
    rows.  The order of equal confidences is then the defined one (ap_per_class(stable=True)); F1, the operating confidence and the
    dict come from the same host lines.  Classes are the label classes inside [0, nc).  save_json keeps the row copy for its records.
    coco: update() makes one more launch per batch (ops.val_coco_match, csrc/cocoeval.hip) on the outputs and the uploaded labels of
    the first (the upload confusion=True shares), leaving the COCO match bits and ranks of every row on the device and adding into one
    device table of ground-truth counts - still nothing synchronises; results() launches ops.val_coco_accumulate once and carries
    'coco' (coco_summary's dict with the cuts coco_max_dets, equal to Validator's).  The run's one device-to-host copy gains ap_tkam,
    recall and the count table, 8 * (80 * nc * len(coco_max_dets)) + 16 * nc bytes; the precision array stays on the device."""

    def __init__(self, imgsz=640, conf=0.001, iou=0.7, single_cls=False, save_json=False, class_map=None, names=None, confusion=False,
                 nc=None, device_metrics=False, coco=False, coco_max_dets=(1, 10, 100)):
        self.imgsz, self.conf, self.iou, self.single_cls = imgsz, conf, iou, single_cls
        self.save_json, self.class_map, self.names = save_json, class_map, names
        self.batches, self.files, self.seen = [], [], 0
        self.jdict = []
        self._reduced = None
        self.confusion, self.nc = confusion, nc
        self._matrix, self._matrix_host = None, None   # i32 [nc + 1, nc + 1] on the device; its copy after _reduce()
        self.device_metrics, self._ncls, self._reduced_dev = device_metrics, nc, None
        self.coco, self.coco_max_dets = coco, coco_cuts(coco_max_dets) if coco else tuple(coco_max_dets)
        self._coco_batches, self._npig, self._coco_host = [], None, None   # (bits, rank) per batch; i32 [nc, 4] on the device; the dict

    @torch.no_grad()
    def update(self, preds, batch):
        from . import ops
        y = preds[0] if isinstance(preds, (list, tuple)) else preds
        out = ops.val_postprocess_match(y, batch['cls'], batch['bboxes'], batch['batch_idx'], batch.get('ori_shape'), self.imgsz, self.conf,
                                        self.iou, self.single_cls, return_device_labels=self.confusion or self.coco)
        self.batches.append(out[:5])
        if self.confusion:
            if self._matrix is None:
                self.nc = y.shape[-1] - 4 if self.nc is None else self.nc
                self._matrix = torch.zeros(self.nc + 1, self.nc + 1, dtype=torch.int32, device=y.device)
            ops.val_confusion(out[0], out[2], out[5], self.nc, cm_conf(self.conf), 0.45, self._matrix)
        if self.coco:
            if self._npig is None:
                self.nc = y.shape[-1] - 4 if self.nc is None else self.nc
                self._npig = torch.zeros(self.nc, 4, dtype=torch.int32, device=y.device)
            self._coco_batches.append(ops.val_coco_match(out[0], out[2], out[5], self.nc, self.coco_max_dets[-1], self._npig))
        self.seen += y.shape[0]
        if self.save_json:
            self.files.extend(batch['im_file'])
        if self._ncls is None:
            self._ncls = y.shape[-1] - 4
        self._reduced = self._reduced_dev = None

    def _coco_parts(self):
        """coco: what the run's one device-to-host copy carries for it, as named parts - ap_tkam and recall as ops.val_coco_accumulate
        returns them (views of the head of its packed buffer; the precision array stays behind) and the ground-truth count table."""
        if not self.coco or not self._coco_batches:
            return {}
        from . import ops
        ap_tkam, recall, _ = ops.val_coco_accumulate([(b[0], c[0], c[1]) for b, c in zip(self.batches, self._coco_batches)], self._npig,
                                                     self.nc, self.coco_max_dets)
        return {'coco_ap': ap_tkam, 'coco_recall': recall, 'npig': self._npig}

    def _coco_empty(self):
        nc = self.nc or 0
        return coco_summary(-np.ones((10, nc, 4, len(self.coco_max_dets))), -np.ones((10, nc, 4, len(self.coco_max_dets))), self.coco_max_dets)

    def _take_riders(self, host):
        """What rides in either reduction's copy besides its own rows: the confusion matrix and the coco parts, by the lines the host
        path ends in."""
        if 'matrix' in host:
            self._matrix_host = host['matrix'].copy()
        if 'npig' in host:
            self._coco_host = coco_summary(host['coco_ap'], host['coco_recall'], self.coco_max_dets, host['npig'])

    def _device_labels(self):
        """The named parts of the batches whose labels live on the device."""
        return {(k, i): t for i, b in enumerate(self.batches) if isinstance(b[3], torch.Tensor) for k, t in (('lab_cls', b[3]), ('lab_off', b[4]))}

    def _labels(self, host):
        """-> the run's target_cls [m] and target_image [m]: every batch's host labels, or the copy's views of its device labels."""
        tcls, timage, first = [], [], 0
        for i, (predn, _, _, lab_cls, lab_off) in enumerate(self.batches):
            B = predn.shape[0]
            c, im = _batch_labels(host.get(('lab_cls', i), lab_cls), host.get(('lab_off', i), lab_off), B, first)
            tcls.append(c)
            timage.append(im)
            first += B
        return _cat(tcls, (0,), np.float32), _cat(timage, (0,), np.int64)

    def _reduce(self):
        """-> (predn [n, 6], correct [n, 10] bool, image [n], target_cls [m], target_image [m]) as numpy, rows in image order."""
        if self._reduced is None:
            from ._lib import to_host
            parts = {(k, i): t for i, b in enumerate(self.batches) for k, t in zip(('predn', 'correct', 'counts'), b)}
            parts.update(self._device_labels())
            if self._matrix is not None:
                parts['matrix'] = self._matrix
            if not self.device_metrics:      # (device_metrics: _reduce_device()'s copy carries them)
                parts.update(self._coco_parts())
            host = to_host(parts)            # the run's one device-to-host copy
            self._take_riders(host)
            rows, hits, image, first = [], [], [], 0
            for i in range(len(self.batches)):
                pn, co, cn = host['predn', i], host['correct', i], host['counts', i]
                live = np.arange(pn.shape[1])[None, :] < cn[:, None]
                rows.append(pn[live])
                hits.append(co[live].astype(bool))
                image.append(first + np.nonzero(live)[0])
                first += len(cn)
            self._reduced = (_cat(rows, (0, 6), np.float32), _cat(hits, (0, 10), bool), _cat(image, (0,), np.int64), *self._labels(host))
        return self._reduced

    def _reduce_device(self):
        """device_metrics: -> (the six outputs of ops.val_ap_curves as numpy, target_cls [m], target_image [m]).  One device-to-host
        copy: the packed result, the confusion matrix, and the labels of the batches whose labels live on the device."""
        if self._reduced_dev is None:
            from . import ops
            from ._lib import to_host
            nc, labs = self._ncls, []
            for _, _, _, lab_cls, lab_off in self.batches:
                if isinstance(lab_cls, torch.Tensor):     # rows outside lab_off[0] .. lab_off[B] belong to no image: class -1, counted nowhere
                    i = torch.arange(lab_cls.numel(), device=lab_cls.device)
                    lab_cls = torch.where((i >= lab_off[0]) & (i < lab_off[-1]), lab_cls, -1.0)
                labs.append(lab_cls)
            parts = {'ap': ops.val_ap_curves([b[:3] for b in self.batches], labs, nc, return_packed=True)[-1]}
            if not self.save_json:                        # (the records need the rows: _reduce()'s copy, which also brings labels and matrix)
                parts.update(self._device_labels())
                if self._matrix is not None:
                    parts['matrix'] = self._matrix
            parts.update(self._coco_parts())
            host = to_host(parts)                         # the run's one device-to-host copy
            self._take_riders(host)
            self._reduced_dev = (*ops.val_ap_split(host['ap'], nc), *(self._reduce()[3:] if self.save_json else self._labels(host)))
        return self._reduced_dev

    def _table(self, classes, p, r, ap, tcls, timage):
        """The reference's print_results table: one record per class that has labels."""
        per_class = []
        for k, c in enumerate(classes):
            mine = tcls == c
            per_class.append({'class': self.names[int(c)] if self.names is not None else int(c), 'images': int(len(np.unique(timage[mine]))),
                              'instances': int(mine.sum()), 'precision': float(p[k]), 'recall': float(r[k]), 'mAP50': float(ap[k, 0]),
                              'mAP50-95': float(ap[k].mean())})
        return per_class

    def results(self, curves=False):
        """curves: the dict also carries 'curves' (ap_per_class's curves as nested lists, plus 'classes'; {} when there is nothing to reduce)."""
        extra = {'curves': {}} if curves else {}
        stats = None      # (classes, p, r, ap, tcls, timage), unless there is nothing to reduce
        if not self.device_metrics:
            predn, correct, _, tcls, timage = self._reduce()
            if (len(predn) or len(tcls)) and correct.any():
                _, _, p, r, _, ap, classes, *cv = ap_per_class(correct, predn[:, 4], predn[:, 5], tcls, curves=curves)
                stats = classes, p, r, ap, tcls, timage
                if curves:
                    extra['curves'] = curves_as_lists(cv[0], classes)
        elif self.batches:
            ap, p_curve, r_curve, pr_curve, n_gt, n_pred, tcls, timage = self._reduce_device()
            # `no row and no label, or no hit at all` of the host path: a hit makes the precision envelope positive at recall 0, and with
            # it the class's AP; without a hit every AP is zero
            if ap.any():
                has = n_gt > 0
                classes = np.nonzero(has)[0]
                _, _, p, r, _, f1_curve = operating_point(p_curve[has], r_curve[has], n_gt[has])
                stats = classes, p, r, ap[has], tcls, timage
                if curves:
                    extra['curves'] = curves_as_lists({'px': np.linspace(0, 1, 1000), 'p': p_curve[has], 'r': r_curve[has], 'f1': f1_curve,
                                                       'pr': pr_curve[has], 'valid': n_pred[has] > 0}, classes)
        if self.coco:
            extra['coco'] = self._coco_host if self._coco_host is not None else self._coco_empty()
        if self.save_json:
            predn, _, image = self._reduce()[:3]
            self.jdict = self._records(predn, image)
        if self.confusion:
            extra['confusion_matrix'] = self._matrix_host.tolist() if self._matrix_host is not None else []
        if stats is None:
            return {**_EMPTY, 'seen': self.seen, 'per_class': [], **extra}
        _, p, r, ap = stats[:4]
        return {'precision': float(p.mean()), 'recall': float(r.mean()), 'mAP50': float(ap[:, 0].mean()), 'mAP50-95': float(ap.mean()),
                'seen': self.seen, 'per_class': self._table(*stats), **extra}

    def _records(self, predn, image):
        """pred_to_json: image_id = the file stem; bbox = top-left x, y, w, h rounded to 3; score rounded to 5."""
        box = torch.from_numpy(predn[:, :4]).clone()
        wh = box[:, 2:] - box[:, :2]
        box = torch.cat([(box[:, :2] + box[:, 2:]) / 2, wh], 1)    # xyxy2xywh (utils/ops.py:337-357) ...
        box[:, :2] -= box[:, 2:] / 2                                # ... then centre -> top-left corner
        out = []
        for i, p, b in zip(image.tolist(), predn.tolist(), box.tolist()):
            c = int(p[5])
            out.append({'image_id': os.path.splitext(os.path.basename(self.files[i]))[0],
                        'category_id': self.class_map[c] if self.class_map is not None else c,
                        'bbox': [round(x, 3) for x in b], 'score': round(p[4], 5)})
        return out

    def write_json(self, path):
        """Write the collected records as the reference's predictions.json; `path`: the file, or the run folder."""
        if not self.save_json:
            raise ValueError('DeviceValidator(save_json=True) collects the records write_json() writes')
        if self._reduced is None or not self.jdict:
            predn, _, image, _, _ = self._reduce()
            self.jdict = self._records(predn, image)
        path = os.path.join(path, 'predictions.json') if os.path.isdir(path) else path
        with open(path, 'w') as f:
            json.dump(self.jdict, f)
        return path


@torch.no_grad()
def validate(model, batches, imgsz=640, conf=0.001, iou=0.7, autocast_dtype=None, on_device=False, save_json=None, names=None,
             confusion=False, device_metrics=False, curves=False, coco=False, coco_max_dets=(1, 10, 100), augment=False, tta_views=None):
    """model in eval mode over an iterable of batches -> metric dict (valTAMTR.py's flow without the dataset plumbing).
    on_device: postprocess and label matching in one HIP launch per batch (DeviceValidator; the dict then also carries 'per_class');
    save_json (a file or folder path, needs on_device): also write the reference's predictions.json there.
    confusion: the dict also carries 'confusion_matrix' ([nc + 1][nc + 1] ints, row = predicted, column = true, last = background).
    device_metrics (needs on_device): AP and the curves are reduced on the device too (DeviceValidator(device_metrics=True)).
    curves: the dict also carries 'curves' (the reference's P / R / F1 / PR curves; see ap_per_class).
    coco: the dict also carries 'coco', the COCO-protocol AP / AR by object size with the cuts coco_max_dets (coco_evaluate on the host
    path, csrc/cocoeval.hip with on_device); it needs nothing beyond the path it selects.
    augment: test-time augmentation (the reference's `augment`, engine/validator.py:109,169; tta.py): every batch's predictions become
    tta.tta_forward's merged tensor over tta_views (default tta.DEFAULT_VIEWS) before either validator sees them, so the confusion
    matrix, COCO and save_json ride along unchanged; the dict then carries 'tta_dropped', the merged rows beyond 512 per image (read
    once, after the last batch)."""
    if save_json and not on_device:
        raise ValueError('validate(save_json=...) needs on_device=True: the records come from the device path')
    if device_metrics and not on_device:
        raise ValueError('validate(device_metrics=True) needs on_device=True: the reduction reads what the device path keeps')
    was_training = model.training
    model.eval()
    v = (DeviceValidator(imgsz, conf, iou, save_json=bool(save_json), names=names, confusion=confusion, device_metrics=device_metrics,
                         coco=coco, coco_max_dets=coco_max_dets) if on_device
         else Validator(imgsz, conf, iou, confusion=confusion, coco=coco, coco_max_dets=coco_max_dets))
    if augment:
        from . import tta
        views, dropped = tta.check_views(tta.DEFAULT_VIEWS if tta_views is None else tta_views), []
    for batch in batches:
        img = batch['img']
        if augment:
            preds, _, _, drop = tta.tta_forward(model, img, batch.get('txt_feats'), views, conf, iou, autocast_dtype=autocast_dtype)
            dropped.append(drop)
        else:
            with torch.autocast(img.device.type, dtype=autocast_dtype or torch.bfloat16, enabled=autocast_dtype is not None):
                preds = model(img, txt_feats=batch.get('txt_feats'))
        v.update(preds, batch)
    model.train(was_training)
    res = v.results(curves=True) if curves else v.results()
    if augment:
        res['tta_dropped'] = int(torch.cat(dropped).sum()) if dropped else 0
    if save_json:
        res['json'] = v.write_json(save_json)
    return res


# ------------------------------------------------------------------------------------------------ the epoch loop
def fitness(metrics):
    """0.1 * mAP50 + 0.9 * mAP50-95 (utils/metrics.py:1252-1256)."""
    return 0.1 * metrics['mAP50'] + 0.9 * metrics['mAP50-95']


def fit(model, train_loader, prepare, epochs, val_loader=None, lr0=1e-4, lrf=1.0, momentum=0.9, weight_decay=1e-4, optimizer='AdamW',
        warmup_iters=2000, warmup_bias_lr=0.1, warmup_momentum=0.8, close_mosaic=0, imgsz=640, reducer=None, rank=0, world=1,
        save_dir=None, max_steps=None, log=None, resume=None, static_graph=False, val_on_device=False, val_device_metrics=False):
    """Train `model` for `epochs` passes over train_loader; defaults are the reference's shipped hyper-parameters
    (cfg/default.yaml:23,84-90; this fork sets nbs = batch, so there is no gradient accumulation and weight decay is unscaled, and
    reads warmup_epochs as an iteration count: trainer.py:263-265,294).

    prepare(batch, training) -> batch on the device (data.preprocess_batch with the prompt table bound).  reducer: dist.GradReducer for
    world > 1 - gradients are SUMMED over ranks, which is the reference's mean-reduce of a loss pre-multiplied by world_size
    (trainer.py:346-347).  Rank 0 validates the EMA weights after every epoch and keeps last.pt / best.pt under save_dir.
    resume: a checkpoint dict written by an earlier fit() ({'epoch', 'best_fitness', 'model', 'ema', 'updates', 'optimizer'}; the caller
    has loaded 'model'): EMA weights and update count, optimizer state, the best fitness so far and the epoch counter continue from it
    (trainer.py:593-615), so the warm-up does not start over, best.pt is only replaced by a better epoch, and a run that resumes inside
    its last `close_mosaic` epochs starts with mosaic already closed.  static_graph: record trunk + VSS blocks + input projection as HIP graphs on the first batch
    (model.capture_static_part; batches of another shape, and evaluation, run eagerly).  val_on_device: the per-epoch validation runs its
    postprocess and label matching on the device (validate(on_device=True)); the record then also holds 'per_class'.  val_device_metrics (with val_on_device): its AP reduction
    runs on the device too (validate(device_metrics=True)).  Returns the per-epoch records."""
    nb = len(train_loader)
    if nb == 0:   # e.g. drop_last with fewer samples per rank than the batch size: the loop below would 'train' for zero steps without a word
        raise ValueError(f'fit(): the training loader yields no batches ({len(train_loader.dataset)} samples, batch size {train_loader.batch_size}, '
                         f'drop_last={getattr(train_loader, "drop_last", None)})')
    opt = build_optimizer(model, name=optimizer, lr=lr0, momentum=momentum, decay=weight_decay,
                          iterations=math.ceil(len(train_loader.dataset) / max(train_loader.batch_size or 1, 1)) * epochs)
    lf = linear_lr(epochs, lrf)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=lf)
    ema = ModelEMA(model) if rank == 0 else None
    # clip + optimizer step + EMA as one table-driven launch group when the combination is served (AdamW, fp32 parameters on the GPU)
    stepper = FusedOptimStep.create(model, opt, ema, max_norm=0.1, shadows=getattr(model, 'autocast_dtype', None) == torch.bfloat16)
    history, best, steps, start = [], None, 0, 0
    if resume is not None:
        start = int(resume.get('epoch', -1)) + 1
        if 'optimizer' in resume:
            opt.load_state_dict(resume['optimizer'])
        if ema is not None and 'ema' in resume:
            ema.ema.load_state_dict(resume['ema'])
            ema.updates = int(resume.get('updates', 0))
        best = resume.get('best_fitness', resume.get('metrics', {}).get('fitness'))  # (second form: checkpoints written before round 3)
        for _ in range(start):
            sched.step()
    mosaic_open = bool(close_mosaic) and hasattr(train_loader.dataset, 'close_mosaic')

    def shut_mosaic():
        train_loader.dataset.close_mosaic()
        from .data import reset_workers
        reset_workers(train_loader)     # persistent workers keep their own copy of the dataset

    if mosaic_open and resume is not None and start > epochs - close_mosaic:   # RESUMED past the switch-over epoch (trainer.py:593-594,617: not a fresh run)
        shut_mosaic()
        mosaic_open = False
    for epoch in range(start, epochs):
        model.train()
        if hasattr(train_loader.sampler, 'set_epoch'):
            train_loader.sampler.set_epoch(epoch)
        if mosaic_open and epoch == epochs - close_mosaic:   # trainer.py:315 tests equality: a run shorter than close_mosaic never closes it
            shut_mosaic()
            mosaic_open = False
        t0, mean_items, waited, i = time.time(), None, 0.0, -1
        opt.zero_grad(set_to_none=True)
        batches = iter(train_loader)
        while True:
            t1 = time.perf_counter()
            batch = next(batches, None)
            waited += time.perf_counter() - t1        # host time blocked on the loader (0 when the workers keep ahead)
            if batch is None:
                break
            i += 1
            warmup(opt, i + nb * epoch, warmup_iters, lf(epoch), warmup_bias_lr, warmup_momentum, momentum)
            batch = prepare(batch, True)
            if static_graph and getattr(model, '_static', None) is None and batch['img'].is_cuda and hasattr(model, 'capture_static_part'):
                static_graph = False   # one attempt
                try:
                    model.capture_static_part(batch['img'], batch['txt_feats'], log=log)   # replays are checked against eager execution
                except Exception as e:  # noqa: BLE001 - training goes on eagerly; say so
                    model.release_static_part()
                    if log:
                        log(f'static part not captured ({type(e).__name__}: {e}); running eagerly')
            if reducer is not None:
                reducer.prepare()
            loss, items = model(batch)
            loss.backward()
            if reducer is not None:
                reducer.finish()
            if stepper is not None:  # clip + AdamW + EMA in four launches (csrc/optim.hip)
                stepper.step()
            else:
                torch.nn.utils.clip_grad_norm_([p for p in model.parameters() if p.grad is not None], max_norm=0.1)
                opt.step()
            if reducer is None:      # (the reducer's gradients are views of its flat buckets, zeroed by prepare())
                opt.zero_grad(set_to_none=True)
            if ema is not None and stepper is None:
                ema.update(model)
            mean_items = items.detach() if mean_items is None else (mean_items * i + items.detach()) / (i + 1)   # no host sync
            steps += 1
            if max_steps is not None and steps >= max_steps:
                break
        rec = {'epoch': epoch, 'steps': steps, 'seconds': time.time() - t0, 'loader_wait': waited, 'lr': [g['lr'] for g in opt.param_groups],
               'loss_items': mean_items.float().cpu().tolist() if mean_items is not None else []}
        sched.step()
        if rank == 0:
            if val_loader is not None:
                rec.update(validate(ema.ema, (prepare(b, False) for b in val_loader), imgsz=imgsz,
                                    autocast_dtype=getattr(model, 'autocast_dtype', None), on_device=val_on_device,
                                    device_metrics=val_device_metrics))
                rec['fitness'] = fitness(rec)
            if save_dir is not None:
                os.makedirs(save_dir, exist_ok=True)
                is_best = val_loader is not None and (best is None or rec['fitness'] >= best)
                if is_best:
                    best = rec['fitness']
                ckpt = {'epoch': epoch, 'best_fitness': best, 'model': model.state_dict(), 'ema': ema.ema.state_dict(), 'updates': ema.updates,
                        'optimizer': opt.state_dict(), 'metrics': {k: v for k, v in rec.items() if isinstance(v, float)}}
                torch.save(ckpt, os.path.join(save_dir, 'last.pt'))
                if is_best:
                    torch.save(ckpt, os.path.join(save_dir, 'best.pt'))
            if log:
                log(rec)
        history.append(rec)
        if max_steps is not None and steps >= max_steps:
            break
    return history
