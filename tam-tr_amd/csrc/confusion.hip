// confusion.hip - the validator's confusion matrix for a whole batch in one launch (tamtr_val_confusion).
//
// Replaces the per-image ConfusionMatrix.process_batch (ultralytics/utils/metrics.py:833-877) as RTDETRValidator.update_metrics calls it
// (ultralytics/models/rtdetrworld/val.py:141-165): IoU matrix, torch.where, a copy to the host, two numpy sorts, two np.unique and a
// Python loop over labels and detections, per image.  Here the kernel reads what tamtr_val_postprocess_match left on the device
// (predn, counts) and the same grouped labels, and adds into one integer matrix that stays on the device for the whole run.
//
// The rule.  Mx is [nc + 1, nc + 1], row = predicted, column = true, index nc = background.  Contract: exact integer equality with
// engine.ConfusionMatrix on CPU fp32 tensors; the IoU has the bits of engine.box_iou (the object is compiled with -ffp-contract=off).
// Per image, with npr = counts[b] rows of predn and nl labels:
//   labels   converted as valmatch.hip step 6: xywh -> xyxy on the normalised values, then x *= lw = fp32(w_orig), y *= lh = fp32(h_orig)
//   classes  truncated towards zero as `.int()` does.  A label or a detection whose class is outside [0, nc) (or NaN) is removed
//            before anything else and counted nowhere (the reference would index out of range; this is the project's definition).
//            Under single_cls the detection classes in predn are already 0 and label classes are left as they are.
//   1. npr == 0: every label adds Mx[nc, gc] += 1.
//   2. npr > 0 and nl == 0: NOTHING is added.  The reference calls process_batch only inside `if nl:`, so detections on an image
//      without labels are not counted as false positives (kept on purpose).
//   3. otherwise the detections with score > cm_conf (fp32) take part;
//      IoU      engine.box_iou(labels, dets) = inter / (((area_l + area_d) - inter) + fp32(1e-7)), CLASS-AGNOSTIC
//      pair     candidate when iou > iou_thres, strict, fp32; a NaN IoU never qualifies
//      L(d)     the candidate label of highest IoU of detection d
//      D(l)     among the detections with L(d) == l, the one of highest IoU
//      Tie rule: the reference's two argsort()[::-1] + np.unique(return_index) passes leave the order of equal IoUs unspecified; here the
//      LOWER label index wins in L and the LOWER detection row wins in D.
//   4. a label with a D(l) adds Mx[cls(D(l)), gc(l)] += 1; every other label adds Mx[nc, gc(l)] += 1.
//   5. ONLY IF the image has at least one matched pair, every confidence-passing detection that is nobody's D(l) adds
//      Mx[cls(d), nc] += 1 (the reference's `if n:`): an image whose detections all miss contributes no false positives (kept on purpose).
//   Cases 1 and 2 are case 3 with no detection / no label; the kernel has one path.
//   Threshold rule: both comparisons are fp32 against the float arguments; ops.val_confusion passes the fp32 nearest to the Python
//   value, which is what torch compares an fp32 tensor with.  iou_thres >= 0 is required: pairs that do not intersect (IoU 0 or NaN)
//   are skipped without the division.
//
// Design: one workgroup (8 waves) per image, nq <= 512, 16 KB of static LDS:
//   a.  thread d owns row d of predn: box, area, class, pass / fail in registers;
//   b.  labels stream through an LDS tile of 512 as in valmatch.hip, so there is no cap on labels per image.  While a tile is staged
//       every in-range label adds 1 to Mx[nc, gc]; every passing thread walks the tile (broadcast reads) and keeps (best IoU, L, gc of L)
//       in registers - labels are visited in ascending order and the comparison is strict, which is the tie rule of L;
//   c.  D as valmatch.hip step 7 finds its prefix maximum: d is its label's D iff no other row claims the same label with a higher IoU,
//       or an equal IoU and a lower row - at most 512 broadcast LDS reads per thread.  A winner adds 1 to Mx[cls, gc] and takes 1 back
//       from Mx[nc, gc], so no per-label flag is needed;
//   d.  "any matched pair" = "any row has an L" (a claimed label always has a winner): one barrier-reduction.
//   Every update is an integer atomic on global memory: the result does not depend on order, accumulation over images, batches and
//   launches needs nothing else, and no size of nc needs a second path.
#include "postproc.h"

#define CF_TILE 512

struct CfShared {
  float lab[CF_TILE][5];   // x1 y1 x2 y2 area of the labels in flight (original-image pixels)
  int gc[CF_TILE];         // their classes, -1: outside [0, nc)
  float best[PP_MAX_Q];    // IoU of row d with L(d)
  int bestl[PP_MAX_Q];     // L(d), -1: none
};

// `.int()` with the range check done in float: NaN, +-inf and anything outside [0, nc) -> -1
__device__ __forceinline__ int cf_class(float c, int nc) {
  const float t = truncf(c);
  return (t >= 0.0f && t < (float)nc) ? (int)t : -1;
}

__global__ __launch_bounds__(PP_THREADS) void val_confusion_kernel(const float* __restrict__ predn, const int32_t* __restrict__ counts, int nq,
                                                                   int nc, const float* __restrict__ lab_cls,
                                                                   const float* __restrict__ lab_box, const int32_t* __restrict__ lab_off,
                                                                   int M, const float* __restrict__ scale, float cm_conf, float thr,
                                                                   int32_t* __restrict__ matrix) {
  __shared__ CfShared s;
  const int b = blockIdx.x, tid = threadIdx.x;
  const size_t ld = (size_t)nc + 1;
  int32_t* bg = matrix + (size_t)nc * ld;   // the background row

  // ---- a. thread d owns row d of predn
  int npr = counts[b];
  npr = npr < 0 ? 0 : (npr > nq ? nq : npr);
  float d0 = 0.f, d1 = 0.f, d2 = 0.f, d3 = 0.f, darea = 0.f;
  int dcl = -1;
  if (tid < npr) {
    const float* r = predn + ((size_t)b * nq + tid) * 6;
    d0 = r[0]; d1 = r[1]; d2 = r[2]; d3 = r[3];
    darea = (d2 - d0) * (d3 - d1);
    if (r[4] > cm_conf) dcl = cf_class(r[5], nc);
  }
  const bool pass = dcl >= 0;

  // ---- b. labels through the tile: background counts, and the arg-max L(d) of every passing row
  const float lw = scale[4 * b + 2], lh = scale[4 * b + 3];
  int l0 = lab_off[b], l1 = lab_off[b + 1];
  l0 = l0 < 0 ? 0 : l0;
  l1 = l1 > M ? M : l1;
  float best = -1.0f;
  int bestl = -1, bestgc = 0;
  for (int t0 = l0; t0 < l1; t0 += CF_TILE) {
    const int nt = l1 - t0 < CF_TILE ? l1 - t0 : CF_TILE;
    if (tid < nt) {
      const float* lb = lab_box + (size_t)(t0 + tid) * 4;
      const float cx = lb[0], cy = lb[1], hw = lb[2] / 2.0f, hh = lb[3] / 2.0f;
      const float x1 = (cx - hw) * lw, y1 = (cy - hh) * lh, x2 = (cx + hw) * lw, y2 = (cy + hh) * lh;
      float* e = s.lab[tid];
      e[0] = x1; e[1] = y1; e[2] = x2; e[3] = y2;
      e[4] = (x2 - x1) * (y2 - y1);
      const int gc = cf_class(lab_cls[t0 + tid], nc);
      s.gc[tid] = gc;
      if (gc >= 0) atomicAdd(bg + gc, 1);
    }
    __syncthreads();
    if (pass) {
      for (int j = 0; j < nt; ++j) {
        const int gc = s.gc[j];
        if (gc < 0) continue;
        const float* e = s.lab[j];
        const float iw = pp_min(e[2], d2) - pp_max(e[0], d0), ih = pp_min(e[3], d3) - pp_max(e[1], d1);
        if (!(iw > 0.0f && ih > 0.0f)) continue;   // inter is 0 (or NaN): IoU 0 or NaN, never above a threshold >= 0
        const float inter = iw * ih;
        const float v = inter / (((e[4] + darea) - inter) + 1e-7f);
        if (v > thr && v > best) { best = v; bestl = t0 + j; bestgc = gc; }
      }
    }
    __syncthreads();
  }

  // ---- c. D(l): the claimant of highest IoU, the lower row among equals
  s.best[tid] = best;
  s.bestl[tid] = bestl;
  const int any = __syncthreads_or(bestl >= 0);
  bool win = bestl >= 0;
  if (win)
    for (int e = 0; e < npr; ++e)
      if (s.bestl[e] == bestl && e != tid) {
        const float o = s.best[e];
        if (o > best || (o == best && e < tid)) win = false;
      }

  // ---- d. the updates
  if (win) {
    atomicAdd(matrix + (size_t)dcl * ld + bestgc, 1);
    atomicAdd(bg + bestgc, -1);
  } else if (pass && any) {
    atomicAdd(matrix + (size_t)dcl * ld + nc, 1);
  }
}

extern "C" int tamtr_val_confusion(const float* predn, const int32_t* counts, int B, int nq, int nc, const float* lab_cls,
                                   const float* lab_box, const int32_t* lab_off, int M, const float* scale, float cm_conf, float iou_thres,
                                   int32_t* matrix, void* stream) {
  if (!predn || !counts || !lab_off || !scale || !matrix || B < 1 || nq < 1 || nc < 1 || M < 0) return TAMTR_EINVAL;
  if (M > 0 && (!lab_cls || !lab_box)) return TAMTR_EINVAL;
  if (!(iou_thres >= 0.0f)) return TAMTR_EINVAL;
  if (nq > PP_MAX_Q) return TAMTR_EUNSUP;
  hipLaunchKernelGGL(val_confusion_kernel, dim3(B), dim3(PP_THREADS), 0, (hipStream_t)stream, predn, counts, nq, nc, lab_cls, lab_box, lab_off,
                     M, scale, cm_conf, iou_thres, matrix);
  return tamtr_launch_status();
}
