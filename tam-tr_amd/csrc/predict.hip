// predict.hip - the predictor's postprocess for a whole batch in one launch (tamtr_detect_postprocess).
//
// Replaces the per-image loop of RTDETRPredictor.postprocess (ultralytics/models/rtdetrworld/predict.py:34-78): xywh -> xyxy
// (utils/ops.py:360-380), class max, confidence (and class) filter, class-aware torchvision.ops.nms on boxes shifted by
// cls * max_wh, scaling to the original image.  The host loop synchronises once per image (engine.nms copies an IoU matrix
// back); here nothing leaves the device and the output has a fixed shape, so the call can be captured into a graph.
//
// Contract: bit-exact with that rule applied in fp32 to the input widened to fp32, every operation rounded on its own (the
// object is compiled with -ffp-contract=off; the IoU division is the correctly rounded fp32 division):
//   box     x1 = cx - w/2, x2 = cx + w/2 (same for y)
//   score   max over the nc class scores, the lowest class index on ties; NaN anywhere in the row -> NaN score (torch.max)
//   filter  score > conf, and cls in classes[] when a class filter is given
//   NMS     shifted box = box + cls * (single_cls ? 0 : max_wh); area = (x2-x1)*(y2-y1); for a kept row i and a later row j
//           (torchvision's nms_kernel.cpp, CPU, operand order included): xx1 = max(x1i, x1j) ... as std::max / std::min,
//           w = max(0, xx2-xx1), h likewise, inter = w*h, iou = inter / (area_i + area_j - inter), no eps (0/0 = NaN, which
//           does not suppress); j is suppressed when iou > thr.  Rows are visited in descending score order, stable
//           (equal scores: ascending query index).
//   Threshold rule: the comparison is done in fp32 against the float argument `iou`.  torchvision compares the float IoU
//   with a double threshold; ops.detect_postprocess passes the largest fp32 <= the double threshold, for which
//   `iou_f32 > thr_f32` and `iou_f32 > thr_f64` agree for every fp32 IoU, so the Python op reproduces torchvision's rule.
//   output  kept rows in NMS order, unshifted, x *= w_orig, y *= h_orig, then score and float(cls); keep = source query.
//
// Design: one workgroup (8 waves) per image, nq <= 512, everything in LDS (about 59 KB):
//   1. rows -> class max: a group of GW lanes (4, 16 or 64, chosen from nc) shares a row, so the class scores are read as
//      consecutive elements instead of a 4 * nd byte stride per lane; (value, index) butterfly with the torch.max rule.
//   2. 64-bit key (~ordered(score) << 32 | query) per row, all ones for rows that fail the filter; a bitonic sort over the
//      next power of two puts the survivors first in NMS order (no separate compaction: the key already holds the query).
//      The float -> ordered-integer map handles conf < 0; -0.0 is folded onto +0.0 so the two tie as torch's sort ties them.
//   3. upper-triangular suppression mask, one 64-bit word per (row, 64-column block), built by whole waves: lane l computes
//      iou(i, 64 w + l) and a ballot forms the word.
//   4. greedy pass in wave 0 with no barrier: lane k holds removal word k; every row is tested with a readlane of its word.
//   5. coalesced write of out / keep (zero / -1 padding after the count) and counts.
#include "postproc.h"

struct PpShared {
  float box[PP_MAX_Q][4];    // unshifted x1 y1 x2 y2 by query
  float score[PP_MAX_Q];     // by query
  int cls[PP_MAX_Q];         // by query
  uint64_t key[PP_MAX_Q];    // sort keys; after the sort, position p holds the p-th row in NMS order
  float sbox[PP_MAX_Q][4];   // shifted boxes in NMS order
  float sarea[PP_MAX_Q];
  uint64_t mask[PP_MAX_Q][PP_WORDS];
  int kept[PP_MAX_Q];        // NMS positions of the kept rows, in order
  int n, count;
};

template <typename T, int GW>
__global__ __launch_bounds__(PP_THREADS) void detect_postprocess_kernel(const T* __restrict__ preds, int nq, int nd,
                                                                        const int32_t* __restrict__ orig_hw, float conf, float thr,
                                                                        int single_cls, float max_wh, const int32_t* __restrict__ classes,
                                                                        int n_classes, float* __restrict__ out, int32_t* __restrict__ keep,
                                                                        int32_t* __restrict__ counts) {
  __shared__ PpShared s;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
  const int nc = nd - 4;
  const T* pb = preds + (size_t)b * nq * nd;
  if (tid == 0) s.n = 0;
  __syncthreads();

  // ---- 1. class max, filter, sort key (a group of GW lanes per row)
  const int sub = tid & (GW - 1);
  int n_local = 0;
  for (int q0 = 0; q0 < nq; q0 += PP_THREADS / GW) {
    const int q = q0 + tid / GW;
    const bool row = q < nq;  // uniform inside the group
    float bv, bx[4] = {0.f, 0.f, 0.f, 0.f};
    int bi;
    const T* r = pb + (size_t)q * nd;
    pp_row_max<T, GW>(r, nc, sub, row, bv, bi);
    if (row && sub == 0)
      for (int k = 0; k < 4; ++k) bx[k] = Elt<T>::ld(r + k);
    if (row && sub == 0) {
      const float dw = bx[2] / 2.0f, dh = bx[3] / 2.0f;
      s.box[q][0] = bx[0] - dw;
      s.box[q][1] = bx[1] - dh;
      s.box[q][2] = bx[0] + dw;
      s.box[q][3] = bx[1] + dh;
      s.score[q] = bv;
      s.cls[q] = bi;
      const bool ok = pp_passes(bv, bi, conf, classes, n_classes);
      s.key[q] = ok ? ((uint64_t)~pp_ordered(bv) << 32) | (uint32_t)q : ~0ull;
      n_local += ok;
    }
  }
  int P = 1;
  while (P < nq) P <<= 1;
  for (int q = nq + tid; q < P; q += PP_THREADS) s.key[q] = ~0ull;
  if (n_local) atomicAdd(&s.n, n_local);
  __syncthreads();
  const int n = s.n;

  // ---- 2. bitonic sort of P <= 512 keys, ascending (= NMS order; failed rows last)
  pp_bitonic_sort(s.key, P, tid);

  // shifted boxes and areas in NMS order
  for (int p = tid; p < n; p += PP_THREADS) {
    const int q = (int)(s.key[p] & 0xffffffffu);
    const float sh = (float)s.cls[q] * (single_cls ? 0.0f : max_wh);
    float bb[4];
    for (int k = 0; k < 4; ++k) { bb[k] = s.box[q][k] + sh; s.sbox[p][k] = bb[k]; }
    s.sarea[p] = (bb[2] - bb[0]) * (bb[3] - bb[1]);
  }
  __syncthreads();

  // ---- 3. suppression mask: word (i, w) bit l = iou(i, 64 w + l) > thr for 64 w + l > i
  pp_nms_mask(s.sbox, s.sarea, s.mask, n, thr, wave, lane);
  __syncthreads();

  // ---- 4. greedy pass, one wave, no barrier: lane k < nw holds removal word k
  if (wave == 0) {
    const int cnt = pp_greedy(s.mask, s.kept, n, lane);
    if (lane == 0) s.count = cnt;
  }
  __syncthreads();

  // ---- 5. outputs: kept rows, then zero / -1 padding
  const int cnt = s.count;
  const float oh = (float)orig_hw[2 * b], ow = (float)orig_hw[2 * b + 1];
  float* ob = out + (size_t)b * nq * 6;
  for (int e = tid; e < nq * 6; e += PP_THREADS) {
    const int r = e / 6, c = e - r * 6;
    float v = 0.0f;
    if (r < cnt) {
      const int q = (int)(s.key[s.kept[r]] & 0xffffffffu);
      v = c < 4 ? s.box[q][c] * ((c & 1) ? oh : ow) : c == 4 ? s.score[q] : (float)s.cls[q];
    }
    ob[e] = v;
  }
  for (int r = tid; r < nq; r += PP_THREADS) keep[(size_t)b * nq + r] = r < cnt ? (int)(s.key[s.kept[r]] & 0xffffffffu) : -1;
  if (tid == 0) counts[b] = cnt;
}

template <typename T>
static void pp_launch(const void* preds, int B, int nq, int nd, const int32_t* orig_hw, float conf, float iou, int single_cls, float max_wh,
                      const int32_t* classes, int n_classes, float* out, int32_t* keep, int32_t* counts, hipStream_t st) {
  const T* p = static_cast<const T*>(preds);
#define PP_LAUNCH(GW)                                                                                                                  \
  hipLaunchKernelGGL((detect_postprocess_kernel<T, GW>), dim3(B), dim3(PP_THREADS), 0, st, p, nq, nd, orig_hw, conf, iou, single_cls, \
                     max_wh, classes, n_classes, out, keep, counts)
  PP_LAUNCH_GW(nd - 4, PP_LAUNCH);
#undef PP_LAUNCH
}

extern "C" int tamtr_detect_postprocess(const void* preds, int dtype, int B, int nq, int nd, const int32_t* orig_hw, float conf, float iou,
                                        int single_cls, float max_wh, const int32_t* classes, int n_classes, float* out, int32_t* keep,
                                        int32_t* counts, void* stream) {
  if (!preds || !orig_hw || !out || !keep || !counts || B < 1 || nq < 1 || nd < 5 || n_classes < 0) return TAMTR_EINVAL;
  if (dtype != TAMTR_F32 && dtype != TAMTR_BF16) return TAMTR_EINVAL;
  if (nq > PP_MAX_Q) return TAMTR_EUNSUP;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == TAMTR_F32)
    pp_launch<float>(preds, B, nq, nd, orig_hw, conf, iou, single_cls, max_wh, classes, n_classes, out, keep, counts, st);
  else
    pp_launch<bf16_t>(preds, B, nq, nd, orig_hw, conf, iou, single_cls, max_wh, classes, n_classes, out, keep, counts, st);
  return tamtr_launch_status();
}
