// valmatch.hip - the validator's postprocess and label matching for a whole batch in one launch (tamtr_val_postprocess_match).
//
// Replaces the per-image loop of engine.Validator.update (RTDETRValidator.postprocess, ultralytics/models/rtdetrworld/val.py:102-173,
// and DetectionValidator._process_batch / match_predictions, ultralytics/engine/validator.py:208-247): class max, confidence mask,
// class-aware NMS, scaling of predictions and labels to the original image, IoU of every label with every kept detection and the
// true-positive table at the ten IoU thresholds 0.5 : 0.05 : 0.95.  The host loop synchronises at least twice per image; here
// nothing leaves the device and the outputs have a fixed shape, so the call can be captured into a graph.
//
// The rule is the VALIDATOR's, which is not the predictor's (predict.hip).  Contract: bit-exact with engine.postprocess +
// engine.process_batch applied to CPU fp32 tensors (the input widened to fp32 first), every operation rounded on its own (the object
// is compiled with -ffp-contract=off; divisions are the correctly rounded fp32 division):
//   box      b = xywh * imgsz first, then x1 = cx - w/2, x2 = cx + w/2 (same for y)   [the predictor converts first, scales last]
//   score    max over the nc class scores, the lowest class index on ties; NaN anywhere in the row -> NaN score (torch.max)
//   order    descending score, stable (equal scores: ascending query; a NaN score sorts first, as torch sorts it).  torch's argsort
//            is not stable; the stable order is this project's definition.
//   filter   the reference applies the UNSORTED mask `score > conf` to the SORTED rows (val.py:113-121, engine.py:353; kept on
//            purpose): sorted position p survives iff the score of QUERY p exceeds conf.
//   NMS      as predict.hip (postproc.h): boxes shifted by cls * max_wh (0 when single_cls), IoU = inter / (area_a + area_b - inter)
//            without eps, suppress when IoU > thr, rows visited in the surviving order.
//   Threshold rule: the comparison is fp32 against the float argument `iou`; ops.val_postprocess_match passes the largest fp32 <= the
//   double threshold, which reproduces torchvision's `iou_f32 > thr_f64` (the reference validator calls torchvision.ops.nms).
//   engine.nms compares in numpy against float32(thr) instead; the two differ only when an IoU equals float32(thr) exactly and that
//   value lies above thr (0.6 is such a threshold, 0.7 is not).
//   scale    cls = 0 when single_cls (label classes are NOT zeroed); predn.x *= sx, predn.y *= sy with sx = fp32(w_orig / imgsz),
//            sy = fp32(h_orig / imgsz) (divisions in double, on the host); label xywh -> xyxy on the normalised values, then
//            x *= lw = fp32(w_orig), y *= lh = fp32(h_orig).  scale[b] = {sx, sy, lw, lh}.
//   IoU      engine.box_iou(labels, predn): inter = max(min(l.x2, d.x2) - max(l.x1, d.x1), 0) * (same in y),
//            iou = inter / (((area_l + area_d) - inter) + fp32(1e-7))
//   match    match_predictions restated without its sequential look: for detection d, l*(d) = the same-class label of highest IoU
//            among those with IoU >= 0.5, iou*(d) that IoU; correct[d, t] = iou*(d) >= IOUV[t] and no d' < d with l*(d') = l*(d) and
//            iou*(d') >= IOUV[t] (each label goes to its most CONFIDENT claimant, not to the one of best IoU - the second np.unique
//            of the reference runs on rows re-sorted by detection).  IOUV = the fp32 values of torch.linspace(0.5, 0.95, 10); fp32
//            `>=`; a NaN IoU and a class mismatch never match.
//   Tie rule: numpy's argsort()[::-1] leaves the order of equal IoUs unspecified; here, among labels of equal IoU the LOWER label
//   index wins (label order = order inside lab_cls / lab_box, i.e. file order inside the image).
//
// Design: one workgroup (8 waves) per image, nq <= 512, about 62 KB of static LDS:
//   1-4. as predict.hip with the validator's box rule, every row sorted and a ballot prefix sum for the confidence quirk;
//   5.   thread d owns kept detection d (box, area, class in registers) and writes its predn row;
//   6.   labels stream through an LDS tile of 512 (the tile lives in the space of the NMS mask, which is dead by then), so there
//        is no cap on labels per image; every thread walks the tile (broadcast reads) and keeps its arg-max in registers.  The
//        division is only done for same-class pairs that intersect (anything else has IoU 0 or NaN, below every threshold);
//   7.   per-detection prefix maximum over earlier detections with the same label, then the ten comparisons.
#include "postproc.h"

#define VM_TILE 512
#define VM_NT 10

struct VmShared {
  float box[PP_MAX_Q][4];    // unshifted x1 y1 x2 y2 by query (input-image pixels)
  float score[PP_MAX_Q];     // by query
  int cls[PP_MAX_Q];         // by query
  uint64_t key[PP_MAX_Q];    // sort keys; after the sort, position p holds the p-th row in descending score order
  int ord[PP_MAX_Q];         // query of the r-th surviving row (NMS order)
  float sbox[PP_MAX_Q][4];   // shifted boxes in NMS order
  float sarea[PP_MAX_Q];
  int kept[PP_MAX_Q];        // NMS positions of the kept rows, in order
  union {
    uint64_t mask[PP_MAX_Q][PP_WORDS];
    struct {
      float lab[VM_TILE][6];  // cls x1 y1 x2 y2 area of the labels in flight (original-image pixels)
      float best[PP_MAX_Q];   // iou*(d)
      int bestl[PP_MAX_Q];    // l*(d), -1: none
    } m;
  } u;
  int wtot[PP_THREADS / WAVE];
  int count;
};
static_assert(sizeof(VmShared) <= 64 * 1024, "static LDS limit");

template <typename T, int GW>
__global__ __launch_bounds__(PP_THREADS) void val_postprocess_match_kernel(const T* __restrict__ preds, int nq, int nd, float imgsz, float conf,
                                                                           float thr, int single_cls, float max_wh,
                                                                           const float* __restrict__ lab_cls, const float* __restrict__ lab_box,
                                                                           const int32_t* __restrict__ lab_off, int M,
                                                                           const float* __restrict__ scale, float* __restrict__ predn,
                                                                           uint8_t* __restrict__ correct, int32_t* __restrict__ counts) {
  __shared__ VmShared s;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
  const int nc = nd - 4;
  const T* pb = preds + (size_t)b * nq * nd;

  // ---- 1. class max, box, sort key of EVERY row (a group of GW lanes per row)
  const int sub = tid & (GW - 1);
  for (int q0 = 0; q0 < nq; q0 += PP_THREADS / GW) {
    const int q = q0 + tid / GW;
    const bool row = q < nq;  // uniform inside the group
    float bv;
    int bi;
    const T* r = pb + (size_t)q * nd;
    pp_row_max<T, GW>(r, nc, sub, row, bv, bi);
    if (row && sub == 0) {
      float bx[4];
      for (int k = 0; k < 4; ++k) bx[k] = Elt<T>::ld(r + k) * imgsz;
      const float dw = bx[2] / 2.0f, dh = bx[3] / 2.0f;
      s.box[q][0] = bx[0] - dw;
      s.box[q][1] = bx[1] - dh;
      s.box[q][2] = bx[0] + dw;
      s.box[q][3] = bx[1] + dh;
      s.score[q] = bv;
      s.cls[q] = bi;
      const uint32_t o = bv != bv ? 0xffffffffu : pp_ordered(bv);  // NaN first, whatever its sign bit
      s.key[q] = ((uint64_t)~o << 32) | (uint32_t)q;
    }
  }
  int P = 1;
  while (P < nq) P <<= 1;
  for (int q = nq + tid; q < P; q += PP_THREADS) s.key[q] = ~0ull;
  __syncthreads();

  // ---- 2. bitonic sort, then the confidence quirk: position p survives iff score[QUERY p] > conf
  pp_bitonic_sort(s.key, P, tid);
  const bool alive = tid < nq && s.score[tid] > conf;
  const uint64_t bal = __ballot(alive);
  if (lane == 0) s.wtot[wave] = __popcll(bal);
  __syncthreads();
  int base = 0, n = 0;
  for (int w = 0; w < PP_THREADS / WAVE; ++w) {
    base += w < wave ? s.wtot[w] : 0;
    n += s.wtot[w];
  }
  if (alive) s.ord[base + __popcll(bal & ((1ull << lane) - 1ull))] = (int)(s.key[tid] & 0xffffffffu);
  __syncthreads();

  // shifted boxes and areas in NMS order
  for (int p = tid; p < n; p += PP_THREADS) {
    const int q = s.ord[p];
    const float sh = (float)s.cls[q] * (single_cls ? 0.0f : max_wh);
    float bb[4];
    for (int k = 0; k < 4; ++k) { bb[k] = s.box[q][k] + sh; s.sbox[p][k] = bb[k]; }
    s.sarea[p] = (bb[2] - bb[0]) * (bb[3] - bb[1]);
  }
  __syncthreads();

  // ---- 3. suppression mask, 4. greedy pass in wave 0
  pp_nms_mask(s.sbox, s.sarea, s.u.mask, n, thr, wave, lane);
  __syncthreads();
  if (wave == 0) {
    const int c = pp_greedy(s.u.mask, s.kept, n, lane);
    if (lane == 0) s.count = c;
  }
  __syncthreads();   // the mask is dead from here on: its space holds the label tile and the arg-max

  // ---- 5. thread d owns kept detection d: native-space row
  const int cnt = s.count;
  const float sx = scale[4 * b], sy = scale[4 * b + 1], lw = scale[4 * b + 2], lh = scale[4 * b + 3];
  const bool det = tid < cnt;
  float d0 = 0.f, d1 = 0.f, d2 = 0.f, d3 = 0.f, dsc = 0.f, dcl = 0.f, darea = 0.f;
  if (det) {
    const int q = s.ord[s.kept[tid]];
    d0 = s.box[q][0] * sx;
    d1 = s.box[q][1] * sy;
    d2 = s.box[q][2] * sx;
    d3 = s.box[q][3] * sy;
    dsc = s.score[q];
    dcl = single_cls ? 0.0f : (float)s.cls[q];
    darea = (d2 - d0) * (d3 - d1);
  }
  if (tid < nq) {
    float* o = predn + ((size_t)b * nq + tid) * 6;
    o[0] = d0; o[1] = d1; o[2] = d2; o[3] = d3; o[4] = dsc; o[5] = dcl;
  }

  // ---- 6. arg-max over the same-class labels, streamed through the tile
  int l0 = lab_off[b], l1 = lab_off[b + 1];
  l0 = l0 < 0 ? 0 : l0;
  l1 = l1 > M ? M : l1;
  float best = -1.0f;
  int bestl = -1;
  for (int t0 = l0; t0 < l1; t0 += VM_TILE) {
    const int nt = l1 - t0 < VM_TILE ? l1 - t0 : VM_TILE;
    if (tid < nt) {
      const float* lb = lab_box + (size_t)(t0 + tid) * 4;
      const float cx = lb[0], cy = lb[1], hw = lb[2] / 2.0f, hh = lb[3] / 2.0f;
      const float x1 = (cx - hw) * lw, y1 = (cy - hh) * lh, x2 = (cx + hw) * lw, y2 = (cy + hh) * lh;
      float* e = s.u.m.lab[tid];
      e[0] = lab_cls[t0 + tid];
      e[1] = x1; e[2] = y1; e[3] = x2; e[4] = y2;
      e[5] = (x2 - x1) * (y2 - y1);
    }
    __syncthreads();
    if (det) {
      for (int j = 0; j < nt; ++j) {
        const float* e = s.u.m.lab[j];
        if (e[0] != dcl) continue;
        const float iw = pp_min(e[3], d2) - pp_max(e[1], d0), ih = pp_min(e[4], d3) - pp_max(e[2], d1);
        if (!(iw > 0.0f && ih > 0.0f)) continue;   // inter is 0 (or NaN): IoU below every threshold
        const float inter = iw * ih;
        const float v = inter / (((e[5] + darea) - inter) + 1e-7f);
        if (v >= 0.5f && v > best) { best = v; bestl = t0 + j; }
      }
    }
    __syncthreads();
  }

  // ---- 7. a label goes to the first (most confident) detection that claims it at each threshold
  s.u.m.best[tid] = best;
  s.u.m.bestl[tid] = bestl;
  __syncthreads();
  float before = -1.0f;   // highest iou* among earlier detections with the same label
  if (bestl >= 0)
    for (int e = 0; e < tid; ++e)
      if (s.u.m.bestl[e] == bestl) before = fmaxf(before, s.u.m.best[e]);
  if (tid < nq) {
    const float iouv[VM_NT] = {0.5f, 0.55f, 0.6f, 0.65f, 0.7f, 0.75f, 0.8f, 0.85f, 0.9f, 0.95f};
    uint8_t* c = correct + ((size_t)b * nq + tid) * VM_NT;
#pragma unroll
    for (int t = 0; t < VM_NT; ++t) c[t] = (bestl >= 0 && best >= iouv[t] && !(before >= iouv[t])) ? 1 : 0;
  }
  if (tid == 0) counts[b] = cnt;
}

template <typename T>
static void vm_launch(const void* preds, int B, int nq, int nd, float imgsz, float conf, float iou, int single_cls, float max_wh,
                      const float* lab_cls, const float* lab_box, const int32_t* lab_off, int M, const float* scale, float* predn,
                      uint8_t* correct, int32_t* counts, hipStream_t st) {
  const T* p = static_cast<const T*>(preds);
#define VM_LAUNCH(GW)                                                                                                                        \
  hipLaunchKernelGGL((val_postprocess_match_kernel<T, GW>), dim3(B), dim3(PP_THREADS), 0, st, p, nq, nd, imgsz, conf, iou, single_cls, max_wh, \
                     lab_cls, lab_box, lab_off, M, scale, predn, correct, counts)
  PP_LAUNCH_GW(nd - 4, VM_LAUNCH);
#undef VM_LAUNCH
}

extern "C" int tamtr_val_postprocess_match(const void* preds, int dtype, int B, int nq, int nd, float imgsz, float conf, float iou,
                                           int single_cls, float max_wh, const float* lab_cls, const float* lab_box,
                                           const int32_t* lab_off, int M, const float* scale, float* predn, uint8_t* correct,
                                           int32_t* counts, void* stream) {
  if (!preds || !lab_off || !scale || !predn || !correct || !counts || B < 1 || nq < 1 || nd < 5 || M < 0) return TAMTR_EINVAL;
  if (M > 0 && (!lab_cls || !lab_box)) return TAMTR_EINVAL;
  if (dtype != TAMTR_F32 && dtype != TAMTR_BF16) return TAMTR_EINVAL;
  if (nq > PP_MAX_Q) return TAMTR_EUNSUP;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == TAMTR_F32)
    vm_launch<float>(preds, B, nq, nd, imgsz, conf, iou, single_cls, max_wh, lab_cls, lab_box, lab_off, M, scale, predn, correct, counts, st);
  else
    vm_launch<bf16_t>(preds, B, nq, nd, imgsz, conf, iou, single_cls, max_wh, lab_cls, lab_box, lab_off, M, scale, predn, correct, counts, st);
  return tamtr_launch_status();
}
