// tta.hip - test-time augmentation on the device: one launch builds a scaled / mirrored view of a batch (tamtr_tta_view), one launch
// merges the views' raw outputs into an ordinary prediction tensor (tamtr_tta_merge).
//
// Replaces DetectionModel._predict_augment (ultralytics/nn/tasks.py:272-295) with scale_img (utils/torch_utils.py:316-327) and
// _descale_pred (tasks.py:286-295), as the predictor and the validator reach them through `augment` (cfg/default.yaml:66,
// engine/predictor.py:135, engine/validator.py:109,169): views of the input, the scale and the flip undone on the boxes, the views
// concatenated along the query axis, and the ordinary NMS postprocess merging them.  YOLO's _clip_augmented (tasks.py:297-306) cuts the
// tails of anchor layers and has no counterpart for a query decoder: every query of every view is a candidate.
//
// ---- tamtr_tta_view: scale_img(x.flip(3) if flip else x, ratio, gs).  The sizes come from the caller (Python doubles): content
// (sh, sw) = (int(H ratio), int(W ratio)), canvas (Hp, Wp) = (ceil(H ratio / gs) gs, ceil(W ratio / gs) gs).  Inside the content
// rectangle the value is torch's bilinear align_corners=False sample: per axis, in fp32, src = max(sc (d + 0.5) - 0.5, 0) with
// sc = float(n_in) / float(n_out), i0 = floor(src), i1 = min(i0 + 1, n_in - 1), l1 = src - i0, l0 = 1 - l1;
// v = l0y (l0x v00 + l1x v01) + l1y (l0x v10 + l1x v11), every operation rounded on its own.  Outside it is 0.447f.  A content
// rectangle of the input's size is a copy (mirrored when flip), bit for bit.  Memory bound: a workgroup writes 256 consecutive
// pixels of one canvas row for the three channels (coalesced stores); its gather touches two source rows per channel, and the
// coordinates are computed once per pixel, not per channel.
//
// ---- tamtr_tta_merge: candidate i = v nq + q of image b is row q of view v.  Every fp32 operation rounds on its own (the object is
// compiled with -ffp-contract=off), the input is widened to fp32:
//   de-augment  cx' = cx kx, then cx' = 1 - cx' when the view is mirrored; cy' = cy ky; w' = w kx; h' = h ky (descale, then de-flip)
//   score, cls  torch.max over the nc scores (pp_row_max); a candidate needs score > conf and, with a filter, cls in classes[]
//   order       descending score, equal scores by ascending i
//   NMS         predict.hip's: x1 = cx' - w'/2 ..., shifted by cls * max_wh unless single_cls, torchvision's operand order, correctly
//               rounded IoU division, row j suppressed when iou > thr in fp32
//   output      the first max_out survivors in order: cx' cy' w' h' and the source row's nc scores widened exactly; src = i; zero rows
//               and src = -1 after them; counts = rows written, dropped = survivors that did not fit.
// Feeding ym to the ordinary postprocess gives what the postprocess of the concatenated de-augmented rows gives: the survivors of a
// greedy NMS do not suppress one another, they come out in score order, and their boxes are recomputed from the same four numbers.
//
// Design: one workgroup of 16 waves per image, N = V nq <= 2048 candidates, about 59 KB of LDS.  A full N x N suppression mask would
// take 512 KB, so predict.hip's mask-then-greedy pass does not carry over:
//   1. class max per row by groups of GW lanes, filter (pp_passes), 64-bit key (~ordered(score) << 32 | i), all ones for rows that fail.
//   2. bitonic sort over the next power of two: survivors first, in NMS order (pp_bitonic_sort_pairs).
//   3. shifted corner boxes in NMS order (pp_merge_sbox).
//   4. greedy pass over tiles of 64 rows, one barrier per tile (pp_greedy_tiles).
//   5. coalesced write of ym / src (zero / -1 padding) and the two counters (pp_merge_write).
// Stages 2 to 5 are postproc.h's, shared with slice.hip; they reach the candidates through TtaRows.
#include "postproc.h"

#define TTA_MAX_N 2048
#define TTA_MAX_V 16
#define TTA_THREADS 1024
#define TTA_WAVES (TTA_THREADS / WAVE)
#define TTA_VIEW_THREADS 256

// ------------------------------------------------------------------------------------------------ the view
struct TtaAxis {
  int i0, i1;
  float l0, l1;
};

__device__ __forceinline__ TtaAxis tta_axis(int d, int n_in, int n_out) {
  const float sc = (float)n_in / (float)n_out;
  const float src = pp_max(sc * ((float)d + 0.5f) - 0.5f, 0.0f);
  TtaAxis a;
  a.i0 = min((int)src, n_in - 1);
  a.i1 = min(a.i0 + 1, n_in - 1);
  a.l1 = src - (float)a.i0;
  a.l0 = 1.0f - a.l1;
  return a;
}

__global__ __launch_bounds__(TTA_VIEW_THREADS) void tta_view_kernel(const float* __restrict__ x, float* __restrict__ out, int H, int W,
                                                                    int sh, int sw, int Hp, int Wp, int flip) {
  const int ox = blockIdx.x * TTA_VIEW_THREADS + threadIdx.x, oy = blockIdx.y, b = blockIdx.z;
  if (ox >= Wp) return;
  const float* xb = x + (size_t)b * 3 * H * W;
  float* ob = out + ((size_t)b * 3 * Hp + oy) * Wp + ox;
  const size_t oplane = (size_t)Hp * Wp, iplane = (size_t)H * W;
  if (oy >= sh || ox >= sw) {
    for (int c = 0; c < 3; ++c) ob[c * oplane] = 0.447f;
    return;
  }
  if (sh == H && sw == W) {  // ratio 1: a copy
    const size_t at = (size_t)oy * W + (flip ? W - 1 - ox : ox);
    for (int c = 0; c < 3; ++c) ob[c * oplane] = xb[c * iplane + at];
    return;
  }
  const TtaAxis ay = tta_axis(oy, H, sh), ax = tta_axis(ox, W, sw);
  const int c0 = flip ? W - 1 - ax.i0 : ax.i0, c1 = flip ? W - 1 - ax.i1 : ax.i1;
  const size_t r0 = (size_t)ay.i0 * W, r1 = (size_t)ay.i1 * W;
  for (int c = 0; c < 3; ++c) {
    const float* p = xb + c * iplane;
    const float top = ax.l0 * p[r0 + c0] + ax.l1 * p[r0 + c1];
    const float bot = ax.l0 * p[r1 + c0] + ax.l1 * p[r1 + c1];
    ob[c * oplane] = ay.l0 * top + ay.l1 * bot;
  }
}

extern "C" int tamtr_tta_view(const float* x, float* out, int B, int H, int W, int sh, int sw, int Hp, int Wp, int flip, void* stream) {
  if (!x || !out || B < 1 || H < 1 || W < 1 || sh < 1 || sw < 1 || Hp < sh || Wp < sw || (flip != 0 && flip != 1)) return TAMTR_EINVAL;
  if (B > 65535 || Hp > 65535) return TAMTR_EUNSUP;  // grid y and z
  hipLaunchKernelGGL(tta_view_kernel, dim3((Wp + TTA_VIEW_THREADS - 1) / TTA_VIEW_THREADS, Hp, B), dim3(TTA_VIEW_THREADS), 0,
                     (hipStream_t)stream, x, out, H, W, sh, sw, Hp, Wp, flip);
  return tamtr_launch_status();
}

// ------------------------------------------------------------------------------------------------ the merge
struct TtaViews {
  const void* y[TTA_MAX_V];
};

struct TtaShared {
  uint64_t key[TTA_MAX_N];      // sort keys; after the sort, position p holds the p-th candidate in NMS order
  int cls[TTA_MAX_N];           // by candidate
  float sbox[TTA_MAX_N][4];     // shifted x1 y1 x2 y2 in NMS order
  uint64_t rem[TTA_MAX_N / 64]; // removed bit per NMS position
  uint64_t tmask[2][64];        // the current tile's 64 x 64 mask, double buffered
  int kept[PP_MAX_Q];           // NMS positions of the first max_out survivors
  int n;
};

// row q of image b in view v, de-augmented: cx' cy' w' h'
template <typename T>
__device__ __forceinline__ void tta_box(const T* r, const float* __restrict__ vw, float (&o)[4]) {
  const float kx = vw[0], ky = vw[1];
  o[0] = Elt<T>::ld(r) * kx;
  if (vw[2] != 0.0f) o[0] = 1.0f - o[0];
  o[1] = Elt<T>::ld(r + 1) * ky;
  o[2] = Elt<T>::ld(r + 2) * kx;
  o[3] = Elt<T>::ld(r + 3) * ky;
}

// The merge's row source: candidate i = v nq + q is row q of view v; a sort key's low word is the candidate, which also indexes cls[]
template <typename T>
struct TtaRows {
  const TtaViews& ys;
  const float* views;
  const int* cls;  // by candidate
  size_t img;
  int nq, nd;
  __device__ __forceinline__ int cand(uint64_t key) const { return (int)(key & 0xffffffffu); }
  __device__ __forceinline__ int cls_of(uint64_t key) const { return cls[cand(key)]; }
  __device__ __forceinline__ const T* row(int i) const {
    const int v = i / nq;
    return static_cast<const T*>(ys.y[v]) + img + (size_t)(i - v * nq) * nd;
  }
  __device__ __forceinline__ void box(int i, float (&o)[4]) const { tta_box<T>(row(i), views + 4 * (i / nq), o); }
};

template <typename T, int GW>
__global__ __launch_bounds__(TTA_THREADS) void tta_merge_kernel(TtaViews ys, int V, int nq, int nd, const float* __restrict__ views,
                                                                float conf, float thr, int single_cls, float max_wh,
                                                                const int32_t* __restrict__ classes, int n_classes, int max_out,
                                                                float* __restrict__ ym, int32_t* __restrict__ src,
                                                                int32_t* __restrict__ counts, int32_t* __restrict__ dropped) {
  __shared__ TtaShared s;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
  const int nc = nd - 4, N = V * nq;
  const TtaRows<T> rows = {ys, views, s.cls, (size_t)b * nq * nd, nq, nd};
  if (tid == 0) s.n = 0;
  for (int w = tid; w < TTA_MAX_N / 64; w += TTA_THREADS) s.rem[w] = 0;
  __syncthreads();

  // ---- 1. class max, filter, sort key (a group of GW lanes per candidate)
  const int sub = tid & (GW - 1);
  int n_local = 0;
  for (int i0 = 0; i0 < N; i0 += TTA_THREADS / GW) {
    const int i = i0 + tid / GW;
    const bool row = i < N;  // uniform inside the group
    const int v = row ? i / nq : 0, q = row ? i - v * nq : 0;
    float bv;
    int bi;
    pp_row_max<T, GW>(static_cast<const T*>(ys.y[v]) + rows.img + (size_t)q * nd, nc, sub, row, bv, bi);
    if (row && sub == 0) {
      s.cls[i] = bi;
      const bool ok = pp_passes(bv, bi, conf, classes, n_classes);
      s.key[i] = ok ? ((uint64_t)~pp_ordered(bv) << 32) | (uint32_t)i : ~0ull;
      n_local += ok;
    }
  }
  int P = 1;
  while (P < N) P <<= 1;
  for (int i = N + tid; i < P; i += TTA_THREADS) s.key[i] = ~0ull;
  if (n_local) atomicAdd(&s.n, n_local);
  __syncthreads();
  const int n = s.n;

  // ---- 2 - 5 (postproc.h): sort of P <= 2048 keys (= NMS order; failed rows last), shifted boxes, greedy pass, outputs
  pp_bitonic_sort_pairs<TTA_THREADS>(s.key, P, tid);
  pp_merge_sbox<TTA_THREADS>(rows, s.key, n, single_cls, max_wh, s.sbox, tid);
  const int cnt = pp_greedy_tiles<TTA_WAVES, 0>(s.sbox, s.rem, s.tmask, s.kept, n, thr, max_out, wave, lane);  // the same in every thread
  __syncthreads();
  pp_merge_write<T, TTA_THREADS>(rows, s.key, s.kept, cnt, max_out, nd, b, tid, ym, src, counts, dropped);
}

template <typename T>
static void tta_launch(const TtaViews& ys, int V, int B, int nq, int nd, const float* views, float conf, float iou, int single_cls,
                       float max_wh, const int32_t* classes, int n_classes, int max_out, float* ym, int32_t* src, int32_t* counts,
                       int32_t* dropped, hipStream_t st) {
#define TTA_LAUNCH(GW)                                                                                                                  \
  hipLaunchKernelGGL((tta_merge_kernel<T, GW>), dim3(B), dim3(TTA_THREADS), 0, st, ys, V, nq, nd, views, conf, iou, single_cls, max_wh, \
                     classes, n_classes, max_out, ym, src, counts, dropped)
  PP_LAUNCH_GW(nd - 4, TTA_LAUNCH);
#undef TTA_LAUNCH
}

extern "C" int tamtr_tta_merge(const void* const* ys, int V, int dtype, int B, int nq, int nd, const float* views, float conf, float iou,
                               int single_cls, float max_wh, const int32_t* classes, int n_classes, int max_out, float* ym, int32_t* src,
                               int32_t* counts, int32_t* dropped, void* stream) {
  if (!ys || !views || !ym || !src || !counts || !dropped || V < 1 || B < 1 || nq < 1 || nd < 5 || n_classes < 0 || max_out < 1)
    return TAMTR_EINVAL;
  if (dtype != TAMTR_F32 && dtype != TAMTR_BF16) return TAMTR_EINVAL;
  TtaViews pv = {};
  for (int v = 0; v < V && v < TTA_MAX_V; ++v) {
    if (!ys[v]) return TAMTR_EINVAL;
    pv.y[v] = ys[v];
  }
  if (V > TTA_MAX_V || (int64_t)V * nq > TTA_MAX_N || max_out > PP_MAX_Q) return TAMTR_EUNSUP;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == TAMTR_F32)
    tta_launch<float>(pv, V, B, nq, nd, views, conf, iou, single_cls, max_wh, classes, n_classes, max_out, ym, src, counts, dropped, st);
  else
    tta_launch<bf16_t>(pv, V, B, nq, nd, views, conf, iou, single_cls, max_wh, classes, n_classes, max_out, ym, src, counts, dropped, st);
  return tamtr_launch_status();
}
