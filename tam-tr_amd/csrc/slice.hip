// slice.hip - sliced prediction for large frames on the device: one launch cuts the windows of one original frame into network inputs
// (tamtr_slice_views), one launch maps every view's rows back to its frame and merges them into an ordinary prediction tensor
// (tamtr_slice_merge).
//
// Replaces what sliced inference does around a detector on the host (crop, resize, forward per crop, shift the boxes, NMS or
// "non-maximum merging" with an IoU or an intersection-over-smaller metric): the reference has no such mode - its predictor stretches
// the whole frame (models/rtdetrworld/predict.py:80-92) - so the two rules below are this project's, stated in tam-tr_amd/slicing.py
// (views_host, merge_host) and held to them bit for bit.
//
// ---- tamtr_slice_views: out[v] = CHW(float(resize_linear_u8(src[y0:y1, x0:x1], S, S)) / 255): predict.letterbox_scalefill and
// to_model_input applied to the crop (`/ 255` as the device evaluates it there: a multiplication by float(1.0 / 255.0)).  The three
// branches of tamtr_resize_linear_u8 (csrc/host/imgproc.c):
//   copy      a window already S x S
//   2x2 mean  a window exactly 2S x 2S: (a + b + c + d + 2) >> 2
//   general   per axis, tap f = (float)((d + 0.5) * ((double)sn / dn) - 0.5) in double (no FMA: -ffp-contract=off), s = floor(f),
//             fraction f - s; horizontally the fraction is zeroed when s < 0 or s >= sn - 1, vertically it is not (both rows are then
//             the same clamped row); the two weights of an axis are rounded on their own, lrintf((1 - fr) * 2048) and
//             lrintf(fr * 2048) (round-half-even); horizontal pass r[x0] * w0 + r[x1] * w1 in int; vertical pass
//             sat_u8((((b0 * (top >> 4)) >> 16) + ((b1 * (bot >> 4)) >> 16) + 2) >> 2).
// Memory bound: a workgroup writes SL_VIEW_THREADS consecutive pixels of one output row for the three planes (coalesced stores); the
// row's vertical taps and weights depend on the block index alone (scalar), the column's are computed once per pixel, not per channel;
// the gather touches two source rows.  The windows travel as a kernel argument (at most SL_MAX_V of them): they are checked on the
// host, so no thread can read outside the frame.
//
// ---- tamtr_slice_merge: frame b owns views view_off[b] .. view_off[b + 1] - 1 of y; candidate i = v_local nq + q is row q of its
// v_local-th view.  Every fp32 operation rounds on its own, the input is widened to fp32:
//   map         cx' = cx kx + ox; cy' = cy ky + oy; w' = w kx; h' = h ky (the whole-frame view: ox = 0, kx = 1 - the identity)
//   score, cls  torch.max over the nc scores (pp_row_max); a candidate needs score > conf and, with a filter, cls in classes[]
//   capacity    the passing candidates in ascending i; the first SL_MAX_C of them go on, overflow = the number of the others
//   order       descending score, equal scores by ascending i
//   NMS         tamtr_tta_merge's: shifted corner boxes, class-aware unless single_cls, greedy; row j goes when overlap > thr in fp32,
//               overlap = IoU (match 0) or inter / min(area_a, area_b) (match 1); NaN does not suppress
//   output      the first max_out survivors in order: cx' cy' w' h' and the source row's nc scores widened exactly; src = i; zero rows
//               and src = -1 after them; counts = rows written, dropped = survivors that did not fit.
//
// Design: one workgroup of 16 waves per frame, up to 64 x 512 = 32768 candidates, of which SL_MAX_C = 4096 may pass the filter.
//   1. class max per row by groups of GW lanes (coalesced), filter, one bit per candidate in LDS (an OR into a bit mask: the result
//      does not depend on the order of the atomics).
//   2. popcount per mask word, exclusive prefix sum over the <= 512 words (wave scans, then the wave totals): the compacted position
//      of candidate i is its word's offset + the set bits below it - ascending i, no counter that threads race for.
//   3. the compacted table: candidate index per position; class max again for the <= SL_MAX_C rows that go on (16 to 320 bytes each,
//      cheaper than an LDS copy of 32768 scores), sort key (~ordered(score) << 32 | position: positions ascend with i).
//   4. the stages of postproc.h, shared with tta.hip, which reach the candidates through SlRows: bitonic sort over the next power of
//      two of the table (pp_bitonic_sort_pairs), shifted corner boxes in NMS order (pp_merge_sbox), the tile-wise greedy pass
//      (pp_greedy_tiles), coalesced write of ym / src and two counters (pp_merge_write); overflow is written here.
// LDS: key 32 KB + cand 16 KB + cls 16 KB + sbox 64 KB + candidate mask 4 KB + word offsets 2 KB + rem 0.5 KB + tile masks 1 KB +
// kept 2 KB = about 138 KB of the CU's 160 KB; one workgroup per CU, which 16 waves fill to half its wave slots anyway.
#include "postproc.h"

#define SL_MAX_V 64
#define SL_MAX_NQ 512
#define SL_MAX_B 255
#define SL_MAX_C 4096
#define SL_MAX_N (SL_MAX_V * SL_MAX_NQ)
#define SL_WORDS (SL_MAX_N / 64)
#define SL_THREADS 1024
#define SL_WAVES (SL_THREADS / WAVE)
#define SL_VIEW_THREADS 256

// ------------------------------------------------------------------------------------------------ the views
struct SlWindows {
  int w[SL_MAX_V][4];  // x0 y0 x1 y1
};

struct SlTap {
  int i0, i1, w0, w1;
};

// linear_taps + the weights of imgproc.c for destination index d of an axis: sn source samples -> dn; `zero_outside`: the horizontal
// rule (fraction zeroed when the tap falls outside 0 .. sn - 2)
__device__ __forceinline__ SlTap sl_tap(int d, int sn, int dn, bool zero_outside) {
  const double scale = (double)sn / (double)dn;
  const float f = (float)(((double)d + 0.5) * scale - 0.5);
  const float fl = floorf(f);
  const int s = (int)fl;
  float fr = f - fl;
  if (zero_outside && (s < 0 || s >= sn - 1)) fr = 0.0f;
  SlTap t;
  t.i0 = min(max(s, 0), sn - 1);
  t.i1 = zero_outside ? min(t.i0 + 1, sn - 1) : min(max(s + 1, 0), sn - 1);
  t.w0 = (int)rintf((1.0f - fr) * 2048.0f);
  t.w1 = (int)rintf(fr * 2048.0f);
  return t;
}

__global__ __launch_bounds__(SL_VIEW_THREADS) void slice_views_kernel(const uint8_t* __restrict__ src, SlWindows win, float* __restrict__ out,
                                                                      int w, int S) {
  const int ox = blockIdx.x * SL_VIEW_THREADS + threadIdx.x, oy = blockIdx.y, v = blockIdx.z;
  if (ox >= S) return;
  const int x0 = win.w[v][0], y0 = win.w[v][1], sw = win.w[v][2] - x0, sh = win.w[v][3] - y0;
  const size_t pitch = (size_t)w * 3, plane = (size_t)S * S;
  const uint8_t* base = src + (size_t)y0 * pitch + (size_t)x0 * 3;  // the crop's first pixel
  float* ob = out + ((size_t)v * 3 * S + oy) * S + ox;
  int val[3];
  if (sh == S && sw == S) {
    const uint8_t* p = base + (size_t)oy * pitch + (size_t)ox * 3;
    for (int c = 0; c < 3; ++c) val[c] = p[c];
  } else if (sw == 2 * S && sh == 2 * S) {
    const uint8_t *r0 = base + (size_t)(2 * oy) * pitch + (size_t)(2 * ox) * 3, *r1 = r0 + pitch;
    for (int c = 0; c < 3; ++c) val[c] = (r0[c] + r0[3 + c] + r1[c] + r1[3 + c] + 2) >> 2;
  } else {
    const SlTap ty = sl_tap(oy, sh, S, false), tx = sl_tap(ox, sw, S, true);
    const uint8_t *r0 = base + (size_t)ty.i0 * pitch, *r1 = base + (size_t)ty.i1 * pitch;
    const int a = tx.i0 * 3, b = tx.i1 * 3;
    for (int c = 0; c < 3; ++c) {
      const int top = r0[a + c] * tx.w0 + r0[b + c] * tx.w1, bot = r1[a + c] * tx.w0 + r1[b + c] * tx.w1;
      const int r = (((ty.w0 * (top >> 4)) >> 16) + ((ty.w1 * (bot >> 4)) >> 16) + 2) >> 2;
      val[c] = r < 0 ? 0 : (r > 255 ? 255 : r);
    }
  }
  // to_model_input's `.float() / 255`, which torch evaluates on the device as a multiplication by float(1.0 / 255.0) (division by a
  // host scalar, ATen BinaryDivTrueKernel; imgaug.hip does the same), so a view has the bits of the plain predictor's input
  for (int c = 0; c < 3; ++c) ob[c * plane] = __fmul_rn((float)val[c], (float)(1.0 / 255.0));
}

extern "C" int tamtr_slice_views(const uint8_t* src, int h, int w, const int32_t* windows, int V, int S, float* out, void* stream) {
  if (!src || !windows || !out || h < 1 || w < 1 || V < 1 || S < 1) return TAMTR_EINVAL;
  SlWindows win = {};
  for (int v = 0; v < V; ++v) {
    const int32_t* q = windows + 4 * v;
    if (q[0] < 0 || q[1] < 0 || q[2] > w || q[3] > h || q[0] >= q[2] || q[1] >= q[3]) return TAMTR_EINVAL;
    for (int k = 0; k < 4 && v < SL_MAX_V; ++k) win.w[v][k] = q[k];
  }
  if (V > SL_MAX_V || S > 65535) return TAMTR_EUNSUP;  // the argument table; grid y
  hipLaunchKernelGGL(slice_views_kernel, dim3((S + SL_VIEW_THREADS - 1) / SL_VIEW_THREADS, S, V), dim3(SL_VIEW_THREADS), 0,
                     (hipStream_t)stream, src, win, out, w, S);
  return tamtr_launch_status();
}

// ------------------------------------------------------------------------------------------------ the merge
struct SlOffsets {
  int off[SL_MAX_B + 1];
};

struct SlShared {
  uint64_t key[SL_MAX_C];      // sort keys by compacted position; after the sort, entry p holds the p-th candidate in NMS order
  int cand[SL_MAX_C];          // candidate i by compacted position (ascending)
  int cls[SL_MAX_C];           // by compacted position
  float sbox[SL_MAX_C][4];     // shifted x1 y1 x2 y2 in NMS order
  uint32_t mask[2 * SL_WORDS]; // bit i: candidate i passes the filter (read back as 64-bit words)
  int woff[SL_WORDS];          // passing candidates before 64-bit word w
  uint64_t rem[SL_MAX_C / 64]; // removed bit per NMS position
  uint64_t tmask[2][64];       // the current tile's 64 x 64 mask, double buffered
  int kept[PP_MAX_Q];          // NMS positions of the first max_out survivors
  int wsum[SL_WORDS / WAVE];   // the scan's wave totals
  int n_pass;
};

// row q of view v mapped to its frame: cx' cy' w' h'
template <typename T>
__device__ __forceinline__ void sl_box(const T* r, const float* __restrict__ vw, float (&o)[4]) {
  const float ox = vw[0], oy = vw[1], kx = vw[2], ky = vw[3];
  o[0] = Elt<T>::ld(r) * kx + ox;
  o[1] = Elt<T>::ld(r + 1) * ky + oy;
  o[2] = Elt<T>::ld(r + 2) * kx;
  o[3] = Elt<T>::ld(r + 3) * ky;
}

// The merge's row source: the frame's rows are contiguous, candidate i is row i; a sort key's low word is a compacted position, which
// indexes cand[] and cls[]
template <typename T>
struct SlRows {
  const T* yb;
  const float* vb;
  const int *cands, *cls;  // by compacted position
  int nq, nd;
  __device__ __forceinline__ int cand(uint64_t key) const { return cands[key & 0xffffffffu]; }
  __device__ __forceinline__ int cls_of(uint64_t key) const { return cls[key & 0xffffffffu]; }
  __device__ __forceinline__ const T* row(int i) const { return yb + (size_t)i * nd; }
  __device__ __forceinline__ void box(int i, float (&o)[4]) const { sl_box<T>(row(i), vb + 4 * (i / nq), o); }
};

template <typename T, int GW, int MATCH>
__global__ __launch_bounds__(SL_THREADS) void slice_merge_kernel(const T* __restrict__ y, SlOffsets offs, int nq, int nd,
                                                                 const float* __restrict__ views, float conf, float thr, int single_cls,
                                                                 float max_wh, const int32_t* __restrict__ classes, int n_classes,
                                                                 int max_out, float* __restrict__ ym, int32_t* __restrict__ src,
                                                                 int32_t* __restrict__ counts, int32_t* __restrict__ dropped,
                                                                 int32_t* __restrict__ overflow) {
  __shared__ SlShared s;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
  const int nc = nd - 4, v0 = offs.off[b], N = (offs.off[b + 1] - v0) * nq;  // N <= SL_MAX_N: checked by the host
  const T* yb = y + (size_t)v0 * nq * nd;                                     // the frame's rows are contiguous: candidate i is row i
  const SlRows<T> rows = {yb, views + (size_t)v0 * 4, s.cand, s.cls, nq, nd};
  const uint64_t* mask64 = reinterpret_cast<const uint64_t*>(s.mask);
  for (int w = tid; w < 2 * SL_WORDS; w += SL_THREADS) s.mask[w] = 0;
  for (int w = tid; w < SL_MAX_C / 64; w += SL_THREADS) s.rem[w] = 0;
  __syncthreads();

  // ---- 1. class max and filter (a group of GW lanes per candidate): one bit per candidate
  const int sub = tid & (GW - 1);
  for (int i0 = 0; i0 < N; i0 += SL_THREADS / GW) {
    const int i = i0 + tid / GW;
    const bool row = i < N;  // uniform inside the group
    float bv;
    int bi;
    pp_row_max<T, GW>(rows.row(row ? i : 0), nc, sub, row, bv, bi);
    if (row && sub == 0 && pp_passes(bv, bi, conf, classes, n_classes)) atomicOr(&s.mask[i >> 5], 1u << (i & 31));
  }
  __syncthreads();

  // ---- 2. exclusive prefix sum of the words' popcounts: thread t < SL_WORDS owns word t (waves 0 .. SL_WORDS / 64 - 1)
  {
    const int c = tid < SL_WORDS ? __popcll(mask64[tid]) : 0;
    int inc = c;
    for (int o = 1; o < WAVE; o <<= 1) {
      const int up = __shfl_up(inc, o, WAVE);
      if (lane >= o) inc += up;
    }
    if (tid < SL_WORDS && lane == WAVE - 1) s.wsum[wave] = inc;
    __syncthreads();
    if (tid < SL_WORDS) {
      int before = 0;
      for (int k = 0; k < wave; ++k) before += s.wsum[k];
      s.woff[tid] = before + inc - c;
      if (tid == SL_WORDS - 1) s.n_pass = before + inc;
    }
    __syncthreads();
  }
  const int n_pass = s.n_pass, n = n_pass < SL_MAX_C ? n_pass : SL_MAX_C;

  // ---- 3. the compacted table, ascending i: the passing candidates beyond SL_MAX_C (the highest i) stay out
  for (int i = tid; i < N; i += SL_THREADS) {
    const uint64_t word = mask64[i >> 6];
    if ((word >> (i & 63)) & 1ull) {
      const int pos = s.woff[i >> 6] + __popcll(word & ((1ull << (i & 63)) - 1ull));
      if (pos < SL_MAX_C) s.cand[pos] = i;
    }
  }
  __syncthreads();
  for (int p0 = 0; p0 < n; p0 += SL_THREADS / GW) {
    const int p = p0 + tid / GW;
    const bool row = p < n;
    float bv;
    int bi;
    pp_row_max<T, GW>(rows.row(row ? s.cand[p] : 0), nc, sub, row, bv, bi);
    if (row && sub == 0) {
      s.cls[p] = bi;
      s.key[p] = ((uint64_t)~pp_ordered(bv) << 32) | (uint32_t)p;
    }
  }
  int P = 1;
  while (P < n) P <<= 1;
  for (int p = n + tid; p < P; p += SL_THREADS) s.key[p] = ~0ull;
  __syncthreads();

  // ---- 4. (postproc.h) sort of P <= SL_MAX_C keys (= NMS order), shifted boxes, greedy pass, outputs
  pp_bitonic_sort_pairs<SL_THREADS>(s.key, P, tid);
  pp_merge_sbox<SL_THREADS>(rows, s.key, n, single_cls, max_wh, s.sbox, tid);
  const int cnt = pp_greedy_tiles<SL_WAVES, MATCH>(s.sbox, s.rem, s.tmask, s.kept, n, thr, max_out, wave, lane);
  __syncthreads();
  pp_merge_write<T, SL_THREADS>(rows, s.key, s.kept, cnt, max_out, nd, b, tid, ym, src, counts, dropped);
  if (tid == 0) overflow[b] = n_pass - n;
}

template <typename T>
static void sl_launch(const void* y, const SlOffsets& offs, int B, int nq, int nd, const float* views, int match, float conf, float thr,
                      int single_cls, float max_wh, const int32_t* classes, int n_classes, int max_out, float* ym, int32_t* src,
                      int32_t* counts, int32_t* dropped, int32_t* overflow, hipStream_t st) {
#define SL_LAUNCH_M(GW, M)                                                                                                                  \
  hipLaunchKernelGGL((slice_merge_kernel<T, GW, M>), dim3(B), dim3(SL_THREADS), 0, st, static_cast<const T*>(y), offs, nq, nd, views, conf, \
                     thr, single_cls, max_wh, classes, n_classes, max_out, ym, src, counts, dropped, overflow)
#define SL_LAUNCH(GW) if (match == 0) SL_LAUNCH_M(GW, 0); else SL_LAUNCH_M(GW, 1)
  PP_LAUNCH_GW(nd - 4, SL_LAUNCH);
#undef SL_LAUNCH
#undef SL_LAUNCH_M
}

extern "C" int tamtr_slice_merge(const void* y, int dtype, int N, int B, int nq, int nd, const int32_t* view_off, const float* views,
                                 int match, float conf, float iou, int single_cls, float max_wh, const int32_t* classes, int n_classes,
                                 int max_out, float* ym, int32_t* src, int32_t* counts, int32_t* dropped, int32_t* overflow,
                                 void* stream) {
  if (!y || !view_off || !views || !ym || !src || !counts || !dropped || !overflow || N < 1 || B < 1 || nq < 1 || nd < 5 ||
      n_classes < 0 || max_out < 1)
    return TAMTR_EINVAL;
  if ((dtype != TAMTR_F32 && dtype != TAMTR_BF16) || (match != 0 && match != 1)) return TAMTR_EINVAL;
  if (B > SL_MAX_B) return TAMTR_EUNSUP;
  SlOffsets offs = {};
  bool wide = false;
  if (view_off[0] != 0 || view_off[B] != N) return TAMTR_EINVAL;
  for (int b = 0; b < B; ++b) {
    const int nv = view_off[b + 1] - view_off[b];
    if (view_off[b] < 0 || nv < 1) return TAMTR_EINVAL;  // every frame owns at least one view
    wide |= nv > SL_MAX_V;
    offs.off[b] = view_off[b];
  }
  offs.off[B] = N;
  if (wide || nq > SL_MAX_NQ || max_out > PP_MAX_Q) return TAMTR_EUNSUP;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == TAMTR_F32)
    sl_launch<float>(y, offs, B, nq, nd, views, match, conf, iou, single_cls, max_wh, classes, n_classes, max_out, ym, src, counts, dropped,
                     overflow, st);
  else
    sl_launch<bf16_t>(y, offs, B, nq, nd, views, match, conf, iou, single_cls, max_wh, classes, n_classes, max_out, ym, src, counts, dropped,
                      overflow, st);
  return tamtr_launch_status();
}
