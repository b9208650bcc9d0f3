// postproc.h - device helpers shared by the two detection postprocess kernels: predict.hip (the predictor's rule) and
// valmatch.hip (the validator's rule), and by the two merges that feed them, tta.hip and slice.hip: the filter and the GW launch
// switch serve all four; the pair sort, the shifted boxes, the tile-wise greedy pass and the output stage (pp_merge_*) are the merges'
// common body, which sees a kernel's candidates through its row source.  All are compiled with -ffp-contract=off; every float
// operation here rounds on its own.
#pragma once
#include "common.h"

#define PP_MAX_Q 512
#define PP_WORDS (PP_MAX_Q / 64)
#define PP_THREADS 512

// torch.max over a row: NaN wins (lowest index among NaNs), else the larger value, equal values -> the lower index
__device__ __forceinline__ bool pp_better(float v, int i, float bv, int bi) {
  const bool vn = v != v, bn = bv != bv;
  if (vn || bn) return vn && (!bn || i < bi);
  return v > bv || (v == bv && i < bi);
}

// float -> uint32 with the same order (ascending); -0.0 folded onto +0.0
__device__ __forceinline__ uint32_t pp_ordered(float s) {
  uint32_t u = s == 0.0f ? 0u : __float_as_uint(s);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// std::max / std::min as torchvision calls them: max(a, b) = a < b ? b : a, min(a, b) = b < a ? b : a
__device__ __forceinline__ float pp_max(float a, float b) { return a < b ? b : a; }
__device__ __forceinline__ float pp_min(float a, float b) { return b < a ? b : a; }

// Class max of one row shared by an aligned group of GW lanes (lane `sub` of the group reads classes sub, sub + GW, ...): every lane
// of the group ends with the torch.max (value, index).  `row` is uniform inside the group; all lanes of the wave must call.
template <typename T, int GW>
__device__ __forceinline__ void pp_row_max(const T* r, int nc, int sub, bool row, float& bv, int& bi) {
  bv = __int_as_float(0xff800000);
  bi = 0x7fffffff;
  if (row)
    for (int c = sub; c < nc; c += GW) {
      const float v = Elt<T>::ld(r + 4 + c);
      if (pp_better(v, c, bv, bi)) { bv = v; bi = c; }
    }
#pragma unroll
  for (int o = GW / 2; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o, WAVE);
    const int oi = __shfl_xor(bi, o, WAVE);
    if (pp_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
  }
}

// The filter: a row needs score > conf (a NaN score fails) and, with a class filter, its class among classes[0 .. n_classes).
__device__ __forceinline__ bool pp_passes(float bv, int bi, float conf, const int32_t* __restrict__ classes, int n_classes) {
  bool ok = bv > conf;
  if (ok && classes) {
    bool in = false;
    for (int k = 0; k < n_classes; ++k) in |= classes[k] == bi;
    ok = in;
  }
  return ok;
}

// The class-max group width GW from the class count nc: 4 lanes per row up to 8 classes, 16 up to 32, else a whole wave.  LAUNCH(GW) is
// the caller's launch statement.
#define PP_LAUNCH_GW(nc, LAUNCH)         \
  do {                                   \
    if ((nc) <= 8) { LAUNCH(4); }        \
    else if ((nc) <= 32) { LAUNCH(16); } \
    else { LAUNCH(64); }                 \
  } while (0)

// Bitonic sort of P <= PP_THREADS keys in LDS, ascending (P a power of two), one key per thread; called by the whole workgroup, ends on a
// barrier.  predict.hip's and valmatch.hip's: measured against pp_bitonic_sort_pairs at P = 512 it saves the pair index arithmetic of 45
// latency-bound steps, about 1.5 us of a 95 us launch (profiles/merge_shared_stages.txt).
__device__ __forceinline__ void pp_bitonic_sort(uint64_t* key, int P, int tid) {
  for (int k = 2; k <= P; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      const int i = tid, l = i ^ j;
      if (i < P && l > i) {
        const uint64_t a = key[i], c = key[l];
        if ((a > c) == ((i & k) == 0)) { key[i] = c; key[l] = a; }
      }
      __syncthreads();
    }
  }
}

// The same sort for any P, by a workgroup of THREADS: thread t takes pairs t, t + THREADS, ... of every step, one barrier per step; ends
// on a barrier.  The merges' (P up to 4096 on 1024 threads).  The keys are unique apart from the ~0ull fillers, so the sorted array does
// not depend on which of the two networks produced it.
template <int THREADS>
__device__ __forceinline__ void pp_bitonic_sort_pairs(uint64_t* key, int P, int tid) {
  for (int k = 2; k <= P; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < P / 2; t += THREADS) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
        const uint64_t a = key[i], c = key[l];
        if ((a > c) == ((i & k) == 0)) { key[i] = c; key[l] = a; }
      }
      __syncthreads();
    }
  }
}

// Upper-triangular suppression mask of n boxes in NMS order: word (i, w) bit l = iou(i, 64 w + l) > thr for 64 w + l > i, with
// torchvision's nms_kernel.cpp arithmetic (operand order included).  Built by whole waves: lane l computes one IoU, a ballot forms
// the word.  The caller puts a barrier after it.
__device__ __forceinline__ void pp_nms_mask(const float (*sbox)[4], const float* sarea, uint64_t (*mask)[PP_WORDS], int n, float thr,
                                            int wave, int lane) {
  const int nw = (n + WAVE - 1) / WAVE;
  for (int t = wave; t < n * nw; t += PP_THREADS / WAVE) {
    const int i = t / nw, w = t - i * nw, j = w * WAVE + lane;
    uint64_t word = 0;
    if (w * WAVE + WAVE - 1 > i) {  // uniform over the wave
      bool sup = false;
      if (j > i && j < n) {
        const float ix1 = sbox[i][0], iy1 = sbox[i][1], ix2 = sbox[i][2], iy2 = sbox[i][3];
        const float xx1 = pp_max(ix1, sbox[j][0]), yy1 = pp_max(iy1, sbox[j][1]);
        const float xx2 = pp_min(ix2, sbox[j][2]), yy2 = pp_min(iy2, sbox[j][3]);
        const float ww = pp_max(0.0f, xx2 - xx1), hh = pp_max(0.0f, yy2 - yy1);
        const float inter = ww * hh;
        const float ovr = inter / ((sarea[i] + sarea[j]) - inter);
        sup = ovr > thr;
      }
      word = __ballot(sup);
    }
    if (lane == 0) mask[i][w] = word;
  }
}

// Greedy pass over the mask, run by ONE wave with no barrier: lane k < nw holds removal word k; every row is tested with a readlane
// of its word.  kept[] receives the positions of the kept rows in order; returns their number (same value in every lane).
__device__ __forceinline__ int pp_greedy(const uint64_t (*mask)[PP_WORDS], int* kept, int n, int lane) {
  const int nw = (n + WAVE - 1) / WAVE;
  uint64_t rem = 0;
  int cnt = 0;
  for (int i = 0; i < n; ++i) {
    const int wi = i >> 6;
    const uint32_t lo = __builtin_amdgcn_readlane((uint32_t)rem, wi), hi = __builtin_amdgcn_readlane((uint32_t)(rem >> 32), wi);
    const uint64_t rw = ((uint64_t)hi << 32) | lo;
    if (!((rw >> (i & 63)) & 1ull)) {
      if (lane == 0) kept[cnt] = i;
      ++cnt;
      if (lane < nw) rem |= mask[i][lane];
    }
  }
  return cnt;
}

// Overlap of two shifted corner boxes with torchvision's nms_kernel.cpp arithmetic (operand order included), as pp_nms_mask has it; `a`
// is the earlier (kept) row.  MATCH 0: IoU = inter / ((area_a + area_b) - inter).  MATCH 1: IoS = inter / min(area_a, area_b), the
// intersection over the smaller box.  0 / 0 is NaN, which no `> thr` passes.
template <int MATCH>
__device__ __forceinline__ float pp_overlap(const float* a, float area_a, const float* b) {
  const float xx1 = pp_max(a[0], b[0]), yy1 = pp_max(a[1], b[1]);
  const float xx2 = pp_min(a[2], b[2]), yy2 = pp_min(a[3], b[3]);
  const float ww = pp_max(0.0f, xx2 - xx1), hh = pp_max(0.0f, yy2 - yy1);
  const float inter = ww * hh;
  const float area_b = (b[2] - b[0]) * (b[3] - b[1]);
  if (MATCH == 1) return inter / pp_min(area_a, area_b);
  return inter / ((area_a + area_b) - inter);
}

__device__ __forceinline__ uint64_t pp_uniform(uint64_t v) {
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
  return ((uint64_t)hi << 32) | lo;  // (the builtins return int: no sign extension of the low word)
}

// Greedy NMS over n boxes in NMS order without an n x n mask, by a workgroup of WAVES waves, over tiles of 64 rows with one barrier per
// tile: the waves build the tile's 64 x 64 mask with ballots (tmask, double buffered); every wave resolves it by itself from registers
// (lane r holds row r's word, 64 readlanes) starting from the tile's removed word; then the tile's kept rows strike all later rows in
// parallel - a wave owns the removed words it writes.  rem: one removed bit per row, ceil(n / 64) words, zero on entry (and a barrier
// behind the zeroing and the boxes).  kept[] receives the positions of the first max_out kept rows in order; returns the number of
// kept rows (the same value in every thread).  The caller puts a barrier after it.
template <int WAVES, int MATCH>
__device__ __forceinline__ int pp_greedy_tiles(const float (*sbox)[4], uint64_t* rem, uint64_t (*tmask)[64], int* kept, int n, float thr,
                                               int max_out, int wave, int lane) {
  const int nw = (n + WAVE - 1) / WAVE;
  int cnt = 0;
  for (int t = 0; t < nw; ++t) {
    const int base = t * WAVE;
    uint64_t* tm = tmask[t & 1];
    // the tile's mask: word r bit l = overlap(base + r, base + l) > thr for l > r
    for (int r = wave; r < WAVE; r += WAVES) {
      bool sup = false;
      const int i = base + r, j = base + lane;
      if (i < n && j < n && lane > r) {
        const float* bi = sbox[i];
        sup = pp_overlap<MATCH>(bi, (bi[2] - bi[0]) * (bi[3] - bi[1]), sbox[j]) > thr;
      }
      const uint64_t word = __ballot(sup);
      if (lane == 0) tm[r] = word;
    }
    __syncthreads();  // also orders the previous tile's strikes before this tile's read of rem[t]
    // resolve, by every wave for itself: lane r holds row r's word
    const uint64_t mine = tm[lane];
    uint64_t cur = pp_uniform(rem[t]);
    if (n - base < WAVE) cur |= ~0ull << (n - base);  // positions past n are no rows
    uint64_t keptw = 0;
    for (int r = 0; r < WAVE; ++r) {
      if (!((cur >> r) & 1ull)) {
        keptw |= 1ull << r;
        const uint32_t lo = __builtin_amdgcn_readlane((uint32_t)mine, r), hi = __builtin_amdgcn_readlane((uint32_t)(mine >> 32), r);
        cur |= ((uint64_t)hi << 32) | lo;
      }
    }
    if (wave == 0 && ((keptw >> lane) & 1ull)) {
      const int pos = cnt + __popcll(keptw & ((1ull << lane) - 1ull));
      if (pos < max_out) kept[pos] = base + lane;
    }
    cnt += __popcll(keptw);
    // the tile's kept rows strike the later rows: wave w owns removed word t + 1 + w, t + 1 + w + WAVES, ...
    for (int w = t + 1 + wave; w < nw; w += WAVES) {
      const int j = w * WAVE + lane;
      const uint64_t had = rem[w];
      bool sup = false;
      if (j < n && !((had >> lane) & 1ull)) {
        const float bj[4] = {sbox[j][0], sbox[j][1], sbox[j][2], sbox[j][3]};
        for (uint64_t m = keptw; m && !sup; m &= m - 1) {
          const float* bi = sbox[base + __builtin_ctzll(m)];
          sup = pp_overlap<MATCH>(bi, (bi[2] - bi[0]) * (bi[3] - bi[1]), bj) > thr;
        }
      }
      const uint64_t word = __ballot(sup);
      if (lane == 0 && word) rem[w] = had | word;
    }
  }
  return cnt;
}

// ---- the merges' common body (tta.hip, slice.hip).  A kernel hands its candidates over as a row source `rows`, a small struct passed by
// value: cand(key) = the candidate of a sort key, cls_of(key) = its class, row(i) = candidate i's source row, box(i, o) = its box
// cx' cy' w' h' in the merged frame.

// cx cy w h -> the corner box shifted by cls * max_wh (not at all when single_cls), as the NMS sees it
__device__ __forceinline__ void pp_shifted_box(const float (&c)[4], int cls, int single_cls, float max_wh, float* out) {
  const float dw = c[2] / 2.0f, dh = c[3] / 2.0f;
  const float sh = (float)cls * (single_cls ? 0.0f : max_wh);
  out[0] = (c[0] - dw) + sh;
  out[1] = (c[1] - dh) + sh;
  out[2] = (c[0] + dw) + sh;
  out[3] = (c[1] + dh) + sh;
}

// Shifted corner boxes of the n sorted candidates, in NMS order (the four box numbers are read again from global memory: 16 bytes per
// row, no LDS copy); ends on a barrier.
template <int THREADS, typename Rows>
__device__ __forceinline__ void pp_merge_sbox(const Rows rows, const uint64_t* key, int n, int single_cls, float max_wh, float (*sbox)[4],
                                              int tid) {
  for (int p = tid; p < n; p += THREADS) {
    float c[4];
    rows.box(rows.cand(key[p]), c);
    pp_shifted_box(c, rows.cls_of(key[p]), single_cls, max_wh, sbox[p]);
  }
  __syncthreads();
}

// Outputs of image b from the greedy pass's kept[] and cnt: the first max_out survivors in order - the box recomputed, the source row's
// scores widened exactly - then zero rows; src = the candidate, -1 after them; counts = rows written, dropped = survivors that did not
// fit.  Coalesced over ym.
template <typename T, int THREADS, typename Rows>
__device__ __forceinline__ void pp_merge_write(const Rows rows, const uint64_t* key, const int* kept, int cnt, int max_out, int nd, int b,
                                               int tid, float* __restrict__ ym, int32_t* __restrict__ src, int32_t* __restrict__ counts,
                                               int32_t* __restrict__ dropped) {
  const int n_rows = cnt < max_out ? cnt : max_out;
  float* ob = ym + (size_t)b * max_out * nd;
  for (int e = tid; e < max_out * nd; e += THREADS) {
    const int r = e / nd, c = e - r * nd;
    float val = 0.0f;
    if (r < n_rows) {
      const int i = rows.cand(key[kept[r]]);
      if (c < 4) {
        float bx[4];
        rows.box(i, bx);
        val = bx[c];
      } else {
        val = Elt<T>::ld(rows.row(i) + c);
      }
    }
    ob[e] = val;
  }
  for (int r = tid; r < max_out; r += THREADS) src[(size_t)b * max_out + r] = r < n_rows ? rows.cand(key[kept[r]]) : -1;
  if (tid == 0) {
    counts[b] = n_rows;
    dropped[b] = cnt - n_rows;
  }
}
