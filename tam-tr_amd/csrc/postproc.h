// postproc.h - device helpers shared by the two detection postprocess kernels: predict.hip (the predictor's rule) and
// valmatch.hip (the validator's rule).  Both are compiled with -ffp-contract=off; every float operation here rounds on its own.
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

// Bitonic sort of P <= PP_THREADS keys in LDS, ascending (P a power of two); called by the whole workgroup, ends on a barrier.
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
