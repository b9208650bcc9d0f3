// text.hip - the frozen CLIP text tower's own kernels (fp32 end to end, forward only): token + position embedding, a dense layer on the
// fp32 MFMA with a fused epilogue, and the pooled projection.  Replaces clip.model.CLIP.encode_text as the reference calls it at
// ultralytics/models/rtdetrworld/train.py:148-150, nn/tasks.py:552-571 (set_classes) and the validator's vocabulary.  Attention and the
// blocks' LayerNorms run on tamtr_selfattn_fwd / tamtr_layernorm_fwd.
#include "common.h"

// ------------------------------------------------------------------------------------------------ embedding front end
// x[r, :] = tok[ids[r], :] + pos[r % L, :], one lane per 4 channels.  An id outside [0, V) is never used as an index: its row becomes NaN
// (the Python wrapper refuses such ids before the launch; a caller of the C ABI sees them in the output).
__global__ __launch_bounds__(256) void text_embed_kernel(const int32_t* __restrict__ ids, const float* __restrict__ tok,
                                                         const float* __restrict__ pos, float* __restrict__ x, long long rows, int L, int W4,
                                                         int V) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * W4) return;
  const long long r = i / W4;
  const int c = (int)(i - r * W4);
  const int id = ids[r];
  float4 o;
  if (id < 0 || id >= V) {
    const float q = __uint_as_float(0x7fc00000u);
    o = make_float4(q, q, q, q);
  } else {
    const float4 t = reinterpret_cast<const float4*>(tok)[(long long)id * W4 + c];
    const float4 p = reinterpret_cast<const float4*>(pos)[(long long)(r % L) * W4 + c];
    o = make_float4(t.x + p.x, t.y + p.y, t.z + p.z, t.w + p.w);
  }
  reinterpret_cast<float4*>(x)[i] = o;
}

extern "C" int tamtr_text_embed(const int32_t* ids, const float* tok, const float* pos, float* x, long long n, int L, int W, int V,
                                void* stream) {
  if (!ids || !tok || !pos || !x || n < 1 || L < 1 || W < 1 || V < 1) return TAMTR_EINVAL;
  if (W % 4 || (((uintptr_t)tok | (uintptr_t)pos | (uintptr_t)x) % 16)) return TAMTR_EUNSUP;
  const long long work = n * L * (W / 4);
  if ((work + 255) / 256 > 0x7fffffffLL) return TAMTR_EUNSUP;
  hipLaunchKernelGGL(text_embed_kernel, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, (hipStream_t)stream, ids, tok, pos, x, n * L, L,
                     W / 4, V);
  return tamtr_launch_status();
}

// ------------------------------------------------------------------------------------------------ fp32 dense layer
// Y[M,N] = epi(X[M,K] @ W[N,K]^T + bias).  A workgroup of four waves owns a 64 x 64 tile of Y, a wave one 32 x 32 quadrant in the 16
// accumulator registers of v_mfma_f32_32x32x2_f32.  M is 77 n (hundreds to a few thousand rows) and N 512 .. 2048, so the tile is small: at
// n = 80, N = 512 there are 97 x 8 workgroups for the 256 CUs, where a 128 x 128 tile would leave a quarter of them idle.  Per k-tile of 32
// both operands are staged in LDS row by row ([row][k], pitch 36 words: 16-byte rows for the float4 stores, and the 16 lanes of a
// ds_read_b128 phase start 36 words apart = on 16 different bank quads).  The MFMA sums over k in any order as long as A and B agree, so
// lane half h takes k = 16 h + j at step j: a lane's 16 operands of a k-tile are contiguous and come in as four ds_read_b128 per matrix
// instead of sixteen ds_read_b32.  The next k-tile travels from HBM / L2 in registers while the current one is multiplied.  Every output
// element is one ordered chain (k-tiles ascending, inside a tile j ascending, lane half 0 before 1): no split-K, no atomics, same bits on
// every run.  Rows >= M read as zeros and are not stored.
#define LT_B 64    // tile edge (M and N)
#define LT_K 32    // k-tile
#define LT_LD 36   // LDS row pitch in words

enum { EPI_NONE = 0, EPI_QUICKGELU = 1, EPI_RESIDUAL = 2 };

template <int EPI>
__global__ __launch_bounds__(256) void linear_f32_kernel(const float* __restrict__ X, const float* __restrict__ Wt,
                                                         const float* __restrict__ bias, const float* R, float* Y, int M, int N, int K) {
  __shared__ __attribute__((aligned(16))) float As[LT_B * LT_LD];
  __shared__ __attribute__((aligned(16))) float Bs[LT_B * LT_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long m0 = (long long)blockIdx.x * LT_B;
  const int n0 = blockIdx.y * LT_B;
  // loader: thread -> (row, 4 k) of both tiles, two row halves
  const int lrow = tid >> 3, lk = (tid & 7) * 4;
  const bool live0 = m0 + lrow < M, live1 = m0 + lrow + 32 < M;
  const float* xa0 = X + (live0 ? m0 + lrow : 0) * K + lk;
  const float* xa1 = X + (live1 ? m0 + lrow + 32 : 0) * K + lk;
  const float* wb0 = Wt + (long long)(n0 + lrow) * K + lk;   // N % 64 == 0: always inside W
  const float* wb1 = wb0 + 32LL * K;
  float4 ra0 = make_float4(0.f, 0.f, 0.f, 0.f), ra1 = ra0;   // rows >= M stay zero: they are never loaded
  if (live0) ra0 = *reinterpret_cast<const float4*>(xa0);
  if (live1) ra1 = *reinterpret_cast<const float4*>(xa1);
  float4 rb0 = *reinterpret_cast<const float4*>(wb0);
  float4 rb1 = *reinterpret_cast<const float4*>(wb1);
  const int wm = wave & 1, wn = wave >> 1, r = lane & 31, h = lane >> 5;
  const float* af = As + (wm * 32 + r) * LT_LD + h * 16;
  const float* bf = Bs + (wn * 32 + r) * LT_LD + h * 16;
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  const int nk = K / LT_K;
  for (int kt = 0; kt < nk; ++kt) {
    *reinterpret_cast<float4*>(As + lrow * LT_LD + lk) = ra0;
    *reinterpret_cast<float4*>(As + (lrow + 32) * LT_LD + lk) = ra1;
    *reinterpret_cast<float4*>(Bs + lrow * LT_LD + lk) = rb0;
    *reinterpret_cast<float4*>(Bs + (lrow + 32) * LT_LD + lk) = rb1;
    __syncthreads();
    if (kt + 1 < nk) {
      const int off = (kt + 1) * LT_K;
      if (live0) ra0 = *reinterpret_cast<const float4*>(xa0 + off);
      if (live1) ra1 = *reinterpret_cast<const float4*>(xa1 + off);
      rb0 = *reinterpret_cast<const float4*>(wb0 + off);
      rb1 = *reinterpret_cast<const float4*>(wb1 + off);
    }
    float a[16], b[16];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float4 ta = *reinterpret_cast<const float4*>(af + 4 * q);
      const float4 tb = *reinterpret_cast<const float4*>(bf + 4 * q);
      a[4 * q] = ta.x; a[4 * q + 1] = ta.y; a[4 * q + 2] = ta.z; a[4 * q + 3] = ta.w;
      b[4 * q] = tb.x; b[4 * q + 1] = tb.y; b[4 * q + 2] = tb.z; b[4 * q + 3] = tb.w;
    }
#pragma unroll
    for (int j = 0; j < 16; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], b[j], acc, 0, 0, 0);
    __syncthreads();
  }
  // C/D map of the 32 x 32 forms: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
  const int col = n0 + wn * 32 + r;
  const float bv = bias ? bias[col] : 0.f;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const long long row = m0 + wm * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
    if (row < M) {
      float v = acc[i] + bv;
      if (EPI == EPI_QUICKGELU) v = v / (1.f + expf(-1.702f * v));   // y sigmoid(1.702 y)
      if (EPI == EPI_RESIDUAL) v += R[row * N + col];                 // R may be Y: read and written by this lane only
      Y[row * N + col] = v;
    }
  }
}

extern "C" int tamtr_linear_f32(const float* X, const float* W, const float* bias, const float* residual, float* Y, int M, int N, int K,
                                int epi, void* stream) {
  if (!X || !W || !Y || M < 1 || N < 1 || K < 1 || epi < EPI_NONE || epi > EPI_RESIDUAL || (epi == EPI_RESIDUAL && !residual))
    return TAMTR_EINVAL;
  if (K % LT_K || N % LT_B || (((uintptr_t)X | (uintptr_t)W) % 16) || N / LT_B > 65535) return TAMTR_EUNSUP;
  const dim3 grid((M + LT_B - 1) / LT_B, N / LT_B);
  hipStream_t s = (hipStream_t)stream;
  if (epi == EPI_NONE) hipLaunchKernelGGL(linear_f32_kernel<EPI_NONE>, grid, dim3(256), 0, s, X, W, bias, residual, Y, M, N, K);
  else if (epi == EPI_QUICKGELU) hipLaunchKernelGGL(linear_f32_kernel<EPI_QUICKGELU>, grid, dim3(256), 0, s, X, W, bias, residual, Y, M, N, K);
  else hipLaunchKernelGGL(linear_f32_kernel<EPI_RESIDUAL>, grid, dim3(256), 0, s, X, W, bias, residual, Y, M, N, K);
  return tamtr_launch_status();
}

// ------------------------------------------------------------------------------------------------ pooled projection
// One workgroup per prompt: the row at the first maximum of ids[n, :] (CLIP's end-of-text token has the highest id), ln_final, the
// [W, E] projection (a lane owns output columns tid, tid + 256, ...; each an ordered sum over W) and the optional L2 normalisation.
#define PP_T 256
#define PP_MAXW 1024
#define PP_MAXE 1024

__device__ __forceinline__ float pp_block_sum(float v, float* red) {
  v = group_sum<WAVE>(v);
  __syncthreads();   // red may still be read from the previous reduction
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(PP_T) void text_pool_project_kernel(const float* __restrict__ x, const int32_t* __restrict__ ids,
                                                                 const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                 const float* __restrict__ proj, float* __restrict__ out, int L, int W, int E,
                                                                 float eps, int norm) {
  __shared__ float xs[PP_MAXW];
  __shared__ float red[4];
  __shared__ int s_row;
  const int n = blockIdx.x, tid = threadIdx.x;
  if (tid < WAVE) {   // first maximum: larger id wins, equal ids keep the smaller position
    int best = INT32_MIN, at = 0x7fffffff;
    for (int l = tid; l < L; l += WAVE) {
      const int v = ids[(long long)n * L + l];
      if (v > best) { best = v; at = l; }
    }
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) {
      const int ob = __shfl_xor(best, o, WAVE), oa = __shfl_xor(at, o, WAVE);
      if (ob > best || (ob == best && oa < at)) { best = ob; at = oa; }
    }
    if (tid == 0) s_row = at;
  }
  __syncthreads();
  const float* row = x + ((long long)n * L + s_row) * W;
  float part = 0.f;
  for (int c = tid; c < W; c += PP_T) { const float v = row[c]; xs[c] = v; part += v; }
  const float mean = pp_block_sum(part, red) / (float)W;
  part = 0.f;
  for (int c = tid; c < W; c += PP_T) { const float d = xs[c] - mean; part += d * d; }
  const float rstd = 1.f / sqrtf(pp_block_sum(part, red) / (float)W + eps);
  for (int c = tid; c < W; c += PP_T) xs[c] = (xs[c] - mean) * rstd * gamma[c] + beta[c];   // each lane rewrites its own entries
  __syncthreads();
  float o[PP_MAXE / PP_T];
  float ss = 0.f;
#pragma unroll
  for (int q = 0; q < PP_MAXE / PP_T; ++q) {
    const int e = tid + q * PP_T;
    float a = 0.f;
    if (e < E)
      for (int c = 0; c < W; ++c) a = fmaf(xs[c], proj[(long long)c * E + e], a);
    o[q] = a;
    ss += a * a;
  }
  float inv = 1.f;
  if (norm) inv = sqrtf(pp_block_sum(ss, red));
#pragma unroll
  for (int q = 0; q < PP_MAXE / PP_T; ++q) {
    const int e = tid + q * PP_T;
    if (e < E) out[(long long)n * E + e] = norm ? o[q] / inv : o[q];
  }
}

extern "C" int tamtr_text_pool_project(const float* x, const int32_t* ids, const float* gamma, const float* beta, const float* proj,
                                       float* out, int n, int L, int W, int E, float eps, int norm, void* stream) {
  if (!x || !ids || !gamma || !beta || !proj || !out || n < 1 || L < 1 || W < 1 || E < 1) return TAMTR_EINVAL;
  if (W > PP_MAXW || E > PP_MAXE) return TAMTR_EUNSUP;
  hipLaunchKernelGGL(text_pool_project_kernel, dim3(n), dim3(PP_T), 0, (hipStream_t)stream, x, ids, gamma, beta, proj, out, L, W, E, eps,
                     norm);
  return tamtr_launch_status();
}
