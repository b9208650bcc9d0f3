// dwgrad.hip - dW[N,K] = dY[M,N]^T X[M,K] (+ db[N] = column sums of dY) for the SHORT and MID-SIZE token-wise products: the 1x1
// convolutions of the trunk (M = B*H*W = 6 400 .. 102 400, 64 .. 512 channels) and the decoder-side linears (M = B*Q = 4 672).
// bf16 in, fp32 MFMA accumulate, fp32 partial results per row slice; the caller adds the slices in order (tamtr_slab_sum_rows).
//
// Why not the batched library GEMM that serves the tall shapes (ops.dw_splitk): per slice the output is a handful of tiles, for which
// the library picks 16-row tiles on 16x4x4 workgroups and runs 10-40 MB of operands at under 1 TB/s; and the bias gradient is two more
// launches.  Here one launch covers (output tiles) x (row slices) ~ 512 workgroups, with the slice count chosen per shape.
//
// Both operands are stored with the REDUCTION index m as the row index, and an MFMA fragment wants 8 consecutive m per lane.  So the
// staging pass transposes: a thread loads 8 rows x 16 bytes (8 columns) - whole 128/256-byte row segments per wave instruction -, turns
// the 8 x 8 block in registers (32 two-source byte permutes) and writes 8 x 16 bytes into a [column][64 m] LDS image, 128-byte rows.  From
// there on it is the tile loop of gemm_bf16.hip's linear_bf16_kernel: ds_read_b128 fragments, 2 x 2 v_mfma_f32_32x32x16_bf16 per wave
// and 16-deep step, two LDS stages, the next 64 rows' global loads in flight under the MFMAs, one barrier per stage.
//
// LDS image: chunk c (16 B = 8 m) of row r at r * 128 + ((c ^ ((r ^ (r >> 3)) & 7)) << 4).  Bank arithmetic (banks of 4 bytes; reads see
// 64 banks = 256 B, writes 32 banks = 128 B):
//   * ds_write_b128 is served in groups of 8 consecutive lanes; those hold columns r = 8 c' + j for c' = 0..7 (j and the chunk rg fixed
//     per instruction and per 8 or 16 lanes): (r ^ (r >> 3)) & 7 = j ^ c', so the 8 lanes land on the 8 different 16-byte slots of the
//     128 bytes: conflict-free.  (With the plain (r & 7) key all 8 would hit one slot.)
//   * ds_read_b128 is served in four groups of 16 lanes, {0-3, 12-15, 20-27} and {4-11, 16-19, 28-31} of each half-wave; lane -> row
//     r0 + lane % 32 with r0 a multiple of 32, chunk 2 ks + lane / 32.  A row's parity picks the 128-byte half of the 256 bytes; inside
//     group one the even rows 0, 2, 12, 14, 20, 22, 24, 26 have keys 0, 2, 5, 7, 6, 4, 3, 1 and the odd rows 1, 3, 13, 15, 21, 23, 25, 27 have
//     1, 3, 4, 6, 7, 5, 2, 0; in group two the even rows 4, 6, 8, 10, 16, 18, 28, 30 have 4, 6, 1, 3, 2, 0, 7, 5 and the odd rows 5, 7, 0, 2, 3,
//     1, 6, 4: eight different keys per half, so every group covers 16 different slots: conflict-free.  (The plain (r & 7) key would
//     repeat each key twice in a group: 2-way.)
//
// Stores: plain, one writer per element of `part`; no atomics, no memset, nothing but the one kernel in the launcher.
#include "common.h"

namespace {

constexpr int DW_T = 256;       // threads: 4 waves as 2 (n) x 2 (k)
constexpr int DW_ROWS = 64;     // reduction rows per stage
constexpr int DW_RB = 128;      // bytes per row of the transposed image (64 m)
constexpr int DW_SMAX = 64;     // most slices
constexpr int DW_MIN_ROWS = 256;  // least rows per slice when there is more than one
constexpr int DW_FILL = 512;    // workgroups that fill the chip (2 per CU)

__device__ __forceinline__ uint32_t dswz(int row, int chunk) { return (uint32_t)row * DW_RB + (uint32_t)((chunk ^ ((row ^ (row >> 3)) & 7)) << 4); }

template <int TN, int TK>
__global__ __launch_bounds__(DW_T, 2) void dw_bf16_kernel(const bf16_t* __restrict__ dY, const bf16_t* __restrict__ X, float* __restrict__ part,
                                                           int with_db, long long M, int N, int K, long long rps, int n_tiles, int k_tiles, int S, long long pitch) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];  // [2 stages][dY^T tile: TN rows | X^T tile: TK rows]
  constexpr int ST_BYTES = (TN + TK) * DW_RB;
  constexpr int NI = TN / 64, KI = TK / 64;  // MFMA tiles per wave along n and k
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wn = wave >> 1, wk = wave & 1;
  const int lr = lane & 31, lh = lane >> 5;
  // ---- XCD-aware assignment (consecutive workgroup ids go round the 8 XCDs, each with an L2 of its own): workgroups that read the same
  // rows sit on one XCD, so that HBM and the fabric see a slice's operands once, not once per XCD.  S >= 8: a slice's tiles all on one XCD;
  // fewer slices: a (slice, n-tile) unit's k-tiles on one XCD (they share the dY tile).  Placement changes speed only.
  const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
  int sl, nt, kt;
  if (S >= 8) {
    const int tiles = n_tiles * k_tiles, t = slot % tiles;
    sl = (slot / tiles) * 8 + xcd; nt = t / k_tiles; kt = t % k_tiles;
  } else {
    const int unit = (slot / k_tiles) * 8 + xcd;
    sl = unit / n_tiles; nt = unit % n_tiles; kt = slot % k_tiles;
  }
  if (sl >= S) return;   // (the whole workgroup: padding of the grid to a multiple of 8)
  const int n0 = nt * TN, k0 = kt * TK;
  const long long m_lo = (long long)sl * rps;
  const long long m_hi = m_lo + rps < M ? m_lo + rps : M;
  const int nst = (int)((m_hi - m_lo + DW_ROWS - 1) / DW_ROWS);

  // ---- staging task: threads [0, TN) the dY tile, [TN, TN + TK) the X tile (whole waves either way); a task = 8 rows x 8 columns
  const bool isY = tid < TN, has_task = tid < TN + TK;
  const int u = isY ? tid : tid - TN;
  const int cpr = (isY ? TN : TK) / 8;   // 16-byte chunks per tile row
  const int c = u % cpr, rg = u / cpr;   // column chunk, row group (8 rows) of the stage
  const int ld = isY ? N : K;
  const int col = (isY ? n0 : k0) + 8 * c;
  const bool col_ok = has_task && col < ld;   // (N, K multiples of 8: a chunk is inside or outside as a whole)
  const bf16_t* src = (isY ? dY : X) + (col_ok ? col : 0);
  const long long mrow = m_lo + rg * 8;
  unsigned char* sdst = smem + (isY ? 0 : TN * DW_RB);
  const bool do_db = with_db && kt == 0 && isY;

  uint4 r[8];
  unsigned live = 0;   // bit i: r[i] holds a row of the slice (else: a re-read of the slice's last row, zeroed before use)
  float colacc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) colacc[j] = 0.f;

  // Every load is issued unconditionally at an address inside the operand (rows past the slice's end re-read its last row, chunks past the
  // last column re-read column 0) and the range check zeroes the VALUE before use: a load under a per-element condition makes the compiler
  // branch around each one and wait for it - 8 dependent round trips per stage instead of 8 loads in flight.
  auto g_load = [&](int st) {
    const long long m = mrow + (long long)st * DW_ROWS;
    live = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const bool in = m + i < m_hi;
      r[i] = *reinterpret_cast<const uint4*>(src + (size_t)(in ? m + i : m_hi - 1) * ld);
      live |= (col_ok && in ? 1u : 0u) << i;
    }
  };
  auto s_store = [&](int stage) {
    if (!has_task) return;
#pragma unroll
    for (int i = 0; i < 8; ++i)
      if (!((live >> i) & 1)) r[i] = make_uint4(0, 0, 0, 0);
    if (do_db) {  // rows in order: this thread's share of the column sums
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const uint32_t d[4] = {r[i].x, r[i].y, r[i].z, r[i].w};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          colacc[2 * q] += __uint_as_float(d[q] << 16);
          colacc[2 * q + 1] += __uint_as_float(d[q] & 0xffff0000u);
        }
      }
    }
    unsigned char* base = sdst + stage * ST_BYTES;
#pragma unroll
    for (int q = 0; q < 4; ++q) {  // columns 2q, 2q + 1 of the 8 rows
      uint32_t lo[4], hi[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {  // rows 2e, 2e + 1
        const uint32_t a = q == 0 ? r[2 * e].x : q == 1 ? r[2 * e].y : q == 2 ? r[2 * e].z : r[2 * e].w;
        const uint32_t b = q == 0 ? r[2 * e + 1].x : q == 1 ? r[2 * e + 1].y : q == 2 ? r[2 * e + 1].z : r[2 * e + 1].w;
        lo[e] = (a & 0xffffu) | (b << 16);
        hi[e] = (a >> 16) | (b & 0xffff0000u);
      }
      *reinterpret_cast<uint4*>(base + dswz(8 * c + 2 * q, rg)) = make_uint4(lo[0], lo[1], lo[2], lo[3]);
      *reinterpret_cast<uint4*>(base + dswz(8 * c + 2 * q + 1, rg)) = make_uint4(hi[0], hi[1], hi[2], hi[3]);
    }
  };

  f32x16 acc[NI][KI];
#pragma unroll
  for (int a = 0; a < NI; ++a)
#pragma unroll
    for (int b = 0; b < KI; ++b)
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[a][b][q] = 0.f;

  g_load(0);
  s_store(0);
  __syncthreads();
  for (int st = 0; st < nst; ++st) {
    const int cur = st & 1;
    if (st + 1 < nst) g_load(st + 1);  // in flight under the MFMAs below
    const unsigned char* sy = smem + cur * ST_BYTES;
    const unsigned char* sx = sy + TN * DW_RB;
#pragma unroll
    for (int ks = 0; ks < DW_ROWS / 16; ++ks) {
      const int ch = ks * 2 + lh;
      s16x8 fy[NI], fx[KI];
#pragma unroll
      for (int i = 0; i < NI; ++i) fy[i] = *reinterpret_cast<const s16x8*>(sy + dswz(wn * (TN / 2) + i * 32 + lr, ch));
#pragma unroll
      for (int j = 0; j < KI; ++j) fx[j] = *reinterpret_cast<const s16x8*>(sx + dswz(wk * (TK / 2) + j * 32 + lr, ch));
#pragma unroll
      for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = 0; j < KI; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fy[i], fx[j], acc[i][j], 0, 0, 0);
    }
    if (st + 1 < nst) {
      s_store(cur ^ 1);  // the other stage was last read before the previous barrier
      __syncthreads();
    }
  }

  // ---- D[row][col]: row = n = (q & 3) + 8 (q >> 2) + 4 lh, col = k = lr: per register two 128-byte row segments per wave
  float* out = part + (size_t)sl * pitch;
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int j = 0; j < KI; ++j) {
      const int k = k0 + wk * (TK / 2) + j * 32 + lr;
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int n = n0 + wn * (TN / 2) + i * 32 + (q & 3) + 8 * (q >> 2) + 4 * lh;
        if (n < N && k < K) out[(size_t)n * K + k] = acc[i][j][q];
      }
    }

  // ---- the slice's column sums of dY behind its product (k-tile 0 only): the 8 row groups' shares added in order; zeros without with_db
  if (kt == 0) {
    float* red = reinterpret_cast<float*>(smem);  // [8 row groups][TN]
    __syncthreads();  // all waves done reading the stages
    if (do_db) {
#pragma unroll
      for (int j = 0; j < 8; ++j) red[rg * TN + 8 * c + j] = colacc[j];
    }
    __syncthreads();
    if (tid < TN && n0 + tid < N) {
      float s = 0.f;
      if (with_db) {
#pragma unroll
        for (int g = 0; g < 8; ++g) s += red[g * TN + tid];
      }
      out[(size_t)N * K + n0 + tid] = s;
    }
  }
}

struct DwPlan {
  int tn, tk, n_tiles, k_tiles, S;
  long long rps;
};

long long dw_rows_per_slice(long long M, int S) { return ((M + S - 1) / S + DW_ROWS - 1) / DW_ROWS * DW_ROWS; }

// Tile and slice count of a shape; false: not served.  Tiles of 128 where the extent reaches 128, 64 x 64 where 128-wide tiles times the
// most slices would leave the chip half empty; then as many slices as bring tiles x S to DW_FILL workgroups, at least DW_MIN_ROWS rows
// each, at most DW_SMAX.  S is settled so that S = ceil(M / rows) with rows = ceil(ceil(M / S) / 64) * 64: no empty slice.
bool dw_plan(long long M, int N, int K, DwPlan* p) {
  if (M <= 0 || N <= 0 || K <= 0 || N % 16 || K % 16 || N > 16384 || K > 16384 || M > (1LL << 40)) return false;
  long long smax = M / DW_MIN_ROWS;
  smax = smax < 1 ? 1 : smax > DW_SMAX ? DW_SMAX : smax;
  int tn = N >= 128 ? 128 : 64, tk = K >= 128 ? 128 : 64;
  auto tiles = [&]() { return (long long)((N + tn - 1) / tn) * ((K + tk - 1) / tk); };
  if (tiles() * smax < DW_FILL / 2) tn = tk = 64;
  const long long t = tiles();
  long long S = (DW_FILL + t - 1) / t;
  S = S < 1 ? 1 : S > smax ? smax : S;
  for (;;) {
    const long long rows = dw_rows_per_slice(M, (int)S), s2 = (M + rows - 1) / rows;
    if (s2 == S) break;
    S = s2;
  }
  p->tn = tn; p->tk = tk;
  p->n_tiles = (N + tn - 1) / tn; p->k_tiles = (K + tk - 1) / tk;
  p->S = (int)S;
  p->rps = dw_rows_per_slice(M, (int)S);
  return true;
}

}  // namespace

extern "C" int tamtr_dw_slices(long long M, int N, int K) {
  DwPlan p;
  return dw_plan(M, N, K, &p) ? p.S : 0;
}

extern "C" int tamtr_dw_bf16(const void* dY, const void* X, float* part, int with_db, long long M, int N, int K, void* stream) {
  if (!dY || !X || !part || M <= 0 || N <= 0 || K <= 0) return TAMTR_EINVAL;
  DwPlan p;
  if (!dw_plan(M, N, K, &p)) return TAMTR_EUNSUP;
  if (((uintptr_t)dY | (uintptr_t)X | (uintptr_t)part) % 16) return TAMTR_EUNSUP;  // 16-byte loads at multiples of 16 bytes from the bases
  const long long pitch = (long long)N * K + (N + 3) / 4 * 4;
  const int groups = p.S >= 8 ? (p.S + 7) / 8 * p.n_tiles * p.k_tiles : (p.S * p.n_tiles + 7) / 8 * p.k_tiles;  // per XCD (see the kernel)
  const dim3 grid((unsigned)groups * 8);
  const size_t lds = (size_t)2 * (p.tn + p.tk) * DW_RB;  // <= 64 KB
#define LAUNCH_DW(TN_, TK_)                                                                                                       \
  hipLaunchKernelGGL((dw_bf16_kernel<TN_, TK_>), grid, dim3(DW_T), lds, (hipStream_t)stream, (const bf16_t*)dY, (const bf16_t*)X, \
                     part, with_db, M, N, K, p.rps, p.n_tiles, p.k_tiles, p.S, pitch)
  if (p.tn == 128 && p.tk == 128) LAUNCH_DW(128, 128);
  else if (p.tn == 128) LAUNCH_DW(128, 64);
  else if (p.tk == 128) LAUNCH_DW(64, 128);
  else LAUNCH_DW(64, 64);
#undef LAUNCH_DW
  return tamtr_launch_status();
}
