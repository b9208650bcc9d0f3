// gmc.hip - global motion compensation for BoT-SORT on the device: one 2x3 warp per frame, estimated from the frames of a batch as
// they were uploaded for the network.  It stands where the reference runs OpenCV on the host per frame (trackers/utils/gmc.py:247-302,
// applySparseOptFlow: grey, goodFeaturesToTrack, calcOpticalFlowPyrLK, estimateAffinePartial2D).  OpenCV is not a dependency of this
// project, so the rule below is the project's own, modelled on that method; tests/gmc_np.py states it in numpy, step by step.
//
// Inputs: frames u8 [B, H, W, 3] RGB (H, W multiples of 8, min(H, W) >= 64), counts i32 [B] (the detections of each frame),
// scale f64 [B, 2] = (sx, sy), network pixels -> original pixels.  Outputs: warps f64 [B, 2, 3] in original pixels (warp b maps the
// paired previous frame's coordinates to frame b's) and stats i32 [B, 4] = (keypoints, tracked, inliers, used).
//
// State (the caller's, persistent): the pyramid and the keypoint slots of the last frame that reached the tracker, and hdr[0] = valid.
//
// Pairing.  A frame with counts[b] <= 0 does not reach the tracker: it gets the identity, zero stats, and never becomes "previous".
// A frame with counts[b] > 0 is paired with the nearest earlier frame of the batch whose count is positive, else with the state if it is
// valid, else with nothing (identity: the first frame of a sequence).  After the batch the state holds the last frame with a positive
// count and is valid; it is unchanged if there was none.  All of it is index arithmetic on `counts`, read on the device.
//
// The rule, per frame:
//  1. Grey g = (77 R + 150 G + 29 B + 128) >> 8 (u8).  L = min(4, 1 + floor(log2(min(H, W) / 32))) pyramid levels; level l + 1 is level l
//     under the 5x5 binomial filter ([1 4 6 4 1] x [1 4 6 4 1], reflect-101 border, (sum + 128) >> 8) at the even pixels.  Integers.
//  2. Keypoints on level 0: 3x3 Sobel derivatives gx, gy (int32); a = sum gx^2, b = sum gx gy, c = sum gy^2 over the 3x3 block (int32,
//     below 2^24, exact in fp32); lambda = ((a + c) - sqrtf((a - c)^2 + 4 b^2)) / 2 in fp32 op by op; 0 within 2 px of the border.
//     max = the frame's largest lambda.  A 32 x 32 grid of cells (pixel (y, x) lies in cell (32 y / H, 32 x / W)): a cell keeps its
//     pixel of largest lambda if lambda > 0 and lambda >= 0.01f * max, ties to the lowest pixel index.  The keypoints are 1024 slots,
//     one per cell, -1 = empty.  (Both maxima are reductions - per tile then per frame, and one wavefront per cell - rather than
//     atomics: the result is the same and no buffer has to be zero beforehand.)
//  3. Pyramidal Lucas-Kanade from the paired frame's keypoints to this frame, fp32, one wavefront per slot, window 21 x 21.  At level
//     l = L-1 .. 0 the point is p = p0 / 2^l; the previous patch I and its gradients Ix = (S(x+1, y) - S(x-1, y)) / 2, Iy likewise
//     (S = bilinear sample, reads clamped to the edge) are sampled once; G = sum [Ix^2, Ix Iy; Ix Iy, Iy^2]; ten times:
//     b = sum (I - J(p + d + (g + v))) (Ix, Iy), v += G^-1 b.  Then g = 2 (g + v) (level 0: g + v).  The point is lost if
//     lambda_min(G) / 441 < 1 at any level, if p0 + g leaves [0, W-1] x [0, H-1], or if that is not finite.
//  4. Fit, fp64, on the n surviving pairs in slot order, in network pixels.  n <= 4: identity.  Hypothesis k = 0 .. 511 takes the points
//     i = mix(2k * 0x9E3779B9 + n) % n and j = mix((2k + 1) * 0x9E3779B9 + n) % (n - 1), j += (j >= i), with
//     mix(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16   (uint32),
//     and is the similarity [a -b tx; b a ty] through both: d = p_j - p_i, e = q_j - q_i, a = (dx ex + dy ey) / |d|^2,
//     b = (dx ey - dy ex) / |d|^2, t = q_i - R p_i (|d|^2 = 0: no inliers).  Inliers: |R p + t - q|^2 <= 9.  The winner has the most,
//     ties to the lowest k.  Its inliers are refitted by least squares: centroids, then a = sum(x'u' + y'w') / sum(x'^2 + y'^2),
//     b = sum(x'w' - y'u') / the same, t = q_mean - R p_mean, every sum in index order.  The points within 1 px of that fit, if more
//     than 4, are refitted once more the same way (points on the edge of a moving object pass at 3 px and pull the fit).  No inliers
//     or a zero denominator: identity.  The warp W goes out in original pixels as D W D^-1 with D = diag(sx, sy): [a, -b sx / sy,
//     tx sx; b sy / sx, a, ty sy].  (Fitting a similarity to points already scaled would be wrong by pixels where sx != sy: a
//     rotation in network pixels is not one in original pixels.)
//
// Streams (tamtr_gmc_estimate_streams; trackers/track.py:33-53 keeps one tracker, and with it one estimator, per image of the batch):
// a batch of B = F * S frames is frame-major, frame f * S + s being the f-th frame of stream s, and the state is stacked: pyr [S, P],
// kp [S, 1024], hdr [S, 4].  The rule above holds per stream: frame i is paired with the nearest earlier frame i - k S whose count is
// positive, else with stream i % S's state if it is valid, else with nothing; after the batch stream s's state holds its last frame
// with a positive count, and is unchanged if it had none.  The launches are the same four for the whole batch.  S = 1 is
// tamtr_gmc_estimate.
//
// Four launches on the caller's stream: pyramid + corner response, cells, LK, fit (+ the state copy in spare workgroups).  The object
// is compiled with -ffp-contract=off so that every fp32 / fp64 operation rounds as the numpy statement's does.
#include "common.h"

#define GMC_SLOTS 1024
#define GMC_HYP 512
#define GMC_TILE 64
#define GMC_COPY_BLOCKS 32

struct GmcGeo {
  int H, W, L, ntx, nty;
  int h[4], w[4];
  long long off[4];
  long long P;      // bytes of one pyramid, padded to 16
};

static inline long long gmc_al16(long long v) { return (v + 15) & ~15ll; }

static bool gmc_geo(int H, int W, GmcGeo* g) {
  if (H < 64 || W < 64 || (H & 7) || (W & 7) || H > 8192 || W > 8192) return false;
  const int m = (H < W ? H : W) / 32;
  int L = 1;
  while (L < 4 && (m >> L)) ++L;
  g->H = H; g->W = W; g->L = L;
  g->ntx = (W + GMC_TILE - 1) / GMC_TILE; g->nty = (H + GMC_TILE - 1) / GMC_TILE;
  long long o = 0;
  for (int l = 0; l < 4; ++l) {
    g->h[l] = H >> l; g->w[l] = W >> l; g->off[l] = o;
    if (l < L) o += (long long)g->h[l] * g->w[l];
  }
  g->P = gmc_al16(o);
  return true;
}

// workspace sections: 0 pyr u8 [B, P], 1 lam f32 [B, H, W], 2 tilemax f32 [B, ntx * nty], 3 kp i32 [B, 1024], 4 pts f32 [B, 1024, 4],
// 5 status i32 [B, 1024] (0 empty slot, 1 lost, 2 tracked), 6 fit i32 [B, 1032] (chosen k, 7 spare, inlier mask of the n pairs),
// 7 pair i32 [B] (-2 none, -1 the state, else the frame), 8 = the end
static long long gmc_section(const GmcGeo& g, int B, int which) {
  const long long sz[8] = {B * g.P, 4ll * B * g.H * g.W, 4ll * B * g.ntx * g.nty, 4ll * B * GMC_SLOTS, 16ll * B * GMC_SLOTS,
                           4ll * B * GMC_SLOTS, 4ll * B * (GMC_SLOTS + 8), 4ll * B};
  long long o = 0;
  for (int i = 0; i < which; ++i) o += gmc_al16(sz[i]);
  return o;
}

__device__ __forceinline__ int gmc_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ int gmc_refl(int v, int n) {      // reflect-101, then clamped: memory-safe for any v
  if (v < 0) v = -v;
  if (v >= n) v = 2 * n - 2 - v;
  return gmc_clamp(v, 0, n - 1);
}

// one pyramid level of a tile: dst (side SD, origin (dox, doy) in a level of dw x dh) from src (side SS, origin (sox, soy), sw x sh), both
// in LDS.  A coordinate outside its level holds the value of its reflection.  The tile's own pixels also go to `gout`.
template <int SD, int SS>
__device__ __forceinline__ void gmc_down(const unsigned char* src, int sox, int soy, int sw, int sh, unsigned char* dst, int dox, int doy,
                                         int dw, int dh, unsigned char* gout, int tx0, int ty0, int tside) {
  const int wt[5] = {1, 4, 6, 4, 1};
  for (int idx = threadIdx.x; idx < SD * SD; idx += blockDim.x) {
    const int ly = idx / SD, lx = idx % SD;
    const int x = gmc_refl(dox + lx, dw), y = gmc_refl(doy + ly, dh);
    int acc = 0;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      const int yy = gmc_clamp(gmc_refl(2 * y + j - 2, sh) - soy, 0, SS - 1);
      int row = 0;
#pragma unroll
      for (int i = 0; i < 5; ++i) {
        const int xx = gmc_clamp(gmc_refl(2 * x + i - 2, sw) - sox, 0, SS - 1);
        row += wt[i] * src[yy * SS + xx];
      }
      acc += wt[j] * row;
    }
    const unsigned char v = (unsigned char)((acc + 128) >> 8);
    if (dst) dst[idx] = v;
    const int gx = dox + lx, gy = doy + ly;
    if (gx >= tx0 && gx < tx0 + tside && gy >= ty0 && gy < ty0 + tside && gx < dw && gy < dh) gout[(long long)gy * dw + gx] = v;
  }
}

// launch 1: grey, pyramid and corner response of one 64 x 64 tile of one frame; halos 14 / 6 / 2 / 0 at levels 0 .. 3
__global__ __launch_bounds__(256) void gmc_pyramid_kernel(const unsigned char* __restrict__ frames, GmcGeo G, unsigned char* __restrict__ pyr,
                                                         float* __restrict__ lam, float* __restrict__ tilemax) {
  __shared__ unsigned char s0[92 * 92], s1[44 * 44], s2[20 * 20];
  __shared__ short sgx[66 * 66], sgy[66 * 66];
  __shared__ float smax[4];
  const int tx = blockIdx.x, ty = blockIdx.y, b = blockIdx.z, H = G.H, W = G.W;
  const unsigned char* fr = frames + (long long)b * H * W * 3;
  unsigned char* py = pyr + (long long)b * G.P;
  const int ox = tx * 64 - 14, oy = ty * 64 - 14;
  for (int idx = threadIdx.x; idx < 92 * 92; idx += 256) {
    const int ly = idx / 92, lx = idx % 92;
    const int x = gmc_refl(ox + lx, W), y = gmc_refl(oy + ly, H);
    const unsigned char* p = fr + ((long long)y * W + x) * 3;
    const unsigned char v = (unsigned char)((77 * p[0] + 150 * p[1] + 29 * p[2] + 128) >> 8);
    s0[idx] = v;
    const int gx = ox + lx, gy = oy + ly;
    if (lx >= 14 && lx < 78 && ly >= 14 && ly < 78 && gx < W && gy < H) py[(long long)gy * W + gx] = v;
  }
  __syncthreads();
  if (G.L > 1) gmc_down<44, 92>(s0, ox, oy, W, H, s1, tx * 32 - 6, ty * 32 - 6, G.w[1], G.h[1], py + G.off[1], tx * 32, ty * 32, 32);
  // Sobel derivatives of the 66 x 66 pixels around the tile
  for (int idx = threadIdx.x; idx < 66 * 66; idx += 256) {
    const int ly = idx / 66 + 13, lx = idx % 66 + 13;      // position in s0
    const unsigned char* r0 = s0 + (ly - 1) * 92 + lx; const unsigned char* r1 = r0 + 92; const unsigned char* r2 = r1 + 92;
    sgx[idx] = (short)((r0[1] + 2 * r1[1] + r2[1]) - (r0[-1] + 2 * r1[-1] + r2[-1]));
    sgy[idx] = (short)((r2[-1] + 2 * r2[0] + r2[1]) - (r0[-1] + 2 * r0[0] + r0[1]));
  }
  __syncthreads();
  if (G.L > 2) gmc_down<20, 44>(s1, tx * 32 - 6, ty * 32 - 6, G.w[1], G.h[1], s2, tx * 16 - 2, ty * 16 - 2, G.w[2], G.h[2], py + G.off[2],
                                tx * 16, ty * 16, 16);
  float m = 0.f;
  for (int idx = threadIdx.x; idx < 64 * 64; idx += 256) {
    const int ly = idx >> 6, lx = idx & 63, gx = tx * 64 + lx, gy = ty * 64 + ly;
    if (gx >= W || gy >= H) continue;
    float v = 0.f;
    if (gx >= 2 && gx < W - 2 && gy >= 2 && gy < H - 2) {
      int a = 0, bb = 0, c = 0;
#pragma unroll
      for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          const int dx = sgx[(ly + j) * 66 + lx + i], dy = sgy[(ly + j) * 66 + lx + i];
          a += dx * dx; bb += dx * dy; c += dy * dy;
        }
      const float af = (float)a, bf = (float)bb, cf = (float)c;
      const float tr = af + cf, d = af - cf;
      float t = 4.0f * bf;
      t = t * bf;
      v = (tr - sqrtf(d * d + t)) * 0.5f;
    }
    lam[((long long)b * H + gy) * W + gx] = v;
    m = fmaxf(m, v);
  }
  m = group_max<64>(m);
  if ((threadIdx.x & 63) == 0) smax[threadIdx.x >> 6] = m;
  __syncthreads();
  if (G.L > 3) gmc_down<8, 20>(s2, tx * 16 - 2, ty * 16 - 2, G.w[2], G.h[2], nullptr, tx * 8, ty * 8, G.w[3], G.h[3], py + G.off[3], tx * 8,
                               ty * 8, 8);
  if (threadIdx.x == 0) tilemax[(long long)b * G.ntx * G.nty + ty * G.ntx + tx] = fmaxf(fmaxf(smax[0], smax[1]), fmaxf(smax[2], smax[3]));
}

// launch 2: one wavefront per cell picks the cell's keypoint
__global__ __launch_bounds__(256) void gmc_cells_kernel(const float* __restrict__ lam, const float* __restrict__ tilemax, GmcGeo G,
                                                       int32_t* __restrict__ kp) {
  const int lane = threadIdx.x & 63, cell = blockIdx.x * 4 + (threadIdx.x >> 6), b = blockIdx.y, H = G.H, W = G.W;
  const int nt = G.ntx * G.nty;
  float m = 0.f;
  for (int i = lane; i < nt; i += 64) m = fmaxf(m, tilemax[(long long)b * nt + i]);
  m = group_max<64>(m);
  const float thr = 0.01f * m;
  const int cy = cell >> 5, cx = cell & 31;
  const int y0 = (cy * H + 31) / 32, y1 = ((cy + 1) * H + 31) / 32, x0 = (cx * W + 31) / 32, x1 = ((cx + 1) * W + 31) / 32;
  const int cw = x1 - x0, n = (y1 - y0) * cw;
  const float* lf = lam + (long long)b * H * W;
  unsigned long long best = 0;
  for (int i = lane; i < n; i += 64) {
    const int pix = (y0 + i / cw) * W + x0 + i % cw;
    const float v = lf[pix];
    if (v > 0.f && v >= thr) {
      const unsigned long long key = ((unsigned long long)__float_as_uint(v) << 32) | (0xffffffffu - (unsigned)pix);
      best = key > best ? key : best;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long other = __shfl_xor(best, o, WAVE);
    best = other > best ? other : best;
  }
  if (lane == 0) kp[(long long)b * GMC_SLOTS + cell] = best ? (int32_t)(0xffffffffu - (unsigned)(best & 0xffffffffu)) : -1;
}

// frame b's pair among the frames of its stream (b - S, b - 2 S, ...), else the stream's state (-1) if `valid`, else nothing (-2)
__device__ __forceinline__ int gmc_pair_of(const int32_t* counts, int b, int S, int valid) {
  if (counts[b] <= 0) return -2;
  for (int q = b - S; q >= 0; q -= S)
    if (counts[q] > 0) return q;
  return valid ? -1 : -2;
}

__device__ __forceinline__ float gmc_bil(const unsigned char* P, int w, int h, float x, float y) {
  const float x0 = floorf(x), y0 = floorf(y);
  const float fx = x - x0, fy = y - y0;
  const int ix = gmc_clamp((int)x0, -1, w), iy = gmc_clamp((int)y0, -1, h);
  const int xa = gmc_clamp(ix, 0, w - 1), xb = gmc_clamp(ix + 1, 0, w - 1), ya = gmc_clamp(iy, 0, h - 1), yb = gmc_clamp(iy + 1, 0, h - 1);
  const float a = P[ya * w + xa], b = P[ya * w + xb], c = P[yb * w + xa], d = P[yb * w + xb];
  const float top = a + fx * (b - a), bot = c + fx * (d - c);
  return top + fy * (bot - top);
}

// launch 3: pyramidal LK, one wavefront per keypoint slot of the paired frame
__global__ __launch_bounds__(256) void gmc_lk_kernel(const int32_t* __restrict__ counts, int S, GmcGeo G, const unsigned char* __restrict__ pyr,
                                                    const int32_t* __restrict__ kp, const unsigned char* __restrict__ st_pyr,
                                                    const int32_t* __restrict__ st_kp, const int32_t* __restrict__ st_hdr,
                                                    float* __restrict__ pts, int32_t* __restrict__ status, int32_t* __restrict__ pair) {
  const int lane = threadIdx.x & 63, slot = blockIdx.x * 4 + (threadIdx.x >> 6), b = blockIdx.y;
  const int sid = b % S;      // the frame's stream: its slice of the stacked state
  st_pyr += (long long)sid * G.P;
  st_kp += sid * GMC_SLOTS;
  const int pi = gmc_pair_of(counts, b, S, st_hdr[4 * sid]);
  if (slot == 0 && lane == 0) pair[b] = pi;
  const long long o = (long long)b * GMC_SLOTS + slot;
  const int k = pi == -2 ? -1 : (pi == -1 ? st_kp[slot] : kp[(long long)pi * GMC_SLOTS + slot]);
  if (k < 0 || k >= G.H * G.W) {      // wave-uniform
    if (lane == 0) { status[o] = 0; pts[o * 4] = pts[o * 4 + 1] = pts[o * 4 + 2] = pts[o * 4 + 3] = 0.f; }
    return;
  }
  const unsigned char* prev = pi == -1 ? st_pyr : pyr + (long long)pi * G.P;
  const unsigned char* cur = pyr + (long long)b * G.P;
  const float px0 = (float)(k % G.W), py0 = (float)(k / G.W);
  float gx = 0.f, gy = 0.f;
  bool ok = true;
  for (int l = G.L - 1; l >= 0; --l) {
    const float sc = 1.0f / (float)(1 << l);
    const float px = px0 * sc, py = py0 * sc;
    const unsigned char* P = prev + G.off[l]; const unsigned char* C = cur + G.off[l];
    const int w = G.w[l], h = G.h[l];
    float I[7], Ix[7], Iy[7], gxx = 0.f, gxy = 0.f, gyy = 0.f;
#pragma unroll
    for (int j = 0; j < 7; ++j) {
      const int i = lane + 64 * j;
      I[j] = Ix[j] = Iy[j] = 0.f;
      if (i < 441) {
        const float x = px + (float)(i % 21 - 10), y = py + (float)(i / 21 - 10);
        I[j] = gmc_bil(P, w, h, x, y);
        Ix[j] = (gmc_bil(P, w, h, x + 1.0f, y) - gmc_bil(P, w, h, x - 1.0f, y)) * 0.5f;
        Iy[j] = (gmc_bil(P, w, h, x, y + 1.0f) - gmc_bil(P, w, h, x, y - 1.0f)) * 0.5f;
        gxx += Ix[j] * Ix[j]; gxy += Ix[j] * Iy[j]; gyy += Iy[j] * Iy[j];
      }
    }
    gxx = group_sum<64>(gxx); gxy = group_sum<64>(gxy); gyy = group_sum<64>(gyy);
    const float det = gxx * gyy - gxy * gxy;
    const float tr = gxx + gyy, d = gxx - gyy;
    float t = 4.0f * gxy;
    t = t * gxy;
    const float lmin = (tr - sqrtf(d * d + t)) * 0.5f;
    if (!(lmin / 441.0f >= 1.0f)) ok = false;
    float vx = 0.f, vy = 0.f;
    for (int it = 0; it < 10; ++it) {
      float bx = 0.f, by = 0.f;
#pragma unroll
      for (int j = 0; j < 7; ++j) {
        const int i = lane + 64 * j;
        if (i < 441) {
          const float x = (px + (float)(i % 21 - 10)) + (gx + vx), y = (py + (float)(i / 21 - 10)) + (gy + vy);
          const float df = I[j] - gmc_bil(C, w, h, x, y);
          bx += df * Ix[j]; by += df * Iy[j];
        }
      }
      bx = group_sum<64>(bx); by = group_sum<64>(by);
      vx = vx + (gyy * bx - gxy * by) / det;
      vy = vy + (gxx * by - gxy * bx) / det;
    }
    if (l > 0) { gx = 2.0f * (gx + vx); gy = 2.0f * (gy + vy); }
    else { gx = gx + vx; gy = gy + vy; }
  }
  const float cx = px0 + gx, cy = py0 + gy;
  if (!(cx >= 0.f && cx <= (float)(G.W - 1) && cy >= 0.f && cy <= (float)(G.H - 1))) ok = false;
  if (lane == 0) {
    status[o] = ok ? 2 : 1;
    pts[o * 4] = px0; pts[o * 4 + 1] = py0; pts[o * 4 + 2] = cx; pts[o * 4 + 3] = cy;
  }
}

__device__ __forceinline__ uint32_t gmc_mix(uint32_t x) {
  x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
  return x;
}

struct GmcSim { double a, b, tx, ty; bool ok; };

__device__ __forceinline__ GmcSim gmc_hyp(int k, int n, const double* X, const double* Y, const double* U, const double* V) {
  const int i = (int)(gmc_mix((uint32_t)(2 * k) * 0x9E3779B9u + (uint32_t)n) % (uint32_t)n);
  int j = (int)(gmc_mix((uint32_t)(2 * k + 1) * 0x9E3779B9u + (uint32_t)n) % (uint32_t)(n - 1));
  j += (j >= i);
  const double dx = X[j] - X[i], dy = Y[j] - Y[i], ex = U[j] - U[i], ey = V[j] - V[i];
  const double den = dx * dx + dy * dy;
  GmcSim s;
  s.ok = den > 0.0;
  s.a = (dx * ex + dy * ey) / den;
  s.b = (dx * ey - dy * ex) / den;
  s.tx = U[i] - (s.a * X[i] - s.b * Y[i]);
  s.ty = V[i] - (s.b * X[i] + s.a * Y[i]);
  return s;
}

__device__ __forceinline__ bool gmc_inlier(const GmcSim& s, double x, double y, double u, double v) {
  const double rx = ((s.a * x - s.b * y) + s.tx) - u, ry = ((s.b * x + s.a * y) + s.ty) - v;
  return rx * rx + ry * ry <= 9.0;
}

// launch 4: workgroups 0 .. B-1 fit one frame each; the others, GMC_COPY_BLOCKS per stream, copy the stream's last tracked frame into
// its state
__global__ __launch_bounds__(256) void gmc_fit_kernel(const int32_t* __restrict__ counts, const double* __restrict__ scale, int B, int S, GmcGeo G,
                                                     const unsigned char* __restrict__ pyr, const int32_t* __restrict__ kp,
                                                     const float* __restrict__ pts, const int32_t* __restrict__ status,
                                                     const int32_t* __restrict__ pair, int32_t* __restrict__ fit, unsigned char* st_pyr,
                                                     int32_t* st_kp, int32_t* st_hdr, double* __restrict__ warps, int32_t* __restrict__ stats) {
  __shared__ double X[GMC_SLOTS], Y[GMC_SLOTS], U[GMC_SLOTS], V[GMC_SLOTS];
  __shared__ int scan[256], hcnt[GMC_HYP], tot[2];
  const int t = threadIdx.x;
  if ((int)blockIdx.x >= B) {
    const int sid = (blockIdx.x - B) / GMC_COPY_BLOCKS, cb = (blockIdx.x - B) % GMC_COPY_BLOCKS;
    int last = -1;
    for (int q = sid; q < B; q += S)
      if (counts[q] > 0) last = q;
    if (last < 0) return;
    const int nth = GMC_COPY_BLOCKS * 256, me = cb * 256 + t;
    const uint4* src = reinterpret_cast<const uint4*>(pyr + (long long)last * G.P);
    uint4* dst = reinterpret_cast<uint4*>(st_pyr + (long long)sid * G.P);
    for (long long i = me; i < G.P / 16; i += nth) dst[i] = src[i];
    for (int i = me; i < GMC_SLOTS; i += nth) st_kp[sid * GMC_SLOTS + i] = kp[(long long)last * GMC_SLOTS + i];
    if (me == 0) st_hdr[4 * sid] = 1;
    return;
  }
  const int b = blockIdx.x;
  double* wo = warps + b * 6;
  int32_t* so = stats + b * 4;
  int32_t* fo = fit + (long long)b * (GMC_SLOTS + 8);
  if (pair[b] == -2 || counts[b] <= 0) {      // block-uniform
    if (t == 0) { wo[0] = 1; wo[1] = 0; wo[2] = 0; wo[3] = 0; wo[4] = 1; wo[5] = 0; so[0] = so[1] = so[2] = so[3] = 0; fo[0] = -1; }
    return;
  }
  // the surviving pairs in slot order
  const int32_t* st = status + (long long)b * GMC_SLOTS;
  const float* pp = pts + (long long)b * GMC_SLOTS * 4;
  int mine = 0, mykp = 0;
  for (int i = 0; i < 4; ++i) { mine += st[4 * t + i] == 2; mykp += st[4 * t + i] > 0; }
  scan[t] = mine;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {
    const int v = t >= o ? scan[t - o] : 0;
    __syncthreads();
    scan[t] += v;
    __syncthreads();
  }
  const int n = scan[255];
  int pos = scan[t] - mine;
  const double sx = scale[2 * b], sy = scale[2 * b + 1];
  for (int i = 0; i < 4; ++i)
    if (st[4 * t + i] == 2) {
      const float* q = pp + (4 * t + i) * 4;
      X[pos] = (double)q[0]; Y[pos] = (double)q[1]; U[pos] = (double)q[2]; V[pos] = (double)q[3];
      ++pos;
    }
  __syncthreads();
  scan[t] = mykp;
  __syncthreads();
  if (t == 0) {
    int s = 0;
    for (int i = 0; i < 256; ++i) s += scan[i];
    tot[0] = s;
  }
  __syncthreads();
  const int nkp = tot[0];
  if (n <= 4) {
    if (t == 0) { wo[0] = 1; wo[1] = 0; wo[2] = 0; wo[3] = 0; wo[4] = 1; wo[5] = 0; so[0] = nkp; so[1] = n; so[2] = 0; so[3] = 0; fo[0] = -1; }
    return;
  }
  for (int k = t; k < GMC_HYP; k += 256) {
    const GmcSim s = gmc_hyp(k, n, X, Y, U, V);
    int c = 0;
    if (s.ok)
      for (int i = 0; i < n; ++i) c += gmc_inlier(s, X[i], Y[i], U[i], V[i]);
    hcnt[k] = c;
  }
  __syncthreads();
  if (t == 0) {
    int bk = 0;
    for (int k = 1; k < GMC_HYP; ++k)
      if (hcnt[k] > hcnt[bk]) bk = k;
    fo[0] = bk;
    for (int i = 0; i < n; ++i) fo[8 + i] = 0;
    GmcSim s = gmc_hyp(bk, n, X, Y, U, V);
    s.ok = s.ok && hcnt[bk] > 0;
    double a = 1, bb = 0, tx = 0, ty = 0, thr = 9.0;
    int used = 0, inl = 0;
    for (int round = 0; round < 2 && s.ok; ++round, thr = 1.0) {      // the winner's inliers at 3 px, then the refit's own at 1 px
      int m = 0;
      double mx = 0, my = 0, mu = 0, mv = 0;
      for (int i = 0; i < n; ++i) {
        const double rx = ((s.a * X[i] - s.b * Y[i]) + s.tx) - U[i], ry = ((s.b * X[i] + s.a * Y[i]) + s.ty) - V[i];
        const bool in = rx * rx + ry * ry <= thr;
        fo[8 + i] = in | (round ? fo[8 + i] & 2 : 0);
        if (in) { ++m; mx += X[i]; my += Y[i]; mu += U[i]; mv += V[i]; }
      }
      if (m <= (round ? 4 : 0)) break;
      mx = mx / m; my = my / m; mu = mu / m; mv = mv / m;
      double sxx = 0, sa = 0, sb = 0;
      for (int i = 0; i < n; ++i)
        if (fo[8 + i] & 1) {
          const double x = X[i] - mx, y = Y[i] - my, u = U[i] - mu, v = V[i] - mv;
          sxx += x * x + y * y; sa += x * u + y * v; sb += x * v - y * u;
        }
      if (!(sxx > 0.0)) break;
      s.a = a = sa / sxx; s.b = bb = sb / sxx;
      s.tx = tx = mu - (a * mx - bb * my); s.ty = ty = mv - (bb * mx + a * my);
      used = 1; inl = m;
      for (int i = 0; i < n; ++i) fo[8 + i] = (fo[8 + i] & 1) * 3;      // bit 1: the mask of the fit that stands
    }
    for (int i = 0; i < n; ++i) fo[8 + i] = (fo[8 + i] >> 1) & 1;
    wo[0] = a; wo[1] = (-bb * sx) / sy; wo[2] = tx * sx; wo[3] = (bb * sy) / sx; wo[4] = a; wo[5] = ty * sy;      // D W D^-1
    so[0] = nkp; so[1] = n; so[2] = inl; so[3] = used;
  }
}

// sizes and offsets as int: -1 = H, W or B outside what is built, or a workspace beyond 2^31 - 1 bytes
extern "C" int tamtr_gmc_workspace_offset(int B, int H, int W, int which) {
  GmcGeo g;
  if (B < 1 || B > 65535 || which < 0 || which > 8 || !gmc_geo(H, W, &g)) return -1;
  return gmc_section(g, B, 8) > 0x7fffffffll ? -1 : (int)gmc_section(g, B, which);
}

extern "C" int tamtr_gmc_workspace_bytes(int B, int H, int W) { return tamtr_gmc_workspace_offset(B, H, W, 8); }

extern "C" int tamtr_gmc_state_bytes(int H, int W) {
  GmcGeo g;
  return gmc_geo(H, W, &g) ? (int)g.P : -1;
}

extern "C" int tamtr_gmc_estimate_streams(const uint8_t* frames, const int32_t* counts, const double* scale, int B, int S, int H, int W,
                                          uint8_t* st_pyr, int32_t* st_kp, int32_t* st_hdr, double* warps, int32_t* stats, void* workspace,
                                          int workspace_bytes, int stages, void* stream) {
  if (!frames || !counts || !scale || !st_pyr || !st_kp || !st_hdr || !warps || !stats || !workspace || B < 1 || B > 65535 || S < 1 ||
      B % S != 0)
    return TAMTR_EINVAL;
  GmcGeo g;
  if (!gmc_geo(H, W, &g)) return TAMTR_EINVAL;
  if (gmc_section(g, B, 8) > 0x7fffffffll) return TAMTR_EUNSUP;
  if (workspace_bytes < gmc_section(g, B, 8) || stages < 1 || stages > 15) return TAMTR_EINVAL;
  if ((reinterpret_cast<uintptr_t>(workspace) & 15) || (reinterpret_cast<uintptr_t>(st_pyr) & 15) || (reinterpret_cast<uintptr_t>(warps) & 7) ||
      (reinterpret_cast<uintptr_t>(scale) & 7))
    return TAMTR_EINVAL;
  unsigned char* ws = static_cast<unsigned char*>(workspace);
  unsigned char* pyr = ws + gmc_section(g, B, 0);
  float* lam = reinterpret_cast<float*>(ws + gmc_section(g, B, 1));
  float* tmax = reinterpret_cast<float*>(ws + gmc_section(g, B, 2));
  int32_t* kp = reinterpret_cast<int32_t*>(ws + gmc_section(g, B, 3));
  float* pts = reinterpret_cast<float*>(ws + gmc_section(g, B, 4));
  int32_t* status = reinterpret_cast<int32_t*>(ws + gmc_section(g, B, 5));
  int32_t* fit = reinterpret_cast<int32_t*>(ws + gmc_section(g, B, 6));
  int32_t* pair = reinterpret_cast<int32_t*>(ws + gmc_section(g, B, 7));
  hipStream_t s = (hipStream_t)stream;
  if (stages & 1) hipLaunchKernelGGL(gmc_pyramid_kernel, dim3(g.ntx, g.nty, B), dim3(256), 0, s, frames, g, pyr, lam, tmax);
  if (stages & 2) hipLaunchKernelGGL(gmc_cells_kernel, dim3(GMC_SLOTS / 4, B), dim3(256), 0, s, lam, tmax, g, kp);
  if (stages & 4)
    hipLaunchKernelGGL(gmc_lk_kernel, dim3(GMC_SLOTS / 4, B), dim3(256), 0, s, counts, S, g, pyr, kp, st_pyr, st_kp, st_hdr, pts, status, pair);
  if (stages & 8)
    hipLaunchKernelGGL(gmc_fit_kernel, dim3(B + S * GMC_COPY_BLOCKS), dim3(256), 0, s, counts, scale, B, S, g, pyr, kp, pts, status, pair, fit,
                       st_pyr, st_kp, st_hdr, warps, stats);
  return tamtr_launch_status();
}

extern "C" int tamtr_gmc_estimate(const uint8_t* frames, const int32_t* counts, const double* scale, int B, int H, int W, uint8_t* st_pyr,
                                  int32_t* st_kp, int32_t* st_hdr, double* warps, int32_t* stats, void* workspace,
                                  int workspace_bytes, int stages, void* stream) {
  return tamtr_gmc_estimate_streams(frames, counts, scale, B, 1, H, W, st_pyr, st_kp, st_hdr, warps, stats, workspace, workspace_bytes, stages,
                                    stream);
}
