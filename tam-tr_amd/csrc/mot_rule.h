// mot_rule.h - what the three tracking evaluators (mot.hip, hota.hip, trackmap.hip) share of the rule written out in mot.hip: the fp64
// box, IoU and ioa that round op by op (the three objects are compiled with -ffp-contract=off), the kind of a ground-truth row, the
// assignment of a frame with its isolated pairs taken out before the solver (mot_lsap.h) runs, the frame filter (steps 1 and 2 of
// the rule, which decide the rows every tracking metric sees) with its workspace, and the slot of a pair in a sparse pair table.
#pragma once
#include "common.h"
#include "mot_lsap.h"

struct MotBox { double x1, y1, x2, y2; };
__device__ __forceinline__ MotBox mot_box(const float* r) { return MotBox{(double)r[0], (double)r[1], (double)r[2], (double)r[3]}; }

// the intersection area, 0 when the boxes do not overlap
__device__ __forceinline__ double mot_inter(const MotBox& a, const MotBox& b) {
  const double iw = fmin(a.x2, b.x2) - fmax(a.x1, b.x1), ih = fmin(a.y2, b.y2) - fmax(a.y1, b.y1);
  if (iw <= 0.0 || ih <= 0.0 || iw != iw || ih != ih) return 0.0;
  return iw * ih;
}

__device__ __forceinline__ double mot_iou(const MotBox& a, const MotBox& b) {
  const double inter = mot_inter(a, b);
  if (!(inter > 0.0)) return 0.0;
  const double uni = ((a.x2 - a.x1) * (a.y2 - a.y1) + (b.x2 - b.x1) * (b.y2 - b.y1)) - inter;
  return uni > 0.0 ? inter / uni : 0.0;
}

__device__ __forceinline__ double mot_ioa(const MotBox& t, const MotBox& region) {
  const double area = (t.x2 - t.x1) * (t.y2 - t.y1);
  return area > 0.0 ? mot_inter(t, region) / area : 0.0;
}

__device__ __forceinline__ int mot_kind(const float* g) { return g[6] == 0.0f ? 0 : g[6] == 1.0f ? 1 : g[6] == 2.0f ? 2 : -1; }

// A frame's assignment is sparse: most rows meet (have a negative cost with) one column only, and that column meets no other row.
// Such a pair is a connected component of its own and belongs to the optimum; a row that meets nothing stays unmatched.  Only the
// rows and columns of larger components go to the solver, as one compacted problem.  S is [n, m]; x[i] receives the column or -1.
struct MotSparse {
  int *rcnt, *rone, *rl, *xr;   // [ng]: columns a row meets, one of them, the solver's rows, its result
  int *ccnt, *cone, *cl;        // [nq]: rows a column meets, one of them, the solver's columns
};

template <int NT>
__device__ void mot_assign_sparse(const double* S, int n, int m, const MotLsap& w, const MotSparse& q, int* x, MotCand* red, int* wsum) {
  const int tid = threadIdx.x;
  for (int i = tid; i < n; i += NT) q.rcnt[i] = 0;
  for (int j = tid; j < m; j += NT) q.ccnt[j] = 0;
  __syncthreads();
  for (int e = tid; e < n * m; e += NT)
    if (S[e] < 0.0) {
      const int i = e / m, j = e - i * m;
      atomicAdd(&q.rcnt[i], 1);
      atomicAdd(&q.ccnt[j], 1);
      q.rone[i] = j;
      q.cone[j] = i;
    }
  __syncthreads();
  for (int i = tid; i < n; i += NT) x[i] = (q.rcnt[i] == 1 && q.ccnt[q.rone[i]] == 1) ? q.rone[i] : -1;
  const int nr = mot_compact<NT>(n, q.rl, wsum, [&](int i) { return q.rcnt[i] >= 1 && !(q.rcnt[i] == 1 && q.ccnt[q.rone[i]] == 1); });
  const int ncl = mot_compact<NT>(m, q.cl, wsum, [&](int j) { return q.ccnt[j] >= 1 && !(q.ccnt[j] == 1 && q.rcnt[q.cone[j]] == 1); });
  __syncthreads();
  if (nr > 0 && ncl > 0) {
    mot_assign<NT>([&](int a, int b) -> double { return S[(size_t)q.rl[a] * m + q.cl[b]]; }, nr, ncl, 0.0, w, q.xr, red);
    for (int a = tid; a < nr; a += NT) x[q.rl[a]] = q.xr[a] >= 0 ? q.cl[q.xr[a]] : -1;
  }
  __syncthreads();
}

// ---- the frame filter: steps 1 and 2 of the rule, stated once for the three update kernels
// The frame-local workspace of an update kernel.  A kernel's own arrays follow at `end`.
struct MotFrame {
  double *iouM, *S;          // [ngl, ntl] the IoU matrix; the cost (- score) matrix of the assignment being solved
  int *reg, *gl, *g3, *xs;   // [ng]: rows of kind 2; kind 0 / 1 rows; positions in gl of step 3's rows; the assignment
  int *tl, *t3, *tdrop;      // [nq]: track rows that survive step 1; positions in tl of step 3's; dropped by step 2
  MotSparse sq;
  unsigned char* end;        // ws + mot_frame_ws_bytes(nq, ng)
};
struct MotFrameSets { int ngl, ntl, n3, m3; };

// 4 * (8 * ng + 6 * nq) is a multiple of 8, so doubles placed at `end` are aligned when the workspace is
static __host__ __device__ inline size_t mot_frame_ws_bytes(size_t nq, size_t ng) { return 16 * ng * nq + 4 * (8 * ng + 6 * nq); }

static __host__ __device__ inline MotFrame mot_frame_carve(unsigned char* ws, size_t nq, size_t ng) {
  MotFrame f;
  f.iouM = reinterpret_cast<double*>(ws);
  f.S = f.iouM + ng * nq;
  f.reg = reinterpret_cast<int*>(f.S + ng * nq);
  f.gl = f.reg + ng; f.g3 = f.gl + ng; f.xs = f.g3 + ng;
  f.tl = f.xs + ng; f.t3 = f.tl + nq; f.tdrop = f.t3 + nq;
  f.sq.rcnt = f.tdrop + nq; f.sq.rone = f.sq.rcnt + ng; f.sq.rl = f.sq.rone + ng; f.sq.xr = f.sq.rl + ng;
  f.sq.ccnt = f.sq.xr + ng; f.sq.cone = f.sq.ccnt + nq; f.sq.cl = f.sq.cone + nq;
  f.end = reinterpret_cast<unsigned char*>(f.sq.cl + nq);
  return f;
}

// One frame, from the row clamp to step 3's sets: G [ng, 7] and Tr [nq, 8] are the frame's rows, graw / traw its counts as given.
// On return gl[0, ngl) lists the kind-0 rows (class in range, id below gcap) and the kind-1 rows, tl[0, ntl) the track rows (class in
// range, id below tcap) that survive step 1, g3[0, n3) the positions in gl of the kind-0 rows and t3[0, m3) the positions in tl of
// the track rows step 2 left (tdrop[j] = 1 for the others).  over[0 .. 2] count what was left out: gt ids beyond gcap, track ids
// beyond tcap, rows beyond ng / nq.  on_region_drop / on_distractor_drop are called with the track row steps 1 / 2 drop.  With
// KEEP_IOU iouM holds the IoU of gl x tl on return; without it iouM is filled only in a frame with a kind-1 row (step 2 is skipped
// in the others: it could drop nothing).  All threads of the workgroup call it; it passes at least one barrier.
template <int NT, bool KEEP_IOU, class OnRegionDrop, class OnDistractorDrop>
__device__ __forceinline__ MotFrameSets mot_frame_filter(const float* G, const float* Tr, int graw, int traw, int ng, int nq, int nc, int gcap,
                                                         int tcap, double thr, int32_t* over, const MotFrame& f, const MotLsap& w, MotCand* red,
                                                         int* wsum, OnRegionDrop on_region_drop, OnDistractorDrop on_distractor_drop) {
  const int tid = threadIdx.x;
  const int ngr = min(max(graw, 0), ng), ntr = min(max(traw, 0), nq);
  if (tid == 0 && (graw > ng || traw > nq)) atomicAdd(&over[2], max(graw - ng, 0) + max(traw - nq, 0));
  // ---- the frame's lists: regions; kind-0 rows (class in range, id inside the table) and kind-1 rows; track rows that survive step 1
  const int nreg = mot_compact<NT>(ngr, f.reg, wsum, [&](int i) { return mot_kind(G + (size_t)i * 7) == 2; });
  const int ngl = mot_compact<NT>(ngr, f.gl, wsum, [&](int i) {
    const float* g = G + (size_t)i * 7;
    const int k = mot_kind(g);
    if (k == 1) return true;
    if (k != 0 || !(g[5] >= 0.0f && g[5] < (float)nc)) return false;
    if (!(g[4] >= 0.0f && g[4] < (float)gcap)) { atomicAdd(&over[0], 1); return false; }
    return true;
  });
  const int ntl = mot_compact<NT>(ntr, f.tl, wsum, [&](int j) {
    const float* t = Tr + (size_t)j * 8;
    if (!(t[6] >= 0.0f && t[6] < (float)nc)) return false;
    if (!(t[4] >= 0.0f && t[4] < (float)tcap)) { atomicAdd(&over[1], 1); return false; }
    const MotBox tb = mot_box(t);
    for (int r = 0; r < nreg; ++r)
      if (mot_ioa(tb, mot_box(G + (size_t)f.reg[r] * 7)) > 0.5) { on_region_drop(t); return false; }
    return true;
  });
  auto iou = [&](int e) {
    const int i = e / ntl, j = e - i * ntl;
    return mot_iou(mot_box(G + (size_t)f.gl[i] * 7), mot_box(Tr + (size_t)f.tl[j] * 8));
  };
  if (KEEP_IOU)
    for (int e = tid; e < ngl * ntl; e += NT) f.iouM[e] = iou(e);
  for (int j = tid; j < ntl; j += NT) f.tdrop[j] = 0;
  __syncthreads();
  // ---- 2. distractors
  const int ndis = mot_compact<NT>(ngl, f.g3, wsum, [&](int i) { return mot_kind(G + (size_t)f.gl[i] * 7) == 1; });
  if (ndis > 0 && ntl > 0) {
    for (int e = tid; e < ngl * ntl; e += NT) {
      const int i = e / ntl, j = e - i * ntl;
      const float* g = G + (size_t)f.gl[i] * 7;
      const double v = KEEP_IOU ? f.iouM[e] : (f.iouM[e] = iou(e));
      f.S[e] = (v >= thr && (g[6] == 1.0f || (int)g[5] == (int)Tr[(size_t)f.tl[j] * 8 + 6])) ? -v : 0.0;
    }
    __syncthreads();
    mot_assign_sparse<NT>(f.S, ngl, ntl, w, f.sq, f.xs, red, wsum);
    for (int k = tid; k < ndis; k += NT) {
      const int i = f.g3[k], j = f.xs[i];
      if (j >= 0 && f.S[(size_t)i * ntl + j] < 0.0) {
        f.tdrop[j] = 1;
        on_distractor_drop(Tr + (size_t)f.tl[j] * 8);
      }
    }
    __syncthreads();
  }
  // ---- step 3's sets
  const int n3 = mot_compact<NT>(ngl, f.g3, wsum, [&](int i) { return mot_kind(G + (size_t)f.gl[i] * 7) == 0; });
  const int m3 = mot_compact<NT>(ntl, f.t3, wsum, [&](int j) { return !f.tdrop[j]; });
  return MotFrameSets{ngl, ntl, n3, m3};
}

#define MOT_MAX_PROBES 256
// the slot of pair (g, t) in an open-addressing table of P keys, claimed if the pair is new; -1 when MOT_MAX_PROBES slots from its
// home are all taken by others
__device__ __forceinline__ int mot_pair_slot(unsigned long long* keys, int P, int g, int t) {
  const unsigned long long key = (((unsigned long long)(unsigned)g << 32) | (unsigned)t) + 1ull;
  unsigned long long h = key * 0x9E3779B97F4A7C15ull;
  h ^= h >> 29;
  int s = (int)(h % (unsigned long long)P);
  const int probes = min(P, MOT_MAX_PROBES);
  for (int q = 0; q < probes; ++q) {
    const unsigned long long old = atomicCAS(&keys[s], 0ull, key);
    if (old == 0ull || old == key) return s;
    s = s + 1 == P ? 0 : s + 1;
  }
  return -1;
}
