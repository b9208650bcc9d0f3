// mot_rule.h - what the MOT evaluation (mot.hip) and HOTA (hota.hip) share of the rule written out in mot.hip: the fp64 box, IoU and
// ioa that round op by op (both objects are compiled with -ffp-contract=off), the kind of a ground-truth row, and the assignment of a
// frame with its isolated pairs taken out before the solver (mot_lsap.h) runs.
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
