// mot_lsap.h - the partial-assignment solver of the MOT evaluation (mot.hip): the shortest-augmenting-path solver with float64 duals
// and one shared `unmatched` column, as trk_assign in track.hip states it, run by a whole workgroup of NT threads instead of
// one wavefront (NT threads, a template argument), with the cost read through a functor (a matrix in the workspace per frame; the pair
// table itself for the identity problem) and its state behind plain pointers (LDS for the per-frame problems, global memory for the
// 1024 x 4096 identity problem, which does not fit the LDS).
//
// mot_assign<NT>(cost, n, m, L, w, x, red): the partial matching of n rows and m columns that minimises sum(c_ij - L) over the matched
// pairs; every row may instead take the extra column m of cost L, which any number of rows may take.  x[i] receives the column of
// row i, or -1.  To MAXIMISE a score s >= 0 pass cost = -s and L = 0: a row then stays unmatched rather than take a negative gain.
// Where the optimum is unique the matching is scipy's linear_sum_assignment(maximize=True) restricted to the pairs with s > 0.
#pragma once
#include "common.h"

struct MotCand {
  double val;
  int it;   // position in `remaining`
  int un;   // 1 = column can end the path (not assigned yet, or the shared `unmatched` column)
};

__device__ __forceinline__ bool mot_cand_wins(const MotCand& a, const MotCand& b) {
  if (a.val != b.val) return a.val < b.val;
  if (a.un != b.un) return a.un > b.un;
  return a.un ? a.it > b.it : a.it < b.it;
}

struct MotLsap {   // sized for R rows and Cn = columns + 1
  double *u, *v, *sp;
  int *path, *row4col, *remaining, *col4row;
  unsigned char *SR, *SC;
};

static __host__ __device__ inline size_t mot_lsap_bytes(size_t R, size_t Cn) {
  return (8 * (R + 2 * Cn) + 4 * (3 * Cn + R) + R + Cn + 15) & ~(size_t)15;
}

__device__ __forceinline__ MotLsap mot_lsap_carve(unsigned char* base, int R, int Cn) {   // base: 8-byte aligned
  MotLsap w;
  w.u = reinterpret_cast<double*>(base);
  w.v = w.u + R;
  w.sp = w.v + Cn;
  w.path = reinterpret_cast<int*>(w.sp + Cn);
  w.row4col = w.path + Cn;
  w.remaining = w.row4col + Cn;
  w.col4row = w.remaining + Cn;
  w.SR = reinterpret_cast<unsigned char*>(w.col4row + R);
  w.SC = w.SR + R;
  return w;
}

// Called by the whole workgroup (NT threads, uniform arguments).  red: NT / WAVE entries of LDS.
template <int NT, typename F>
__device__ void mot_assign(F cost, int n, int m, double L, const MotLsap& w, int* x, MotCand* red) {
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wv = tid / WAVE;
  const int Cn = m + 1;
  for (int i = tid; i < n; i += NT) { w.u[i] = 0.0; w.col4row[i] = -1; }
  for (int j = tid; j < Cn; j += NT) { w.v[j] = 0.0; w.row4col[j] = -1; w.path[j] = -1; }
  __syncthreads();
  const double INF = __longlong_as_double(0x7ff0000000000000ll);
  bool failed = false;
  for (int cur = 0; cur < n && !failed; ++cur) {
    for (int i = tid; i < n; i += NT) w.SR[i] = 0;
    for (int j = tid; j < Cn; j += NT) { w.SC[j] = 0; w.sp[j] = INF; w.remaining[j] = Cn - j - 1; }
    __syncthreads();
    int num_remaining = Cn, i = cur, sink = -1;
    double minVal = 0.0;
    while (sink == -1 && num_remaining > 0) {
      if (tid == 0) w.SR[i] = 1;
      const double ui = w.u[i];
      MotCand best{INF, 0x7fffffff, 0};
      for (int it = tid; it < num_remaining; it += NT) {
        const int j = w.remaining[it];
        const double c = j == m ? L : cost(i, j);
        const double r = ((minVal + c) - ui) - w.v[j];
        double s = w.sp[j];
        if (r < s) { w.path[j] = i; w.sp[j] = r; s = r; }
        MotCand cnd{s, it, (j == m || w.row4col[j] == -1) ? 1 : 0};
        if (mot_cand_wins(cnd, best)) best = cnd;
      }
#pragma unroll
      for (int o = WAVE / 2; o > 0; o >>= 1) {
        MotCand other{__shfl_xor(best.val, o, WAVE), __shfl_xor(best.it, o, WAVE), __shfl_xor(best.un, o, WAVE)};
        if (mot_cand_wins(other, best)) best = other;
      }
      if (lane == 0) red[wv] = best;
      __syncthreads();
      best = red[0];
#pragma unroll
      for (int k = 1; k < (NT / WAVE); ++k)
        if (mot_cand_wins(red[k], best)) best = red[k];
      if (!(best.val < INF) || best.it >= num_remaining) { failed = true; break; }   // NaN costs
      minVal = best.val;
      const int j = w.remaining[best.it];
      const int r4c = j == m ? -1 : w.row4col[j];
      if (r4c == -1) sink = j; else i = r4c;
      __syncthreads();   // every thread has read remaining[] and red[] before they are edited
      --num_remaining;
      if (tid == 0) { w.SC[j] = 1; w.remaining[best.it] = w.remaining[num_remaining]; }
      __syncthreads();
    }
    if (failed || sink == -1) { failed = true; break; }
    for (int r = tid; r < n; r += NT) {
      if (r == cur) w.u[r] += minVal;
      else if (w.SR[r]) w.u[r] += minVal - w.sp[w.col4row[r]];
    }
    for (int j = tid; j < Cn; j += NT)
      if (w.SC[j]) w.v[j] -= minVal - w.sp[j];
    __syncthreads();
    if (tid == 0) {
      int j = sink;
      for (int guard = 0; guard <= n; ++guard) {
        const int r = w.path[j];
        if (j != m) w.row4col[j] = r;
        const int t = w.col4row[r];
        w.col4row[r] = j;
        j = t;
        if (r == cur) break;
      }
    }
    __syncthreads();
  }
  __syncthreads();
  for (int i = tid; i < n; i += NT) {
    const int j = w.col4row[i];
    x[i] = (failed || j < 0 || j >= m) ? -1 : j;
  }
  __syncthreads();
}

// the i in [0, n) with pred(i), in index order -> list; called by the whole workgroup, pred once per i; returns their number.
// wsum: NT / WAVE ints of LDS.
template <int NT, typename F>
__device__ int mot_compact(int n, int* list, int* wsum, F pred) {
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wv = tid / WAVE;
  int cnt = 0;
  for (int i0 = 0; i0 < n; i0 += NT) {
    const int i = i0 + tid;
    const bool p = i < n && pred(i);
    const unsigned long long b = __ballot(p);
    if (lane == 0) wsum[wv] = __popcll(b);
    __syncthreads();
    int off = cnt, tot = 0;
#pragma unroll
    for (int k = 0; k < (NT / WAVE); ++k) {
      const int s = wsum[k];
      if (k < wv) off += s;
      tot += s;
    }
    if (p) list[off + __popcll(b & ((1ull << lane) - 1ull))] = i;
    cnt += tot;
    __syncthreads();
  }
  return cnt;
}
