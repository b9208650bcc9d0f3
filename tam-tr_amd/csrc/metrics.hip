// metrics.hip - the validator's AP per class and IoU threshold and its P / R / PR curves in one launch (tamtr_val_ap_curves).
//
// Replaces the host reduction of a validation run, ap_per_class + compute_ap (ultralytics/utils/metrics.py:999-1029,1073-1127): an argsort
// of every prediction of the run, a Python loop over classes and ten compute_ap calls per class, all after a copy of every row to the
// host.  Here the kernel reads what tamtr_val_postprocess_match left on the device, ordered by ops.val_ap_curves, and leaves a few
// hundred KB of results.  F1, the smoothed arg-max confidence and p / r / f1 / tp / fp follow on the host from the returned curves.
//
// The rule is engine.ap_per_class(stable=True, curves=True) in fp64 (the object is compiled with -ffp-contract=off, no fast-math: every
// operation below rounds once, division is the correctly rounded one).
//   order    rows are sorted by class ascending, then confidence descending, then original order (image order, then row order): the
//            host's np.argsort(-conf, kind='stable') followed by its per-class masks.  The caller sorts; seg_off[c] .. seg_off[c + 1] are
//            the rows of class c.  Dead rows (row index >= counts[b]) are in no segment.
//   n_gt[c]  the number of labels with float(c) == class.  Labels outside [0, nc) are counted nowhere; the host rule would give such
//            a label class a (zero) row of its own, which the dense [0, nc) outputs have no place for.
//   per class c with n = n_gt[c] and segment rows i = 0 .. k - 1 (k = n_pred[c]), per threshold t:
//            tpc[i, t]    inclusive count of correct[., t] over rows 0 .. i
//            recall[i]    tpc / (n + 1e-16)
//            precision[i] tpc / (i + 1)
//            A class with n == 0 or k == 0 keeps all-zero rows in every output.
//   AP       knots (0, 1), (recall[i], precision[i]) ..., (1, 0); envelope = suffix maximum of the knots' precision;
//            y[g] = interp(grid[g], knot recall, envelope) on the 101-point grid; ap = h * (sum_g y[g] - 0.5 * (y[0] + y[100])) with
//            h = grid[1] - grid[0] and the sum taken serially g = 0 .. 100 (the host's y.sum() is pairwise: the two differ by roundings).
//   r_curve  interp(-px, -conf, recall[:, 0], left = 0);  p_curve  interp(-px, -conf, precision[:, 0], left = 1); right = last value.
//   pr_curve interp(px, knot recall of threshold 0, its envelope).
//   interp   numpy's: j = the largest index with xp[j] <= x; `left` below xp[0]; fp[last] at or beyond xp[last]; fp[j] when x == xp[j];
//            otherwise ((fp[j + 1] - fp[j]) / (xp[j + 1] - xp[j])) * (x - xp[j]) + fp[j], as separate operations.  Repeated xp (recall repeats at
//            every false positive, tied confidences repeat) use the LAST of the run, so xp[j + 1] > xp[j] strictly and the slope is finite.
//   grids    px = numpy's linspace(0, 1, 1000) and grid = linspace(0, 1, 101) are operands: i / 999.0 does not have numpy's bits.
//   Assumed: tpc <= n (a label is matched at most once per threshold), so recall <= 1 and the knots ascend.  Otherwise the knot (1, 0)
//   breaks the order and numpy's own search result depends on its path; nothing is read out of bounds here either way.
//
// Design: one workgroup of 256 threads per (class, threshold), no atomics of any kind, so two runs give the same bits.
//   a.  n_gt[c]: a plain count over the M labels, strided over the threads, reduced through LDS - by each of the class's ten workgroups;
//   b.  forward over the segment in tiles of VAL_AP_TILE rows: inclusive scan of correct[:, t] (wave scan + wave totals in LDS) plus
//       the carry of the tiles before -> tpc i32, scratch [10, N];
//   c.  backward over the tiles: suffix maximum of tpc / (i + 1) with the carry of the tiles after -> envelope f64, scratch [10, N]
//       (max is exact, so the order of combination does not matter).  The end knots need no storage: envelope(0) = max(1, .) = 1;
//   d.  the 101 grid points one per thread, binary search over the knots' recall; y to LDS, thread 0 sums in grid order;
//   e.  the threshold-0 workgroup also writes the three 1000-point rows of its class, n_gt and n_pred.
//   No cap on the segment length.  Every workgroup writes all of its outputs, zeros included: the caller need not clear them.
#include "common.h"

#define VAL_AP_TILE 256
#define VAL_AP_T 10        // IoU thresholds
#define VAL_AP_G 101       // AP recall grid
#define VAL_AP_PX 1000     // curve grid

struct ApShared {
  int isum[VAL_AP_TILE / WAVE];
  double dmax[VAL_AP_TILE / WAVE];
  double y[VAL_AP_G];
};

// knots of one (class, threshold): index 0 = (0, 1), 1 .. k = the curve, k + 1 = (1, 0)
struct ApKnots {
  const int32_t* tpc;   // [k]
  const double* env;    // [k]
  int k;
  double den;           // n + 1e-16
  __device__ __forceinline__ double xp(int j) const { return j == 0 ? 0.0 : (j == k + 1 ? 1.0 : (double)tpc[j - 1] / den); }
  __device__ __forceinline__ double fp(int j) const { return j == 0 ? 1.0 : (j == k + 1 ? 0.0 : env[j - 1]); }
};

// numpy's interp over the knots; x is inside [0, 1] = [xp(0), xp(last)]
__device__ double ap_interp_knots(const ApKnots& kn, double x) {
  const int last = kn.k + 1;
  if (x < 0.0) return 1.0;
  if (x >= 1.0) return 0.0;               // at or beyond xp[last]
  int lo = 0, hi = last;                  // xp(lo) <= x < xp(hi)
  while (hi - lo > 1) {
    const int mid = lo + ((hi - lo) >> 1);
    if (kn.xp(mid) <= x) lo = mid; else hi = mid;
  }
  const double x0 = kn.xp(lo), y0 = kn.fp(lo);
  if (x0 == x) return y0;
  const double slope = (kn.fp(lo + 1) - y0) / (kn.xp(lo + 1) - x0);
  return slope * (x - x0) + y0;
}

// interp(-px, -conf, f, left): conf descends over the k rows; f(j) = tpc0[j] / den (recall) or tpc0[j] / (j + 1) (precision)
template <bool RECALL>
__device__ double ap_interp_conf(const float* conf, const int32_t* tpc0, int k, double den, double px, double left) {
  const double x = -px;
  if (x < -(double)conf[0]) return left;
  auto f = [&](int j) { return RECALL ? (double)tpc0[j] / den : (double)tpc0[j] / (double)(j + 1); };
  if (x >= -(double)conf[k - 1]) return f(k - 1);
  int lo = 0, hi = k - 1;                 // -conf[lo] <= x < -conf[hi]
  while (hi - lo > 1) {
    const int mid = lo + ((hi - lo) >> 1);
    if (-(double)conf[mid] <= x) lo = mid; else hi = mid;
  }
  const double x0 = -(double)conf[lo], y0 = f(lo);
  if (x0 == x) return y0;
  const double slope = (f(lo + 1) - y0) / (-(double)conf[lo + 1] - x0);
  return slope * (x - x0) + y0;
}

__global__ __launch_bounds__(VAL_AP_TILE) void val_ap_curves_kernel(const float* __restrict__ conf, const uint8_t* __restrict__ correct,
                                                                    const int32_t* __restrict__ seg_off, int N, int nc,
                                                                    const float* __restrict__ lab_cls, int M, const double* __restrict__ px,
                                                                    const double* __restrict__ grid, int32_t* __restrict__ tpc_all,
                                                                    double* __restrict__ env_all, double* __restrict__ ap,
                                                                    double* __restrict__ p_curve, double* __restrict__ r_curve,
                                                                    double* __restrict__ pr_curve, int32_t* __restrict__ n_gt,
                                                                    int32_t* __restrict__ n_pred) {
  __shared__ ApShared s;
  const int c = blockIdx.x / VAL_AP_T, t = blockIdx.x % VAL_AP_T, tid = threadIdx.x;
  const int lane = tid & (WAVE - 1), wave = tid / WAVE;
  constexpr int NW = VAL_AP_TILE / WAVE;

  // ---- a. labels of this class
  int cnt = 0;
  const float fc = (float)c;
  for (int m = tid; m < M; m += VAL_AP_TILE) cnt += lab_cls[m] == fc ? 1 : 0;
#pragma unroll
  for (int o = WAVE / 2; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, WAVE);
  if (lane == 0) s.isum[wave] = cnt;
  __syncthreads();
  int n = 0;
#pragma unroll
  for (int w = 0; w < NW; ++w) n += s.isum[w];
  __syncthreads();

  int s0 = seg_off[c], s1 = seg_off[c + 1];
  s0 = s0 < 0 ? 0 : (s0 > N ? N : s0);
  s1 = s1 < s0 ? s0 : (s1 > N ? N : s1);
  const int k = s1 - s0;
  const bool valid = n > 0 && k > 0;
  if (t == 0) {
    if (tid == 0) { n_gt[c] = n; n_pred[c] = k; }
    if (!valid)
      for (int g = tid; g < VAL_AP_PX; g += VAL_AP_TILE) {
        const size_t o = (size_t)c * VAL_AP_PX + g;
        p_curve[o] = 0.0; r_curve[o] = 0.0; pr_curve[o] = 0.0;
      }
  }
  if (!valid) {
    if (tid == 0) ap[(size_t)c * VAL_AP_T + t] = 0.0;
    return;
  }

  const float* cf = conf + s0;
  const uint8_t* hit = correct + (size_t)s0 * VAL_AP_T + t;
  int32_t* tpc = tpc_all + (size_t)t * N + s0;
  double* env = env_all + (size_t)t * N + s0;

  // ---- b. forward: inclusive count of hits
  int carry = 0;
  for (int i0 = 0; i0 < k; i0 += VAL_AP_TILE) {
    const int i = i0 + tid;
    int v = i < k ? (hit[(size_t)i * VAL_AP_T] != 0 ? 1 : 0) : 0;
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) {
      const int o = __shfl_up(v, d, WAVE);
      if (lane >= d) v += o;
    }
    if (lane == WAVE - 1) s.isum[wave] = v;
    __syncthreads();
    int before = carry, total = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      const int x = s.isum[w];
      if (w < wave) before += x;
      total += x;
    }
    if (i < k) tpc[i] = v + before;
    carry += total;
    __syncthreads();
  }

  // ---- c. backward: suffix maximum of the precision (the end knot (1, 0) is the starting carry)
  double best = 0.0;
  for (int i0 = ((k - 1) / VAL_AP_TILE) * VAL_AP_TILE; i0 >= 0; i0 -= VAL_AP_TILE) {
    const int i = i0 + tid;
    double v = i < k ? (double)tpc[i] / (double)(i + 1) : 0.0;
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) {
      const double o = __shfl_down(v, d, WAVE);
      if (lane + d < WAVE) v = fmax(v, o);
    }
    if (lane == 0) s.dmax[wave] = v;
    __syncthreads();
    double after = best, total = best;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      const double x = s.dmax[w];
      if (w > wave) after = fmax(after, x);
      total = fmax(total, x);
    }
    if (i < k) env[i] = fmax(v, after);
    best = total;
    __syncthreads();
  }
  __threadfence_block();
  __syncthreads();   // tpc and env of this workgroup are read back below by other threads

  // ---- d. AP on the 101-point grid
  ApKnots kn;
  kn.tpc = tpc; kn.env = env; kn.k = k;
  kn.den = (double)n + 1e-16;
  if (tid < VAL_AP_G) s.y[tid] = ap_interp_knots(kn, grid[tid]);
  __syncthreads();
  if (tid == 0) {
    double sum = 0.0;
    for (int g = 0; g < VAL_AP_G; ++g) sum += s.y[g];
    const double h = grid[1] - grid[0];
    ap[(size_t)c * VAL_AP_T + t] = h * (sum - 0.5 * (s.y[0] + s.y[VAL_AP_G - 1]));
  }

  // ---- e. the curves of the class (threshold 0)
  if (t == 0)
    for (int g = tid; g < VAL_AP_PX; g += VAL_AP_TILE) {
      const size_t o = (size_t)c * VAL_AP_PX + g;
      const double x = px[g];
      r_curve[o] = ap_interp_conf<true>(cf, tpc, k, kn.den, x, 0.0);
      p_curve[o] = ap_interp_conf<false>(cf, tpc, k, kn.den, x, 1.0);
      pr_curve[o] = ap_interp_knots(kn, x);
    }
}

extern "C" int tamtr_val_ap_tile(void) { return VAL_AP_TILE; }

static inline bool ap_misaligned(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) != 0; }

extern "C" int tamtr_val_ap_curves(const float* conf, const uint8_t* correct, const int32_t* seg_off, int N, int nc, const float* lab_cls,
                                   int M, const double* px, const double* grid, int32_t* tpc_scratch, double* env_scratch, double* ap,
                                   double* p_curve, double* r_curve, double* pr_curve, int32_t* n_gt, int32_t* n_pred, void* stream) {
  if (!conf || !correct || !seg_off || !px || !grid || !tpc_scratch || !env_scratch || !ap || !p_curve || !r_curve || !pr_curve || !n_gt ||
      !n_pred || N < 1 || nc < 1 || M < 0)
    return TAMTR_EINVAL;
  if (M > 0 && !lab_cls) return TAMTR_EINVAL;
  if (ap_misaligned(conf, 4) || ap_misaligned(seg_off, 4) || ap_misaligned(lab_cls, 4) || ap_misaligned(tpc_scratch, 4) ||
      ap_misaligned(n_gt, 4) || ap_misaligned(n_pred, 4) || ap_misaligned(px, 8) || ap_misaligned(grid, 8) || ap_misaligned(env_scratch, 8) ||
      ap_misaligned(ap, 8) || ap_misaligned(p_curve, 8) || ap_misaligned(r_curve, 8) || ap_misaligned(pr_curve, 8))
    return TAMTR_EINVAL;
  if (nc > (1 << 20) || N > (1 << 30)) return TAMTR_EUNSUP;
  hipLaunchKernelGGL(val_ap_curves_kernel, dim3((unsigned)nc * VAL_AP_T), dim3(VAL_AP_TILE), 0, (hipStream_t)stream, conf, correct, seg_off, N,
                     nc, lab_cls, M, px, grid, tpc_scratch, env_scratch, ap, p_curve, r_curve, pr_curve, n_gt, n_pred);
  return tamtr_launch_status();
}
