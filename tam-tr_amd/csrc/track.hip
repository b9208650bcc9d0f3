// track.hip - ByteTrack on the device: BYTETracker.update (ultralytics/trackers/byte_tracker.py:238-351, with
// utils/kalman_filter.py:33-180 and utils/matching.py:20-126) for the B frames of a predictor batch, in order, inside ONE launch
// (tamtr_bytetrack_update).
//
// Replaces the reference's per-frame host loop (trackers/track.py:40-53): copy the frame's boxes to the host, numpy Kalman filters,
// bbox_ioa and lap.lapjv three times.  Here the kernel reads what tamtr_detect_postprocess left on the device (out [B, nq, 6],
// counts [B]) and writes tracks [B, nq, 8] (x1 y1 x2 y2 id score cls idx; zero after the count) and tcounts [B]; the tracker's state
// lives in a slot table on the device, so nothing synchronises.
//
// The table (capacity T, owned by the caller; the numpy twin tests/bytetrack_np.py keeps the same one):
//   mean f64 [T, 8], cov f64 [T, 8, 8]
//   meta i32 [T, 8]   state, is_activated, track_id, frame_id, start_frame, tracklet_len, idx, flags
//   sc   f32 [T, 2]   score, cls
//   hdr  i32 [8]      frame_id, next_id, live slots, overflow count, 0...
// state: 0 free, 1 Tracked, 2 Lost, 3 Removed but still listed: the reference drops a lost track that aged out from its lost list only
// one update later (it filters with the removed list as it stood before the frame's removals, byte_tracker.py:344-346); until then the
// track still takes part in the first association, where a match revives it, and in the duplicate removal.
// flags: 1 = the mean still is the fp32 measurement it was initiated with (numpy then derives the first predict's process noise and
// the first projection's std in fp32, because `0.05 * np.float32` is fp32), 2 = the id is in the reference's removed list (such a
// track, revived and lost again, leaves the lost list at once).  New tracks take the lowest free slots; when there are more of them
// than free slots the excess is counted in hdr[3] and not created - nothing is written past the table.
//
// Arithmetic (the object is compiled with -ffp-contract=off):
//   filter   fp64 as numpy: initiate / predict / project / update.  F = [[I, I], [0, I]], so F P F^T is block additions in numpy's
//            order ((A + C) + (B + D), B + D, C + D, D); the gain is one 4x4 Cholesky solve; P - K (S K^T) as multi_dot orders it.
//   costs    fp32 in the reference's operation order: tlbr cast to fp32 (a detection's is x1 y1 (x2-x1)+x1 (y2-y1)+y1, as an STrack
//            without a mean reports it), bbox_ioa(iou=True) with eps = fp32(1e-7), d = 1 - iou, fused = 1 - (1 - d) * score.
//   scores   compared in fp32 with the fp32 thresholds, `>` and `<` as the reference (a score equal to track_high_thresh is in
//            neither set).
// Assignment: lap.lapjv(cost, extend_cost=True, cost_limit=L) returns the partial matching that minimises sum(c_ij - L).  The same
// optimum comes from lsap.hip's shortest-augmenting-path solver (float64 duals) when every row may also take one shared `unmatched`
// column of cost L with unlimited capacity: a path that reaches that column ends there, its dual stays 0, and the problem is
// n x (m + 1).  Where the optimum is unique the matching is the reference's.
//
// Design: one workgroup of one wavefront per tracker; the frames are a loop with a barrier between the steps.  The grid dimension is
// the stream dimension (tamtr_*_update_streams, which stand where trackers/track.py:33-53 keeps one tracker per image of the batch):
// a batch of B = F * S images is frame-major, image f * S + s being the f-th frame of stream s; workgroup s owns tracker s - its
// slice of the stacked tables mean / cov / meta / sc [/ tfeat] [S, T, ...], hdr [S, 8] and of the workspace - and walks the images
// f * S + s, f = 0 .. F-1.  The workgroups share nothing and never synchronise with each other, so stream s computes what a launch
// with S = 1 on its own images and tables computes, bit for bit; the single-tracker entry points ARE that launch.  A stream without
// a frame at some position keeps its image with counts = 0: it does not reach the tracker.
// Lists (pool, unconfirmed, high / low detections ...) are built in index order with ballots, the cost matrices and lists live in a
// workspace in global memory (L2-resident), the solver's duals and paths in LDS.  One lane runs one track's filter.  The work is tiny
// and latency-bound.
//
// BoT-SORT (tamtr_botsort_update): BOTSORT.update (trackers/bot_sort.py with byte_tracker.py:81-97 and utils/kalman_filter.py:222-368)
// is the same kernel compiled with KF = KF_XYWH; the table, the lists, the costs and the assignment are the ones above.  It differs in:
//   filter   KalmanFilterXYWH: the state is (x, y, w, h, vx, vy, vw, vh), the measurement tlwh_to_xywh in fp32 (x1 + w / 2, y1 + h / 2,
//            w, h), and every std comes from mean[2] and mean[3].  A new track's mean AND covariance are fp32 arrays in numpy (every
//            entry of initiate's std list is an fp32 scalar, so the squares are fp32 too); while the mean still is that measurement
//            (TRK_RAW) predict and project derive their stds and square them in fp32.  The tlbr of a mean is x - w/2, y - h/2,
//            w + x1, h + y1.
//   predict  a pool track that is not Tracked gets mean[6] = mean[7] = 0 first (bot_sort.py:97-110; ByteTrack zeroes mean[7] only).
//   warp     after the pool's predict and before the first association frame b's warp H = warps[b] (f64 [2, 3], row-major, original
//            pixels; a null `warps` is the identity for every frame) goes to every pool track and every unconfirmed track
//            (byte_tracker.py:277-280, multi_gmc): with R = H[:, :2], t = H[:, 2]: mean = kron(I4, R) @ mean, mean[:2] += t,
//            cov = (R8 @ cov) @ R8^T.  R8 is block diagonal, so each entry of a product has two terms that are not a product with
//            zero: two products and one sum, each rounded on its own here (-ffp-contract=off).  numpy's R8.dot(cov) goes through
//            BLAS, which may fuse a product into the sum, so the two can differ in the last bit; the tests hold mean and cov to 1e-6
//            relative, not to the bit.  The result is an fp64 array: a warped track is no longer TRK_RAW, also under the
//            identity warp (the reference run with an image).  A frame without detections does not reach the tracker, and its
//            warp is not applied.
//   costs    get_dists with with_reid off (the reference builds no embeddings) is ByteTrack's fused IoU distance; proximity_thresh
//            and appearance_thresh act on embeddings only and are not read by tamtr_botsort_update.
//
// BoT-SORT with ReID (tamtr_botsort_reid_update): the KF_XYWH kernel once more, with the appearance half of the reference's rule
// (BOTrack.update_features bot_sort.py:55-64, BOTSORT.init_track :166-174, BOTSORT.get_dists :176-190, matching.embedding_distance
// utils/matching.py:84-105; the numpy twin is tests/botsort_reid_np.py).  The reference ships no encoder; here every detection row
// comes with a feature row feat f32 [B, nq, D] (tamtr_reid_rows below gathers and normalises them), and the table gains
// tfeat f32 [T, D], a track's smooth_feat.  It differs from the kernel above in two places:
//   costs    steps 4 and 6 (get_dists): with d the raw fp32 IoU distance and f its fused form, a pair with !(d > proximity_thresh)
//            (fp32 compare, as numpy compares an fp32 array with a python scalar) also gets the embedding distance
//            e = max(0, 1 - uv / (sqrt(uu) * sqrt(vv))) / 2 with uv, uu, vv the fp64 dot products of the track's smooth_feat and the
//            detection's row (scipy's cdist(..., 'cosine') widens fp32 inputs to fp64; a |cosine| above 1 is clipped to 1 first, as
//            scipy does); e > appearance_thresh (fp64) gives 1; the cost is min(f, e) in fp64, which is what np.minimum of an fp32
//            and an fp64 array returns - so this instantiation keeps its cost matrix in fp64.  The other pairs keep f.  The gated
//            pairs of 64 matrix entries are collected with one ballot and the wave takes them one at a time: lane l sums the
//            products of elements l, l + 64, ... in that order, the 64 partial sums go through an xor butterfly (32, 16, ... 1).
//            The second association stays plain IoU distance (byte_tracker.py:298).
//   features after each of the three match loops the wave walks the matched (slot, detection) pairs; update_features in fp32, every
//            operation rounded on its own: x = f / |f|, s = fp32(0.9) * s + fp32(1 - 0.9) * x, s = s / |s|, where |.| is the square
//            root of the sum of squares taken as above (lane partial sums in element order, xor butterfly) in fp32.  A new track's
//            row is a copy of its detection's row (there smooth_feat IS curr_feat).  A lost track keeps its row.
//            A feature row of zero norm is outside the contract (the reference divides by zero there).
#include "common.h"

#define TRK_FREE 0
#define TRK_TRACKED 1
#define TRK_LOST 2
#define TRK_LIMBO 3
#define TRK_RAW 1
#define TRK_EVER_REMOVED 2
enum { KF_XYAH, KF_XYWH };
enum { M_STATE, M_ACT, M_ID, M_FRAME, M_START, M_LEN, M_IDX, M_FLAGS };

// ---------------------------------------------------------------------------------------------------------------- small helpers
// the i in [0, n) with pred(i), in index order -> list; called by the whole wave; returns their number
template <typename F>
__device__ __forceinline__ int trk_compact(int n, int* list, int lane, F pred) {
  int cnt = 0;
  for (int i0 = 0; i0 < n; i0 += WAVE) {
    const int i = i0 + lane;
    const bool p = i < n && pred(i);
    const unsigned long long b = __ballot(p);
    if (p) list[cnt + __popcll(b & ((1ull << lane) - 1ull))] = i;
    cnt += __popcll(b);
  }
  return cnt;
}

// bbox_ioa(a, b, iou=True), utils/metrics.py:17-46, fp32 op by op
__device__ __forceinline__ float trk_iou(const float* a, const float* b) {
  float iw = fminf(a[2], b[2]) - fmaxf(a[0], b[0]);
  float ih = fminf(a[3], b[3]) - fmaxf(a[1], b[1]);
  iw = iw < 0.0f ? 0.0f : iw;
  ih = ih < 0.0f ? 0.0f : ih;
  const float inter = iw * ih;
  float area = (b[2] - b[0]) * (b[3] - b[1]);
  area = (area + (a[2] - a[0]) * (a[3] - a[1])) - inter;
  return inter / (area + (float)1e-7);
}

// STrack.tlbr from the filter mean (byte_tracker.py:151-166), fp64, then the cast to fp32
// (KF_XYWH: BOTrack.tlwh, bot_sort.py:87-94: the width is mean[2] itself)
template <int KF>
__device__ __forceinline__ void trk_tlbr(const double* m, float* o) {
  const double w = KF == KF_XYWH ? m[2] : m[2] * m[3];
  const double x1 = m[0] - w / 2, y1 = m[1] - m[3] / 2;
  o[0] = (float)x1;
  o[1] = (float)y1;
  o[2] = (float)(w + x1);
  o[3] = (float)(m[3] + y1);
}

// convert_coords of a detection (tlbr_to_tlwh, then tlwh_to_xyah or tlwh_to_xywh): fp32 throughout
template <int KF>
__device__ __forceinline__ void trk_xyah(const float* d, float* z) {
  const float w = d[2] - d[0], h = d[3] - d[1];
  z[0] = d[0] + w / 2.0f;
  z[1] = d[1] + h / 2.0f;
  z[2] = KF == KF_XYWH ? w : w / h;
  z[3] = h;
}

// ---------------------------------------------------------------------------------------------------------------- Kalman filter
template <int KF>
__device__ void kf_initiate(double* m, double* P, const float* z) {
  if (KF == KF_XYWH) {   // every std and its square in fp32: 2 * (1 / 20) and 10 * (1 / 160), times an fp32 width or height
    const float pw = (float)0.1 * z[2], ph = (float)0.1 * z[3], vw = (float)0.0625 * z[2], vh = (float)0.0625 * z[3];
    const float dg[8] = {pw * pw, ph * ph, pw * pw, ph * ph, vw * vw, vh * vh, vw * vw, vh * vh};
    for (int i = 0; i < 8; ++i) {
      m[i] = i < 4 ? (double)z[i] : 0.0;
      for (int j = 0; j < 8; ++j) P[i * 8 + j] = i == j ? (double)dg[i] : 0.0;
    }
    return;
  }
  const float sp32 = (float)0.1 * z[3], sv32 = (float)0.0625 * z[3];   // 2 * (1 / 20) and 10 * (1 / 160), times an fp32 height
  const double sp = sp32, sv = sv32;
  const double dg[8] = {sp * sp, sp * sp, 1e-2 * 1e-2, sp * sp, sv * sv, sv * sv, 1e-5 * 1e-5, sv * sv};
  for (int i = 0; i < 8; ++i) {
    m[i] = i < 4 ? (double)z[i] : 0.0;
    for (int j = 0; j < 8; ++j) P[i * 8 + j] = i == j ? dg[i] : 0.0;
  }
}

// KalmanFilterXYWH's squared stds (position of w, of h, velocity of w, of h): fp32 while the mean is the fp32 measurement
__device__ __forceinline__ void kf_stds_xywh(const double* m, bool raw, double* o) {
  if (raw) {
    const float w = (float)m[2], h = (float)m[3];
    const float s[4] = {(float)(1.0 / 20) * w, (float)(1.0 / 20) * h, (float)(1.0 / 160) * w, (float)(1.0 / 160) * h};
    for (int i = 0; i < 4; ++i) o[i] = s[i] * s[i];
  } else {
    const double s[4] = {1.0 / 20 * m[2], 1.0 / 20 * m[3], 1.0 / 160 * m[2], 1.0 / 160 * m[3]};
    for (int i = 0; i < 4; ++i) o[i] = s[i] * s[i];
  }
}

template <int KF>
__device__ void kf_predict(double* m, double* P, bool raw, bool not_tracked) {
  if (not_tracked) {
    if (KF == KF_XYWH) m[6] = 0.0;
    m[7] = 0.0;
  }
  double q[8];
  if (KF == KF_XYWH) {
    double s[4];
    kf_stds_xywh(m, raw, s);
    for (int i = 0; i < 8; ++i) q[i] = s[(i >> 2) * 2 + (i & 1)];
  } else if (raw) {
    const float h = (float)m[3];
    const float sp = (float)(1.0 / 20) * h, sv = (float)(1.0 / 160) * h;
    const float cp = (float)1e-2, cv = (float)1e-5;
    const float qf[8] = {sp * sp, sp * sp, cp * cp, sp * sp, sv * sv, sv * sv, cv * cv, sv * sv};
    for (int i = 0; i < 8; ++i) q[i] = qf[i];
  } else {
    const double sp = 1.0 / 20 * m[3], sv = 1.0 / 160 * m[3];
    const double qd[8] = {sp * sp, sp * sp, 1e-2 * 1e-2, sp * sp, sv * sv, sv * sv, 1e-5 * 1e-5, sv * sv};
    for (int i = 0; i < 8; ++i) q[i] = qd[i];
  }
  for (int i = 0; i < 4; ++i) m[i] = m[i] + m[i + 4];
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) {
      const double A = P[i * 8 + j], Bq = P[i * 8 + j + 4], C = P[(i + 4) * 8 + j], D = P[(i + 4) * 8 + j + 4];
      P[i * 8 + j] = (A + C) + (Bq + D);
      P[i * 8 + j + 4] = Bq + D;
      P[(i + 4) * 8 + j] = C + D;
    }
  for (int i = 0; i < 8; ++i) P[i * 9] += q[i];
}

template <int KF>
__device__ void kf_update(double* mg, double* Pg, const float* z, bool raw) {
  double m[8], P[64];
  for (int i = 0; i < 8; ++i) m[i] = mg[i];
  for (int i = 0; i < 64; ++i) P[i] = Pg[i];
  double dg[4];
  if (KF == KF_XYWH) {
    double s[4];
    kf_stds_xywh(m, raw, s);
    dg[0] = s[0]; dg[1] = s[1]; dg[2] = s[0]; dg[3] = s[1];
  } else {
    const double sp = raw ? (double)((float)(1.0 / 20) * (float)m[3]) : 1.0 / 20 * m[3];
    dg[0] = sp * sp; dg[1] = sp * sp; dg[2] = 1e-1 * 1e-1; dg[3] = sp * sp;
  }
  double S[4][4], L[4][4];
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) { S[i][j] = P[i * 8 + j] + (i == j ? dg[i] : 0.0); L[i][j] = 0.0; }
  for (int j = 0; j < 4; ++j) {
    double s = S[j][j];
    for (int k = 0; k < j; ++k) s -= L[j][k] * L[j][k];
    L[j][j] = sqrt(s);
    for (int i = j + 1; i < 4; ++i) {
      double t = S[i][j];
      for (int k = 0; k < j; ++k) t -= L[i][k] * L[j][k];
      L[i][j] = t / L[j][j];
    }
  }
  double K[8][4];   // K^T = S^-1 (P H^T)^T, column by column
  for (int i = 0; i < 8; ++i) {
    double y[4];
    for (int k = 0; k < 4; ++k) {
      double t = P[i * 8 + k];
      for (int l = 0; l < k; ++l) t -= L[k][l] * y[l];
      y[k] = t / L[k][k];
    }
    for (int k = 3; k >= 0; --k) {
      double t = y[k];
      for (int l = k + 1; l < 4; ++l) t -= L[l][k] * K[i][l];
      K[i][k] = t / L[k][k];
    }
  }
  double inn[4], SKt[4][8];
  for (int k = 0; k < 4; ++k) inn[k] = (double)z[k] - m[k];
  for (int k = 0; k < 4; ++k)
    for (int j = 0; j < 8; ++j) {
      double t = 0.0;
      for (int l = 0; l < 4; ++l) t += S[k][l] * K[j][l];
      SKt[k][j] = t;
    }
  for (int i = 0; i < 8; ++i) {
    double t = 0.0;
    for (int k = 0; k < 4; ++k) t += K[i][k] * inn[k];
    mg[i] = m[i] + t;
    for (int j = 0; j < 8; ++j) {
      double c = 0.0;
      for (int k = 0; k < 4; ++k) c += K[i][k] * SKt[k][j];
      Pg[i * 8 + j] = P[i * 8 + j] - c;
    }
  }
}

// STrack.multi_gmc for one track (byte_tracker.py:81-97), in place: H = a b tx / c d ty
__device__ void kf_warp(double* m, double* P, const double* H) {
  const double a = H[0], b = H[1], tx = H[2], c = H[3], d = H[4], ty = H[5];
  for (int k = 0; k < 8; k += 2) {
    const double x = m[k], y = m[k + 1];
    m[k] = a * x + b * y;
    m[k + 1] = c * x + d * y;
  }
  m[0] += tx;
  m[1] += ty;
  for (int k = 0; k < 8; k += 2)      // R8 @ P: rows in pairs
    for (int j = 0; j < 8; ++j) {
      const double x = P[k * 8 + j], y = P[(k + 1) * 8 + j];
      P[k * 8 + j] = a * x + b * y;
      P[(k + 1) * 8 + j] = c * x + d * y;
    }
  for (int i = 0; i < 8; ++i)         // (R8 @ P) @ R8^T: columns in pairs
    for (int k = 0; k < 8; k += 2) {
      const double x = P[i * 8 + k], y = P[i * 8 + k + 1];
      P[i * 8 + k] = x * a + y * b;
      P[i * 8 + k + 1] = x * c + y * d;
    }
}

// ---------------------------------------------------------------------------------------------------------------- assignment
struct TrkCand {
  double val;
  int it;   // position in `remaining`
  int un;   // 1 = column can end the path (not assigned yet, or the shared `unmatched` column)
};

__device__ __forceinline__ bool trk_cand_wins(const TrkCand& a, const TrkCand& b) {
  if (a.val != b.val) return a.val < b.val;
  if (a.un != b.un) return a.un > b.un;
  return a.un ? a.it > b.it : a.it < b.it;
}

struct TrkLsap {   // LDS, sized for R <= T rows and Cn <= nq + 1 columns
  double *u, *v, *sp;
  int *path, *row4col, *remaining, *col4row;
  unsigned char *SR, *SC;
};

// The partial matching of n rows and m columns that minimises sum(c_ij - L): lsap.hip's solver with the extra column m of cost L that
// any number of rows may take.  cost is [n, m] row-major; x[i] receives the column of row i, or -1.  Called by the whole wave.
template <typename C>
__device__ void trk_assign(const C* cost, int n, int m, double L, const TrkLsap& w, int* x, int lane) {
  const int Cn = m + 1;
  for (int i = lane; i < n; i += WAVE) { w.u[i] = 0.0; w.col4row[i] = -1; }
  for (int j = lane; j < Cn; j += WAVE) { w.v[j] = 0.0; w.row4col[j] = -1; w.path[j] = -1; }
  __syncthreads();
  const double INF = __longlong_as_double(0x7ff0000000000000ll);
  bool failed = false;
  for (int cur = 0; cur < n && !failed; ++cur) {
    for (int i = lane; i < n; i += WAVE) w.SR[i] = 0;
    for (int j = lane; j < Cn; j += WAVE) { w.SC[j] = 0; w.sp[j] = INF; w.remaining[j] = Cn - j - 1; }
    __syncthreads();
    int num_remaining = Cn, i = cur, sink = -1;
    double minVal = 0.0;
    while (sink == -1 && num_remaining > 0) {
      if (lane == 0) w.SR[i] = 1;
      const double ui = w.u[i];
      TrkCand best{INF, 0x7fffffff, 0};
      for (int it = lane; it < num_remaining; it += WAVE) {
        const int j = w.remaining[it];
        const double c = j == m ? L : (double)cost[(size_t)i * m + j];
        const double r = ((minVal + c) - ui) - w.v[j];
        double s = w.sp[j];
        if (r < s) { w.path[j] = i; w.sp[j] = r; s = r; }
        TrkCand cnd{s, it, (j == m || w.row4col[j] == -1) ? 1 : 0};
        if (trk_cand_wins(cnd, best)) best = cnd;
      }
#pragma unroll
      for (int o = WAVE / 2; o > 0; o >>= 1) {
        TrkCand other{__shfl_xor(best.val, o, WAVE), __shfl_xor(best.it, o, WAVE), __shfl_xor(best.un, o, WAVE)};
        if (trk_cand_wins(other, best)) best = other;
      }
      if (!(best.val < INF) || best.it >= num_remaining) { failed = true; break; }   // NaN costs
      minVal = best.val;
      const int j = w.remaining[best.it];
      const int r4c = j == m ? -1 : w.row4col[j];
      if (r4c == -1) sink = j; else i = r4c;
      __syncthreads();   // every lane has read remaining[] before it is edited
      --num_remaining;
      if (lane == 0) { w.SC[j] = 1; w.remaining[best.it] = w.remaining[num_remaining]; }
      __syncthreads();
    }
    if (failed || sink == -1) { failed = true; break; }
    for (int r = lane; r < n; r += WAVE) {
      if (r == cur) w.u[r] += minVal;
      else if (w.SR[r]) w.u[r] += minVal - w.sp[w.col4row[r]];
    }
    for (int j = lane; j < Cn; j += WAVE)
      if (w.SC[j]) w.v[j] -= minVal - w.sp[j];
    __syncthreads();
    if (lane == 0) {
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
  for (int i = lane; i < n; i += WAVE) {
    const int j = w.col4row[i];
    x[i] = (failed || j < 0 || j >= m) ? -1 : j;
  }
  __syncthreads();
}

// ---------------------------------------------------------------------------------------------------------------- the tracker
struct TrkParams {
  const float* out;
  const int32_t* counts;
  int B, nq, T;
  double* mean;
  double* cov;
  int32_t* meta;
  float* sc;
  int32_t* hdr;
  float high, low, newt;
  double match;
  int max_time_lost;
  float* tracks;
  int32_t* tcounts;
  unsigned char* ws;
  const double* warps;   // KF_XYWH only: [B, 2, 3] or null
  int S;                 // streams: B = F * S images, frame-major; workgroup s owns tracker s
  size_t ws_stride;      // bytes from one tracker's workspace to the next
  static constexpr bool reid = false;
  using cost_t = float;
};

struct TrkReidParams : TrkParams {
  const float* feat;   // [B, nq, D], the rows of tamtr_reid_rows
  float* tfeat;        // [T, D], smooth_feat of a slot's track
  int D;
  float prox;
  double app;
  static constexpr bool reid = true;
  using cost_t = double;   // np.minimum(fp32 fused cost, fp64 embedding distance) is fp64
};

static size_t trk_ws_bytes(int T, int nq) { return 4 * ((size_t)T * nq + 4 * (size_t)T + 4 * (size_t)nq + 7 * (size_t)T + 5 * (size_t)nq); }
static size_t trk_reid_ws_bytes(int T, int nq) { return trk_ws_bytes(T, nq) + 4 * (size_t)T * nq; }   // the cost matrix is fp64
static size_t trk_lds_bytes(int T, int nq) {
  const size_t R = T, Cn = (size_t)nq + 1;
  return 8 * (R + 2 * Cn) + 4 * (3 * Cn + R) + R + Cn + 16;
}

// ---------------------------------------------------------------------------------------------------------------- ReID
template <typename V>
__device__ __forceinline__ V trk_wave_sum(V x) {
#pragma unroll
  for (int o = WAVE / 2; o > 0; o >>= 1) x += __shfl_xor(x, o, WAVE);
  return x;
}

// BOTrack.update_features (bot_sort.py:55-64) of a track that has a smooth_feat `sm`, with the detection's row f: fp32, op by op.
// Called by the whole wave; lane l owns elements l, l + 64, ...
__device__ __forceinline__ void trk_feat_update(float* sm, const float* f, int D, int lane) {
  float ss = 0.0f;
  for (int k = lane; k < D; k += WAVE) { const float x = f[k]; ss += x * x; }
  const float n1 = sqrtf(trk_wave_sum(ss));
  float s2 = 0.0f;
  for (int k = lane; k < D; k += WAVE) {
    const float x = f[k] / n1;
    const float y = (float)0.9 * sm[k] + (float)(1 - 0.9) * x;
    sm[k] = y;
    s2 += y * y;
  }
  const float n2 = sqrtf(trk_wave_sum(s2));
  for (int k = lane; k < D; k += WAVE) sm[k] = sm[k] / n2;
}

// the matched pairs (row i of a cost matrix, its column xs[i] >= 0) in row order, one at a time: the slot's feature row is updated
template <typename FS, typename FD>
__device__ __forceinline__ void trk_reid_matched(const TrkReidParams& p, const float* fb, const int* xs, int n, int lane, FS slot_of,
                                                 FD det_of) {
  for (int i0 = 0; i0 < n; i0 += WAVE) {
    const int i = i0 + lane;
    const int j = i < n ? xs[i] : -1;
    const int s = j >= 0 ? slot_of(i) : 0, dj = j >= 0 ? det_of(j) : 0;
    unsigned long long todo = __ballot(j >= 0);
    while (todo) {
      const int l = __ffsll(todo) - 1;
      todo &= todo - 1;
      trk_feat_update(p.tfeat + (size_t)__shfl(s, l, WAVE) * p.D, fb + (size_t)__shfl(dj, l, WAVE) * p.D, p.D, lane);
    }
  }
}

// BOTSORT.get_dists (bot_sort.py:176-190) for n tracks x m detections -> cost [n, m] fp64
template <typename FS, typename FD>
__device__ __forceinline__ void trk_reid_costs(const TrkReidParams& p, double* cost, const float* tb, const float* db, const float* d,
                                               const float* fb, int n, int m, int lane, FS slot_of, FD det_of) {
  const int D = p.D;
  for (int e0 = 0; e0 < n * m; e0 += WAVE) {
    const int e = e0 + lane;
    int s = 0, dj = 0;
    double c = 0.0;
    bool near = false;
    if (e < n * m) {
      const int i = e / m;
      s = slot_of(i);
      dj = det_of(e - i * m);
      const float dist = 1.0f - trk_iou(tb + 4 * s, db + 4 * dj);
      c = 1.0f - (1.0f - dist) * d[(size_t)dj * 6 + 4];
      near = !(dist > p.prox);
    }
    unsigned long long todo = __ballot(near);
    while (todo) {
      const int l = __ffsll(todo) - 1;
      todo &= todo - 1;
      const float* u = p.tfeat + (size_t)__shfl(s, l, WAVE) * D;
      const float* v = fb + (size_t)__shfl(dj, l, WAVE) * D;
      double uv = 0.0, uu = 0.0, vv = 0.0;
      for (int k = lane; k < D; k += WAVE) {
        const double a = u[k], b = v[k];
        uv += a * b;
        uu += a * a;
        vv += b * b;
      }
      uv = trk_wave_sum(uv);
      uu = trk_wave_sum(uu);
      vv = trk_wave_sum(vv);
      double cs = uv / (sqrt(uu) * sqrt(vv));
      if (fabs(cs) > 1.0) cs = copysign(1.0, cs);
      double em = fmax(0.0, 1.0 - cs) / 2.0;
      if (em > p.app) em = 1.0;
      if (lane == l) c = fmin(c, em);
    }
    if (e < n * m) cost[e] = c;
  }
}

// a matched track: STrack.update / re_activate (byte_tracker.py:112-145)
template <int KF>
__device__ __forceinline__ void trk_matched(const TrkParams& p, int s, const float* d, int dj, int fid, bool keep_len) {
  int32_t* mt = p.meta + (size_t)s * 8;
  float z[4];
  trk_xyah<KF>(d + (size_t)dj * 6, z);
  kf_update<KF>(p.mean + (size_t)s * 8, p.cov + (size_t)s * 64, z, mt[M_FLAGS] & TRK_RAW);
  mt[M_FLAGS] &= ~TRK_RAW;
  mt[M_LEN] = keep_len ? mt[M_LEN] + 1 : 0;
  mt[M_STATE] = TRK_TRACKED;
  mt[M_ACT] = 1;
  mt[M_FRAME] = fid;
  mt[M_IDX] = dj;
  p.sc[2 * s] = d[(size_t)dj * 6 + 4];
  p.sc[2 * s + 1] = d[(size_t)dj * 6 + 5];
}

template <int KF, typename P>
__global__ __launch_bounds__(WAVE) void bytetrack_kernel(P p) {
  constexpr bool REID = P::reid;
  using cost_t = typename P::cost_t;
  extern __shared__ __align__(16) unsigned char lds[];
  const int lane = threadIdx.x, T = p.T, nq = p.nq, S = p.S, sid = blockIdx.x;
  // this workgroup's tracker: its slice of the stacked tables and of the workspace
  p.mean += (size_t)sid * T * 8;
  p.cov += (size_t)sid * T * 64;
  p.meta += (size_t)sid * T * 8;
  p.sc += (size_t)sid * T * 2;
  p.hdr += 8 * sid;
  p.ws += (size_t)sid * p.ws_stride;
  if constexpr (REID) p.tfeat += (size_t)sid * T * p.D;
  TrkLsap w;
  {
    const int R = T, Cn = nq + 1;
    w.u = reinterpret_cast<double*>(lds);
    w.v = w.u + R;
    w.sp = w.v + Cn;
    w.path = reinterpret_cast<int*>(w.sp + Cn);
    w.row4col = w.path + Cn;
    w.remaining = w.row4col + Cn;
    w.col4row = w.remaining + Cn;
    w.SR = reinterpret_cast<unsigned char*>(w.col4row + R);
    w.SC = w.SR + R;
  }
  cost_t* cost = reinterpret_cast<cost_t*>(p.ws);               // [T, nq]
  float* tb = reinterpret_cast<float*>(cost + (size_t)T * nq);   // tlbr of a slot's track [T, 4]
  float* db = tb + 4 * (size_t)T;                 // tlbr of a detection [nq, 4]
  int* pool = reinterpret_cast<int*>(db + 4 * (size_t)nq);
  int *unconf = pool + T, *rest = unconf + T, *freel = rest + T, *xs = freel + T, *newly_lost = xs + T, *dup = newly_lost + T;
  int *hi = dup + T, *lo = hi + nq, *left = lo + nq, *newd = left + nq, *used = newd + nq;

  int fid = p.hdr[0], next_id = p.hdr[1], over = p.hdr[3];
  for (int b = sid; b < p.B; b += S) {   // the stream's frames, in order
    const int nd = min(max(p.counts[b], 0), nq);
    const float* d = p.out + (size_t)b * nq * 6;
    float* trow = p.tracks + (size_t)b * nq * 8;
    const float* fb = nullptr;   // ReID: the frame's feature rows [nq, D]
    if constexpr (REID) fb = p.feat + (size_t)b * nq * p.D;
    if (nd == 0) {   // trackers/track.py:46-47: the tracker is not called, nothing ages
      for (int e = lane; e < nq * 8; e += WAVE) trow[e] = 0.0f;
      if (lane == 0) p.tcounts[b] = 0;
      continue;
    }
    ++fid;
    // ---- 1. detections: their tlbr, the high and the low set
    for (int j = lane; j < nd; j += WAVE) {
      const float* r = d + (size_t)j * 6;
      db[4 * j] = r[0];
      db[4 * j + 1] = r[1];
      db[4 * j + 2] = (r[2] - r[0]) + r[0];
      db[4 * j + 3] = (r[3] - r[1]) + r[1];
      used[j] = 0;
    }
    const int nhi = trk_compact(nd, hi, lane, [&](int j) { return d[(size_t)j * 6 + 4] > p.high; });
    const int nlo = trk_compact(nd, lo, lane, [&](int j) { const float s = d[(size_t)j * 6 + 4]; return s > p.low && s < p.high; });
    // ---- 2. unconfirmed tracks and the pool (activated tracked + lost), in slot order
    const int nun = trk_compact(T, unconf, lane, [&](int s) { return p.meta[s * 8 + M_STATE] == TRK_TRACKED && !p.meta[s * 8 + M_ACT]; });
    const int npool = trk_compact(T, pool, lane, [&](int s) {
      const int st = p.meta[s * 8 + M_STATE];
      return (st == TRK_TRACKED && p.meta[s * 8 + M_ACT]) || st == TRK_LOST || st == TRK_LIMBO;
    });
    for (int s = lane; s < T; s += WAVE) { newly_lost[s] = 0; dup[s] = 0; }
    __syncthreads();
    // ---- 3. predict the pool (not the unconfirmed tracks); KF_XYWH: then the frame's warp, to the pool and the unconfirmed tracks
    double H[6] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0};
    if (KF == KF_XYWH && p.warps)
      for (int i = 0; i < 6; ++i) H[i] = p.warps[(size_t)b * 6 + i];
    for (int i = lane; i < npool; i += WAVE) {
      const int s = pool[i];
      int32_t* mt = p.meta + (size_t)s * 8;
      kf_predict<KF>(p.mean + (size_t)s * 8, p.cov + (size_t)s * 64, mt[M_FLAGS] & TRK_RAW, mt[M_STATE] != TRK_TRACKED);
      mt[M_FLAGS] &= ~TRK_RAW;
      if (KF == KF_XYWH) kf_warp(p.mean + (size_t)s * 8, p.cov + (size_t)s * 64, H);
      trk_tlbr<KF>(p.mean + (size_t)s * 8, tb + 4 * s);
    }
    for (int i = lane; i < nun; i += WAVE) {
      const int s = unconf[i];
      if (KF == KF_XYWH) {
        kf_warp(p.mean + (size_t)s * 8, p.cov + (size_t)s * 64, H);
        p.meta[(size_t)s * 8 + M_FLAGS] &= ~TRK_RAW;
      }
      trk_tlbr<KF>(p.mean + (size_t)s * 8, tb + 4 * s);
    }
    __syncthreads();
    // ---- 4. first association: pool x high detections, fused distance, match_thresh
    if (npool > 0 && nhi > 0) {
      if constexpr (REID) {
        trk_reid_costs(p, cost, tb, db, d, fb, npool, nhi, lane, [&](int i) { return pool[i]; }, [&](int j) { return hi[j]; });
      } else {
        for (int e = lane; e < npool * nhi; e += WAVE) {
          const int i = e / nhi, j = e - i * nhi, dj = hi[j];
          const float dist = 1.0f - trk_iou(tb + 4 * pool[i], db + 4 * dj);
          cost[e] = 1.0f - (1.0f - dist) * d[(size_t)dj * 6 + 4];
        }
      }
      __syncthreads();
      trk_assign(cost, npool, nhi, p.match, w, xs, lane);
    } else {
      for (int i = lane; i < npool; i += WAVE) xs[i] = -1;
      __syncthreads();
    }
    for (int i = lane; i < npool; i += WAVE) {
      const int j = xs[i];
      if (j >= 0) {
        const int s = pool[i];
        trk_matched<KF>(p, s, d, hi[j], fid, p.meta[s * 8 + M_STATE] == TRK_TRACKED);
        used[hi[j]] = 1;
      }
    }
    if constexpr (REID) trk_reid_matched(p, fb, xs, npool, lane, [&](int i) { return pool[i]; }, [&](int j) { return hi[j]; });
    __syncthreads();
    // ---- 5. second association: the unmatched pool tracks in state Tracked x low detections, plain IoU distance, 0.5
    const int nrest = trk_compact(npool, rest, lane, [&](int i) { return xs[i] < 0 && p.meta[pool[i] * 8 + M_STATE] == TRK_TRACKED; });
    __syncthreads();
    if (nrest > 0 && nlo > 0) {
      for (int e = lane; e < nrest * nlo; e += WAVE) {
        const int i = e / nlo, j = e - i * nlo;
        cost[e] = 1.0f - trk_iou(tb + 4 * pool[rest[i]], db + 4 * lo[j]);
      }
      __syncthreads();
      trk_assign(cost, nrest, nlo, 0.5, w, xs, lane);
    } else {
      for (int i = lane; i < nrest; i += WAVE) xs[i] = -1;
      __syncthreads();
    }
    for (int i = lane; i < nrest; i += WAVE) {
      const int s = pool[rest[i]], j = xs[i];
      if (j >= 0) {
        trk_matched<KF>(p, s, d, lo[j], fid, true);
      } else if (p.meta[s * 8 + M_FLAGS] & TRK_EVER_REMOVED) {
        p.meta[s * 8 + M_STATE] = TRK_FREE;
      } else {
        p.meta[s * 8 + M_STATE] = TRK_LOST;
        newly_lost[s] = 1;
      }
    }
    if constexpr (REID) trk_reid_matched(p, fb, xs, nrest, lane, [&](int i) { return pool[rest[i]]; }, [&](int j) { return lo[j]; });
    __syncthreads();
    // ---- 6. unconfirmed tracks x the high detections still free, fused distance, 0.7; the unmatched ones are removed
    const int nleft = trk_compact(nhi, left, lane, [&](int k) { return !used[hi[k]]; });
    __syncthreads();
    if (nun > 0 && nleft > 0) {
      if constexpr (REID) {
        trk_reid_costs(p, cost, tb, db, d, fb, nun, nleft, lane, [&](int i) { return unconf[i]; }, [&](int j) { return hi[left[j]]; });
      } else {
        for (int e = lane; e < nun * nleft; e += WAVE) {
          const int i = e / nleft, j = e - i * nleft, dj = hi[left[j]];
          const float dist = 1.0f - trk_iou(tb + 4 * unconf[i], db + 4 * dj);
          cost[e] = 1.0f - (1.0f - dist) * d[(size_t)dj * 6 + 4];
        }
      }
      __syncthreads();
      trk_assign(cost, nun, nleft, 0.7, w, xs, lane);
    } else {
      for (int i = lane; i < nun; i += WAVE) xs[i] = -1;
      __syncthreads();
    }
    for (int i = lane; i < nun; i += WAVE) {
      const int s = unconf[i], j = xs[i];
      if (j >= 0) {
        trk_matched<KF>(p, s, d, hi[left[j]], fid, true);
        used[hi[left[j]]] = 1;
      } else {
        p.meta[s * 8 + M_STATE] = TRK_FREE;
      }
    }
    if constexpr (REID) trk_reid_matched(p, fb, xs, nun, lane, [&](int i) { return unconf[i]; }, [&](int j) { return hi[left[j]]; });
    __syncthreads();
    // ---- 7. new tracks from what is left, score >= new_track_thresh, into the lowest free slots
    const int nnew = trk_compact(nleft, newd, lane, [&](int k) { const int dj = hi[left[k]]; return !used[dj] && !(d[(size_t)dj * 6 + 4] < p.newt); });
    const int nfree = trk_compact(T, freel, lane, [&](int s) { return p.meta[s * 8 + M_STATE] == TRK_FREE; });
    __syncthreads();
    const int ncreate = min(nnew, nfree);
    over += nnew - ncreate;
    for (int k = lane; k < ncreate; k += WAVE) {
      const int s = freel[k], dj = hi[left[newd[k]]];
      float z[4];
      trk_xyah<KF>(d + (size_t)dj * 6, z);
      kf_initiate<KF>(p.mean + (size_t)s * 8, p.cov + (size_t)s * 64, z);
      int32_t* mt = p.meta + (size_t)s * 8;
      mt[M_STATE] = TRK_TRACKED;
      mt[M_ACT] = fid == 1;
      mt[M_ID] = next_id + k;
      mt[M_FRAME] = fid;
      mt[M_START] = fid;
      mt[M_LEN] = 0;
      mt[M_IDX] = dj;
      mt[M_FLAGS] = TRK_RAW;
      p.sc[2 * s] = d[(size_t)dj * 6 + 4];
      p.sc[2 * s + 1] = d[(size_t)dj * 6 + 5];
    }
    next_id += ncreate;
    if constexpr (REID)      // a new track's smooth_feat is its detection's row
      for (int k = 0; k < ncreate; ++k) {
        float* sm = p.tfeat + (size_t)freel[k] * p.D;
        const float* f = fb + (size_t)hi[left[newd[k]]] * p.D;
        for (int c = lane; c < p.D; c += WAVE) sm[c] = f[c];
      }
    __syncthreads();
    // ---- 8. lost tracks age out; one removed a frame ago leaves now
    for (int s = lane; s < T; s += WAVE) {
      int32_t* mt = p.meta + (size_t)s * 8;
      if (mt[M_STATE] == TRK_LIMBO) {
        mt[M_STATE] = TRK_FREE;
      } else if (mt[M_STATE] == TRK_LOST && !newly_lost[s] && fid - mt[M_FRAME] > p.max_time_lost) {
        mt[M_STATE] = TRK_LIMBO;
        mt[M_FLAGS] |= TRK_EVER_REMOVED;
      }
    }
    __syncthreads();
    // ---- 9. duplicates: tracked x lost with distance < 0.15; the younger side goes, the tracked side on equal age
    const int nA = trk_compact(T, pool, lane, [&](int s) { return p.meta[s * 8 + M_STATE] == TRK_TRACKED; });
    const int nB = trk_compact(T, unconf, lane, [&](int s) { const int st = p.meta[s * 8 + M_STATE]; return st == TRK_LOST || st == TRK_LIMBO; });
    for (int s = lane; s < T; s += WAVE)
      if (p.meta[s * 8 + M_STATE] != TRK_FREE) trk_tlbr<KF>(p.mean + (size_t)s * 8, tb + 4 * s);
    __syncthreads();
    for (int e = lane; e < nA * nB; e += WAVE) {
      const int i = e / nB, sa = pool[i], sb = unconf[e - i * nB];
      if (1.0f - trk_iou(tb + 4 * sa, tb + 4 * sb) < (float)0.15) {
        const int tp = p.meta[sa * 8 + M_FRAME] - p.meta[sa * 8 + M_START], tq = p.meta[sb * 8 + M_FRAME] - p.meta[sb * 8 + M_START];
        dup[tp > tq ? sb : sa] = 1;
      }
    }
    __syncthreads();
    for (int s = lane; s < T; s += WAVE)
      if (dup[s]) p.meta[s * 8 + M_STATE] = TRK_FREE;
    __syncthreads();
    // ---- 10. rows: the activated tracks in state Tracked, in slot order; zero after the count
    int cnt = trk_compact(T, rest, lane, [&](int s) { return p.meta[s * 8 + M_STATE] == TRK_TRACKED && p.meta[s * 8 + M_ACT]; });
    cnt = min(cnt, nq);
    __syncthreads();
    for (int k = lane; k < cnt; k += WAVE) {
      const int s = rest[k];
      float* r = trow + (size_t)k * 8;
      r[0] = tb[4 * s]; r[1] = tb[4 * s + 1]; r[2] = tb[4 * s + 2]; r[3] = tb[4 * s + 3];
      r[4] = (float)p.meta[s * 8 + M_ID];
      r[5] = p.sc[2 * s];
      r[6] = p.sc[2 * s + 1];
      r[7] = (float)p.meta[s * 8 + M_IDX];
    }
    for (int e = cnt * 8 + lane; e < nq * 8; e += WAVE) trow[e] = 0.0f;
    if (lane == 0) p.tcounts[b] = cnt;
    __syncthreads();
  }
  int live = 0;
  for (int s0 = 0; s0 < T; s0 += WAVE) live += __popcll(__ballot(s0 + lane < T && p.meta[(s0 + lane) * 8 + M_STATE] != TRK_FREE));
  if (lane == 0) { p.hdr[0] = fid; p.hdr[1] = next_id; p.hdr[2] = live; p.hdr[3] = over; }
}

// the workspace of S trackers: the single-tracker byte count rounded up to 16 (trk_ws_bytes is only a multiple of 4, and the ReID cost
// matrix at the head of a workspace is fp64), S times; as int, 0 = unsupported
static size_t trk_ws_stride(size_t one) { return (one + 15) & ~(size_t)15; }
static int trk_ws_int(size_t n) { return n > 0x7fffffff ? 0 : (int)n; }

extern "C" int tamtr_bytetrack_workspace_bytes(int T, int nq) { return T < 1 || nq < 1 ? 0 : trk_ws_int(trk_ws_bytes(T, nq)); }

extern "C" int tamtr_bytetrack_streams_workspace_bytes(int S, int T, int nq) {
  return S < 1 || T < 1 || nq < 1 ? 0 : trk_ws_int((size_t)S * trk_ws_stride(trk_ws_bytes(T, nq)));
}

#define REID_MAX_D 1024

extern "C" int tamtr_botsort_reid_workspace_bytes(int T, int nq) { return T < 1 || nq < 1 ? 0 : trk_ws_int(trk_reid_ws_bytes(T, nq)); }

extern "C" int tamtr_botsort_reid_streams_workspace_bytes(int S, int T, int nq) {
  return S < 1 || T < 1 || nq < 1 ? 0 : trk_ws_int((size_t)S * trk_ws_stride(trk_reid_ws_bytes(T, nq)));
}

// The one launcher of all three instantiations (REID: feat and tfeat are read, the workspace holds an fp64 cost matrix); S = 1 is the
// single-tracker entry points' call.  S trackers need (S - 1) strides and one tracker's bytes.
template <int KF, bool REID>
static int trk_launch(const float* out, const int32_t* counts, const double* warps, const float* feat, int B, int S, int nq, double* mean,
                      double* cov, int32_t* meta, float* sc, int32_t* hdr, float* tfeat, int D, int T, float track_high_thresh,
                      float track_low_thresh, float new_track_thresh, double match_thresh, int max_time_lost, float proximity_thresh,
                      double appearance_thresh, float* tracks, int32_t* tcounts, void* workspace, int workspace_bytes, void* stream) {
  if (!out || !counts || !mean || !cov || !meta || !sc || !hdr || !tracks || !tcounts || !workspace || B < 1 || nq < 1 || T < 1 || S < 1 ||
      B % S != 0)
    return TAMTR_EINVAL;
  if (REID && (!feat || !tfeat || D < 1)) return TAMTR_EINVAL;
  if (warps && (reinterpret_cast<uintptr_t>(warps) & 7)) return TAMTR_EINVAL;
  if (REID && (reinterpret_cast<uintptr_t>(workspace) & 7)) return TAMTR_EINVAL;
  const size_t one = REID ? trk_reid_ws_bytes(T, nq) : trk_ws_bytes(T, nq), stride = trk_ws_stride(one);
  const size_t need = (size_t)(S - 1) * stride + one;
  if ((REID && D > REID_MAX_D) || need > 0x7fffffff || trk_lds_bytes(T, nq) > 64 * 1024) return TAMTR_EUNSUP;
  if (workspace_bytes < 0 || (size_t)workspace_bytes < need) return TAMTR_EINVAL;
  const TrkParams base{out, counts, B, nq, T, mean, cov, meta, sc, hdr, track_high_thresh, track_low_thresh, new_track_thresh, match_thresh,
                       max_time_lost, tracks, tcounts, static_cast<unsigned char*>(workspace), warps, S, stride};
  if constexpr (REID) {
    TrkReidParams p;
    static_cast<TrkParams&>(p) = base;
    p.feat = feat;
    p.tfeat = tfeat;
    p.D = D;
    p.prox = proximity_thresh;
    p.app = appearance_thresh;
    hipLaunchKernelGGL((bytetrack_kernel<KF, TrkReidParams>), dim3(S), dim3(WAVE), trk_lds_bytes(T, nq), (hipStream_t)stream, p);
  } else {
    hipLaunchKernelGGL((bytetrack_kernel<KF, TrkParams>), dim3(S), dim3(WAVE), trk_lds_bytes(T, nq), (hipStream_t)stream, base);
  }
  return tamtr_launch_status();
}

extern "C" int tamtr_bytetrack_update_streams(const float* out, const int32_t* counts, int B, int S, int nq, double* mean, double* cov,
                                              int32_t* meta, float* sc, int32_t* hdr, int T, float track_high_thresh, float track_low_thresh,
                                              float new_track_thresh, double match_thresh, int max_time_lost, float* tracks,
                                              int32_t* tcounts, void* workspace, int workspace_bytes, void* stream) {
  return trk_launch<KF_XYAH, false>(out, counts, nullptr, nullptr, B, S, nq, mean, cov, meta, sc, hdr, nullptr, 0, T, track_high_thresh,
                                    track_low_thresh, new_track_thresh, match_thresh, max_time_lost, 0.0f, 0.0, tracks, tcounts, workspace,
                                    workspace_bytes, stream);
}

extern "C" int tamtr_bytetrack_update(const float* out, const int32_t* counts, int B, int nq, double* mean, double* cov, int32_t* meta,
                                      float* sc, int32_t* hdr, int T, float track_high_thresh, float track_low_thresh,
                                      float new_track_thresh, double match_thresh, int max_time_lost, float* tracks, int32_t* tcounts,
                                      void* workspace, int workspace_bytes, void* stream) {
  return tamtr_bytetrack_update_streams(out, counts, B, 1, nq, mean, cov, meta, sc, hdr, T, track_high_thresh, track_low_thresh,
                                        new_track_thresh, match_thresh, max_time_lost, tracks, tcounts, workspace, workspace_bytes, stream);
}

extern "C" int tamtr_botsort_update_streams(const float* out, const int32_t* counts, const double* warps, int B, int S, int nq, double* mean,
                                            double* cov, int32_t* meta, float* sc, int32_t* hdr, int T, float track_high_thresh,
                                            float track_low_thresh, float new_track_thresh, double match_thresh, int max_time_lost,
                                            float* tracks, int32_t* tcounts, void* workspace, int workspace_bytes, void* stream) {
  return trk_launch<KF_XYWH, false>(out, counts, warps, nullptr, B, S, nq, mean, cov, meta, sc, hdr, nullptr, 0, T, track_high_thresh,
                                    track_low_thresh, new_track_thresh, match_thresh, max_time_lost, 0.0f, 0.0, tracks, tcounts, workspace,
                                    workspace_bytes, stream);
}

extern "C" int tamtr_botsort_update(const float* out, const int32_t* counts, const double* warps, int B, int nq, double* mean, double* cov,
                                    int32_t* meta, float* sc, int32_t* hdr, int T, float track_high_thresh, float track_low_thresh,
                                    float new_track_thresh, double match_thresh, int max_time_lost, float* tracks, int32_t* tcounts,
                                    void* workspace, int workspace_bytes, void* stream) {
  return tamtr_botsort_update_streams(out, counts, warps, B, 1, nq, mean, cov, meta, sc, hdr, T, track_high_thresh, track_low_thresh,
                                      new_track_thresh, match_thresh, max_time_lost, tracks, tcounts, workspace, workspace_bytes, stream);
}

// ---------------------------------------------------------------------------------------------------------------- BoT-SORT with ReID
extern "C" int tamtr_botsort_reid_update_streams(const float* out, const int32_t* counts, const double* warps, const float* feat, int B,
                                                 int S, int nq, double* mean, double* cov, int32_t* meta, float* sc, int32_t* hdr,
                                                 float* tfeat, int D, int T, float track_high_thresh, float track_low_thresh,
                                                 float new_track_thresh, double match_thresh, int max_time_lost, float proximity_thresh,
                                                 double appearance_thresh, float* tracks, int32_t* tcounts, void* workspace,
                                                 int workspace_bytes, void* stream) {
  return trk_launch<KF_XYWH, true>(out, counts, warps, feat, B, S, nq, mean, cov, meta, sc, hdr, tfeat, D, T, track_high_thresh,
                                   track_low_thresh, new_track_thresh, match_thresh, max_time_lost, proximity_thresh, appearance_thresh,
                                   tracks, tcounts, workspace, workspace_bytes, stream);
}

extern "C" int tamtr_botsort_reid_update(const float* out, const int32_t* counts, const double* warps, const float* feat, int B, int nq,
                                         double* mean, double* cov, int32_t* meta, float* sc, int32_t* hdr, float* tfeat, int D, int T,
                                         float track_high_thresh, float track_low_thresh, float new_track_thresh, double match_thresh,
                                         int max_time_lost, float proximity_thresh, double appearance_thresh, float* tracks,
                                         int32_t* tcounts, void* workspace, int workspace_bytes, void* stream) {
  return tamtr_botsort_reid_update_streams(out, counts, warps, feat, B, 1, nq, mean, cov, meta, sc, hdr, tfeat, D, T, track_high_thresh,
                                           track_low_thresh, new_track_thresh, match_thresh, max_time_lost, proximity_thresh,
                                           appearance_thresh, tracks, tcounts, workspace, workspace_bytes, stream);
}

// reid_rows: feat[b, j, :] = the row embed[b, keep[b, j], :] widened to fp32 and normalised twice, for j < counts[b]; zero after the
// count.  Twice, because the reference's BOTrack(feat) runs update_features on a track without a smooth_feat: feat /= |feat|, then
// smooth_feat = feat - the same array - and smooth_feat /= |smooth_feat| (bot_sort.py:57-64).  One wavefront per row.  |x| is the
// fp32 square root of the fp32 sum of squares taken in this order: lane l adds up the squares of its elements in ascending index
// (VEC: elements 4 (l + 64 c) .. + 3 for c = 0, 1, ...; scalar: elements l + 64 c), then the 64 partial sums go through an xor
// butterfly (32, 16, ... 1).  A keep index outside [0, nqm) gives a zero row; a row of zero norm is outside the contract.
#define REID_WAVES 4

template <typename TE, bool VEC>
__device__ __forceinline__ float reid_sumsq_load(const TE* x, int D, int lane) {
  float ss = 0.0f;
  if (VEC) {
    for (int k = 4 * lane; k < D; k += 4 * WAVE) {
      float v[4];
      Elt<TE>::ld4(x + k, v);
      ss += v[0] * v[0]; ss += v[1] * v[1]; ss += v[2] * v[2]; ss += v[3] * v[3];
    }
  } else {
    for (int k = lane; k < D; k += WAVE) { const float v = Elt<TE>::ld(x + k); ss += v * v; }
  }
  return ss;
}

template <typename TE, bool VEC>
__global__ __launch_bounds__(REID_WAVES* WAVE) void reid_rows_kernel(const TE* __restrict__ embed, const int32_t* __restrict__ keep,
                                                                     const int32_t* __restrict__ counts, int B, int nqm, int nq, int D,
                                                                     float* __restrict__ feat) {
  const int lane = threadIdx.x & (WAVE - 1);
  const long long row = (long long)blockIdx.x * REID_WAVES + (threadIdx.x >> 6);
  if (row >= (long long)B * nq) return;
  const int b = (int)(row / nq), j = (int)(row - (long long)b * nq);
  float* o = feat + (size_t)row * D;
  const int q = j < min(max(counts[b], 0), nq) ? keep[row] : -1;
  if (q < 0 || q >= nqm) {
    for (int k = lane; k < D; k += WAVE) o[k] = 0.0f;
    return;
  }
  const TE* x = embed + ((size_t)b * nqm + q) * D;
  const float n1 = sqrtf(trk_wave_sum(reid_sumsq_load<TE, VEC>(x, D, lane)));
  float s2 = 0.0f;
  if (VEC) {
    for (int k = 4 * lane; k < D; k += 4 * WAVE) {
      float v[4];
      Elt<TE>::ld4(x + k, v);
      for (int i = 0; i < 4; ++i) { v[i] = v[i] / n1; s2 += v[i] * v[i]; }
      *reinterpret_cast<float4*>(o + k) = make_float4(v[0], v[1], v[2], v[3]);
    }
  } else {
    for (int k = lane; k < D; k += WAVE) { const float v = Elt<TE>::ld(x + k) / n1; s2 += v * v; o[k] = v; }
  }
  const float n2 = sqrtf(trk_wave_sum(s2));
  if (VEC) {
    for (int k = 4 * lane; k < D; k += 4 * WAVE) {
      float4 v = *reinterpret_cast<float4*>(o + k);
      v.x = v.x / n2; v.y = v.y / n2; v.z = v.z / n2; v.w = v.w / n2;
      *reinterpret_cast<float4*>(o + k) = v;
    }
  } else {
    for (int k = lane; k < D; k += WAVE) o[k] = o[k] / n2;
  }
}

template <typename TE>
static void reid_rows_launch(const void* embed, const int32_t* keep, const int32_t* counts, int B, int nqm, int nq, int D, float* feat,
                             hipStream_t stream) {
  const long long rows = (long long)B * nq;
  const dim3 grid((unsigned)((rows + REID_WAVES - 1) / REID_WAVES)), block(REID_WAVES * WAVE);
  const bool vec = D % 4 == 0 && !(reinterpret_cast<uintptr_t>(embed) & (4 * sizeof(TE) - 1)) && !(reinterpret_cast<uintptr_t>(feat) & 15);
  if (vec)
    hipLaunchKernelGGL((reid_rows_kernel<TE, true>), grid, block, 0, stream, static_cast<const TE*>(embed), keep, counts, B, nqm, nq, D, feat);
  else
    hipLaunchKernelGGL((reid_rows_kernel<TE, false>), grid, block, 0, stream, static_cast<const TE*>(embed), keep, counts, B, nqm, nq, D, feat);
}

extern "C" int tamtr_reid_rows(const void* embed, int dtype, const int32_t* keep, const int32_t* counts, int B, int nqm, int nq, int D,
                               float* feat, void* stream) {
  if (!embed || !keep || !counts || !feat || B < 1 || nqm < 1 || nq < 1 || D < 1) return TAMTR_EINVAL;
  if (D > REID_MAX_D || (dtype != TAMTR_F32 && dtype != TAMTR_BF16) || (long long)B * nq > 0x7fffffffll / REID_WAVES) return TAMTR_EUNSUP;
  if (dtype == TAMTR_F32) reid_rows_launch<float>(embed, keep, counts, B, nqm, nq, D, feat, (hipStream_t)stream);
  else reid_rows_launch<bf16_t>(embed, keep, counts, B, nqm, nq, D, feat, (hipStream_t)stream);
  return tamtr_launch_status();
}
