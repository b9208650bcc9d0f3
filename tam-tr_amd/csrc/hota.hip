// hota.hip - HOTA (higher order tracking accuracy) on the device, next to the MOT evaluation of mot.hip: the counts behind HOTA, DetA,
// AssA, DetRe / DetPr, AssRe / AssPr and LocA at 19 localisation thresholds, per class, of the tracker's rows against ground truth.
// The definitions are TrackEval's HOTA.eval_sequence.  tamtr_hota_update takes the B frames of a predictor batch in ONE launch, on
// the rows tamtr_bytetrack_update left on the device; tamtr_hota_end_sequence is the second pass and the reduction, three launches per
// sequence.  engine.hota_evaluate is the numpy statement of the same rule and this file's checker.
//
// THE RULE
// Inputs: those of the MOT evaluation (mot.hip): per frame, ground-truth rows x1 y1 x2 y2 id cls kind and track rows, fp32.  Steps 1
//   (regions) and 2 (distractors) of the MOT rule run unchanged, with their thresholds (ioa > 0.5; iou >= thr, 0.5 by default).  What
//   survives is the input here: per class c the kind-0 ground-truth rows and the track rows of class c.  An identity is (class, id)
//   on both sides.  Ids are unique within a frame on either side.
// Thresholds: alpha = np.arange(0.05, 0.99, 0.05), 19 fp64 values made on the host and handed over as they are (k / 20 differs
//   from several of them in the last bit); eps = np.finfo(float).eps.
// Similarity: per frame and class, S[i, j] is the fp64 IoU of ground truth i and track j, mot_iou's bits.  Every positive IoU takes
//   part, not only those of at least 0.5.
// Pass 1, over the frames of the sequence, per class:
//   sim_iou[i, j] = S[i, j] / ((rowsum_i + colsum_j) - S[i, j]) where that denominator is > eps, else 0 (the sums over the class's rows);
//   pot[g, t] += sim_iou;  gcount[g] += 1 for each ground truth present;  tcount[c, t] += 1 for each track present.
//   Then gas[g, t] = pot / ((gcount[g] + tcount[t]) - pot).
// Pass 2, per frame and class: ONE assignment maximises the sum of gas[g_i, t_j] * S[i, j].  A matched pair with S >= alpha_a - eps is
//   a TP at threshold a: its S is added to loc_sum[c, a] and mc_a[g, t] += 1.  A pair with S = 0 has score 0 and counts nowhere, so the
//   partial matching over the positive scores is TrackEval's full linear_sum_assignment.  FN[c, a] = gt_dets[c] - TP[c, a],
//   FP[c, a] = trk_dets[c] - TP[c, a]; a frame with one side empty adds to gt_dets / trk_dets only.
// Per sequence, class and threshold: ass_sum = sum over pairs of mc_a * mc_a / max(1, gcount + tcount - mc_a); assre_sum the same with
//   max(1, gcount), asspr_sum with max(1, tcount).  These sums, TP, loc_sum, gt_dets and trk_dets are what an evaluator keeps; they add
//   over sequences and classes.  engine.hota_summary: DetA = TP / max(1, TP + FN + FP), DetRe = TP / max(1, TP + FN),
//   DetPr = TP / max(1, TP + FP), AssA = ass_sum / max(1, TP) (AssRe, AssPr likewise), LocA = max(1e-10, loc_sum) / max(1e-10, TP),
//   HOTA = sqrt(DetA * AssA).
//
// STATE (owned by the caller, all zero when fresh; ops.HOTA_STATE_SPEC; G gt identities, T track ids, P pair slots, L log entries,
// F frames)
//   gstate  i32 [G, 2]      per gt identity (a dense row, as in mot.hip): frames present, class + 1           (sequence)
//   tcount  i32 [nc, T]     frames a track identity is present in                                            (sequence)
//   pkey    i64 [P]         the sparse pair table, open addressing: ((gt row << 32) | track id) + 1, 0 free   (sequence)
//   ppot    f64 [P]         the pair's pot                                                                    (sequence)
//   phist   i32 [P, 20]     matches of the pair by level = the number of thresholds its S passed             (sequence)
//   fidx    i32 [F, 4]      per logged frame: first log entry, entries, ground-truth rows n, track rows m     (sequence)
//   log     i32 [L, 4]      16 bytes per positive pair of a frame: S (f64), pair slot, row i and column j (u16 each)   (sequence)
//   dets    i32 [nc, 2]     gt_dets, trk_dets                                                                (run totals)
//   tp_lvl  i32 [nc, 20]    matched pairs by level                                                           (run totals)
//   loc_lvl f64 [nc, 20]    the sum of their S by level                                                      (run totals)
//   ass     f64 [3, nc, 19] ass_sum, assre_sum, asspr_sum                                                    (run totals)
//   hdr     i32 [16]        frames logged, log entries used, then what was left out: rows with a gt identity beyond G, with a track
//                           id beyond T, rows beyond ng / nq, pairs beyond L, frames beyond F, pairs that found no slot
// A pair matched at level k is a TP for every threshold a < k, so TP[c, a] = sum of tp_lvl[c, k] over k > a, loc_sum likewise, and the
// 19 mc_a of a pair are a suffix sum over its 20-bin histogram.  There is no [19, G, T] table.  Whatever exceeds a capacity is counted
// in hdr and left out: nothing is written past a table.
// Several streams (tamtr_hota_update_streams, tamtr_hota_end_streams): each of the twelve tensors gains a leading S (gstate [S, G, 2],
// ..., hdr [S, 16]; the state array still holds 12 pointers) and slice s is the state above for stream s, run totals included: the
// single entries take state[k][s] as it is.
//
// DESIGN
// Update: one workgroup of 256 threads walks the frames in order, as mot_update_kernel does, so every pot cell has one adder per frame
// and the frames add in order: plain fp64 adds, no atomics, the same sum on every run.  Steps 1 and 2 are mot_frame_filter
// (mot_rule.h), as in mot_update_kernel; running both evaluators runs them twice.  The update's workspace is the filter's block
// (mot_frame_ws_bytes), then rsum [ng] and csum [nq].  The frame's positive pairs go to the log with the slot of
// their pair, so the second pass needs neither the boxes nor a table lookup; the log grows by the pairs present, not by nq x ng.
// End of sequence, launch 1 (matching): `workgroups` workgroups stride over the logged frames - they are independent, unlike CLEAR's.
// Each scatters the frame's pairs into a dense score matrix in its own slice of the workspace, takes out the isolated pairs and
// solves the rest (mot_assign_sparse), then bumps the level bins of the matched pairs (integer atomics; loc_lvl is an fp64 atomic
// add, so its last bits depend on the order).  Launch 2 (reduction): one thread per pair slot forms the pair's 19 terms, adds them to
// `ass` (fp64 atomics) and clears the slot.  Launch 3 clears gstate, tcount and the two counters of hdr.
// Several streams: as in mot.hip.  Update: grid = S, workgroup s walks the images s, s + S, ... of the frame-major batch on slice s
// (hota_stream) of the state and of the workspace; an image whose `active` word is 0 is no frame of its stream (nothing is logged, no
// frame is used up).  End: the same three launches with the stream as the grid's second dimension; the workgroups of a stream whose
// `ending` word is 0 return at once.  `workgroups` is per stream (the host picks min(64, 1024 / S), at least 1) and each has its own
// workspace slice inside its stream's.  No atomic is shared between streams; ppot stays plain in-order adds.  The single entries are
// the same launchers with S = 1 and no masks.
#include "common.h"
#include "mot_rule.h"

#define HOTA_THREADS 256
#define HOTA_NA 19
#define HOTA_LEVELS 20

enum { HH_FRAMES, HH_LOG, HH_OVER_GT, HH_OVER_TRK, HH_OVER_ROWS, HH_OVER_LOG, HH_OVER_FRAMES, HH_OVER_PAIRS };

struct HotaPair {
  double s;
  int32_t slot;
  uint16_t i, j;
};
static_assert(sizeof(HotaPair) == 16, "a log entry is 16 bytes");

struct HotaState {
  int32_t* gstate;
  int32_t* tcount;
  unsigned long long* pkey;
  double* ppot;
  int32_t* phist;
  int32_t* fidx;
  HotaPair* log;
  int32_t* dets;
  int32_t* tp_lvl;
  double* loc_lvl;
  double* ass;
  int32_t* hdr;
  int nc, G, T, P, L, F;
};

// slice s of a stacked state: every tensor of HOTA_STATE_SPEC has a leading S
static __device__ inline HotaState hota_stream(HotaState st, int s) {
  const size_t z = (size_t)s;
  st.gstate += z * st.G * 2;
  st.tcount += z * st.nc * st.T;
  st.pkey += z * st.P;
  st.ppot += z * st.P;
  st.phist += z * st.P * HOTA_LEVELS;
  st.fidx += z * st.F * 4;
  st.log += z * st.L;
  st.dets += z * st.nc * 2;
  st.tp_lvl += z * st.nc * HOTA_LEVELS;
  st.loc_lvl += z * st.nc * HOTA_LEVELS;
  st.ass += z * 3 * st.nc * HOTA_NA;
  st.hdr += z * 16;
  return st;
}

static size_t hota_update_ws_bytes(size_t nq, size_t ng) { return mot_frame_ws_bytes(nq, ng) + 8 * (ng + nq); }   // the frame's block, then rsum and csum
static __host__ __device__ inline size_t hota_end_ws_per_group(size_t nq, size_t ng) { return (8 * ng * nq + 4 * (5 * ng + 3 * nq) + 15) & ~(size_t)15; }

struct HotaUpdateParams {
  const float* tracks;
  const int32_t* tcounts;
  const float* gt;
  const int32_t* gcounts;
  const int32_t* active;   // [B] or NULL: an image whose word is 0 is no frame of its stream
  int B, S, nq, ng;
  double thr, eps;
  HotaState st;
  unsigned char* ws;
  size_t ws_slice;   // bytes between the workspaces of two streams
};

__global__ __launch_bounds__(HOTA_THREADS) void hota_update_kernel(HotaUpdateParams p) {
  extern __shared__ __align__(16) unsigned char lds[];
  __shared__ int wsum[(HOTA_THREADS / WAVE)];
  __shared__ MotCand red[(HOTA_THREADS / WAVE)];
  __shared__ int lcnt;
  // workgroup s owns slice s of the state and of the workspace, and the images s, s + S, ... of the batch
  const int s = blockIdx.x;
  const HotaState st = hota_stream(p.st, s);
  const int tid = threadIdx.x, nq = p.nq, ng = p.ng, nc = st.nc;
  const MotLsap w = mot_lsap_carve(lds, ng, nq + 1);
  const MotFrame f = mot_frame_carve(p.ws + (size_t)s * p.ws_slice, nq, ng);
  const double* iouM = f.iouM;
  const int *gl = f.gl, *g3 = f.g3, *tl = f.tl, *t3 = f.t3;
  double* rsum = reinterpret_cast<double*>(f.end);   // [n3] the row sums of the class's similarity; 8-byte aligned (mot_frame_ws_bytes)
  double* csum = rsum + ng;                          // [m3]
  int fid = st.hdr[HH_FRAMES], used = st.hdr[HH_LOG];

  for (int b = s; b < p.B; b += p.S) {
    if (p.active && p.active[b] == 0) continue;   // uniform: not a frame of this stream
    if (fid >= st.F) {   // uniform: the frame is left out whole
      if (tid == 0) atomicAdd(&st.hdr[HH_OVER_FRAMES], 1);
      continue;
    }
    const float* G = p.gt + (size_t)b * ng * 7;
    const float* Tr = p.tracks + (size_t)b * nq * 8;
    if (tid == 0) lcnt = 0;   // the filter passes a barrier between this store and pass 1's atomicAdd
    // ---- steps 1 and 2 of the MOT rule
    const MotFrameSets fs = mot_frame_filter<HOTA_THREADS, true>(G, Tr, p.gcounts[b], p.tcounts[b], ng, nq, nc, st.G, st.T, p.thr,
                                                                 &st.hdr[HH_OVER_GT], f, w, red, wsum, [](const float*) {}, [](const float*) {});
    const int ntl = fs.ntl, n3 = fs.n3, m3 = fs.m3;
    auto gcls = [&](int a) { return (int)G[(size_t)gl[g3[a]] * 7 + 5]; };
    auto gidx = [&](int a) { return (int)G[(size_t)gl[g3[a]] * 7 + 4]; };
    auto tcls = [&](int c2) { return (int)Tr[(size_t)tl[t3[c2]] * 8 + 6]; };
    auto tidx = [&](int c2) { return (int)Tr[(size_t)tl[t3[c2]] * 8 + 4]; };
    auto sim = [&](int a, int c2) { return iouM[(size_t)g3[a] * ntl + t3[c2]]; };
    // ---- pass 1: presence counts, the sums of the class's similarity, pot and the log
    for (int a = tid; a < n3; a += HOTA_THREADS) {
      const int c = gcls(a);
      atomicAdd(&st.gstate[(size_t)gidx(a) * 2], 1);
      st.gstate[(size_t)gidx(a) * 2 + 1] = c + 1;
      atomicAdd(&st.dets[c * 2], 1);
      double s = 0.0;
      for (int c2 = 0; c2 < m3; ++c2)
        if (tcls(c2) == c) s += sim(a, c2);
      rsum[a] = s;
    }
    for (int c2 = tid; c2 < m3; c2 += HOTA_THREADS) {
      const int c = tcls(c2);
      atomicAdd(&st.tcount[(size_t)c * st.T + tidx(c2)], 1);
      atomicAdd(&st.dets[c * 2 + 1], 1);
      double s = 0.0;
      for (int a = 0; a < n3; ++a)
        if (gcls(a) == c) s += sim(a, c2);
      csum[c2] = s;
    }
    __syncthreads();
    for (int e = tid; e < n3 * m3; e += HOTA_THREADS) {
      const int a = e / m3, c2 = e - a * m3;
      const double v = sim(a, c2);
      if (!(v > 0.0) || gcls(a) != tcls(c2)) continue;
      const double den = (rsum[a] + csum[c2]) - v;
      const int slot = mot_pair_slot(st.pkey, st.P, gidx(a), tidx(c2));
      if (slot < 0) { atomicAdd(&st.hdr[HH_OVER_PAIRS], 1); continue; }
      st.ppot[slot] += den > p.eps ? v / den : 0.0;
      const int k = used + atomicAdd(&lcnt, 1);
      if (k < st.L) st.log[k] = HotaPair{v, slot, (uint16_t)a, (uint16_t)c2};
      else atomicAdd(&st.hdr[HH_OVER_LOG], 1);
    }
    __syncthreads();
    const int written = min(lcnt, st.L - used);
    if (tid == 0) {
      int32_t* fx = st.fidx + (size_t)fid * 4;
      fx[0] = used; fx[1] = written; fx[2] = n3; fx[3] = m3;
    }
    used += written;
    ++fid;
    __syncthreads();   // lcnt is read by all before the next frame clears it
  }
  if (tid == 0) { st.hdr[HH_FRAMES] = fid; st.hdr[HH_LOG] = used; }
}

struct HotaMatchParams {
  HotaState st;
  const int32_t* ending;   // [S] or NULL: the workgroups of a stream whose word is 0 return at once
  int nq, ng;
  double eps;
  double alpha[HOTA_NA];
  unsigned char* ws;
  size_t ws_slice;
};

__global__ __launch_bounds__(HOTA_THREADS) void hota_match_kernel(HotaMatchParams p) {
  extern __shared__ __align__(16) unsigned char lds[];
  __shared__ int wsum[(HOTA_THREADS / WAVE)];
  __shared__ MotCand red[(HOTA_THREADS / WAVE)];
  const int s = blockIdx.y;
  if (p.ending && p.ending[s] == 0) return;
  const HotaState st = hota_stream(p.st, s);
  const int tid = threadIdx.x, nq = p.nq, ng = p.ng;
  const MotLsap w = mot_lsap_carve(lds, ng, nq + 1);
  unsigned char* base = p.ws + (size_t)s * p.ws_slice + (size_t)blockIdx.x * hota_end_ws_per_group(nq, ng);
  double* S = reinterpret_cast<double*>(base);                     // [n, m] minus the score
  int* x = reinterpret_cast<int*>(S + (size_t)ng * nq);
  MotSparse sq;
  sq.rcnt = x + ng; sq.rone = sq.rcnt + ng; sq.rl = sq.rone + ng; sq.xr = sq.rl + ng;
  sq.ccnt = sq.xr + ng; sq.cone = sq.ccnt + nq; sq.cl = sq.cone + nq;
  const int frames = min(st.hdr[HH_FRAMES], st.F);
  for (int f = blockIdx.x; f < frames; f += gridDim.x) {
    const int32_t* fx = st.fidx + (size_t)f * 4;
    const int off = fx[0], np = fx[1], n = fx[2], m = fx[3];
    if (np <= 0) continue;
    if (off < 0 || off > st.L - np || n > ng || m > nq) {   // a frame logged for wider rows than this launch is sized for
      if (tid == 0) atomicAdd(&st.hdr[HH_OVER_ROWS], 1);
      continue;
    }
    const HotaPair* pairs = st.log + off;
    for (int e = tid; e < n * m; e += HOTA_THREADS) S[e] = 0.0;
    __syncthreads();
    for (int e = tid; e < np; e += HOTA_THREADS) {
      const HotaPair q = pairs[e];
      if (q.i >= n || q.j >= m || q.slot < 0 || q.slot >= st.P) continue;
      const unsigned long long key = st.pkey[q.slot] - 1ull;
      const int g = (int)(key >> 32), t = (int)(unsigned)key;
      if (g >= st.G || t >= st.T) continue;
      const int c = st.gstate[(size_t)g * 2 + 1] - 1;
      if (c < 0 || c >= st.nc) continue;
      const double pot = st.ppot[q.slot];
      const double gas = pot / ((double)(st.gstate[(size_t)g * 2] + st.tcount[(size_t)c * st.T + t]) - pot);
      S[(size_t)q.i * m + q.j] = -(gas * q.s);
    }
    __syncthreads();
    mot_assign_sparse<HOTA_THREADS>(S, n, m, w, sq, x, red, wsum);
    for (int e = tid; e < np; e += HOTA_THREADS) {
      const HotaPair q = pairs[e];
      if (q.i >= n || q.j >= m || q.slot < 0 || q.slot >= st.P) continue;
      if (x[q.i] != q.j || !(S[(size_t)q.i * m + q.j] < 0.0)) continue;
      int level = 0;
#pragma unroll
      for (int a = 0; a < HOTA_NA; ++a) level += q.s >= p.alpha[a] - p.eps ? 1 : 0;
      const int c = st.gstate[(size_t)(int)((st.pkey[q.slot] - 1ull) >> 32) * 2 + 1] - 1;
      atomicAdd(&st.phist[(size_t)q.slot * HOTA_LEVELS + level], 1);
      atomicAdd(&st.tp_lvl[c * HOTA_LEVELS + level], 1);
      atomicAdd(&st.loc_lvl[c * HOTA_LEVELS + level], q.s);
    }
    __syncthreads();   // S and x are read before the next frame overwrites them
  }
}

__global__ __launch_bounds__(HOTA_THREADS) void hota_reduce_kernel(HotaState all, const int32_t* ending) {
  if (ending && ending[blockIdx.y] == 0) return;
  const HotaState st = hota_stream(all, blockIdx.y);
  const size_t plane = (size_t)st.nc * HOTA_NA;
  for (int s = blockIdx.x * HOTA_THREADS + threadIdx.x; s < st.P; s += gridDim.x * HOTA_THREADS) {
    const unsigned long long k1 = st.pkey[s];
    if (k1 == 0ull) continue;
    const unsigned long long key = k1 - 1ull;
    const int g = (int)(key >> 32), t = (int)(unsigned)key;
    int32_t* hist = st.phist + (size_t)s * HOTA_LEVELS;
    if (g < st.G && t < st.T) {
      const int c = st.gstate[(size_t)g * 2 + 1] - 1;
      if (c >= 0 && c < st.nc) {
        const int gc = st.gstate[(size_t)g * 2], tc = st.tcount[(size_t)c * st.T + t];
        int mc = 0;
        for (int a = HOTA_NA - 1; a >= 0; --a) {
          mc += hist[a + 1];
          if (mc <= 0) continue;
          const double sq = (double)mc * (double)mc;
          atomicAdd(&st.ass[(size_t)c * HOTA_NA + a], sq / (double)max(1, gc + tc - mc));
          atomicAdd(&st.ass[plane + (size_t)c * HOTA_NA + a], sq / (double)max(1, gc));
          atomicAdd(&st.ass[2 * plane + (size_t)c * HOTA_NA + a], sq / (double)max(1, tc));
        }
      }
    }
    for (int k = 0; k < HOTA_LEVELS; ++k) hist[k] = 0;
    st.ppot[s] = 0.0;
    st.pkey[s] = 0ull;
  }
}

__global__ __launch_bounds__(HOTA_THREADS) void hota_clear_kernel(HotaState all, const int32_t* ending) {
  if (ending && ending[blockIdx.y] == 0) return;
  const HotaState st = hota_stream(all, blockIdx.y);
  const size_t ng = (size_t)st.G * 2, nt = (size_t)st.nc * st.T;
  for (size_t e = (size_t)blockIdx.x * HOTA_THREADS + threadIdx.x; e < ng + nt; e += (size_t)gridDim.x * HOTA_THREADS) {
    if (e < ng) st.gstate[e] = 0;
    else st.tcount[e - ng] = 0;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) { st.hdr[HH_FRAMES] = 0; st.hdr[HH_LOG] = 0; }
}

extern "C" int tamtr_hota_workspace_bytes(int nq, int ng, int workgroups) {
  if (nq < 1 || ng < 1 || workgroups < 1) return 0;
  const size_t a = hota_update_ws_bytes(nq, ng), b = (size_t)workgroups * hota_end_ws_per_group(nq, ng);
  const size_t n = (a > b ? a : b) + 16;
  return n > 0x7fffffff ? 0 : (int)n;
}

static bool hota_unsupported(int nq, int ng, int workgroups, const HotaState& st) {
  return tamtr_hota_workspace_bytes(nq, ng, workgroups) == 0 || mot_lsap_bytes(ng, (size_t)nq + 1) > 60 * 1024 || nq > 65535 || ng > 65535 ||
         workgroups > 1024 || st.G > (1 << 24) || st.T > (1 << 24) || st.nc > (1 << 16) || (size_t)st.nc * st.T > 0x7fffffff ||
         (size_t)st.P * HOTA_LEVELS > 0x7fffffff;   // ids travel as fp32
}

static bool hota_state_invalid(const HotaState& st) {
  return !st.gstate || !st.tcount || !st.pkey || !st.ppot || !st.phist || !st.fidx || !st.log || !st.dets || !st.tp_lvl || !st.loc_lvl ||
         !st.ass || !st.hdr || st.nc < 1 || st.G < 1 || st.T < 1 || st.P < 1 || st.L < 1 || st.F < 1;
}

// state: the 12 device pointers in HOTA_STATE_SPEC's order; caps: G, T, P, L, F
static HotaState hota_state(void* const* state, int nc, const int* caps) {
  if (!state || !caps) return HotaState{};
  return HotaState{(int32_t*)state[0], (int32_t*)state[1], (unsigned long long*)state[2], (double*)state[3], (int32_t*)state[4],
                   (int32_t*)state[5], (HotaPair*)state[6], (int32_t*)state[7], (int32_t*)state[8], (double*)state[9], (double*)state[10],
                   (int32_t*)state[11], nc, caps[0], caps[1], caps[2], caps[3], caps[4]};
}

// S stacked evaluators: each stream's slice of the workspace is the single size rounded up to 16 bytes
static size_t hota_ws_slice(int nq, int ng, int workgroups) { return ((size_t)tamtr_hota_workspace_bytes(nq, ng, workgroups) + 15) & ~(size_t)15; }

extern "C" int tamtr_hota_streams_workspace_bytes(int S, int nq, int ng, int workgroups) {
  if (S < 1 || tamtr_hota_workspace_bytes(nq, ng, workgroups) == 0) return 0;
  const size_t slice = hota_ws_slice(nq, ng, workgroups);
  return slice > (size_t)0x7fffffff / S ? 0 : (int)(S * slice);
}

static bool hota_streams_unsupported(int S, int nq, int ng, int workgroups, const HotaState& st) {
  return hota_unsupported(nq, ng, workgroups, st) || S > 65535 || tamtr_hota_streams_workspace_bytes(S, nq, ng, workgroups) == 0;
}

// The one place hota_update_kernel is launched from; tamtr_hota_update is S = 1 without a mask.  The last stream's slice need not be
// rounded up, so with S = 1 the workspace asked for is the single entry's.
extern "C" int tamtr_hota_update_streams(const float* tracks, const int32_t* tcounts, const float* gt, const int32_t* gcounts, int B, int S, int nq,
                                         int ng, int nc, double iou_thr, double eps, const int32_t* active, void* const* state, const int* caps,
                                         void* workspace, int workspace_bytes, void* stream) {
  const HotaState st = hota_state(state, nc, caps);
  if (!tracks || !tcounts || !gt || !gcounts || hota_state_invalid(st) || !workspace || B < 1 || nq < 1 || ng < 1 || !(iou_thr > 0.0) ||
      !(eps > 0.0) || ((uintptr_t)workspace & 15) || S < 1 || B % S != 0)
    return TAMTR_EINVAL;
  if (hota_streams_unsupported(S, nq, ng, 1, st)) return TAMTR_EUNSUP;
  const size_t slice = hota_ws_slice(nq, ng, 1);
  if (workspace_bytes < 0 || (size_t)workspace_bytes < (S - 1) * slice + hota_update_ws_bytes(nq, ng)) return TAMTR_EINVAL;
  HotaUpdateParams p{tracks, tcounts, gt, gcounts, active, B, S, nq, ng, iou_thr, eps, st, static_cast<unsigned char*>(workspace), slice};
  hipLaunchKernelGGL(hota_update_kernel, dim3(S), dim3(HOTA_THREADS), mot_lsap_bytes(ng, (size_t)nq + 1), (hipStream_t)stream, p);
  return tamtr_launch_status();
}

extern "C" int tamtr_hota_update(const float* tracks, const int32_t* tcounts, const float* gt, const int32_t* gcounts, int B, int nq, int ng,
                                 int nc, double iou_thr, double eps, void* const* state, const int* caps, void* workspace,
                                 int workspace_bytes, void* stream) {
  return tamtr_hota_update_streams(tracks, tcounts, gt, gcounts, B, 1, nq, ng, nc, iou_thr, eps, nullptr, state, caps, workspace, workspace_bytes,
                                   stream);
}

// The one place the three launches of the end of a sequence are made from: the stream is the grid's second dimension, and the
// workgroups of a stream that is not ending return at once.  tamtr_hota_end_sequence is S = 1 without a mask.
extern "C" int tamtr_hota_end_streams(const double* alpha, double eps, int nc, int S, const int32_t* ending, int nq, int ng, int workgroups,
                                      void* const* state, const int* caps, void* workspace, int workspace_bytes, void* stream) {
  const HotaState st = hota_state(state, nc, caps);
  if (!alpha || hota_state_invalid(st) || !workspace || nq < 1 || ng < 1 || workgroups < 1 || !(eps > 0.0) || ((uintptr_t)workspace & 15) || S < 1)
    return TAMTR_EINVAL;
  if (hota_streams_unsupported(S, nq, ng, workgroups, st)) return TAMTR_EUNSUP;
  const size_t slice = hota_ws_slice(nq, ng, workgroups);
  if (workspace_bytes < 0 || (size_t)workspace_bytes < (S - 1) * slice + (size_t)workgroups * hota_end_ws_per_group(nq, ng)) return TAMTR_EINVAL;
  HotaMatchParams p{st, ending, nq, ng, eps, {}, static_cast<unsigned char*>(workspace), slice};
  for (int a = 0; a < HOTA_NA; ++a) p.alpha[a] = alpha[a];   // host memory: the 19 values as numpy made them
  hipLaunchKernelGGL(hota_match_kernel, dim3(workgroups, S), dim3(HOTA_THREADS), mot_lsap_bytes(ng, (size_t)nq + 1), (hipStream_t)stream, p);
  const int blocks = (st.P + HOTA_THREADS - 1) / HOTA_THREADS;
  hipLaunchKernelGGL(hota_reduce_kernel, dim3(blocks < 1024 ? blocks : 1024, S), dim3(HOTA_THREADS), 0, (hipStream_t)stream, st, ending);
  const size_t cells = (size_t)st.G * 2 + (size_t)st.nc * st.T;
  const size_t cb = (cells + HOTA_THREADS - 1) / HOTA_THREADS;
  hipLaunchKernelGGL(hota_clear_kernel, dim3(cb < 1024 ? (int)cb : 1024, S), dim3(HOTA_THREADS), 0, (hipStream_t)stream, st, ending);
  return tamtr_launch_status();
}

extern "C" int tamtr_hota_end_sequence(const double* alpha, double eps, int nc, int nq, int ng, int workgroups, void* const* state,
                                       const int* caps, void* workspace, int workspace_bytes, void* stream) {
  return tamtr_hota_end_streams(alpha, eps, nc, 1, nullptr, nq, ng, workgroups, state, caps, workspace, workspace_bytes, stream);
}
