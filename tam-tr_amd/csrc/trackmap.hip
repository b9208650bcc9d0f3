// trackmap.hip - track-mAP on the device, next to the MOT evaluation (mot.hip) and HOTA (hota.hip): average precision over whole
// tracks, ranked by mean confidence and matched to ground-truth tracks by spatio-temporal IoU.  It is the score VisDrone-MOT ranks
// by; the definitions are TrackEval's TrackMAP for boxes, with no area or time ranges and no cap on tracks.  tamtr_trackmap_update
// takes the B frames of a predictor batch in ONE launch, on the rows tamtr_bytetrack_update left on the device;
// tamtr_trackmap_end_sequence matches the sequence's tracks and appends them to the run's table, six launches per sequence; the
// run's accumulation is tamtr_val_coco_accumulate (cocoeval.hip) on that table.  engine.track_map_evaluate is the numpy statement
// of the same rule and this file's checker.
//
// THE RULE
// Inputs: those of the MOT evaluation (mot.hip): per frame, ground-truth rows x1 y1 x2 y2 id cls kind and track rows, fp32; a track
//   row carries its score (column 5 of the tracker's [B, nq, 8] rows; 1 for a result file without scores).  Steps 1 (regions) and 2
//   (distractors) of the MOT rule run unchanged.  What survives is the input here.  An identity is (class, id) on both sides.  Ids
//   are unique within a frame on either side.
// Sums, per identity and pair, fp64 on the fp32 values, added in frame order; area = (x2 - x1) * (y2 - y1):
//   ground truth g: garea[g] += area, gframes[g] += 1;   track t: tarea[t] += area, tscore[t] += score, tframes[t] += 1;
//   every same-class pair of the frame whose intersection (iw * ih with iw > 0 and ih > 0) is positive: inter[g, t] += intersection.
// End of a sequence: IoU(g, t) = inter / ((garea[g] + tarea[t]) - inter) where that union is > 0, else 0; a pair that never
//   intersected has IoU 0.  A track's score is tscore / tframes.
// Matching, per class and threshold thr: the tracks go by score descending, equal scores by track id ascending.  Each takes the
//   still-unmatched ground truth that wins this scan over the ground truths in dense-row order: best starts at
//   min(thr, 1 - 1e-10); a candidate with IoU >= best - eps (eps = np.finfo(float).eps) replaces the choice and sets best = IoU, so
//   the later candidate wins a tie.  A matched ground truth is taken.  The matching is greedy, not an assignment: that is the protocol.
// A sequence adds to the run, per track: its score, its class and one bit per threshold (matched or not), in class order and then
//   the order above; per class: the number of ground-truth identities.
// End of the run, per class and threshold: the rows sorted by score descending (stable), cumulative TP / FP, recall = tp / n_gt,
//   precision = tp / ((tp + fp) + eps), the precision envelope from the right, the 101 recall points by searchsorted(.., 'left'),
//   AP = their mean, AR = the last recall (0 without tracks); a class without ground truth is -1.  This is engine.coco_accumulate
//   on one range and one cut.
//
// STATE (owned by the caller, all zero when fresh; ops.TRACKMAP_STATE_SPEC; G gt identities, T track ids, P pair slots, R run rows)
//   gstate    i32 [G, 2]      per gt identity (a dense row, as in mot.hip): frames present, class + 1     (sequence)
//   garea     f64 [G]         its area sum                                                                (sequence)
//   tframes   i32 [nc, T]     frames a track identity is present in                                       (sequence)
//   tsum      f64 [nc, T, 2]  its area sum and its score sum                                              (sequence)
//   pkey      i64 [P]         the sparse pair table, open addressing: ((gt row << 32) | track id) + 1, 0 free   (sequence)
//   pinter    f64 [P]         the pair's intersection sum                                                 (sequence)
//   rscore    f64 [R]         the run's table: a track's mean score                                       (run)
//   rmeta     i32 [R, 2]      its class, its bits (bit a = matched at threshold a)                        (run)
//   gt_tracks i32 [nc]        ground-truth identities                                                     (run)
//   hdr       i32 [16]        run rows used, sequences ended, then what was left out: rows with a gt identity beyond G, with a track
//                             id beyond T, rows beyond ng / nq, pairs that found no slot, tracks beyond R
// Whatever exceeds a capacity is counted in hdr and left out: nothing is written past a table.
//
// DESIGN
// Update: one workgroup of 256 threads walks the frames in order, as hota_update_kernel does, so every sum has one adder per frame and
// the frames add in order: plain fp64 adds, no atomics, the same bits on every run.  Steps 1 and 2 are mot_frame_filter (mot_rule.h) without
// the IoU matrix, which is filled only in a frame with a distractor; the update's workspace is the filter's block (mot_frame_ws_bytes).
// End of sequence, all in global workspace so that no count has to fit a workgroup or its LDS:
//   1 prep     mean scores (a NaN mean sorts as -inf), zeroed counters and `taken` bytes;
//   2 rank     a track's place is the number of live tracks of its class that go before it, counted against LDS tiles of 256 (T / 256
//              tiles per workgroup): a sort of any length.  The same launch counts each track's candidates over the pair slots and the
//              ground-truth identities per class (integer atomics);
//   3 offsets  one workgroup: the classes' row offsets and, in rank order, where each track's candidate list starts;
//   4 fill     one thread per pair slot writes (gt row, IoU) into its track's list;
//   5 match    one wave per (threshold, class), serial over the tracks in order; the lanes stride over a track's candidates and a
//              shuffle reduction picks the largest IoU among the untaken ones, the larger dense row on a tie.  That is the scan above
//              whenever two candidates of a track are equal or differ by more than eps.  Waves of different thresholds share nothing;
//   6 clear    the sequence's state, and the run's row count moves on.
// The order inside a candidate list depends on the run, the pick does not: every output has the same bits on every run.
#include "common.h"
#include "mot_rule.h"

#define TM_THREADS 256
#define TM_MAX_THR 10

enum { TH_ROWS, TH_SEQS, TH_OVER_GT, TH_OVER_TRK, TH_OVER_ROWS, TH_OVER_PAIRS, TH_OVER_RUN };

struct TmState {
  int32_t* gstate;
  double* garea;
  int32_t* tframes;
  double* tsum;
  unsigned long long* pkey;
  double* pinter;
  double* rscore;
  int32_t* rmeta;
  int32_t* gt_tracks;
  int32_t* hdr;
  int nc, G, T, P, R;
};

// the end-of-sequence workspace: doubles first, then ints, then bytes
struct TmEndWs {
  double *mean, *cand_iou;                                             // [nc, T], [P]
  int32_t *nlive, *coff, *order, *ccount, *cstart, *cursor, *cand_g;   // [nc], [nc + 1], 4 x [nc, T], [P]
  unsigned char* taken;                                                // [nc, TM_MAX_THR, G]
};

static size_t tm_update_ws_bytes(size_t nq, size_t ng) { return mot_frame_ws_bytes(nq, ng); }
static size_t tm_end_ws_bytes(size_t nc, size_t G, size_t T, size_t P) {
  return (8 * (nc * T + P) + 4 * (2 * nc + 1 + 4 * nc * T + P) + nc * TM_MAX_THR * G + 15) & ~(size_t)15;
}
static __host__ __device__ inline TmEndWs tm_end_carve(unsigned char* ws, size_t nc, size_t G, size_t T, size_t P) {
  TmEndWs w;
  w.mean = reinterpret_cast<double*>(ws);
  w.cand_iou = w.mean + nc * T;
  w.nlive = reinterpret_cast<int32_t*>(w.cand_iou + P);
  w.coff = w.nlive + nc;
  w.order = w.coff + nc + 1;
  w.ccount = w.order + nc * T;
  w.cstart = w.ccount + nc * T;
  w.cursor = w.cstart + nc * T;
  w.cand_g = w.cursor + nc * T;
  w.taken = reinterpret_cast<unsigned char*>(w.cand_g + P);
  return w;
}

__device__ __forceinline__ double tm_area(const float* r) { return ((double)r[2] - (double)r[0]) * ((double)r[3] - (double)r[1]); }

struct TmUpdateParams {
  const float* tracks;
  const int32_t* tcounts;
  const float* gt;
  const int32_t* gcounts;
  int B, nq, ng;
  double thr;
  TmState st;
  unsigned char* ws;
};

__global__ __launch_bounds__(TM_THREADS) void trackmap_update_kernel(TmUpdateParams p) {
  extern __shared__ __align__(16) unsigned char lds[];
  __shared__ int wsum[(TM_THREADS / WAVE)];
  __shared__ MotCand red[(TM_THREADS / WAVE)];
  const TmState& st = p.st;
  const int tid = threadIdx.x, nq = p.nq, ng = p.ng, nc = st.nc;
  const MotLsap w = mot_lsap_carve(lds, ng, nq + 1);
  const MotFrame f = mot_frame_carve(p.ws, nq, ng);
  const int *gl = f.gl, *g3 = f.g3, *tl = f.tl, *t3 = f.t3;

  for (int b = 0; b < p.B; ++b) {
    const float* G = p.gt + (size_t)b * ng * 7;
    const float* Tr = p.tracks + (size_t)b * nq * 8;
    // ---- steps 1 and 2 of the MOT rule; the sums need no IoU
    const MotFrameSets fs = mot_frame_filter<TM_THREADS, false>(G, Tr, p.gcounts[b], p.tcounts[b], ng, nq, nc, st.G, st.T, p.thr,
                                                                &st.hdr[TH_OVER_GT], f, w, red, wsum, [](const float*) {}, [](const float*) {});
    const int n3 = fs.n3, m3 = fs.m3;
    auto grow = [&](int a) { return G + (size_t)gl[g3[a]] * 7; };
    auto trow = [&](int c2) { return Tr + (size_t)tl[t3[c2]] * 8; };
    // ---- the sums: ids are unique within a frame, so every cell has one adder
    for (int a = tid; a < n3; a += TM_THREADS) {
      const float* g = grow(a);
      const int gi = (int)g[4];
      st.gstate[(size_t)gi * 2] += 1;
      st.gstate[(size_t)gi * 2 + 1] = (int)g[5] + 1;
      st.garea[gi] += tm_area(g);
    }
    for (int c2 = tid; c2 < m3; c2 += TM_THREADS) {
      const float* t = trow(c2);
      const size_t cell = (size_t)(int)t[6] * st.T + (int)t[4];
      st.tframes[cell] += 1;
      st.tsum[cell * 2] += tm_area(t);
      st.tsum[cell * 2 + 1] += (double)t[5];
    }
    for (int e = tid; e < n3 * m3; e += TM_THREADS) {
      const int a = e / m3, c2 = e - a * m3;
      const float *g = grow(a), *t = trow(c2);
      if ((int)g[5] != (int)t[6]) continue;
      const double v = mot_inter(mot_box(g), mot_box(t));
      if (!(v > 0.0)) continue;
      const int slot = mot_pair_slot(st.pkey, st.P, (int)g[4], (int)t[4]);
      if (slot < 0) { atomicAdd(&st.hdr[TH_OVER_PAIRS], 1); continue; }
      st.pinter[slot] += v;
    }
    __syncthreads();   // the lists are read before the next frame overwrites them
  }
}

// ------------------------------------------------------------------------------------------------ end of a sequence
struct TmEndParams {
  TmState st;
  int nthr;
  double eps;
  double thr[TM_MAX_THR];
  unsigned char* ws;
};

// the pair of an occupied slot: its gt row, track id and class, or false for a key that names nothing live
__device__ __forceinline__ bool tm_pair(const TmState& st, unsigned long long k1, int& g, int& t, int& c) {
  if (k1 == 0ull) return false;
  const unsigned long long key = k1 - 1ull;
  g = (int)(key >> 32); t = (int)(unsigned)key;
  if (g < 0 || g >= st.G || t < 0 || t >= st.T) return false;
  c = st.gstate[(size_t)g * 2 + 1] - 1;
  if (c < 0 || c >= st.nc) return false;
  return st.tframes[(size_t)c * st.T + t] > 0;
}

__global__ __launch_bounds__(TM_THREADS) void trackmap_prep_kernel(TmEndParams p) {
  const TmState& st = p.st;
  const TmEndWs w = tm_end_carve(p.ws, st.nc, st.G, st.T, st.P);
  const size_t cells = (size_t)st.nc * st.T, nt = (size_t)st.nc * TM_MAX_THR * st.G;
  const size_t stride = (size_t)gridDim.x * TM_THREADS, e0 = (size_t)blockIdx.x * TM_THREADS + threadIdx.x;
  for (size_t e = e0; e < cells; e += stride) {
    const int n = st.tframes[e];
    const double m = n > 0 ? st.tsum[e * 2 + 1] / (double)n + 0.0 : 0.0;
    w.mean[e] = m == m ? m : -INFINITY;
    w.ccount[e] = 0;
  }
  for (size_t e = e0; e < nt; e += stride) w.taken[e] = 0;
  for (size_t e = e0; e < (size_t)st.nc; e += stride) w.nlive[e] = 0;
}

// grid (ceil(T / 256), nc)
__global__ __launch_bounds__(TM_THREADS) void trackmap_rank_kernel(TmEndParams p) {
  __shared__ double sm[TM_THREADS];
  __shared__ int sl[TM_THREADS];
  const TmState& st = p.st;
  const TmEndWs w = tm_end_carve(p.ws, st.nc, st.G, st.T, st.P);
  const int tid = threadIdx.x, c = blockIdx.y, T = st.T;
  const int i = blockIdx.x * TM_THREADS + tid;
  const size_t row = (size_t)c * T;
  const bool live = i < T && st.tframes[row + i] > 0;
  const double mi = live ? w.mean[row + i] : 0.0;
  int before = 0;
  for (int j0 = 0; j0 < T; j0 += TM_THREADS) {
    const int j = j0 + tid;
    sl[tid] = j < T && st.tframes[row + j] > 0;
    sm[tid] = j < T ? w.mean[row + j] : 0.0;
    __syncthreads();
    if (live) {
      const int nj = min(TM_THREADS, T - j0);
      for (int k = 0; k < nj; ++k)
        before += (sl[k] && (sm[k] > mi || (sm[k] == mi && j0 + k < i))) ? 1 : 0;
    }
    __syncthreads();
  }
  if (live) {
    if (before < T) w.order[row + before] = i;
    atomicAdd(&w.nlive[c], 1);
  }
  // the candidates per track and the ground-truth identities per class, over the whole grid
  const size_t nb = (size_t)gridDim.x * gridDim.y, bid = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
  for (size_t s = bid * TM_THREADS + tid; s < (size_t)st.P; s += nb * TM_THREADS) {
    int g, t, cc;
    if (tm_pair(st, st.pkey[s], g, t, cc)) atomicAdd(&w.ccount[(size_t)cc * T + t], 1);
  }
  for (size_t g = bid * TM_THREADS + tid; g < (size_t)st.G; g += nb * TM_THREADS) {
    const int cc = st.gstate[g * 2 + 1] - 1;
    if (st.gstate[g * 2] > 0 && cc >= 0 && cc < st.nc) atomicAdd(&st.gt_tracks[cc], 1);
  }
}

// one workgroup
__global__ __launch_bounds__(TM_THREADS) void trackmap_offsets_kernel(TmEndParams p) {
  __shared__ int wsum[(TM_THREADS / WAVE)];
  const TmState& st = p.st;
  const TmEndWs w = tm_end_carve(p.ws, st.nc, st.G, st.T, st.P);
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wv = tid / WAVE, T = st.T;
  if (tid == 0) {
    int off = 0;
    for (int c = 0; c < st.nc; ++c) { w.coff[c] = off; off += min(max(w.nlive[c], 0), T); }
    w.coff[st.nc] = off;
  }
  int running = 0;
  for (int c = 0; c < st.nc; ++c) {
    const int n = min(max(w.nlive[c], 0), T);
    const size_t row = (size_t)c * T;
    for (int r0 = 0; r0 < n; r0 += TM_THREADS) {
      const int r = r0 + tid;
      int t = -1, v = 0;
      if (r < n) {
        t = w.order[row + r];
        if (t < 0 || t >= T) t = -1;
        else v = w.ccount[row + t];
      }
      int inc = v;   // inclusive scan inside the wave
#pragma unroll
      for (int d = 1; d < WAVE; d <<= 1) {
        const int o = __shfl_up(inc, d, WAVE);
        if (lane >= d) inc += o;
      }
      if (lane == WAVE - 1) wsum[wv] = inc;
      __syncthreads();
      int off = running, tot = 0;
#pragma unroll
      for (int k = 0; k < (TM_THREADS / WAVE); ++k) {
        const int s = wsum[k];
        if (k < wv) off += s;
        tot += s;
      }
      if (r < n) {
        w.cstart[row + r] = off + inc - v;
        if (t >= 0) w.cursor[row + t] = off + inc - v;
      }
      running += tot;
      __syncthreads();
    }
  }
}

__global__ __launch_bounds__(TM_THREADS) void trackmap_fill_kernel(TmEndParams p) {
  const TmState& st = p.st;
  const TmEndWs w = tm_end_carve(p.ws, st.nc, st.G, st.T, st.P);
  for (size_t s = (size_t)blockIdx.x * TM_THREADS + threadIdx.x; s < (size_t)st.P; s += (size_t)gridDim.x * TM_THREADS) {
    int g, t, c;
    if (!tm_pair(st, st.pkey[s], g, t, c)) continue;
    const size_t cell = (size_t)c * st.T + t;
    const int pos = atomicAdd(&w.cursor[cell], 1);
    if (pos < 0 || pos >= st.P) continue;
    const double inter = st.pinter[s];
    const double uni = (st.garea[g] + st.tsum[cell * 2]) - inter;
    w.cand_g[pos] = g;
    w.cand_iou[pos] = uni > 0.0 ? inter / uni : 0.0;
  }
}

// grid (nthr, nc), one wave each
__global__ __launch_bounds__(WAVE) void trackmap_match_kernel(TmEndParams p) {
  const TmState& st = p.st;
  const TmEndWs w = tm_end_carve(p.ws, st.nc, st.G, st.T, st.P);
  const int lane = threadIdx.x, a = blockIdx.x, c = blockIdx.y, T = st.T;
  const size_t row = (size_t)c * T;
  const int n = min(max(w.nlive[c], 0), T);
  const long long base = (long long)st.hdr[TH_ROWS] + w.coff[c];
  unsigned char* taken = w.taken + ((size_t)c * TM_MAX_THR + a) * st.G;
  const double floor_ = fmin(p.thr[a], 1.0 - 1e-10) - p.eps;
  if (a == 0)
    for (int r = lane; r < n; r += WAVE) {
      const int t = w.order[row + r];
      if (base + r < st.R && t >= 0 && t < T) {
        st.rscore[base + r] = w.mean[row + t];
        st.rmeta[(base + r) * 2] = c;
      }
    }
  for (int r = 0; r < n; ++r) {
    const int t = w.order[row + r];
    if (t < 0 || t >= T) continue;
    const int cnt = w.ccount[row + t];
    if (cnt <= 0) continue;          // uniform over the wave
    const int s0 = w.cstart[row + r];
    double bi = -1.0;
    int bg = -1;
    for (int k = lane; k < cnt; k += WAVE) {
      const int pos = s0 + k;
      if (pos < 0 || pos >= st.P) continue;
      const int g = w.cand_g[pos];
      const double v = w.cand_iou[pos];
      if (g < 0 || g >= st.G || taken[g]) continue;
      if (v > bi || (v == bi && g > bg)) { bi = v; bg = g; }
    }
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) {
      const double oi = __shfl_xor(bi, o, WAVE);
      const int og = __shfl_xor(bg, o, WAVE);
      if (oi > bi || (oi == bi && og > bg)) { bi = oi; bg = og; }
    }
    if (bg >= 0 && bi >= floor_) {
      if (lane == 0) {
        taken[bg] = 1;
        if (base + r < st.R) atomicOr(&st.rmeta[(base + r) * 2 + 1], 1 << a);
      }
      __syncthreads();   // one wave: the store to `taken` is seen by the next track's loads
    }
  }
}

__global__ __launch_bounds__(TM_THREADS) void trackmap_clear_kernel(TmEndParams p) {
  const TmState& st = p.st;
  const TmEndWs w = tm_end_carve(p.ws, st.nc, st.G, st.T, st.P);
  const size_t stride = (size_t)gridDim.x * TM_THREADS, e0 = (size_t)blockIdx.x * TM_THREADS + threadIdx.x;
  for (size_t e = e0; e < (size_t)st.G; e += stride) { st.gstate[e * 2] = 0; st.gstate[e * 2 + 1] = 0; st.garea[e] = 0.0; }
  for (size_t e = e0; e < (size_t)st.nc * st.T; e += stride) { st.tframes[e] = 0; st.tsum[e * 2] = 0.0; st.tsum[e * 2 + 1] = 0.0; }
  for (size_t e = e0; e < (size_t)st.P; e += stride) { st.pkey[e] = 0ull; st.pinter[e] = 0.0; }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const int used = min(max(st.hdr[TH_ROWS], 0), st.R), total = w.coff[st.nc];
    const int fit = min(total, st.R - used);
    st.hdr[TH_ROWS] = used + fit;
    st.hdr[TH_SEQS] += 1;
    if (total > fit) st.hdr[TH_OVER_RUN] += total - fit;
  }
}

extern "C" int tamtr_trackmap_workspace_bytes(int nq, int ng, int nc, int gt_capacity, int track_capacity, int pair_capacity) {
  if (nq < 1 || ng < 1 || nc < 1 || gt_capacity < 1 || track_capacity < 1 || pair_capacity < 1) return 0;
  if (nq > 65535 || ng > 65535 || nc > 4096 || gt_capacity > (1 << 24) || track_capacity > (1 << 24) || pair_capacity > (1 << 28)) return 0;
  if ((size_t)nc * track_capacity > 0x7fffffff / 16 || (size_t)nc * TM_MAX_THR * gt_capacity > 0x7fffffff) return 0;
  const size_t a = tm_update_ws_bytes(nq, ng), b = tm_end_ws_bytes(nc, gt_capacity, track_capacity, pair_capacity);
  const size_t n = (a > b ? a : b) + 16;
  return n > 0x7fffffff ? 0 : (int)n;
}

static bool tm_state_invalid(const TmState& st) {
  return !st.gstate || !st.garea || !st.tframes || !st.tsum || !st.pkey || !st.pinter || !st.rscore || !st.rmeta || !st.gt_tracks || !st.hdr ||
         st.nc < 1 || st.G < 1 || st.T < 1 || st.P < 1 || st.R < 1;
}

// state: the 10 device pointers in TRACKMAP_STATE_SPEC's order; caps: G, T, P, R
static TmState tm_state(void* const* state, int nc, const int* caps) {
  if (!state || !caps) return TmState{};
  return TmState{(int32_t*)state[0], (double*)state[1], (int32_t*)state[2], (double*)state[3], (unsigned long long*)state[4], (double*)state[5],
                 (double*)state[6], (int32_t*)state[7], (int32_t*)state[8], (int32_t*)state[9], nc, caps[0], caps[1], caps[2], caps[3]};
}

extern "C" int tamtr_trackmap_update(const float* tracks, const int32_t* tcounts, const float* gt, const int32_t* gcounts, int B, int nq, int ng,
                                     int nc, double iou_thr, void* const* state, const int* caps, void* workspace, int workspace_bytes,
                                     void* stream) {
  const TmState st = tm_state(state, nc, caps);
  if (!tracks || !tcounts || !gt || !gcounts || tm_state_invalid(st) || !workspace || B < 1 || nq < 1 || ng < 1 || !(iou_thr > 0.0) ||
      ((uintptr_t)workspace & 15))
    return TAMTR_EINVAL;
  if (tamtr_trackmap_workspace_bytes(nq, ng, st.nc, st.G, st.T, st.P) == 0 || st.R > (1 << 30) ||
      mot_lsap_bytes(ng, (size_t)nq + 1) > 60 * 1024)
    return TAMTR_EUNSUP;
  if ((size_t)workspace_bytes < tm_update_ws_bytes(nq, ng)) return TAMTR_EINVAL;
  TmUpdateParams p{tracks, tcounts, gt, gcounts, B, nq, ng, iou_thr, st, static_cast<unsigned char*>(workspace)};
  hipLaunchKernelGGL(trackmap_update_kernel, dim3(1), dim3(TM_THREADS), mot_lsap_bytes(ng, (size_t)nq + 1), (hipStream_t)stream, p);
  return tamtr_launch_status();
}

extern "C" int tamtr_trackmap_end_sequence(const double* thresholds, int n_thresholds, double eps, int nc, void* const* state, const int* caps,
                                           void* workspace, int workspace_bytes, void* stream) {
  const TmState st = tm_state(state, nc, caps);
  if (!thresholds || n_thresholds < 1 || n_thresholds > TM_MAX_THR || tm_state_invalid(st) || !workspace || !(eps > 0.0) ||
      ((uintptr_t)workspace & 15))
    return TAMTR_EINVAL;
  if (tamtr_trackmap_workspace_bytes(1, 1, st.nc, st.G, st.T, st.P) == 0 || st.R > (1 << 30)) return TAMTR_EUNSUP;
  if ((size_t)workspace_bytes < tm_end_ws_bytes(st.nc, st.G, st.T, st.P)) return TAMTR_EINVAL;
  TmEndParams p{st, n_thresholds, eps, {}, static_cast<unsigned char*>(workspace)};
  for (int a = 0; a < n_thresholds; ++a) p.thr[a] = thresholds[a];   // host memory: the values as numpy made them
  hipStream_t s = (hipStream_t)stream;
  auto blocks = [](size_t n) { const size_t b = (n + TM_THREADS - 1) / TM_THREADS; return dim3((unsigned)(b < 1 ? 1 : b < 1024 ? b : 1024)); };
  const size_t cells = (size_t)st.nc * st.T, nt = (size_t)st.nc * TM_MAX_THR * st.G;
  hipLaunchKernelGGL(trackmap_prep_kernel, blocks(cells > nt ? cells : nt), dim3(TM_THREADS), 0, s, p);
  hipLaunchKernelGGL(trackmap_rank_kernel, dim3((unsigned)((st.T + TM_THREADS - 1) / TM_THREADS), (unsigned)st.nc), dim3(TM_THREADS), 0, s, p);
  hipLaunchKernelGGL(trackmap_offsets_kernel, dim3(1), dim3(TM_THREADS), 0, s, p);
  hipLaunchKernelGGL(trackmap_fill_kernel, blocks(st.P), dim3(TM_THREADS), 0, s, p);
  hipLaunchKernelGGL(trackmap_match_kernel, dim3((unsigned)n_thresholds, (unsigned)st.nc), dim3(WAVE), 0, s, p);
  const size_t most = cells > (size_t)st.P ? cells : (size_t)st.P;
  hipLaunchKernelGGL(trackmap_clear_kernel, blocks(most > (size_t)st.G ? most : (size_t)st.G), dim3(TM_THREADS), 0, s, p);
  return tamtr_launch_status();
}
