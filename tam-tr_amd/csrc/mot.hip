// mot.hip - MOT evaluation on the device: CLEAR-MOT (MOTA, MOTP, FP, FN, IDSW, Frag, MT / PT / ML) and identity (IDF1, IDP, IDR)
// counts of the tracker's rows against ground truth, per class.  The reference leaves this to an outside toolkit; the definitions are
// TrackEval's CLEAR and Identity.  tamtr_mot_update takes the B frames of a predictor batch, in order, in ONE launch, reading the rows
// tamtr_bytetrack_update left on the device; tamtr_mot_end_sequence reduces a sequence in one launch.  engine.mot_evaluate is the
// numpy statement of the same rule and this file's checker.
//
// THE RULE
// Inputs, per frame of one sequence, frames in order:
//   ground-truth rows  x1 y1 x2 y2 id cls kind   kind 0 object, 1 distractor (annotated, not to be scored), 2 ignored region
//   track rows         x1 y1 x2 y2 id cls        (the device reads them from the tracker's 8-column rows: id at 4, cls at 6)
//   all fp32, pixels of the original image.  A class outside [0, nc) on a kind-0 row or on a track row takes that row out of
//   everything; kinds 1 and 2 ignore their class; any other kind takes the row out.
// Arithmetic: coordinates are promoted to fp64; the object is compiled with -ffp-contract=off, so device and numpy agree to the bit
// on every IoU and every threshold comparison.
//   iw = min(ax2, bx2) - max(ax1, bx1), ih likewise; iw <= 0 or ih <= 0 -> 0; else inter = iw * ih,
//   union = (areaA + areaB) - inter, iou = inter / union, 0 when union <= 0.
//   ioa(track, region) = inter / area_track, 0 when the track area is not positive.
//   A pair qualifies when iou >= thr (0.5 by default; exactly thr qualifies).
// Per frame:
//   1. Regions.  A track row whose ioa with any kind-2 row is > 0.5 is dropped (exactly 0.5 stays).
//   2. Distractors.  One assignment between all kind-0 and kind-1 rows and the remaining track rows; score = iou where the pair
//      qualifies and the classes agree (a kind-1 row agrees with every class), else 0; maximise the total.  Track rows matched with
//      score > 0 to a kind-1 row are dropped.  Kind-1 and kind-2 rows then leave the frame.
//   3. CLEAR matching per class c, between the kind-0 rows of class c and the remaining track rows of class c: score = iou + 1000 if
//      the pair qualifies and the track id equals the id this ground truth was last matched to (in any earlier frame, however long
//      ago), iou if it only qualifies, else 0.  Maximise the total; matches with score > 0 are TP, unmatched ground truths FN,
//      unmatched tracks FP.  iou_sum adds the IoU itself.  A matched ground truth whose last-matched id exists and differs is one
//      IDSW; then its last-matched id is updated.
//   4. Pair counts.  Every qualifying pair of step 3's two sets adds 1 to pair[gt id, track id], matched or not; gt_dets and trk_dets
//      count the rows of the two sets, and every gt id counts the frames it is present in.
// Per sequence:
//   a gt id present in n frames and matched in m: m / n > 0.8 is MT, < 0.2 is ML, else PT.  Its Frag is the number of maximal runs
//   of consecutive matched frames, minus 1 (absent or unmatched frames break a run).
//   Identity, per class: IDTP = the largest total of pair counts over one-to-one matchings of the gt ids and track ids of the class
//   (TrackEval's (G+T) x (G+T) problem: a matching costs sum(gt_dets) + sum(trk_dets) - 2 sum(pair) there);
//   IDFN = gt_dets - IDTP, IDFP = trk_dets - IDTP.  An id that changes class mid-sequence is a different identity in each class.
// Summary (engine.mot_summary), per class and summed: MOTA = 1 - (FN + FP + IDSW) / gt_dets, MOTP = iou_sum / TP, Recall = TP / gt_dets,
//   Precision = TP / trk_dets, IDF1 = IDTP / (IDTP + 0.5 IDFP + 0.5 IDFN), IDP = IDTP / trk_dets, IDR = IDTP / gt_dets; nan on a zero
//   denominator.  Counts of several sequences add.
//
// STATE (owned by the caller, all zero when fresh; ops.MOT_STATE_SPEC)
//   gstate  i32 [G, 8]   per gt identity: last-matched track id + 1, frames present, frames matched, runs, last matched frame, class + 1
//   counts  i32 [nc, 16] TP FN FP IDSW gt_dets trk_dets Frag MT PT ML IDTP gt_ids drop_region drop_distractor 0 0   (run totals)
//   iou_sum f64 [nc]
//   pair    i32 [G, T]   the sequence's pair table
//   hdr     i32 [8]      frame counter of the sequence, gt ids beyond G, track ids beyond T, rows beyond ng / nq, 0...
// gt ids reach the device as dense rows [0, G) - the host maps (class, id) to them, so a row has one class and pair needs no class
// axis; track ids are used as they are, [0, T).  An id or a per-frame row count beyond capacity is counted in hdr and the row is left
// out: nothing is written past a table.  The CLEAR counts add straight into the run totals; Frag, MT / PT / ML, gt_ids and IDTP are
// added by tamtr_mot_end_sequence, which then clears gstate, the rows of pair it used and the frame counter.
// Several streams (tamtr_mot_update_streams, tamtr_mot_end_streams): every tensor gains a leading S - gstate [S, G, 8], counts
// [S, nc, 16], iou_sum [S, nc], pair [S, G, T], hdr [S, 8] - and slice s is the state above for stream s, run totals included: the
// single entries take state[k][s] as it is.  The host keeps one (class, id) -> dense row map per stream.
//
// DESIGN
// Update: one workgroup of 256 threads walks the frames in order (step 3 depends on the frame before; the whole update is one launch,
// so the frames' independent parts are not split over workgroups - that would need a grid-wide barrier).  Steps 1 and 2 are
// mot_frame_filter (mot_rule.h), which hota.hip and trackmap.hip call too.  The frame's IoU matrix
// (all gt rows x all surviving track rows, fp64) lives in the caller's workspace in global memory (300 x 300 f64 does not fit the
// LDS), and next to it the cost matrix of the assignment being solved, written once per assignment by all threads so the solver's
// serial steps read one value each.  Step 3 is solved as ONE assignment over all classes with score 0 on a class mismatch: the
// problem is block diagonal, so its optimum is the per-class optima.  Step 2 is skipped in a frame without a kind-1 row (it could drop
// nothing).  Before the solver runs, the pairs that are a connected component of their own (a row and a column that meet only each
// other) are matched directly - in a typical frame that is most of them - and only the contested rows and columns are solved.  The solver (mot_lsap.h) keeps duals and paths in LDS.  Counts are integer atomics
// (order-free); iou_sum is an fp64 atomic add, so its last bits depend on the order (n * 2^-53 relative).
// End of sequence: one workgroup per class.  It lists the class's gt rows, reduces MT / PT / ML / Frag, drops the track ids whose
// pair column is zero over those rows (a block-wide column scan), solves the identity assignment with the solver's state in the
// workspace (global memory: 1024 x 4097 does not fit the LDS) and clears what it read.
// Several streams: sequences are independent, so the stream is the grid.  Update: grid = S, and workgroup s walks the images s, s + S,
// ... of a frame-major batch (image f * S + s is the f-th frame of stream s, the tracker's layout in track.hip) on slice s of the state
// and of the workspace, the run totals included - no atomic is shared between streams, so stream s gets the single evaluator's
// result.  An image whose `active` word is 0 is no frame of its stream: no frame counter moves and its rows are not read (a stream
// that has ended keeps its place in the batch so; so does one without ground truth).  End: grid (nc, S), and the workgroups of a
// stream whose `ending` word is 0 return at once.  The workspace is S slices of the single size, each rounded up to 16 bytes; the LDS
// is per workgroup and unchanged.  The single entries are the same launchers with S = 1 and no masks.
#include "common.h"
#include "mot_rule.h"

#ifndef MOT_UPDATE_THREADS
#define MOT_UPDATE_THREADS 256
#endif
#define MOT_END_THREADS 256

enum { GS_LAST, GS_PRESENT, GS_MATCHED, GS_RUNS, GS_LASTF, GS_CLS };
enum { K_TP, K_FN, K_FP, K_IDSW, K_GT, K_TRK, K_FRAG, K_MT, K_PT, K_ML, K_IDTP, K_GTIDS, K_DROP_REGION, K_DROP_DISTRACTOR };
enum { H_FRAME, H_OVER_GT, H_OVER_TRK, H_OVER_ROWS };

struct MotParams {
  const float* tracks;
  const int32_t* tcounts;
  const float* gt;
  const int32_t* gcounts;
  const int32_t* active;   // [B] or NULL: an image whose word is 0 is no frame of its stream
  int B, S, nq, ng, nc, G, T;
  double thr;
  int32_t* gstate;
  int32_t* counts;
  double* iou_sum;
  int32_t* pair;
  int32_t* hdr;
  unsigned char* ws;
  size_t ws_slice;   // bytes between the workspaces of two streams
};

static size_t mot_update_ws_bytes(size_t nq, size_t ng) { return mot_frame_ws_bytes(nq, ng) + 4 * nq; }   // the frame's block, then tm
static size_t mot_end_ws_per_class(size_t G, size_t T) { return ((4 * (2 * G + T) + 15) & ~(size_t)15) + mot_lsap_bytes(G, T + 1); }

__global__ __launch_bounds__(MOT_UPDATE_THREADS) void mot_update_kernel(MotParams q) {
  extern __shared__ __align__(16) unsigned char lds[];
  // workgroup s owns slice s of every state tensor and of the workspace, and the images s, s + S, ... of the batch
  const int s = blockIdx.x;
  MotParams p = q;
  p.gstate += (size_t)s * p.G * 8;
  p.counts += (size_t)s * p.nc * 16;
  p.iou_sum += (size_t)s * p.nc;
  p.pair += (size_t)s * p.G * p.T;
  p.hdr += (size_t)s * 8;
  p.ws += (size_t)s * p.ws_slice;
  __shared__ int wsum[(MOT_UPDATE_THREADS / WAVE)];
  __shared__ MotCand red[(MOT_UPDATE_THREADS / WAVE)];
  const int tid = threadIdx.x, nq = p.nq, ng = p.ng, nc = p.nc;
  const MotLsap w = mot_lsap_carve(lds, ng, nq + 1);
  const MotFrame f = mot_frame_carve(p.ws, nq, ng);
  double *iouM = f.iouM, *S = f.S;
  int *gl = f.gl, *g3 = f.g3, *xs = f.xs, *tl = f.tl, *t3 = f.t3;
  int* tm = reinterpret_cast<int*>(f.end);   // [m3] step 3's matched flags
  const double thr = p.thr;
  int fid = p.hdr[H_FRAME];

  for (int b = s; b < p.B; b += p.S) {
    if (p.active && p.active[b] == 0) continue;   // uniform: not a frame of this stream
    ++fid;
    const float* G = p.gt + (size_t)b * ng * 7;
    const float* Tr = p.tracks + (size_t)b * nq * 8;
    // ---- 1 and 2: regions and distractors; the drops are counted per class
    const MotFrameSets fs = mot_frame_filter<MOT_UPDATE_THREADS, true>(
        G, Tr, p.gcounts[b], p.tcounts[b], ng, nq, nc, p.G, p.T, thr, &p.hdr[H_OVER_GT], f, w, red, wsum,
        [&](const float* t) { atomicAdd(&p.counts[(int)t[6] * 16 + K_DROP_REGION], 1); },
        [&](const float* t) { atomicAdd(&p.counts[(int)t[6] * 16 + K_DROP_DISTRACTOR], 1); });
    const int ntl = fs.ntl, n3 = fs.n3, m3 = fs.m3;
    // either branch of step 3 passes a barrier between these stores and its writes to tm
    for (int j = tid; j < m3; j += MOT_UPDATE_THREADS) tm[j] = 0;
    // ---- 3. CLEAR matching, all classes in one block-diagonal assignment
    auto qualifies = [&](int a, int c2, double& v) -> bool {
      const int i = g3[a], j = t3[c2];
      v = iouM[(size_t)i * ntl + j];
      return v >= thr && (int)G[(size_t)gl[i] * 7 + 5] == (int)Tr[(size_t)tl[j] * 8 + 6];
    };
    auto cost3 = [&](int a, int c2) -> double {
      double v;
      if (!qualifies(a, c2, v)) return 0.0;
      const int gid = (int)G[(size_t)gl[g3[a]] * 7 + 4], trk = (int)Tr[(size_t)tl[t3[c2]] * 8 + 4];
      return p.gstate[(size_t)gid * 8 + GS_LAST] == trk + 1 ? -(v + 1000.0) : -v;
    };
    if (n3 > 0 && m3 > 0) {
      for (int e = tid; e < n3 * m3; e += MOT_UPDATE_THREADS) S[e] = cost3(e / m3, e % m3);
      __syncthreads();
      mot_assign_sparse<MOT_UPDATE_THREADS>(S, n3, m3, w, f.sq, xs, red, wsum);
    } else {
      for (int a = tid; a < n3; a += MOT_UPDATE_THREADS) xs[a] = -1;
      __syncthreads();
    }
    for (int a = tid; a < n3; a += MOT_UPDATE_THREADS) {
      const float* g = G + (size_t)gl[g3[a]] * 7;
      const int c = (int)g[5];
      int32_t* gs = p.gstate + (size_t)(int)g[4] * 8;
      int32_t* cn = p.counts + c * 16;
      atomicAdd(&cn[K_GT], 1);
      gs[GS_PRESENT] += 1;
      gs[GS_CLS] = c + 1;
      const int j = xs[a];
      double v = 0.0;
      if (j >= 0 && S[(size_t)a * m3 + j] < 0.0 && qualifies(a, j, v)) {
        const int trk = (int)Tr[(size_t)tl[t3[j]] * 8 + 4];
        tm[j] = 1;
        atomicAdd(&cn[K_TP], 1);
        atomicAdd(&p.iou_sum[c], v);
        if (gs[GS_LAST] != 0 && gs[GS_LAST] != trk + 1) atomicAdd(&cn[K_IDSW], 1);
        gs[GS_LAST] = trk + 1;
        if (gs[GS_MATCHED] == 0 || gs[GS_LASTF] != fid - 1) gs[GS_RUNS] += 1;
        gs[GS_MATCHED] += 1;
        gs[GS_LASTF] = fid;
      } else {
        atomicAdd(&cn[K_FN], 1);
      }
    }
    __syncthreads();
    for (int c2 = tid; c2 < m3; c2 += MOT_UPDATE_THREADS) {
      int32_t* cn = p.counts + (int)Tr[(size_t)tl[t3[c2]] * 8 + 6] * 16;
      atomicAdd(&cn[K_TRK], 1);
      if (!tm[c2]) atomicAdd(&cn[K_FP], 1);
    }
    // ---- 4. pair counts
    for (int e = tid; e < n3 * m3; e += MOT_UPDATE_THREADS) {
      const int a = e / m3, c2 = e - a * m3;
      if (S[e] < 0.0) {   // the pair qualifies
        const int gid = (int)G[(size_t)gl[g3[a]] * 7 + 4], trk = (int)Tr[(size_t)tl[t3[c2]] * 8 + 4];
        atomicAdd(&p.pair[(size_t)gid * p.T + trk], 1);
      }
    }
    __syncthreads();
  }
  if (tid == 0) p.hdr[H_FRAME] = fid;
}

struct MotEndParams {
  int nc, G, T, G_used;
  const int32_t* ending;    // [S] or NULL: the workgroups of a stream whose word is 0 return at once
  const int32_t* gt_used;   // [S] or NULL: G_used per stream
  int32_t* gstate;
  int32_t* counts;
  int32_t* pair;
  int32_t* hdr;
  unsigned char* ws;
  size_t per_class, ws_slice;
};

__global__ __launch_bounds__(MOT_END_THREADS) void mot_end_kernel(MotEndParams q) {
  __shared__ int wsum[(MOT_END_THREADS / WAVE)];
  __shared__ MotCand red[(MOT_END_THREADS / WAVE)];
  const int tid = threadIdx.x, c = blockIdx.x, s = blockIdx.y, T = q.T;
  if (q.ending && q.ending[s] == 0) return;
  MotEndParams p = q;
  p.gstate += (size_t)s * p.G * 8;
  p.counts += (size_t)s * p.nc * 16;
  p.pair += (size_t)s * p.G * p.T;
  p.hdr += (size_t)s * 8;
  if (p.gt_used) p.G_used = max(p.gt_used[s], 0);
  unsigned char* base = p.ws + (size_t)s * p.ws_slice + (size_t)c * p.per_class;
  int* rows = reinterpret_cast<int*>(base);
  int *x = rows + p.G, *cols = x + p.G;
  const MotLsap w = mot_lsap_carve(base + ((4 * (2 * (size_t)p.G + T) + 15) & ~(size_t)15), p.G, T + 1);
  int32_t* cn = p.counts + c * 16;
  if (c == 0 && tid == 0) p.hdr[H_FRAME] = 0;
  const int n = mot_compact<MOT_END_THREADS>(min(p.G_used, p.G), rows, wsum, [&](int g) { return p.gstate[(size_t)g * 8 + GS_CLS] == c + 1; });
  if (n == 0) return;
  for (int a = tid; a < n; a += MOT_END_THREADS) {
    const int32_t* gs = p.gstate + (size_t)rows[a] * 8;
    const double ratio = (double)gs[GS_MATCHED] / (double)gs[GS_PRESENT];
    atomicAdd(&cn[ratio > 0.8 ? K_MT : ratio < 0.2 ? K_ML : K_PT], 1);
    atomicAdd(&cn[K_GTIDS], 1);
    if (gs[GS_RUNS] > 1) atomicAdd(&cn[K_FRAG], gs[GS_RUNS] - 1);
  }
  // the track ids some gt of the class met
  const int m = mot_compact<MOT_END_THREADS>(T, cols, wsum, [&](int t) {
    for (int a = 0; a < n; ++a)
      if (p.pair[(size_t)rows[a] * T + t]) return true;
    return false;
  });
  if (m > 0) {
    auto cost = [&](int a, int j) -> double { return -(double)p.pair[(size_t)rows[a] * T + cols[j]]; };
    mot_assign<MOT_END_THREADS>(cost, n, m, 0.0, w, x, red);
    int idtp = 0;
    for (int a = tid; a < n; a += MOT_END_THREADS)
      if (x[a] >= 0) idtp += p.pair[(size_t)rows[a] * T + cols[x[a]]];
    if (idtp) atomicAdd(&cn[K_IDTP], idtp);
    __syncthreads();
  }
  // clear what this class used
  for (size_t e = tid; e < (size_t)n * T; e += MOT_END_THREADS) p.pair[(size_t)rows[e / T] * T + e % T] = 0;
  for (int e = tid; e < n * 8; e += MOT_END_THREADS) p.gstate[(size_t)rows[e >> 3] * 8 + (e & 7)] = 0;
}

extern "C" int tamtr_mot_workspace_bytes(int nq, int ng, int nc, int G_cap, int T_cap) {
  if (nq < 1 || ng < 1 || nc < 1 || G_cap < 1 || T_cap < 1) return 0;
  const size_t a = mot_update_ws_bytes(nq, ng), b = (size_t)nc * mot_end_ws_per_class(G_cap, T_cap);
  const size_t n = (a > b ? a : b) + 16;
  return n > 0x7fffffff ? 0 : (int)n;
}

static bool mot_unsupported(int nq, int ng, int nc, int G, int T) {
  return tamtr_mot_workspace_bytes(nq, ng, nc, G, T) == 0 || mot_lsap_bytes(ng, (size_t)nq + 1) > 60 * 1024 || (size_t)G * T > 0x7fffffff ||
         G > (1 << 24) || T > (1 << 24) || nc > (1 << 16);   // ids travel as fp32
}

// S stacked evaluators: each stream's slice of the workspace is the single size rounded up to 16 bytes
static size_t mot_ws_slice(int nq, int ng, int nc, int G, int T) { return ((size_t)tamtr_mot_workspace_bytes(nq, ng, nc, G, T) + 15) & ~(size_t)15; }

extern "C" int tamtr_mot_streams_workspace_bytes(int S, int nq, int ng, int nc, int G_cap, int T_cap) {
  if (S < 1 || tamtr_mot_workspace_bytes(nq, ng, nc, G_cap, T_cap) == 0) return 0;
  const size_t slice = mot_ws_slice(nq, ng, nc, G_cap, T_cap);
  return slice > (size_t)0x7fffffff / S ? 0 : (int)(S * slice);
}

static bool mot_streams_unsupported(int S, int nq, int ng, int nc, int G, int T) {
  return mot_unsupported(nq, ng, nc, G, T) || S > 65535 || tamtr_mot_streams_workspace_bytes(S, nq, ng, nc, G, T) == 0;
}

// The one place mot_update_kernel is launched from; tamtr_mot_update is S = 1 without a mask.  The last stream's slice need not be
// rounded up, so with S = 1 the workspace asked for is the single entry's.
extern "C" int tamtr_mot_update_streams(const float* tracks, const int32_t* tcounts, const float* gt, const int32_t* gcounts, int B, int S, int nq,
                                        int ng, int nc, double iou_thr, const int32_t* active, int32_t* gstate, int32_t* counts, double* iou_sum,
                                        int32_t* pair, int32_t* hdr, int G_cap, int T_cap, void* workspace, int workspace_bytes, void* stream) {
  if (!tracks || !tcounts || !gt || !gcounts || !gstate || !counts || !iou_sum || !pair || !hdr || !workspace || B < 1 || nq < 1 || ng < 1 ||
      nc < 1 || G_cap < 1 || T_cap < 1 || !(iou_thr > 0.0) || ((uintptr_t)workspace & 15) || S < 1 || B % S != 0)
    return TAMTR_EINVAL;
  if (mot_streams_unsupported(S, nq, ng, nc, G_cap, T_cap)) return TAMTR_EUNSUP;
  const size_t slice = mot_ws_slice(nq, ng, nc, G_cap, T_cap);
  if (workspace_bytes < 0 || (size_t)workspace_bytes < (S - 1) * slice + (size_t)tamtr_mot_workspace_bytes(nq, ng, nc, G_cap, T_cap)) return TAMTR_EINVAL;
  MotParams p{tracks, tcounts, gt, gcounts, active, B, S, nq, ng, nc, G_cap, T_cap, iou_thr, gstate, counts, iou_sum, pair, hdr,
              static_cast<unsigned char*>(workspace), slice};
  hipLaunchKernelGGL(mot_update_kernel, dim3(S), dim3(MOT_UPDATE_THREADS), mot_lsap_bytes(ng, (size_t)nq + 1), (hipStream_t)stream, p);
  return tamtr_launch_status();
}

extern "C" int tamtr_mot_update(const float* tracks, const int32_t* tcounts, const float* gt, const int32_t* gcounts, int B, int nq, int ng,
                                int nc, double iou_thr, int32_t* gstate, int32_t* counts, double* iou_sum, int32_t* pair, int32_t* hdr,
                                int G_cap, int T_cap, void* workspace, int workspace_bytes, void* stream) {
  return tamtr_mot_update_streams(tracks, tcounts, gt, gcounts, B, 1, nq, ng, nc, iou_thr, nullptr, gstate, counts, iou_sum, pair, hdr, G_cap, T_cap,
                                  workspace, workspace_bytes, stream);
}

// The one place mot_end_kernel is launched from: grid (nc, S).  gt_used NULL: G_used for every stream (the single entry).
static int mot_end_launch(int nc, int S, const int32_t* ending, const int32_t* gt_used, int G_used, int32_t* gstate, int32_t* counts, int32_t* pair,
                          int32_t* hdr, int G_cap, int T_cap, void* workspace, int workspace_bytes, void* stream) {
  if (!gstate || !counts || !pair || !hdr || !workspace || nc < 1 || G_cap < 1 || T_cap < 1 || G_used < 0 || ((uintptr_t)workspace & 15) || S < 1)
    return TAMTR_EINVAL;
  if (mot_streams_unsupported(S, 1, 1, nc, G_cap, T_cap)) return TAMTR_EUNSUP;
  const size_t slice = mot_ws_slice(1, 1, nc, G_cap, T_cap);
  if (workspace_bytes < 0 || (size_t)workspace_bytes < (S - 1) * slice + (size_t)nc * mot_end_ws_per_class(G_cap, T_cap)) return TAMTR_EINVAL;
  MotEndParams p{nc, G_cap, T_cap, G_used, ending, gt_used, gstate, counts, pair, hdr, static_cast<unsigned char*>(workspace),
                 mot_end_ws_per_class(G_cap, T_cap), slice};
  hipLaunchKernelGGL(mot_end_kernel, dim3(nc, S), dim3(MOT_END_THREADS), 0, (hipStream_t)stream, p);
  return tamtr_launch_status();
}

extern "C" int tamtr_mot_end_sequence(int nc, int32_t* gstate, int32_t* counts, int32_t* pair, int32_t* hdr, int G_cap, int T_cap, int G_used,
                                      void* workspace, int workspace_bytes, void* stream) {
  return mot_end_launch(nc, 1, nullptr, nullptr, G_used, gstate, counts, pair, hdr, G_cap, T_cap, workspace, workspace_bytes, stream);
}

extern "C" int tamtr_mot_end_streams(int nc, int S, const int32_t* ending, const int32_t* gt_used, int32_t* gstate, int32_t* counts, int32_t* pair,
                                     int32_t* hdr, int G_cap, int T_cap, void* workspace, int workspace_bytes, void* stream) {
  if (!gt_used) return TAMTR_EINVAL;
  return mot_end_launch(nc, S, ending, gt_used, 0, gstate, counts, pair, hdr, G_cap, T_cap, workspace, workspace_bytes, stream);
}
