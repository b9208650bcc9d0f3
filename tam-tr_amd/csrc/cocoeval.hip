// cocoeval.hip - COCO-protocol bbox evaluation on the device: the per-image matching of a whole batch in one launch
// (tamtr_val_coco_match) and the accumulation of a whole run in one launch (tamtr_val_coco_accumulate).
//
// Replaces the step the reference leaves to pycocotools: valTAMTR.py:15 sets save_json=True "if you need to cal coco metrice",
// dataset/yolo2coco.py builds the annotation file and requirements.txt:44 lists pycocotools for "COCO mAP"; COCOeval then matches per image
// and category in Python loops and accumulates with numpy.  Here the kernels read what tamtr_val_postprocess_match left on the device
// (predn, counts) and the same grouped labels tamtr_val_confusion reads.  The checker is engine.coco_evaluate (numpy, the same rule).
//
// The rule (COCO bbox protocol, iscrowd = 0 throughout; every image of the run is evaluated, also one without labels).
//   inputs   per image the live rows of predn (row < counts[b]; x1 y1 x2 y2 score cls), already in descending score order with equal
//            scores in query order (valmatch.hip's stable order, which a mergesort on -score keeps), and the image's labels converted
//            as valmatch.hip step 6 / confusion.hip: xywh -> xyxy on the normalised fp32 values, then x *= fp32(w_orig), y *= fp32(h_orig).
//            Classes truncate towards zero as `.int()`.  A row or label whose class is outside [0, nc) (or NaN) and a row whose score is
//            NaN take part in nothing.
//   fp64     every operation below is fp64 on the fp32 corners widened to fp64 (the object is compiled with -ffp-contract=off):
//            w = x2 - x1, h = y2 - y1, area = w * h;  iw = min(x2) - max(x1), ih likewise;  IoU = 0 when iw <= 0 or ih <= 0, else
//            i = iw * ih, u = (area_d + area_g) - i, IoU = u <= 0 ? 0 : i / u.  No eps.  A NaN IoU never qualifies.
//   T, R     T = numpy's linspace(0.5, 0.95, 10), R = numpy's linspace(0, 1, 101): operands, not recomputed.
//   ranges   a = 0..3: [0, 1e10], [0, 32^2], [32^2, 96^2], [96^2, 1e10], inclusive at both ends; outside(area, a) = area < lo or area > hi.
//   max_dets ascending, at most 4 entries; D = the last one.
//   matching per image, category, range a and threshold t (the 40 (t, a) problems are independent):
//     1. ground truths of the category: ignore[g] = outside(area_g, a); order: non-ignored first, file order inside each group.
//     2. detections of the category: the first D in score order (rank < D).  Later ones take part in nothing and consume nothing.
//     3. per detection in order: best = min(T[t], 1 - 1e-10), m = none; walk the ground truths in the order of 1.; skip a matched one;
//        stop when m is a non-ignored one and the walk reaches an ignored one; skip when iou < best; else best = iou, m = g.
//        So IoU == threshold matches, the LATER ground truth wins among equal IoUs, and an ignored one is only taken when no
//        non-ignored one qualifies: m = the arg-max of (non-ignored, IoU, position) over the unmatched ones with IoU >= best.
//        A matched detection takes ignore[m]; m is then taken, ignored or not.
//     4. an unmatched detection whose own area is outside the range is ignored.
//   npig[k, a] = the number of non-ignored ground truths of category k in range a over the run.
//   accumulation per category k, range a, cut M in max_dets, threshold t: the rows of k with rank < M, score descending, equal scores in
//     image order then row order (the caller sorts: two stable sorts, as for metrics.hip).  npig == 0: every entry is -1.  Otherwise
//     tp / fp = inclusive counts of matched / unmatched rows that are not ignored (ignored rows advance neither);
//     rc = tp / npig;  pr = tp / ((fp + tp) + 2.220446049250313e-16);  pr becomes its suffix maximum;
//     precision[t, r, k, a, M] = pr[i] at the first row i with rc[i] >= R[r] (searchsorted left), 0 when there is none;
//     recall[t, k, a, M] = the last rc, 0 with no rows;  ap_tkam[t, k, a, M] = (sum_r precision, serial in r) / 101, or -1.
//
// Design of the match kernel: one workgroup of 8 waves per image, nq <= 512.
//   a.  setup by the whole workgroup.  Thread d owns row d: class, rank among the live rows of its class (a count over the rows
//       before it), box to LDS.  Labels are ranked by (class, file index) with a counting pass - position = the number of labels that
//       sort before - so there is no cap on nc and none on labels; per range, a second counting pass over the label's class segment
//       gives its place in "non-ignored first, file order".  Every in-range label adds 1 to npig[k, a] where it is not ignored
//       (integer atomics: order-free, as the confusion matrix).  Each row finds its class segment by binary search.
//   b.  the label table (boxes, the four orders, the matched planes, the sorted classes) lives in LDS when the image has at most
//       CE_TILE = 512 labels and in the caller's workspace otherwise (44 bytes per label of the batch): one code path through flat
//       pointers.
//   c.  wave w owns range a = w & 3 and the five thresholds 5 * (w >> 2) ...; it walks the detections serially with NO workgroup
//       barrier.  Its lanes stride over the ground truths of the detection's class in the range's order, recompute the IoU (cheaper
//       than sharing it) and keep per threshold the lane's best (key, position), key = IoU bits | non-ignored << 63 - IoU is
//       positive, so unsigned order on the key is the order on (non-ignored, IoU); a lane walks ascending positions and replaces on >=,
//       the "later wins" rule.  The wave's arg-max is a ballot and a scalar walk over the (few) lanes that have a candidate, again
//       with "equal key: the later position".  The matched bits of position j are read and written only by lane j & 63 of the one
//       wave that owns the plane, so program order is all the ordering they need.
//   d.  each wave leaves (matched bits | ignored bits << 16) for its five thresholds in LDS; after one barrier thread d merges the two
//       halves per range and stores the row's four words and its rank.
//
// Design of the accumulate kernel: one workgroup of 256 threads per (k, a, M, t); no atomics and no floating-point reduction whose
// order could vary, so two runs give the same bits.
//   a.  forward over the class segment in tiles of 256 rows: the total tp (integer).
//   b.  backward over the tiles: exclusive suffix counts of tp and fp flags with carries give every row's inclusive tp and fp as
//       total - suffix; pr and its suffix maximum (wave scan, wave maxima in LDS, the carry of the tiles after; max is exact).
//       A row of rank >= M is handled as an ignored row: it repeats its predecessor's (tp, fp), which changes neither a suffix maximum
//       (pr >= 0) nor a first-row-reaching-a-recall.
//   c.  the 101 picks need no stored curve: rc is a step function of tp, so row i is "the first row with rc >= R[r]" exactly for the
//       r with rc[i - 1] < R[r] <= rc[i] (row 0: R[r] <= rc[0]); the thread that owns such a row binary-searches R and writes its
//       envelope value for that range of r into LDS.  At most 101 writes per workgroup; uncovered r keep 0.
//   d.  thread 0 sums the 101 values in grid order; the first 101 threads store them.
#include "common.h"

#define CE_THREADS 512
#define CE_WAVES (CE_THREADS / WAVE)
#define CE_MAX_Q 512
#define CE_TILE 512      // labels of one image that fit the LDS table
#define CE_T 10
#define CE_R 101
#define CE_A 4
#define CE_WS_PER_LABEL 44   // box 16 + order 4 * 4 + matched planes 8 + sorted class 4

#define ACC_TILE 256

__device__ __forceinline__ int ce_class(float c, int nc) {
  const float t = truncf(c);
  return (t >= 0.0f && t < (float)nc) ? (int)t : -1;
}

__device__ __forceinline__ int ce_outside(double area) {   // bit a = outside range a
  const double s2 = 1024.0, m2 = 9216.0, big = 1e10;
  int o = 0;
  if (area < 0.0 || area > big) o |= 1;
  if (area < 0.0 || area > s2) o |= 2;
  if (area < s2 || area > m2) o |= 4;
  if (area < m2 || area > big) o |= 8;
  return o;
}

struct CeShared {
  float4 lbox[CE_TILE];            // label boxes in (class, file index) order
  int ord[CE_A][CE_TILE];          // per range: position -> index into lbox | ignored << 31
  uint8_t mt[CE_WAVES][CE_TILE];   // per wave: matched bits of its five thresholds, by position in the range's order
  int scls[CE_TILE];               // sorted label classes (nc = out of range, at the end)
  float4 dbox[CE_MAX_Q];
  int dcls[CE_MAX_Q];              // class, -1: takes part in nothing
  int4 dmeta[CE_MAX_Q];            // class, rank, first label (sorted position) of the row's class, labels of the row's class
  uint32_t res[CE_WAVES][CE_MAX_Q];
};

__global__ __launch_bounds__(CE_THREADS) void val_coco_match_kernel(const float* __restrict__ predn, const int32_t* __restrict__ counts, int nq,
                                                                    int nc, const float* __restrict__ lab_cls,
                                                                    const float* __restrict__ lab_box, const int32_t* __restrict__ lab_off,
                                                                    int M, const float* __restrict__ scale, const double* __restrict__ thr,
                                                                    int max_det, int32_t* __restrict__ bits, int32_t* __restrict__ rank,
                                                                    int32_t* __restrict__ npig, uint8_t* __restrict__ ws) {
  __shared__ CeShared s;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;

  int npr = counts[b];
  npr = npr < 0 ? 0 : (npr > nq ? nq : npr);
  int l0 = lab_off[b], l1 = lab_off[b + 1];
  l0 = l0 < 0 ? 0 : (l0 > M ? M : l0);
  l1 = l1 < l0 ? l0 : (l1 > M ? M : l1);
  const int nl = l1 - l0;

  // ---- b. where the label table lives
  float4* lbox;
  int* ord;
  uint8_t* mt;
  int* scls;
  int ostride;
  if (nl <= CE_TILE) {
    lbox = s.lbox; ord = &s.ord[0][0]; mt = &s.mt[0][0]; scls = s.scls; ostride = CE_TILE;
  } else {
    lbox = reinterpret_cast<float4*>(ws) + l0;
    ord = reinterpret_cast<int*>(ws + (size_t)16 * M) + l0;
    mt = ws + (size_t)32 * M + l0;
    scls = reinterpret_cast<int*>(ws + (size_t)40 * M) + l0;
    ostride = M;
  }

  // ---- a. rows: class, box
  int dcl = -1;
  if (tid < npr) {
    const float* r = predn + ((size_t)b * nq + tid) * 6;
    s.dbox[tid] = make_float4(r[0], r[1], r[2], r[3]);
    if (r[4] == r[4]) dcl = ce_class(r[5], nc);
  }
  if (tid < CE_MAX_Q) s.dcls[tid] = dcl;

  // labels: position in (class, file index) order by counting
  const float lw = scale[4 * b + 2], lh = scale[4 * b + 3];
  for (int i = tid; i < nl; i += CE_THREADS) {
    int ci = ce_class(lab_cls[l0 + i], nc);
    if (ci < 0) ci = nc;
    int pos = 0;
    for (int j = 0; j < nl; ++j) {
      int cj = ce_class(lab_cls[l0 + j], nc);
      if (cj < 0) cj = nc;
      pos += (cj < ci || (cj == ci && j < i)) ? 1 : 0;
    }
    const float* lb = lab_box + (size_t)(l0 + i) * 4;
    const float cx = lb[0], cy = lb[1], hw = lb[2] / 2.0f, hh = lb[3] / 2.0f;
    lbox[pos] = make_float4((cx - hw) * lw, (cy - hh) * lh, (cx + hw) * lw, (cy + hh) * lh);
    scls[pos] = ci;
    for (int w = 0; w < CE_WAVES; ++w) mt[(size_t)w * ostride + i] = 0;
  }
  __threadfence_block();
  __syncthreads();

  // per range: the label's place in "non-ignored first, file order" inside its class segment
  for (int p = tid; p < nl; p += CE_THREADS) {
    const int c = scls[p];
    if (c >= nc) continue;
    const float4 g = lbox[p];
    const int mine = ce_outside(((double)g.z - (double)g.x) * ((double)g.w - (double)g.y));
    int before[CE_A] = {0, 0, 0, 0}, total[CE_A] = {0, 0, 0, 0}, ign_before[CE_A] = {0, 0, 0, 0};
    int q = p;
    while (q > 0 && scls[q - 1] == c) --q;          // segment start
    for (; q < nl && scls[q] == c; ++q) {
      const float4 e = lbox[q];
      const int o = ce_outside(((double)e.z - (double)e.x) * ((double)e.w - (double)e.y));
#pragma unroll
      for (int a = 0; a < CE_A; ++a) {
        const int ig = (o >> a) & 1;
        total[a] += 1 - ig;
        if (q < p) { before[a] += 1 - ig; ign_before[a] += ig; }
      }
    }
#pragma unroll
    for (int a = 0; a < CE_A; ++a) {
      const int ig = (mine >> a) & 1;
      const int place = ig ? total[a] + ign_before[a] : before[a];
      // position `place` of the segment, which starts at p - (before + ign_before)
      const int seg0 = p - (before[a] + ign_before[a]);
      ord[(size_t)a * ostride + seg0 + place] = p | (ig << 31);
      if (!ig) atomicAdd(npig + (size_t)c * CE_A + a, 1);
    }
  }

  // rows: rank in class, class segment
  int rk = -1, seg = 0, cnt = 0;
  if (dcl >= 0) {
    rk = 0;
    for (int e = 0; e < tid; ++e) rk += s.dcls[e] == dcl ? 1 : 0;
    int lo = 0, hi = nl;                           // first position with scls >= dcl
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (scls[mid] < dcl) lo = mid + 1; else hi = mid; }
    seg = lo;
    hi = nl;                                       // first position with scls > dcl
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (scls[mid] <= dcl) lo = mid + 1; else hi = mid; }
    cnt = lo - seg;
  }
  s.dmeta[tid] = make_int4(dcl, rk, seg, cnt);
  __threadfence_block();
  __syncthreads();

  // ---- c. the wave's five (t, a) problems over the detections, serially, no workgroup barrier
  const int a = wave & 3, t0 = (wave >> 2) * 5;
  double T[5];
#pragma unroll
  for (int u = 0; u < 5; ++u) { const double t = thr[t0 + u]; T[u] = t < 1.0 - 1e-10 ? t : 1.0 - 1e-10; }
  const int* aord = ord + (size_t)a * ostride;
  uint8_t* amt = mt + (size_t)wave * ostride;
  for (int d = 0; d < npr; ++d) {
    uint32_t word = 0;
    const int4 meta = s.dmeta[d];
    if (meta.x >= 0 && meta.y < max_det) {
      const float4 db = s.dbox[d];
      const double dx1 = db.x, dy1 = db.y, dx2 = db.z, dy2 = db.w;
      const double darea = (dx2 - dx1) * (dy2 - dy1);
      const int s0 = meta.z, n = meta.w;
      unsigned long long bkey[5] = {0, 0, 0, 0, 0};
      int bj[5] = {0, 0, 0, 0, 0};
      for (int j = lane; j < n; j += WAVE) {
        const int o = aord[s0 + j];
        const float4 g = lbox[o & 0x7fffffff];
        const double gx1 = g.x, gy1 = g.y, gx2 = g.z, gy2 = g.w;
        const double iw = (dx2 < gx2 ? dx2 : gx2) - (dx1 > gx1 ? dx1 : gx1), ih = (dy2 < gy2 ? dy2 : gy2) - (dy1 > gy1 ? dy1 : gy1);
        if (!(iw > 0.0 && ih > 0.0)) continue;
        const double inter = iw * ih;
        const double uni = (darea + (gx2 - gx1) * (gy2 - gy1)) - inter;
        if (!(uni > 0.0)) continue;
        const double iou = inter / uni;
        if (!(iou >= T[0])) continue;
        const uint32_t taken = amt[s0 + j];
        const unsigned long long key = (unsigned long long)__double_as_longlong(iou) | (o < 0 ? 0ull : 0x8000000000000000ull);
#pragma unroll
        for (int u = 0; u < 5; ++u)
          if (iou >= T[u] && !((taken >> u) & 1u) && key >= bkey[u]) { bkey[u] = key; bj[u] = j; }
      }
      uint32_t mbits = 0, ibits = 0;
      if (__ballot((bkey[0] | bkey[1] | bkey[2] | bkey[3] | bkey[4]) != 0ull) != 0ull) {   // most rows: no ground truth in reach
#pragma unroll
        for (int u = 0; u < 5; ++u) {
          unsigned long long cand = __ballot(bkey[u] != 0ull);
          if (cand == 0ull) continue;
          unsigned long long wkey = 0ull;
          int wj = -1;
          while (cand) {                      // scalar walk: the lane index is wave-uniform, the reads are v_readlane
            const int l = __builtin_ctzll(cand);
            cand &= cand - 1;
            const uint32_t klo = __builtin_amdgcn_readlane((uint32_t)bkey[u], l), khi = __builtin_amdgcn_readlane((uint32_t)(bkey[u] >> 32), l);
            const int jj = __builtin_amdgcn_readlane(bj[u], l);
            const unsigned long long k = ((unsigned long long)khi << 32) | klo;
            if (k > wkey || (k == wkey && jj > wj)) { wkey = k; wj = jj; }
          }
          if (lane == (wj & (WAVE - 1))) amt[s0 + wj] |= (uint8_t)(1u << u);
          mbits |= 1u << u;
          if (!(wkey >> 63)) ibits |= 1u << u;
        }
      }
      if ((ce_outside(darea) >> a) & 1) ibits |= ~mbits & 31u;
      word = (mbits << t0) | (ibits << (16 + t0));
    }
    if (lane == 0) s.res[wave][d] = word;
  }
  __syncthreads();

  // ---- d. the row's four words and its rank
  if (tid < nq) {
    int4 w = make_int4(0, 0, 0, 0);
    if (tid < npr) {
      w.x = (int)(s.res[0][tid] | s.res[4][tid]);
      w.y = (int)(s.res[1][tid] | s.res[5][tid]);
      w.z = (int)(s.res[2][tid] | s.res[6][tid]);
      w.w = (int)(s.res[3][tid] | s.res[7][tid]);
    }
    *reinterpret_cast<int4*>(bits + ((size_t)b * nq + tid) * 4) = w;
    rank[(size_t)b * nq + tid] = rk;
  }
}

extern "C" int tamtr_val_coco_workspace_bytes(int B, int nq, int M) {
  if (B < 1 || nq < 1 || M < 0 || nq > CE_MAX_Q) return 0;
  if ((long long)M * CE_WS_PER_LABEL + 16 > 0x7fffffffLL) return 0;
  return M * CE_WS_PER_LABEL + 16;   // never 0 for a supported shape
}

static inline bool ce_misaligned(const void* p, size_t al) { return ((uintptr_t)p & (al - 1)) != 0; }

extern "C" int tamtr_val_coco_match(const float* predn, const int32_t* counts, int B, int nq, int nc, const float* lab_cls,
                                    const float* lab_box, const int32_t* lab_off, int M, const float* scale, const double* thresholds,
                                    int max_det, int32_t* bits, int32_t* rank, int32_t* npig, void* workspace, int workspace_bytes,
                                    void* stream) {
  if (!predn || !counts || !lab_off || !scale || !thresholds || !bits || !rank || !npig || !workspace || B < 1 || nq < 1 || nc < 1 || M < 0 ||
      max_det < 1)
    return TAMTR_EINVAL;
  if (M > 0 && (!lab_cls || !lab_box)) return TAMTR_EINVAL;
  if (ce_misaligned(thresholds, 8) || ce_misaligned(bits, 16) || ce_misaligned(workspace, 16) || ce_misaligned(rank, 4) || ce_misaligned(npig, 4))
    return TAMTR_EINVAL;
  if (nq > CE_MAX_Q) return TAMTR_EUNSUP;
  const int need = tamtr_val_coco_workspace_bytes(B, nq, M);
  if (need == 0) return TAMTR_EUNSUP;
  if (workspace_bytes < need) return TAMTR_EINVAL;
  hipLaunchKernelGGL(val_coco_match_kernel, dim3(B), dim3(CE_THREADS), 0, (hipStream_t)stream, predn, counts, nq, nc, lab_cls, lab_box, lab_off, M,
                     scale, thresholds, max_det, bits, rank, npig, (uint8_t*)workspace);
  return tamtr_launch_status();
}

// ------------------------------------------------------------------------------------------------ accumulation
struct AccShared {
  int isum[ACC_TILE / WAVE];
  int jsum[ACC_TILE / WAVE];
  double dmax[ACC_TILE / WAVE];
  double y[CE_R];
};

__global__ __launch_bounds__(ACC_TILE) void val_coco_accumulate_kernel(const int32_t* __restrict__ bits, const int32_t* __restrict__ rank,
                                                                       const int32_t* __restrict__ seg_off, int N, int nc,
                                                                       const int32_t* __restrict__ npig, const int32_t* __restrict__ max_dets,
                                                                       int n_m, const double* __restrict__ grid, double* __restrict__ precision,
                                                                       double* __restrict__ recall, double* __restrict__ ap_tkam) {
  __shared__ AccShared s;
  constexpr int NW = ACC_TILE / WAVE;
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
  int id = blockIdx.x;
  const int t = id % CE_T; id /= CE_T;
  const int m = id % n_m; id /= n_m;
  const int a = id % CE_A;
  const int k = id / CE_A;
  const size_t o_tkam = (((size_t)t * nc + k) * CE_A + a) * n_m + m;
  const size_t p_stride = (size_t)nc * CE_A * n_m;                       // between consecutive r
  double* prec = precision + (size_t)t * CE_R * p_stride + ((size_t)k * CE_A + a) * n_m + m;

  const int np = npig[(size_t)k * CE_A + a];
  if (np <= 0) {
    for (int r = tid; r < CE_R; r += ACC_TILE) prec[(size_t)r * p_stride] = -1.0;
    if (tid == 0) { recall[o_tkam] = -1.0; ap_tkam[o_tkam] = -1.0; }
    return;
  }
  int s0 = seg_off[k], s1 = seg_off[k + 1];
  s0 = s0 < 0 ? 0 : (s0 > N ? N : s0);
  s1 = s1 < s0 ? s0 : (s1 > N ? N : s1);
  const int n = s1 - s0;
  const int cut = max_dets[m];
  const int32_t* wb = bits + (size_t)s0 * CE_A + a;
  const int32_t* rkp = rank + s0;
  const double dnp = (double)np;
  if (tid < CE_R) s.y[tid] = 0.0;

  // flags of row i: 1 = tp, 2 = fp, 0 = ignored or beyond the cut
  auto flags = [&](int i) -> int {
    if (i >= n) return 0;
    const int r = rkp[i];
    if (r < 0 || r >= cut) return 0;
    const uint32_t w = (uint32_t)wb[(size_t)i * CE_A];
    if ((w >> (16 + t)) & 1u) return 0;
    return ((w >> t) & 1u) ? 1 : 2;
  };

  // ---- a. forward: total tp and fp
  int ctp = 0, cfp = 0;
  for (int i = tid; i < n; i += ACC_TILE) { const int f = flags(i); ctp += f & 1; cfp += f >> 1; }
#pragma unroll
  for (int o = WAVE / 2; o > 0; o >>= 1) { ctp += __shfl_xor(ctp, o, WAVE); cfp += __shfl_xor(cfp, o, WAVE); }
  if (lane == 0) { s.isum[wave] = ctp; s.jsum[wave] = cfp; }
  __syncthreads();
  int tot_tp = 0, tot_fp = 0;
#pragma unroll
  for (int w = 0; w < NW; ++w) { tot_tp += s.isum[w]; tot_fp += s.jsum[w]; }
  __syncthreads();

  // ---- b. + c. backward: inclusive counts as total - suffix, precision, suffix maximum, the picks
  int after_tp = 0, after_fp = 0;     // flags of the tiles after this one
  double best = 0.0;                  // suffix maximum of the tiles after this one
  for (int i0 = n > 0 ? ((n - 1) / ACC_TILE) * ACC_TILE : -1; i0 >= 0; i0 -= ACC_TILE) {
    const int i = i0 + tid;
    const int f = flags(i);
    int vt = f & 1, vf = f >> 1;      // inclusive suffix counts inside the wave
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) {
      const int ot = __shfl_down(vt, d, WAVE), of = __shfl_down(vf, d, WAVE);
      if (lane + d < WAVE) { vt += ot; vf += of; }
    }
    if (lane == 0) { s.isum[wave] = vt; s.jsum[wave] = vf; }
    __syncthreads();
    int later_tp = after_tp, later_fp = after_fp, tile_tp = 0, tile_fp = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      const int x = s.isum[w], y = s.jsum[w];
      if (w > wave) { later_tp += x; later_fp += y; }
      tile_tp += x; tile_fp += y;
    }
    // rows strictly after i: the wave's inclusive suffix minus the row's own flag, plus later waves and tiles
    const int tp = tot_tp - (later_tp + vt - (f & 1)), fp = tot_fp - (later_fp + vf - (f >> 1));
    const double pr = i < n ? (double)tp / ((double)(fp + tp) + 2.220446049250313e-16) : 0.0;
    double v = pr;
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) {
      const double o = __shfl_down(v, d, WAVE);
      if (lane + d < WAVE) v = fmax(v, o);
    }
    if (lane == 0) s.dmax[wave] = v;
    __syncthreads();
    double later = best, tile_max = best;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      const double x = s.dmax[w];
      if (w > wave) later = fmax(later, x);
      tile_max = fmax(tile_max, x);
    }
    const double env = fmax(v, later);
    if (i < n && ((f & 1) || i == 0)) {
      const double rc = (double)tp / dnp;
      int r = 0;
      if (i > 0) {                                  // first r with R[r] > rc of the row before
        const double rc_prev = (double)(tp - 1) / dnp;
        int lo = 0, hi = CE_R;
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (grid[mid] <= rc_prev) lo = mid + 1; else hi = mid; }
        r = lo;
      }
      for (; r < CE_R && grid[r] <= rc; ++r) s.y[r] = env;
    }
    after_tp += tile_tp; after_fp += tile_fp;
    best = tile_max;
    __syncthreads();
  }

  // ---- d. outputs
  __syncthreads();
  if (tid < CE_R) prec[(size_t)tid * p_stride] = s.y[tid];
  if (tid == 0) {
    double sum = 0.0;
    for (int r = 0; r < CE_R; ++r) sum += s.y[r];
    ap_tkam[o_tkam] = sum / 101.0;
    recall[o_tkam] = n > 0 ? (double)tot_tp / dnp : 0.0;
  }
}

extern "C" int tamtr_val_coco_accumulate(const int32_t* bits, const int32_t* rank, const int32_t* seg_off, int N, int nc, const int32_t* npig,
                                         const int32_t* max_dets, int n_max_dets, const double* grid, double* precision, double* recall,
                                         double* ap_tkam, void* stream) {
  if (!bits || !rank || !seg_off || !npig || !max_dets || !grid || !precision || !recall || !ap_tkam || N < 1 || nc < 1) return TAMTR_EINVAL;
  if (n_max_dets < 1 || n_max_dets > 4) return TAMTR_EINVAL;
  if (ce_misaligned(bits, 4) || ce_misaligned(rank, 4) || ce_misaligned(seg_off, 4) || ce_misaligned(npig, 4) || ce_misaligned(max_dets, 4) ||
      ce_misaligned(grid, 8) || ce_misaligned(precision, 8) || ce_misaligned(recall, 8) || ce_misaligned(ap_tkam, 8))
    return TAMTR_EINVAL;
  if (nc > (1 << 16) || N > (1 << 30)) return TAMTR_EUNSUP;
  hipLaunchKernelGGL(val_coco_accumulate_kernel, dim3((unsigned)nc * CE_A * n_max_dets * CE_T), dim3(ACC_TILE), 0, (hipStream_t)stream, bits, rank,
                     seg_off, N, nc, npig, max_dets, n_max_dets, grid, precision, recall, ap_tkam);
  return tamtr_launch_status();
}
