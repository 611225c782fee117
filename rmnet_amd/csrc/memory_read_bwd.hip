// memory_read_bwd.hip -- gradients of the (regional) memory read for gfx950: include/rmnet_hip.h, rmnet_memory_read_backward_f32.
//
// Per object, with M = T h w memory cells and N = h w queries, mm / qm the 0/1 maps of the cell rectangles (memory_read.hip's
// header: "as if multiplied by 0"), Km = K mm, Vm = V mm, Qm = Q qm:
//     S = Km^T Qm / sqrt(De)   [M, N]        P = soft-max of S over the M cells (a masked cell stays in it with logit 0)
//     R = Vm P                               mem_val = cat(R, q_val qm)
// and, with G = d mem_val[:Do], G2 = d mem_val[Do:]:
//     d q_val = G2 qm          delta_n = sum_d G[d, n] R[d, n]          dP = Vm^T G          dS = P o (dP - delta)
//     d V = (G P^T) mm         d K = (Qm dS^T / sqrt(De)) mm            d Q = (Km dS / sqrt(De)) qm
//
// Like the forward, nothing here touches a masked cell:
//   * a masked MEMORY cell gets no gradient (a zero is written) and feeds none; it counts in every query's soft-max maximum
//     (logit 0) and denominator (c exp(0 - max) for the c masked cells of the object, added once per query in mrb_stats);
//   * a masked QUERY has P = 1 / M on every cell: nothing for dK or dQ, and the rank-one term (1 / M) sum_{n masked} G[:, n] on the
//     dV of every live cell -- one vector per object (mrb_plan), added when dV is written;
//   * an object whose memory cells are all masked has no memory tile: only d q_val is non-zero.
// So the kernels run over the COMPACTED live memory cells x the COMPACTED live queries; the rectangles are read on the device.
//
// The launches -- no M x N matrix in memory, no floating-point atomics (every output element has one writer and one fixed order):
//   mrb_plan    block 0 of an object: the raster-order lists of its live memory cells and live queries (ballot + popcount);
//               the other blocks: d q_val, the zeros of the masked cells of dK / dV / dQ, the rank-one vector.
//   mrb_stats<0>, mrb_stats<1>   64 live queries x one of eight ranges of the live memory cells per workgroup: the ranges' soft-max
//               maxima, then (second launch) their sums of exp(S - max) against the maximum of the maxima.
//   mrb_finish  per live query: max, sum (the ranges' sums in index order + the masked cells' term) and delta.  Two words per
//               query; P = exp(S - max) / sum, so equal logits give fl(1 / M) exactly when M is a power of two.
//   mrb_pass<false> ("dkv")   owns 32 live memory cells, loops over the tiles of 32 live queries: dV and dK.
//   mrb_pass<true>  ("dq")    owns 32 live queries, loops over the tiles of 32 live memory cells: dQ.  With few query tiles the
//               memory axis is cut into up to eight ranges (from the shapes alone) for occupancy; the ranges' partial dQ go to the
//               workspace and mrb_dq_merge adds them in index order.
//               Both recompute S and P from the statistics and dP = V^T G in chunks of 64 value channels.
// Arithmetic: every product is v_mfma_f32_16x16x4_f32 -- fp32 in, fp32 accumulate, a k-ordered fmaf chain -- whatever arithmetic
// the forward ran in.  De is padded to the MFMA's k step (and to 16 where it is an output row), Do to the chunk, the cell tiles to
// 32, all with zeros in LDS; value channels beyond 512 go to further workgroups (grid.y), which repeat S and dP.
//
// LDS strides: an operand read as [k][i] (lane (l15, g) reads row 4 ks + g, column l15) is conflict-free on a row stride of 48
// floats, one read as [i][k] (row l15, column 4 ks + g) on 36; a tile that is read both ways (the streamed key-side tile, the
// G chunk) has stride 36 and pays a two-way conflict on half of its [k][i] reads.
#include "common.h"

#include <mutex>

namespace rmnet {
namespace {

constexpr int kThreads = 256;
constexpr int kBM = 32;            // memory cells per tile
constexpr int kBN = 32;            // queries per tile
constexpr int kDC = 64;            // value channels per LDS stage
constexpr int kNC = 8;             // stages per workgroup's dV accumulators: 512 channels
constexpr int kS1 = 48;            // row stride of a [k][i]-read tile
constexpr int kS2 = 36;            // row stride of an [i][k]-read tile
constexpr int kSQ = 80;            // mrb_stats: row stride of its 64-query tile
constexpr int kDeMax = 224;
constexpr int kAuxBlocks = 32;     // elementwise blocks per object in mrb_plan
constexpr int kStatSplits = 8;    // ranges of the memory axis in mrb_stats
constexpr int kDqSplitMax = 8;    // ... and at most in mrb_pass<true>

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct BArgs {
  const float *mk, *mv, *qk;
  const float *out;     // the forward's mem_val [no][2 Do][hw]
  const float *gout;    // its gradient
  const int32_t* mem_rects;
  const int32_t* qry_rects;
  float *dmk, *dmv, *dqk, *dqv;
  int32_t* cnt;         // [no][4]: live memory cells, live queries
  int32_t* qidx;        // [no][hw] live queries in raster order
  int32_t* midx;        // [no][T hw] live memory cells (t * hw + cell) in raster order
  float *smax, *ssum, *sdelta;   // [no][hw] by live query
  float *pmax, *psum;            // [no][kStatSplits][hw] the ranges' maxima and sums
  float* dqpart;                 // [no][splits][De][hw] partial dQ by live query (null: mrb_pass<true> writes dQ itself)
  float* gsum;          // [no][Do] the masked queries' rank-one dV term
  int no, De, Do, T, h, w, hw, thw;
  long long mk_cs, mk_os, mv_cs, mv_os;
  float sqrt_de;
};

__device__ inline bool mem_live(const BArgs& a, int o, int j) {
  if (!a.mem_rects) return true;
  const int t = j / a.hw, pos = j - t * a.hw;
  const int cy = pos / a.w, cx = pos - cy * a.w;
  const int32_t* r = a.mem_rects + ((size_t)o * a.T + t) * 4;
  return cx >= r[0] && cx <= r[1] && cy >= r[2] && cy <= r[3];
}
__device__ inline bool qry_live(const BArgs& a, int o, int cell) {
  if (!a.qry_rects) return true;
  const int cy = cell / a.w, cx = cell - cy * a.w;
  const int32_t* r = a.qry_rects + (size_t)o * 4;
  return cx >= r[0] && cx <= r[1] && cy >= r[2] && cy <= r[3];
}

// Raster-order list of the cells j < n with live(j); returns their number.  All threads of the block call it.
template <class Live>
__device__ inline int compact(int n, int32_t* dst, int* sh, Live live_of) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int total = 0;
  for (int base = 0; base < n; base += kThreads) {
    const int j = base + tid;
    const bool live = j < n && live_of(j);
    const unsigned long long b = __ballot(live);
    const int before = __popcll(b & ((1ull << lane) - 1ull));
    if (lane == 0) sh[wave] = __popcll(b);
    __syncthreads();
    int off = total;
    for (int k = 0; k < wave; ++k) off += sh[k];
    if (live) dst[off + before] = j;
    total += sh[0] + sh[1] + sh[2] + sh[3];
    __syncthreads();
  }
  return total;
}

__global__ __launch_bounds__(kThreads) void mrb_plan(const BArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  int* sh = reinterpret_cast<int*>(lds);
  const int tid = threadIdx.x, o = blockIdx.y, lane = tid & 63, wave = tid >> 6;
  if (blockIdx.x == 0) {
    const int ml = compact(a.thw, a.midx + (size_t)o * a.thw, sh, [&](int j) { return mem_live(a, o, j); });
    const int nl = compact(a.hw, a.qidx + (size_t)o * a.hw, sh, [&](int j) { return qry_live(a, o, j); });
    if (tid == 0) {
      a.cnt[o * 4] = ml; a.cnt[o * 4 + 1] = nl; a.cnt[o * 4 + 2] = 0; a.cnt[o * 4 + 3] = 0;
    }
    return;
  }
  const int nb = (int)gridDim.x - 1, b = (int)blockIdx.x - 1;
  const size_t start = (size_t)b * kThreads + tid, stride = (size_t)nb * kThreads;
  if (a.dqv) {   // d q_val = G2 qm
    const size_t n = (size_t)a.Do * a.hw;
    const float* g2 = a.gout + ((size_t)o * 2 * a.Do + a.Do) * a.hw;
    float* dst = a.dqv + (size_t)o * a.Do * a.hw;
    for (size_t i = start; i < n; i += stride) {
      const int cell = (int)(i % (size_t)a.hw);
      dst[i] = qry_live(a, o, cell) ? g2[i] : 0.0f;
    }
  }
  if (a.mem_rects) {   // the masked cells' zeros (the live cells are written by mrb_pass)
    if (a.dqk) {
      const size_t n = (size_t)a.De * a.hw;
      for (size_t i = start; i < n; i += stride)
        if (!qry_live(a, o, (int)(i % (size_t)a.hw))) a.dqk[(size_t)o * a.De * a.hw + i] = 0.0f;
    }
    if (a.dmk) {
      const size_t n = (size_t)a.De * a.thw;
      for (size_t i = start; i < n; i += stride) {
        const size_t c = i / (size_t)a.thw;
        const int j = (int)(i - c * a.thw);
        if (!mem_live(a, o, j)) a.dmk[(size_t)o * a.mk_os + c * a.mk_cs + j] = 0.0f;
      }
    }
    if (a.dmv) {
      const size_t n = (size_t)a.Do * a.thw;
      for (size_t i = start; i < n; i += stride) {
        const size_t c = i / (size_t)a.thw;
        const int j = (int)(i - c * a.thw);
        if (!mem_live(a, o, j)) a.dmv[(size_t)o * a.mv_os + c * a.mv_cs + j] = 0.0f;
      }
    }
  }
  if (a.dmv) {   // (1 / M) sum over the masked queries of G[d, n]: one wave per channel, lanes stride the cells, a fixed butterfly
    const float* g = a.gout + (size_t)o * 2 * a.Do * a.hw;
    for (int d = b * 4 + wave; d < a.Do; d += nb * 4) {
      float s = 0.0f;
      if (a.qry_rects)
        for (int cell = lane; cell < a.hw; cell += 64)
          if (!qry_live(a, o, cell)) s += g[(size_t)d * a.hw + cell];
#pragma unroll
      for (int x = 32; x > 0; x >>= 1) s += __shfl_xor(s, x);
      if (lane == 0) a.gsum[(size_t)o * a.Do + d] = s / (float)a.thw;
    }
  }
}

// ---------------------------------------------------------------------------------------------- statistics
// mrb_stats is instantiated for KR = 4, 16 or 28 rows of eight key channels per loader thread (De <= 32, <= 128, <= 224): the
// loader then has no bound to test, and its K tile has 8 KR rows.
inline int stats_rows(int De) { return De <= 32 ? 4 : De <= 128 ? 16 : 28; }
inline size_t stats_lds_bytes(int De) {
  const int dep = (De + 3) & ~3;
  return ((size_t)dep * kSQ + (size_t)8 * stats_rows(De) * kS1 + 64) * sizeof(float);
}

constexpr size_t kStatsLdsMax = ((size_t)kDeMax * (kSQ + kS1) + 64) * sizeof(float);
static_assert(kStatsLdsMax + 1024 <= (size_t)kLdsBytesPerCU, "mrb_stats's tiles must fit one CU at De = 224");

// 64 live queries x one of kStatSplits contiguous ranges of the live memory tiles.  PASS 0: the range's maximum per query ->
// pmax; PASS 1 (a launch of its own: it needs every range's maximum): the range's sum of exp(S - max) -> psum.  The maximum of
// maxima is exact, and the ranges' sums are added in index order by mrb_finish, so nothing depends on which workgroup ran when.
template <int PASS, int KR>
__global__ __launch_bounds__(kThreads) void mrb_stats(const BArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int dep = (a.De + 3) & ~3;
  float* Qt = lds;                  // [dep][kSQ]: 64 queries
  float* Kt = Qt + dep * kSQ;       // [8 KR][kS1]: 32 memory cells (rows >= dep are never read)
  int* qc = reinterpret_cast<int*>(Kt + 8 * KR * kS1);   // [64] the queries' cells
  const int tid = threadIdx.x, sp = blockIdx.y, o = blockIdx.z;
  const int wave = tid >> 6, lane = tid & 63, l15 = lane & 15, g = lane >> 4;
  const int ml = a.cnt[o * 4], nl = a.cnt[o * 4 + 1];
  const int n0 = blockIdx.x * 64;
  if (n0 >= nl) return;
  if (tid < 64) qc[tid] = n0 + tid < nl ? a.qidx[(size_t)o * a.hw + n0 + tid] : -1;
  __syncthreads();
  {
    const int col = tid & 63, cell = qc[col];
    const float* qb = a.qk + (size_t)o * a.De * a.hw;
    for (int c = tid >> 6; c < dep; c += 4) Qt[c * kSQ + col] = (c < a.De && cell >= 0) ? qb[(size_t)c * a.hw + cell] : 0.0f;
  }
  const int njt = (ml + kBM - 1) / kBM;
  const int jt0 = (int)((long long)sp * njt / kStatSplits), jt1 = (int)((long long)(sp + 1) * njt / kStatSplits);
  const int n = n0 + wave * 16 + l15;
  const size_t slot = ((size_t)o * kStatSplits + sp) * a.hw + n;
  float mx = -INFINITY, sum = 0.0f;
  if (PASS == 1) {
    if (n < nl)
      for (int s2 = 0; s2 < kStatSplits; ++s2) mx = fmaxf(mx, a.pmax[((size_t)o * kStatSplits + s2) * a.hw + n]);
    if (a.thw - ml > 0 || n >= nl) mx = fmaxf(mx, 0.0f);     // the masked memory cells: logit 0 each
  }
  const float* mkb = a.mk + (size_t)o * a.mk_os;
  const int col = tid & 31, rg = tid >> 5;
  float kst[KR];
  // No predicate in the loader: a column beyond the live cells re-reads the last live cell (its logits are skipped below), a row
  // beyond De re-reads row De - 1 (it meets a zero row of Qt).
  auto k_load = [&](int jt) {
    const int m = jt * kBM + col;
    const int j = a.midx[(size_t)o * a.thw + (m < ml ? m : ml - 1)];
    const float* kp = mkb + (size_t)(rg < a.De ? rg : a.De - 1) * a.mk_cs + j;
    const long long up = 8 * a.mk_cs;
#pragma unroll
    for (int k = 0; k < KR; ++k) {
      kst[k] = *kp;
      if (rg + 8 * k + 8 < a.De) kp += up;
    }
  };
  if (jt0 < jt1) k_load(jt0);
  for (int jt = jt0; jt < jt1; ++jt) {
    __syncthreads();
#pragma unroll
    for (int k = 0; k < KR; ++k) Kt[(rg + 8 * k) * kS1 + col] = kst[k];
    __syncthreads();
    if (jt + 1 < jt1) k_load(jt + 1);     // in flight under the MFMAs below
    f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f};
    for (int ks = 0; ks < dep / 4; ++ks) {
      const float a0 = Kt[(4 * ks + g) * kS1 + l15];
      const float a1 = Kt[(4 * ks + g) * kS1 + 16 + l15];
      const float bq = Qt[(4 * ks + g) * kSQ + wave * 16 + l15];
      s0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, bq, s0, 0, 0, 0);
      s1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, bq, s1, 0, 0, 0);
    }
    const int mb = jt * kBM + 4 * g;
#pragma unroll
    for (int half = 0; half < 2; ++half)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (mb + 16 * half + r >= ml) continue;
        const float s = (half ? s1[r] : s0[r]) / a.sqrt_de;
        if (PASS == 0) mx = fmaxf(mx, s);
        else sum += expf(s - mx);
      }
  }
  if (PASS == 0) {
    mx = fmaxf(mx, __shfl_xor(mx, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    if (g == 0 && n < nl) a.pmax[slot] = mx;
  } else {
    sum += __shfl_xor(sum, 16);
    sum += __shfl_xor(sum, 32);
    if (g == 0 && n < nl) a.psum[slot] = sum;
  }
}

// Per live query: the maximum, the sum (the ranges' sums in index order, then the masked cells' c exp(-max)) and
// delta_n = sum_d G[d, n] R[d, n] (four strided partial sums, merged in order).
__global__ __launch_bounds__(kThreads) void mrb_finish(const BArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* red = lds;                 // [4][64]
  const int tid = threadIdx.x, o = blockIdx.y, q = tid & 63, part = tid >> 6;
  const int ml = a.cnt[o * 4], nl = a.cnt[o * 4 + 1];
  const int n = blockIdx.x * 64 + q;
  if ((int)blockIdx.x * 64 >= nl) return;
  const int cell = n < nl ? a.qidx[(size_t)o * a.hw + n] : -1;
  float acc = 0.0f;
  if (cell >= 0) {
    const float* gb = a.gout + (size_t)o * 2 * a.Do * a.hw + cell;
    const float* rb = a.out + (size_t)o * 2 * a.Do * a.hw + cell;
    for (int d = part; d < a.Do; d += 4) acc = fmaf(gb[(size_t)d * a.hw], rb[(size_t)d * a.hw], acc);
  }
  red[part * 64 + q] = acc;
  __syncthreads();
  if (part == 0 && cell >= 0) {
    const int cmask = a.thw - ml;
    float mx = -INFINITY, sum = 0.0f;
    for (int s2 = 0; s2 < kStatSplits; ++s2) mx = fmaxf(mx, a.pmax[((size_t)o * kStatSplits + s2) * a.hw + n]);
    if (cmask > 0) mx = fmaxf(mx, 0.0f);
    for (int s2 = 0; s2 < kStatSplits; ++s2) sum += a.psum[((size_t)o * kStatSplits + s2) * a.hw + n];
    if (cmask > 0) sum += (float)cmask * expf(-mx);
    a.smax[(size_t)o * a.hw + n] = mx;
    a.ssum[(size_t)o * a.hw + n] = sum;
    a.sdelta[(size_t)o * a.hw + n] = ((red[q] + red[64 + q]) + red[128 + q]) + red[192 + q];
  }
}

// dQ when the memory axis of mrb_pass<true> was split: the ranges' partial sums in index order, then the scale.
__global__ __launch_bounds__(kThreads) void mrb_dq_merge(const BArgs a, int nsplit) {
  const int o = blockIdx.y;
  const int nl = a.cnt[o * 4 + 1];
  const size_t total = (size_t)a.De * nl;
  for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (size_t)gridDim.x * kThreads) {
    const int c = (int)(i / nl), n = (int)(i - (size_t)c * nl);
    float v = 0.0f;
    for (int s2 = 0; s2 < nsplit; ++s2) v += a.dqpart[(((size_t)o * nsplit + s2) * a.De + c) * a.hw + n];
    a.dqk[((size_t)o * a.De + c) * a.hw + a.qidx[(size_t)o * a.hw + n]] = v / a.sqrt_de;
  }
}

// ---------------------------------------------------------------------------------------------- the two gradient passes
inline size_t pass_lds_bytes(int De) {
  const int dep16 = (De + 15) & ~15;
  return ((size_t)dep16 * (kS1 + kS2) + kDC * (kS1 + kS2) + kBM * kS2 + kBM * kS1) * sizeof(float);
}
constexpr size_t kPassLdsMax = ((size_t)kDeMax * (kS1 + kS2) + kDC * (kS1 + kS2) + kBM * kS2 + kBM * kS1) * sizeof(float);
static_assert(kPassLdsMax + 1024 <= (size_t)kLdsBytesPerCU, "mrb_pass's tiles must fit one CU at De = 224");

// DQ = false: the workgroup owns one memory tile (K tile resident, V columns fixed) and streams the query tiles (Q, G, the
//             statistics); it writes dV for the value channels [512 row, +512) and, when row == dk_y, dK.
// DQ = true : the workgroup owns one query tile (Q tile resident, G columns and statistics fixed) and streams the memory
//             tiles (K, V); it writes dQ.
// Workgroup b of a launch lands on XCD b % 8.  Every workgroup of an object streams the same tiles (dkv: all of Q and G; dq: all of
// K and V), so the workgroups of one object belong on one L2: each XCD gets a contiguous range of logical ids (bijective for any
// count), a logical id is (object, row, slot), and the slots of an object are dealt to its tiles with a stride coprime to their
// number -- the live tiles are a prefix that only the device knows, and a contiguous run of slots then holds its share of them.
__device__ inline int xcd_remap(int b, int n) {
  const int q = n >> 3, r = n & 7, x = b & 7;
  return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + (b >> 3);
}

template <bool DQ>
__global__ __launch_bounds__(kThreads) void mrb_pass(const BArgs a, int need_dv, int dk_y, int nx, int ny, int slot_stride) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int dep4 = (a.De + 3) & ~3, dep16 = (a.De + 15) & ~15;
  float* Ot = lds;                    // [dep16][kS1] own key-side tile: K[c][m] (dkv) / Q[c][n] (dq)
  float* St = Ot + dep16 * kS1;       // [dep16][kS2] streamed key-side tile: Q[c][n] (dkv) / K[c][m] (dq)
  float* Vc = St + dep16 * kS2;       // [kDC][kS1] V chunk [d][m]
  float* Gc = Vc + kDC * kS1;         // [kDC][kS2] G chunk [d][n]
  float* Pt = Gc + kDC * kS2;         // [kBM][kS2] P[m][n]
  float* Dt = Pt + kBM * kS2;         // [kBM][kS2] (dkv) or [kBM][kS1] (dq): dS[m][n]
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63, l15 = lane & 15, g = lane >> 4;
  const int wm = wave & 1, wn = wave >> 1;      // this wave's 16 x 16 tile of S and dP
  int o, by, tile;
  {
    const int L = xcd_remap((int)blockIdx.x, (int)gridDim.x);
    o = L / (nx * ny);
    const int rem = L - o * nx * ny;
    by = rem / nx;
    tile = (int)(((long long)(rem - by * nx) * slot_stride) % nx);
  }
  const int ml = a.cnt[o * 4], nl = a.cnt[o * 4 + 1];
  const int own0 = tile * (DQ ? kBN : kBM);
  if (own0 >= (DQ ? nl : ml)) return;
  const bool want_dk = DQ || by == dk_y;     // the logit gradient is needed     // the logit gradient is needed
  const bool want_dv = !DQ && need_dv;
  const int nchunk = (a.Do + kDC - 1) / kDC;
  const int nct = dep16 >> 4;
  const int32_t* midx = a.midx + (size_t)o * a.thw;
  const int32_t* qidx = a.qidx + (size_t)o * a.hw;
  const float* mkb = a.mk + (size_t)o * a.mk_os;
  const float* mvb = a.mv + (size_t)o * a.mv_os;
  const float* qkb = a.qk + (size_t)o * a.De * a.hw;
  const float* gb = a.gout + (size_t)o * 2 * a.Do * a.hw;

  // loader thread: column col of a tile, rows rg + 8 k
  const int col = tid & 31, rg = tid >> 5;
  int mcell, ncell;    // this column's memory cell / query cell (-1: beyond the live cells)
  if (DQ) { ncell = own0 + col < nl ? qidx[own0 + col] : -1; mcell = -1; }
  else { mcell = own0 + col < ml ? midx[own0 + col] : -1; ncell = -1; }
  for (int c = rg; c < dep16; c += 8) {
    float v = 0.0f;
    if (c < a.De) {
      if (DQ) { if (ncell >= 0) v = qkb[(size_t)c * a.hw + ncell]; }
      else if (mcell >= 0) v = mkb[(size_t)c * a.mk_cs + mcell];
    }
    Ot[c * kS1 + col] = v;
  }

  // statistics of this wave's query column (dq: fixed)
  float st_mx = 0.0f, st_sum = 1.0f, st_dl = 0.0f;
  bool n_ok = false;
  auto load_stats = [&](int n0) {
    const int n = n0 + 16 * wn + l15;
    n_ok = n < nl;
    st_mx = n_ok ? a.smax[(size_t)o * a.hw + n] : 0.0f;
    st_sum = n_ok ? a.ssum[(size_t)o * a.hw + n] : 1.0f;
    st_dl = n_ok ? a.sdelta[(size_t)o * a.hw + n] : 0.0f;
  };
  if (DQ) load_stats(own0);

  float vst[kDC / 8], gst[kDC / 8];
  auto stage_load = [&](int ch) {
    const int d0 = ch * kDC + rg;
#pragma unroll
    for (int k = 0; k < kDC / 8; ++k) {
      const int d = d0 + 8 * k;
      vst[k] = (d < a.Do && mcell >= 0) ? mvb[(size_t)d * a.mv_cs + mcell] : 0.0f;
      gst[k] = (d < a.Do && ncell >= 0) ? gb[(size_t)d * a.hw + ncell] : 0.0f;
    }
  };
  auto stage_write = [&]() {
#pragma unroll
    for (int k = 0; k < kDC / 8; ++k) {
      Vc[(rg + 8 * k) * kS1 + col] = vst[k];
      Gc[(rg + 8 * k) * kS2 + col] = gst[k];
    }
  };

  f32x4 dv[kNC][2];     // dkv: dV[d = 64 c + 16 wave + ..][m = 16 mt + ..]
  f32x4 dk[4][2];       // dK[c = 16 (wave + 4 i) + ..][m] (dkv) / dQ[c][n] (dq)
#pragma unroll
  for (int c = 0; c < kNC; ++c) dv[c][0] = dv[c][1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < 4; ++i) dk[i][0] = dk[i][1] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nsteps = ((DQ ? ml : nl) + 31) / 32;
  // dq: row `by` of ny walks its contiguous share of the memory tiles
  const int step0 = DQ ? (int)((long long)by * nsteps / ny) : 0, step1 = DQ ? (int)((long long)(by + 1) * nsteps / ny) : nsteps;
  for (int step = step0; step < step1; ++step) {
    const int s0i = step * 32;
    if (DQ) mcell = s0i + col < ml ? midx[s0i + col] : -1;
    else ncell = s0i + col < nl ? qidx[s0i + col] : -1;
    stage_load(0);                       // in flight under the logits below
    __syncthreads();                     // the previous step's reads of St / Dt are done (and, at the first step, Ot is complete)
    for (int c = rg; c < dep16; c += 8) {
      float v = 0.0f;
      if (c < a.De) {
        if (DQ) { if (mcell >= 0) v = mkb[(size_t)c * a.mk_cs + mcell]; }
        else if (ncell >= 0) v = qkb[(size_t)c * a.hw + ncell];
      }
      St[c * kS2 + col] = v;
    }
    if (!DQ) load_stats(s0i);
    __syncthreads();
    // ---- S[m][n] = sum_c K[c][m] Q[c][n]: A = K ([k][i]), B = Q ([k][j])
    f32x4 sacc = {0.f, 0.f, 0.f, 0.f};
    {
      const float* Ka = DQ ? St : Ot;
      const float* Qb = DQ ? Ot : St;
      const int ksa = DQ ? kS2 : kS1, ksb = DQ ? kS1 : kS2;
      for (int ks = 0; ks < dep4 / 4; ++ks)
        sacc = __builtin_amdgcn_mfma_f32_16x16x4f32(Ka[(4 * ks + g) * ksa + 16 * wm + l15], Qb[(4 * ks + g) * ksb + 16 * wn + l15], sacc, 0,
                                                    0, 0);
    }
    const int m_base = (DQ ? s0i : own0) + 16 * wm + 4 * g;
    float p[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const bool ok = n_ok && m_base + r < ml;
      p[r] = ok ? expf(sacc[r] / a.sqrt_de - st_mx) / st_sum : 0.0f;
      if (want_dv) Pt[(16 * wm + 4 * g + r) * kS2 + 16 * wn + l15] = p[r];
    }
    // ---- over the value channels: dP[m][n] += sum_d V[d][m] G[d][n]; dkv: dV[d][m] += sum_n G[d][n] P[m][n]
    f32x4 dp = {0.f, 0.f, 0.f, 0.f};
    for (int cb = 0; cb < nchunk; cb += kNC) {
      const bool mine = want_dv && cb == by * kNC;
#pragma unroll
      for (int c = 0; c < kNC; ++c) {
        const int ch = cb + c;
        if (ch < nchunk) {
          __syncthreads();               // the previous chunk's reads are done; P is visible
          stage_write();
          if (ch + 1 < nchunk) stage_load(ch + 1);     // in flight under this chunk's MFMAs
          __syncthreads();
          if (want_dk) {
#pragma unroll
            for (int ks = 0; ks < kDC / 4; ++ks)
              dp = __builtin_amdgcn_mfma_f32_16x16x4f32(Vc[(4 * ks + g) * kS1 + 16 * wm + l15], Gc[(4 * ks + g) * kS2 + 16 * wn + l15], dp, 0,
                                                        0, 0);
          }
          if (mine) {
#pragma unroll
            for (int ks = 0; ks < kBN / 4; ++ks) {
              const float ga = Gc[(16 * wave + l15) * kS2 + 4 * ks + g];
              dv[c][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(ga, Pt[l15 * kS2 + 4 * ks + g], dv[c][0], 0, 0, 0);
              dv[c][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(ga, Pt[(16 + l15) * kS2 + 4 * ks + g], dv[c][1], 0, 0, 0);
            }
          }
        }
      }
    }
    if (!want_dk) continue;
    // ---- dS = P o (dP - delta); dkv: dK[c][m] += sum_n Q[c][n] dS[m][n]; dq: dQ[c][n] += sum_m K[c][m] dS[m][n]
#pragma unroll
    for (int r = 0; r < 4; ++r) Dt[(16 * wm + 4 * g + r) * (DQ ? kS1 : kS2) + 16 * wn + l15] = p[r] * (dp[r] - st_dl);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int ct = wave + 4 * i;
      if (ct < nct) {
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
          const float ca = St[(16 * ct + l15) * kS2 + 4 * ks + g];
          const float b0 = DQ ? Dt[(4 * ks + g) * kS1 + l15] : Dt[l15 * kS2 + 4 * ks + g];
          const float b1 = DQ ? Dt[(4 * ks + g) * kS1 + 16 + l15] : Dt[(16 + l15) * kS2 + 4 * ks + g];
          dk[i][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(ca, b0, dk[i][0], 0, 0, 0);
          dk[i][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(ca, b1, dk[i][1], 0, 0, 0);
        }
      }
    }
  }

  // ---- write-out: lane holds rows 4 g + r, column l15 of every accumulator tile
  int ocell[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int x = own0 + 16 * t + l15;
    ocell[t] = DQ ? (x < nl ? qidx[x] : -1) : (x < ml ? midx[x] : -1);
  }
  if (want_dv) {
    float* dst = a.dmv + (size_t)o * a.mv_os;
#pragma unroll
    for (int c = 0; c < kNC; ++c)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int d = (by * kNC + c) * kDC + 16 * wave + 4 * g + r;
        if (d >= a.Do) continue;
        const float rank1 = a.gsum[(size_t)o * a.Do + d];
#pragma unroll
        for (int t = 0; t < 2; ++t)
          if (ocell[t] >= 0) dst[(size_t)d * a.mv_cs + ocell[t]] = dv[c][t][r] + rank1;
      }
  }
  if (want_dk) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int c = 16 * (wave + 4 * i) + 4 * g + r;
        if (c >= a.De) continue;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          if (ocell[t] < 0) continue;
          if (DQ && a.dqpart) {
            a.dqpart[(((size_t)o * ny + by) * a.De + c) * a.hw + own0 + 16 * t + l15] = dk[i][t][r];
            continue;
          }
          const float v = dk[i][t][r] / a.sqrt_de;
          if (DQ) a.dqk[((size_t)o * a.De + c) * a.hw + ocell[t]] = v;
          else a.dmk[(size_t)o * a.mk_os + (size_t)c * a.mk_cs + ocell[t]] = v;
        }
      }
  }
}

// A dynamic LDS request above 64 KB needs the function attribute: set once per device and kernel, for the largest De
// (conv_rows_core.h has the same rule: never while the stream is capturing, so the first call on a device must be an eager one).
template <auto Kernel, size_t kBytes>
int lds_prepare(hipStream_t st) {
  static std::mutex mu;
  static bool done[64] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return RMNET_E_LAUNCH;
  std::lock_guard<std::mutex> lock(mu);
  if (done[dev]) return RMNET_OK;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(st, &cs) != hipSuccess) return RMNET_E_LAUNCH;
  if (cs != hipStreamCaptureStatusNone) return RMNET_E_UNSUPPORTED;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kBytes) != hipSuccess)
    return RMNET_E_LAUNCH;
  done[dev] = true;
  return RMNET_OK;
}

inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }

// Ranges of the memory axis in the dq launch: enough workgroups for the chip from shapes alone (not from T: the workspace stays
// linear in it), at most kDqSplitMax.
inline int dq_splits(int no, long long hw) {
  const long long pairs = ((hw + kBN - 1) / kBN) * no;
  long long ns = 512 / pairs;
  if (ns > kDqSplitMax) ns = kDqSplitMax;
  return ns < 1 ? 1 : (int)ns;
}

inline int coprime_stride(int n) {   // about 0.618 n, coprime to n (n - 1 always is)
  if (n <= 2) return 1;
  int s = (int)(0.618 * n);
  if (s < 1) s = 1;
  auto gcd = [](int x, int y) { while (y) { const int t = x % y; x = y; y = t; } return x; };
  while (gcd(s, n) != 1) ++s;
  return s;
}

}  // namespace

// Workspace: [cnt][qidx][smax][ssum][sdelta][pmax][psum][gsum][dq partials] (each rounded up to 256 bytes; none depends on T),
// then midx [no][T hw] -- so the size is an exact linear function of T.
size_t memory_read_bwd_ws_bytes(int no, int De, int Do, int T, int h, int w) {
  const size_t hw = (size_t)h * w;
  const int nsq = dq_splits(no, (long long)hw);
  return al256((size_t)no * 16) + 4 * al256((size_t)no * hw * 4) + 2 * al256((size_t)no * kStatSplits * hw * 4) +
         al256((size_t)no * Do * 4) + (nsq > 1 ? al256((size_t)no * nsq * De * hw * 4) : 0) + (size_t)no * T * hw * 4;
}

int launch_memory_read_bwd(const MemReadBwdArgs& m, hipStream_t st) {
  if (!m.mk || !m.mv || !m.qk || !m.qv || !m.out || !m.gout) return RMNET_E_INVALID_ARG;
  if (!m.dmk && !m.dmv && !m.dqk && !m.dqv) return RMNET_E_INVALID_ARG;
  if (m.no <= 0 || m.De <= 0 || m.Do <= 0 || m.T <= 0 || m.h <= 0 || m.w <= 0) return RMNET_E_INVALID_ARG;
  if ((m.mem_rects == nullptr) != (m.qry_rects == nullptr)) return RMNET_E_INVALID_ARG;
  const long long hw = (long long)m.h * m.w, thw = hw * m.T;
  if (thw > (1LL << 30) || m.no > 65535) return RMNET_E_UNSUPPORTED;
  const long long mk_cs = m.mk_cs ? m.mk_cs : thw, mv_cs = m.mv_cs ? m.mv_cs : thw;
  const long long mk_os = m.mk_os ? m.mk_os : mk_cs * m.De, mv_os = m.mv_os ? m.mv_os : mv_cs * m.Do;
  if (mk_cs < thw || mv_cs < thw) return RMNET_E_INVALID_ARG;
  if (m.De > kDeMax) return RMNET_E_UNSUPPORTED;
  const long long ndo = ((long long)m.Do + kNC * kDC - 1) / (kNC * kDC);
  if (((thw + kBM - 1) / kBM) * ndo * m.no > 0x7fffffffLL) return RMNET_E_UNSUPPORTED;   // workgroups of the dkv launch
  if (!m.ws || m.ws_bytes < memory_read_bwd_ws_bytes(m.no, m.De, m.Do, m.T, m.h, m.w)) return RMNET_E_WORKSPACE;
  if ((reinterpret_cast<uintptr_t>(m.ws) & 3) != 0) return RMNET_E_INVALID_ARG;

  BArgs a;
  a.mk = m.mk; a.mv = m.mv; a.qk = m.qk; a.out = m.out; a.gout = m.gout;
  a.mem_rects = m.mem_rects; a.qry_rects = m.qry_rects;
  a.dmk = m.dmk; a.dmv = m.dmv; a.dqk = m.dqk; a.dqv = m.dqv;
  a.no = m.no; a.De = m.De; a.Do = m.Do; a.T = m.T; a.h = m.h; a.w = m.w; a.hw = (int)hw; a.thw = (int)thw;
  a.mk_cs = mk_cs; a.mk_os = mk_os; a.mv_cs = mv_cs; a.mv_os = mv_os;
  a.sqrt_de = sqrtf((float)m.De);
  char* p = static_cast<char*>(m.ws);
  a.cnt = reinterpret_cast<int32_t*>(p); p += al256((size_t)m.no * 16);
  a.qidx = reinterpret_cast<int32_t*>(p); p += al256((size_t)m.no * hw * 4);
  a.smax = reinterpret_cast<float*>(p); p += al256((size_t)m.no * hw * 4);
  a.ssum = reinterpret_cast<float*>(p); p += al256((size_t)m.no * hw * 4);
  a.sdelta = reinterpret_cast<float*>(p); p += al256((size_t)m.no * hw * 4);
  a.pmax = reinterpret_cast<float*>(p); p += al256((size_t)m.no * kStatSplits * hw * 4);
  a.psum = reinterpret_cast<float*>(p); p += al256((size_t)m.no * kStatSplits * hw * 4);
  a.gsum = reinterpret_cast<float*>(p); p += al256((size_t)m.no * m.Do * 4);
  const int nsq = dq_splits(m.no, hw);
  a.dqpart = nullptr;
  if (nsq > 1) { a.dqpart = reinterpret_cast<float*>(p); p += al256((size_t)m.no * nsq * m.De * hw * 4); }
  a.midx = reinterpret_cast<int32_t*>(p);

  const bool heavy = m.dmk || m.dmv || m.dqk;
  const size_t shm = pass_lds_bytes(m.De), shm_stats = stats_lds_bytes(m.De);
  if (heavy && shm_stats > 65536)
  {
    if (int e = lds_prepare<mrb_stats<0, 16>, kStatsLdsMax>(st)) return e;
    if (int e = lds_prepare<mrb_stats<1, 16>, kStatsLdsMax>(st)) return e;
    if (int e = lds_prepare<mrb_stats<0, 28>, kStatsLdsMax>(st)) return e;
    if (int e = lds_prepare<mrb_stats<1, 28>, kStatsLdsMax>(st)) return e;
  }
  if (heavy && shm > 65536) {
    if (m.dmk || m.dmv)
      if (int e = lds_prepare<mrb_pass<false>, kPassLdsMax>(st)) return e;
    if (m.dqk)
      if (int e = lds_prepare<mrb_pass<true>, kPassLdsMax>(st)) return e;
  }
  hipLaunchKernelGGL(mrb_plan, dim3(1 + kAuxBlocks, m.no), dim3(kThreads), 64, st, a);
  if (int e = check_launch()) return e;
  if (!heavy) return RMNET_OK;
  const dim3 gs((unsigned)((hw + 63) / 64), kStatSplits, m.no);
  const int kr = stats_rows(m.De);
  if (kr == 4) {
    hipLaunchKernelGGL((mrb_stats<0, 4>), gs, dim3(kThreads), shm_stats, st, a);
    hipLaunchKernelGGL((mrb_stats<1, 4>), gs, dim3(kThreads), shm_stats, st, a);
  } else if (kr == 16) {
    hipLaunchKernelGGL((mrb_stats<0, 16>), gs, dim3(kThreads), shm_stats, st, a);
    hipLaunchKernelGGL((mrb_stats<1, 16>), gs, dim3(kThreads), shm_stats, st, a);
  } else {
    hipLaunchKernelGGL((mrb_stats<0, 28>), gs, dim3(kThreads), shm_stats, st, a);
    hipLaunchKernelGGL((mrb_stats<1, 28>), gs, dim3(kThreads), shm_stats, st, a);
  }
  if (int e = check_launch()) return e;
  hipLaunchKernelGGL(mrb_finish, dim3((unsigned)((hw + 63) / 64), m.no), dim3(kThreads), 1024, st, a);
  if (int e = check_launch()) return e;
  if (m.dmk || m.dmv) {
    // dV needs one workgroup row per 512 value channels; dK rides in row 0 (or is the only row when dV is not wanted)
    const int nx = (int)((thw + kBM - 1) / kBM), ny = m.dmv ? (int)ndo : 1;
    hipLaunchKernelGGL(mrb_pass<false>, dim3((unsigned)(nx * ny * m.no)), dim3(kThreads), shm, st, a, m.dmv ? 1 : 0, m.dmk ? 0 : -1, nx, ny,
                       coprime_stride(nx));
    if (int e = check_launch()) return e;
  }
  if (m.dqk) {
    const int nx = (int)((hw + kBN - 1) / kBN);
    hipLaunchKernelGGL(mrb_pass<true>, dim3((unsigned)(nx * nsq * m.no)), dim3(kThreads), shm, st, a, 0, 0, nx, nsq, coprime_stride(nx));
    if (int e = check_launch()) return e;
    if (nsq > 1) {
      hipLaunchKernelGGL(mrb_dq_merge, dim3(64, m.no), dim3(kThreads), 0, st, a, nsq);
      if (int e = check_launch()) return e;
    }
  }
  return RMNET_OK;
}

}  // namespace rmnet
