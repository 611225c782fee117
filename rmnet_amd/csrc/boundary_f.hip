// boundary_f.hip -- the four integer counts behind the boundary measure F (utils/metrics.py:119-169) of every (frame, object) pair,
// from two uint8 label maps, as bit work on wave64.
//
// With seg = (label == k) for k = 1 .. K (a label above K belongs to no object):
//   n_fg     = |bmap(pred_k)|                                 n_gt     = |bmap(gt_k)|                       (utils/metrics.py:151-152)
//   fg_match = |bmap(pred_k) & dilate(bmap(gt_k), disk(r))|   gt_match = |bmap(gt_k) & dilate(bmap(pred_k), disk(r))|     (:141-148)
// bmap is seg2bmap with width / height unset (utils/metrics.py:202-213): with e / s / se the map shifted by one pixel towards the
// origin and ZERO in the column / row that has no neighbour,
//   b = seg ^ e | seg ^ s | seg ^ se;   b[-1, :] = seg[-1, :] ^ e[-1, :];   b[:, -1] = seg[:, -1] ^ s[:, -1];   b[-1, -1] = 0
// which is b = (E & (seg ^ e)) | (S & (seg ^ s)) | (E & S & (seg ^ se)) with E = (x < W - 1), S = (y < H - 1) at every pixel, the
// H == 1 and W == 1 maps included.  disk(r) = {(dy, dx): dx^2 + dy^2 <= r^2} (skimage.morphology.disk) and the dilation reads 0
// outside the image (skimage.morphology.binary_dilation = scipy.ndimage.binary_dilation, border value 0).
//
// Pass 1, bf_bitrows: one wave per (frame, block of 8 rows, 64-pixel word).  Lane l is pixel x = 64 w + l; it loads its own label
// and its right neighbour's in the block's rows and the row below them from both maps (consecutive bytes across the wave, all loads
// in flight together), and for every row and object one __ballot of the boundary predicate IS the word: bit l = pixel 64 w + l,
// bits at x >= W are 0.  Lane k - 1 keeps object k's two words and stores them into the workspace
//   bits [N][K][2][H][WW] 64-bit words, WW = ceil(W / 64), map 0 = pred, map 1 = gt.
// The waves of row block 0, word 0 also clear their frame's counts, so the caller does not pre-zero them.
//
// Pass 2, bf_match: one thread per (frame, object, row, word).  The dilated word at (y, w) is the OR over d = 0 .. r of the
// horizontal dilation by hw(d) = floor(sqrt(r^2 - d^2)) of (row y - d | row y + d), rows outside the image dropped.  The horizontal
// dilation works on the word and its two neighbours (hw <= 40 < 64: no bit comes from further away; the neighbour of the first /
// last word of a row is 0, so nothing wraps from one row or frame into the next): an OR of left shifts over 0 .. hw and of right
// shifts over 0 .. hw, each by doubling the reach (1, 2, 4, ... then one last shift by what is missing).  AND with the other
// map's own word, __popcll, a wave reduction and four integer atomic adds per wave: integer sums are exact in any order, so two
// calls return the same bits.  No LDS, no scratch.
#include "common.h"

namespace rmnet {
namespace {

typedef unsigned long long u64;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / RMNET_WAVE;
constexpr int kMaxObjects = 64;      // one lane per object keeps its words in pass 1
constexpr int kMaxRadius = 40;       // < 64: a dilated word depends on its two neighbours only
constexpr int kRows = 8;             // rows per wave in pass 1: each label row is loaded once for the row above it and once for itself

__global__ __launch_bounds__(kThreads) void bf_bitrows(const uint8_t* __restrict__ pred, const uint8_t* __restrict__ gt,
                                                       u64* __restrict__ bits, int32_t* __restrict__ counts, int N, int K, int H, int W,
                                                       int WW, int RB, long long n_waves) {
  const int lane = threadIdx.x & (RMNET_WAVE - 1);
  const long long g = (long long)blockIdx.x * kWaves + (threadIdx.x >> 6);      // wave-uniform
  if (g >= n_waves) return;
  const int w = (int)(g % WW);
  const long long blk = g / WW;
  const int y0 = (int)(blk % RB) * kRows;
  const int n = (int)(blk / RB);
  if (y0 == 0 && w == 0 && lane < K) {
    int32_t* c = counts + ((size_t)n * K + lane) * 4;
    c[0] = c[1] = c[2] = c[3] = 0;
  }
  const int x = w * 64 + lane;
  const bool in = x < W, E = x + 1 < W;
  // rows y0 .. y0 + kRows of the word's pixels and of their right neighbours, every load issued before the first use.
  // 0xFFFF is no label: a pixel outside the map never equals k, and E / S mask every term that would read it
  int p0[kRows + 1], p1[kRows + 1], g0[kRows + 1], g1[kRows + 1];
#pragma unroll
  for (int i = 0; i <= kRows; ++i) {
    const bool row = y0 + i < H;
    const size_t at = ((size_t)n * H + (row ? y0 + i : 0)) * W + x;             // (row 0 stands in for a row that is not read)
    p0[i] = row && in ? pred[at] : 0xFFFF;
    p1[i] = row && E ? pred[at + 1] : 0xFFFF;
    g0[i] = row && in ? gt[at] : 0xFFFF;
    g1[i] = row && E ? gt[at + 1] : 0xFFFF;
  }
  const size_t plane = (size_t)H * WW;
#pragma unroll
  for (int i = 0; i < kRows; ++i) {
    const int y = y0 + i;
    if (y >= H) break;                                                          // (wave-uniform)
    const bool S = y + 1 < H;
    u64 mine_p = 0, mine_g = 0;
    for (int k = 1; k <= K; ++k) {
      const bool ps = p0[i] == k, gs = g0[i] == k;
      const bool pb = (E && (ps != (p1[i] == k))) || (S && in && (ps != (p0[i + 1] == k))) || (E && S && (ps != (p1[i + 1] == k)));
      const bool gb = (E && (gs != (g1[i] == k))) || (S && in && (gs != (g0[i + 1] == k))) || (E && S && (gs != (g1[i + 1] == k)));
      const u64 pw = __ballot(pb), gw = __ballot(gb);
      if (lane == k - 1) { mine_p = pw; mine_g = gw; }
    }
    if (lane < K) {
      u64* o = bits + ((size_t)n * K + lane) * 2 * plane + (size_t)y * WW + w;
      o[0] = mine_p;
      o[plane] = mine_g;
    }
  }
}

// word `c` of a bit row with its neighbours `l` (lower x) and `r` (higher x), dilated by hw columns: bit x = OR of bits x - hw .. x + hw
__device__ inline u64 dilate_word(u64 l, u64 c, u64 r, int hw) {
  u64 up = c, dn = c;      // up: OR of bits x - reach + 1 .. x (carries from l);  dn: OR of bits x .. x + reach - 1 (carries from r)
  int reach = 1;
  while (2 * reach <= hw + 1) {                    // (hw is uniform over the launch: scalar control flow; reach <= 16 here)
    up |= (up << reach) | (l >> (64 - reach));
    l |= l << reach;
    dn |= (dn >> reach) | (r << (64 - reach));
    r |= r >> reach;
    reach *= 2;
  }
  const int f = hw + 1 - reach;                    // 0 <= f < reach <= 32
  if (f > 0) {
    up |= (up << f) | (l >> (64 - f));
    dn |= (dn >> f) | (r << (64 - f));
  }
  return up | dn;
}

__global__ __launch_bounds__(kThreads) void bf_match(const u64* __restrict__ bits, int32_t* __restrict__ counts, int H, int WW, int radius,
                                                     int blocks_per_plane) {
  const long long plane = (long long)H * WW;
  const long long nk = blockIdx.x / blocks_per_plane;                            // (frame, object) pair
  const long long p = (long long)(blockIdx.x % blocks_per_plane) * kThreads + threadIdx.x;
  const bool valid = p < plane;
  const int y = valid ? (int)(p / WW) : 0, w = valid ? (int)(p % WW) : 0;
  const u64* P = bits + (size_t)nk * 2 * plane;
  const u64* G = P + plane;
  const bool hasl = valid && w > 0, hasr = valid && w + 1 < WW;
  const u64 pc = valid ? P[p] : 0, gc = valid ? G[p] : 0;
  u64 pd = 0, gd = 0;
  int hw = radius;
  for (int d = 0; d <= radius; ++d) {
    while (hw * hw + d * d > radius * radius) --hw;                              // hw = floor(sqrt(r^2 - d^2)) >= 0, exact in integers
    u64 pl = 0, pm = 0, pr = 0, gl = 0, gm = 0, gr = 0;
    if (valid && y - d >= 0) {
      const long long q = p - (long long)d * WW;
      pm = P[q]; gm = G[q];
      if (hasl) { pl = P[q - 1]; gl = G[q - 1]; }
      if (hasr) { pr = P[q + 1]; gr = G[q + 1]; }
    }
    if (valid && d > 0 && y + d < H) {
      const long long q = p + (long long)d * WW;
      pm |= P[q]; gm |= G[q];
      if (hasl) { pl |= P[q - 1]; gl |= G[q - 1]; }
      if (hasr) { pr |= P[q + 1]; gr |= G[q + 1]; }
    }
    pd |= dilate_word(pl, pm, pr, hw);
    gd |= dilate_word(gl, gm, gr, hw);
  }
  const int n_fg = wave_sum(__popcll(pc)), n_gt = wave_sum(__popcll(gc));
  const int fg_match = wave_sum(__popcll(pc & gd)), gt_match = wave_sum(__popcll(gc & pd));
  if ((threadIdx.x & (RMNET_WAVE - 1)) == 0) {
    int32_t* c = counts + (size_t)nk * 4;
    if (n_fg) atomicAdd(c + 0, n_fg);
    if (n_gt) atomicAdd(c + 1, n_gt);
    if (fg_match) atomicAdd(c + 2, fg_match);
    if (gt_match) atomicAdd(c + 3, gt_match);
  }
}

}  // namespace

size_t boundary_match_ws_bytes(int N, int K, int H, int W) {
  return (size_t)N * K * 2 * H * ((W + 63) / 64) * sizeof(u64);
}

int launch_boundary_match(const uint8_t* pred, const uint8_t* gt, int N, int K, int H, int W, int radius, int32_t* counts, void* ws,
                          size_t ws_bytes, hipStream_t st) {
  if (!pred || !gt || !counts || N <= 0 || K <= 0 || H <= 0 || W <= 0) return RMNET_E_INVALID_ARG;
  if (K > kMaxObjects || radius < 0 || radius > kMaxRadius) return RMNET_E_UNSUPPORTED;
  if (!ws || ws_bytes < boundary_match_ws_bytes(N, K, H, W)) return RMNET_E_WORKSPACE;
  if ((reinterpret_cast<uintptr_t>(ws) & 7) || (reinterpret_cast<uintptr_t>(counts) & 3)) return RMNET_E_INVALID_ARG;
  const int WW = (W + 63) / 64;
  const int RB = (H + kRows - 1) / kRows;
  const long long n_waves = (long long)N * RB * WW;
  const long long plane = (long long)H * WW;
  const long long bpp = (plane + kThreads - 1) / kThreads;
  const long long grid1 = (n_waves + kWaves - 1) / kWaves, grid2 = bpp * N * K;
  if (grid1 >= (1LL << 31) || grid2 >= (1LL << 31)) return RMNET_E_UNSUPPORTED;
  u64* bits = static_cast<u64*>(ws);
  hipLaunchKernelGGL(bf_bitrows, dim3((unsigned)grid1), dim3(kThreads), 0, st, pred, gt, bits, counts, N, K, H, W, WW, RB, n_waves);
  hipLaunchKernelGGL(bf_match, dim3((unsigned)grid2), dim3(kThreads), 0, st, bits, counts, H, WW, radius, (int)bpp);
  return check_launch();
}

}  // namespace rmnet
