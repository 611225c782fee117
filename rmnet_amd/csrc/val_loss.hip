// val_loss.hip -- the validation loss of a clip, Lovasz-softmax + NLL (core/test.py:97, models/lovasz_loss.py), without a sort.
//
// With e = |fg - p_c| the error of a pixel for class c, F(t) / B(t) the numbers of foreground / background pixels of the class
// whose error exceeds t and G the foreground count, the Lovasz extension of the class is the integral over t in [0, 1] of
//   J(t) = 1 - (G - F(t)) / (G + B(t))
// (Abel summation of the reference's dot(errors_sorted, lovasz_grad); J does not increase in t).  Two integer histograms of
// key = (unsigned)(e * bins) per class, hist[c][fg][0 .. bins], bracket the integral: the Riemann sum with the counts of bins >= k
// is an upper bound (hi), the one with the counts of bins > k a lower bound (lo), hi - lo <= 1 / bins.  Bin `bins` holds e == 1
// alone and has no width.  A valid pixel (label != ignore_index) is bad when its label is >= K (checked first) or when any of its
// K probabilities is outside [0, 1] (NaN included); bad pixels are counted and left out of every sum.
//
// vl_hist: what I chose and why.
//   * Pixels go in groups of 4 consecutive indices of the flattened [N*H*W] clip, one group per lane per step, a workgroup over a
//     contiguous range of groups, so a wave's load of one class plane is 1 KB contiguous.  A group is read with one 16-byte load
//     per class (and one 4-byte load of the labels) when it lies inside one frame and the address is aligned; any other group
//     (a frame boundary inside it, the end of the clip, a plane size or a base pointer that is no multiple of 4 elements) is
//     read element by element.  The choice is per lane and per class, so head, body and tail need no separate loops.
//   * The K probabilities of a pixel are read twice: once to decide whether the pixel is bad (which needs all K before any count
//     is made) and once to count.  K goes up to 255, so they cannot be kept in registers; the second read hits the cache.
//   * The keys are extremely skewed towards the two ends: 0 where the network is right and sure, `bins` and the bins just below
//     it where it is wrong and sure (the first measurement, profiles/r31_a_val_loss.md, had 87 % of a saturated network's
//     elements there, and as single global atomics on a few addresses they cost 160 ms).  Keys 0 and `bins` are aggregated over
//     the wave: one __ballot + popcount per pixel of the group, end and foreground flag, summed in scalar registers, and lane 0
//     adds the four totals into LDS -- four LDS adds per wave, class and step in place of up to 512 on one address.
//   * The LB lowest and the HB highest bins of every class live in a privatised histogram in dynamic LDS for the lifetime of
//     the workgroup.  With S the largest power of two for which K * 2 * S * 4 bytes <= 62 KB: the whole histogram when
//     bins + 1 <= S (LB = bins + 1, HB = 0), else LB = HB = S / 2.  LDS adds do not go through the memory side, and the
//     workgroup flushes its non-zero entries once at its end.
//   * Only the keys in between, the sparse remainder, go out as individual relaxed, agent-scope integer atomics.  Integer sums
//     do not depend on the order: two calls return the same bits.
//   * The grid is at most kMaxBlocks workgroups whatever the device, so the float64 NLL partials -- one per workgroup, reduced in
//     a fixed order over lanes, waves and workgroups, no float atomics -- are the same on every device too.
// vl_scan: one workgroup per class.  The 16 waves take 16 contiguous segments of the bins; pass 1 sums each segment's counts
// (integers: any order), pass 2 walks the segment from its top in steps of 64 x 16 bins: every lane takes 16 consecutive bins,
// one wave-wide suffix scan over the lanes' totals per step (shuffles are LDS round trips: one scan per 1024 bins, not per 64),
// and the lane adds its float64 terms from its top bin down; lanes, then waves, are reduced in a fixed order.  Workgroup 0 also
// adds the NLL partials and the pixel counters in workgroup order.  Plain stores only; no static LDS (dynamic, sized at launch).
// The histogram is cleared by a memset in front of vl_hist (a memset node under capture): the caller never pre-zeros.
#include "val_loss_parts.h"

namespace rmnet {
namespace {

using namespace vl;      // the layout, the LDS rule and the wave reductions are shared with val_loss_bwd.hip

extern __shared__ __align__(8) unsigned char vl_dyn[];

// partials: [kMaxBlocks] double nll, then [kMaxBlocks][3] long long (valid good, bad label, bad probability)
__global__ __launch_bounds__(kHistThreads) void vl_hist(const float* __restrict__ probs, const uint8_t* __restrict__ labels,
                                                        u32* __restrict__ hist, double* __restrict__ part_nll,
                                                        long long* __restrict__ part_cnt, long long P, long long HW, int K, int ignore,
                                                        int bins, int LB, int HB, long long groups, long long per_block) {
  const int S = LB + HB;                                                      // slots per class and flag: [0, LB) low, [LB, S) high
  const u32 hi0 = HB ? (u32)(bins + 1 - HB) : (u32)bins + 1;                  // first high bin (none: above every key)
  u32* low = reinterpret_cast<u32*>(vl_dyn);                                  // [K][2][S]
  double* red = reinterpret_cast<double*>(vl_dyn + (size_t)K * 2 * S * sizeof(u32));           // [kHistWaves][4], 8-byte aligned
  const int tid = threadIdx.x, lane = tid & (RMNET_WAVE - 1), wave = tid >> 6;
  const int n_low = K * 2 * S;
  for (int i = tid; i < n_low; i += kHistThreads) low[i] = 0;
  __syncthreads();

  const long long g0 = (long long)blockIdx.x * per_block;
  const long long g1 = g0 + per_block < groups ? g0 + per_block : groups;
  const float fbins = (float)bins;
  const size_t stride = (size_t)bins + 1;
  double nll = 0.0;
  int n_good = 0, n_badl = 0, n_badp = 0;

  for (long long gb = g0; gb < g1; gb += kHistThreads) {                       // (uniform over the workgroup)
    const long long g = gb + tid;
    const bool act = g < g1;
    const long long p0 = act ? g * 4 : 0;
    const int cnt = act ? (int)(P - p0 < 4 ? P - p0 : 4) : 0;
    const long long n0 = p0 / HW, r0 = p0 - n0 * HW;
    const bool one_frame = cnt == 4 && r0 + 3 < HW;
    // class-0 element offset of each pixel; pixels past `cnt` stand on pixel p0 and are never read
    size_t off[4];
    int lab[4];
    bool good[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      long long r = r0 + j, n = n0;
      if (r >= HW) { r -= HW; ++n; if (r >= HW) { n = (p0 + j) / HW; r = (p0 + j) - n * HW; } }      // (HW < 4: more than one wrap)
      off[j] = j < cnt ? (size_t)n * K * HW + r : 0;
    }
    if (cnt == 4 && (reinterpret_cast<uintptr_t>(labels + p0) & 3) == 0) {
      const u32 w = *reinterpret_cast<const u32*>(labels + p0);
#pragma unroll
      for (int j = 0; j < 4; ++j) lab[j] = (w >> (8 * j)) & 0xFF;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) lab[j] = j < cnt ? labels[p0 + j] : 0;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool valid = j < cnt && lab[j] != ignore;
      const bool badl = valid && lab[j] >= K;
      n_badl += badl;
      good[j] = valid && !badl;                                                // candidates: pass A may still find a bad probability
    }
    // pass A: is any probability of a candidate outside [0, 1]?
    bool okp[4] = {true, true, true, true};
    for (int c = 0; c < K; ++c) {
      float v[4];
      const size_t co = (size_t)c * HW;
      const float* q = probs + off[0] + co;
      if (one_frame && (reinterpret_cast<uintptr_t>(q) & 15) == 0) {
        const float4 t = *reinterpret_cast<const float4*>(q);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = j < cnt ? probs[off[j] + co] : 0.f;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) okp[j] = okp[j] && (v[j] >= 0.f && v[j] <= 1.f);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      n_badp += good[j] && !okp[j];
      good[j] = good[j] && okp[j];
      n_good += good[j];
    }
    // pass B: the counts.  Every lane of the wave runs every step (the ballots need them all).
    for (int c = 0; c < K; ++c) {
      float v[4];
      const size_t co = (size_t)c * HW;
      const float* q = probs + off[0] + co;
      if (one_frame && (reinterpret_cast<uintptr_t>(q) & 15) == 0) {
        const float4 t = *reinterpret_cast<const float4*>(q);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = j < cnt ? probs[off[j] + co] : 0.f;
      }
      int zb = 0, zf = 0, tb = 0, tf = 0;
      u32* lo_c = low + (size_t)c * 2 * S;
      u32* hi_c = hist + (size_t)c * 2 * stride;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool fg = lab[j] == c;
        const float e = fabsf((fg ? 1.f : 0.f) - v[j]);
        const u32 key = good[j] ? (u32)(e * fbins) : 0u;                       // in [0, bins]: e is in [0, 1] for a good pixel
        const bool zero = good[j] && key == 0, top = good[j] && key == (u32)bins;
        zb += __popcll(__ballot(zero && !fg));
        zf += __popcll(__ballot(zero && fg));
        tb += __popcll(__ballot(top && !fg));
        tf += __popcll(__ballot(top && fg));
        if (good[j] && !zero && !top) {
          if (key < (u32)LB) atomicAdd(lo_c + (fg ? S : 0) + key, 1u);
          else if (key >= hi0) atomicAdd(lo_c + (fg ? S : 0) + LB + (key - hi0), 1u);
          else __hip_atomic_fetch_add(hi_c + (fg ? stride : 0) + key, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (good[j] && fg) nll += (double)(-logf(v[j]));
      }
      if (lane == 0) {
        const int ts = HB ? S - 1 : bins;                                       // the slot of bin `bins`
        if (zb) atomicAdd(lo_c, (u32)zb);
        if (zf) atomicAdd(lo_c + S, (u32)zf);
        if (tb) atomicAdd(lo_c + ts, (u32)tb);
        if (tf) atomicAdd(lo_c + S + ts, (u32)tf);
      }
    }
  }

  // the workgroup's partials, lanes then waves in a fixed order
  nll = wave_sum_f64(nll);
  n_good = wave_sum(n_good); n_badl = wave_sum(n_badl); n_badp = wave_sum(n_badp);
  long long* redc = reinterpret_cast<long long*>(red + kHistWaves);
  if (lane == 0) { red[wave] = nll; redc[wave * 3 + 0] = n_good; redc[wave * 3 + 1] = n_badl; redc[wave * 3 + 2] = n_badp; }
  __syncthreads();
  if (tid == 0) {
    double s = 0.0;
    long long a = 0, b = 0, d = 0;
    for (int w = 0; w < kHistWaves; ++w) { s += red[w]; a += redc[w * 3]; b += redc[w * 3 + 1]; d += redc[w * 3 + 2]; }
    part_nll[blockIdx.x] = s;
    part_cnt[blockIdx.x * 3 + 0] = a; part_cnt[blockIdx.x * 3 + 1] = b; part_cnt[blockIdx.x * 3 + 2] = d;
  }
  // flush the privatised low bins
  for (int i = tid; i < n_low; i += kHistThreads) {
    const u32 v = low[i];
    if (v) {
      const int cf = i / S, slot = i - cf * S;
      const u32 k = slot < LB ? (u32)slot : hi0 + (u32)(slot - LB);
      __hip_atomic_fetch_add(hist + (size_t)cf * stride + k, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

__global__ __launch_bounds__(kScanThreads) void vl_scan(const u32* __restrict__ hist, const double* __restrict__ part_nll,
                                                        const long long* __restrict__ part_cnt, int n_blocks, int bins,
                                                        double* __restrict__ per_class, double* __restrict__ nll_sum,
                                                        long long* __restrict__ counts) {
  double* red = reinterpret_cast<double*>(vl_dyn);                              // [kScanWaves][2] doubles
  u32* tot = reinterpret_cast<u32*>(vl_dyn + kScanWaves * 2 * sizeof(double));  // [kScanWaves][2]
  const int tid = threadIdx.x, lane = tid & (RMNET_WAVE - 1), wave = tid >> 6;
  const int c = blockIdx.x;
  const size_t stride = (size_t)bins + 1;
  const u32* hb = hist + (size_t)c * 2 * stride;      // background counts
  const u32* hf = hb + stride;                        // foreground counts
  const int seg = (bins + kScanWaves - 1) / kScanWaves;
  const int k0 = wave * seg < bins ? wave * seg : bins;
  const int k1 = k0 + seg < bins ? k0 + seg : bins;   // this wave's bins [k0, k1) of [0, bins)
  u32 sf = 0, sb = 0;
  for (int k = k0 + lane; k < k1; k += RMNET_WAVE) { sf += hf[k]; sb += hb[k]; }
  sf = (u32)wave_sum((int)sf); sb = (u32)wave_sum((int)sb);
  if (lane == 0) { tot[wave * 2] = sf; tot[wave * 2 + 1] = sb; }
  __syncthreads();
  u32 carry_f = hf[bins], carry_b = hb[bins];         // the counts of the bins above this wave's segment
  u32 G = carry_f;
  for (int w = 0; w < kScanWaves; ++w) {
    G += tot[w * 2];
    if (w > wave) { carry_f += tot[w * 2]; carry_b += tot[w * 2 + 1]; }
  }
  const double dG = (double)G;
  double acc_hi = 0.0, acc_lo = 0.0;
  if (G != 0) {
    for (int top = k1; top > k0; top -= RMNET_WAVE * kRun) {                    // (uniform over the wave)
      const int base = top - RMNET_WAVE * kRun + lane * kRun;                   // this lane's bins [base, base + kRun), below `top`
      u32 f[kRun], b[kRun], sf2 = 0, sb2 = 0;
#pragma unroll
      for (int i = 0; i < kRun; ++i) {
        const bool in = base + i >= k0;
        f[i] = in ? hf[base + i] : 0u; b[i] = in ? hb[base + i] : 0u;
        sf2 += f[i]; sb2 += b[i];
      }
      const u32 inc_f = wave_suffix(sf2, lane), inc_b = wave_suffix(sb2, lane);  // one scan over the lanes' totals per step
      u32 run_f = carry_f + inc_f - sf2, run_b = carry_b + inc_b - sb2;          // the counts of the bins above this lane's run
#pragma unroll
      for (int i = kRun - 1; i >= 0; --i) {
        const u32 fge = run_f + f[i], bge = run_b + b[i];
        if (base + i >= k0) {
          acc_hi += 1.0 - (dG - (double)fge) / (dG + (double)bge);
          acc_lo += 1.0 - (dG - (double)run_f) / (dG + (double)run_b);
        }
        run_f = fge; run_b = bge;
      }
      carry_f += __shfl(inc_f, 0); carry_b += __shfl(inc_b, 0);                 // lane 0 holds the step's whole sum
    }
  }
  acc_hi = wave_sum_f64(acc_hi); acc_lo = wave_sum_f64(acc_lo);
  if (lane == 0) { red[wave * 2] = acc_hi; red[wave * 2 + 1] = acc_lo; }
  __syncthreads();
  if (tid == 0) {
    double hi = 0.0, lo = 0.0;
    for (int w = 0; w < kScanWaves; ++w) { hi += red[w * 2]; lo += red[w * 2 + 1]; }
    per_class[c * 3 + 0] = dG;
    per_class[c * 3 + 1] = lo / (double)bins;
    per_class[c * 3 + 2] = hi / (double)bins;
    if (c == 0) {
      double s = 0.0;
      long long a = 0, b = 0, d = 0;
      for (int i = 0; i < n_blocks; ++i) { s += part_nll[i]; a += part_cnt[i * 3]; b += part_cnt[i * 3 + 1]; d += part_cnt[i * 3 + 2]; }
      nll_sum[0] = s;
      counts[0] = a; counts[1] = b; counts[2] = d;
    }
  }
}

}  // namespace

size_t clip_loss_ws_bytes(int K, int bins) {
  if (K < 1 || K > 255 || !bins_ok(bins)) return 0;
  return partial_offset(K, bins) + (size_t)kMaxBlocks * (sizeof(double) + 3 * sizeof(long long));
}

int launch_clip_hist(const float* probs, const uint8_t* labels, int N, int K, int H, int W, int ignore_index, int bins, double* per_class,
                     double* nll_sum, long long* counts, void* ws, size_t ws_bytes, hipStream_t st, int* n_blocks) {
  if (!probs || !labels || !per_class || !nll_sum || !counts || N <= 0 || H <= 0 || W <= 0) return RMNET_E_INVALID_ARG;
  if (K < 1 || K > 255 || !bins_ok(bins)) return RMNET_E_INVALID_ARG;
  const long long HW = (long long)H * W, P = HW * N;
  if (P >= (1LL << 31)) return RMNET_E_UNSUPPORTED;
  if (!ws || ws_bytes < clip_loss_ws_bytes(K, bins)) return RMNET_E_WORKSPACE;
  if ((reinterpret_cast<uintptr_t>(ws) & 7) || (reinterpret_cast<uintptr_t>(probs) & 3) || (reinterpret_cast<uintptr_t>(per_class) & 7) ||
      (reinterpret_cast<uintptr_t>(nll_sum) & 7) || (reinterpret_cast<uintptr_t>(counts) & 7))
    return RMNET_E_INVALID_ARG;
  const int ignore = ignore_index >= 0 && ignore_index <= 255 ? ignore_index : 256;      // 256 is no label: nothing is ignored
  int LB, HB;
  lds_bins(K, bins, &LB, &HB);
  u32* hist = static_cast<u32*>(ws);
  double* part_nll = reinterpret_cast<double*>(static_cast<unsigned char*>(ws) + partial_offset(K, bins));
  long long* part_cnt = reinterpret_cast<long long*>(part_nll + kMaxBlocks);
  long long groups, blocks, per_block;
  stream_grid(P, &groups, &blocks, &per_block);
  if (hipMemsetAsync(hist, 0, hist_words(K, bins) * sizeof(u32), st) != hipSuccess) return RMNET_E_LAUNCH;
  const size_t lds1 = (size_t)K * 2 * (LB + HB) * sizeof(u32) + kHistWaves * (sizeof(double) + 3 * sizeof(long long));
  hipLaunchKernelGGL(vl_hist, dim3((unsigned)blocks), dim3(kHistThreads), lds1, st, probs, labels, hist, part_nll, part_cnt, P, HW, K,
                     ignore, bins, LB, HB, groups, per_block);
  *n_blocks = (int)blocks;
  return RMNET_OK;
}

int launch_clip_loss(const float* probs, const uint8_t* labels, int N, int K, int H, int W, int ignore_index, int bins, double* per_class,
                     double* nll_sum, long long* counts, void* ws, size_t ws_bytes, hipStream_t st) {
  int blocks = 0;
  const int rc = launch_clip_hist(probs, labels, N, K, H, W, ignore_index, bins, per_class, nll_sum, counts, ws, ws_bytes, st, &blocks);
  if (rc != RMNET_OK) return rc;
  const u32* hist = static_cast<const u32*>(ws);
  const double* part_nll = reinterpret_cast<const double*>(static_cast<const unsigned char*>(ws) + partial_offset(K, bins));
  const long long* part_cnt = reinterpret_cast<const long long*>(part_nll + kMaxBlocks);
  const size_t lds2 = kScanWaves * 2 * (sizeof(double) + sizeof(u32));
  hipLaunchKernelGGL(vl_scan, dim3((unsigned)K), dim3(kScanThreads), lds2, st, hist, part_nll, part_cnt, blocks, bins, per_class,
                     nll_sum, counts);
  return check_launch();
}

}  // namespace rmnet
