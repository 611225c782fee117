// val_loss_bwd.hip -- the gradient of the training loss of core/train.py:180, Lovasz-softmax + NLL, with respect to the
// probabilities, from the same two integer histograms per class that give its value (val_loss.hip) and again without a sort.
//
// Sorted by descending error e = |fg - p_c|, with G the class's foreground count and F / B the foreground / background pixels
// strictly before a pixel, the reference's _lovasz_grad gives a foreground pixel the weight 1 / (G + B) and a background pixel
// (G - F) / ((G + B)(G + B + 1)); the weights carry no gradient (the permutation is detached), so dL_c / dp_c = s * weight with
// s = -1 on a foreground pixel, +1 on a background pixel and 0 where e == 0 (the derivative torch gives abs at 0).  The histogram
// ties the pixels of one bin.  With F>, B> the counts of the bins above k and F>=, B>= those of the bins at or above k, the table is
// the mean of the two tie orders "the bin's foregrounds first" and "the bin's backgrounds first", pixels of one kind sharing their
// mean (the background sum telescopes):
//   g_fg[c][k] = (1 / (G + B>) + 1 / (G + B>=)) / 2          g_bg[c][k] = (G - (F> + F>=) / 2) / ((G + B>)(G + B>=))
// The bin's pixels together carry J(>= k) - J(> k), a present class's weights add up to 1, and the table is the sort's gradient
// exactly where no bin of the class holds more than one pixel.  The gradient with respect to probs[n, c, y, x] is
//   s * g_kind[c][key] / n_present + [c == label] * (-1 / (p_label * n_good)),
// 0 in all K channels of a pixel that is ignored or bad (label >= K, a probability outside [0, 1] or NaN): the pixels the value
// leaves out.  An absent class has an all-zero table.
//
// vl_hist (val_loss.hip) is launched unchanged.  vl_grad_table is vl_scan with two more outputs per bin: the same segments, the same
// wave-wide suffix scan and the same float64 sums in the same order, so per_class, nll_sum and counts get the bits that
// rmnet_clip_loss_f32 gives them; where vl_scan only adds the two Riemann terms of a bin, this kernel also writes the bin's two
// table entries OVER the bin's two counts (float32 bits in the u32 slots: the table has the histogram's shape, and a bin's counts
// are dead once the lane that scans the bin holds them in registers).  Who reads and writes what: a wave reads its own segment in
// pass 1, before any of its lanes writes; in pass 2 a lane loads its 16 bins, then stores them, and no other lane touches them; bin
// `bins` is read by every thread before the first barrier and written by thread 0 after the last one.  Each entry is computed in
// float64 from the integer counts -- G + B, F> + F>= and its half are exact; the reciprocals, their sum, the product of the two
// unions and the quotient round once each -- and rounded once to float32.
//
// vl_grad_apply: vl_hist's streaming pass (groups of 4 pixels, 16-byte loads and stores where the group lies in one frame and the
// address is aligned, element accesses elsewhere; pass A decides whether a pixel is bad, pass B reads the probabilities again),
// with a table gather in place of the histogram add and a store of the gradient.  The LB lowest and HB highest entries of every
// class's tables are staged in dynamic LDS by lds_bins' rule (LB = HB = 0: every gather goes to memory; the two are measured in
// profiles/r34_a_loss_grad.md).  n_present and n_good are read from per_class and counts on the device.  No atomics; every element
// of grad is written exactly once, zeros included, so the caller never pre-zeros and two calls give the same bits.
//
// One rounding per operation: contraction is off for this translation unit (HIP's __fmul_rn / __fadd_rn are header functions and
// fuse all the same, flow_affine.hip), and the per-element arithmetic is written as plain operators, in fp32:
//   e = |fg - p|;  key = (unsigned)(e * bins);  w = (s * g) * inv_present;  grad = w            (s * g is exact)
//   on the label's channel  grad = w + (float)(-1.0 / ((double)p * (double)n_good))             (the product and the quotient in float64)
// with inv_present = (float)(1.0 / (double)n_present).
#include "val_loss_parts.h"

#pragma clang fp contract(off)

namespace rmnet {
namespace {

using namespace vl;

// 1: vl_grad_apply stages the lowest and highest table entries in LDS; 0: plain cached gathers.  The default is what measured
// faster (profiles/r34_a_loss_grad.md); tools/loss_grad_bench.py builds the other one with -DRMNET_VL_GRAD_STAGE=... to compare.
#ifndef RMNET_VL_GRAD_STAGE
#define RMNET_VL_GRAD_STAGE 1
#endif

extern __shared__ __align__(8) unsigned char vlb_dyn[];

__device__ inline float table_fg(double dG, double bgt, double bge) {
  const double a = dG + bgt, b = dG + bge;                       // exact: integers below 2^33
  return (float)((1.0 / a + 1.0 / b) * 0.5);
}
__device__ inline float table_bg(double dG, double fgt, double fge, double bgt, double bge) {
  const double a = dG + bgt, b = dG + bge;
  return (float)((dG - (fgt + fge) * 0.5) / (a * b));            // the numerator is exact (half-integers below 2^34)
}

__global__ __launch_bounds__(kScanThreads) void vl_grad_table(u32* hist, const double* __restrict__ part_nll,
                                                              const long long* __restrict__ part_cnt, int n_blocks, int bins,
                                                              double* __restrict__ per_class, double* __restrict__ nll_sum,
                                                              long long* __restrict__ counts) {
  double* red = reinterpret_cast<double*>(vlb_dyn);                              // [kScanWaves][2] doubles
  u32* tot = reinterpret_cast<u32*>(vlb_dyn + kScanWaves * 2 * sizeof(double));  // [kScanWaves][2]
  const int tid = threadIdx.x, lane = tid & (RMNET_WAVE - 1), wave = tid >> 6;
  const int c = blockIdx.x;
  const size_t stride = (size_t)bins + 1;
  u32* hb = hist + (size_t)c * 2 * stride;            // background counts, then the background table
  u32* hf = hb + stride;                              // foreground counts, then the foreground table
  const int seg = (bins + kScanWaves - 1) / kScanWaves;
  const int k0 = wave * seg < bins ? wave * seg : bins;
  const int k1 = k0 + seg < bins ? k0 + seg : bins;   // this wave's bins [k0, k1) of [0, bins)
  u32 sf = 0, sb = 0;
  for (int k = k0 + lane; k < k1; k += RMNET_WAVE) { sf += hf[k]; sb += hb[k]; }
  sf = (u32)wave_sum((int)sf); sb = (u32)wave_sum((int)sb);
  if (lane == 0) { tot[wave * 2] = sf; tot[wave * 2 + 1] = sb; }
  const u32 top_f = hf[bins], top_b = hb[bins];       // read by every thread before the barrier, overwritten after the last one
  __syncthreads();
  u32 carry_f = top_f, carry_b = top_b;               // the counts of the bins above this wave's segment
  u32 G = carry_f;
  for (int w = 0; w < kScanWaves; ++w) {
    G += tot[w * 2];
    if (w > wave) { carry_f += tot[w * 2]; carry_b += tot[w * 2 + 1]; }
  }
  const double dG = (double)G;
  double acc_hi = 0.0, acc_lo = 0.0;
  for (int top = k1; top > k0; top -= RMNET_WAVE * kRun) {                      // (uniform over the wave)
    const int base = top - RMNET_WAVE * kRun + lane * kRun;                     // this lane's bins [base, base + kRun), below `top`
    u32 f[kRun], b[kRun], sf2 = 0, sb2 = 0;
#pragma unroll
    for (int i = 0; i < kRun; ++i) {
      const bool in = base + i >= k0;
      f[i] = in ? hf[base + i] : 0u; b[i] = in ? hb[base + i] : 0u;
      sf2 += f[i]; sb2 += b[i];
    }
    const u32 inc_f = wave_suffix(sf2, lane), inc_b = wave_suffix(sb2, lane);    // one scan over the lanes' totals per step
    u32 run_f = carry_f + inc_f - sf2, run_b = carry_b + inc_b - sb2;            // the counts of the bins above this lane's run
#pragma unroll
    for (int i = kRun - 1; i >= 0; --i) {
      const u32 fge = run_f + f[i], bge = run_b + b[i];
      if (base + i >= k0) {
        float gf = 0.f, gb = 0.f;                                               // an absent class: an all-zero table
        if (G != 0) {
          acc_hi += 1.0 - (dG - (double)fge) / (dG + (double)bge);
          acc_lo += 1.0 - (dG - (double)run_f) / (dG + (double)run_b);
          gf = table_fg(dG, (double)run_b, (double)bge);
          gb = table_bg(dG, (double)run_f, (double)fge, (double)run_b, (double)bge);
        }
        hf[base + i] = __float_as_uint(gf);
        hb[base + i] = __float_as_uint(gb);
      }
      run_f = fge; run_b = bge;
    }
    carry_f += __shfl(inc_f, 0); carry_b += __shfl(inc_b, 0);                   // lane 0 holds the step's whole sum
  }
  acc_hi = wave_sum_f64(acc_hi); acc_lo = wave_sum_f64(acc_lo);
  if (lane == 0) { red[wave * 2] = acc_hi; red[wave * 2 + 1] = acc_lo; }
  __syncthreads();
  if (tid == 0) {
    // bin `bins` (e == 1 alone): nothing lies above it
    hf[bins] = __float_as_uint(G != 0 ? table_fg(dG, 0.0, (double)top_b) : 0.f);
    hb[bins] = __float_as_uint(G != 0 ? table_bg(dG, 0.0, (double)top_f, 0.0, (double)top_b) : 0.f);
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

__global__ __launch_bounds__(kHistThreads) void vl_grad_apply(const float* __restrict__ probs, const uint8_t* __restrict__ labels,
                                                              const float* __restrict__ table, const double* __restrict__ per_class,
                                                              const long long* __restrict__ counts, float* __restrict__ grad,
                                                              long long P, long long HW, int K, int ignore, int bins, int LB, int HB,
                                                              long long groups, long long per_block) {
  const int S = LB + HB;                                                      // slots per class and kind: [0, LB) low, [LB, S) high
  const u32 hi0 = HB ? (u32)(bins + 1 - HB) : (u32)bins + 1;                  // first high bin (none: above every key)
  float* low = reinterpret_cast<float*>(vlb_dyn);                             // [K][2][S]
  const int tid = threadIdx.x, lane = tid & (RMNET_WAVE - 1);
  const size_t stride = (size_t)bins + 1;
  const int n_low = K * 2 * S;
  for (int i = tid; i < n_low; i += kHistThreads) {
    const int cf = i / S, slot = i - cf * S;
    const u32 k = slot < LB ? (u32)slot : hi0 + (u32)(slot - LB);
    low[i] = table[(size_t)cf * stride + k];
  }
  // the present classes and the good pixels, from the device: every wave counts for itself
  int n_present = 0;
  for (int c = lane; c < K; c += RMNET_WAVE) n_present += per_class[c * 3] > 0.0;
  n_present = wave_sum(n_present);
  const float inv_present = n_present ? (float)(1.0 / (double)n_present) : 0.f;
  const double d_good = (double)counts[0];
  if (n_low) __syncthreads();                                                  // (uniform: a kernel argument)

  const long long g0 = (long long)blockIdx.x * per_block;
  const long long g1 = g0 + per_block < groups ? g0 + per_block : groups;
  const float fbins = (float)bins;

  for (long long gb = g0; gb < g1; gb += kHistThreads) {
    const long long g = gb + tid;
    if (g >= g1) continue;
    const long long p0 = g * 4;
    const int cnt = (int)(P - p0 < 4 ? P - p0 : 4);
    const long long n0 = p0 / HW, r0 = p0 - n0 * HW;
    const bool one_frame = cnt == 4 && r0 + 3 < HW;
    // class-0 element offset of each pixel; pixels past `cnt` stand on pixel p0 and are never read or written
    size_t off[4];
    int lab[4];
    bool good[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      long long r = r0 + j, n = n0;
      if (r >= HW) { r -= HW; ++n; if (r >= HW) { n = (p0 + j) / HW; r = (p0 + j) - n * HW; } }      // (HW < 4: more than one wrap)
      off[j] = j < cnt ? (size_t)n * K * HW + r : (size_t)n0 * K * HW + r0;
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
    for (int j = 0; j < 4; ++j) good[j] = j < cnt && lab[j] != ignore && lab[j] < K;
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
    for (int j = 0; j < 4; ++j) good[j] = good[j] && okp[j];
    // pass B: the gradient of every class
    for (int c = 0; c < K; ++c) {
      float v[4], o[4];
      const size_t co = (size_t)c * HW;
      const float* q = probs + off[0] + co;
      if (one_frame && (reinterpret_cast<uintptr_t>(q) & 15) == 0) {
        const float4 t = *reinterpret_cast<const float4*>(q);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = j < cnt ? probs[off[j] + co] : 0.f;
      }
      const float* lo_c = low + (size_t)c * 2 * S;
      const float* tb_c = table + (size_t)c * 2 * stride;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        o[j] = 0.f;
        if (good[j]) {
          const bool fg = lab[j] == c;
          const float e = fabsf((fg ? 1.f : 0.f) - v[j]);
          const u32 key = (u32)(e * fbins);                                    // in [0, bins]: e is in [0, 1] for a good pixel
          float gk;
          if (key < (u32)LB) gk = lo_c[(fg ? S : 0) + key];
          else if (key >= hi0) gk = lo_c[(fg ? S : 0) + LB + (key - hi0)];
          else gk = tb_c[(fg ? stride : 0) + key];
          const float s = e == 0.f ? 0.f : (fg ? -1.f : 1.f);                  // abs has derivative 0 at 0
          float w = (s * gk) * inv_present;
          if (fg) w = w + (float)(-1.0 / ((double)v[j] * d_good));
          o[j] = w;
        }
      }
      float* dst = grad + off[0] + co;
      if (one_frame && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
        *reinterpret_cast<float4*>(dst) = make_float4(o[0], o[1], o[2], o[3]);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (j < cnt) grad[off[j] + co] = o[j];
      }
    }
  }
}

}  // namespace

size_t clip_loss_grad_ws_bytes(int K, int bins) { return clip_loss_ws_bytes(K, bins); }

int launch_clip_loss_grad(const float* probs, const uint8_t* labels, int N, int K, int H, int W, int ignore_index, int bins, float* grad,
                          double* per_class, double* nll_sum, long long* counts, void* ws, size_t ws_bytes, hipStream_t st) {
  if (!grad) return RMNET_E_INVALID_ARG;
  // the rules of the forward entry, before anything is launched; then grad's own
  if (!probs || !labels || !per_class || !nll_sum || !counts || N <= 0 || H <= 0 || W <= 0) return RMNET_E_INVALID_ARG;
  if (K < 1 || K > 255 || !bins_ok(bins)) return RMNET_E_INVALID_ARG;
  const long long HW = (long long)H * W, P = HW * N;
  if (P >= (1LL << 31)) return RMNET_E_UNSUPPORTED;
  if (reinterpret_cast<uintptr_t>(grad) & 3) return RMNET_E_INVALID_ARG;
  const uintptr_t pa = reinterpret_cast<uintptr_t>(probs), ga = reinterpret_cast<uintptr_t>(grad);
  const uintptr_t bytes = (uintptr_t)P * K * sizeof(float);
  if (pa < ga + bytes && ga < pa + bytes) return RMNET_E_INVALID_ARG;                     // grad must not overlap probs
  int blocks = 0;
  const int rc = launch_clip_hist(probs, labels, N, K, H, W, ignore_index, bins, per_class, nll_sum, counts, ws, ws_bytes, st, &blocks);
  if (rc != RMNET_OK) return rc;
  const int ignore = ignore_index >= 0 && ignore_index <= 255 ? ignore_index : 256;
  u32* hist = static_cast<u32*>(ws);
  const double* part_nll = reinterpret_cast<const double*>(static_cast<const unsigned char*>(ws) + partial_offset(K, bins));
  const long long* part_cnt = reinterpret_cast<const long long*>(part_nll + kMaxBlocks);
  const size_t lds2 = kScanWaves * 2 * (sizeof(double) + sizeof(u32));
  hipLaunchKernelGGL(vl_grad_table, dim3((unsigned)K), dim3(kScanThreads), lds2, st, hist, part_nll, part_cnt, blocks, bins, per_class,
                     nll_sum, counts);
  int LB = 0, HB = 0;
  if (RMNET_VL_GRAD_STAGE) lds_bins(K, bins, &LB, &HB);
  long long groups, nb, per_block;
  stream_grid(P, &groups, &nb, &per_block);
  const size_t lds3 = (size_t)K * 2 * (LB + HB) * sizeof(float);
  hipLaunchKernelGGL(vl_grad_apply, dim3((unsigned)nb), dim3(kHistThreads), lds3, st, probs, labels, reinterpret_cast<const float*>(hist),
                     per_class, counts, grad, P, HW, K, ignore, bins, LB, HB, groups, per_block);
  return check_launch();
}

}  // namespace rmnet
