// val_loss_parts.h -- what val_loss.hip (the value of the loss) and val_loss_bwd.hip (its gradient) share: the workspace layout,
// the rule for the bins kept in LDS, the launch geometry of the streaming pass and the two fixed-order wave reductions.
#pragma once
#include "common.h"

namespace rmnet {
namespace vl {

typedef unsigned int u32;

constexpr int kHistThreads = 512;
constexpr int kHistWaves = kHistThreads / RMNET_WAVE;
constexpr int kMaxBlocks = 512;
constexpr int kLdsWords = 15872;                  // 62 KB of privatised bins
constexpr int kScanThreads = 1024;
constexpr int kScanWaves = kScanThreads / RMNET_WAVE;
constexpr int kRun = 16;                          // consecutive bins per lane and step of the scan's second pass
constexpr int kMinBins = 2, kMaxBins = 1 << 22;

inline bool bins_ok(int bins) { return bins >= kMinBins && bins <= kMaxBins && (bins & (bins - 1)) == 0; }

// the bins kept in LDS: [0, LB) and [bins + 1 - HB, bins]
inline void lds_bins(int K, int bins, int* LB, int* HB) {
  int s = 1;
  while (2 * s * 2 * K <= kLdsWords) s *= 2;
  if (bins + 1 <= s) { *LB = bins + 1; *HB = 0; } else { *LB = s / 2; *HB = s / 2; }
}

inline size_t hist_words(int K, int bins) { return (size_t)K * 2 * ((size_t)bins + 1); }
inline size_t partial_offset(int K, int bins) { return (hist_words(K, bins) * sizeof(u32) + 7) & ~(size_t)7; }

// the streaming pass: groups of 4 pixels, a workgroup over `per_block` contiguous groups (whole steps of kHistThreads)
inline void stream_grid(long long P, long long* groups, long long* blocks, long long* per_block) {
  *groups = (P + 3) / 4;
  long long b = (*groups + kHistThreads - 1) / kHistThreads;
  if (b > kMaxBlocks) b = kMaxBlocks;
  long long pb = (*groups + b - 1) / b;
  pb = (pb + kHistThreads - 1) / kHistThreads * kHistThreads;              // whole steps: a wave's groups stay contiguous
  *per_block = pb;
  *blocks = (*groups + pb - 1) / pb;
}

__device__ inline double wave_sum_f64(double v) {      // xor tree: the same order in every call
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// inclusive suffix sum over the wave: lane l gets the sum of lanes l .. 63
__device__ inline u32 wave_suffix(u32 v, int lane) {
#pragma unroll
  for (int o = 1; o < RMNET_WAVE; o <<= 1) {
    const u32 t = __shfl_down(v, o);
    if (lane + o < RMNET_WAVE) v += t;
  }
  return v;
}

}  // namespace vl

// val_loss.hip: the argument rules of rmnet_clip_loss_f32, then the memset and vl_hist on `st`; *n_blocks workgroups wrote partials
int launch_clip_hist(const float* probs, const uint8_t* labels, int N, int K, int H, int W, int ignore_index, int bins, double* per_class,
                     double* nll_sum, long long* counts, void* ws, size_t ws_bytes, hipStream_t st, int* n_blocks);

}  // namespace rmnet
