// split_f16.h -- the vocabulary that every split-fp16 convolution kernel shares (conv3x3, conv3x3_rows, conv_split, conv_rows, stem,
// flow_conv, flow_stem): the native vector types, the K step and workgroup size, the activation scale and fp16 window, the LDS swizzle
// of the per-tap kernels, the per-element split, and the byte-range overlap test of the argument rules.  Nothing about a particular
// kernel's tiles or row images belongs here (the tap-row engine's: conv_rows_core.h).
#pragma once

#include "common.h"

namespace rmnet {
namespace {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));   // 16 bytes of packed halves.  A native vector: an array of HIP's
                                                                    // uint4 (a struct) is not kept in registers but placed in LDS

constexpr int kKT = 32;          // K per step (one tap x 32 input channels)
constexpr int kThreads = 512;
constexpr float kActScale = 64.0f;                 // 2^6
constexpr float kActUnscale = 1.0f / 64.0f;
constexpr float kF16Max = 65504.0f;

// [row][32 halves] images (64-B rows); the 16-byte chunk index is XOR-swizzled with row bits 1..2 so that the fragment reads
// (16 rows x 4 chunks per 64 lanes) and the tile writes spread over all banks.
__device__ inline int swz(int row, int chunk) { return row * kKT + ((chunk ^ ((row >> 1) & 3)) << 3); }

// The split of four activations: c = clamp(64 v), hi = fp16(c), lo = fp16(c - hi); an element outside the fp16 window (NaN included:
// it saturates to -65504) adds `count` to bad.
__device__ inline void split4(const f32x4 v, half4& hi, half4& lo, int& bad, int count = 1) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float y = v[e] * kActScale;
    bad += !(fabsf(y) <= kF16Max) ? count : 0;
    const float c = fminf(fmaxf(y, -kF16Max), kF16Max);
    const _Float16 h = (_Float16)c;
    hi[e] = h;
    lo[e] = (_Float16)(c - (float)h);
  }
}

inline bool overlap(const void* p, long long pn, const void* q, long long qn) {
  const char* a = reinterpret_cast<const char*>(p);
  const char* b = reinterpret_cast<const char*>(q);
  return a < b + qn && b < a + pn;
}

}  // namespace
}  // namespace rmnet
