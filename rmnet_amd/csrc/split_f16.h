// split_f16.h -- the vocabulary that every split-fp16 convolution kernel shares (conv3x3, conv3x3_rows, conv_split, conv_rows, stem,
// flow_conv, flow_stem): the native vector types, the K step and workgroup size, the activation scale and fp16 window, the LDS swizzle
// of the per-tap kernels, the per-element split, the 3x3 border test, the epilogue's head, and the byte-range overlap test of the
// argument rules.  Nothing about a particular kernel's tiles or row images belongs here (the tap-row engine's: conv_rows_core.h; the
// decoder kernels' loader, epilogue and argument rules: conv3x3_parts.h).
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

// The border test of a 3x3 / pad 1 kernel, once per pixel: bit t = tap t of pixel m (linear NHWC index) lies inside the H x W map; a
// pixel past M has no tap inside.
__device__ inline unsigned taps_inside(int m, int M, int H, int W) {
  const bool pin = m < M;
  const int r = (pin ? m : 0) % (H * W);
  const int ph = r / W, pw = r % W;
  unsigned bits = 0;
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    const int h = ph + t / 3 - 1, w = pw + t % 3 - 1;
    bits |= (pin && h >= 0 && h < H && w >= 0 && w < W ? 1u : 0u) << t;
  }
  return bits;
}

// The epilogue's head for a lane's TI x TJ accumulator tiles: acc = (acc + accx) * unscale / 64 + shift for the channels cb + 16 j ..
// (4 each), in place and for all tiles before the tail's first store: for all the compiler knows these vectors alias the output, and
// read between the stores they would cost one more waited-for round trip per channel tile.  Then an empty statement the optimiser
// cannot see through: without it the loop is sunk into the tail's guarded stores, and each tile's wait for its unscale vector then
// includes the stores issued before it.
template <int TI, int TJ>
__device__ __forceinline__ void unscale_shift(f32x4 (&acc)[TI][TJ], const f32x4 (&accx)[TI][TJ], const float* unscale, const float* shift, int cb) {
#pragma unroll
  for (int j = 0; j < TJ; ++j) {
    const f32x4 us = *reinterpret_cast<const f32x4*>(unscale + cb + 16 * j) * kActUnscale;
    const f32x4 b = shift ? *reinterpret_cast<const f32x4*>(shift + cb + 16 * j) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < TI; ++i) acc[i][j] = (acc[i][j] + accx[i][j]) * us + b;
  }
#pragma unroll
  for (int j = 0; j < TJ; ++j)
#pragma unroll
    for (int i = 0; i < TI; ++i) asm volatile("" : "+v"(acc[i][j]));
}

inline bool overlap(const void* p, long long pn, const void* q, long long qn) {
  const char* a = reinterpret_cast<const char*>(p);
  const char* b = reinterpret_cast<const char*>(q);
  return a < b + qn && b < a + pn;
}

}  // namespace
}  // namespace rmnet
