// conv3x3_rows.hip -- the decoder's 3x3 / stride 1 / pad 1 convolution with Cin = Cout = 256 (csrc/conv3x3.hip's arithmetic,
// arguments and results, bit for bit), on the tap-row engine of csrc/conv_rows_core.h (read its header first): C = 256, MT = 128,
// wave w owns all 128 pixels x channels 32w .. 32w+31.
//
// How it differs from the two kernels of conv3x3.hip.  Those walk K = (tap, channel block) with an LDS tile of one tap x 32
// channels: every activation is fetched, ReLU'd, scaled, clamped, split and written to LDS nine times, once per tap, and every one
// of the 72 K steps ends in a workgroup barrier.  Here a tap row of 130 pixels x 256 channels x (hi + lo) is staged once (3 times
// per workgroup instead of 9, and 3 x 130 instead of 9 x 128 pixel rows of global traffic), and its 24 K steps run without a global
// activation load, a split, an LDS write or a barrier: six barriers per workgroup instead of 72.
//
// What this file adds to the engine:
//   * staging from fp32: the per-element expression of the per-tap loader (optional ReLU, * 64, range test, clamp, hi = fp16(c),
//     lo = fp16(c - hi)) without its border select (the engine masks at the fragment reads).  The range count is taken while the
//     centre row (dy = 0) is staged, for the workgroup's own pixels only: each element once.  The staging writes (ds_write_b64:
//     groups of 16 lanes = 2 consecutive rows x 64 B) are conflict-free under the engine's swizzle.
// The argument struct, the argument rules and the epilogue (residual, ReLU, fp32 store, range word) are conv3x3.hip's kernels' own
// text: csrc/conv3x3_parts.h.
// Only Cin = 256 fits with the K order kept (Cin = 512 would need 266 KB); other shapes stay on conv3x3.hip's kernels.
// Measured: profiles/r20_a_conv3x3_rows.md.
#include "conv3x3_parts.h"
#include "conv_rows_core.h"

namespace rmnet {
namespace {

constexpr int kCin = 256;        // input channels (fixed: the row image is sized for it)
constexpr int kRowsLdsBytes = rows_image_bytes(kCin, kMT);
static_assert(kRowsLdsBytes == 137216, "8 blocks x 2 planes x 134 rows x 64 B");
static_assert(kRowsLdsBytes <= kLdsBytesPerCU, "LDS budget");
constexpr int kStageBatch = 8;                     // staging loads in flight per thread before the first split (16: the same time)
constexpr int kStagePasses = kMT / 8;              // full staging passes: 8 rows x 256 channels per pass and workgroup

__global__ __launch_bounds__(kThreads) void conv3x3_rows(ConvArgs a) {
  using Core = RowsCore<kCin, kMT>;
  constexpr int kPlaneHalves = Core::kPlaneHalves, kBlockHalves = Core::kBlockHalves;
  _Float16* const lds = rows_lds;
  const int tid = threadIdx.x, wave = tid >> 6;
  const int m0 = blockIdx.x * kMT;
  Core core;
  core.begin(tid, wave, 0, m0, a.wp, a.M, a.H, a.W);

  // staging items: thread -> (row 2 * (tid / 128) + (tid / 8) % 2 of each pass of 8 rows, channel block (tid / 16) % 8, channels
  // 4 * (tid % 8) .. of it): 8 lanes read 128 contiguous bytes, 16 lanes write two consecutive 64-byte LDS rows
  const int srow = 2 * (tid >> 7) + ((tid >> 3) & 1);
  const int sj = tid & 7;
  const unsigned scol = ((tid >> 4) & 7) * kKT + 4 * sj;
  _Float16* const sdst = lds + ((tid >> 4) & 7) * kBlockHalves + swzr(srow, sj >> 1) + 4 * (sj & 1);   // + 8 rows per pass: the swizzle bit stays
  int bad = 0;
  // RELU: a.relu_in; CENTRE: the tap row is dy = 0 (the one that counts) -- both uniform over a tap row
  auto split_store = [&](auto relu, auto centre, f32x4 x4, int row, int qb) __attribute__((always_inline)) {
    const int own = row >= 1 && row <= kMT && qb + row < a.M ? 1 : 0;      // (centre row: staged row r is pixel m0 - 1 + r)
    if constexpr (decltype(relu)::value) {
#pragma unroll
      for (int e = 0; e < 4; ++e) x4[e] = x4[e] < 0.0f ? 0.0f : x4[e];       // (keeps NaN: it is counted below)
    }
    half4 hi, lo;
    split4(x4, hi, lo, bad, decltype(centre)::value ? own : 0);
    _Float16* d = sdst + (row - srow) * kKT;
    *reinterpret_cast<half4*>(d) = hi;
    *reinterpret_cast<half4*>(d + kPlaneHalves) = lo;
  };
  auto stage = [&](auto relu, auto centre, int ty) __attribute__((always_inline)) {
    int qb = m0 + (ty - 1) * a.W - 1;                     // the pixel of staged row 0
    asm volatile("" : "+s"(qb));                          // (opaque: for the centre row it is loop-invariant, and the 17 addresses
                                                          // and flags derived from it would be hoisted in front of the K loop and spilled)
    auto src = [&](int row) {
      const int q = min(max(qb + row, 0), a.M - 1);       // (outside the tensor: any pixel inside it; all its readers are masked)
      return reinterpret_cast<const f32x4*>(a.x + ((unsigned)q * kCin + scol));
    };
    // the loads of kStageBatch passes (all 8 channel blocks of 64 rows) are in flight before the first split
#pragma unroll
    for (int g = 0; g < kStagePasses / kStageBatch; ++g) {
      f32x4 v[kStageBatch];
#pragma unroll
      for (int k = 0; k < kStageBatch; ++k) v[k] = *src(srow + 8 * (kStageBatch * g + k));
#pragma unroll
      for (int k = 0; k < kStageBatch; ++k) split_store(relu, centre, v[k], srow + 8 * (kStageBatch * g + k), qb);
    }
    if (tid < 128) {                                      // rows 128, 129 (waves 0 and 1)
      const f32x4 v = *src(srow + kMT);
      split_store(relu, centre, v, srow + kMT, qb);
    }
  };

  // the K loop: three tap rows; the engine loaded the first step's weight fragments in begin()
#pragma unroll 1
  for (int ty = 0; ty < 3; ++ty) {
    __syncthreads();                                         // the readers of the row image have finished
    if (a.relu_in) {
      if (ty == 1)
        stage(Flag<true>{}, Flag<true>{}, ty);
      else
        stage(Flag<true>{}, Flag<false>{}, ty);
    } else {
      if (ty == 1)
        stage(Flag<false>{}, Flag<true>{}, ty);
      else
        stage(Flag<false>{}, Flag<false>{}, ty);
    }
    __syncthreads();
#pragma unroll 1
    for (int tx = 0; tx < 3; ++tx) core.run_tap(3 * ty + tx);
  }

  // the epilogue: pixels m0 + 16i + fr, channels 32*wave + 16j + 4*fc ..
  int me = m0;                                               // (opaque: the pixel indices are formed again here; taken from the
  asm volatile("" : "+s"(me));                               // mask computation they stay live across the K loop and spill)
  conv3x3_epilogue(a, core.acc, core.accx, me + core.fr, wave * 32 + 4 * core.fc, bad);
}

}  // namespace
}  // namespace rmnet

extern "C" int rmnet_conv3x3_rows_f32(const float* x, const void* wpack, const float* w_unscale, const float* bias, const float* res,
                                      int flags, int N, int H, int W, int Cin, float* out, int32_t* range_word, void* stream) {
  using namespace rmnet;
  ConvArgs a;
  int rc = conv3x3_args(a, x, wpack, w_unscale, bias, res, flags, N, H, W, Cin, out, range_word);
  if (rc != RMNET_OK) return rc;
  if (Cin != kCin) return RMNET_E_UNSUPPORTED;              // the row image holds exactly 256 channels
  rc = rows_prepare<conv3x3_rows, kRowsLdsBytes>((hipStream_t)stream);
  if (rc != RMNET_OK) return rc;
  hipLaunchKernelGGL(conv3x3_rows, dim3((unsigned)((a.M + kMT - 1) / kMT)), dim3(kThreads), kRowsLdsBytes, (hipStream_t)stream, a);
  return check_launch();
}
