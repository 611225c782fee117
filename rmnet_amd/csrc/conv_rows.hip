// conv_rows.hip -- the trunks' 3x3 / stride 1 / pad 1 bottleneck convolutions with Cin = Cout = C in {64, 128, 256} on pre-split
// activations (csrc/conv_split.hip: conv_split_pre with RMNET_CONV_X_SPLIT -- its arithmetic, arguments and results, bit for bit),
// on the tap-row engine of csrc/conv_rows_core.h (read its header first): MT x C = 32768, i.e. MT = 128, 256, 512 for C = 256, 128,
// 64; wave w owns the pixels 128 (w / CB) .. and the channels 32 (w % CB) .., CB = C / 32.
//
// What this file adds to the engine:
//   * staging is a copy: the input is already split, and a 16-byte chunk of the split form is 8 halves of one plane -- a chunk of
//     the image.  Thread -> (chunk tid % 4, row parity tid / 4 % 2, plane tid / 8 % 2, channel block tid / 16 % CB, row pair
//     tid / 16 / CB) of each pass of 64 / CB rows, 16 passes.  A ds_write_b128 is served in groups of 8 consecutive lanes on 32
//     banks: the 8 lanes write an even row and the next (2 x 64 B, whatever the chunk swizzle does inside a row), i.e. all eight
//     16-byte slots of a 128-byte bank row -- conflict-free.  (A pixel's hi and lo chunks in one group would meet: the planes lie a
//     multiple of 128 B apart.)  4 lanes read 64 contiguous bytes, 16 lanes two pixels' 128, a wave whole 128-byte lines;
//   * nothing is counted for the input (its producer did).  The epilogue tail is conv_split_pre's, expression for expression: ReLU,
//     and for a split output split4 with its count of the produced elements outside the window.
// No residual and no second output: those calls stay on conv_split_pre.  Measured: profiles/r21_a_trunk_rows.md.
#include "conv_rows_core.h"

namespace rmnet {
namespace {

constexpr int kTileElems = 32768;                  // MT x C
constexpr int kStageBatch = 8;                     // staging loads in flight per thread before the first LDS write
constexpr int kStagePasses = 16;                   // 512 chunks per pass: MT x C / 4 chunks in 16 passes

constexpr int rows_mt(int C) { return kTileElems / C; }
constexpr int rows_lds_bytes(int C) { return rows_image_bytes(C, rows_mt(C)); }
static_assert(rows_lds_bytes(256) == 137216 && rows_lds_bytes(128) == 134144 && rows_lds_bytes(64) == 132608, "(MT + 6) rows x C x 4 B");
static_assert(rows_lds_bytes(256) <= kLdsBytesPerCU, "LDS budget");

struct RowsArgs {
  const _Float16* xs;      // [M][C / 32][2][32] fp16
  const half8* wp;         // [9][C / 32][2][C][32] fp16
  const float* unscale;    // [C]
  const float* shift;      // [C] or null
  float* out;              // OS 0: [M][C] fp32
  _Float16* outs;          // OS 1: [M][C / 32][2][32] fp16
  int* range;              // or null
  int M, H, W, relu_out;
};

template <int C, bool OS>
__global__ __launch_bounds__(kThreads) void conv_rows(RowsArgs a) {
  constexpr int MT = rows_mt(C);                     // pixels per workgroup
  using Core = RowsCore<C, MT>;
  constexpr int CB = Core::kCB, kPlaneHalves = Core::kPlaneHalves, kBlockHalves = Core::kBlockHalves;
  constexpr int kPassRows = 2 * (kThreads / 16) / CB;          // rows per staging pass
  static_assert(kPassRows % 8 == 0 && kPassRows * kStagePasses == MT, "a pass keeps the swizzle bit; 16 passes stage MT rows");
  static_assert(kStagePasses % kStageBatch == 0, "whole batches");
  _Float16* const lds = rows_lds;
  const int tid = threadIdx.x, wave = tid >> 6;
  const int wc = wave % CB, wp = wave / CB;          // the wave's channels 32 wc .., its pixels 128 wp ..
  const int m0 = blockIdx.x * MT;
  Core core;
  core.begin(tid, wc, 128 * wp, m0 + 128 * wp, a.wp, a.M, a.H, a.W);
  const int fr = core.fr, fc = core.fc;

  // staging items (see the header): row srow + kPassRows * pass, 16-byte chunk sch of plane spl of channel block sblk
  const int sch = tid & 3, spl = (tid >> 3) & 1, sblk = (tid >> 4) % CB;
  const int srow = 2 * ((tid >> 4) / CB) + ((tid >> 2) & 1);
  const unsigned scol = sblk * (2 * kKT) + spl * kKT + 8 * sch;                                     // halves inside a pixel
  _Float16* const sdst = lds + sblk * kBlockHalves + spl * kPlaneHalves + swzr(srow, sch);          // + kPassRows rows per pass: the swizzle bit stays
  auto stage = [&](int ty) __attribute__((always_inline)) {
    int qb = m0 + (ty - 1) * a.W - 1;                     // the pixel of staged row 0
    asm volatile("" : "+s"(qb));                          // (opaque: for the centre row it is loop-invariant, and the addresses derived
                                                          // from it would be hoisted in front of the K loop and spilled)
    auto src = [&](int row) {
      const int q = min(max(qb + row, 0), a.M - 1);       // (outside the tensor: any pixel inside it; all its readers are masked)
      return reinterpret_cast<const u32x4*>(a.xs + ((unsigned)q * (unsigned)(2 * C) + scol));      // (halves, below 2^32: M * C < 2^31)
    };
#pragma unroll
    for (int g = 0; g < kStagePasses / kStageBatch; ++g) {
      u32x4 v[kStageBatch];
#pragma unroll
      for (int k = 0; k < kStageBatch; ++k) v[k] = *src(srow + kPassRows * (kStageBatch * g + k));
#pragma unroll
      for (int k = 0; k < kStageBatch; ++k) *reinterpret_cast<u32x4*>(sdst + kPassRows * (kStageBatch * g + k) * kKT) = v[k];
    }
    if (tid < 16 * CB) {                                  // rows MT, MT + 1: the first row pair of one more pass
      const u32x4 v = *src(srow + MT);
      *reinterpret_cast<u32x4*>(sdst + MT * kKT) = v;
    }
  };

  // the K loop: three tap rows; the engine loaded the first step's weight fragments in begin()
#pragma unroll 1
  for (int ty = 0; ty < 3; ++ty) {
    __syncthreads();                                         // the readers of the row image have finished
    stage(ty);
    __syncthreads();
#pragma unroll 1
    for (int tx = 0; tx < 3; ++tx) core.run_tap(3 * ty + tx);
  }

  // epilogue: conv_split_pre's without the residual, expression for expression (pixel m0 + 128 wp + 16i + fr, channels
  // 32 wc + 16j + 4 fc ..)
  int me = m0 + 128 * wp;                                    // (opaque: the pixel indices are formed again here; taken from the
  asm volatile("" : "+v"(me));                               // mask computation they stay live across the K loop)
  int bad = 0;
  core.unscale_shift(a.unscale, a.shift, wc);
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int co = wc * 32 + j * 16 + 4 * fc;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int m = me + i * 16 + fr;
      if (m >= a.M) continue;
      f32x4 v = core.acc[i][j];
      if (a.relu_out) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = v[e] < 0.0f ? 0.0f : v[e];
      }
      if constexpr (OS) {
        half4 hi, lo;
        split4(v, hi, lo, bad);
        _Float16* o = a.outs + (size_t)m * (2 * C) + (co >> 5) * (2 * kKT) + (co & 31);
        *reinterpret_cast<half4*>(o) = hi;
        *reinterpret_cast<half4*>(o + kKT) = lo;
      } else {
        *reinterpret_cast<f32x4*>(a.out + (size_t)m * C + co) = v;
      }
    }
  }
  if (a.range && bad) atomicAdd(a.range, bad);
}

template <int C, bool OS>
int rows_launch(const RowsArgs& a, hipStream_t st) {
  const int rc = rows_prepare<conv_rows<C, OS>, rows_lds_bytes(C)>(st);
  if (rc != RMNET_OK) return rc;
  hipLaunchKernelGGL((conv_rows<C, OS>), dim3((unsigned)((a.M + rows_mt(C) - 1) / rows_mt(C))), dim3(kThreads), rows_lds_bytes(C), st, a);
  return check_launch();
}

}  // namespace
}  // namespace rmnet

extern "C" int rmnet_conv_rows_pre_f32(const void* x, const void* wpack, const float* w_unscale, const float* shift, const float* res,
                                       int flags, int N, int H, int W, int Cin, int Cout, int ksize, int stride, void* out, float* out2,
                                       int out_split, int32_t* range_word, void* stream) {
  using namespace rmnet;
  // rmnet_conv_split_pre_f32's argument rules (conv_split.hip), then the class this kernel serves
  if (flags & ~(RMNET_CONV_RELU_IN | RMNET_CONV_RELU_OUT | RMNET_CONV_X_SPLIT | RMNET_CONV_OUT_SPLIT)) return RMNET_E_INVALID_ARG;
  const bool xs = (flags & RMNET_CONV_X_SPLIT) != 0, os = (flags & RMNET_CONV_OUT_SPLIT) != 0;
  if (!x || !wpack || !w_unscale || !out || N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return RMNET_E_INVALID_ARG;
  if (xs && (flags & RMNET_CONV_RELU_IN)) return RMNET_E_INVALID_ARG;
  if (os && out2) return RMNET_E_INVALID_ARG;
  if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(wpack) | reinterpret_cast<uintptr_t>(w_unscale) |
       reinterpret_cast<uintptr_t>(shift) | reinterpret_cast<uintptr_t>(res) | reinterpret_cast<uintptr_t>(out) |
       reinterpret_cast<uintptr_t>(out2)) & 15)
    return RMNET_E_INVALID_ARG;
  if (out2 && (res || out_split <= 0 || out_split >= Cout || out_split % 4)) return RMNET_E_INVALID_ARG;
  if (!xs || ksize != 3 || stride != 1 || Cin != Cout || (Cin != 64 && Cin != 128 && Cin != 256) || res || out2) return RMNET_E_UNSUPPORTED;
  const long long M = (long long)N * H * W;
  if (M * Cin >= (1LL << 31)) return RMNET_E_UNSUPPORTED;   // (int pixel index, 32-bit offsets in halves)
  if (overlap(out, M * Cout * 4, x, M * Cin * 4)) return RMNET_E_INVALID_ARG;      // (either form has 4 bytes per element)
  RowsArgs a;
  a.xs = reinterpret_cast<const _Float16*>(x); a.wp = reinterpret_cast<const half8*>(wpack); a.unscale = w_unscale; a.shift = shift;
  a.out = os ? nullptr : reinterpret_cast<float*>(out); a.outs = os ? reinterpret_cast<_Float16*>(out) : nullptr;
  a.range = range_word; a.M = (int)M; a.H = H; a.W = W;
  a.relu_out = (flags & RMNET_CONV_RELU_OUT) != 0;
  hipStream_t st = (hipStream_t)stream;
  if (Cin == 256) return os ? rows_launch<256, true>(a, st) : rows_launch<256, false>(a, st);
  if (Cin == 128) return os ? rows_launch<128, true>(a, st) : rows_launch<128, false>(a, st);
  return os ? rows_launch<64, true>(a, st) : rows_launch<64, false>(a, st);
}
