// conv3x3_parts.h -- what the decoder's three 256-output 3x3 kernels share, once: conv3x3_split and conv3x3_wreg (csrc/conv3x3.hip)
// and conv3x3_rows (csrc/conv3x3_rows.hip).  The three must return the same bits; the argument struct, the argument rules, the
// per-tap activation loader of the first two, the tap-class dispatch and the fp32 epilogue are therefore one text.  (The border test
// and the epilogue's head are shared with the trunk kernels too and live in split_f16.h.)  The kernels keep what differs: who owns
// which tile, where the weights wait, and the K loop with its scheduling directives.
#pragma once

#include <type_traits>

#include "split_f16.h"

namespace rmnet {
namespace {

constexpr int kCout = 256;       // output channels (fixed)
constexpr int kMT = 128;         // pixels per workgroup

template <bool B>
using Flag = std::bool_constant<B>;

struct ConvArgs {
  const float* x;          // [M][Cin]
  const half8* wp;         // [9 * Cin / 32][2][256][32] fp16
  const float* w_unscale;  // [256]
  const float* bias;       // [256] or null
  const float* res;        // [M][256] or null
  float* out;              // [M][256]
  int* range;              // or null
  int M, H, W, Cin, relu_in, relu_out;
};

// The argument rules of all three exports; fills `a` when they hold.  Everything that is INVALID_ARG but the overlap first, then what
// is UNSUPPORTED, then the overlap (it needs the sizes).
inline int conv3x3_args(ConvArgs& a, const float* x, const void* wpack, const float* w_unscale, const float* bias, const float* res,
                        int flags, int N, int H, int W, int Cin, float* out, int32_t* range_word) {
  if (!x || !wpack || !w_unscale || !out || N <= 0 || H <= 0 || W <= 0 || Cin <= 0) return RMNET_E_INVALID_ARG;
  if (flags & ~(RMNET_CONV_RELU_IN | RMNET_CONV_RELU_OUT)) return RMNET_E_INVALID_ARG;
  if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(wpack) | reinterpret_cast<uintptr_t>(w_unscale) |
       reinterpret_cast<uintptr_t>(bias) | reinterpret_cast<uintptr_t>(res) | reinterpret_cast<uintptr_t>(out)) & 15)
    return RMNET_E_INVALID_ARG;
  if (Cin % kKT) return RMNET_E_UNSUPPORTED;
  const long long M = (long long)N * H * W;
  if (M * (long long)(Cin > kCout ? Cin : kCout) >= (1LL << 31)) return RMNET_E_UNSUPPORTED;   // (int pixel index, size_t offsets)
  // out must not overlap x (other workgroups read x's halo); it may BE res: each element is read, then written, by one thread.  The
  // epilogue reads all of a thread's residual values before its first store; a thread reads exactly the elements it later writes
  // and no other thread touches them, so that is safe as well
  if (overlap(out, M * kCout * sizeof(float), x, M * Cin * sizeof(float))) return RMNET_E_INVALID_ARG;
  a.x = x; a.wp = reinterpret_cast<const half8*>(wpack); a.w_unscale = w_unscale; a.bias = bias; a.res = res; a.out = out;
  a.range = range_word; a.M = (int)M; a.H = H; a.W = W; a.Cin = Cin;
  a.relu_in = (flags & RMNET_CONV_RELU_IN) != 0;
  a.relu_out = (flags & RMNET_CONV_RELU_OUT) != 0;
  return RMNET_OK;
}

// The per-tap activation loader of conv3x3_split and conv3x3_wreg: 2 x float4 per thread and K step (pixel p = tid/8 + 64i of the
// workgroup's 128, channels 4*(tid&7) .. of the step's 32).
// K is walked tap by tap, and inside a tap channel block by channel block.  What depends on the tap alone is set once per tap:
// whether the pixel's tap lies inside the map, and the address of its first channel block.  A tap outside the map reads the
// pixel itself instead (an address inside the tensor, whatever the tap) and the loaded values are replaced by zeros, so the load
// has no branch.  Per step only the uniform base moves, by 32 channels.
struct TapLoader {
  const ConvArgs& a;
  int tid, c4;
  int pm[2];               // the pixel (0 past M)
  unsigned inside[2];      // taps_inside() of it: the border test, once per pixel
  f32x4 xr[2];             // the step's loaded values
  const float* xb;         // a.x + the channel block (uniform)
  unsigned xo[2];          // the tap's pixel x Cin + the thread's channels, in elements (M x Cin < 2^31)
  bool in[2];
  int bad;                 // elements outside the fp16 window, counted at the centre tap

  __device__ __forceinline__ void begin(int tid_, int m0) {
    tid = tid_, c4 = tid_ & 7, bad = 0;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int m = m0 + (tid >> 3) + 64 * i;
      pm[i] = m < a.M ? m : 0;
      inside[i] = taps_inside(m, a.M, a.H, a.W);
    }
  }
  __device__ __forceinline__ void set_tap(int tap) {
    const int d = (tap / 3 - 1) * a.W + (tap % 3 - 1);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      in[i] = (inside[i] >> tap) & 1;
      xo[i] = (unsigned)(pm[i] + (in[i] ? d : 0)) * a.Cin + 4 * c4;
    }
    xb = a.x;
  }
  __device__ __forceinline__ void load() {
#pragma unroll
    for (int i = 0; i < 2; ++i) xr[i] = *reinterpret_cast<const f32x4*>(xb + xo[i]);
    xb += kKT;
  }
  // the loaded values, split, into the X hi / lo planes [128][32] at buf.  RELU: a.relu_in, CENTRE: the tap is the centre tap (the
  // one that counts) -- both uniform over a tap, so the element loop has neither test.  (The loop is written out: with split4() in
  // its place the compiler gives other code, as it did in conv_split's fp32 branch.)
  template <bool RELU, bool CENTRE>
  __device__ __forceinline__ void store(_Float16* buf) {
    _Float16* xh = buf;
    _Float16* xl = buf + kMT * kKT;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      half4 hi, lo;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float v = in[i] ? xr[i][e] : 0.0f;
        if constexpr (RELU) v = v < 0.0f ? 0.0f : v;          // (keeps NaN: it is counted below)
        const float y = v * kActScale;
        if constexpr (CENTRE) bad += !(fabsf(y) <= kF16Max) ? 1 : 0;
        const float c = fminf(fmaxf(y, -kF16Max), kF16Max);   // NaN -> -65504 (saturated, counted)
        const _Float16 h = (_Float16)c;
        hi[e] = h;
        lo[e] = (_Float16)(c - (float)h);
      }
      const int p = (tid >> 3) + 64 * i;
      const int o = swz(p, c4 >> 1) + 4 * (c4 & 1);
      *reinterpret_cast<half4*>(xh + o) = hi;
      *reinterpret_cast<half4*>(xl + o) = lo;
    }
  }
};

// The tap classes: run_taps(relu, centre, t0, t1) for taps 0 .. 3, the centre tap (the one that counts), taps 5 .. 8, one after the
// other, and all of it once with and once without the input ReLU -- the loop instances that the loader's store<> is compiled into.
template <class RunTaps>
__device__ __forceinline__ void run_tap_classes(int relu_in, RunTaps&& run_taps) {
  auto run = [&](auto relu) __attribute__((always_inline)) {
    run_taps(relu, Flag<false>{}, 0, 4);
    run_taps(relu, Flag<true>{}, 4, 5);
    run_taps(relu, Flag<false>{}, 5, 9);
  };
  if (relu_in)
    run(Flag<true>{});
  else
    run(Flag<false>{});
}

// The fp32 epilogue of a lane that holds TI x TJ MFMA tiles D[co][px]: pixels mb + 16 i (mb = the lane's first pixel, tile base + fr)
// and the 4 consecutive channels cb + 16 j .. (cb = the lane's first channel, tile base + 4 fc), i.e. one float4 of NHWC memory per
// tile.
// The residual: out may BE res, so the compiler keeps every read of res in front of the stores that follow it in the source.
// All reads are therefore issued here, before the first store (one round trip, not TI x TJ dependent ones; the K loop's registers
// are dead by now).  This is safe with out == res: a thread reads exactly the elements it later writes, and no other thread
// touches them.
template <int TI, int TJ>
__device__ __forceinline__ void conv3x3_epilogue(const ConvArgs& a, f32x4 (&acc)[TI][TJ], f32x4 (&accx)[TI][TJ], int mb, int cb, int bad) {
  f32x4 r[TI][TJ];
  if (a.res) {
#pragma unroll
    for (int i = 0; i < TI; ++i) {
      const int m = mb + 16 * i;
#pragma unroll
      for (int j = 0; j < TJ; ++j)
        r[i][j] = m < a.M ? *reinterpret_cast<const f32x4*>(a.res + (size_t)m * kCout + (cb + 16 * j)) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
  }
  unscale_shift(acc, accx, a.w_unscale, a.bias, cb);
#pragma unroll
  for (int j = 0; j < TJ; ++j) {
#pragma unroll
    for (int i = 0; i < TI; ++i) {
      const int m = mb + 16 * i;
      if (m >= a.M) continue;
      f32x4 v = acc[i][j];
      if (a.res) v += r[i][j];
      if (a.relu_out) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = v[e] < 0.0f ? 0.0f : v[e];
      }
      *reinterpret_cast<f32x4*>(a.out + (size_t)m * kCout + (cb + 16 * j)) = v;
    }
  }
  if (a.range && bad) atomicAdd(a.range, bad);
}

}  // namespace
}  // namespace rmnet
