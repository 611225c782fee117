// flow_conv.hip -- TinyFlowNet's wide convolutions on the split-fp16 arithmetic of conv_split.hip, written once over a TAP LIST so
// that the forward convolutions (k = 3 or 5, stride 1 or 2, padding k / 2) and ConvTranspose2d(4, stride 2, padding 1) run the same
// code, with bias and none / ReLU / LeakyReLU(0.1) in the epilogue:
//
//   out[n, so*i + a, so*j + b, coff + co] =
//       act(unscale[co] / 64 * sum_{ty < KH, tx < KW, ci < Cin} x[n, si*i + oy + ty, si*j + ox + tx, ci] * Wp[phase][ty][tx][ci][co] + shift[co])
//
//   forward      so = 1, si = stride, KH = KW = k, oy = ox = -k / 2, one phase; (i, j) runs over the OUTPUT map;
//   transposed   so = 2, si = 1, KH = KW = 2, four phases (a, b) in {0, 1}^2 = blockIdx.z, oy = a - 1, ox = b - 1; (i, j) runs over the
//                INPUT map and phase (a, b) writes the output pixels (2i + a, 2j + b): every output pixel belongs to exactly one phase.
//                From y = 2 iy - 1 + ky the tap ty of phase a is ky = 3 - a - 2 ty ({3, 1} for a = 0, {2, 0} for a = 1), in x alike;
//                the packer (ops.flow_conv_pack) lays the weights out per phase, the kernel never sees the 4x4 kernel.
//
// Input and output carry an explicit channel stride (floats per pixel): x_ld >= ceil32(Cin) -- Cin need not be a multiple of 32, the
// pack holds zero weights for the channels Cin .. ceil32(Cin) - 1 and whatever the input holds there is saturated to a finite fp16 and
// multiplied by zero -- and out_ld with a channel offset coff: only the channels coff .. coff + Cout - 1 of a pixel are written.  So a
// layer reads a concatenation buffer, and writes its share of the next one, in place.
//
// Arithmetic: conv_split.hip's (see there and conv3x3.hip) -- fp16 hi + lo operands, Ah*Wh in one fp32 accumulator set and
// Ah*Wl + Al*Wh in a second one on v_mfma_f32_16x16x32_f16, activations scaled by 2^6, weights by the packer's per-channel power of
// two.  Activations with |64 x| > 65504 (NaN and Inf included) are saturated and counted into the caller's range word by the
// workgroups of the first Cout slice (and of phase 0: its four taps read every input pixel that any phase reads).  An element is
// counted at EVERY tap that reads it, i.e. possibly more than once: the word is zero exactly when no real channel (ci < Cin) of any
// pixel the convolution reads is outside the window, and its value has no other meaning.
//
// GEMM view: M = N * Hg * Wg grid pixels, N = Cout, K = taps * ceil32(Cin) ordered (tap, channel); one K step is one tap x 32
// channels.  The tile is conv_split.hip's Narrow: 128 px x 64 ch, waves 4 x 2 of 2 x 2 MFMA tiles, two workgroups per CU
// (<= 128 VGPRs).  Its Mid tile (128 x 128) is not used: the hi*hi products are accumulated in two levels here (per tap, then
// over the taps: see ptap below), which costs a third accumulator set that Mid cannot hold inside 128 VGPRs, and without it the
// whole network's error against float64 was 3.7 - 4.3 times the library's.  One LDS double buffer (X hi/lo [128][32] + W hi/lo
// [64][32] fp16: 48 KB) taken as DYNAMIC shared memory, one barrier per K step, the next step's operands prefetched into VGPRs
// (native vector types) while the MFMAs run, the last step peeled, sched_barrier(0) around the MFMA block:
// profiles/r12_a_weight_prefetch.md says why for each.
#include "split_f16.h"      // the vector types, kKT, kThreads, the activation scale, swz (conv3x3.hip's LDS layout)

namespace rmnet {
namespace {

struct FlowArgs {
  const float* x;          // [N][H][W][x_ld]
  const u32x4* wp;         // [phase][KH * KW][CB][2][Cout][32] fp16
  const float* unscale;    // [Cout]
  const float* shift;      // [Cout] or null
  float* out;              // [N][Ho][Wo][out_ld], channels coff .. coff + Cout - 1
  int* range;              // or null
  int M, H, W, Hg, Wg, Ho, Wo, Cin, CB, x_ld, Cout, out_ld, coff, KH, KW, si, so, act;
};

template <int WM, int WN, int TI, int TJ>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(4))) void flow_taps(FlowArgs a) {
  static_assert(WM * WN * 64 == kThreads, "8 waves");
  static_assert(TI >= TJ, "weight fragments held, activation fragments streamed");
  constexpr int MT = WM * TI * 16, NT = WN * TJ * 16;
  constexpr int XI = MT / 64;                      // activation float4s per thread and step
  constexpr int WI = NT / 64;                      // weight 16-byte chunks per thread and step
  constexpr int kXPlane = MT * kKT, kWPlane = NT * kKT;
  constexpr int kBufHalves = 2 * kXPlane + 2 * kWPlane;
  static_assert(2 * kBufHalves * 2 <= 64 * 1024, "dynamic LDS without a function attribute");
  extern __shared__ __attribute__((aligned(16))) _Float16 lds[];      // 2 * kBufHalves halves, sized at launch

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave % WM, wn = wave / WM;
  const int m0 = blockIdx.x * MT, n0 = blockIdx.y * NT;
  const int CB = a.CB, taps = a.KH * a.KW, steps = taps * CB;
  const int HWg = a.Hg * a.Wg;
  const int pa = a.so == 2 ? (int)(blockIdx.z >> 1) : 0, pb = a.so == 2 ? (int)(blockIdx.z & 1) : 0;   // the phase (a, b)
  const int oy = a.so == 2 ? pa - 1 : -(a.KH >> 1), ox = a.so == 2 ? pb - 1 : -(a.KW >> 1);
  const u32x4* wphase = a.wp + (size_t)blockIdx.z * steps * (a.Cout * 8);

  // loader items: activations XI x float4 (pixel p = tid/8 + 64i, channels 4*(tid&7) ..), weights WI x 16 B
  const int c4 = tid & 7;
  int pbase[XI];             // input pixel of tap (0, 0), flat index (may lie outside the map: see ok)
  unsigned ok[XI];           // bit t: tap t of this grid pixel lies inside the map (KH * KW <= 25 taps; past M: none does)
#pragma unroll
  for (int i = 0; i < XI; ++i) {
    const int m = m0 + (tid >> 3) + 64 * i;
    const int n = m / HWg, r = m - n * HWg;
    const int gi = r / a.Wg, gj = r - gi * a.Wg;
    const int h0 = gi * a.si + oy, w0 = gj * a.si + ox;
    pbase[i] = (n * a.H + h0) * a.W + w0;
    unsigned bits = 0;
    for (int t = 0; t < taps; ++t) {
      const int ty = t / a.KW, tx = t - ty * a.KW;
      if (m < a.M && (unsigned)(h0 + ty) < (unsigned)a.H && (unsigned)(w0 + tx) < (unsigned)a.W) bits |= 1u << t;
    }
    ok[i] = bits;
  }
  f32x4 xr[XI];
  u32x4 wr[WI];
  int bad = 0;
  const bool count = a.range != nullptr && blockIdx.y == 0 && blockIdx.z == 0;   // (every slice and phase reads the same inputs)

  auto load_x = [&](int s) {
    const int tap = s / CB, cb = s - tap * CB;
    const int ty = tap / a.KW, tx = tap - ty * a.KW;
#pragma unroll
    for (int i = 0; i < XI; ++i) {
      if ((ok[i] >> tap) & 1) {
        const size_t off = (size_t)(pbase[i] + ty * a.W + tx) * a.x_ld + cb * kKT + 4 * c4;
        xr[i] = *reinterpret_cast<const f32x4*>(a.x + off);
      } else {
        xr[i] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
    }
  };
  auto load_w = [&](int s) {
    const u32x4* wsrc = wphase + (size_t)s * (a.Cout * 8);
#pragma unroll
    for (int i = 0; i < WI; ++i) {
      const int q = tid + kThreads * i;
      const int plane = q / (NT * 4), co = (q >> 2) % NT, ch = q & 3;
      wr[i] = wsrc[plane * (a.Cout * 4) + (n0 + co) * 4 + ch];
    }
  };

  auto store_x = [&](int s, _Float16* buf) {
    const int nreal = a.Cin - (s % CB) * kKT - 4 * c4;     // this thread's channels below Cin: the pack's zero channels are not counted
    _Float16* xh = buf;
    _Float16* xl = buf + kXPlane;
#pragma unroll
    for (int i = 0; i < XI; ++i) {
      half4 hi, lo;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float y = xr[i][e] * kActScale;
        bad += (count && e < nreal && !(fabsf(y) <= kF16Max)) ? 1 : 0;  // (the padding's zeros pass)
        const float c = fminf(fmaxf(y, -kF16Max), kF16Max);            // (NaN becomes finite too)
        const _Float16 h = (_Float16)c;
        hi[e] = h;
        lo[e] = (_Float16)(c - (float)h);
      }
      const int p = (tid >> 3) + 64 * i;
      const int o = swz(p, c4 >> 1) + 4 * (c4 & 1);
      *reinterpret_cast<half4*>(xh + o) = hi;
      *reinterpret_cast<half4*>(xl + o) = lo;
    }
  };
  auto store_w = [&](_Float16* buf) {
    _Float16* wb = buf + 2 * kXPlane;
#pragma unroll
    for (int i = 0; i < WI; ++i) {
      const int q = tid + kThreads * i;
      const int plane = q / (NT * 4), co = (q >> 2) % NT, ch = q & 3;
      *reinterpret_cast<u32x4*>(wb + plane * kWPlane + swz(co, ch)) = wr[i];
    }
  };

  // hi*hi in two levels -- ptap holds the running sum of ONE tap (CB steps) and is added to acc when the tap ends -- and the two
  // cross terms apart.  The running sum is rounded once per step, and in one level that is taps * CB (up to 625) roundings of a
  // sum that has reached its full size; in two levels it is CB roundings of a tap's sum and one per tap of the whole.  The cross
  // terms are 2^-11 of the hi*hi term, so their roundings do not matter.
  f32x4 acc[TI][TJ], ptap[TI][TJ], accx[TI][TJ];
#pragma unroll
  for (int i = 0; i < TI; ++i)
#pragma unroll
    for (int j = 0; j < TJ; ++j) acc[i][j] = ptap[i][j] = accx[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  auto end_tap = [&] {
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
      for (int j = 0; j < TJ; ++j) {
        acc[i][j] += ptap[i][j];
        ptap[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
  };

  load_x(0);
  load_w(0);
  store_x(0, lds);
  store_w(lds);
  __syncthreads();
  const int fr = lane & 15, fc = lane >> 4;
  auto mma = [&](const _Float16* cur) {
    const _Float16* xh = cur;
    const _Float16* xl = cur + kXPlane;
    const _Float16* wh = cur + 2 * kXPlane;
    const _Float16* wl = wh + kWPlane;
    half8 ah[TJ], al[TJ];
#pragma unroll
    for (int j = 0; j < TJ; ++j) {
      const int o = swz(wn * TJ * 16 + j * 16 + fr, fc);
      ah[j] = *reinterpret_cast<const half8*>(wh + o);
      al[j] = *reinterpret_cast<const half8*>(wl + o);
    }
#pragma unroll
    for (int i = 0; i < TI; ++i) {
      const int o = swz(wm * TI * 16 + i * 16 + fr, fc);
      const half8 bh = *reinterpret_cast<const half8*>(xh + o);
      const half8 bl = *reinterpret_cast<const half8*>(xl + o);
#pragma unroll
      for (int j = 0; j < TJ; ++j) ptap[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[j], bh, ptap[i][j], 0, 0, 0);
#pragma unroll
      for (int j = 0; j < TJ; ++j) accx[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[j], bl, accx[i][j], 0, 0, 0);
#pragma unroll
      for (int j = 0; j < TJ; ++j) accx[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[j], bh, accx[i][j], 0, 0, 0);
    }
  };
  // The last step is apart, so that the loop body has no branch around the loads and the stores: all of a step's global loads are
  // in flight before its first MFMA.
  int left = CB;                        // steps left in the current tap
  for (int s = 0; s + 1 < steps; ++s) {
    _Float16* nxt = lds + ((s + 1) & 1) * kBufHalves;
    load_x(s + 1);
    load_w(s + 1);
    __builtin_amdgcn_sched_barrier(0);
    mma(lds + (s & 1) * kBufHalves);
    __builtin_amdgcn_sched_barrier(0);
    if (--left == 0) {
      end_tap();
      left = CB;
    }
    store_x(s + 1, nxt);
    store_w(nxt);
    __syncthreads();
  }
  mma(lds + ((steps - 1) & 1) * kBufHalves);
  end_tap();                            // (the last step ends the last tap)

  // epilogue: D[co][px] -- lane holds grid pixel fr of each 16-pixel tile and channels 4*fc .. 4*fc+3 of each 16-channel tile.
  // Unscale and shift in place, for all tiles, before the first store (for all the compiler knows these vectors alias out).
#pragma unroll
  for (int j = 0; j < TJ; ++j) {
    const int co = n0 + wn * TJ * 16 + j * 16 + 4 * fc;
    const f32x4 us = *reinterpret_cast<const f32x4*>(a.unscale + co) * kActUnscale;
    const f32x4 b = a.shift ? *reinterpret_cast<const f32x4*>(a.shift + co) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < TI; ++i) acc[i][j] = (acc[i][j] + accx[i][j]) * us + b;
  }
  // (An empty statement the optimiser cannot see through: it keeps the loop above out of the guarded stores below.)
#pragma unroll
  for (int j = 0; j < TJ; ++j)
#pragma unroll
    for (int i = 0; i < TI; ++i) asm volatile("" : "+v"(acc[i][j]));
  int eHW = HWg, eW = a.Wg;
  asm volatile("" : "+s"(eHW), "+s"(eW));      // (the divisors' reciprocals are formed here, not kept in VGPRs through the main loop)
#pragma unroll
  for (int i = 0; i < TI; ++i) {
    int m = m0 + wm * TI * 16 + i * 16 + fr;
    asm volatile("" : "+v"(m));                // (nor the quotients)
    if (m >= a.M) continue;
    int opix = m;                       // forward: the grid IS the output map
    if (a.so == 2) {
      const int n = m / eHW, r = m - n * eHW;
      const int gi = r / eW, gj = r - gi * eW;
      opix = (n * a.Ho + 2 * gi + pa) * a.Wo + 2 * gj + pb;
    }
    float* orow = a.out + (size_t)opix * a.out_ld + a.coff;
#pragma unroll
    for (int j = 0; j < TJ; ++j) {
      const int co = n0 + wn * TJ * 16 + j * 16 + 4 * fc;
      f32x4 v = acc[i][j];
      if (a.act == 1) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = v[e] < 0.0f ? 0.0f : v[e];
      } else if (a.act == 2) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = v[e] > 0.0f ? v[e] : v[e] * 0.1f;      // epilogue.hip's LeakyReLU(0.1), bit for bit
      }
      *reinterpret_cast<f32x4*>(orow + co) = v;
    }
  }
  if (bad) atomicAdd(a.range, bad);     // (bad != 0 only with a range word)
}

template <int WM, int WN, int TI, int TJ>
void launch(const FlowArgs& a, int phases, hipStream_t st) {
  constexpr int MT = WM * TI * 16, NT = WN * TJ * 16;
  constexpr size_t lds_bytes = 2 * (2 * MT * kKT + 2 * NT * kKT) * sizeof(_Float16);
  hipLaunchKernelGGL((flow_taps<WM, WN, TI, TJ>), dim3((unsigned)((a.M + MT - 1) / MT), (unsigned)(a.Cout / NT), (unsigned)phases),
                     dim3(kThreads), lds_bytes, st, a);
}

}  // namespace
}  // namespace rmnet

extern "C" int rmnet_flow_conv_f32(const float* x, int x_ld, const void* wpack, const float* w_unscale, const float* shift, int flags,
                                   int N, int H, int W, int Cin, int Cout, int ksize, int stride, float* out, int out_ld, int coff,
                                   int32_t* range_word, void* stream) {
  using namespace rmnet;
  if (!x || !wpack || !w_unscale || !out || N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return RMNET_E_INVALID_ARG;
  if (flags & ~(RMNET_FLOW_RELU | RMNET_FLOW_LEAKY | RMNET_FLOW_TRANSPOSED)) return RMNET_E_INVALID_ARG;
  if ((flags & RMNET_FLOW_RELU) && (flags & RMNET_FLOW_LEAKY)) return RMNET_E_INVALID_ARG;
  if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(wpack) | reinterpret_cast<uintptr_t>(w_unscale) |
       reinterpret_cast<uintptr_t>(shift) | reinterpret_cast<uintptr_t>(out)) & 15)
    return RMNET_E_INVALID_ARG;
  const bool tr = (flags & RMNET_FLOW_TRANSPOSED) != 0;
  if (tr ? (ksize != 4 || stride != 2) : ((ksize != 3 && ksize != 5) || (stride != 1 && stride != 2))) return RMNET_E_UNSUPPORTED;
  if (Cout % 64) return RMNET_E_UNSUPPORTED;
  const int CB = (Cin + kKT - 1) / kKT;
  if (x_ld % 4 || x_ld < CB * kKT || out_ld % 4 || coff % 4 || coff < 0 || out_ld < coff + Cout) return RMNET_E_INVALID_ARG;
  const int pad = ksize / 2;
  const int Ho = tr ? 2 * H : (H + 2 * pad - ksize) / stride + 1, Wo = tr ? 2 * W : (W + 2 * pad - ksize) / stride + 1;
  const long long Mi = (long long)N * H * W, Mo = (long long)N * Ho * Wo;
  if (Mi * x_ld >= (1LL << 31) || Mo * out_ld >= (1LL << 31)) return RMNET_E_UNSUPPORTED;   // (int pixel index, size_t offsets)
  // out must not overlap x: other workgroups read the same input pixels.  (The whole strided ranges are compared: a layer never
  // writes into the buffer it reads.)
  const char* xb = reinterpret_cast<const char*>(x);
  const char* ob = reinterpret_cast<const char*>(out);
  if (ob < xb + Mi * x_ld * sizeof(float) && xb < ob + Mo * out_ld * sizeof(float)) return RMNET_E_INVALID_ARG;
  FlowArgs a;
  a.x = x; a.wp = reinterpret_cast<const u32x4*>(wpack); a.unscale = w_unscale; a.shift = shift; a.out = out; a.range = range_word;
  a.H = H; a.W = W; a.Ho = Ho; a.Wo = Wo; a.Cin = Cin; a.CB = CB; a.x_ld = x_ld; a.Cout = Cout; a.out_ld = out_ld; a.coff = coff;
  a.Hg = tr ? H : Ho; a.Wg = tr ? W : Wo; a.M = (int)(tr ? Mi : Mo);
  a.KH = a.KW = tr ? 2 : ksize; a.si = tr ? 1 : stride; a.so = tr ? 2 : 1;
  a.act = (flags & RMNET_FLOW_LEAKY) ? 2 : ((flags & RMNET_FLOW_RELU) ? 1 : 0);
  const int phases = tr ? 4 : 1;
  hipStream_t st = (hipStream_t)stream;
  launch<4, 2, 2, 2>(a, phases, st);     // 128 px x 64 ch
  return check_launch();
}
