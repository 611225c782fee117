// conv_split.hip -- general split-fp16 implicit-GEMM convolution: kernel 1x1 or 3x3, stride 1 or 2, padding ksize / 2,
// fp32 NHWC in and out, Cin % 32 == 0, Cout % 64 == 0.  Runs the ResNet-50 trunks' bottleneck convolutions (BatchNorm
// folded into the pack, skip add and ReLU in the epilogue) and the fused key / value heads.
//
// Arithmetic: that of conv3x3.hip (see there) -- both operands carried as fp16 hi + lo, three product terms
// Ah*Wh + Ah*Wl + Al*Wh on v_mfma_f32_16x16x32_f16 in two fp32 accumulator sets, activations scaled by the exact 2^6,
// weights by a per-output-channel power of two chosen by the packer.  Out-of-window activations (|x| >= 1023.5, NaN, Inf)
// are saturated and counted in the caller's range word once per input element that the convolution reads: at the tap
// (ky, kx) with ky, kx in {pad} (stride 1, or 1x1) or {pad, 2} (3x3 / stride 2: the even rows / columns are the centre
// tap's, the odd ones the last tap's of the output to their upper left).
//
// GEMM view: M = N*Ho*Wo output pixels, N = Cout, K = ksize^2 * Cin ordered (tap, input channel); one K step of 32 is one
// tap x 32 contiguous input channels.  Workgroup = 512 threads (8 waves) = MT pixels x NT output channels, blockIdx.y
// picks the NT-channel slice of Cout.  Waves are WM (pixels) x WN (channels), each owns TI x TJ 16x16 MFMA tiles.  Tiles
// (chosen on the host, rmnet_conv_split_f32):
//   Big    MT 128 x NT 256 (WM 2, WN 4, 4x4 tiles/wave)  Cout % 256 == 0 on maps that give >= 512 workgroups: the
//          decoder kernel's shape (238 VGPRs, 96 KB of LDS, declared and allocated: one workgroup per CU);
//   Mid    MT 128 x NT 128 (WM 2, WN 4, 4x2 tiles/wave)  Cout % 128 == 0 otherwise: the 1/16 maps (M = 25,920 at the
//          bench shape) give only 203 Big workgroups for 256 CUs.  Held to 128 VGPRs (4 waves per SIMD) and 64 KB of
//          LDS, two Mid workgroups share a CU, so the 406 of a 256-channel 1/16 convolution run in one round;
//   Narrow MT 128 x NT 64  (WM 4, WN 2, 2x2 tiles/wave)  Cout = 64 (layer1 at 1/4), also two workgroups per CU.
// Every tile's registers, LDS and scratch are asserted from the compiler's metadata by tests/test_kernel_resources.py: no spills,
// and exactly the declared LDS (96 / 64 / 48 KB).
// One LDS double buffer (X hi/lo [MT][32] + W hi/lo [NT][32] fp16), one barrier per K step, as in conv3x3.hip.  The next step's
// operands are prefetched into VGPRs (native vector types: an array of HIP's uint4 would be placed in LDS) while the MFMAs run.
//
// One kernel template, conv_split<WM, WN, TI, TJ, WPE, XS, OS>, serves the fp32 tensors and the split ACTIVATION form
// (include/rmnet_hip.h): [M][C / 32][2][32] fp16 -- per pixel and block of 32 channels the 32 hi halves, then the 32 lo halves, of
// c = clamp(64 * pre(v)).  A pixel has the byte stride it has in fp32, and every 16-byte chunk is 8 halves of one plane: exactly a
// chunk of the LDS image.  XS: the input is in that form; OS: the output is written in it.  Tiles, weight path, mma, K order and
// the epilogue's arithmetic are common to the four (XS, OS) pairs; what differs stands in `if constexpr` branches:
//   load_x / store_x   XS 0: a float4 per item (thread = pixel tid / 8 + 64 i, channels 4 (tid % 8) ..), ReLU, split4 and the range
//                            count at every tap and Cout slice that reads the element, two 8-byte LDS stores;
//                      XS 1: a 16-byte load and a 16-byte LDS store per item (chunk tid % 8: plane tid % 8 / 4, channels
//                            8 (tid % 4) ..); nothing is converted, clamped or counted (the producer did that, once per element);
//   the K loop         XS 0, Mid only: the loads are taken "in turn" (see kInTurn); every other instance has all of a step's loads
//                            in flight before its first MFMA;
//   the store          OS 0: a lane's 4 channels as one float4, to out, or to out / out2 on either side of csplit;
//                      OS 1: as 8 bytes of hi and 8 bytes of lo (split4), the elements outside the window counted here, once each.
// 12 instances: 3 tiles x 4 pairs.  rmnet_conv_split_f32 is the (0, 0) pair alone, rmnet_conv_split_pre_f32 takes all four.
//
// The code of all of them is conv_split_body<..., RG>; the kernel conv_split<...> calls it with RG = false.  RG = true is the REGIONAL
// instance, the kernel conv_split_region (rmnet_conv_split_region_f32): the Mid tile with split input and two fp32 outputs, for the
// key / value heads of the frame step, whose consumers (csrc/bank.hip: bk_append, bk_main) use only the cells inside one rectangle
// per image.  Its GEMM rows are those cells, compacted -- image after image, each rectangle row-major -- through a prefix table in
// LDS; its outputs are NCHW, and every cell outside a rectangle is written as +0.0 by the workgroup that owns the cell's place in the
// flat N*H*W index.  The weight path, the mma, the K order and the epilogue's arithmetic are the dense kernel's, so a cell inside a
// rectangle gets the dense kernel's bits (tests/test_conv_split_region.py).  64 KB + 1284 B of LDS, 126 VGPRs: two workgroups per CU.
#include "split_f16.h"      // the vector types, kKT, kThreads, the activation scale, swz, split4, overlap

namespace rmnet {
namespace {

struct SplitArgs {
  const float* x;          // XS 0: [N][H][W][Cin] fp32
  const _Float16* xs;      // XS 1: [N][H][W][Cin / 32][2][32] fp16
  const u32x4* wp;         // [k*k][Cin / 32][2][Cout][32] fp16
  const float* unscale;    // [Cout]
  const float* shift;      // [Cout] or null
  const float* res;        // [M][Cout] fp32 or null
  float* out;              // OS 0: [M][Cout] fp32, or [M][csplit] with out2
  float* out2;             // OS 0 only: null, or [M][Cout - csplit]: channels csplit .. Cout-1
  _Float16* outs;          // OS 1: [M][Cout / 32][2][32] fp16
  int* range;              // or null
  int M, H, W, Ho, Wo, Cin, Cout, csplit, ksize, stride, pad, relu_in, relu_out;
};

// The regional instance (RG; the kernel conv_split_region below): M = N*H*W cells, out / out2 are NCHW
struct RegionArgs : SplitArgs {
  const int32_t* rects;    // [N][4] (cx0, cx1, cy0, cy1), inclusive; the kernel clamps them to the map as bk_append / bk_main do
};
constexpr int kRegionMaxObjects = 64;      // objects per launch: the size of the LDS tables (as kBankMaxObj, a launch of the bank read)

// The regional instance's row map, in LDS next to the double buffer: pref[o] = cells inside the rectangles of the objects before o
// (pref[N] = the GEMM's rows), rect[o] = object o's clamped rectangle.  Row g is cell g - pref[o] of object o in bk_append's
// enumeration (the rectangle row-major): cy0 + n / rw, cx0 + n % rw.
struct RegionTables {
  int pref[kRegionMaxObjects + 1];
  int rect[kRegionMaxObjects][4];
};
__device__ __forceinline__ RegionTables& region_tables() {
  __shared__ RegionTables t;
  return t;
}
// g < pref[NO]: the object and the cell (row, column) of row g.  An empty object has no row: pref[o] <= g < pref[o + 1] names one
__device__ __forceinline__ void region_row(const RegionTables& t, int NO, int g, int& o, int& cy, int& cx) {
  int lo = 0, hi = NO;                  // pref[lo] <= g < pref[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (t.pref[mid] <= g) lo = mid; else hi = mid;
  }
  const int n = g - t.pref[lo], rw = t.rect[lo][1] - t.rect[lo][0] + 1, ry = n / rw;
  o = lo;
  cy = t.rect[lo][2] + ry;
  cx = t.rect[lo][0] + (n - ry * rw);
}

// The body of every instance.  WPE: waves per SIMD the register allocation must allow -- 2 (one workgroup per CU) for Big, 4 (two)
// for Mid / Narrow.  RG: the GEMM's rows are the cells inside the objects' rectangles, compacted; what differs stands in
// `if constexpr (RG)` branches (the row map of the loader and of the epilogue, the NCHW stores, the zero fill).
template <int WM, int WN, int TI, int TJ, int WPE, bool XS, bool OS, bool RG, class Args>
__device__ __forceinline__ void conv_split_body(const Args a) {
  static_assert(WM * WN * 64 == kThreads, "8 waves");
  static_assert(!RG || (XS && !OS), "the regional instance takes a split input and writes fp32");
  constexpr int MT = WM * TI * 16, NT = WN * TJ * 16;
  constexpr int XI = MT / 64;                      // activation items per thread and step (16 bytes each, either form)
  constexpr int WI = NT / 64;                      // weight 16-byte chunks per thread and step
  constexpr int kXPlane = MT * kKT, kWPlane = NT * kKT;
  constexpr int kBufHalves = 2 * kXPlane + 2 * kWPlane;
  static_assert(2 * kBufHalves * 2 <= kLdsBytesPerCU, "LDS budget");
  __shared__ __attribute__((aligned(16))) _Float16 lds[2 * kBufHalves];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave % WM, wn = wave / WM;
  const int m0 = blockIdx.x * MT, n0 = blockIdx.y * NT;
  const int CB = a.Cin / kKT, steps = a.ksize * a.ksize * CB;
  const int HWo = a.Ho * a.Wo;

  // loader items: activations XI x 16 bytes (pixel p = tid/8 + 64i; c4: see load_x / store_x in the header), weights WI x 16 B
  const int c4 = tid & 7;
  int pbase[XI], ph[XI], pw[XI];      // input pixel of tap (0, 0): flat index, row, column (outside the map: not read)
  if constexpr (RG) {
    // One wave clamps the rectangles and scans their areas into the tables
    RegionTables& rt = region_tables();
    const int NO = a.M / HWo;
    if (tid < RMNET_WAVE) {
      Rect rc{1, 0, 1, 0};
      if (tid < NO) {
        const int32_t* r = a.rects + 4 * tid;
        rc = Rect{max(r[0], 0), min(r[1], a.W - 1), max(r[2], 0), min(r[3], a.H - 1)};
      }
      const int incl = wave_scan_incl_fast(rc.area());
      if (tid == 0) rt.pref[0] = 0;
      if (tid < NO) {
        rt.pref[tid + 1] = incl;
        rt.rect[tid][0] = rc.cx0; rt.rect[tid][1] = rc.cx1; rt.rect[tid][2] = rc.cy0; rt.rect[tid][3] = rc.cy1;
      }
    }
    __syncthreads();
    // The fill: the cells [m0, m0 + MT) of the flat N*H*W index that lie outside their object's rectangle are +0.0 in this
    // workgroup's NT channels.  The grid covers every cell and no workgroup computes a cell outside a rectangle, so every element
    // of the outputs is written exactly once.  Thread = one cell (a wave stores 64 consecutive floats of a channel plane) and the
    // channels tid / MT, + kThreads / MT, ...
    {
      static_assert(kThreads % MT == 0, "a thread of the fill owns one cell");
      const int f = m0 + tid % MT;
      bool fill = f < a.M;
      const int o = fill ? f / HWo : 0, cell = f - o * HWo;
      if (fill) {
        const int cy = cell / a.Wo, cx = cell - cy * a.Wo;
        fill = !Rect{rt.rect[o][0], rt.rect[o][1], rt.rect[o][2], rt.rect[o][3]}.contains(cy, cx);
      }
      if (fill) {
        const int c2 = a.Cout - a.csplit;
        for (int c = n0 + tid / MT; c < n0 + NT; c += kThreads / MT) {
          if (c < a.csplit)
            a.out[((size_t)o * a.csplit + c) * HWo + cell] = 0.0f;
          else
            a.out2[((size_t)o * c2 + (c - a.csplit)) * HWo + cell] = 0.0f;
        }
      }
    }
    const int total = rt.pref[NO];
    if (m0 >= total) return;            // (the whole workgroup: no row of this tile is a cell of a rectangle)
#pragma unroll
    for (int i = 0; i < XI; ++i) {
      const int g = m0 + (tid >> 3) + 64 * i;
      int o = 0, cy = -4 + a.pad, cx = a.pad;       // (past the last row: every tap's row is < 0)
      if (g < total) region_row(rt, NO, g, o, cy, cx);
      ph[i] = cy - a.pad;
      pw[i] = cx - a.pad;
      pbase[i] = (o * a.H + ph[i]) * a.W + pw[i];
    }
  } else {
#pragma unroll
    for (int i = 0; i < XI; ++i) {
      const int m = m0 + (tid >> 3) + 64 * i;
      const int n = m / HWo, r = m - n * HWo;
      const int ho = r / a.Wo, wo = r - ho * a.Wo;
      ph[i] = m < a.M ? ho * a.stride - a.pad : -4;       // (past M: every tap's row is < 0)
      pw[i] = wo * a.stride - a.pad;
      pbase[i] = (n * a.H + ph[i]) * a.W + pw[i];
    }
  }
  f32x4 xr[XI];
  u32x4 xq[XI];
  u32x4 wr[WI];
  int bad = 0;

  auto load_x = [&](int s) {
    const int tap = s / CB, cb = s - tap * CB;
    const int ky = tap / a.ksize, kx = tap - ky * a.ksize;
#pragma unroll
    for (int i = 0; i < XI; ++i) {
      const int h = ph[i] + ky, w = pw[i] + kx;
      const bool in = (unsigned)h < (unsigned)a.H && (unsigned)w < (unsigned)a.W;
      if constexpr (XS) {
        if (in) {
          // (in halves, below 2^32: the entry holds N*H*W*Cin below 2^31 -- a uniform base and a 32-bit offset per lane)
          const unsigned off = (unsigned)(pbase[i] + ky * a.W + kx) * (unsigned)(2 * a.Cin) + (unsigned)(cb * (2 * kKT) + 8 * c4);
          xq[i] = *reinterpret_cast<const u32x4*>(a.xs + off);
        } else {
          xq[i] = u32x4{0u, 0u, 0u, 0u};
        }
      } else {
        if (in) {
          const size_t off = (size_t)(pbase[i] + ky * a.W + kx) * a.Cin + cb * kKT + 4 * c4;
          xr[i] = *reinterpret_cast<const f32x4*>(a.x + off);
        } else {
          xr[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
      }
    }
  };
  auto load_w = [&](int s) {
    const u32x4* wsrc = a.wp + (size_t)s * (a.Cout * 8);
#pragma unroll
    for (int i = 0; i < WI; ++i) {
      const int q = tid + kThreads * i;
      const int plane = q / (NT * 4), co = (q >> 2) % NT, ch = q & 3;
      wr[i] = wsrc[(unsigned)(plane * (a.Cout * 4) + (n0 + co) * 4 + ch)];      // (uniform base, 32-bit lane offset)
    }
  };

  auto counted = [&](int t) { return t == a.pad || (a.stride == 2 && a.ksize == 3 && t == 2); };

  auto store_x = [&](int s, _Float16* buf) {
    if constexpr (XS) {
#pragma unroll
      for (int i = 0; i < XI; ++i) {
        const int p = (tid >> 3) + 64 * i;
        *reinterpret_cast<u32x4*>(buf + (c4 >> 2) * kXPlane + swz(p, c4 & 3)) = xq[i];
      }
    } else {
      const int tap = s / CB, ky = tap / a.ksize, kx = tap - ky * a.ksize;
      const bool count = blockIdx.y == 0 && counted(ky) && counted(kx);   // (every Cout slice reads the same inputs: count in one)
      _Float16* xh = buf;
      _Float16* xl = buf + kXPlane;
#pragma unroll
      for (int i = 0; i < XI; ++i) {
        // split4's arithmetic, element for element, written out: with a call of split4(v, hi, lo, bad, count) here the compiler gives
        // the fp32-input instances other code (Mid: 128 VGPRs instead of 126, 21 more instructions)
        half4 hi, lo;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float v = xr[i][e];
          if (a.relu_in) v = v < 0.0f ? 0.0f : v;          // (keeps NaN: it is counted below)
          const float y = v * kActScale;
          bad += (count && !(fabsf(y) <= kF16Max)) ? 1 : 0;  // (the padding's zeros pass)
          const float c = fminf(fmaxf(y, -kF16Max), kF16Max);
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
  auto store_w = [&](_Float16* buf) {
    _Float16* wb = buf + 2 * kXPlane;
#pragma unroll
    for (int i = 0; i < WI; ++i) {
      const int q = tid + kThreads * i;
      const int plane = q / (NT * 4), co = (q >> 2) % NT, ch = q & 3;
      *reinterpret_cast<u32x4*>(wb + plane * kWPlane + swz(co, ch)) = wr[i];
    }
  };

  f32x4 acc[TI][TJ], accx[TI][TJ];      // hi*hi, and the two cross terms apart
#pragma unroll
  for (int i = 0; i < TI; ++i)
#pragma unroll
    for (int j = 0; j < TJ; ++j) acc[i][j] = accx[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  load_x(0);
  load_w(0);
  store_x(0, lds);
  store_w(lds);
  __syncthreads();
  const int fr = lane & 15, fc = lane >> 4;
  // A fragment's swizzle depends on its row's bits 1..2 alone, which a step of 16 rows leaves alone: one address per operand
  // (xo, wo) and constant offsets from it, instead of one address register per fragment
  const int xo = swz(wm * TI * 16 + fr, fc), wo = 2 * kXPlane + swz(wn * TJ * 16 + fr, fc);
  constexpr int kFrag = 16 * kKT;
  auto mma = [&](const _Float16* cur, auto&& halfway) {
    const _Float16* xb = cur + xo;
    const _Float16* wb = cur + wo;
    if constexpr (TJ >= TI) {             // all activation fragments held, weight fragments streamed (Big)
      half8 bh[TI], bl[TI];
#pragma unroll
      for (int i = 0; i < TI; ++i) {
        bh[i] = *reinterpret_cast<const half8*>(xb + i * kFrag);
        bl[i] = *reinterpret_cast<const half8*>(xb + kXPlane + i * kFrag);
      }
#pragma unroll
      for (int j = 0; j < TJ; ++j) {
        const half8 ah = *reinterpret_cast<const half8*>(wb + j * kFrag);
        const half8 al = *reinterpret_cast<const half8*>(wb + kWPlane + j * kFrag);
#pragma unroll
        for (int i = 0; i < TI; ++i) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bh[i], acc[i][j], 0, 0, 0);
#pragma unroll
        for (int i = 0; i < TI; ++i) accx[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bl[i], accx[i][j], 0, 0, 0);
#pragma unroll
        for (int i = 0; i < TI; ++i) accx[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, bh[i], accx[i][j], 0, 0, 0);
        if (j == TJ / 2 - 1) halfway();
      }
    } else {                              // the other way round (Mid, Narrow): 24 fragment VGPRs instead of 40, inside 128
      half8 ah[TJ], al[TJ];
#pragma unroll
      for (int j = 0; j < TJ; ++j) {
        ah[j] = *reinterpret_cast<const half8*>(wb + j * kFrag);
        al[j] = *reinterpret_cast<const half8*>(wb + kWPlane + j * kFrag);
      }
#pragma unroll
      for (int i = 0; i < TI; ++i) {
        const half8 bh = *reinterpret_cast<const half8*>(xb + i * kFrag);
        const half8 bl = *reinterpret_cast<const half8*>(xb + kXPlane + i * kFrag);
#pragma unroll
        for (int j = 0; j < TJ; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[j], bh, acc[i][j], 0, 0, 0);
#pragma unroll
        for (int j = 0; j < TJ; ++j) accx[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[j], bl, accx[i][j], 0, 0, 0);
#pragma unroll
        for (int j = 0; j < TJ; ++j) accx[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[j], bh, accx[i][j], 0, 0, 0);
        if (i == TI / 2 - 1) halfway();
      }
    }
  };
  // The last step is apart, so that the loop body has no branch around the loads and the stores (see conv3x3.hip).  All of a step's
  // global loads are in flight before its first MFMA, and nothing that waits for them is moved in among the MFMAs -- except in
  // Mid with fp32 input, which cannot hold 8 VGPRs of activations and 8 of weights in flight next to its fragments inside 128 VGPRs,
  // so it takes them in turn: the activations fly during the first half of the MFMAs and are split and stored half way (the other
  // buffer is free from the last barrier on), the weights fly during the second half.  With a split input Mid has 16 VGPRs of loads
  // in flight and nothing to convert, so no tile takes its loads in turn.
  constexpr bool kInTurn = !XS && TI > TJ && WPE == 4 && WI > 1;
  for (int s = 0; s + 1 < steps; ++s) {
    _Float16* nxt = lds + ((s + 1) & 1) * kBufHalves;
    load_x(s + 1);
    if constexpr (!kInTurn) load_w(s + 1);
    __builtin_amdgcn_sched_barrier(0);
    mma(lds + (s & 1) * kBufHalves, [&] {
      if constexpr (kInTurn) {
        __builtin_amdgcn_sched_barrier(0);
        load_w(s + 1);
        store_x(s + 1, nxt);
        __builtin_amdgcn_sched_barrier(0);
      }
    });
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (!kInTurn) store_x(s + 1, nxt);
    store_w(nxt);
    __syncthreads();
  }
  mma(lds + ((steps - 1) & 1) * kBufHalves, [] {});

  // epilogue: D[co][px] -- lane holds pixel fr of each 16-pixel tile and channels 4*fc .. 4*fc+3 of each 16-channel tile.
  // The residual: an fp32 out may BE res (a split one never is), so the compiler keeps every read of res in front of the stores that
  // follow it in the source.  All TI x TJ reads are therefore issued here, before the first store (one round trip, not TI x TJ
  // dependent ones; the loader's registers are dead by now).  This is safe with out == res: a thread reads exactly the elements it
  // later writes, and no other thread touches them.
  f32x4 r[TI][TJ];
  if (!RG && a.res) {
#pragma unroll
    for (int i = 0; i < TI; ++i) {
      const int m = m0 + wm * TI * 16 + i * 16 + fr;
#pragma unroll
      for (int j = 0; j < TJ; ++j) {
        const int co = n0 + wn * TJ * 16 + j * 16 + 4 * fc;
        r[i][j] = m < a.M ? *reinterpret_cast<const f32x4*>(a.res + (size_t)m * a.Cout + co) : f32x4{0.f, 0.f, 0.f, 0.f};
      }
    }
  }
  // Unscale and shift in place, for all tiles, before the first store: for all the compiler knows these vectors alias out too, and
  // read between the stores they would cost one more waited-for round trip per channel tile.
#pragma unroll
  for (int j = 0; j < TJ; ++j) {
    const int co = n0 + wn * TJ * 16 + j * 16 + 4 * fc;
    const f32x4 us = *reinterpret_cast<const f32x4*>(a.unscale + co) * kActUnscale;
    const f32x4 b = a.shift ? *reinterpret_cast<const f32x4*>(a.shift + co) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < TI; ++i) acc[i][j] = (acc[i][j] + accx[i][j]) * us + b;
  }
  // (An empty statement the optimiser cannot see through: without it the loop above is sunk into the guarded stores below, and
  // each tile's wait for its unscale vector then includes the stores issued before it.)
#pragma unroll
  for (int j = 0; j < TJ; ++j)
#pragma unroll
    for (int i = 0; i < TI; ++i) asm volatile("" : "+v"(acc[i][j]));
  if constexpr (RG) {
    // NCHW: a lane's 4 channels are 4 dword stores, the 16 lanes of a tile's pixels cover 16 consecutive rows of the map (cells
    // that are consecutive in memory, but for the ends of the rectangle's rows).  No residual; rows past the last are not stored.
    const RegionTables& rt = region_tables();
    const int NO = a.M / HWo, total = rt.pref[NO];
    int po[TI], pcell[TI];
#pragma unroll
    for (int i = 0; i < TI; ++i) {
      const int g = m0 + wm * TI * 16 + i * 16 + fr;
      int cy = 0, cx = 0;
      po[i] = -1;
      if (g < total) region_row(rt, NO, g, po[i], cy, cx);
      pcell[i] = cy * a.Wo + cx;
    }
    const int c2 = a.Cout - a.csplit;
#pragma unroll
    for (int j = 0; j < TJ; ++j) {
      const int co = n0 + wn * TJ * 16 + j * 16 + 4 * fc;
      const bool key = co < a.csplit;        // (csplit % 4 == 0: a lane's 4 channels fall on one side)
#pragma unroll
      for (int i = 0; i < TI; ++i) {
        if (po[i] < 0) continue;
        f32x4 v = acc[i][j];
        if (a.relu_out) {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = v[e] < 0.0f ? 0.0f : v[e];
        }
        float* o = key ? a.out + ((size_t)po[i] * a.csplit + co) * HWo + pcell[i]
                       : a.out2 + ((size_t)po[i] * c2 + (co - a.csplit)) * HWo + pcell[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) o[(size_t)e * HWo] = v[e];
      }
    }
    return;
  }
#pragma unroll
  for (int j = 0; j < TJ; ++j) {
    const int co = n0 + wn * TJ * 16 + j * 16 + 4 * fc;
#pragma unroll
    for (int i = 0; i < TI; ++i) {
      const int m = m0 + wm * TI * 16 + i * 16 + fr;
      if (m >= a.M) continue;
      f32x4 v = acc[i][j];
      if (a.res) v += r[i][j];
      if (a.relu_out) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = v[e] < 0.0f ? 0.0f : v[e];
      }
      if constexpr (OS) {
        half4 hi, lo;
        split4(v, hi, lo, bad);
        _Float16* o = a.outs + (size_t)m * (2 * a.Cout) + (co >> 5) * (2 * kKT) + (co & 31);
        *reinterpret_cast<half4*>(o) = hi;
        *reinterpret_cast<half4*>(o + kKT) = lo;
      } else {
        const size_t off = (size_t)m * a.Cout + co;
        if (!a.out2)
          *reinterpret_cast<f32x4*>(a.out + off) = v;
        else if (co < a.csplit)         // (csplit % 4 == 0: a lane's 4 channels fall on one side)
          *reinterpret_cast<f32x4*>(a.out + (size_t)m * a.csplit + co) = v;
        else
          *reinterpret_cast<f32x4*>(a.out2 + (size_t)m * (a.Cout - a.csplit) + (co - a.csplit)) = v;
      }
    }
  }
  if (a.range && bad) atomicAdd(a.range, bad);
}

template <int WM, int WN, int TI, int TJ, int WPE, bool XS, bool OS>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(WPE))) void conv_split(SplitArgs a) {
  conv_split_body<WM, WN, TI, TJ, WPE, XS, OS, false>(a);
}

// The regional instance: the Mid tile, split in, fp32 NCHW out (the key / value heads of the frame step; see the entry below)
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(4))) void conv_split_region(RegionArgs a) {
  conv_split_body<2, 4, 4, 2, 4, true, false, true>(a);
}

template <int WM, int WN, int TI, int TJ, int WPE, bool XS, bool OS>
void launch(const SplitArgs& a, hipStream_t st) {
  constexpr int MT = WM * TI * 16, NT = WN * TJ * 16;
  hipLaunchKernelGGL((conv_split<WM, WN, TI, TJ, WPE, XS, OS>), dim3((unsigned)((a.M + MT - 1) / MT), (unsigned)(a.Cout / NT)),
                     dim3(kThreads), 0, st, a);
}

template <bool XS, bool OS>
void launch_tile(const SplitArgs& a, hipStream_t st) {      // the choice of tile (see the header)
  if (a.Cout % 256 == 0 && (long long)((a.M + 127) / 128) * (a.Cout / 256) >= 512)
    launch<2, 4, 4, 4, 2, XS, OS>(a, st);     // Big    128 x 256
  else if (a.Cout % 128 == 0)
    launch<2, 4, 4, 2, 4, XS, OS>(a, st);     // Mid    128 x 128
  else
    launch<4, 2, 2, 2, 4, XS, OS>(a, st);     // Narrow 128 x 64
}

// fp32 NHWC -> split form, one item = 8 channels of one block: 32 bytes in, 16 bytes of hi and 16 of lo out.  No LDS.
constexpr int kSplitActThreads = 256;
__global__ __launch_bounds__(kSplitActThreads) void split_act(const float* __restrict__ x, _Float16* __restrict__ out, size_t items,
                                                              int relu, int* range) {
  int bad = 0;
  for (size_t q = (size_t)blockIdx.x * kSplitActThreads + threadIdx.x; q < items; q += (size_t)gridDim.x * kSplitActThreads) {
    f32x4 v[2];
    v[0] = *reinterpret_cast<const f32x4*>(x + q * 8);
    v[1] = *reinterpret_cast<const f32x4*>(x + q * 8 + 4);
    half8 hi, lo;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      if (relu) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[k][e] = v[k][e] < 0.0f ? 0.0f : v[k][e];      // (keeps NaN)
      }
      half4 h4, l4;
      split4(v[k], h4, l4, bad);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        hi[4 * k + e] = h4[e];
        lo[4 * k + e] = l4[e];
      }
    }
    _Float16* o = out + (q >> 2) * (2 * kKT) + (q & 3) * 8;
    *reinterpret_cast<half8*>(o) = hi;
    *reinterpret_cast<half8*>(o + kKT) = lo;
  }
  if (range && bad) atomicAdd(range, bad);
}

// The argument rules and the launch of the three entries.  `allowed`: the flag bits the entry takes.  Everything that is an invalid
// argument is decided before anything that is unsupported, except the overlaps, which need the sizes.  `region`: the regional
// entry, whose own rules stand next to the shared ones of their kind: `rects`, a split input and two fp32 outputs (invalid
// otherwise); 3x3, stride 1, Cout % 128 == 0 and at most kRegionMaxObjects images (unsupported otherwise); no output on `rects`.
int conv_split_entry(const void* x, const void* wpack, const float* w_unscale, const float* shift, const float* res, int flags, int allowed,
                     int N, int H, int W, int Cin, int Cout, int ksize, int stride, void* out, float* out2, int out_split,
                     int32_t* range_word, void* stream, bool region = false, const int32_t* rects = nullptr) {
  if (!x || !wpack || !w_unscale || !out || N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return RMNET_E_INVALID_ARG;
  if (flags & ~allowed) return RMNET_E_INVALID_ARG;
  const bool xs = (flags & RMNET_CONV_X_SPLIT) != 0, os = (flags & RMNET_CONV_OUT_SPLIT) != 0;
  if (xs && (flags & RMNET_CONV_RELU_IN)) return RMNET_E_INVALID_ARG;      // (the producer of a split tensor applies it)
  if (os && out2) return RMNET_E_INVALID_ARG;
  if (region && (!rects || !xs || !out2 || (reinterpret_cast<uintptr_t>(rects) & 15))) return RMNET_E_INVALID_ARG;
  if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(wpack) | reinterpret_cast<uintptr_t>(w_unscale) |
       reinterpret_cast<uintptr_t>(shift) | reinterpret_cast<uintptr_t>(res) | reinterpret_cast<uintptr_t>(out) |
       reinterpret_cast<uintptr_t>(out2)) & 15)
    return RMNET_E_INVALID_ARG;
  if (out2 && (res || out_split <= 0 || out_split >= Cout || out_split % 4)) return RMNET_E_INVALID_ARG;
  if ((ksize != 1 && ksize != 3) || (stride != 1 && stride != 2)) return RMNET_E_UNSUPPORTED;
  if (Cin % kKT || Cout % 64) return RMNET_E_UNSUPPORTED;
  if (region && (ksize != 3 || stride != 1 || Cout % 128 || N > kRegionMaxObjects)) return RMNET_E_UNSUPPORTED;
  const int pad = ksize / 2;
  const int Ho = (H + 2 * pad - ksize) / stride + 1, Wo = (W + 2 * pad - ksize) / stride + 1;
  const long long Mi = (long long)N * H * W, M = (long long)N * Ho * Wo;
  if (Mi * Cin >= (1LL << 31) || M * Cout >= (1LL << 31)) return RMNET_E_UNSUPPORTED;   // (int pixel index, size_t offsets)
  // Either form has 4 bytes per element.  No output may overlap x (other workgroups read the same input pixels).  An fp32 out may BE
  // res: each element is read, then written, by one thread, and the epilogue's early reads are of exactly the elements that the
  // thread later writes.  A split out must not overlap res: its hi and lo chunks are not where the fp32 elements of the same
  // channels are
  const long long xbytes = Mi * Cin * 4, c1 = out2 ? out_split : Cout;
  if (overlap(out, M * c1 * 4, x, xbytes)) return RMNET_E_INVALID_ARG;
  if (os && res && overlap(out, M * c1 * 4, res, M * Cout * 4)) return RMNET_E_INVALID_ARG;
  if (out2) {
    if (overlap(out2, M * (Cout - c1) * 4, x, xbytes) || overlap(out2, M * (Cout - c1) * 4, out, M * c1 * 4)) return RMNET_E_INVALID_ARG;
  }
  if (region && (overlap(out, M * c1 * 4, rects, 16LL * N) || overlap(out2, M * (Cout - c1) * 4, rects, 16LL * N))) return RMNET_E_INVALID_ARG;
  RegionArgs a;
  a.rects = rects;
  a.x = xs ? nullptr : reinterpret_cast<const float*>(x);
  a.xs = xs ? reinterpret_cast<const _Float16*>(x) : nullptr;
  a.wp = reinterpret_cast<const u32x4*>(wpack); a.unscale = w_unscale; a.shift = shift; a.res = res;
  a.out = os ? nullptr : reinterpret_cast<float*>(out); a.out2 = out2; a.outs = os ? reinterpret_cast<_Float16*>(out) : nullptr;
  a.range = range_word; a.M = (int)M; a.H = H; a.W = W; a.Ho = Ho; a.Wo = Wo; a.Cin = Cin; a.Cout = Cout; a.csplit = (int)c1;
  a.ksize = ksize; a.stride = stride; a.pad = pad;
  a.relu_in = (flags & RMNET_CONV_RELU_IN) != 0;
  a.relu_out = (flags & RMNET_CONV_RELU_OUT) != 0;
  hipStream_t st = (hipStream_t)stream;
  if (region)       // the grid of the worst case, every cell inside its rectangle: the rectangles stay on the device
    hipLaunchKernelGGL(conv_split_region, dim3((unsigned)((a.M + 127) / 128), (unsigned)(a.Cout / 128)), dim3(kThreads), 0, st, a);
  else if (xs && os) launch_tile<true, true>(a, st);
  else if (xs) launch_tile<true, false>(a, st);
  else if (os) launch_tile<false, true>(a, st);
  else launch_tile<false, false>(a, st);
  return check_launch();
}

}  // namespace
}  // namespace rmnet

extern "C" int rmnet_conv_split_f32(const float* x, const void* wpack, const float* w_unscale, const float* shift,
                                    const float* res, int flags, int N, int H, int W, int Cin, int Cout, int ksize, int stride,
                                    float* out, float* out2, int out_split, int32_t* range_word, void* stream) {
  return rmnet::conv_split_entry(x, wpack, w_unscale, shift, res, flags, RMNET_CONV_RELU_IN | RMNET_CONV_RELU_OUT, N, H, W, Cin, Cout,
                                 ksize, stride, out, out2, out_split, range_word, stream);
}

extern "C" int rmnet_conv_split_pre_f32(const void* x, const void* wpack, const float* w_unscale, const float* shift, const float* res,
                                        int flags, int N, int H, int W, int Cin, int Cout, int ksize, int stride, void* out, float* out2,
                                        int out_split, int32_t* range_word, void* stream) {
  return rmnet::conv_split_entry(x, wpack, w_unscale, shift, res, flags,
                                 RMNET_CONV_RELU_IN | RMNET_CONV_RELU_OUT | RMNET_CONV_X_SPLIT | RMNET_CONV_OUT_SPLIT, N, H, W, Cin, Cout,
                                 ksize, stride, out, out2, out_split, range_word, stream);
}

extern "C" int rmnet_conv_split_region_f32(const void* x, const void* wpack, const float* w_unscale, const float* shift, int flags, int N,
                                           int H, int W, int Cin, int Cout, int ksize, int stride, const int32_t* rects, float* out,
                                           float* out2, int out_split, int32_t* range_word, void* stream) {
  return rmnet::conv_split_entry(x, wpack, w_unscale, shift, nullptr, flags, RMNET_CONV_RELU_OUT | RMNET_CONV_X_SPLIT, N, H, W, Cin, Cout,
                                 ksize, stride, out, out2, out_split, range_word, stream, true, rects);
}

extern "C" int rmnet_split_act_f32(const float* x, long long M, int C, int relu, void* out, int32_t* range_word, void* stream) {
  using namespace rmnet;
  if (!x || !out || M <= 0 || C <= 0) return RMNET_E_INVALID_ARG;
  if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out)) & 15) return RMNET_E_INVALID_ARG;
  if (C % kKT) return RMNET_E_UNSUPPORTED;
  if (M > (1LL << 40) / C) return RMNET_E_UNSUPPORTED;
  if (overlap(out, M * C * 4, x, M * C * 4)) return RMNET_E_INVALID_ARG;      // (an item's output is not where its input was)
  const size_t items = (size_t)M * C / 8;
  const size_t blocks = (items + kSplitActThreads - 1) / kSplitActThreads;
  const unsigned grid = (unsigned)(blocks < (size_t)kNumCUs * 8 ? blocks : (size_t)kNumCUs * 8);
  hipLaunchKernelGGL(split_act, dim3(grid), dim3(kSplitActThreads), 0, (hipStream_t)stream, x, reinterpret_cast<_Float16*>(out), items,
                     relu != 0, range_word);
  return check_launch();
}
