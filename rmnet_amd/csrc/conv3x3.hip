// conv3x3.hip -- 3x3 / stride 1 / pad 1 convolution, fp32 NHWC in and out, Cout = 256, on the fp16 MFMA
// pipes with split operands: the decoder's 256-channel convolutions (Decoder.convFM, ResMM, RF3, RF2).
//
// Arithmetic.  Every fp32 operand is split into fp16 hi + lo (hi = fp16(v), lo = fp16(v - hi): v = hi + lo
// to 2^-22 relative) and each product keeps three terms, Ah*Wh + Ah*Wl + Al*Wh, accumulated in fp32 by
// v_mfma_f32_16x16x32_f16 -- the scheme of bk_main<split> (bank.hip), fp32-class accuracy at 16/3 the
// rate of the fp32 MFMA.  Both operands are scaled by powers of two so that their lo planes stay out of
// fp16's subnormals (exact, undone in the epilogue):
//   weights      per output channel by 2^e, e chosen so that max |w[co]| * 2^e lies in [2^14, 2^15)
//                (done once by the packer, see include/rmnet_hip.h);
//   activations  by kActScale = 2^6 in the loader (the bank's window): |x| must stay below
//                65504 / 64 = 1023.5.  A value outside (or NaN / Inf) is clamped, and counted in the
//                caller's range word (each element once, at the centre tap): a non-zero word means
//                "redo these convolutions in fp32".
//
// GEMM view: M = N*H*W pixels, N = 256 output channels, K = 9*Cin ordered (tap, input channel), so
// one K step of 32 is one tap x 32 contiguous input channels of NHWC memory.
//
// Workgroup = 512 threads (8 waves) = 128 consecutive pixels x all 256 output channels; waves are
// 2 (pixels) x 4 (channels), each owns a 64 x 64 output tile = 4 x 4 MFMA tiles (2 x 64 accumulator
// VGPRs: hi*hi and the cross terms apart).  The per-tap halo is not staged: the 9 taps of a pixel tile re-read the same ~(128+2W)
// pixel rows, which stay in L2 between steps.
//
// Per K step (32 of K) and workgroup:
//   global reads   activations 128 px x 32 ch x 4 B  = 16 KB   (fp32; split in registers)
//                  weights     256 co x 32 x 2 planes x 2 B = 32 KB  (pre-split, pre-packed, L2-resident)
//   LDS            one buffer  X hi/lo [128][32] + W hi/lo [256][32] fp16 = 48 KB, two buffers = 96 KB = 98304 B, which is also
//                  what the kernel is allocated (tests/test_kernel_resources.py); one barrier per step (store the next step's
//                  tile while the MFMAs read this one)
//   LDS writes     48 KB: the next step's tile, nothing else.  The prefetched operands wait in VGPRs (2 x float4 of
//                  activations, 4 x 16 B of weights per thread): all six loads are issued before the step's first MFMA; the
//                  activations are waited for half way through the MFMAs, the weights after the last
//   LDS reads      per wave 8 A + 8 B fragments x 1 KB = 16 KB, per CU 128 KB (~512 clk at 256 B/clk)
//   MFMA           per wave 4 x 4 tiles x 3 terms = 48 x v_mfma_f32_16x16x32_f16 (16 clk) = 768 clk;
//                  two waves per SIMD -> 1536 clk per step per SIMD, which is the bound.
//   VALU split     8 elements per thread per step, ~75 VALU instructions per wave with their addresses: 300 clk per wave, 600 per
//                  SIMD, which is NOT negligible next to 1536 when it runs after the MFMAs (both waves of a SIMD share the one
//                  barrier per step, so they split at the same time and the matrix pipe stands idle).  It is therefore issued
//                  BETWEEN the MFMAs of the step's second half, one MFMA to three VALU instructions, and what it computes per
//                  step is only what changes per step: the K loop runs over the taps and, inside a tap, over the channel blocks,
//                  so the tap's offset and border test (a per-pixel 9-bit mask, a clamped address and a select of zero: no
//                  branch) are set once per tap, and the input ReLU and the range count are compiled into the loop instance
//                  that needs them (with / without ReLU x centre tap or not) instead of being tested per element.
// Ceiling at the 1/4-resolution shape (M = 414720, Cin = 256): 3240 workgroups, 72 steps each,
// 1536 clk/step -> ~13 rounds x 110 k clk / 2.4 GHz ~ 0.6 ms (= the 2.5 PF fp16 roof / 3).
//
// Two kernels.  All of the above is conv3x3_split, which rmnet_conv3x3_split_lds_f32 launches.  rmnet_conv3x3_split_f32 launches
// conv3x3_wreg (below conv3x3_split in this file): the same pixels, channels, arithmetic and K order, but the weights do not pass
// through LDS.  A weight fragment is used by two waves only in conv3x3_split's layout, and by one in conv3x3_wreg's, so each lane
// loads its own 16 bytes of it from the pack.  Per K step and workgroup, conv3x3_wreg:
//   global reads   as above: activations 16 KB, weights 32 KB (each byte by exactly one wave, in whole 1 KB fragments)
//   LDS            X hi/lo [128][32] fp16 = 16 KB per buffer, two buffers = 32768 B (= 2 * 2 * 128 * 32 * 2; tests/test_conv3x3_wreg.py)
//   LDS writes     16 KB (the next step's X tile); no weight writes (32 ds_write_b128 wave-instructions per step gone)
//   LDS reads      per wave 8 pixel tiles x hi/lo x 1 KB = 16 KB, per CU 128 KB as above, but all of it X; each tile's two reads are
//                  issued one tile (six MFMAs) ahead of their use
//   registers      weights 2 sets x 4 fragments x 4 VGPRs (this step's, the next step's), activations' prefetch 8, X fragments 16
//   MFMA           per wave 8 x 2 tiles x 3 terms = 48, the same 1536 clk per step and SIMD; the ceiling above is unchanged.
// Measured (profiles/r19_a_conv3x3_wreg.md): 4-7 % less time per call than conv3x3_split, the same bits.
//
// What the two kernels (and conv3x3_rows of csrc/conv3x3_rows.hip, which must return the same bits) have in common is written once,
// in csrc/conv3x3_parts.h: ConvArgs and the argument rules, the per-tap activation loader (border bits, set_tap, the two loads, the
// split into the X planes), the tap-class dispatch and the fp32 epilogue.  This file keeps what differs: the tile ownership, the
// weights' way, mma() and the K loops with their fences and groups (profiles/r32_a_decoder_conv_fold.md).
#include "conv3x3_parts.h"

namespace rmnet {
namespace {

constexpr int kXPlane = kMT * kKT;                 // halves per activation plane
constexpr int kWPlane = kCout * kKT;               // halves per weight plane
constexpr int kBufHalves = 2 * kXPlane + 2 * kWPlane;
static_assert(2 * kBufHalves * 2 <= kLdsBytesPerCU, "LDS budget");

__global__ __launch_bounds__(kThreads) void conv3x3_split(ConvArgs a) {
  __shared__ __attribute__((aligned(16))) _Float16 lds[2 * kBufHalves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave & 1, wn = wave >> 1;
  const int m0 = blockIdx.x * kMT;
  const int CB = a.Cin / kKT;

  TapLoader ld{a};
  ld.begin(tid, m0);
  // weights: 4 x 16 B per thread (chunk q = tid + 512i of the step's 2048); per step their uniform base moves by one step's pack
  u32x4 wr[4];
  const u32x4* wsrc = reinterpret_cast<const u32x4*>(a.wp);   // the step's pack (uniform)
  auto load = [&] {       // the next step's operands, activations first: the MFMA block waits for them alone half way
    ld.load();
#pragma unroll
    for (int i = 0; i < 4; ++i) wr[i] = wsrc[(unsigned)(tid + kThreads * i)];
    wsrc += 2 * kWPlane / 8;
  };
  auto store_w = [&](_Float16* buf) {
    _Float16* wb = buf + 2 * kXPlane;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int q = tid + kThreads * i;
      const int plane = q >> 10, co = (q >> 2) & (kCout - 1), ch = q & 3;
      *reinterpret_cast<u32x4*>(wb + plane * kWPlane + swz(co, ch)) = wr[i];
    }
  };

  // two accumulator sets: hi*hi, and the two cross terms (2^-11 smaller) -- the large sum then takes one rounding per K step
  // instead of three
  f32x4 acc[4][4], accx[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = accx[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  ld.set_tap(0);
  load();
  if (a.relu_in)
    ld.store<true, false>(lds);
  else
    ld.store<false, false>(lds);
  store_w(lds);
  __syncthreads();
  const int fr = lane & 15, fc = lane >> 4;
  auto mma = [&](const _Float16* __restrict__ cur, auto&& halfway) __attribute__((always_inline)) {
    const _Float16* xh = cur;
    const _Float16* xl = cur + kXPlane;
    const _Float16* wh = cur + 2 * kXPlane;
    const _Float16* wl = wh + kWPlane;
    half8 bh[4], bl[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int o = swz(wm * 64 + i * 16 + fr, fc);
      bh[i] = *reinterpret_cast<const half8*>(xh + o);
      bl[i] = *reinterpret_cast<const half8*>(xl + o);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int o = swz(wn * 64 + j * 16 + fr, fc);
      const half8 ah = *reinterpret_cast<const half8*>(wh + o);
      const half8 al = *reinterpret_cast<const half8*>(wl + o);
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bh[i], acc[i][j], 0, 0, 0);
#pragma unroll
      for (int i = 0; i < 4; ++i) accx[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bl[i], accx[i][j], 0, 0, 0);
#pragma unroll
      for (int i = 0; i < 4; ++i) accx[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, bh[i], accx[i][j], 0, 0, 0);
      if (j == 1) halfway();
    }
  };
  // The loop runs over the steps that are PREFETCHED, 1 .. steps-1 in K order, and multiplies the step before; the last step is
  // apart, so that the loop body has no branch around the loads and the stores: with one, the compiler cannot tell at the loop's
  // head which loads are still in flight and waits for the activation loads before it issues the weight loads and the MFMAs.
  // All of a step's global loads are issued before its first MFMA (the first fence).  Half way through the MFMAs the next step's
  // activations are split and written to the other buffer.  That block opens with a fence: left free, the compiler moves the whole
  // split in front of the step's first MFMA and waits for the activation loads there, which undoes the prefetch.  Behind the fence
  // the 24 sched_group_barrier pairs place the split's VALU work and the X-plane ds_writes BETWEEN the MFMAs of the second half,
  // one MFMA to three VALU instructions, where the matrix pipe covers them; with the fence alone they stay in one block between
  // the two halves.  The wait there is for the two activation loads only, the four weight loads stay in flight until the last MFMA
  // is issued (the last fence keeps their wait and their ds_writes behind it).  Writing the other buffer at any point of a step is
  // safe: its last readers were the MFMAs of the step before, and they finished before the barrier that ended that step -- which
  // is also what lets mma() take its source buffer as restrict: without it the fragment reads of the second half, and with them
  // its MFMAs, are ordered behind the X-plane writes and nothing overlaps.
  int par = 0;            // the buffer of the step that is multiplied
  auto run_taps = [&](auto relu, auto centre, int t0, int t1) __attribute__((always_inline)) {
#pragma unroll 1
    for (int tap = t0; tap < t1; ++tap) {
      if (tap) ld.set_tap(tap);
      const int n = tap ? CB : CB - 1;       // (tap 0's first block was the prologue's)
      for (int k = 0; k < n; ++k) {
        _Float16* nxt = lds + (par ^ 1) * kBufHalves;
        load();
        __builtin_amdgcn_sched_barrier(0);
        mma(lds + par * kBufHalves, [&] {
          __builtin_amdgcn_sched_barrier(0);
          ld.store<decltype(relu)::value, decltype(centre)::value>(nxt);
        });
#pragma unroll
        for (int g = 0; g < 24; ++g) {
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);     // one MFMA,
          __builtin_amdgcn_sched_group_barrier(0x002, 3, 0);     // three VALU instructions of the split
        }
        __builtin_amdgcn_sched_barrier(0);
        store_w(nxt);
        __syncthreads();
        par ^= 1;
      }
    }
  };
  run_tap_classes(a.relu_in, run_taps);
  mma(lds + par * kBufHalves, [] {});

  conv3x3_epilogue(a, acc, accx, m0 + wm * 64 + fr, wn * 64 + 4 * fc, ld.bad);   // pixels .. + 16i, channels .. + 16j ..
}


// ---------------------------------------------------------------------------------------------------------------- conv3x3_wreg
// The same convolution with the weights kept out of LDS (the banner's last part).  Arguments, loader and epilogue are the shared
// ones, arithmetic and K order per accumulator are conv3x3_split's, so outputs and range words are bit for bit the same; what differs:
//   waves        the 8 waves divide the 256 output channels: wave w owns all 128 pixels x channels 32w .. 32w+31 = 8 x 2 MFMA tiles
//                (still 48 MFMAs per wave and step, still 2 x 64 accumulator VGPRs).  No two waves need the same weight fragment.
//   weights      the A fragment of one MFMA tile (16 channels x 32 of K of one plane) is 1 KB of contiguous pack memory, and lane
//                (fr, fc) owns the 16 bytes at fr*64 + fc*16: one 16-byte load per lane and fragment, four per step (2 channel
//                tiles x hi / lo), straight into the VGPRs the next step's MFMAs read.  Two register sets take turns (the step
//                loop runs in pairs), so nothing is copied except once per tap when the tap's step count is odd.
//   activations  as in conv3x3_split: fp32 loads, tap mask, the split between the MFMAs of the step's second half, swizzled X
//                planes.  Every wave reads all eight pixel tiles' hi / lo fragments (16 KB per wave and step, what a wave of
//                conv3x3_split reads), each tile's two reads one tile ahead of the six MFMAs that use it.
//   LDS          X only: 2 buffers x 2 planes x [128][32] fp16 = 32768 B.
constexpr int kXBufHalves = 2 * kXPlane;

__global__ __launch_bounds__(kThreads) void conv3x3_wreg(ConvArgs a) {
  __shared__ __attribute__((aligned(16))) _Float16 lds[2 * kXBufHalves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, fc = lane >> 4;
  const int m0 = blockIdx.x * kMT;
  const int CB = a.Cin / kKT;

  TapLoader ld{a};
  ld.begin(tid, m0);
  // weight fragments [2 * channel tile + plane]: 16-byte chunk plane*1024 + co*4 + fc of the step's 2048, co = 32*wave + 16*j + fr
  half8 wa[4], wb[4];
  const half8* wsrc = a.wp;                                  // the step's pack (uniform)
  const unsigned wl = (wave * 32 + fr) * 4 + fc;             // the lane's chunk of channel tile 0, plane hi
  auto load_w = [&](half8(&w)[4]) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int p = 0; p < 2; ++p) w[2 * j + p] = wsrc[wl + (unsigned)(p * (kWPlane / 8) + j * 64)];
    wsrc += 2 * kWPlane / 8;
  };

  // acc[pixel tile][channel tile]: hi*hi, and the two cross terms, as in conv3x3_split
  f32x4 acc[8][2], accx[8][2];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = accx[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  ld.set_tap(0);
  ld.load();
  load_w(wa);
  if (a.relu_in)
    ld.store<true, false>(lds);
  else
    ld.store<false, false>(lds);
  __syncthreads();
  // One pixel tile at a time: its hi / lo fragments, then its six MFMAs -- per accumulator Ah*Bh, then Ah*Bl, then Al*Bh, which is
  // conv3x3_split's order.  (The swizzle term of a fragment's address depends on fr alone: the eight tiles are 1 KB apart.)
  auto mma = [&](const _Float16* __restrict__ cur, const half8(&w)[4], auto&& halfway) __attribute__((always_inline)) {
    const _Float16* xh = cur + swz(fr, fc);
    const _Float16* xl = xh + kXPlane;
    half8 bh[2], bl[2];       // tile i + 1's fragments are read in front of tile i's MFMAs
    bh[0] = *reinterpret_cast<const half8*>(xh);
    bl[0] = *reinterpret_cast<const half8*>(xl);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      if (i + 1 < 8) {
        bh[(i + 1) & 1] = *reinterpret_cast<const half8*>(xh + (i + 1) * 16 * kKT);
        bl[(i + 1) & 1] = *reinterpret_cast<const half8*>(xl + (i + 1) * 16 * kKT);
      }
      const half8 h = bh[i & 1], l = bl[i & 1];
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w[2 * j], h, acc[i][j], 0, 0, 0);
#pragma unroll
      for (int j = 0; j < 2; ++j) accx[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w[2 * j], l, accx[i][j], 0, 0, 0);
#pragma unroll
      for (int j = 0; j < 2; ++j) accx[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w[2 * j + 1], h, accx[i][j], 0, 0, 0);
      if (i == 3) halfway();
    }
  };
  // A step: all six loads of the next step first (the weights into the register set this step does not read), the MFMAs of this
  // one, the next step's activation split between the MFMAs of the second half (conv3x3_split's fences and groups), the barrier.
  // The weight loads stay in flight across the barrier: their first readers are the next step's MFMAs.
  int par = 0;
  auto step = [&](auto relu, auto centre, const half8(&wc)[4], half8(&wn)[4]) __attribute__((always_inline)) {
    _Float16* nxt = lds + (par ^ 1) * kXBufHalves;
    ld.load();
    __builtin_amdgcn_sched_barrier(0);     // (activations first: the split half way waits for them alone, by count)
    load_w(wn);
    __builtin_amdgcn_sched_barrier(0);
    mma(lds + par * kXBufHalves, wc, [&] {
      __builtin_amdgcn_sched_barrier(0);
      ld.store<decltype(relu)::value, decltype(centre)::value>(nxt);
    });
#pragma unroll
    for (int g = 0; g < 24; ++g) {
      if (g % 6 == 0 && g < 18) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);     // the next tile's two fragment reads
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);     // one MFMA,
      __builtin_amdgcn_sched_group_barrier(0x002, 3, 0);     // three VALU instructions of the split
    }
    __builtin_amdgcn_sched_barrier(0);
    __syncthreads();
    par ^= 1;
  };
  auto run_taps = [&](auto relu, auto centre, int t0, int t1) __attribute__((always_inline)) {
#pragma unroll 1
    for (int tap = t0; tap < t1; ++tap) {
      if (tap) ld.set_tap(tap);
      const int n = tap ? CB : CB - 1;       // (tap 0's first block was the prologue's)
      int k = 0;
#pragma unroll 1
      for (; k + 1 < n; k += 2) {            // in pairs: the two weight sets change roles, no copy
        step(relu, centre, wa, wb);
        step(relu, centre, wb, wa);
      }
      if (k < n) {                           // an odd count: one more step, and the sets change names
        step(relu, centre, wa, wb);
#pragma unroll
        for (int f = 0; f < 4; ++f) wa[f] = wb[f];
      }
    }
  };
  run_tap_classes(a.relu_in, run_taps);
  mma(lds + par * kXBufHalves, wa, [] {});

  conv3x3_epilogue(a, acc, accx, m0 + fr, wave * 32 + 4 * fc, ld.bad);      // pixels m0 + 16i + fr, channels 32*wave + 16j + 4*fc ..
}

// both entries: the argument rules of conv3x3_parts.h, one kernel each
int conv3x3_launch(void (*kernel)(ConvArgs), const float* x, const void* wpack, const float* w_unscale, const float* bias,
                   const float* res, int flags, int N, int H, int W, int Cin, float* out, int32_t* range_word, void* stream) {
  ConvArgs a;
  const int rc = conv3x3_args(a, x, wpack, w_unscale, bias, res, flags, N, H, W, Cin, out, range_word);
  if (rc != RMNET_OK) return rc;
  hipLaunchKernelGGL(kernel, dim3((unsigned)((a.M + kMT - 1) / kMT)), dim3(kThreads), 0, (hipStream_t)stream, a);
  return check_launch();
}

}  // namespace
}  // namespace rmnet

extern "C" int rmnet_conv3x3_split_f32(const float* x, const void* wpack, const float* w_unscale, const float* bias,
                                       const float* res, int flags, int N, int H, int W, int Cin, float* out,
                                       int32_t* range_word, void* stream) {
  return rmnet::conv3x3_launch(rmnet::conv3x3_wreg, x, wpack, w_unscale, bias, res, flags, N, H, W, Cin, out, range_word, stream);
}

extern "C" int rmnet_conv3x3_split_lds_f32(const float* x, const void* wpack, const float* w_unscale, const float* bias,
                                           const float* res, int flags, int N, int H, int W, int Cin, float* out,
                                           int32_t* range_word, void* stream) {
  return rmnet::conv3x3_launch(rmnet::conv3x3_split, x, wpack, w_unscale, bias, res, flags, N, H, W, Cin, out, range_word, stream);
}
