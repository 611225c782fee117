// conv_rows_core.h -- the tap-row engine of the 3x3 / stride 1 / pad 1 split-fp16 convolutions that stage the activations of a whole
// tap ROW in LDS once: conv3x3_rows (csrc/conv3x3_rows.hip, the decoder, fp32 input) and conv_rows<C, OS> (csrc/conv_rows.hip, the
// trunks, split input).  Those files keep their staging, their epilogue tails and their exports; everything between is here, once.
//
// The row image.  A workgroup of 512 threads owns the MT consecutive pixels m0 .. m0+MT-1 of the linear NHWC pixel index and all
// C = Cin = Cout channels.  The three taps of one tap row (dy fixed, dx = -1, 0, +1) read the MT + 2 consecutive pixels
// m0 + dy*W - 1 .. m0 + dy*W + MT, shifted by one pixel per tap.  So a tap row is staged once (3 stagings and six barriers per
// workgroup), and the 3 taps x C/32 channel blocks that read it run without a global activation load, an LDS write or a barrier.
//   LDS (dynamic, rows_image_bytes(C, MT)): [channel block 0..C/32-1][plane hi, lo][MT + 2 staged + 4 zero rows][32] fp16, 64-byte
//   rows: (MT + 6) x C x 4 B.  MT x C = 32768 fills the CU's 160 KiB: 137216, 134144, 132608 B for C = 256, 128, 64.
// The 8 waves are (MT / 128) x (C / 32): a wave owns 128 pixels (8 tiles of 16, from pixel offset `pix`) x 32 channels (2 tiles of 16,
// wave column `wcol`): acc[8][2] / accx[8][2].
//
// Why the bits equal those of the per-tap kernels (conv3x3_wreg of csrc/conv3x3.hip, conv_split's split-input instances of csrc/conv_split.hip):
//   * steps run in (tap 0..8, channel block 0..C/32-1) order; per step and pixel tile Ah*Wh into acc, then Ah*Wl, then Al*Wh into
//     accx: every accumulator sees the same operands in the same order, whatever the wave layout;
//   * the weight fragments go straight from the pack into two alternating register sets, one step ahead, no weight LDS;
//   * the per-element split (split4) and the epilogue head (unscale_shift) are the ones of split_f16.h;
//   * the border test (taps_inside, split_f16.h) moved, its result did not.  The per-tap loaders replace the value of a tap outside the map by zero before the
//     split; here a staged row serves three taps of different pixels (the row that is the dx = 0 tap of one pixel is the row-wrap
//     neighbour for dx = -1 of the next), so the staged rows are never masked.  Instead each lane selects, once per (pixel tile, tap),
//     the LDS row it reads: the real row, or one of the plane's rows of zeros -- the same +0.0 operand bits.  Staged pixels outside
//     [0, M) are read from a clamped address inside the tensor; every reader of such a row is a masked tap.
//
// Zero rows: four per plane (256 B, written once at the start), so that a masked lane can read its zeros from the 16-byte slot of the
// bank row that its real row lies in: kStaged + (row + 2) % 4 = row mod 4, given (MT + 2) % 4 == 2.  With ONE zero row the masked
// lanes met the real rows of their lane group on the same banks (measured on conv3x3_rows: SQ_LDS_BANK_CONFLICT 4 % of the LDS
// cycles at 1/4 resolution, 14 % at 1/16, where more pixels lie on a border).
// Swizzle: the 16-byte chunk index is XORed with 2 * (bit 2 of the row).  A ds_read_b128 is served in four groups of 16 lanes, each
// of which holds, for every row residue mod 4, the rows R, R+12 at chunk c and R+4, R+8 at chunk c^1 (c = 0 or 2): with this
// swizzle the four land in four different 16-byte slots of the 256-byte bank row for any R, i.e. for all three row shifts.  It
// depends on the row and the 64-byte row pitch alone; a staging pass that advances by a multiple of 8 rows keeps the swizzle bit.
// Measured: profiles/r20_a_conv3x3_rows.md, profiles/r21_a_trunk_rows.md, profiles/r22_a_rows_core.md.
#pragma once

#include <mutex>

#include "split_f16.h"      // the vector types, kKT, kThreads, the activation scale, split4, overlap

namespace rmnet {
namespace {

constexpr int kZeroRows = 4;                      // rows of zeros behind the staged ones: 256 B, one 16-byte slot for every slot of a bank row
constexpr int kAhead = 1;                          // pixel tiles that the fragment reads run ahead of their MFMAs (2 and 3: the same time)

constexpr int rows_image_bytes(int C, int MT) { return (MT + 2 + kZeroRows) * C * 4; }

// halves from the start of a plane to 16-byte chunk `chunk` of row `row`
__device__ inline int swzr(int row, int chunk) { return row * kKT + ((chunk ^ ((row >> 1) & 2)) << 3); }

extern __shared__ __attribute__((aligned(16))) _Float16 rows_lds[];      // rows_image_bytes(C, MT), sized at launch

template <int C, int MT>
struct RowsCore {
  static constexpr int kCB = C / kKT;                         // channel blocks
  static constexpr int kStaged = MT + 2;                      // staged pixel rows of a tap row
  static constexpr int kPlaneHalves = (kStaged + kZeroRows) * kKT;   // one plane of one channel block
  static constexpr int kBlockHalves = 2 * kPlaneHalves;       // hi + lo
  static constexpr int kWPlane = C * kKT;                     // halves per weight plane of the pack
  static_assert(C % kKT == 0 && kCB % 2 == 0 && MT % 128 == 0 && (MT / 128) * kCB == 8, "8 waves of 128 pixels x 32 channels");
  static_assert(kStaged % 4 == 2, "the zero row of a masked lane: (kStaged + (row + 2) % 4) % 4 == row % 4");
  static_assert(kCB * kBlockHalves * 2 == rows_image_bytes(C, MT), "the image");

  int fr, fc, pix;
  unsigned inside[3];
  // weight fragments [2 * channel tile + plane]: 16-byte chunk plane * 4C + co * 4 + fc of the step's 8C, co = 32 wcol + 16 j + fr; the
  // pack is walked step by step, and the last step loads its own fragments again
  half8 wa[4], wb[4];
  const half8* wsrc;                                          // the pack of the step that is loaded next (uniform)
  const half8* wlast;
  unsigned wl;
  f32x4 acc[8][2], accx[8][2];                                // [pixel tile][channel tile]: hi*hi, and the two cross terms

  // m1: the wave's first pixel, m0 + pix
  __device__ __forceinline__ void begin(int tid, int wcol, int pix_, int m1, const half8* wp, int M, int H, int W) {
    fr = tid & 15, fc = (tid & 63) >> 4, pix = pix_;
    // the zero rows: 2 kCB planes x 256 B, 16 bytes per thread
    if (tid < 16 * 2 * kCB) *reinterpret_cast<half8*>(rows_lds + (tid >> 4) * kPlaneHalves + kStaged * kKT + 8 * (tid & 15)) = half8{0, 0, 0, 0, 0, 0, 0, 0};
    // the border test, once per pixel: bit t of pixel tile i's 9 bits = tap t of pixel m1 + 16i + fr lies inside the map (past M: none
    // does) -- the per-tap loaders' test, for the pixels whose fragments this lane reads; three tiles per register
    inside[0] = inside[1] = inside[2] = 0u;
#pragma unroll
    for (int i = 0; i < 8; ++i) inside[i / 3] |= taps_inside(m1 + 16 * i + fr, M, H, W) << (9 * (i % 3));
    wsrc = wp;
    wlast = wp + (9 * kCB - 1) * (2 * kWPlane / 8);
    wl = (wcol * 32 + fr) * 4 + fc;
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[i][j] = accx[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    load_w(wa);
  }

  __device__ __forceinline__ void load_w(half8 (&w)[4]) {
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int p = 0; p < 2; ++p) w[2 * j + p] = wsrc[wl + (unsigned)(p * (kWPlane / 8) + j * 64)];
    wsrc = wsrc == wlast ? wsrc : wsrc + 2 * kWPlane / 8;
  }

  // One tap = kCB steps from the staged row image, free-running.  Per pixel tile the lane's read address is chosen once per tap:
  // row pix + 16i + fr + dx + 1 (swizzled), or the zero row when the tap of that pixel is outside the map.  The channel block and the
  // plane are constant offsets.  Fragments are read one tile ahead of their six MFMAs, across the step boundaries too.
  __device__ __forceinline__ void run_tap(int tap) {
    const int dx1 = tap % 3;                                 // dx + 1
    unsigned ao[8];                                          // halves
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const bool in = (inside[i / 3] >> (9 * (i % 3) + tap)) & 1;
      const int row = pix + 16 * i + fr + dx1;
      const unsigned real = (unsigned)swzr(row, fc);
      // the zero row that lies in the same 16-byte slot of the 256-byte bank row as the real one: a masked lane then conflicts with
      // no lane of its group, whatever the other lanes read
      ao[i] = in ? real : (unsigned)((kStaged + ((row + 2) & 3)) * kKT) + (real & (kKT - 1));
    }
    half8 bh[kAhead + 1], bl[kAhead + 1];
    auto frag = [&](int n) __attribute__((always_inline)) {  // tile n % 8 of step n / 8 of the tap
      const _Float16* p = rows_lds + ao[n & 7] + (n >> 3) * kBlockHalves;
      bh[n % (kAhead + 1)] = *reinterpret_cast<const half8*>(p);
      bl[n % (kAhead + 1)] = *reinterpret_cast<const half8*>(p + kPlaneHalves);
    };
    auto mma = [&](int cb, const half8(&w)[4]) __attribute__((always_inline)) {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        if (8 * cb + i + kAhead < 8 * kCB) frag(8 * cb + i + kAhead);
        const half8 h = bh[(8 * cb + i) % (kAhead + 1)], l = bl[(8 * cb + i) % (kAhead + 1)];
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w[2 * j], h, acc[i][j], 0, 0, 0);
#pragma unroll
        for (int j = 0; j < 2; ++j) accx[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w[2 * j], l, accx[i][j], 0, 0, 0);
#pragma unroll
        for (int j = 0; j < 2; ++j) accx[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w[2 * j + 1], h, accx[i][j], 0, 0, 0);
      }
    };
    // a step: the four weight loads of the next step first (into the set this step does not read), then per pixel tile the next
    // tile's two fragment reads and this tile's six MFMAs, in that order (left free, the reads sink to just in front of their
    // MFMAs and every tile waits out the LDS latency)
    auto step = [&](int cb, const half8(&wc)[4], half8(&wn)[4]) __attribute__((always_inline)) {
      __builtin_amdgcn_sched_barrier(0);
      load_w(wn);
      __builtin_amdgcn_sched_barrier(0);
      mma(cb, wc);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);   // the next tile's two fragment reads
        __builtin_amdgcn_sched_group_barrier(0x008, 6, 0);   // six MFMAs
      }
    };
#pragma unroll
    for (int n = 0; n < kAhead; ++n) frag(n);
#pragma unroll
    for (int cb = 0; cb < kCB; cb += 2) {                    // in pairs: the two weight sets change roles, no copy
      step(cb, wa, wb);
      step(cb + 1, wb, wa);
    }
    __builtin_amdgcn_sched_barrier(0);
  }

  // the epilogue's head (split_f16.h) for channels 32 wcol + 16 j + 4 fc ..
  __device__ __forceinline__ void unscale_shift(const float* unscale, const float* shift, int wcol) {
    rmnet::unscale_shift(acc, accx, unscale, shift, wcol * 32 + 4 * fc);
  }
};

// A dynamic LDS request above 64 KB needs the function attribute; it is set once per device and kernel instance, at the first launch,
// and never while the stream is capturing (a first launch inside a capture is refused: run the convolution once eagerly before
// capturing).
template <auto Kernel, int kBytes>
int rows_prepare(hipStream_t st) {
  static std::mutex mu;
  static bool done[64] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return RMNET_E_LAUNCH;
  std::lock_guard<std::mutex> lock(mu);
  if (done[dev]) return RMNET_OK;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(st, &cs) != hipSuccess) return RMNET_E_LAUNCH;
  if (cs != hipStreamCaptureStatusNone) return RMNET_E_UNSUPPORTED;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kBytes) != hipSuccess)
    return RMNET_E_LAUNCH;
  done[dev] = true;
  return RMNET_OK;
}

}  // namespace
}  // namespace rmnet
