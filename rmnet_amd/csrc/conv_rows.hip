// conv_rows.hip -- the trunks' 3x3 / stride 1 / pad 1 bottleneck convolutions with Cin = Cout = C in {64, 128, 256} on pre-split
// activations (csrc/conv_split.hip: conv_split_pre with RMNET_CONV_X_SPLIT -- its arithmetic, arguments and results, bit for bit),
// with the activations of a whole tap ROW staged in LDS once.  The design is conv3x3_rows's (csrc/conv3x3_rows.hip; read its header
// first): what follows says what is the same and what differs.
//
// The same:
//   * K order (tap 0..8, channel block 0..C/32-1); per step and pixel tile Ah*Wh into acc, then Ah*Wl, then Al*Wh into accx: this is
//     conv_split's order, so every accumulator sees the same operands in the same order whatever the wave layout;
//   * a workgroup of 512 threads owns MT consecutive pixels of the linear NHWC index and ALL C output channels, and stages the
//     MT + 2 pixels m0 + dy*W - 1 .. m0 + dy*W + MT of one tap row once (three stagings, six barriers per workgroup); the three taps
//     of the row then run without a global activation load, an LDS write or a barrier;
//   * staged rows are never masked: a lane selects, once per (pixel tile, tap), its real LDS row or the row of zeros that lies in the
//     same 16-byte slot of the bank row (four zero rows per plane) -- the +0.0 operand bits that conv_split_pre's loader puts in
//     place of a tap outside the map.  Staged pixels outside [0, M) are read from a clamped address; all their readers are masked;
//   * weight fragments go straight from the pack into two alternating register sets, one step ahead, no weight LDS;
//   * the fragment reads' swizzle (16-byte chunk XOR 2 * bit 2 of the row) and the zero-row choice: they depend on the row, the
//     64-byte row pitch and (MT + 2) % 4 == 2 alone, which hold for every MT here.
// What differs:
//   * geometry: MT x C = 32768, i.e. MT = 128, 256, 512 for C = 256, 128, 64; the 8 waves are (MT / 128) x (C / 32), each owning
//     128 pixels x 32 channels (acc[8][2], accx[8][2]).  LDS image [channel block][plane hi, lo][MT + 2 staged + 4 zero rows][32]
//     fp16 = (MT + 6) x C x 4 B = 137216, 134144, 132608 B (dynamic);
//   * staging is a copy: the input is already split, and a 16-byte chunk of the split form is 8 halves of one plane -- a chunk of
//     the image.  Thread -> (chunk tid % 4, row parity tid / 4 % 2, plane tid / 8 % 2, channel block tid / 16 % CB, row pair
//     tid / 16 / CB) of each pass of 64 / CB rows, 16 passes.  A ds_write_b128 is served in groups of 8 consecutive lanes on 32
//     banks: the 8 lanes write an even row and the next (2 x 64 B, whatever the chunk swizzle does inside a row), i.e. all eight
//     16-byte slots of a 128-byte bank row -- conflict-free.  (A pixel's hi and lo chunks in one group would meet: the planes lie a
//     multiple of 128 B apart.)  4 lanes read 64 contiguous bytes, 16 lanes two pixels' 128, a wave whole 128-byte lines;
//   * nothing is counted for the input (its producer did).  The epilogue is conv_split_pre's, expression for expression: unscale,
//     shift, ReLU, and for a split output split4 with its count of the produced elements outside the window.
// No residual and no second output: those calls stay on conv_split_pre.  Measured: profiles/r21_a_trunk_rows.md.
#include <mutex>

#include "common.h"

namespace rmnet {
namespace {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

constexpr int kKT = 32;          // K per step (one tap x 32 input channels)
constexpr int kThreads = 512;
constexpr float kActScale = 64.0f;                 // 2^6
constexpr float kActUnscale = 1.0f / 64.0f;
constexpr float kF16Max = 65504.0f;
constexpr int kTileElems = 32768;                  // MT x C
constexpr int kZeroRows = 4;                       // rows of zeros behind the staged ones: 256 B, one 16-byte slot for every slot of a bank row
constexpr int kAhead = 1;                          // pixel tiles that the fragment reads run ahead of their MFMAs
constexpr int kStageBatch = 8;                     // staging loads in flight per thread before the first LDS write
constexpr int kStagePasses = 16;                   // 512 chunks per pass: MT x C / 4 chunks in 16 passes

constexpr int rows_mt(int C) { return kTileElems / C; }
constexpr int rows_lds_bytes(int C) { return (rows_mt(C) + 2 + kZeroRows) * C * 4; }
static_assert(rows_lds_bytes(256) == 137216 && rows_lds_bytes(128) == 134144 && rows_lds_bytes(64) == 132608, "(MT + 6) rows x C x 4 B");
static_assert(rows_lds_bytes(256) <= kLdsBytesPerCU, "LDS budget");

// halves from the start of a plane to 16-byte chunk `chunk` of row `row` (conv3x3_rows's swizzle)
__device__ inline int swzr(int row, int chunk) { return row * kKT + ((chunk ^ ((row >> 1) & 2)) << 3); }

// conv_split_pre's split4 (csrc/conv_split.hip), expression for expression
__device__ inline void split4(const f32x4 v, half4& hi, half4& lo, int& bad) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float y = v[e] * kActScale;
    bad += !(fabsf(y) <= kF16Max) ? 1 : 0;
    const float c = fminf(fmaxf(y, -kF16Max), kF16Max);
    const _Float16 h = (_Float16)c;
    hi[e] = h;
    lo[e] = (_Float16)(c - (float)h);
  }
}

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

extern __shared__ __attribute__((aligned(16))) _Float16 conv_rows_lds[];      // rows_lds_bytes(C), sized at launch

template <int C, bool OS>
__global__ __launch_bounds__(kThreads) void conv_rows(RowsArgs a) {
  constexpr int MT = rows_mt(C);                     // pixels per workgroup
  constexpr int CB = C / kKT;                        // channel blocks
  constexpr int kStaged = MT + 2;                    // staged pixel rows of a tap row
  constexpr int kPlaneHalves = (kStaged + kZeroRows) * kKT;   // one plane of one channel block
  constexpr int kBlockHalves = 2 * kPlaneHalves;     // hi + lo
  constexpr int kWPlane = C * kKT;                   // halves per weight plane of the pack
  constexpr int kPassRows = 2 * (kThreads / 16) / CB;          // rows per staging pass
  static_assert(C % kKT == 0 && CB % 2 == 0 && MT % 128 == 0 && (MT / 128) * CB == 8, "8 waves of 128 pixels x 32 channels");
  static_assert(kStaged % 4 == 2, "the zero row of a masked lane: (kStaged + (row + 2) % 4) % 4 == row % 4");
  static_assert(kPassRows % 8 == 0 && kPassRows * kStagePasses == MT, "a pass keeps the swizzle bit; 16 passes stage MT rows");
  static_assert(kStagePasses % kStageBatch == 0, "whole batches");
  _Float16* const lds = conv_rows_lds;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wc = wave % CB, wp = wave / CB;          // the wave's channels 32 wc .., its pixels 128 wp ..
  const int fr = lane & 15, fc = lane >> 4;
  const int m0 = blockIdx.x * MT;
  const int HW = a.H * a.W;

  // the zero rows: 2 CB planes x 256 B, 16 bytes per thread
  if (tid < 16 * 2 * CB) *reinterpret_cast<half8*>(lds + (tid >> 4) * kPlaneHalves + kStaged * kKT + 8 * (tid & 15)) = half8{0, 0, 0, 0, 0, 0, 0, 0};

  // the border test, once per pixel: bit t of pixel tile i's 9 bits = tap t of pixel m0 + 128 wp + 16i + fr lies inside the map (past
  // M: none does) -- conv_split_pre's test, for the pixels whose fragments this lane reads; three tiles per register
  unsigned inside[3] = {0u, 0u, 0u};
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int m = m0 + 128 * wp + 16 * i + fr;
    const bool pin = m < a.M;
    const int r = (pin ? m : 0) % HW;
    const int ph = r / a.W, pw = r % a.W;
    unsigned bits = 0;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int h = ph + t / 3 - 1, w = pw + t % 3 - 1;
      bits |= (pin && h >= 0 && h < a.H && w >= 0 && w < a.W ? 1u : 0u) << t;
    }
    inside[i / 3] |= bits << (9 * (i % 3));
  }

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

  // weight fragments [2 * channel tile + plane]: 16-byte chunk plane * 4C + co * 4 + fc of the step's 8C, co = 32 wc + 16 j + fr; the
  // pack is walked step by step, and the last step loads its own fragments again
  half8 wa[4], wb[4];
  const half8* wsrc = a.wp;                                  // the pack of the step that is loaded next (uniform)
  const half8* const wlast = a.wp + (9 * CB - 1) * (2 * kWPlane / 8);
  const unsigned wl = (wc * 32 + fr) * 4 + fc;
  auto load_w = [&](half8(&w)[4]) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int p = 0; p < 2; ++p) w[2 * j + p] = wsrc[wl + (unsigned)(p * (kWPlane / 8) + j * 64)];
    wsrc = wsrc == wlast ? wsrc : wsrc + 2 * kWPlane / 8;
  };

  // acc[pixel tile][channel tile]: hi*hi, and the two cross terms, as in conv_split
  f32x4 acc[8][2], accx[8][2];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = accx[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // One tap = CB steps from the staged row image, free-running (conv3x3_rows's run_tap).  Per pixel tile the lane's read address is
  // chosen once per tap: row 128 wp + 16i + fr + dx + 1 (swizzled), or the zero row when the tap of that pixel is outside the map.
  auto run_tap = [&](int tap) __attribute__((always_inline)) {
    const int dx1 = tap % 3;                                 // dx + 1
    unsigned ao[8];                                          // halves
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const bool in = (inside[i / 3] >> (9 * (i % 3) + tap)) & 1;
      const int row = 128 * wp + 16 * i + fr + dx1;
      const unsigned real = (unsigned)swzr(row, fc);
      // the zero row that lies in the same 16-byte slot of the 256-byte bank row as the real one
      ao[i] = in ? real : (unsigned)((kStaged + ((row + 2) & 3)) * kKT) + (real & (kKT - 1));
    }
    half8 bh[kAhead + 1], bl[kAhead + 1];
    auto frag = [&](int n) __attribute__((always_inline)) {  // tile n % 8 of step n / 8 of the tap
      const _Float16* p = lds + ao[n & 7] + (n >> 3) * kBlockHalves;
      bh[n % (kAhead + 1)] = *reinterpret_cast<const half8*>(p);
      bl[n % (kAhead + 1)] = *reinterpret_cast<const half8*>(p + kPlaneHalves);
    };
    auto mma = [&](int cb, const half8(&w)[4]) __attribute__((always_inline)) {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        if (8 * cb + i + kAhead < 8 * CB) frag(8 * cb + i + kAhead);
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
    // tile's two fragment reads and this tile's six MFMAs, in that order
    auto step = [&](int cb, const half8(&wcur)[4], half8(&wnxt)[4]) __attribute__((always_inline)) {
      __builtin_amdgcn_sched_barrier(0);
      load_w(wnxt);
      __builtin_amdgcn_sched_barrier(0);
      mma(cb, wcur);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);   // the next tile's two fragment reads
        __builtin_amdgcn_sched_group_barrier(0x008, 6, 0);   // six MFMAs
      }
    };
#pragma unroll
    for (int n = 0; n < kAhead; ++n) frag(n);
#pragma unroll
    for (int cb = 0; cb < CB; cb += 2) {                     // in pairs: the two weight sets change roles, no copy
      step(cb, wa, wb);
      step(cb + 1, wb, wa);
    }
    __builtin_amdgcn_sched_barrier(0);
  };

  load_w(wa);
#pragma unroll 1
  for (int ty = 0; ty < 3; ++ty) {
    __syncthreads();                                         // the readers of the row image have finished
    stage(ty);
    __syncthreads();
#pragma unroll 1
    for (int tx = 0; tx < 3; ++tx) run_tap(3 * ty + tx);
  }

  // epilogue: conv_split_pre's without the residual, expression for expression (pixel m0 + 128 wp + 16i + fr, channels
  // 32 wc + 16j + 4 fc ..)
  int me = m0 + 128 * wp;                                    // (opaque: the pixel indices are formed again here; taken from the
  asm volatile("" : "+v"(me));                               // mask computation they stay live across the K loop)
  int bad = 0;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int co = wc * 32 + j * 16 + 4 * fc;
    const f32x4 us = *reinterpret_cast<const f32x4*>(a.unscale + co) * kActUnscale;
    const f32x4 b = a.shift ? *reinterpret_cast<const f32x4*>(a.shift + co) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i][j] = (acc[i][j] + accx[i][j]) * us + b;
  }
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int i = 0; i < 8; ++i) asm volatile("" : "+v"(acc[i][j]));
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int co = wc * 32 + j * 16 + 4 * fc;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int m = me + i * 16 + fr;
      if (m >= a.M) continue;
      f32x4 v = acc[i][j];
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

// A dynamic LDS request above 64 KB needs the function attribute; it is set once per device and instance, at the first launch, and
// never while the stream is capturing (a first launch inside a capture is refused: run the convolution once eagerly before
// capturing) -- conv3x3_rows's rows_prepare.
template <int C, bool OS>
int rows_launch(const RowsArgs& a, hipStream_t st) {
  static std::mutex mu;
  static bool done[64] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return RMNET_E_LAUNCH;
  {
    std::lock_guard<std::mutex> lock(mu);
    if (!done[dev]) {
      hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
      if (hipStreamIsCapturing(st, &cs) != hipSuccess) return RMNET_E_LAUNCH;
      if (cs != hipStreamCaptureStatusNone) return RMNET_E_UNSUPPORTED;
      if (hipFuncSetAttribute(reinterpret_cast<const void*>(conv_rows<C, OS>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              rows_lds_bytes(C)) != hipSuccess)
        return RMNET_E_LAUNCH;
      done[dev] = true;
    }
  }
  hipLaunchKernelGGL((conv_rows<C, OS>), dim3((unsigned)((a.M + rows_mt(C) - 1) / rows_mt(C))), dim3(kThreads), rows_lds_bytes(C), st, a);
  return check_launch();
}

inline bool overlap(const void* p, long long pn, const void* q, long long qn) {
  const char* a = reinterpret_cast<const char*>(p);
  const char* b = reinterpret_cast<const char*>(q);
  return a < b + qn && b < a + pn;
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
