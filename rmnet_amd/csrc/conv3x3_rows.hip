// conv3x3_rows.hip -- the decoder's 3x3 / stride 1 / pad 1 convolution with Cin = Cout = 256 (csrc/conv3x3.hip's arithmetic,
// arguments and results, bit for bit), with the activations of a whole tap ROW staged in LDS once.
//
// How it differs from the two kernels of conv3x3.hip.  Those walk K = (tap, channel block) with an LDS tile of one tap x 32
// channels: every activation is fetched, ReLU'd, scaled, clamped, split and written to LDS nine times, once per tap, and every one
// of the 72 K steps ends in a workgroup barrier.  Here the K order is the same, but the LDS holds one tap row x ALL 256 channels:
//   a workgroup owns the 128 consecutive pixels m0 .. m0+127 of the linear NHWC pixel index.  The three taps of one tap row
//   (dy fixed, dx = -1, 0, +1) read the 130 consecutive pixels m0 + dy*W - 1 .. m0 + dy*W + 128, shifted by one pixel per tap.
//   130 pixels x 256 channels x (hi + lo) x 2 B = 133120 B fit the CU's 160 KiB.  So a tap row is staged once (3 times per
//   workgroup instead of 9, and 3 x 130 instead of 9 x 128 pixel rows of global traffic), and the 3 taps x 8 channel blocks =
//   24 K steps that read it run without a global activation load, a split, an LDS write or a barrier: six barriers per
//   workgroup instead of 72.
//
// What is kept from conv3x3_wreg, and why the bits are equal:
//   * 512 threads; wave w owns all 128 pixels x channels 32w .. 32w+31 (acc[8][2] / accx[8][2]);
//   * steps run in (tap 0..8, channel block 0..7) order; per step and pixel tile Ah*Bh into acc, then Ah*Bl, then Al*Bh into accx:
//     every accumulator sees the same operands in the same order;
//   * the weight fragments go straight from the pack into two alternating register sets, one step ahead;
//   * the per-element expression (optional ReLU, * 64, range test, clamp, hi = fp16(c), lo = fp16(c - hi)) and the epilogue are
//     copied expression for expression.
// What moved: the border test.  conv3x3_wreg's loader replaces the value of a tap outside the map by zero before the split; here a
// staged row serves three taps of different pixels (the row that is the dx = 0 tap of one pixel is the row-wrap neighbour for
// dx = -1 of the next), so the staged rows are never masked.  Instead each lane selects, once per (pixel tile, tap), the LDS row it
// reads: the real row, or one of the plane's rows of zeros -- the same +0.0 operand bits the loader's select produced.  Staged pixels
// outside [0, M) are read from a clamped address inside the tensor; every reader of such a row is a masked tap.
// The range count is taken while the centre row (dy = 0) is staged, for the workgroup's own pixels only: each element once.
//
// LDS image (dynamic, kRowsLdsBytes): [channel block 0..7][plane hi, lo][row 0..133][32] fp16, 64-byte rows.  Rows 0..129 are the
// staged pixels, rows 130..133 are zeros (written once at the start): 256 B, so that a masked lane can read its zeros from the
// 16-byte slot of the bank row that its real row lies in.  With ONE zero row the masked lanes met the real rows of their lane group
// on the same banks (measured: SQ_LDS_BANK_CONFLICT 4 % of the LDS cycles at 1/4 resolution, 14 % at 1/16, where more pixels lie
// on a border).  8 x 2 x 134 x 64 B = 137216 B.
// Swizzle: the 16-byte chunk index is XORed with 2 * (bit 2 of the row).  A ds_read_b128 is served in four groups of 16 lanes, each
// of which holds, for every row residue mod 4, the rows R, R+12 at chunk c and R+4, R+8 at chunk c^1 (c = 0 or 2): with this
// swizzle the four land in four different 16-byte slots of the 256-byte bank row for any R, i.e. for all three row shifts.  The
// staging writes (ds_write_b64: groups of 16 lanes = 2 consecutive rows x 64 B) are conflict-free as well.
//
// Only Cin = 256 fits with the K order kept (Cin = 512 would need 266 KB); other shapes stay on conv3x3.hip's kernels.
// Measured: profiles/r20_a_conv3x3_rows.md.
#include <mutex>

#include "common.h"

namespace rmnet {
namespace {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kCout = 256;       // output channels (fixed)
constexpr int kCin = 256;        // input channels (fixed: the row image is sized for it)
constexpr int kMT = 128;         // pixels per workgroup
constexpr int kKT = 32;          // K per step (one tap x 32 input channels)
constexpr int kCB = kCin / kKT;  // channel blocks
constexpr int kThreads = 512;
constexpr float kActScale = 64.0f;                 // 2^6
constexpr float kActUnscale = 1.0f / 64.0f;
constexpr float kF16Max = 65504.0f;
constexpr int kWPlane = kCout * kKT;               // halves per weight plane of the pack
constexpr int kStaged = kMT + 2;                   // staged pixel rows of a tap row
constexpr int kZeroRows = 4;                       // rows of zeros behind them: 256 B, one 16-byte slot for every slot of a bank row
constexpr int kPlaneHalves = (kStaged + kZeroRows) * kKT;   // one plane of one channel block
constexpr int kBlockHalves = 2 * kPlaneHalves;     // hi + lo
constexpr int kRowsLdsBytes = kCB * kBlockHalves * 2;
static_assert(kRowsLdsBytes == 137216, "8 blocks x 2 planes x 134 rows x 64 B");
static_assert(kRowsLdsBytes <= kLdsBytesPerCU, "LDS budget");
constexpr int kAhead = 1;                          // pixel tiles that the fragment reads run ahead of their MFMAs (2 and 3: the same time)
constexpr int kStageBatch = 8;                     // staging loads in flight per thread before the first split (16: the same time)
constexpr int kStagePasses = kMT / 8;              // full staging passes: 8 rows x 256 channels per pass and workgroup

// halves from the start of a plane to 16-byte chunk `chunk` of row `row`
__device__ inline int swzr(int row, int chunk) { return row * kKT + ((chunk ^ ((row >> 1) & 2)) << 3); }

template <bool B>
struct Flag {
  static constexpr bool value = B;
};

struct RowsArgs {
  const float* x;          // [M][256]
  const half8* wp;         // [72][2][256][32] fp16
  const float* w_unscale;  // [256]
  const float* bias;       // [256] or null
  const float* res;        // [M][256] or null
  float* out;              // [M][256]
  int* range;              // or null
  int M, H, W, relu_in, relu_out;
};

extern __shared__ __attribute__((aligned(16))) _Float16 rows_lds[];      // kRowsLdsBytes, sized at launch

__global__ __launch_bounds__(kThreads) void conv3x3_rows(RowsArgs a) {
  _Float16* const lds = rows_lds;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, fc = lane >> 4;
  const int m0 = blockIdx.x * kMT;
  const int HW = a.H * a.W;

  // the zero rows: 16 planes x 256 B, 16 bytes per thread
  if (tid < 16 * 2 * kCB) *reinterpret_cast<half8*>(lds + (tid >> 4) * kPlaneHalves + kStaged * kKT + 8 * (tid & 15)) = half8{0, 0, 0, 0, 0, 0, 0, 0};

  // the border test, once per pixel: bit t of pixel tile i's 9 bits = tap t of pixel m0 + 16i + fr lies inside the map (past M: none
  // does) -- conv3x3_wreg's mask, for the pixels whose fragments this lane reads; three tiles per register
  unsigned inside[3] = {0u, 0u, 0u};
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int m = m0 + 16 * i + fr;
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

  // staging items: thread -> (row 2 * (tid / 128) + (tid / 8) % 2 of each pass of 8 rows, channel block (tid / 16) % 8, channels
  // 4 * (tid % 8) .. of it): 8 lanes read 128 contiguous bytes, 16 lanes write two consecutive 64-byte LDS rows
  const int srow = 2 * (tid >> 7) + ((tid >> 3) & 1);
  const int sj = tid & 7;
  const unsigned scol = ((tid >> 4) & 7) * kKT + 4 * sj;
  _Float16* const sdst = lds + ((tid >> 4) & 7) * kBlockHalves + swzr(srow, sj >> 1) + 4 * (sj & 1);   // + 8 rows per pass: the swizzle bit stays
  int bad = 0;
  // RELU: a.relu_in; CENTRE: the tap row is dy = 0 (the one that counts) -- both uniform over a tap row
  auto split_store = [&](auto relu, auto centre, const f32x4 x4, int row, int qb) __attribute__((always_inline)) {
    const int own = row >= 1 && row <= kMT && qb + row < a.M ? 1 : 0;      // (centre row: staged row r is pixel m0 - 1 + r)
    half4 hi, lo;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float v = x4[e];
      if constexpr (decltype(relu)::value) v = v < 0.0f ? 0.0f : v;          // (keeps NaN: it is counted below)
      const float y = v * kActScale;
      if constexpr (decltype(centre)::value) bad += !(fabsf(y) <= kF16Max) ? own : 0;
      const float c = fminf(fmaxf(y, -kF16Max), kF16Max);   // NaN -> -65504 (saturated, counted)
      const _Float16 h = (_Float16)c;
      hi[e] = h;
      lo[e] = (_Float16)(c - (float)h);
    }
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

  // weight fragments [2 * channel tile + plane]: conv3x3_wreg's (16-byte chunk plane*1024 + co*4 + fc of the step's 2048,
  // co = 32*wave + 16*j + fr); the pack is walked step by step, and the last step loads its own fragments again
  half8 wa[4], wb[4];
  const half8* wsrc = a.wp;                                  // the pack of the step that is loaded next (uniform)
  const half8* const wlast = a.wp + (9 * kCB - 1) * (2 * kWPlane / 8);
  const unsigned wl = (wave * 32 + fr) * 4 + fc;
  auto load_w = [&](half8(&w)[4]) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int p = 0; p < 2; ++p) w[2 * j + p] = wsrc[wl + (unsigned)(p * (kWPlane / 8) + j * 64)];
    wsrc = wsrc == wlast ? wsrc : wsrc + 2 * kWPlane / 8;
  };

  // acc[pixel tile][channel tile]: hi*hi, and the two cross terms, as in conv3x3.hip
  f32x4 acc[8][2], accx[8][2];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = accx[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // One tap = 8 steps from the staged row image, free-running.  Per pixel tile the lane's read address is chosen once per tap:
  // row 16i + fr + dx + 1 (swizzled), or the zero row when the tap of that pixel is outside the map.  The channel block and the
  // plane are constant offsets.  Fragments are read one tile ahead of their six MFMAs, across the step boundaries too.
  auto run_tap = [&](int tap) __attribute__((always_inline)) {
    const int dx1 = tap % 3;                                 // dx + 1
    unsigned ao[8];                                          // halves
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const bool in = (inside[i / 3] >> (9 * (i % 3) + tap)) & 1;
      const int row = 16 * i + fr + dx1;
      const unsigned real = (unsigned)swzr(row, fc);
      // the zero row that lies in the same 16-byte slot of the 256-byte bank row as the real one (130 + (row + 2) % 4 = row mod 4):
      // a masked lane then conflicts with no lane of its group, whatever the other lanes read
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
  };

  load_w(wa);
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
    for (int tx = 0; tx < 3; ++tx) run_tap(3 * ty + tx);
  }

  // epilogue: conv3x3_wreg's, expression for expression (pixel m0 + 16i + fr, channels 32*wave + 16j + 4*fc ..).  All residual
  // reads come before the first store: out may BE res
  int me = m0;                                               // (opaque: the pixel indices are formed again here; taken from the
  asm volatile("" : "+s"(me));                               // mask computation they stay live across the K loop and spill)
  f32x4 r[8][2];
  if (a.res) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int m = me + i * 16 + fr;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int co = wave * 32 + j * 16 + 4 * fc;
        r[i][j] = m < a.M ? *reinterpret_cast<const f32x4*>(a.res + (size_t)m * kCout + co) : f32x4{0.f, 0.f, 0.f, 0.f};
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int co = wave * 32 + j * 16 + 4 * fc;
    const f32x4 us = *reinterpret_cast<const f32x4*>(a.w_unscale + co) * kActUnscale;
    const f32x4 b = a.bias ? *reinterpret_cast<const f32x4*>(a.bias + co) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i][j] = (acc[i][j] + accx[i][j]) * us + b;
  }
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int i = 0; i < 8; ++i) asm volatile("" : "+v"(acc[i][j]));
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int co = wave * 32 + j * 16 + 4 * fc;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int m = me + i * 16 + fr;
      if (m >= a.M) continue;
      const size_t off = (size_t)m * kCout + co;
      f32x4 v = acc[i][j];
      if (a.res) v += r[i][j];
      if (a.relu_out) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = v[e] < 0.0f ? 0.0f : v[e];
      }
      *reinterpret_cast<f32x4*>(a.out + off) = v;
    }
  }
  if (a.range && bad) atomicAdd(a.range, bad);
}

// A dynamic LDS request above 64 KB needs the function attribute; it is set once per device, at the first launch on it, and never
// while the stream is capturing (a first launch inside a capture is refused: run the convolution once eagerly before capturing).
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
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(conv3x3_rows), hipFuncAttributeMaxDynamicSharedMemorySize, kRowsLdsBytes) !=
      hipSuccess)
    return RMNET_E_LAUNCH;
  done[dev] = true;
  return RMNET_OK;
}

}  // namespace
}  // namespace rmnet

extern "C" int rmnet_conv3x3_rows_f32(const float* x, const void* wpack, const float* w_unscale, const float* bias, const float* res,
                                      int flags, int N, int H, int W, int Cin, float* out, int32_t* range_word, void* stream) {
  using namespace rmnet;
  // rmnet_conv3x3_split_f32's rules (conv3x3.hip: conv3x3_launch), then Cin
  if (!x || !wpack || !w_unscale || !out || N <= 0 || H <= 0 || W <= 0 || Cin <= 0) return RMNET_E_INVALID_ARG;
  if (flags & ~(RMNET_CONV_RELU_IN | RMNET_CONV_RELU_OUT)) return RMNET_E_INVALID_ARG;
  if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(wpack) | reinterpret_cast<uintptr_t>(w_unscale) |
       reinterpret_cast<uintptr_t>(bias) | reinterpret_cast<uintptr_t>(res) | reinterpret_cast<uintptr_t>(out)) & 15)
    return RMNET_E_INVALID_ARG;
  if (Cin % kKT) return RMNET_E_UNSUPPORTED;
  const long long M = (long long)N * H * W;
  if (M * (long long)(Cin > kCout ? Cin : kCout) >= (1LL << 31)) return RMNET_E_UNSUPPORTED;   // (int pixel index, size_t offsets)
  const char* xb = reinterpret_cast<const char*>(x);
  const char* ob = reinterpret_cast<const char*>(out);
  if (ob < xb + M * Cin * sizeof(float) && xb < ob + M * kCout * sizeof(float)) return RMNET_E_INVALID_ARG;
  if (Cin != kCin) return RMNET_E_UNSUPPORTED;              // the row image holds exactly 256 channels
  const int rc = rows_prepare((hipStream_t)stream);
  if (rc != RMNET_OK) return rc;
  RowsArgs a;
  a.x = x; a.wp = reinterpret_cast<const half8*>(wpack); a.w_unscale = w_unscale; a.bias = bias; a.res = res; a.out = out;
  a.range = range_word; a.M = (int)M; a.H = H; a.W = W;
  a.relu_in = (flags & RMNET_CONV_RELU_IN) != 0;
  a.relu_out = (flags & RMNET_CONV_RELU_OUT) != 0;
  hipLaunchKernelGGL(conv3x3_rows, dim3((unsigned)((M + kMT - 1) / kMT)), dim3(kThreads), kRowsLdsBytes, (hipStream_t)stream, a);
  return check_launch();
}
