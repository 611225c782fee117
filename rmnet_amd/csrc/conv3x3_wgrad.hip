// conv3x3_wgrad.hip -- the weight and bias gradient of the decoder's 3x3 / stride 1 / pad 1 convolutions with 256 outputs, and the
// stage pass that puts an incoming gradient into the fp16 window (include/rmnet_hip.h: rmnet_conv3x3_wgrad_f32,
// rmnet_conv_grad_stage_f32).
//
//   dW[co][ky][kx][ci] = sum over the pixels p = (n, y, x) of  g[p][co] * pre(x)[n, y + ky - 1, x + kx - 1][ci]   (zero outside the map)
//   db[co]             = sum over the pixels of g[p][co]                                 both divided by the staging scale of g
//
// A GEMM with M = 256 (co), N = 9 Cin (tap, ci) and the pixel as reduction index, in the project's three-term split-fp16 arithmetic:
// both operands are scaled by 2^6, clamped to fp16's window and split into hi = fp16(c), lo = fp16(c - hi); hi.hi goes to one fp32
// accumulator, hi.lo + lo.hi to a second (v_mfma_f32_16x16x32_f16), the two are added once at the end.
//
// Work.  A workgroup (512 threads, 8 waves) owns all 256 co x 9 taps x kCT = 16 input channels for one RANGE of pixels (plan below)
// and writes that partial dW to the workspace; wave v owns co 32 v .. 32 v + 31: 2 x 9 tiles of 16 x 16, twice (144 accumulator
// registers).  wgrad_bias sums g over the eighths of the same ranges, one thread per co, and wgrad_merge adds the partials of an
// element in range (and eighth) order, undoes the scales (all powers of two) and writes dW / db: no atomics, every element written once, the same bits every call.
//
// LDS (dynamic only).  The reduction index is the strided index of both channels-last operands, so both tiles are kept as
// [pixel][channel] images and read with ds_read_b64_tr_b16: a 16-lane group g reads the 4 pixels x 16 channels blocks of the pixels
// 8 g + 4 r + q (r = 0, 1 the two reads of a half8, q = 0..3 the element) -- the same pixel order for both operands, which is all a
// product needs.  Lane 4 q + p of a group supplies the address of pixel q, channels 4 p .. 4 p + 3 (8-byte aligned); no lane is ever
// masked: pixels past the range read the zero row.
//   g:  two buffers of [hi, lo][32 pixels][256 + 16 co]: a pixel row is 544 B, so the 8 rows a 32-lane half reads start 8 banks apart
//       ((a / 4) % 64): 8 rows x 8 banks, conflict-free.  69632 B.
//   x:  ONE image per sub-range of up to kSub = 512 pixels, [hi | lo][rows][16 ci], rows = the sub-range's pixels in linear NHW order
//       with W + 1 more on either side, + one row of zeros.  A tap is a constant row offset dy W + dx; a pixel whose tap leaves the map
//       (the neighbours in linear order are then another row's or another image's pixels) is pointed at the zero row instead.  A row
//       is 32 B: the 8 rows of a half are 256 B = all 64 banks, conflict-free when consecutive (taps at a border repeat the zero row,
//       one address).  x is loaded once per workgroup and sub-range, not once per tap.
#include <mutex>

#include "split_f16.h"

namespace rmnet {
namespace {

constexpr int kWgCout = 256;
constexpr int kCT = 16;            // input channels per workgroup
constexpr int kSub = 512;          // pixels per x image
constexpr int kMaxW = 448;         // (kSub + 2 (W + 1) + 1 rows of 64 B next to the g buffers must fit 160 KB: 159936 B)
constexpr int kRangeMin = 256;     // fewest pixels worth a range of their own
constexpr int kMaxRanges = 64;
constexpr int kTargetWGs = 768;    // workgroups to aim for (256 CUs, one workgroup each, three rounds)
constexpr int kBiasSplit = 8;      // wgrad_bias cuts a range into that many chunks (RL is a multiple of 32)
constexpr int kGRow = kWgCout + 16;            // halves per pixel row of a g plane
constexpr int kGPlane = kKT * kGRow;           // halves
constexpr int kGBytes = 2 * 2 * kGPlane * 2;   // two buffers of hi + lo

struct WgradPlan {
  int nct, nranges, RL;
};
// The ranges: as many as fill the GPU with the Cin / 16 channel tiles, none shorter than kRangeMin, at most kMaxRanges; RL pixels each
// (a multiple of the K step), the last one shorter.
inline WgradPlan wgrad_plan(long long P, int Cin) {
  WgradPlan p;
  p.nct = Cin / kCT;
  long long nr = kTargetWGs / p.nct;
  const long long by_len = (P + kRangeMin - 1) / kRangeMin;
  if (nr > by_len) nr = by_len;
  if (nr > kMaxRanges) nr = kMaxRanges;
  if (nr < 1) nr = 1;
  p.RL = (int)((((P + nr - 1) / nr) + kKT - 1) / kKT * kKT);
  p.nranges = (int)((P + p.RL - 1) / p.RL);
  return p;
}
inline int x_rows(int W) { return kSub + 2 * (W + 1) + 1; }
inline size_t wgrad_lds_bytes(int W) { return (size_t)kGBytes + (size_t)x_rows(W) * kCT * 2 * 2; }

struct WgradArgs {
  const float* x;   // [P][Cin]
  const float* g;   // [P][256], staged
  float* part;      // [nranges][256][9][Cin]
  int* range;       // or null
  int P, H, W, Cin, relu_in, RL;
};

typedef __fp16 tr_half4 __attribute__((__vector_size__(4 * sizeof(__fp16))));   // the builtin's own vector type
typedef __attribute__((address_space(3))) tr_half4 lds_tr_half4;

// Two transposed reads = the half8 operand of one lane: elements 0..3 from the block at off0, 4..7 from the block at off1 (halves).
__device__ __forceinline__ half8 tr_read2(const _Float16* base, int off0, int off1) {
  const half4 a = __builtin_bit_cast(half4, __builtin_amdgcn_ds_read_tr16_b64_v4f16((lds_tr_half4*)(base + off0)));
  const half4 b = __builtin_bit_cast(half4, __builtin_amdgcn_ds_read_tr16_b64_v4f16((lds_tr_half4*)(base + off1)));
  return half8{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
}

extern __shared__ __attribute__((aligned(16))) _Float16 wgrad_lds[];   // wgrad_lds_bytes(W), sized at launch

__global__ __launch_bounds__(kThreads) void conv3x3_wgrad(const WgradArgs a) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ct = blockIdx.x, rg = blockIdx.y;
  const int p_begin = rg * a.RL;
  const int p_end = p_begin + a.RL < a.P ? p_begin + a.RL : a.P;
  const int halo = a.W + 1;
  const int xrows = kSub + 2 * halo + 1;
  const int zero_row = xrows - 1;
  _Float16* const gbuf = wgrad_lds;
  _Float16* const xh = wgrad_lds + 2 * 2 * kGPlane;
  _Float16* const xl = xh + xrows * kCT;

  f32x4 acc[2][9], accx[2][9];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int t = 0; t < 9; ++t) acc[j][t] = accx[j][t] = f32x4{0.f, 0.f, 0.f, 0.f};

  // the g loader: pixel tid / 16 of the step's 32, channels 4 (tid % 16) + 64 i
  const int gp = tid >> 4, gc = 4 * (tid & 15);
  f32x4 gr[4];
  int bad = 0;
  // the operand reads: group, the lane's pixel q and channel chunk p inside a block
  const int grp = lane >> 4, q = (lane >> 2) & 3, cp = lane & 3;
  const int a_off = (8 * grp + q) * kGRow + 32 * wave + 4 * cp;     // halves; + 4 r kGRow, + 16 j

  for (int s0 = p_begin; s0 < p_end; s0 += kSub) {
    const int s1 = s0 + kSub < p_end ? s0 + kSub : p_end;
    __syncthreads();   // the last sub-range's reads of the x image are over
    // ---- the x image: rows 0 .. s1 - s0 + 2 halo - 1 = pixels s0 - halo .., then zeros up to and including the zero row
    {
      const int nrows = s1 - s0 + 2 * halo;
      const int c4 = tid & 3;
      for (int r = tid >> 2; r < xrows; r += kThreads / 4) {
        const int pix = s0 - halo + r;
        half4 hi = half4{0, 0, 0, 0}, lo = half4{0, 0, 0, 0};
        if (r < nrows && pix >= 0 && pix < a.P) {
          f32x4 v = *reinterpret_cast<const f32x4*>(a.x + (size_t)pix * a.Cin + ct * kCT + 4 * c4);
          if (a.relu_in) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = v[e] < 0.0f ? 0.0f : v[e];   // (keeps NaN: it is counted)
          }
          split4(v, hi, lo, bad, pix >= s0 && pix < s1 ? 1 : 0);             // counted once: by the sub-range that owns the pixel
        }
        *reinterpret_cast<half4*>(xh + r * kCT + 4 * c4) = hi;
        *reinterpret_cast<half4*>(xl + r * kCT + 4 * c4) = lo;
      }
    }
    // ---- the K loop: 32 pixels a step, g double-buffered
    auto load_g = [&](int k0) __attribute__((always_inline)) {
      const int pix = k0 + gp;
#pragma unroll
      for (int i = 0; i < 4; ++i)
        gr[i] = pix < s1 ? *reinterpret_cast<const f32x4*>(a.g + (size_t)pix * kWgCout + gc + 64 * i) : f32x4{0.f, 0.f, 0.f, 0.f};
    };
    load_g(s0);
    int cur = 0;
    for (int k0 = s0; k0 < s1; k0 += kKT, cur ^= 1) {
      _Float16* const gh = gbuf + cur * 2 * kGPlane;
      _Float16* const gl = gh + kGPlane;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        half4 hi, lo;
        split4(gr[i], hi, lo, bad, ct == 0 ? 1 : 0);                       // (every channel tile reads g: the first one counts)
        *reinterpret_cast<half4*>(gh + gp * kGRow + gc + 64 * i) = hi;
        *reinterpret_cast<half4*>(gl + gp * kGRow + gc + 64 * i) = lo;
      }
      __syncthreads();
      if (k0 + kKT < s1) load_g(k0 + kKT);
      // the lane's two pixels and their x rows, tap by tap
      int xrow[2];
      unsigned inside[2];
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const int pk = k0 + 8 * grp + 4 * r + q;
        inside[r] = taps_inside(pk, s1, a.H, a.W);
        xrow[r] = pk - s0 + halo;
      }
      half8 ah[2], al[2];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        ah[j] = tr_read2(gh, a_off + 16 * j, a_off + 16 * j + 4 * kGRow);
        al[j] = tr_read2(gl, a_off + 16 * j, a_off + 16 * j + 4 * kGRow);
      }
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        const int d = (t / 3 - 1) * a.W + (t % 3 - 1);
        const int o0 = (((inside[0] >> t) & 1) ? xrow[0] + d : zero_row) * kCT + 4 * cp;
        const int o1 = (((inside[1] >> t) & 1) ? xrow[1] + d : zero_row) * kCT + 4 * cp;
        const half8 bh = tr_read2(xh, o0, o1);
        const half8 bl = tr_read2(xl, o0, o1);
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[j][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[j], bh, acc[j][t], 0, 0, 0);
#pragma unroll
        for (int j = 0; j < 2; ++j) accx[j][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[j], bl, accx[j][t], 0, 0, 0);
#pragma unroll
        for (int j = 0; j < 2; ++j) accx[j][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[j], bh, accx[j][t], 0, 0, 0);
      }
    }
  }
  // ---- the partial: D[co][ci], lane = (co / 4 % 4, ci), element = co % 4
  float* const part = a.part + (size_t)rg * kWgCout * 9 * a.Cin;
  const int ci = ct * kCT + (lane & 15);
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int co = 32 * wave + 16 * j + 4 * grp + e;
        part[((size_t)co * 9 + t) * a.Cin + ci] = acc[j][t][e] + accx[j][t][e];
      }
  if (a.range) {
    bad = wave_sum(bad);
    if (lane == 0 && bad) atomicAdd(a.range, bad);
  }
}

// The sum of g over one eighth of a range (chunk blockIdx.y of range blockIdx.x; RL / 8 pixels), one thread per output channel,
// pixel by pixel: a workgroup reads whole 1 KB rows, the loads of a thread do not depend on each other, only its additions do.
// (One chunk per range took longer than the weight gradient itself: 48 workgroups of 3616 dependent steps at the training shape.)
__global__ __launch_bounds__(kWgCout) void wgrad_bias(const float* g, float* part_b, int P, int RL) {
  const int rg = blockIdx.x, ch = blockIdx.y, co = threadIdx.x;
  const int CL = RL / kBiasSplit;
  const int p_begin = rg * RL + ch * CL;
  const int p_end = p_begin + CL < P ? p_begin + CL : P;
  float s = 0.0f;
#pragma unroll 8
  for (int p = p_begin; p < p_end; ++p) s += g[(size_t)p * kWgCout + co];
  part_b[(rg * kBiasSplit + ch) * kWgCout + co] = s;
}

// dW / db = the partials added in range order, times 2^-12 (dW: the two operand scales) and the inverse of the staging scale's two
// factors: all exact.
__global__ __launch_bounds__(256) void wgrad_merge(const float* part, const float* part_b, const float* g_scale, float* dw, float* db,
                                                   int nranges, int n_dw) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  const float ia = 1.0f / g_scale[0], ib = 1.0f / g_scale[1];
  if (idx < n_dw) {
    float s = part[idx];
    for (int r = 1; r < nranges; ++r) s += part[(size_t)r * n_dw + idx];
    dw[idx] = s * (kActUnscale * kActUnscale) * ia * ib;
  } else if (db && idx < n_dw + kWgCout) {
    const int co = idx - n_dw;
    float s = part_b[co];
    for (int r = 1; r < nranges * kBiasSplit; ++r) s += part_b[r * kWgCout + co];
    db[co] = s * ia * ib;
  }
}

// The stage pass: gs = [act > 0] g 2^s with 2^s amax in [2^8, 2^9) (s = 0 for amax = 0, NaN or Inf), 2^s as the product of the two
// floats written to g_scale (the second is 1 unless amax < 2^-118, where 2^s alone is no fp32 number).
__global__ __launch_bounds__(256) void conv_grad_stage(const float* g, const float* act, const float* amax, float* gs, float* g_scale,
                                                       long long n4) {
  const float am = *amax;
  int s = 0;
  if (am > 0.0f && am <= 3.4028234663852886e38f) {
    int ex;
    frexpf(am, &ex);
    s = 9 - ex;
  }
  const int s1 = s > 126 ? 126 : s;
  const float fa = ldexpf(1.0f, s1), fb = ldexpf(1.0f, s - s1);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    g_scale[0] = fa;
    g_scale[1] = fb;
  }
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
    f32x4 v = reinterpret_cast<const f32x4*>(g)[i];
    if (act) {
      const f32x4 o = reinterpret_cast<const f32x4*>(act)[i];
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = o[e] > 0.0f ? v[e] : 0.0f;
    }
    reinterpret_cast<f32x4*>(gs)[i] = v * fa * fb;
  }
}

int wgrad_prepare(hipStream_t st) {
  static std::mutex mu;
  static bool done[64] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return RMNET_E_LAUNCH;
  std::lock_guard<std::mutex> lock(mu);
  if (done[dev]) return RMNET_OK;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(st, &cs) != hipSuccess) return RMNET_E_LAUNCH;
  if (cs != hipStreamCaptureStatusNone) return RMNET_E_UNSUPPORTED;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(conv3x3_wgrad), hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)wgrad_lds_bytes(kMaxW)) != hipSuccess)
    return RMNET_E_LAUNCH;
  done[dev] = true;
  return RMNET_OK;
}

inline size_t wgrad_ws_bytes(long long P, int Cin) {
  const WgradPlan p = wgrad_plan(P, Cin);
  return (size_t)p.nranges * ((size_t)kWgCout * 9 * Cin + kBiasSplit * kWgCout) * sizeof(float);
}

inline bool wgrad_shape_ok(int N, int H, int W, int Cin) { return N > 0 && H > 0 && W > 0 && Cin > 0; }
inline bool wgrad_supported(int N, int H, int W, int Cin) {
  const long long P = (long long)N * H * W;
  return Cin % kKT == 0 && W <= kMaxW && P * (long long)(Cin > kWgCout ? Cin : kWgCout) < (1LL << 31) && 9LL * Cin * kWgCout < (1LL << 31);
}

}  // namespace
}  // namespace rmnet

using namespace rmnet;

extern "C" size_t rmnet_conv3x3_wgrad_workspace_bytes(int N, int H, int W, int Cin) {
  if (!wgrad_shape_ok(N, H, W, Cin) || !wgrad_supported(N, H, W, Cin)) return 0;
  return wgrad_ws_bytes((long long)N * H * W, Cin);
}

extern "C" int rmnet_conv3x3_wgrad_f32(const float* x, const float* g, const float* g_scale, int flags, int N, int H, int W, int Cin,
                                       float* dw, float* db, void* workspace, size_t workspace_bytes, int32_t* range_word, void* stream) {
  if (!x || !g || !g_scale || !dw || !wgrad_shape_ok(N, H, W, Cin)) return RMNET_E_INVALID_ARG;
  if (flags & ~RMNET_CONV_RELU_IN) return RMNET_E_INVALID_ARG;
  if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(g_scale) |
       reinterpret_cast<uintptr_t>(dw) | reinterpret_cast<uintptr_t>(db) | reinterpret_cast<uintptr_t>(workspace)) & 15)
    return RMNET_E_INVALID_ARG;
  if (reinterpret_cast<uintptr_t>(range_word) & 3) return RMNET_E_INVALID_ARG;
  if (!wgrad_supported(N, H, W, Cin)) return RMNET_E_UNSUPPORTED;
  const long long P = (long long)N * H * W;
  const long long n_dw = 9LL * Cin * kWgCout;
  // the outputs are written while other workgroups may still read x and g
  if (overlap(dw, n_dw * 4, x, P * Cin * 4) || overlap(dw, n_dw * 4, g, P * kWgCout * 4)) return RMNET_E_INVALID_ARG;
  if (db && (overlap(db, kWgCout * 4, x, P * Cin * 4) || overlap(db, kWgCout * 4, g, P * kWgCout * 4) || overlap(db, kWgCout * 4, dw, n_dw * 4)))
    return RMNET_E_INVALID_ARG;
  const size_t need = wgrad_ws_bytes(P, Cin);
  if (!workspace || workspace_bytes < need) return RMNET_E_WORKSPACE;
  if (overlap(workspace, (long long)need, x, P * Cin * 4) || overlap(workspace, (long long)need, g, P * kWgCout * 4) ||
      overlap(workspace, (long long)need, dw, n_dw * 4) || (db && overlap(workspace, (long long)need, db, kWgCout * 4)))
    return RMNET_E_INVALID_ARG;
  // (the merge reads g_scale while it writes dw and db; every workgroup may add to the range word)
  const void* outs[3] = {dw, db, workspace};
  const long long out_bytes[3] = {n_dw * 4, kWgCout * 4, (long long)need};
  for (int i = 0; i < 3; ++i) {
    if (!outs[i]) continue;
    if (overlap(outs[i], out_bytes[i], g_scale, 8) || (range_word && overlap(outs[i], out_bytes[i], range_word, 4))) return RMNET_E_INVALID_ARG;
  }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int rc = wgrad_prepare(st);
  if (rc != RMNET_OK) return rc;
  const WgradPlan p = wgrad_plan(P, Cin);
  float* part = reinterpret_cast<float*>(workspace);
  float* part_b = part + (size_t)p.nranges * n_dw;
  WgradArgs a;
  a.x = x; a.g = g; a.part = part; a.range = range_word;
  a.P = (int)P; a.H = H; a.W = W; a.Cin = Cin; a.relu_in = (flags & RMNET_CONV_RELU_IN) != 0; a.RL = p.RL;
  hipLaunchKernelGGL(conv3x3_wgrad, dim3(p.nct, p.nranges), dim3(kThreads), wgrad_lds_bytes(W), st, a);
  if (db) hipLaunchKernelGGL(wgrad_bias, dim3(p.nranges, kBiasSplit), dim3(kWgCout), 0, st, g, part_b, (int)P, p.RL);
  const long long n_out = n_dw + (db ? kWgCout : 0);
  hipLaunchKernelGGL(wgrad_merge, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, st, part, part_b, g_scale, dw, db, p.nranges, (int)n_dw);
  return check_launch();
}

extern "C" int rmnet_conv_grad_stage_f32(const float* g, const float* act, const float* amax, long long n, float* gs, float* g_scale,
                                         void* stream) {
  if (!g || !amax || !gs || !g_scale || n <= 0 || n % 4) return RMNET_E_INVALID_ARG;
  if ((reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(act) | reinterpret_cast<uintptr_t>(gs) |
       reinterpret_cast<uintptr_t>(g_scale)) & 15)
    return RMNET_E_INVALID_ARG;
  if (reinterpret_cast<uintptr_t>(amax) & 3) return RMNET_E_INVALID_ARG;
  if (n >= (1LL << 31)) return RMNET_E_UNSUPPORTED;
  // gs may be g itself (an element is read, then written, by one thread); it must not overlap act partially or the scalars
  if (overlap(gs, n * 4, amax, 4) || overlap(gs, n * 4, g_scale, 8) || overlap(g_scale, 8, amax, 4)) return RMNET_E_INVALID_ARG;
  if (gs != g && overlap(gs, n * 4, g, n * 4)) return RMNET_E_INVALID_ARG;
  if (act && overlap(gs, n * 4, act, n * 4)) return RMNET_E_INVALID_ARG;
  const long long n4 = n / 4;
  long long blocks = (n4 + 255) / 256;
  if (blocks > 8 * kNumCUs) blocks = 8 * kNumCUs;
  hipLaunchKernelGGL(conv_grad_stage, dim3((unsigned)blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), g, act, amax, gs,
                     g_scale, n4);
  return check_launch();
}
