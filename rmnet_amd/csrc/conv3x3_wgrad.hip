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

#include "conv3x3_wgrad_parts.h"

namespace rmnet {
namespace {

extern __shared__ __attribute__((aligned(16))) _Float16 wgrad_lds[];   // wgrad_lds_bytes(W), sized at launch

// (the three bodies: conv3x3_wgrad_parts.h, here for the one tile of 256 output channels)
__global__ __launch_bounds__(kThreads) void conv3x3_wgrad(const WgradArgs a) { wgrad_tile(a, wgrad_lds, kWgCout, 0, kWgCout); }

// The sum of g over one eighth of a range (chunk blockIdx.y of range blockIdx.x; RL / 8 pixels), one thread per output channel.
// (One chunk per range took longer than the weight gradient itself: 48 workgroups of 3616 dependent steps at the training shape.)
__global__ __launch_bounds__(kWgCout) void wgrad_bias(const float* g, float* part_b, int P, int RL) {
  wgrad_bias_chunk(g, part_b, P, RL, kWgCout, blockIdx.x, blockIdx.y, threadIdx.x);
}

__global__ __launch_bounds__(256) void wgrad_merge(const float* part, const float* part_b, const float* g_scale, float* dw, float* db,
                                                   int nranges, int n_dw) {
  wgrad_merge_element(part, part_b, g_scale, dw, db, nranges, n_dw, kWgCout, blockIdx.x * 256 + threadIdx.x);
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
  std::lock_guard<std::mutex> lock(mu);
  return wgrad_set_lds_attribute(reinterpret_cast<const void*>(conv3x3_wgrad), done, st);
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
  int rc = wgrad_check_args(x, g, g_scale, flags, N, H, W, Cin, kWgCout, dw, db, workspace, workspace_bytes, range_word);
  if (rc != RMNET_OK) return rc;
  const long long P = (long long)N * H * W;
  const long long n_dw = 9LL * Cin * kWgCout;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  rc = wgrad_prepare(st);
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
