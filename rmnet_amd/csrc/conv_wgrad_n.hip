// conv_wgrad_n.hip -- the weight and bias gradient of a 3x3 / stride 1 / pad 1 convolution with any multiple of 128 output channels
// (the key / value heads: 128 and 512), and the stage pass for the gradients the memory read hands back (include/rmnet_hip.h:
// rmnet_conv3x3_wgrad_n_f32, rmnet_conv_grad_stage_rect_f32).
//
// The weight gradient is the GEMM of conv3x3_wgrad.hip, body for body (conv3x3_wgrad_parts.h): the same three-term split-fp16
// arithmetic, the same [pixel][channel] LDS images, the same order of additions.  What is new is the walk over the output channels:
// a gradient row holds Cout floats, blockIdx.z picks a tile of up to 256 of them, and the last tile of a Cout that is no multiple
// of 256 holds 128: it runs as a 256-wide workgroup whose upper four waves load and reach every barrier but issue no MFMA (their
// halves of the g planes are zeros nobody reads).  The ranges are planned for Cin / 16 * ceil(Cout / 256) workgroups each, so that
// Cout = 256 gets the plan, the partials and the bits of rmnet_conv3x3_wgrad_f32.  Only the first channel tile of an output-channel
// tile counts g in the range word and only the first output-channel tile counts x: once per element.
//
// The stage pass writes gs[n, y, x, c] = g[n, c, y, x] 2^s inside image n's rectangle and +0.0 outside (a select: what lies outside
// is not looked at, so a NaN there stays there) from a channels-last tensor (elementwise, 16 bytes a thread) or from planes
// (element (n, c, y, x) at n sn + c sc + y W + x: an NCHW tensor, a [:, :, t] slice).  The planes are transposed through an LDS tile
// of 32 channels x 64 pixels: a wave reads 64 consecutive pixels of one plane (256 B) and a thread writes four channels of one
// pixel (16 B, eight threads a 128-B row segment).
#include <mutex>

#include "conv3x3_wgrad_parts.h"

namespace rmnet {
namespace {

extern __shared__ __attribute__((aligned(16))) _Float16 wgrad_n_lds[];   // sized at launch

__global__ __launch_bounds__(kThreads) void conv_wgrad_n(const WgradArgs a, const int cout) {
  const int co0 = blockIdx.z * kWgCout;
  wgrad_tile(a, wgrad_n_lds, cout, co0, cout - co0 < kWgCout ? cout - co0 : kWgCout);
}

// chunk blockIdx.y of range blockIdx.x, output channels 128 blockIdx.z ..
__global__ __launch_bounds__(128) void bias_grad_n(const float* g, float* part_b, int P, int RL, int cout) {
  wgrad_bias_chunk(g, part_b, P, RL, cout, blockIdx.x, blockIdx.y, blockIdx.z * 128 + threadIdx.x);
}

__global__ __launch_bounds__(256) void merge_grad_n(const float* part, const float* part_b, const float* g_scale, float* dw, float* db,
                                                    int nranges, int n_dw, int cout) {
  wgrad_merge_element(part, part_b, g_scale, dw, db, nranges, n_dw, cout, blockIdx.x * 256 + threadIdx.x);
}

struct StageRectArgs {
  const float* g;
  const int32_t* rects;   // [N][4] (cx0, cx1, cy0, cy1), inclusive, or null
  const float* amax;
  float* gs;              // [N][H][W][C]
  float* g_scale;
  long long sn, sc;       // planes: the strides of n and c in floats
  int N, C, H, W;
};

// 2^s as two factors, as conv_grad_stage computes it: 2^s amax in [2^8, 2^9), s = 0 for amax = 0, NaN or Inf.
__device__ __forceinline__ void stage_scale(const float am, float& fa, float& fb) {
  int s = 0;
  if (am > 0.0f && am <= 3.4028234663852886e38f) {
    int ex;
    frexpf(am, &ex);
    s = 9 - ex;
  }
  const int s1 = s > 126 ? 126 : s;
  fa = ldexpf(1.0f, s1);
  fb = ldexpf(1.0f, s - s1);
}

__device__ __forceinline__ bool in_rect(const int32_t* rects, int n, int y, int x) {
  if (!rects) return true;
  const int32_t* r = rects + 4 * n;
  return x >= r[0] && x <= r[1] && y >= r[2] && y <= r[3];
}

constexpr int kStC = 32, kStP = 64, kStRow = kStP + 1;   // the transpose tile: channels, pixels, floats per LDS row

template <bool kPlanes>
__global__ __launch_bounds__(256) void grad_stage_rect(const StageRectArgs a) {
  float fa, fb;
  stage_scale(*a.amax, fa, fb);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    a.g_scale[0] = fa;
    a.g_scale[1] = fb;
  }
  const int HW = a.H * a.W;
  if constexpr (!kPlanes) {
    const int c4n = a.C / 4;
    const long long n4 = (long long)a.N * HW * c4n;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
      const int pix = (int)(i / c4n);
      const int n = pix / HW, r = pix - n * HW;
      const f32x4 v = reinterpret_cast<const f32x4*>(a.g)[i];
      reinterpret_cast<f32x4*>(a.gs)[i] = in_rect(a.rects, n, r / a.W, r % a.W) ? v * fa * fb : f32x4{0.f, 0.f, 0.f, 0.f};
    }
  } else {
    float* const tile = reinterpret_cast<float*>(wgrad_n_lds);   // [kStC][kStRow]
    const int npt = (HW + kStP - 1) / kStP, nctl = (a.C + kStC - 1) / kStC;
    int b = blockIdx.x;
    const int pt = b % npt;
    b /= npt;
    const int ctl = b % nctl, n = b / nctl;
    const int p0 = pt * kStP, c0 = ctl * kStC;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // in: channel c0 + wave + 4 i, pixel p0 + lane.  A pixel outside the rectangle is not read at all.
    const int pi = p0 + lane;
    const bool take = pi < HW && in_rect(a.rects, n, pi / a.W, pi % a.W);
#pragma unroll
    for (int i = 0; i < kStC / 4; ++i) {
      const int c = c0 + wave + 4 * i;
      float v = 0.0f;
      if (take && c < a.C) v = a.g[(long long)n * a.sn + (long long)c * a.sc + pi] * fa * fb;
      tile[(wave + 4 * i) * kStRow + lane] = v;
    }
    __syncthreads();
    // out: pixel p0 + tid / 8 (+ 32), channels c0 + 4 (tid % 8) ..
    const int c4 = 4 * (threadIdx.x & 7);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int pl = (threadIdx.x >> 3) + 32 * h;
      if (p0 + pl < HW && c0 + c4 < a.C) {
        const f32x4 v{tile[(c4 + 0) * kStRow + pl], tile[(c4 + 1) * kStRow + pl], tile[(c4 + 2) * kStRow + pl], tile[(c4 + 3) * kStRow + pl]};
        *reinterpret_cast<f32x4*>(a.gs + ((long long)n * HW + p0 + pl) * a.C + c0 + c4) = v;
      }
    }
  }
}

int wgrad_n_prepare(hipStream_t st) {
  static std::mutex mu;
  static bool done[64] = {};
  std::lock_guard<std::mutex> lock(mu);
  return wgrad_set_lds_attribute(reinterpret_cast<const void*>(conv_wgrad_n), done, st);
}

inline bool wgrad_n_cout_ok(int Cout) { return Cout > 0 && Cout % 128 == 0; }

}  // namespace
}  // namespace rmnet

using namespace rmnet;

extern "C" size_t rmnet_conv3x3_wgrad_n_workspace_bytes(int N, int H, int W, int Cin, int Cout) {
  if (!wgrad_shape_ok(N, H, W, Cin) || !wgrad_n_cout_ok(Cout) || !wgrad_supported(N, H, W, Cin, Cout)) return 0;
  return wgrad_ws_bytes((long long)N * H * W, Cin, Cout);
}

extern "C" int rmnet_conv3x3_wgrad_n_f32(const float* x, const float* g, const float* g_scale, int flags, int N, int H, int W, int Cin,
                                         int Cout, float* dw, float* db, void* workspace, size_t workspace_bytes, int32_t* range_word,
                                         void* stream) {
  if (Cout <= 0) return RMNET_E_INVALID_ARG;
  if (Cout % 128) return RMNET_E_UNSUPPORTED;
  int rc = wgrad_check_args(x, g, g_scale, flags, N, H, W, Cin, Cout, dw, db, workspace, workspace_bytes, range_word);
  if (rc != RMNET_OK) return rc;
  const long long P = (long long)N * H * W;
  const long long n_dw = 9LL * Cin * Cout;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  rc = wgrad_n_prepare(st);
  if (rc != RMNET_OK) return rc;
  const WgradPlan p = wgrad_plan(P, Cin, Cout);
  float* part = reinterpret_cast<float*>(workspace);
  float* part_b = part + (size_t)p.nranges * n_dw;
  WgradArgs a;
  a.x = x; a.g = g; a.part = part; a.range = range_word;
  a.P = (int)P; a.H = H; a.W = W; a.Cin = Cin; a.relu_in = (flags & RMNET_CONV_RELU_IN) != 0; a.RL = p.RL;
  hipLaunchKernelGGL(conv_wgrad_n, dim3(p.nct, p.nranges, p.ncot), dim3(kThreads), wgrad_lds_bytes(W), st, a, Cout);
  if (db) hipLaunchKernelGGL(bias_grad_n, dim3(p.nranges, kBiasSplit, Cout / 128), dim3(128), 0, st, g, part_b, (int)P, p.RL, Cout);
  const long long n_out = n_dw + (db ? Cout : 0);
  hipLaunchKernelGGL(merge_grad_n, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, st, part, part_b, g_scale, dw, db, p.nranges,
                     (int)n_dw, Cout);
  return check_launch();
}

extern "C" int rmnet_conv_grad_stage_rect_f32(const float* g, int layout, long long sn, long long sc, const int32_t* rects,
                                              const float* amax, int N, int C, int H, int W, float* gs, float* g_scale, void* stream) {
  if (!g || !amax || !gs || !g_scale || N <= 0 || C <= 0 || H <= 0 || W <= 0) return RMNET_E_INVALID_ARG;
  if (layout != RMNET_GRAD_LAYOUT_NHWC && layout != RMNET_GRAD_LAYOUT_PLANES) return RMNET_E_INVALID_ARG;
  if ((reinterpret_cast<uintptr_t>(gs) | reinterpret_cast<uintptr_t>(g_scale)) & 15) return RMNET_E_INVALID_ARG;
  if ((reinterpret_cast<uintptr_t>(g) & (layout == RMNET_GRAD_LAYOUT_NHWC ? 15 : 3)) || (reinterpret_cast<uintptr_t>(amax) & 3) ||
      (reinterpret_cast<uintptr_t>(rects) & 3))
    return RMNET_E_INVALID_ARG;
  if (C % 4) return RMNET_E_UNSUPPORTED;
  const long long HW = (long long)H * W, n = (long long)N * C * HW;
  if (n >= (1LL << 31)) return RMNET_E_UNSUPPORTED;
  long long g_floats = n;   // the floats from g to the end of its last element
  if (layout == RMNET_GRAD_LAYOUT_PLANES) {
    // planes must not fold onto each other: a channel's plane inside its stride, an image's channels inside its stride
    if (sc < HW || sn < (C - 1) * sc + HW) return RMNET_E_INVALID_ARG;
    g_floats = (N - 1) * sn + (C - 1) * sc + HW;
    if (g_floats >= (1LL << 31)) return RMNET_E_UNSUPPORTED;
  }
  // gs is written while g, the rectangles and amax are read (the channels-last form MAY be staged in place, as conv_grad_stage)
  if (overlap(gs, n * 4, amax, 4) || overlap(gs, n * 4, g_scale, 8) || overlap(g_scale, 8, amax, 4)) return RMNET_E_INVALID_ARG;
  if (!(layout == RMNET_GRAD_LAYOUT_NHWC && gs == g) && overlap(gs, n * 4, g, g_floats * 4)) return RMNET_E_INVALID_ARG;
  if (overlap(g_scale, 8, g, g_floats * 4)) return RMNET_E_INVALID_ARG;
  if (rects && (overlap(gs, n * 4, rects, 16LL * N) || overlap(g_scale, 8, rects, 16LL * N))) return RMNET_E_INVALID_ARG;
  StageRectArgs a;
  a.g = g; a.rects = rects; a.amax = amax; a.gs = gs; a.g_scale = g_scale; a.sn = sn; a.sc = sc; a.N = N; a.C = C; a.H = H; a.W = W;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (layout == RMNET_GRAD_LAYOUT_NHWC) {
    long long blocks = (n / 4 + 255) / 256;
    if (blocks > 8 * kNumCUs) blocks = 8 * kNumCUs;
    hipLaunchKernelGGL(grad_stage_rect<false>, dim3((unsigned)blocks), dim3(256), 0, st, a);
  } else {
    const long long blocks = (long long)N * ((HW + kStP - 1) / kStP) * ((C + kStC - 1) / kStC);   // (< 2^31: n is)
    hipLaunchKernelGGL(grad_stage_rect<true>, dim3((unsigned)blocks), dim3(256), kStC * kStRow * sizeof(float), st, a);
  }
  return check_launch();
}
