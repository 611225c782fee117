// flow_head.hip -- TinyFlowNet's 2-channel flow heads and 2 -> 2 flow upsamplers in plain fp32 FMA, reading and writing the
// channels-last concatenation buffers in place.
//
// flow_head: out [N][2][H][W] (NCHW) = conv3x3_p1(x[..., :Cin], w) + bias for x [N][H][W][x_ld].  With two output channels the
// convolution is bound by reading x once, and the small levels (8x14, 16x28) have too few pixels to fill the chip by pixel tiles
// alone, so the grid is (pixel tile) x (channel slice):
//   * a workgroup (256 threads) owns 14 x 14 output pixels of one image and ONE slice of kCS = 32 input channels.  It stages the
//     16 x 16 halo tile of that slice in LDS (zeros outside the map and for the channels >= Cin: the last 16-byte group of a pixel
//     is masked element by element, what the padding channels hold is never used);
//   * each thread is one halo pixel and accumulates its 18 partial sums part[tap][co] = sum_c x[pixel][c] * w[co][c][tap] over the
//     slice's 32 channels in channel order -- the weights are uniform across the wave and come through the scalar cache;
//   * the partials go to LDS and every output pixel adds the nine it needs, taps in the order ky, kx, into the workspace
//     ws [slice][N][2][H][W];
//   * flow_head_sum adds bias + slice 0 + slice 1 + ... in slice order.
// Every sum has a fixed order that depends on Cin alone: no atomics, the same bits from call to call and for any N.
//
// flow_up: ConvTranspose2d(2, 2, 4, stride 2, padding 1) of flow [N][2][h][w] in its four-phase form (8 FMAs per value, in the
// order ci, ty, tx), one thread per output pixel, which writes the channels coff, coff + 1 of out [N][2h][2w][out_ld] and +0.0 into
// coff + 2 .. out_ld - 1 as 16-byte stores.
#include "common.h"

namespace rmnet {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;
constexpr int kHH = 16, kHW = 16;          // halo tile (= threads)
constexpr int kOH = kHH - 2, kOW = kHW - 2;
constexpr int kCS = 32;                    // channels per slice
constexpr int kXStride = kCS + 4;          // padded pixel row: conflict-free 16-byte reads at one pixel per lane
constexpr int kPStride = 19;               // 18 partials per pixel, odd stride
constexpr int kLdsBytes = kThreads * kXStride * 4;
static_assert(kHH * kHW == kThreads, "one thread per halo pixel");
static_assert(kPStride <= kXStride, "the partials reuse the x tile");

extern __shared__ __attribute__((aligned(16))) float lds[];      // x tile [pixel][kXStride], then the partials [pixel][kPStride]

// wpack [ceil32(Cin)][9][2]: w[co][c][ky][kx] at (c * 9 + 3 * ky + kx) * 2 + co, zero for c >= Cin
__global__ __launch_bounds__(kThreads) void flow_head(const float* __restrict__ x, int x_ld, const float* __restrict__ wpack,
                                                      float* __restrict__ ws, int N, int H, int W, int Cin, int TY, int TX, int S) {
  const int tid = threadIdx.x;
  int t = blockIdx.x;
  const int s = t % S;
  t /= S;
  const int n = t / (TY * TX);
  t -= n * (TY * TX);
  const int ty = t / TX, tx = t - ty * TX;
  const int y0 = ty * kOH - 1, x0 = tx * kOW - 1;       // the halo tile's first pixel
  const int c0 = s * kCS;

  // loader items: 8 x (pixel p = tid / 8 + 32 i, channels c0 + 4 * (tid & 7) .. + 3)
  const int q4 = tid & 7;
  const int c = c0 + 4 * q4;                            // c < Cin <= x_ld and x_ld % 4 == 0: the 16 bytes are inside the pixel
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int p = (tid >> 3) + 32 * i;
    const int gy = y0 + p / kHW, gx = x0 + p % kHW;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if ((unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W && c < Cin) {
      v = *reinterpret_cast<const f32x4*>(x + ((n * H + gy) * W + gx) * x_ld + c);      // (N * H * W * x_ld < 2^31)
#pragma unroll
      for (int e = 1; e < 4; ++e) v[e] = c + e < Cin ? v[e] : 0.0f;
    }
    *reinterpret_cast<f32x4*>(lds + p * kXStride + 4 * q4) = v;
  }
  __syncthreads();

  float part[9][2];
#pragma unroll
  for (int k = 0; k < 9; ++k) part[k][0] = part[k][1] = 0.0f;
  const float* wp = wpack + (size_t)c0 * 18;
#pragma unroll 1                   // (72 weights in SGPRs per pass)
  for (int c4 = 0; c4 < kCS / 4; ++c4) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(lds + tid * kXStride + 4 * c4);
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int k = 0; k < 9; ++k) {
        part[k][0] = fmaf(v[e], wp[((4 * c4 + e) * 9 + k) * 2], part[k][0]);
        part[k][1] = fmaf(v[e], wp[((4 * c4 + e) * 9 + k) * 2 + 1], part[k][1]);
      }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    lds[tid * kPStride + 2 * k] = part[k][0];
    lds[tid * kPStride + 2 * k + 1] = part[k][1];
  }
  __syncthreads();

  const int oy = tid / kHW, ox = tid % kHW;
  const int gy = ty * kOH + oy, gx = tx * kOW + ox;
  if (oy >= kOH || ox >= kOW || gy >= H || gx >= W) return;
  float s0 = 0.0f, s1 = 0.0f;
#pragma unroll
  for (int ky = 0; ky < 3; ++ky)
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const float* p = lds + ((oy + ky) * kHW + ox + kx) * kPStride + 2 * (ky * 3 + kx);
      s0 += p[0];
      s1 += p[1];
    }
  const size_t plane = (size_t)H * W;
  float* o = ws + ((size_t)s * N + n) * 2 * plane + (size_t)gy * W + gx;
  o[0] = s0;
  o[plane] = s1;
}

// out[i] = bias[co] + ws[0][i] + ws[1][i] + ..., i over [N][2][H][W]
__global__ __launch_bounds__(256) void flow_head_sum(const float* __restrict__ ws, const float* __restrict__ bias, float* __restrict__ out,
                                                     int plane, int total, int S) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  float v = bias[(i / plane) & 1];
  for (int s = 0; s < S; ++s) v += ws[(size_t)s * total + i];
  out[i] = v;
}

__global__ __launch_bounds__(256) void flow_up(const float* __restrict__ flow, const float* __restrict__ w, float* __restrict__ out,
                                               int h, int wd, int out_ld, int coff, int total) {
  const int i = blockIdx.x * 256 + threadIdx.x;      // output pixel (n, Y, X)
  if (i >= total) return;
  const int X = i % (2 * wd);
  const int r = i / (2 * wd);
  const int Y = r % (2 * h), n = r / (2 * h);
  const int a = Y & 1, b = X & 1;
  const int iy0 = (Y >> 1) + a - 1, ix0 = (X >> 1) + b - 1;
  float v0 = 0.0f, v1 = 0.0f;
#pragma unroll
  for (int ci = 0; ci < 2; ++ci)
#pragma unroll
    for (int ty = 0; ty < 2; ++ty)
#pragma unroll
      for (int tx = 0; tx < 2; ++tx) {
        const int iy = iy0 + ty, ix = ix0 + tx;
        if ((unsigned)iy >= (unsigned)h || (unsigned)ix >= (unsigned)wd) continue;
        const float f = flow[((size_t)(n * 2 + ci) * h + iy) * wd + ix];
        const int k = (3 - a - 2 * ty) * 4 + (3 - b - 2 * tx);
        v0 = fmaf(f, w[(ci * 2 + 0) * 16 + k], v0);
        v1 = fmaf(f, w[(ci * 2 + 1) * 16 + k], v1);
      }
  float* o = out + (size_t)i * out_ld + coff;
  *reinterpret_cast<f32x4*>(o) = f32x4{v0, v1, 0.0f, 0.0f};
  for (int c = coff + 4; c < out_ld; c += 4) *reinterpret_cast<f32x4*>(o + (c - coff)) = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
}

inline int head_slices(int Cin) { return (Cin + kCS - 1) / kCS; }

}  // namespace
}  // namespace rmnet

extern "C" size_t rmnet_flow_head_workspace_bytes(int N, int H, int W, int Cin) {
  using namespace rmnet;
  if (N <= 0 || H <= 0 || W <= 0 || Cin <= 0) return 0;
  return (size_t)head_slices(Cin) * N * 2 * H * W * sizeof(float);
}

extern "C" int rmnet_flow_head_f32(const float* x, int x_ld, const float* wpack, const float* bias, int N, int H, int W, int Cin,
                                   float* out, void* workspace, size_t workspace_bytes, void* stream) {
  using namespace rmnet;
  if (!x || !wpack || !bias || !out || !workspace || N <= 0 || H <= 0 || W <= 0 || Cin <= 0) return RMNET_E_INVALID_ARG;
  if (x_ld % 4 || x_ld < Cin) return RMNET_E_INVALID_ARG;
  if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(workspace)) & 15) return RMNET_E_INVALID_ARG;
  if ((reinterpret_cast<uintptr_t>(wpack) | reinterpret_cast<uintptr_t>(bias) | reinterpret_cast<uintptr_t>(out)) & 3) return RMNET_E_INVALID_ARG;
  const int S = head_slices(Cin);
  const int TY = (H + kOH - 1) / kOH, TX = (W + kOW - 1) / kOW;
  const long long groups = (long long)N * TY * TX * S;
  const long long total = (long long)N * 2 * H * W;
  if ((long long)N * H * W * x_ld >= (1LL << 31) || groups >= (1LL << 31) || total >= (1LL << 31)) return RMNET_E_UNSUPPORTED;
  if (workspace_bytes < rmnet_flow_head_workspace_bytes(N, H, W, Cin)) return RMNET_E_INVALID_ARG;
  float* ws = static_cast<float*>(workspace);
  hipLaunchKernelGGL(flow_head, dim3((unsigned)groups), dim3(kThreads), kLdsBytes, (hipStream_t)stream, x, x_ld, wpack, ws, N, H, W, Cin,
                     TY, TX, S);
  hipLaunchKernelGGL(flow_head_sum, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, ws, bias, out, H * W,
                     (int)total, S);
  return check_launch();
}

extern "C" int rmnet_flow_up_f32(const float* flow, const float* w, int N, int h, int w_, float* out, int out_ld, int coff, void* stream) {
  using namespace rmnet;
  if (!flow || !w || !out || N <= 0 || h <= 0 || w_ <= 0) return RMNET_E_INVALID_ARG;
  if (out_ld <= 0 || out_ld % 4 || coff < 0 || coff % 4 || coff + 2 > out_ld) return RMNET_E_INVALID_ARG;
  if (reinterpret_cast<uintptr_t>(out) & 15) return RMNET_E_INVALID_ARG;
  if ((reinterpret_cast<uintptr_t>(flow) | reinterpret_cast<uintptr_t>(w)) & 3) return RMNET_E_INVALID_ARG;
  const long long total = (long long)N * 4 * h * w_;
  if (total * out_ld >= (1LL << 31)) return RMNET_E_UNSUPPORTED;
  hipLaunchKernelGGL(flow_up, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, flow, w, out, h, w_, out_ld, coff,
                     (int)total);
  return check_launch();
}
