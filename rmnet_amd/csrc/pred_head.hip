// pred_head.hip -- the decoder's prediction head: out [n][2][Hq][Wq] (NCHW) = conv3x3_p1(relu(x), w) + bias for a channels-last fp32
// x [n][Hq][Wq][C], C % 32 == 0 (the network: 256), plain fp32 FMA.  With two output channels the kernel is bound by reading x once;
// the stand-alone ReLU pass in front of the convolution and the NHWC -> NCHW copy behind it are gone.
//
// A workgroup (512 threads) owns 14 x 30 output pixels and stages their 16 x 32 halo tile, 32 channels at a time, in LDS (ReLU in
// the loader, zeros outside the map; the next chunk travels in registers).  Each thread is ONE halo pixel and accumulates its 18
// partial sums part[tap][co] = sum_c relu(x[pixel][c]) * w[co][c][tap] -- the weights are uniform across the wave and come through
// the scalar cache, so the inner loop is one LDS read per four channels and 72 FMAs.  The partials then go to LDS and every output
// pixel adds the nine it needs: out[co][y][x] = bias[co] + sum_tap part[(y + ky, x + kx)][tap][co].
#include "common.h"

namespace rmnet {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 512;
constexpr int kHH = 16, kHW = 32;          // halo tile (= threads)
constexpr int kOH = kHH - 2, kOW = kHW - 2;
constexpr int kCK = 32;                    // channels per chunk
constexpr int kXStride = kCK + 4;          // padded pixel row: conflict-free 16-byte reads at one pixel per lane
constexpr int kPStride = 19;               // 18 partials per pixel, odd stride
static_assert(kHH * kHW == kThreads, "one thread per halo pixel");

__global__ __launch_bounds__(kThreads) void pred_head(const float* __restrict__ x, const float* __restrict__ w,
                                                      const float* __restrict__ bias, float* __restrict__ out, int Hq, int Wq, int C,
                                                      int TY, int TX) {
  __shared__ __attribute__((aligned(16))) float lds[kThreads * kXStride];      // x chunk, then the partials [pixel][kPStride]
  const int tid = threadIdx.x;
  int t = blockIdx.x;
  const int n = t / (TY * TX);
  t -= n * (TY * TX);
  const int ty = t / TX, tx = t - ty * TX;
  const int y0 = ty * kOH - 1, x0 = tx * kOW - 1;       // the halo tile's first pixel

  // loader items: 8 x (pixel p = (tid + 512 i) / 8, channels 4 * (tid & 7) .. + 3 of the chunk)
  const int q4 = tid & 7;
  int src[8];                       // element offset of the pixel's channel 4 q4 (n * Hq * Wq * C < 2^31), -1 outside the map
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int p = (tid >> 3) + 64 * i;
    const int gy = y0 + p / kHW, gx = x0 + p % kHW;
    src[i] = ((unsigned)gy < (unsigned)Hq && (unsigned)gx < (unsigned)Wq) ? ((n * Hq + gy) * Wq + gx) * C + 4 * q4 : -1;
  }
  f32x4 xr[8];
  auto load = [&](int cb) {
#pragma unroll
    for (int i = 0; i < 8; ++i)
      xr[i] = src[i] >= 0 ? *reinterpret_cast<const f32x4*>(x + src[i] + cb * kCK) : f32x4{0.f, 0.f, 0.f, 0.f};
  };
  auto store = [&]() {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      f32x4 v = xr[i];
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = v[e] < 0.0f ? 0.0f : v[e];        // (ReLU keeps NaN)
      *reinterpret_cast<f32x4*>(lds + ((tid >> 3) + 64 * i) * kXStride + 4 * q4) = v;
    }
  };

  float part[2][9];
#pragma unroll
  for (int co = 0; co < 2; ++co)
#pragma unroll
    for (int k = 0; k < 9; ++k) part[co][k] = 0.0f;

  const int CB = C / kCK;
  load(0);
  for (int cb = 0; cb < CB; ++cb) {
    __syncthreads();                  // (the chunk before has been read)
    store();
    __syncthreads();
    if (cb + 1 < CB) load(cb + 1);
    const float* w0 = w + (size_t)cb * kCK * 9;                 // w[0][cb * 32][0][0]
    const float* w1 = w0 + (size_t)C * 9;                       // w[1][...]
#pragma unroll 1                   // (72 weights in SGPRs per pass; unrolled further, the scalar registers spill)
    for (int c4 = 0; c4 < kCK / 4; ++c4) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(lds + tid * kXStride + 4 * c4);
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int k = 0; k < 9; ++k) {
          part[0][k] = fmaf(v[e], w0[(4 * c4 + e) * 9 + k], part[0][k]);
          part[1][k] = fmaf(v[e], w1[(4 * c4 + e) * 9 + k], part[1][k]);
        }
    }
  }
  __syncthreads();
#pragma unroll
  for (int co = 0; co < 2; ++co)
#pragma unroll
    for (int k = 0; k < 9; ++k) lds[tid * kPStride + co * 9 + k] = part[co][k];
  __syncthreads();

  const int oy = tid / kHW, ox = tid % kHW;
  const int gy = ty * kOH + oy, gx = tx * kOW + ox;
  if (oy >= kOH || ox >= kOW || gy >= Hq || gx >= Wq) return;
  float s0 = bias[0], s1 = bias[1];
#pragma unroll
  for (int ky = 0; ky < 3; ++ky)
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const float* p = lds + ((oy + ky) * kHW + ox + kx) * kPStride + ky * 3 + kx;
      s0 += p[0];
      s1 += p[9];
    }
  const size_t plane = (size_t)Hq * Wq;
  float* o = out + (size_t)n * 2 * plane + (size_t)gy * Wq + gx;
  o[0] = s0;
  o[plane] = s1;
}

}  // namespace
}  // namespace rmnet

extern "C" int rmnet_pred_head_f32(const float* x, const float* w, const float* bias, int n, int Hq, int Wq, int C, float* out,
                                   void* stream) {
  using namespace rmnet;
  if (!x || !w || !bias || !out || n <= 0 || Hq <= 0 || Wq <= 0 || C <= 0) return RMNET_E_INVALID_ARG;
  if (reinterpret_cast<uintptr_t>(x) & 15) return RMNET_E_INVALID_ARG;
  if ((reinterpret_cast<uintptr_t>(w) | reinterpret_cast<uintptr_t>(bias) | reinterpret_cast<uintptr_t>(out)) & 3) return RMNET_E_INVALID_ARG;
  if (C % kCK) return RMNET_E_UNSUPPORTED;
  const int TY = (Hq + kOH - 1) / kOH, TX = (Wq + kOW - 1) / kOW;
  const long long tiles = (long long)n * TY * TX;
  if ((long long)n * Hq * Wq * C >= (1LL << 31) || tiles >= (1LL << 31)) return RMNET_E_UNSUPPORTED;
  hipLaunchKernelGGL(pred_head, dim3((unsigned)tiles), dim3(kThreads), 0, (hipStream_t)stream, x, w, bias, out, Hq, Wq, C, TY, TX);
  return check_launch();
}
