// tta.hip -- multi-scale and flipped inference (utils/helpers.py:44-78) around the network passes: the bilinear resize of the frames
// and the merge of the per-entry probability clips, written from the formula of torch's bilinear kernel with align_corners=False
// (include/rmnet_hip.h H1):
//
//   tta_resize   src [P,Hs,Ws] f32 -> dst [P,Hd,Wd] f32, F.interpolate(scale_factor=fs) with the scales given as floats; with
//                `flip` the row is written mirrored, which is torch.flip(resized, dims=[-1]) without a second pass
//   tta_merge    E <= 8 sources [N,K,hs_e,ws_e] f32, each resized to (H, W) (F.interpolate(size=)), a flipped source read
//                mirrored, summed in entry order and divided by E -> mean [N,K,H,W] f32 and, optionally, labels [N,H,W] u8, the first
//                index of the maximum of the written means.  No intermediate tensor: every source element is read once per output
//                row pair that needs it and every output is written once.
//
// The coordinate rule of one axis, axis(d, in, scale):  s = max(fl(fl(scale * fl(d + 0.5f)) - 0.5f), 0), i0 = min((int)s, in - 1),
// i1 = min(i0 + 1, in - 1), l1 = fl(s - (float)i0), l0 = fl(1 - l1).  The value is
//   fl( fl(l0y * fl(fl(l0x*A) + fl(l1x*B))) + fl(l1y * fl(fl(l0x*C) + fl(l1x*D))) )
// with A, B, C, D at (i0y,i0x), (i0y,i1x), (i1y,i0x), (i1y,i1x).  Every product and sum is rounded on its own, hence the pragma: hipcc
// contracts a * b + c into one fused operation in device code unless told otherwise.  The division by E is an IEEE division
// (correctly rounded by default; -ffast-math is not passed).
//
// Both kernels are memory bound.  In the merge a lane owns four consecutive output columns of one row and walks the K planes, and
// inside a plane the entries; the running first-index maximum of the means it writes becomes the label.  No LDS, no scratch.
#include "common.h"

#pragma clang fp contract(off)

namespace rmnet {
namespace {

constexpr int kThreads = 256;
constexpr int kMergeX = 64, kMergeY = 4;        // a merge workgroup: 64 column groups x 4 rows
constexpr int kV = 4;                           // output columns per lane in the merge
constexpr int kMaxSide = 1 << 24;               // source sides are exact floats

struct Axis { int i0, i1; float l0, l1; };

__device__ inline Axis axis(int d, int in, float scale) {
  Axis a;
  const float s = fmaxf(scale * ((float)d + 0.5f) - 0.5f, 0.0f);
  a.i0 = (int)fminf(s, (float)(in - 1));                  // min((int)s, in - 1) without converting a float past the int range
  a.i1 = min(a.i0 + 1, in - 1);
  a.l1 = s - (float)a.i0;
  a.l0 = 1.0f - a.l1;
  return a;
}

__device__ inline float blend(float l0y, float l1y, float l0x, float l1x, float A, float B, float C, float D) {
  return l0y * (l0x * A + l1x * B) + l1y * (l0x * C + l1x * D);
}

// ------------------------------------------------------------------------------------------------ frames
// grid: x = ceil(Wd / kThreads), y = Hd, z = min(P, 65535); a lane owns one output column of one row and walks the planes
__global__ __launch_bounds__(kThreads) void tta_resize(const float* __restrict__ src, float* __restrict__ dst, int P, int Hs, int Ws,
                                                       int Hd, int Wd, float scale_h, float scale_w, int flip) {
  const int x = blockIdx.x * kThreads + threadIdx.x;
  const int y = blockIdx.y;
  if (x >= Wd) return;
  const Axis ay = axis(y, Hs, scale_h), ax = axis(x, Ws, scale_w);
  const long long plane_s = (long long)Hs * Ws, plane_d = (long long)Hd * Wd;
  const long long r0 = (long long)ay.i0 * Ws, r1 = (long long)ay.i1 * Ws;
  const long long at = (long long)y * Wd + (flip ? Wd - 1 - x : x);
  for (int p = blockIdx.z; p < P; p += gridDim.z) {
    const float* s = src + p * plane_s;
    dst[p * plane_d + at] = blend(ay.l0, ay.l1, ax.l0, ax.l1, s[r0 + ax.i0], s[r0 + ax.i1], s[r1 + ax.i0], s[r1 + ax.i1]);
  }
}

// ------------------------------------------------------------------------------------------------ probabilities
struct MergeSrc {
  const float* p[RMNET_TTA_MAX_ENTRIES];
  int hs[RMNET_TTA_MAX_ENTRIES], ws[RMNET_TTA_MAX_ENTRIES], flipped[RMNET_TTA_MAX_ENTRIES];
  float scale_h[RMNET_TTA_MAX_ENTRIES], scale_w[RMNET_TTA_MAX_ENTRIES];      // fl((float)hs / (float)H), fl((float)ws / (float)W): host divisions
};

// grid: x = ceil(ceil(W / 4) / 64), y = ceil(H / 4), z = min(N, 65535).  The coordinates of an entry are a dozen VALU operations per
// axis and are formed again for every plane.  Kept in registers over the K loop (the entry count a template parameter) they cost
// some 60 VGPRs per entry, 344 at six entries and 488 at eight, i.e. one wave per SIMD, and that kernel was the slower one: 6.17
// against 5.87 ms on the clip of profiles/r28_a_tta.md.  Sixteen dword gathers per entry and plane for four outputs are what both pay.
__global__ __launch_bounds__(kThreads) void tta_merge(MergeSrc q, float* __restrict__ mean, uint8_t* __restrict__ labels, int E, int N,
                                                      int K, int H, int W) {
  const int x0 = (blockIdx.x * kMergeX + threadIdx.x) * kV;
  const int y = blockIdx.y * kMergeY + threadIdx.y;
  if (x0 >= W || y >= H) return;
  const long long HW = (long long)H * W;
  const long long at = (long long)y * W + x0;
  const bool full = x0 + kV <= W;
  const float entries = (float)E;
  for (int n = blockIdx.z; n < N; n += gridDim.z) {
    float best[kV];
    int idx[kV];
#pragma unroll
    for (int i = 0; i < kV; ++i) { best[i] = -INFINITY; idx[i] = 0; }
    for (int k = 0; k < K; ++k) {
      const long long plane = (long long)n * K + k;
      float acc[kV];
      for (int e = 0; e < E; ++e) {
        const int hs = q.hs[e], ws = q.ws[e], flipped = q.flipped[e];
        const float scale_w = q.scale_w[e];
        const Axis ay = axis(y, hs, q.scale_h[e]);
        const float* s = q.p[e] + plane * ((long long)hs * ws);
        const float* a = s + ay.i0 * ws;
        const float* b = s + ay.i1 * ws;
#pragma unroll
        for (int i = 0; i < kV; ++i) {
          const Axis ax = axis(min(x0 + i, W - 1), ws, scale_w);       // (a column past the row's end is computed in bounds, not stored)
          const int c0 = flipped ? ws - 1 - ax.i0 : ax.i0, c1 = flipped ? ws - 1 - ax.i1 : ax.i1;
          const float v = blend(ay.l0, ay.l1, ax.l0, ax.l1, a[c0], a[c1], b[c0], b[c1]);
          acc[i] = e == 0 ? v : acc[i] + v;
        }
      }
      float* dst = mean + plane * HW + at;
#pragma unroll
      for (int i = 0; i < kV; ++i) {
        acc[i] = acc[i] / entries;
        if (acc[i] > best[i]) { best[i] = acc[i]; idx[i] = k; }      // strictly greater: the first index of the maximum stays
      }
      if (full && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
        *reinterpret_cast<float4*>(dst) = make_float4(acc[0], acc[1], acc[2], acc[3]);
      } else {
#pragma unroll
        for (int i = 0; i < kV; ++i)
          if (x0 + i < W) dst[i] = acc[i];
      }
    }
    if (labels) {
      uint8_t* lab = labels + (long long)n * HW + at;
      if (full && (reinterpret_cast<uintptr_t>(lab) & 3) == 0) {
        *reinterpret_cast<uint32_t*>(lab) = (uint32_t)idx[0] | ((uint32_t)idx[1] << 8) | ((uint32_t)idx[2] << 16) | ((uint32_t)idx[3] << 24);
      } else {
#pragma unroll
        for (int i = 0; i < kV; ++i)
          if (x0 + i < W) lab[i] = (uint8_t)idx[i];
      }
    }
  }
}

inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }
inline bool good_scale(float s) { return s > 0.0f && s <= 3.0e38f; }        // finite and positive (false for a NaN)

}  // namespace

int launch_resize_bilinear(const float* src, int P, int Hs, int Ws, int Hd, int Wd, float scale_h, float scale_w, int flip, float* dst,
                           hipStream_t st) {
  if (!src || !dst || P <= 0 || Hs <= 0 || Ws <= 0 || Hd <= 0 || Wd <= 0) return RMNET_E_INVALID_ARG;
  if (!good_scale(scale_h) || !good_scale(scale_w) || !aligned4(src) || !aligned4(dst)) return RMNET_E_INVALID_ARG;
  if (Hd > 65535 || Hs > kMaxSide || Ws > kMaxSide) return RMNET_E_UNSUPPORTED;
  hipLaunchKernelGGL(tta_resize, dim3((unsigned)((Wd + kThreads - 1) / kThreads), (unsigned)Hd, (unsigned)min(P, 65535)), dim3(kThreads), 0,
                     st, src, dst, P, Hs, Ws, Hd, Wd, scale_h, scale_w, flip ? 1 : 0);
  return check_launch();
}

int launch_tta_merge(const float* const* srcs, const int* hs, const int* ws, const int* flipped, int E, int N, int K, int H, int W,
                     float* mean, uint8_t* labels, hipStream_t st) {
  if (!srcs || !hs || !ws || !flipped || !mean || N <= 0 || H <= 0 || W <= 0) return RMNET_E_INVALID_ARG;
  if (E < 1 || E > RMNET_TTA_MAX_ENTRIES || K < 1 || K > 255 || !aligned4(mean)) return RMNET_E_INVALID_ARG;
  MergeSrc q = {};
  for (int e = 0; e < E; ++e) {
    if (!srcs[e] || hs[e] <= 0 || ws[e] <= 0 || !aligned4(srcs[e])) return RMNET_E_INVALID_ARG;
    if (hs[e] > kMaxSide || ws[e] > kMaxSide || (long long)hs[e] * ws[e] >= (1LL << 31)) return RMNET_E_UNSUPPORTED;      // row offsets inside a plane are 32-bit
    q.p[e] = srcs[e]; q.hs[e] = hs[e]; q.ws[e] = ws[e]; q.flipped[e] = flipped[e] ? 1 : 0;
    q.scale_h[e] = (float)hs[e] / (float)H; q.scale_w[e] = (float)ws[e] / (float)W;
  }
  if ((H + kMergeY - 1) / kMergeY > 65535) return RMNET_E_UNSUPPORTED;
  const unsigned gx = (unsigned)(((W + kV - 1) / kV + kMergeX - 1) / kMergeX), gy = (unsigned)((H + kMergeY - 1) / kMergeY);
  hipLaunchKernelGGL(tta_merge, dim3(gx, gy, (unsigned)min(N, 65535)), dim3(kMergeX, kMergeY), 0, st, q, mean, labels, E, N, K, H, W);
  return check_launch();
}

}  // namespace rmnet
