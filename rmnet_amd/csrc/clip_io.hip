// clip_io.hip -- the two ends of the inference driver (core/inference.py:50-71) as per-pixel kernels: uint8 frames and label maps in,
// uint8 label maps and overlay frames out.  Every result equals the reference's host arithmetic bit for bit (include/rmnet_hip.h F1):
//
//   cio_normalize   frames [N,H,W,3] u8 -> [N,3,H,W] f32: fl32(u / 255.f), then fl32((double(x) - mean[c]) / std[c]), as numpy's
//                   img_normalize (utils/helpers.py:133-135) followed by astype(float32) (utils/data_transforms.py:93)
//   cio_onehot      labels [N,H,W] u8 -> [N,K,H,W] u8 through an optional 256-entry remap table (utils/helpers.py:81-90 after
//                   ReorganizeObjectID, utils/data_transforms.py:53-68)
//   cio_argmax      prob [N,K,H,W] f32 -> labels [N,H,W] u8, the first index of the maximum
//   cio_lowest_*    the smallest label of every frame, into the int32 [N] workspace of the overlay
//   cio_overlay     get_segmentation (utils/helpers.py:165-176) restated per pixel; see the rule in front of the kernel
//
// All of them are memory bound: a lane owns V consecutive pixels of one frame (V = 4, or 16 for the byte-only one-hot planes)
// whenever the plane size and the pointers allow dword / dwordx4 accesses, and V = 1 otherwise.  The workgroups of a frame are
// blockIdx.x / blocks_per_frame, so the frame index is wave-uniform and no 64-bit division happens per lane except the one that
// finds a lane's row in the overlay.  No LDS, no scratch.
//
// The double arithmetic of the overlay must round every product and every sum on its own, which is what numpy does; hipcc
// contracts a * b + c into one fused operation in device code unless told otherwise, hence the pragma below.  (The divisions of
// cio_normalize are IEEE divisions: correctly rounded by default, and -ffast-math is not passed.)
#include "common.h"

#pragma clang fp contract(off)

namespace rmnet {
namespace {

constexpr int kThreads = 256;
constexpr int kLowIter = 8;          // pixel groups per lane in cio_lowest: one atomic per wave and 64 * V * kLowIter pixels

struct Norm3 { double mean[3], std[3]; };
struct Blend { double mean[3], std[3], alpha, one_minus_alpha; int ignore_idx; };

// V consecutive bytes at p (aligned to V for V = 4, 16), one per int
template <int V> __device__ inline void load_bytes(const uint8_t* p, int (&b)[V]) {
  if constexpr (V == 1) {
    b[0] = p[0];
  } else if constexpr (V == 4) {
    const uint32_t w = *reinterpret_cast<const uint32_t*>(p);
#pragma unroll
    for (int i = 0; i < 4; ++i) b[i] = (w >> (8 * i)) & 255u;
  } else {
    const uint4 w = *reinterpret_cast<const uint4*>(p);
    const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int i = 0; i < 16; ++i) b[i] = (ws[i >> 2] >> (8 * (i & 3))) & 255u;
  }
}

template <int V> __device__ inline void store_bytes(uint8_t* p, const int (&b)[V]) {
  if constexpr (V == 1) {
    p[0] = (uint8_t)b[0];
  } else {
    uint32_t ws[V / 4];
#pragma unroll
    for (int j = 0; j < V / 4; ++j)
      ws[j] = (uint32_t)b[4 * j] | ((uint32_t)b[4 * j + 1] << 8) | ((uint32_t)b[4 * j + 2] << 16) | ((uint32_t)b[4 * j + 3] << 24);
    if constexpr (V == 4) {
      *reinterpret_cast<uint32_t*>(p) = ws[0];
    } else if constexpr (V == 12) {
      uint32_t* q = reinterpret_cast<uint32_t*>(p);
      q[0] = ws[0]; q[1] = ws[1]; q[2] = ws[2];
    } else {
      *reinterpret_cast<uint4*>(p) = make_uint4(ws[0], ws[1], ws[2], ws[3]);
    }
  }
}

// first pixel of this lane inside its frame, or -1 when the lane has none
template <int V> __device__ inline long long lane_pixel(unsigned bpf, long long HW) {
  const long long p = ((long long)(blockIdx.x % bpf) * kThreads + threadIdx.x) * V;
  return p < HW ? p : -1;
}

// ------------------------------------------------------------------------------------------------ frames in
template <int V>
__global__ __launch_bounds__(kThreads) void cio_normalize(const uint8_t* __restrict__ in, float* __restrict__ out, long long HW, unsigned bpf,
                                                          Norm3 q) {
  const long long n = blockIdx.x / bpf;
  const long long p = lane_pixel<V>(bpf, HW);
  if (p < 0) return;
  const uint8_t* src = in + (n * HW + p) * 3;
  int b[3 * V];
  if constexpr (V == 4) {
    int w0[4], w1[4], w2[4];
    load_bytes<4>(src, w0); load_bytes<4>(src + 4, w1); load_bytes<4>(src + 8, w2);
#pragma unroll
    for (int i = 0; i < 4; ++i) { b[i] = w0[i]; b[4 + i] = w1[i]; b[8 + i] = w2[i]; }
  } else {
    b[0] = src[0]; b[1] = src[1]; b[2] = src[2];
  }
  float* dst = out + n * 3 * HW + p;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float y[V];
#pragma unroll
    for (int i = 0; i < V; ++i) {
      const float x = (float)b[3 * i + c] / 255.0f;
      y[i] = (float)(((double)x - q.mean[c]) / q.std[c]);
    }
    if constexpr (V == 4) *reinterpret_cast<float4*>(dst + c * HW) = make_float4(y[0], y[1], y[2], y[3]);
    else dst[c * HW] = y[0];
  }
}

// ------------------------------------------------------------------------------------------------ label maps in
template <int V>
__global__ __launch_bounds__(kThreads) void cio_onehot(const uint8_t* __restrict__ labels, const uint8_t* __restrict__ lut,
                                                       uint8_t* __restrict__ out, int K, long long HW, unsigned bpf) {
  const long long n = blockIdx.x / bpf;
  const long long p = lane_pixel<V>(bpf, HW);
  if (p < 0) return;
  int l[V];
  load_bytes<V>(labels + n * HW + p, l);
  if (lut) {
#pragma unroll
    for (int i = 0; i < V; ++i) l[i] = lut[l[i]];
  }
  uint8_t* dst = out + n * K * HW + p;
  for (int k = 0; k < K; ++k) {
    int o[V];
#pragma unroll
    for (int i = 0; i < V; ++i) o[i] = l[i] == k;
    store_bytes<V>(dst + k * HW, o);
  }
}

// ------------------------------------------------------------------------------------------------ label maps out
template <int V>
__global__ __launch_bounds__(kThreads) void cio_argmax(const float* __restrict__ prob, uint8_t* __restrict__ labels, int K, long long HW,
                                                       unsigned bpf) {
  const long long n = blockIdx.x / bpf;
  const long long p = lane_pixel<V>(bpf, HW);
  if (p < 0) return;
  const float* src = prob + n * K * HW + p;
  float best[V];
  int idx[V];
#pragma unroll
  for (int i = 0; i < V; ++i) { best[i] = -INFINITY; idx[i] = 0; }
#pragma unroll 4
  for (int k = 0; k < K; ++k) {
    float v[V];
    if constexpr (V == 4) {
      const float4 f = *reinterpret_cast<const float4*>(src + k * HW);
      v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
    } else {
      v[0] = src[k * HW];
    }
#pragma unroll
    for (int i = 0; i < V; ++i)
      if (v[i] > best[i]) { best[i] = v[i]; idx[i] = k; }          // strictly greater: the first index of the maximum stays
  }
  store_bytes<V>(labels + n * HW + p, idx);
}

// ------------------------------------------------------------------------------------------------ overlay frames out
__global__ void cio_lowest_init(int32_t* __restrict__ lowest, int N) {
  const int n = blockIdx.x * kThreads + threadIdx.x;
  if (n < N) lowest[n] = 255;                                       // no label is larger
}

template <int V>
__global__ __launch_bounds__(kThreads) void cio_lowest_min(const uint8_t* __restrict__ labels, int32_t* __restrict__ lowest, long long HW,
                                                           unsigned bpf) {
  const long long n = blockIdx.x / bpf;
  const uint8_t* lab = labels + n * HW;
  const long long p0 = ((long long)(blockIdx.x % bpf) * kLowIter * kThreads + threadIdx.x) * V;
  int m = 255;
#pragma unroll
  for (int it = 0; it < kLowIter; ++it) {
    const long long p = p0 + (long long)it * kThreads * V;
    if (p < HW) {
      int l[V];
      load_bytes<V>(lab + p, l);
#pragma unroll
      for (int i = 0; i < V; ++i) m = min(m, l[i]);
    }
  }
  m = wave_min(m);
  if ((threadIdx.x & (RMNET_WAVE - 1)) == 0 && m < 255) atomicMin(lowest + n, m);      // a minimum: the same bits in any order
}

// (uint8) of a double the way numpy casts it for values in (-1, 256): towards zero.  Outside that range, where numpy's cast is
// undefined, the result saturates; a NaN gives 0.
__device__ inline int to_u8(double d) { return !(d > 0.0) ? 0 : d >= 255.0 ? 255 : (int)d; }

// PALETTE[o][c] of utils/helpers.py:139-157: the 16 DAVIS colours (bits 0, 1, 2 of the id give 128 in red, green, blue and bit 3
// adds 64 to red, where 128 + 64 is stored as 191), then grey [o, o, o]
__device__ inline int palette(int o, int c) {
  if (o >= 16) return o;
  if (c == 0) return ((o & 1) << 7) + ((o >> 3 & 1) << 6) - ((o & 1) & (o >> 3 & 1));
  return ((o >> c) & 1) << 7;
}

// The rule of utils/helpers.py:165-176 at one pixel.  S = the labels of this frame without its smallest one and without
// ignore_idx (np.unique(mask)[1:] minus the ignored id).  The reference walks S in ascending order; object o blends the pixels
// that carry it and then blackens its contour, binary_dilation(mask == o) ^ (mask == o) with the 4-neighbour cross and nothing
// beyond the border.  At one pixel with label L that is: one event per neighbour label o != L in S (v = 0 at step o) and, when L
// is in S, the blend at step L.  A zero after the blend leaves 0, a zero before it leaves the blend of 0:
//   L in S:      0 if a neighbour event is above L, else blend(0) if one is below L, else blend(denormalised)
//   L not in S:  0 if there is any neighbour event, else the denormalised pixel
// Each of the three products / sums of the denormalisation and of the blend is rounded on its own (contraction is off).
template <int V>
__global__ __launch_bounds__(kThreads) void cio_overlay(const float* __restrict__ frames, const uint8_t* __restrict__ labels,
                                                        const int32_t* __restrict__ lowest, uint8_t* __restrict__ out, int H, int W,
                                                        long long HW, unsigned bpf, Blend q) {
  const long long n = blockIdx.x / bpf;
  const long long p = lane_pixel<V>(bpf, HW);
  if (p < 0) return;
  const uint8_t* lab = labels + n * HW;
  const float* src = frames + n * 3 * HW + p;
  const int low = lowest[n], ign = q.ignore_idx;
  int own[V];
  load_bytes<V>(lab + p, own);
  float x[3][V];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    if constexpr (V == 4) {
      const float4 f = *reinterpret_cast<const float4*>(src + c * HW);
      x[c][0] = f.x; x[c][1] = f.y; x[c][2] = f.z; x[c][3] = f.w;
    } else {
      x[c][0] = src[c * HW];
    }
  }
  int py = (int)(p / W), px = (int)(p % W);
  int o8[3 * V];
#pragma unroll
  for (int i = 0; i < V; ++i) {
    const long long at = p + i;
    const int L = own[i];
    int nb[4];
    nb[0] = px > 0 ? (i > 0 ? own[i > 0 ? i - 1 : 0] : (int)lab[at - 1]) : -1;
    nb[1] = px + 1 < W ? (i + 1 < V ? own[i + 1 < V ? i + 1 : 0] : (int)lab[at + 1]) : -1;
    nb[2] = py > 0 ? (int)lab[at - W] : -1;
    nb[3] = py + 1 < H ? (int)lab[at + W] : -1;
    int zlo = 256, zhi = -1;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int o = nb[j];
      if (o >= 0 && o != L && o != low && o != ign) { zlo = min(zlo, o); zhi = max(zhi, o); }
    }
    const bool mine = L != low && L != ign;
    const bool zero = mine ? zhi > L : zhi >= 0;                    // the last event is a contour
    const bool from_zero = mine && zlo < L;                         // the blend starts from a blackened pixel
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      int v = to_u8(((double)x[c][i] * q.std[c] + q.mean[c]) * 255.0);
      if (from_zero) v = 0;
      if (mine) v = to_u8((double)v * q.alpha + q.one_minus_alpha * (double)palette(L, c));
      o8[3 * i + c] = zero ? 0 : v;
    }
    if (++px == W) { px = 0; ++py; }
  }
  uint8_t* dst = out + (n * HW + p) * 3;
  if constexpr (V == 4) {
    store_bytes<12>(dst, o8);
  } else {
    dst[0] = (uint8_t)o8[0]; dst[1] = (uint8_t)o8[1]; dst[2] = (uint8_t)o8[2];
  }
}

inline bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// workgroups per frame for `per_block` pixels each, and the whole grid; false when the launch would pass 2^31 - 1 workgroups
inline bool grid_for(int N, long long HW, long long per_block, unsigned* bpf, unsigned* grid) {
  const long long b = (HW + per_block - 1) / per_block;
  if (b >= (1LL << 31) || b * N >= (1LL << 31)) return false;
  *bpf = (unsigned)b;
  *grid = (unsigned)(b * N);
  return true;
}

}  // namespace

int launch_frames_normalize(const uint8_t* frames, int N, int H, int W, const double* mean, const double* std, float* out, hipStream_t st) {
  if (!frames || !out || !mean || !std || N <= 0 || H <= 0 || W <= 0) return RMNET_E_INVALID_ARG;
  Norm3 q;
  for (int c = 0; c < 3; ++c) {
    if (std[c] == 0.0) return RMNET_E_INVALID_ARG;
    q.mean[c] = mean[c]; q.std[c] = std[c];
  }
  if (!aligned(out, 4)) return RMNET_E_INVALID_ARG;
  const long long HW = (long long)H * W;
  const bool vec = HW % 4 == 0 && aligned(frames, 4) && aligned(out, 16);
  unsigned bpf, grid;
  if (!grid_for(N, HW, kThreads * (vec ? 4 : 1), &bpf, &grid)) return RMNET_E_UNSUPPORTED;
  if (vec) hipLaunchKernelGGL(cio_normalize<4>, dim3(grid), dim3(kThreads), 0, st, frames, out, HW, bpf, q);
  else hipLaunchKernelGGL(cio_normalize<1>, dim3(grid), dim3(kThreads), 0, st, frames, out, HW, bpf, q);
  return check_launch();
}

int launch_labels_onehot(const uint8_t* labels, const uint8_t* lut, int N, int K, int H, int W, uint8_t* out, hipStream_t st) {
  if (!labels || !out || N <= 0 || K <= 0 || H <= 0 || W <= 0) return RMNET_E_INVALID_ARG;
  if (K > 255) return RMNET_E_UNSUPPORTED;
  const long long HW = (long long)H * W;
  const int V = HW % 16 == 0 && aligned(labels, 16) && aligned(out, 16) ? 16 : HW % 4 == 0 && aligned(labels, 4) && aligned(out, 4) ? 4 : 1;
  unsigned bpf, grid;
  if (!grid_for(N, HW, kThreads * V, &bpf, &grid)) return RMNET_E_UNSUPPORTED;
  if (V == 16) hipLaunchKernelGGL(cio_onehot<16>, dim3(grid), dim3(kThreads), 0, st, labels, lut, out, K, HW, bpf);
  else if (V == 4) hipLaunchKernelGGL(cio_onehot<4>, dim3(grid), dim3(kThreads), 0, st, labels, lut, out, K, HW, bpf);
  else hipLaunchKernelGGL(cio_onehot<1>, dim3(grid), dim3(kThreads), 0, st, labels, lut, out, K, HW, bpf);
  return check_launch();
}

int launch_argmax_labels(const float* prob, int N, int K, int H, int W, uint8_t* labels, hipStream_t st) {
  if (!prob || !labels || N <= 0 || K <= 0 || H <= 0 || W <= 0 || !aligned(prob, 4)) return RMNET_E_INVALID_ARG;
  if (K > 255) return RMNET_E_UNSUPPORTED;
  const long long HW = (long long)H * W;
  const bool vec = HW % 4 == 0 && aligned(prob, 16) && aligned(labels, 4);
  unsigned bpf, grid;
  if (!grid_for(N, HW, kThreads * (vec ? 4 : 1), &bpf, &grid)) return RMNET_E_UNSUPPORTED;
  if (vec) hipLaunchKernelGGL(cio_argmax<4>, dim3(grid), dim3(kThreads), 0, st, prob, labels, K, HW, bpf);
  else hipLaunchKernelGGL(cio_argmax<1>, dim3(grid), dim3(kThreads), 0, st, prob, labels, K, HW, bpf);
  return check_launch();
}

int launch_overlay(const float* frames, const uint8_t* labels, int N, int H, int W, const double* mean, const double* std, double alpha,
                   int ignore_idx, uint8_t* out, int32_t* ws, size_t ws_bytes, hipStream_t st) {
  if (!frames || !labels || !out || !mean || !std || N <= 0 || H <= 0 || W <= 0 || !aligned(frames, 4)) return RMNET_E_INVALID_ARG;
  if (!(alpha >= 0.0 && alpha <= 1.0)) return RMNET_E_INVALID_ARG;
  Blend q;
  for (int c = 0; c < 3; ++c) {
    if (std[c] == 0.0) return RMNET_E_INVALID_ARG;
    q.mean[c] = mean[c]; q.std[c] = std[c];
  }
  q.alpha = alpha;
  q.one_minus_alpha = 1.0 - alpha;                                   // np.ones(...) * (1 - alpha): one host subtraction
  q.ignore_idx = ignore_idx;
  if (!ws || ws_bytes < (size_t)N * sizeof(int32_t)) return RMNET_E_WORKSPACE;
  if (!aligned(ws, 4)) return RMNET_E_INVALID_ARG;
  const long long HW = (long long)H * W;
  const bool vec = HW % 4 == 0 && aligned(frames, 16) && aligned(labels, 4) && aligned(out, 4);
  const int V = vec ? 4 : 1;
  unsigned bpf, grid, bpf_low, grid_low;
  if (!grid_for(N, HW, kThreads * V, &bpf, &grid) || !grid_for(N, HW, (long long)kThreads * V * kLowIter, &bpf_low, &grid_low))
    return RMNET_E_UNSUPPORTED;
  hipLaunchKernelGGL(cio_lowest_init, dim3((unsigned)((N + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, ws, N);
  if (vec) {
    hipLaunchKernelGGL(cio_lowest_min<4>, dim3(grid_low), dim3(kThreads), 0, st, labels, ws, HW, bpf_low);
    hipLaunchKernelGGL(cio_overlay<4>, dim3(grid), dim3(kThreads), 0, st, frames, labels, ws, out, H, W, HW, bpf, q);
  } else {
    hipLaunchKernelGGL(cio_lowest_min<1>, dim3(grid_low), dim3(kThreads), 0, st, labels, ws, HW, bpf_low);
    hipLaunchKernelGGL(cio_overlay<1>, dim3(grid), dim3(kThreads), 0, st, frames, labels, ws, out, H, W, HW, bpf, q);
  }
  return check_launch();
}

}  // namespace rmnet
