// decoder_glue_bwd.hip -- the gradients of the decoder's glue: the adjoint of the x2 / x4 bilinear upsample (align_corners = False)
// and the backward of the prediction head out = conv3x3_p1(relu(x), w) + bias (include/rmnet_hip.h: rmnet_upsample_bwd_f32,
// rmnet_pred_head_bwd_f32).  Plain fp32 FMA, no atomics, no memset: every output element is written exactly once and has the same
// bits on every call.
//
// 1. The upsample's adjoint is a GATHER with constant weights.  The forward (csrc/epilogue.hip: tap2x, and torch) reads, for the fine
//    index d, src = max((d + 0.5) / S - 0.5, 0), i0 = floor(src), i1 = i0 + (i0 < n - 1) with the weights 1 - (src - i0), src - i0.
//    So coarse j is read by the 2 S fine indices d = S j - S / 2 + t, t = 0 .. 2 S - 1, with the weight (2 t + 1) / (2 S) for t < S and
//    its mirror behind; at j = 0 the S / 2 taps before the map do not exist and the next S / 2 weigh 1 (the clamp of src folds the
//    weight of coarse -1 onto coarse 0); at j = n - 1 the mirror image of that (adj_row below).  2-D is the outer product.
//    SUMMATION ORDER of one output element: fine rows ascending; inside a row s = 0, then s = fma(wx, g, s) over the row's existing
//    fine columns ascending; then acc = fma(wy, s, acc), acc = 0 before the first row.
//    NHWC: a thread is one coarse pixel x 4 channels and reads 16 bytes of channels per tap.  NCHW: a thread is one 16-byte group of
//    fine columns (4 / S coarse columns) of one coarse row and reads the group as one vector where g and the fine rows are 16-byte
//    aligned, the S / 2 columns on either side as scalars.  Grid-stride loops over at most kUpBlocks workgroups.
//
// 2. The prediction head.  With G[k][ky][kx](y, x) = g[k][y - ky + 1][x - kx + 1] (zero outside the map) both gradients read the
//    SAME 18 values of g at an input pixel p = (y, x):
//      dx[p][c]           = [x[p][c] > 0] * sum over k, ky, kx (in that order, dx = fma(w, G, dx) from 0) of w[k][c][ky][kx] * G[k][ky][kx](p)
//      dw[k][c][ky][kx]   = sum over p of relu(x)[p][c] * G[k][ky][kx](p)          (relu(x) = x > 0 ? x : 0: a NaN counts as 0)
//      db[k]              = sum over p of g[k][p]
//    so ONE pass over x produces dx and the partials of dw and db (two kernels would read x twice; the one pass needs 72
//    accumulators + 72 weights for the 4 channels of a lane, inside the 256 registers of a 256-thread workgroup, no scratch).
//    A workgroup (256 threads) owns kPhCT = 32 channels (8 lanes x 4) of one RANGE of pixels (linear n, y, x order; ph_plan below)
//    as 32 pixel SLOTS: slot s walks the pixels begin + s, begin + s + 32, ... and keeps acc = fma(relu(x), G, acc).  The slots'
//    partials are then added in slot order (through dynamic LDS, one output plane at a time) and written to the workspace;
//    pred_head_bwd_merge adds the ranges' partials in range order.  g is read from global memory (8 lanes share an address; it is
//    1 / 128 of the bytes of x at C = 256).
#include "split_f16.h"

namespace rmnet {
namespace {

constexpr int kGlueThreads = 256;
constexpr int kUpBlocks = 4 * kNumCUs;

// ------------------------------------------------------------------------------------------------ 1. upsample, adjoint
template <int S>
__device__ __forceinline__ void adj_row(int j, int n, float (&wt)[2 * S]) {
#pragma unroll
  for (int t = 0; t < 2 * S; ++t) {
    float v = (float)(t < S ? 2 * t + 1 : 4 * S - 2 * t - 1) * (0.5f / S);
    if (j == 0) v = t < S / 2 ? 0.0f : (t < S ? 1.0f : v);
    if (j == n - 1) v = t >= S + S / 2 ? 0.0f : (t >= S ? 1.0f : v);
    wt[t] = v;
  }
}

template <int S>
__global__ __launch_bounds__(kGlueThreads) void upsample_bwd_nhwc(const float* __restrict__ g, float* __restrict__ out, int h, int w,
                                                                  int C4, long long items) {
  const int W = S * w;
  for (long long it = (long long)blockIdx.x * kGlueThreads + threadIdx.x; it < items; it += (long long)gridDim.x * kGlueThreads) {
    const int c4 = (int)(it % C4);
    const long long pix = it / C4;
    const int j = (int)(pix % w);
    const long long row = pix / w;                     // img * h + i
    const int i = (int)(row % h);
    const long long img = row / h;
    float wy[2 * S], wx[2 * S];
    adj_row<S>(i, h, wy);
    adj_row<S>(j, w, wx);
    const float* base = g + ((img * S * h) * W) * (long long)C4 * 4 + 4 * c4;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll                      // (fully: the weights are register arrays)
    for (int ty = 0; ty < 2 * S; ++ty) {
      const int r = S * i - S / 2 + ty;
      f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int tx = 0; tx < 2 * S; ++tx) {
        const int c = S * j - S / 2 + tx;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (wy[ty] != 0.0f && wx[tx] != 0.0f) v = *reinterpret_cast<const f32x4*>(base + ((long long)r * W + c) * C4 * 4);
        s = __builtin_elementwise_fma(f32x4{wx[tx], wx[tx], wx[tx], wx[tx]}, v, s);
      }
      acc = __builtin_elementwise_fma(f32x4{wy[ty], wy[ty], wy[ty], wy[ty]}, s, acc);
    }
    *reinterpret_cast<f32x4*>(out + it * 4) = acc;
  }
}

template <int S, bool VEC>
__global__ __launch_bounds__(kGlueThreads) void upsample_bwd_nchw(const float* __restrict__ g, float* __restrict__ out, int h, int w,
                                                                  long long items) {
  constexpr int Q = 4 / S;            // coarse columns per thread: one 16-byte group of fine columns
  constexpr int NV = 4 + S;           // fine columns a thread reads per row: the group and S / 2 on either side
  const int W = S * w;
  const int GW = (w + Q - 1) / Q;
  for (long long it = (long long)blockIdx.x * kGlueThreads + threadIdx.x; it < items; it += (long long)gridDim.x * kGlueThreads) {
    const int jq = (int)(it % GW);
    const long long row = it / GW;                     // plane * h + i
    const int i = (int)(row % h);
    const long long plane = row / h;
    float wy[2 * S], wx[Q][2 * S];
    adj_row<S>(i, h, wy);
#pragma unroll
    for (int q = 0; q < Q; ++q) adj_row<S>(jq * Q + q, w, wx[q]);
    const float* base = g + plane * (long long)(S * h) * W;
    const int c0 = 4 * jq;
    float acc[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) acc[q] = 0.0f;
#pragma unroll
    for (int ty = 0; ty < 2 * S; ++ty) {
      const int r = S * i - S / 2 + ty;
      float v[NV];
#pragma unroll
      for (int e = 0; e < NV; ++e) v[e] = 0.0f;
      if (wy[ty] != 0.0f) {
        const float* p = base + (long long)r * W + c0;
        if (VEC) {
          const f32x4 m = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
          for (int e = 0; e < 4; ++e) v[S / 2 + e] = m[e];
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (c0 + e < W) v[S / 2 + e] = p[e];
        }
#pragma unroll
        for (int e = 0; e < S / 2; ++e) {
          if (c0 - S / 2 + e >= 0) v[e] = p[e - S / 2];
          if (c0 + 4 + e < W) v[S / 2 + 4 + e] = p[4 + e];
        }
      }
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        float s = 0.0f;
#pragma unroll
        for (int tx = 0; tx < 2 * S; ++tx) s = fmaf(wx[q][tx], v[S * q + tx], s);
        acc[q] = fmaf(wy[ty], s, acc[q]);
      }
    }
#pragma unroll
    for (int q = 0; q < Q; ++q)
      if (jq * Q + q < w) out[row * w + jq * Q + q] = acc[q];
  }
}

// ------------------------------------------------------------------------------------------------ 2. prediction head, backward
constexpr int kPhCT = 32;             // channels per workgroup: 8 lanes x 4
constexpr int kPhSlots = 32;          // pixel slots per workgroup (kGlueThreads / 8)
constexpr int kPhRangeMin = 256;      // at most one range per this many pixels (or part of them)
constexpr int kPhMaxRanges = 128;
constexpr int kPhTargetWGs = 1024;    // workgroups to aim for (256 CUs, two workgroups each, two rounds)
constexpr int kPhLdsBytes = kGlueThreads * 9 * 4 * 4;      // one output plane of every thread's partials: [thread][tap][4 channels]
static_assert(kPhSlots * 8 == kGlueThreads, "8 lanes per pixel slot");

struct PhPlan {
  int nct, nranges, RL;
};
// The ranges: as many as fill the GPU with the C / 32 channel tiles, at most one per kPhRangeMin pixels or part of them, at most
// kPhMaxRanges; RL pixels each (a multiple of the slots), the last one shorter.
inline PhPlan ph_plan(long long P, int C) {
  PhPlan p;
  p.nct = C / kPhCT;
  long long nr = kPhTargetWGs / p.nct;
  const long long by_len = (P + kPhRangeMin - 1) / kPhRangeMin;
  if (nr > by_len) nr = by_len;
  if (nr > kPhMaxRanges) nr = kPhMaxRanges;
  if (nr < 1) nr = 1;
  p.RL = (int)((((P + nr - 1) / nr) + kPhSlots - 1) / kPhSlots * kPhSlots);
  p.nranges = (int)((P + p.RL - 1) / p.RL);
  return p;
}
inline size_t ph_part_floats(int C) { return (size_t)18 * C + 2; }      // a range's partial: dw [2][C][3][3], then db [2]

struct PhArgs {
  const float* x;    // [P][C]
  const float* w;    // [2][C][9]
  const float* g;    // [n][2][Hq][Wq]
  float* dx;         // [P][C] or null
  float* part;       // [nranges][18 C + 2] or null
  int P, Hq, Wq, C, RL, want_dw;
};

extern __shared__ __attribute__((aligned(16))) float ph_lds[];      // kPhLdsBytes, sized at launch

__global__ __launch_bounds__(kGlueThreads) void pred_head_bwd(const PhArgs a) {
  const int tid = threadIdx.x, lane = tid & 7, slot = tid >> 3;
  const int ct = blockIdx.x, rg = blockIdx.y;
  const int p_begin = rg * a.RL;
  const int p_end = p_begin + a.RL < a.P ? p_begin + a.RL : a.P;
  const int c0 = ct * kPhCT + 4 * lane;
  const int HW = a.Hq * a.Wq;
  const bool want_dx = a.dx != nullptr, want_dw = a.want_dw != 0;

  // the lane's weights, wv[k][tap] = w[k][c0 .. c0 + 3][tap]
  f32x4 wv[2][9];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    float flat[36];
    if (want_dx) {
#pragma unroll
      for (int i = 0; i < 9; ++i) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(a.w + ((size_t)k * a.C + c0) * 9 + 4 * i);
#pragma unroll
        for (int e = 0; e < 4; ++e) flat[4 * i + e] = t[e];
      }
    } else {
#pragma unroll
      for (int i = 0; i < 36; ++i) flat[i] = 0.0f;
    }
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
      for (int e = 0; e < 4; ++e) wv[k][t][e] = flat[e * 9 + t];
  }

  f32x4 acc[2][9];
#pragma unroll
  for (int k = 0; k < 2; ++k)
#pragma unroll
    for (int t = 0; t < 9; ++t) acc[k][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  float accb[2] = {0.0f, 0.0f};

  int p = p_begin + slot;
  int img = p / HW;
  int y = (p - img * HW) / a.Wq;
  int x = p - img * HW - y * a.Wq;
  for (; p < p_end; p += kPhSlots) {
    f32x4 xv = {0.f, 0.f, 0.f, 0.f};
    if (want_dx || want_dw) xv = *reinterpret_cast<const f32x4*>(a.x + (size_t)p * a.C + c0);
    const float* gp = a.g + (size_t)img * 2 * HW + y * a.Wq + x;
    float G[2][9];
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const int yy = y + 1 - ky, xx = x + 1 - kx;
        const bool in = (unsigned)yy < (unsigned)a.Hq && (unsigned)xx < (unsigned)a.Wq;
        const int off = (1 - ky) * a.Wq + (1 - kx);
        G[0][ky * 3 + kx] = in ? gp[off] : 0.0f;
        G[1][ky * 3 + kx] = in ? gp[off + HW] : 0.0f;
      }
    if (want_dx) {
      f32x4 d = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int k = 0; k < 2; ++k)
#pragma unroll
        for (int t = 0; t < 9; ++t) d = __builtin_elementwise_fma(wv[k][t], f32x4{G[k][t], G[k][t], G[k][t], G[k][t]}, d);
#pragma unroll
      for (int e = 0; e < 4; ++e) d[e] = xv[e] > 0.0f ? d[e] : 0.0f;         // (NaN: 0, threshold_backward's rule)
      *reinterpret_cast<f32x4*>(a.dx + (size_t)p * a.C + c0) = d;
    }
    if (want_dw) {
      f32x4 r;
#pragma unroll
      for (int e = 0; e < 4; ++e) r[e] = xv[e] > 0.0f ? xv[e] : 0.0f;        // (NaN: 0)
#pragma unroll
      for (int k = 0; k < 2; ++k)
#pragma unroll
        for (int t = 0; t < 9; ++t) acc[k][t] = __builtin_elementwise_fma(r, f32x4{G[k][t], G[k][t], G[k][t], G[k][t]}, acc[k][t]);
    }
    accb[0] += G[0][4];
    accb[1] += G[1][4];
    // the slot's next pixel
    x += kPhSlots;
    while (x >= a.Wq) {
      x -= a.Wq;
      ++y;
    }
    while (y >= a.Hq) {
      y -= a.Hq;
      ++img;
    }
  }
  if (!a.part) return;

  // ---- the slots' partials, added in slot order
  float* const part = a.part + (size_t)rg * (18 * (size_t)a.C + 2);
  if (want_dw) {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      __syncthreads();               // (the plane before has been read)
#pragma unroll
      for (int t = 0; t < 9; ++t) *reinterpret_cast<f32x4*>(ph_lds + (tid * 9 + t) * 4) = acc[k][t];
      __syncthreads();
      for (int o = tid; o < kPhCT * 9; o += kGlueThreads) {          // o = (channel of the tile) * 9 + tap
        const int cl = o / 9, t = o - cl * 9;
        const float* src = ph_lds + ((cl >> 2) * 9 + t) * 4 + (cl & 3);
        float s = src[0];
        for (int sl = 1; sl < kPhSlots; ++sl) s += src[sl * 8 * 9 * 4];
        part[((size_t)k * a.C + ct * kPhCT) * 9 + o] = s;
      }
    }
  }
  if (ct == 0) {
    __syncthreads();
    if (lane == 0) {
      ph_lds[2 * slot] = accb[0];
      ph_lds[2 * slot + 1] = accb[1];
    }
    __syncthreads();
    if (tid < 2) {
      float s = ph_lds[tid];
      for (int sl = 1; sl < kPhSlots; ++sl) s += ph_lds[2 * sl + tid];
      part[18 * (size_t)a.C + tid] = s;
    }
  }
}

// dw / db = the ranges' partials added in range order
__global__ __launch_bounds__(kGlueThreads) void pred_head_bwd_merge(const float* part, float* dw, float* db, int nranges, int n_dw) {
  const int idx = blockIdx.x * kGlueThreads + threadIdx.x;
  if (idx >= n_dw + 2) return;
  const size_t stride = (size_t)n_dw + 2;
  float s = part[idx];
  for (int r = 1; r < nranges; ++r) s += part[r * stride + idx];
  if (idx < n_dw) {
    if (dw) dw[idx] = s;
  } else if (db) {
    db[idx - n_dw] = s;
  }
}

inline bool ph_shape_ok(int n, int Hq, int Wq, int C) { return n > 0 && Hq > 0 && Wq > 0 && C > 0; }
inline bool ph_supported(int n, int Hq, int Wq, int C) { return C % kPhCT == 0 && (long long)n * Hq * Wq * C < (1LL << 31); }
inline size_t ph_ws_bytes(long long P, int C) { return (size_t)ph_plan(P, C).nranges * ph_part_floats(C) * sizeof(float); }

}  // namespace
}  // namespace rmnet

using namespace rmnet;

extern "C" int rmnet_upsample_bwd_f32(const float* g, long long N, int C, int h, int w, int factor, int nhwc, float* out, void* stream) {
  if (!g || !out || N <= 0 || C <= 0 || h <= 0 || w <= 0) return RMNET_E_INVALID_ARG;
  if (factor != 2 && factor != 4) return RMNET_E_UNSUPPORTED;
  if ((reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(out)) & (nhwc ? 15 : 3)) return RMNET_E_INVALID_ARG;
  if (nhwc && C % 4) return RMNET_E_INVALID_ARG;
  // (checked in floating point first: the product of five ints may not fit 64 bits)
  if ((double)N * C * h * w * factor * factor >= 2147483648.0) return RMNET_E_UNSUPPORTED;
  const long long n_out = N * C * h * w, n_g = n_out * factor * factor;
  if (overlap(out, n_out * 4, g, n_g * 4)) return RMNET_E_INVALID_ARG;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (nhwc) {
    const long long items = n_out / 4;
    long long blocks = (items + kGlueThreads - 1) / kGlueThreads;
    if (blocks > kUpBlocks) blocks = kUpBlocks;
    if (factor == 2)
      hipLaunchKernelGGL(upsample_bwd_nhwc<2>, dim3((unsigned)blocks), dim3(kGlueThreads), 0, st, g, out, h, w, C / 4, items);
    else
      hipLaunchKernelGGL(upsample_bwd_nhwc<4>, dim3((unsigned)blocks), dim3(kGlueThreads), 0, st, g, out, h, w, C / 4, items);
    return check_launch();
  }
  const int Q = 4 / factor;
  const long long items = N * C * h * ((w + Q - 1) / Q);
  long long blocks = (items + kGlueThreads - 1) / kGlueThreads;
  if (blocks > kUpBlocks) blocks = kUpBlocks;
  // one 16-byte read per group of fine columns where every fine row starts on a 16-byte boundary
  const bool vec = !(reinterpret_cast<uintptr_t>(g) & 15) && (factor * w) % 4 == 0;
#define RMNET_UPB(S, V) hipLaunchKernelGGL((upsample_bwd_nchw<S, V>), dim3((unsigned)blocks), dim3(kGlueThreads), 0, st, g, out, h, w, items)
  if (factor == 2) {
    if (vec) RMNET_UPB(2, true); else RMNET_UPB(2, false);
  } else {
    if (vec) RMNET_UPB(4, true); else RMNET_UPB(4, false);
  }
#undef RMNET_UPB
  return check_launch();
}

extern "C" size_t rmnet_pred_head_bwd_workspace_bytes(int n, int Hq, int Wq, int C) {
  if (!ph_shape_ok(n, Hq, Wq, C) || !ph_supported(n, Hq, Wq, C)) return 0;
  return ph_ws_bytes((long long)n * Hq * Wq, C);
}

extern "C" int rmnet_pred_head_bwd_f32(const float* x, const float* w, const float* g, int n, int Hq, int Wq, int C, float* dx, float* dw,
                                       float* db, void* workspace, size_t workspace_bytes, void* stream) {
  if (!x || !w || !g || !ph_shape_ok(n, Hq, Wq, C)) return RMNET_E_INVALID_ARG;
  if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(w) | reinterpret_cast<uintptr_t>(dx) |
       reinterpret_cast<uintptr_t>(workspace)) & 15)
    return RMNET_E_INVALID_ARG;
  if ((reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(dw) | reinterpret_cast<uintptr_t>(db)) & 3) return RMNET_E_INVALID_ARG;
  if (!ph_supported(n, Hq, Wq, C)) return RMNET_E_UNSUPPORTED;
  const long long P = (long long)n * Hq * Wq;
  const long long n_dw = 18LL * C;
  const bool reduce = dw || db;
  const size_t need = reduce ? ph_ws_bytes(P, C) : 0;
  if (reduce && (!workspace || workspace_bytes < need)) return RMNET_E_WORKSPACE;
  // every output is written while other workgroups still read the inputs, and the outputs are distinct
  const void* ins[3] = {x, w, g};
  const long long in_bytes[3] = {P * C * 4, n_dw * 4, P * 2 * 4};
  const void* outs[4] = {dx, dw, db, reduce ? workspace : nullptr};
  const long long out_bytes[4] = {P * C * 4, n_dw * 4, 2 * 4, (long long)need};
  for (int i = 0; i < 4; ++i) {
    if (!outs[i]) continue;
    for (int j = 0; j < 3; ++j)
      if (overlap(outs[i], out_bytes[i], ins[j], in_bytes[j])) return RMNET_E_INVALID_ARG;
    for (int j = i + 1; j < 4; ++j)
      if (outs[j] && overlap(outs[i], out_bytes[i], outs[j], out_bytes[j])) return RMNET_E_INVALID_ARG;
  }
  if (!dx && !reduce) return RMNET_OK;       // nothing was asked for
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const PhPlan p = ph_plan(P, C);
  PhArgs a;
  a.x = x; a.w = w; a.g = g; a.dx = dx; a.part = reduce ? reinterpret_cast<float*>(workspace) : nullptr;
  a.P = (int)P; a.Hq = Hq; a.Wq = Wq; a.C = C; a.RL = p.RL; a.want_dw = dw != nullptr;
  hipLaunchKernelGGL(pred_head_bwd, dim3(p.nct, p.nranges), dim3(kGlueThreads), kPhLdsBytes, st, a);
  if (reduce)
    hipLaunchKernelGGL(pred_head_bwd_merge, dim3((unsigned)((n_dw + 2 + kGlueThreads - 1) / kGlueThreads)), dim3(kGlueThreads), 0, st,
                       a.part, dw, db, p.nranges, (int)n_dw);
  return check_launch();
}
