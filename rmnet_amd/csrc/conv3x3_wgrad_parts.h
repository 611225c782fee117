// conv3x3_wgrad_parts.h -- what the two weight-gradient files share (conv3x3_wgrad.hip: 256 output channels, the decoder's;
// conv_wgrad_n.hip: any multiple of 128, the key / value heads'): the constants, the range plan, the LDS budget, the transposed
// operand read, and the bodies of the three kernels (the GEMM over one pixel range, the bias chunk sum, the merge), written for an
// output-channel TILE of a gradient whose rows hold `cout` floats.  The decoder's kernels instantiate them with the constants
// (cout = 256, tile 0, 256 wide), which folds every tile test away; the layouts, the arithmetic and its order are described in
// conv3x3_wgrad.hip.
#pragma once

#include "split_f16.h"

namespace rmnet {
namespace {

constexpr int kWgCout = 256;       // output channels per workgroup (the last tile of a wider gradient may hold 128)
constexpr int kCT = 16;            // input channels per workgroup
constexpr int kSub = 512;          // pixels per x image
constexpr int kMaxW = 448;         // (kSub + 2 (W + 1) + 1 rows of 64 B next to the g buffers must fit 160 KB: 159936 B)
constexpr int kRangeMin = 256;     // fewest pixels worth a range of their own
constexpr int kMaxRanges = 64;
constexpr int kTargetWGs = 768;    // workgroups to aim for (256 CUs, one workgroup each, three rounds)
constexpr int kBiasSplit = 8;      // the bias kernels cut a range into that many chunks (RL is a multiple of 32)
constexpr int kGRow = kWgCout + 16;            // halves per pixel row of a g plane
constexpr int kGPlane = kKT * kGRow;           // halves
constexpr int kGBytes = 2 * 2 * kGPlane * 2;   // two buffers of hi + lo

struct WgradPlan {
  int nct, ncot, nranges, RL;
};
// The ranges: as many as fill the GPU with the Cin / 16 channel tiles of every output-channel tile, none shorter than kRangeMin, at
// most kMaxRanges; RL pixels each (a multiple of the K step), the last one shorter.
inline WgradPlan wgrad_plan(long long P, int Cin, int Cout = kWgCout) {
  WgradPlan p;
  p.nct = Cin / kCT;
  p.ncot = (Cout + kWgCout - 1) / kWgCout;
  long long nr = kTargetWGs / (p.nct * p.ncot);
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
inline size_t wgrad_ws_bytes(long long P, int Cin, int Cout = kWgCout) {
  const WgradPlan p = wgrad_plan(P, Cin, Cout);
  return (size_t)p.nranges * ((size_t)Cout * 9 * Cin + kBiasSplit * Cout) * sizeof(float);
}

struct WgradArgs {
  const float* x;   // [P][Cin]
  const float* g;   // [P][cout], staged
  float* part;      // [nranges][cout][9][Cin]
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

// One workgroup of the GEMM: channel tile blockIdx.x, pixel range blockIdx.y, the output channels co0 .. co0 + tw - 1 (tw = 256 or
// 128) of a gradient with `cout` floats a row.  A wave whose 32 channels lie past the tile takes part in the loads and reaches
// every barrier, but reads no operand, issues no MFMA and writes nothing.
__device__ __forceinline__ void wgrad_tile(const WgradArgs& a, _Float16* const lds, const int cout, const int co0, const int tw) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ct = blockIdx.x, rg = blockIdx.y;
  const int p_begin = rg * a.RL;
  const int p_end = p_begin + a.RL < a.P ? p_begin + a.RL : a.P;
  const int halo = a.W + 1;
  const int xrows = kSub + 2 * halo + 1;
  const int zero_row = xrows - 1;
  const bool live = 32 * wave < tw;
  _Float16* const gbuf = lds;
  _Float16* const xh = lds + 2 * 2 * kGPlane;
  _Float16* const xl = xh + xrows * kCT;

  f32x4 acc[2][9], accx[2][9];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int t = 0; t < 9; ++t) acc[j][t] = accx[j][t] = f32x4{0.f, 0.f, 0.f, 0.f};

  // the g loader: pixel tid / 16 of the step's 32, channels 4 (tid % 16) + 64 i of the tile
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
          // counted once: by the sub-range that owns the pixel, in the first output-channel tile
          split4(v, hi, lo, bad, pix >= s0 && pix < s1 && co0 == 0 ? 1 : 0);
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
        gr[i] = pix < s1 && 64 * i < tw ? *reinterpret_cast<const f32x4*>(a.g + (size_t)pix * cout + co0 + gc + 64 * i)
                                        : f32x4{0.f, 0.f, 0.f, 0.f};
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
      if (!live) continue;
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
  if (live) {
    float* const part = a.part + (size_t)rg * cout * 9 * a.Cin;
    const int ci = ct * kCT + (lane & 15);
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int co = co0 + 32 * wave + 16 * j + 4 * grp + e;
          part[((size_t)co * 9 + t) * a.Cin + ci] = acc[j][t][e] + accx[j][t][e];
        }
  }
  if (a.range) {
    bad = wave_sum(bad);
    if (lane == 0 && bad) atomicAdd(a.range, bad);
  }
}

// The sum of output channel co of g over chunk ch of range rg (RL / 8 pixels), pixel by pixel: a workgroup reads whole rows of its
// channels, the loads of a thread do not depend on each other, only its additions do.
__device__ __forceinline__ void wgrad_bias_chunk(const float* g, float* part_b, int P, int RL, int cout, int rg, int ch, int co) {
  const int CL = RL / kBiasSplit;
  const int p_begin = rg * RL + ch * CL;
  const int p_end = p_begin + CL < P ? p_begin + CL : P;
  float s = 0.0f;
#pragma unroll 8
  for (int p = p_begin; p < p_end; ++p) s += g[(size_t)p * cout + co];
  part_b[(rg * kBiasSplit + ch) * cout + co] = s;
}

// Element idx of dW / db = the partials added in range order, times 2^-12 (dW: the two operand scales) and the inverse of the staging
// scale's two factors: all exact.
__device__ __forceinline__ void wgrad_merge_element(const float* part, const float* part_b, const float* g_scale, float* dw, float* db,
                                                    int nranges, int n_dw, int cout, int idx) {
  const float ia = 1.0f / g_scale[0], ib = 1.0f / g_scale[1];
  if (idx < n_dw) {
    float s = part[idx];
    for (int r = 1; r < nranges; ++r) s += part[(size_t)r * n_dw + idx];
    dw[idx] = s * (kActUnscale * kActUnscale) * ia * ib;
  } else if (db && idx < n_dw + cout) {
    const int co = idx - n_dw;
    float s = part_b[co];
    for (int r = 1; r < nranges * kBiasSplit; ++r) s += part_b[r * cout + co];
    db[co] = s * ia * ib;
  }
}

inline bool wgrad_shape_ok(int N, int H, int W, int Cin) { return N > 0 && H > 0 && W > 0 && Cin > 0; }
inline bool wgrad_supported(int N, int H, int W, int Cin, int Cout = kWgCout) {
  const long long P = (long long)N * H * W;
  return Cin % kKT == 0 && W <= kMaxW && P * (long long)(Cin > Cout ? Cin : Cout) < (1LL << 31) && 9LL * Cin * Cout < (1LL << 31);
}

// The argument rules of the two weight-gradient entries, everything before the first launch: RMNET_OK or the code to return.
inline int wgrad_check_args(const float* x, const float* g, const float* g_scale, int flags, int N, int H, int W, int Cin, int Cout,
                            const float* dw, const float* db, const void* workspace, size_t workspace_bytes, const int32_t* range_word) {
  if (!x || !g || !g_scale || !dw || !wgrad_shape_ok(N, H, W, Cin)) return RMNET_E_INVALID_ARG;
  if (flags & ~RMNET_CONV_RELU_IN) return RMNET_E_INVALID_ARG;
  if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(g_scale) |
       reinterpret_cast<uintptr_t>(dw) | reinterpret_cast<uintptr_t>(db) | reinterpret_cast<uintptr_t>(workspace)) & 15)
    return RMNET_E_INVALID_ARG;
  if (reinterpret_cast<uintptr_t>(range_word) & 3) return RMNET_E_INVALID_ARG;
  if (!wgrad_supported(N, H, W, Cin, Cout)) return RMNET_E_UNSUPPORTED;
  const long long P = (long long)N * H * W;
  const long long n_dw = 9LL * Cin * Cout;
  // the outputs are written while other workgroups may still read x and g
  if (overlap(dw, n_dw * 4, x, P * Cin * 4) || overlap(dw, n_dw * 4, g, P * Cout * 4)) return RMNET_E_INVALID_ARG;
  if (db && (overlap(db, Cout * 4, x, P * Cin * 4) || overlap(db, Cout * 4, g, P * Cout * 4) || overlap(db, Cout * 4, dw, n_dw * 4)))
    return RMNET_E_INVALID_ARG;
  const size_t need = wgrad_ws_bytes(P, Cin, Cout);
  if (!workspace || workspace_bytes < need) return RMNET_E_WORKSPACE;
  if (overlap(workspace, (long long)need, x, P * Cin * 4) || overlap(workspace, (long long)need, g, P * Cout * 4) ||
      overlap(workspace, (long long)need, dw, n_dw * 4) || (db && overlap(workspace, (long long)need, db, Cout * 4)))
    return RMNET_E_INVALID_ARG;
  // (the merge reads g_scale while it writes dw and db; every workgroup may add to the range word)
  const void* outs[3] = {dw, db, workspace};
  const long long out_bytes[3] = {n_dw * 4, Cout * 4, (long long)need};
  for (int i = 0; i < 3; ++i) {
    if (!outs[i]) continue;
    if (overlap(outs[i], out_bytes[i], g_scale, 8) || (range_word && overlap(outs[i], out_bytes[i], range_word, 4))) return RMNET_E_INVALID_ARG;
  }
  return RMNET_OK;
}

// hipFuncAttributeMaxDynamicSharedMemorySize for a weight-gradient kernel, once per device and outside capture; `done` is the
// caller's per-device table (64 entries), guarded by the caller's mutex.
inline int wgrad_set_lds_attribute(const void* kernel, bool* done, hipStream_t st) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return RMNET_E_LAUNCH;
  if (done[dev]) return RMNET_OK;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(st, &cs) != hipSuccess) return RMNET_E_LAUNCH;
  if (cs != hipStreamCaptureStatusNone) return RMNET_E_UNSUPPORTED;
  if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)wgrad_lds_bytes(kMaxW)) != hipSuccess) return RMNET_E_LAUNCH;
  done[dev] = true;
  return RMNET_OK;
}

}  // namespace
}  // namespace rmnet
