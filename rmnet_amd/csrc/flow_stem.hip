// flow_stem.hip -- TinyFlowNet's front end in one launch: zero-padding of the two frames to the padded size, the bilinear halving
// (a 2x2 mean), the 6-channel concatenation, conv1 (7x7 / stride 2 / pad 3, 6 -> 64), bias and LeakyReLU(0.1), written channels-last:
//   c1 [N][Hc][Wc][64] = leaky(conv(pair) + bias),  Hh = Hpad / 2, Hc = (Hh - 1) / 2 + 1 (W alike),
//   pair[n][c][Y][X]   = mean of the padded frame (img0 for c < 3, img1 behind it) over rows 2Y, 2Y + 1 and columns 2X, 2X + 1,
//   padded frame       = the NCHW frame shifted by (lh, lw), zeros outside it.
// Neither the padded frames nor the half-resolution pair is ever written: the kernel reads img0 and img1 in place, frame n at a
// batch stride of the caller's (frame t of a [N][T][3][H][W] clip needs no copy).
//
// Arithmetic: stem.hip's, term for term -- pair times 2^6, saturated at +-65504 (out-of-window elements counted), split into fp16
// hi + lo; weights pre-split per output channel by the packer (rmnet_amd.ops.flow_stem_pack: stem_pack's layout with Cin 6, K = 294
// padded to 320); Ah*Wh + Ah*Wl + Al*Wh on v_mfma_f32_16x16x32_f16 in two fp32 accumulator sets.
//
// Tiling: there is no pool, so a workgroup (512 threads, 8 waves) owns 16 x 16 conv pixels = a 37 x 37 patch of the pair, staged once
// in LDS as [row][col][ci] fp16 hi / lo planes.  GEMM view: M = 256 conv pixels = 16 tiles, one conv row each (wave w takes rows w and
// w + 8: no idle slot), N = 64 channels (4 tiles, all in every wave), K = (7 ky + kx) 6 + ci in 10 steps of 32.  Inside one ky the K
// index runs along the patch row, so an activation fragment is 4 four-byte LDS reads (a ky row is 42 halves: no even pair straddles two) at pixel base + off(k),
// off(k) = k + (k / 42) * (37 - 7) * 6.  The weight pack stays in LDS (80 KB) while the workgroup walks tiles blockIdx.x, + gridDim.x, ...; the next tile's
// patch is fetched into registers (72 per thread: the 2x2 blocks are added up only when they are staged, so the loads stay in
// flight under the MFMAs of this tile).  The epilogue stores a lane's four
// channels as one 16-byte store, straight from the accumulators.  Each pair element is counted in the range word by the one
// workgroup whose 32 x 32 core (patch offset 3) holds it.
// LDS: 81,920 B of pack + 32,856 B of patch planes + 512 B of epilogue constants (unscale / 64, bias) = 115,296 B, dynamic (prepared once per device: rows_prepare): one workgroup
// (two waves per SIMD) per CU.  Measurements: profiles/r23_a_front_ends.md.
#include "conv_rows_core.h"      // rows_prepare; and through it split_f16.h: the vector types, kThreads, the activation scale, swz

namespace rmnet {
namespace {

typedef _Float16 half2 __attribute__((ext_vector_type(2)));

constexpr int kCout = 64;
constexpr int kCin = 6;
constexpr int kCT = 16;                    // conv tile edge
constexpr int kPW = 2 * (kCT - 1) + 7;     // patch edge (37)
constexpr int kCore = 2 * kCT;             // pair pixels a tile owns per dimension (32), at patch offset 3
constexpr int kTI = 2;                     // M tiles (conv rows) per wave
constexpr int kKReal = 49 * kCin;          // 294
constexpr int kKP = (kKReal + 31) / 32 * 32;          // 320
constexpr int kSteps = kKP / 32;
constexpr int kWHalves = kKP * kCout * 2;  // hi + lo planes of every step
constexpr int kPatch = kPW * kPW * kCin;   // halves per plane
constexpr int kNP = (kPW * kPW + kThreads - 1) / kThreads;      // patch pixels per thread (3)
constexpr int kRowSkip = (kPW - 7) * kCin;
constexpr int kEpOffset = (kWHalves * 2 + kPatch * 4 + 15) / 16 * 16;      // the epilogue's unscale / 64 and bias, [2][64] floats
constexpr int kFlowStemLdsBytes = kEpOffset + 2 * kCout * 4;
static_assert(kFlowStemLdsBytes <= kLdsBytesPerCU, "LDS budget");
static_assert((7 * kCin) % 2 == 0 && kKReal % 2 == 0 && kPatch % 2 == 0, "pairs of halves stay inside a ky row and 4-byte aligned");
static_assert(kTI * 8 == kCT && kThreads == 512, "eight waves, two conv rows each");
// (the furthest LDS read: the last conv pixel's base + off(kKReal - 1) is the patch's last element)
static_assert((2 * (kCT - 1) * kPW + 2 * (kCT - 1)) * kCin + (kKReal - 1) + 6 * kRowSkip == kPatch - 1, "patch extent");

extern __shared__ __attribute__((aligned(16))) _Float16 fs_lds[];      // kFlowStemLdsBytes, sized at launch

struct FlowStemArgs {
  const float* img0;       // [N][3][H][W], frame n at img0 + n * bs0
  const float* img1;       // [N][3][H][W], frame n at img1 + n * bs1
  long long bs0, bs1;
  const uint4* wp;         // [10][2][64][32] fp16
  const float* unscale;    // [64]
  const float* bias;       // [64] or null
  float* out;              // [N][Hc][Wc][64]
  int* range;              // or null
  int N, H, W, lh, lw, Hh, Wh, Hc, Wc, TY, TX, tiles;
};

__global__ __launch_bounds__(kThreads) void flow_stem(FlowStemArgs a) {
  _Float16* wlds = fs_lds;
  _Float16* ph = fs_lds + kWHalves;      // patch hi, lo: [row][col][ci]
  _Float16* pl = ph + kPatch;
  float* ep = reinterpret_cast<float*>(reinterpret_cast<unsigned char*>(fs_lds) + kEpOffset);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, fc = lane >> 4;

  // the weight pack and the epilogue's constants, once per workgroup (the first barrier of the tile loop publishes them)
  if (tid < kCout) {
    ep[tid] = a.unscale[tid] * kActUnscale;
    ep[kCout + tid] = a.bias ? a.bias[tid] : 0.0f;
  }
  for (int q = tid; q < kWHalves / 8; q += kThreads) {
    const int sp = q >> 8, co = (q >> 2) & 63, ch = q & 3;
    *reinterpret_cast<uint4*>(wlds + sp * (kCout * 32) + swz(co, ch)) = a.wp[q];
  }

  // this lane's conv pixels (row wave + 8 i, column fr): patch offset of tap (0, 0), channel 0
  int pbase[kTI];
#pragma unroll
  for (int i = 0; i < kTI; ++i) pbase[i] = (2 * (wave + 8 * i) * kPW + 2 * fr) * kCin;

  // loader items: patch pixel rc = tid + 512 i (i < 3), every channel of it: the 2x2 block of the padded frame.  The four values
  // stay apart until store() adds them, so that nothing waits for the loads before the MFMAs of the tile in between are issued.
  float xr[kNP][kCin][4];
  auto load = [&](int tile) {
    const int n = tile / (a.TY * a.TX), r = tile - n * (a.TY * a.TX);
    const int ty = r / a.TX, tx = r - ty * a.TX;
    const int y0 = kCore * ty - 3, x0 = kCore * tx - 3;
    const size_t plane = (size_t)a.H * a.W;
#pragma unroll
    for (int i = 0; i < kNP; ++i) {
      const int rc = tid + kThreads * i;
      const int py = rc / kPW, px = rc - py * kPW;
      const int y = y0 + py, x = x0 + px;
      const bool in = rc < kPW * kPW && (unsigned)y < (unsigned)a.Hh && (unsigned)x < (unsigned)a.Wh;
      const int iy = 2 * y - a.lh, ix = 2 * x - a.lw;       // the frame's element under the block's first corner
      const bool r0 = in && (unsigned)iy < (unsigned)a.H, r1 = in && (unsigned)(iy + 1) < (unsigned)a.H;
      const bool c0 = (unsigned)ix < (unsigned)a.W, c1 = (unsigned)(ix + 1) < (unsigned)a.W;
      const size_t pix = (size_t)iy * a.W + ix;             // (dereferenced under the four flags only)
#pragma unroll
      for (int c = 0; c < kCin; ++c) {
        const float* p = (c < 3 ? a.img0 + (size_t)n * a.bs0 : a.img1 + (size_t)n * a.bs1) + (c % 3) * plane + pix;
        xr[i][c][0] = r0 && c0 ? p[0] : 0.0f;
        xr[i][c][1] = r0 && c1 ? p[1] : 0.0f;
        xr[i][c][2] = r1 && c0 ? p[a.W] : 0.0f;
        xr[i][c][3] = r1 && c1 ? p[a.W + 1] : 0.0f;
      }
    }
  };

  int bad = 0;
  auto store = [&]() {
#pragma unroll
    for (int i = 0; i < kNP; ++i) {
      const int rc = tid + kThreads * i;
      if (rc >= kPW * kPW) continue;
      const int py = rc / kPW, px = rc - py * kPW;
      const bool core = (unsigned)(py - 3) < (unsigned)kCore && (unsigned)(px - 3) < (unsigned)kCore;
#pragma unroll
      for (int c = 0; c < kCin; ++c) {
        const float y = 0.25f * ((xr[i][c][0] + xr[i][c][1]) + (xr[i][c][2] + xr[i][c][3])) * kActScale;
        bad += (core && !(fabsf(y) <= kF16Max)) ? 1 : 0;      // (outside the map: zeros, which pass)
        const float s = fminf(fmaxf(y, -kF16Max), kF16Max);
        const _Float16 h = (_Float16)s;
        ph[rc * kCin + c] = h;
        pl[rc * kCin + c] = (_Float16)(s - (float)h);
      }
    }
  };

  int tile = blockIdx.x;
  if (tile < a.tiles) load(tile);
  for (; tile < a.tiles; tile += gridDim.x) {
    __syncthreads();                      // (every wave is done with the patch of the tile before; first pass: nothing)
    store();
    __syncthreads();
    const int next = tile + gridDim.x;
    if (next < a.tiles) load(next);       // (in flight under the MFMAs)

    f32x4 acc[kTI][4], accx[kTI][4];
#pragma unroll
    for (int i = 0; i < kTI; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = accx[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

#pragma unroll 1
    for (int s = 0; s < kSteps; ++s) {
      half8 ah[4], al[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int o = swz(j * 16 + fr, fc);
        ah[j] = *reinterpret_cast<const half8*>(wlds + (2 * s) * (kCout * 32) + o);
        al[j] = *reinterpret_cast<const half8*>(wlds + (2 * s + 1) * (kCout * 32) + o);
      }
      // (a ky row is 42 halves, so no pair k, k + 1 with k even straddles two patch rows: four 4-byte reads per plane)
      int off[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        int k = 32 * s + 8 * fc + 2 * e;
        k = k < kKReal ? k : 0;           // (zero weights there: any finite activation will do)
        off[e] = k + (k / (7 * kCin)) * kRowSkip;
      }
#pragma unroll
      for (int i = 0; i < kTI; ++i) {
        half8 bh, bl;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const half2 h = *reinterpret_cast<const half2*>(ph + pbase[i] + off[e]);
          const half2 l = *reinterpret_cast<const half2*>(pl + pbase[i] + off[e]);
          bh[2 * e] = h[0]; bh[2 * e + 1] = h[1];
          bl[2 * e] = l[0]; bl[2 * e + 1] = l[1];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[j], bh, acc[i][j], 0, 0, 0);
#pragma unroll
        for (int j = 0; j < 4; ++j) accx[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[j], bl, accx[i][j], 0, 0, 0);
#pragma unroll
        for (int j = 0; j < 4; ++j) accx[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[j], bh, accx[i][j], 0, 0, 0);
      }
    }

    // D[co][px]: lane holds pixel fr of each conv row and channels 4 fc .. 4 fc + 3 of each 16-channel tile
    const int n = tile / (a.TY * a.TX), r = tile - n * (a.TY * a.TX);
    const int ty = r / a.TX, tx = r - ty * a.TX;
    const int gx = kCT * tx + fr;
#pragma unroll
    for (int i = 0; i < kTI; ++i) {
      const int gy = kCT * ty + wave + 8 * i;
      if (gy >= a.Hc || gx >= a.Wc) continue;
      float* o = a.out + (((size_t)n * a.Hc + gy) * a.Wc + gx) * kCout;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int co = j * 16 + 4 * fc;
        const f32x4 us = *reinterpret_cast<const f32x4*>(ep + co);
        const f32x4 b = *reinterpret_cast<const f32x4*>(ep + kCout + co);
        f32x4 v = (acc[i][j] + accx[i][j]) * us + b;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = v[e] > 0.0f ? v[e] : v[e] * 0.1f;      // (LeakyReLU keeps NaN)
        *reinterpret_cast<f32x4*>(o + co) = v;
      }
    }
  }
  if (a.range && bad) atomicAdd(a.range, bad);
}

}  // namespace
}  // namespace rmnet

extern "C" int rmnet_flow_stem_f32(const float* img0, const float* img1, long long batch_stride0, long long batch_stride1,
                                   const void* wpack, const float* w_unscale, const float* bias, int N, int H, int W, int Hpad, int Wpad, int lh, int lw, float* out, int32_t* range_word,
                                   void* stream) {
  using namespace rmnet;
  if (!img0 || !img1 || !wpack || !w_unscale || !out || N <= 0 || H <= 0 || W <= 0 || Hpad <= 0 || Wpad <= 0) return RMNET_E_INVALID_ARG;
  if (lh < 0 || lw < 0 || (long long)lh + H > Hpad || (long long)lw + W > Wpad) return RMNET_E_INVALID_ARG;
  if ((reinterpret_cast<uintptr_t>(wpack) | reinterpret_cast<uintptr_t>(w_unscale) | reinterpret_cast<uintptr_t>(bias) |
       reinterpret_cast<uintptr_t>(out)) & 15)
    return RMNET_E_INVALID_ARG;
  if ((reinterpret_cast<uintptr_t>(img0) | reinterpret_cast<uintptr_t>(img1)) & 3) return RMNET_E_INVALID_ARG;
  if ((Hpad | Wpad) & 1) return RMNET_E_UNSUPPORTED;          // (the halving is a 2x2 mean for even padded sizes only)
  FlowStemArgs a;
  a.Hh = Hpad / 2; a.Wh = Wpad / 2;
  a.Hc = (a.Hh - 1) / 2 + 1; a.Wc = (a.Wh - 1) / 2 + 1;
  a.TY = (a.Hc + kCT - 1) / kCT; a.TX = (a.Wc + kCT - 1) / kCT;
  const long long tiles = (long long)N * a.TY * a.TX;
  const long long frame = 3LL * H * W, in_elems = (long long)N * frame, out_elems = (long long)N * a.Hc * a.Wc * kCout;
  if (batch_stride0 < frame || batch_stride1 < frame) return RMNET_E_INVALID_ARG;
  const long long span0 = (N - 1) * batch_stride0 + frame, span1 = (N - 1) * batch_stride1 + frame;
  if (in_elems >= (1LL << 31) || out_elems >= (1LL << 31) || tiles >= (1LL << 31)) return RMNET_E_UNSUPPORTED;
  if (overlap(out, out_elems * 4, img0, span0 * 4) || overlap(out, out_elems * 4, img1, span1 * 4)) return RMNET_E_INVALID_ARG;
  hipStream_t st = (hipStream_t)stream;
  const int rc = rows_prepare<flow_stem, kFlowStemLdsBytes>(st);
  if (rc != RMNET_OK) return rc;
  a.img0 = img0; a.img1 = img1; a.bs0 = batch_stride0; a.bs1 = batch_stride1; a.wp = reinterpret_cast<const uint4*>(wpack); a.unscale = w_unscale; a.bias = bias; a.out = out;
  a.range = range_word; a.N = N; a.H = H; a.W = W; a.lh = lh; a.lw = lw; a.tiles = (int)tiles;
  // persistent workgroups, one per CU at a time (LDS): two per CU in all, so that a CU that finishes early takes another share
  const unsigned grid = (unsigned)(tiles < 2 * kNumCUs ? tiles : 2 * kNumCUs);
  hipLaunchKernelGGL(flow_stem, dim3(grid), dim3(kThreads), kFlowStemLdsBytes, st, a);
  return check_launch();
}
