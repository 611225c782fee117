// stem.hip -- the encoder stems in one launch: 7x7 / stride 2 / pad 3 convolution of the NCHW input planes (Cin = 3: frame; Cin = 5:
// frame, mask, other-objects mask), folded BatchNorm, ReLU and MaxPool2d(3, stride 2, padding 1), written channels-last:
//   out [N][Hp][Wp][64] = max_pool(relu(conv(x) * g + shift)),  Hc = (H - 1) / 2 + 1, Hp = (Hc - 1) / 2 + 1 (W alike).
// The half-resolution 64-channel activation (26 MB per 480p image) never leaves the CU, and the 5-channel torch.cat in front of the
// memory encoder's stem is not built: the kernel reads the three sources in place.
//
// Arithmetic: that of conv3x3.hip / conv_split.hip -- activations times 2^6 split into fp16 hi + lo (out-of-window elements
// saturated and counted), weights pre-split per output channel by the packer (rmnet_amd.ops.stem_pack, BatchNorm scale folded in),
// three product terms Ah*Wh + Ah*Wl + Al*Wh on v_mfma_f32_16x16x32_f16 in two fp32 accumulator sets.
//
// Tiling: a workgroup (512 threads, 8 waves) owns 8 x 8 pooled pixels = the 17 x 17 conv pixels they pool over = a 39 x 39 input
// patch, staged once in LDS as [row][col][ci] fp16 hi / lo planes.  GEMM view: M = 289 conv pixels (19 tiles of 16; wave w takes tiles
// w, w + 8, w + 16), N = 64 channels (4 tiles, all in every wave), K = (7 ky + kx) Cin + ci padded with zero weights to 160 / 256.  Inside
// one ky the K index runs along the patch row, so an activation fragment is 8 two-byte LDS reads at pixel base + off(k), off(k) =
// k + (k / 7 Cin) * (39 - 7) Cin.  The whole weight pack stays in LDS (40 / 64 KB) while the workgroup walks tiles blockIdx.x,
// + gridDim.x, ...; the next tile's patch is fetched into registers during the epilogue and the pool.  The conv tile (ReLU applied, -inf outside the map)
// goes to LDS over the patch, and the pool reads it from there.  Each input element is counted in the range word by the one
// workgroup whose 32 x 32 core holds it, so the halo is not counted twice.
// -Rpass-analysis=kernel-resource-usage: Cin 5: 208 VGPRs, 144,144 B of LDS; Cin 3: 202 VGPRs, 119,568 B; no spills, no scratch; one
// workgroup (two waves per SIMD) per CU, by LDS.  Measurements: profiles/r09_a_stem_head.md.
#include "split_f16.h"      // the vector types, kThreads, the activation scale, swz

namespace rmnet {
namespace {

constexpr int kCout = 64;
constexpr int kPT = 8;                     // pooled tile edge
constexpr int kCT = 2 * kPT + 1;           // conv tile edge (17)
constexpr int kPW = 2 * (kCT - 1) + 7;     // input patch edge (39)
constexpr int kCore = 4 * kPT;             // input pixels a tile owns per dimension (32), at patch offset 5
constexpr int kM = kCT * kCT;              // 289 conv pixels
constexpr int kMTiles = (kM + 15) / 16;    // 19
constexpr int kTI = 3;                     // M tiles per wave (8 waves x 3 >= 19)
constexpr int kCtStride = kCout + 4;       // conv tile row in LDS, padded: 16 pixel rows spread over the banks

struct StemArgs {
  const float* frame;      // [N][3][H][W]
  const float* mask;       // [N][H][W] or null
  const float* other;      // [N][H][W] or null
  const uint4* wp;         // [Kp / 32][2][64][32] fp16
  const float* unscale;    // [64]
  const float* shift;      // [64] or null
  float* out;              // [N][Hp][Wp][64]
  int* range;              // or null
  int N, H, W, Hc, Wc, Hp, Wp, TY, TX, tiles;
};

template <int CIN>
__global__ __launch_bounds__(kThreads) void stem_split(StemArgs a) {
  constexpr int KREAL = 49 * CIN;
  constexpr int KP = (KREAL + 31) / 32 * 32;           // 160 / 256
  constexpr int STEPS = KP / 32;
  constexpr int kWHalves = KP * kCout * 2;             // hi + lo planes of every step
  constexpr int kPatch = kPW * kPW * CIN;              // halves per plane
  constexpr int NP = (kPW * kPW + kThreads - 1) / kThreads;      // patch pixels per thread (3)
  constexpr int kRowSkip = (kPW - 7) * CIN;
  constexpr int kUnionBytes = kM * kCtStride * 4 > kPatch * 4 ? kM * kCtStride * 4 : kPatch * 4;
  static_assert(kWHalves * 2 + kUnionBytes <= kLdsBytesPerCU, "LDS budget");
  __shared__ __attribute__((aligned(16))) _Float16 wlds[kWHalves];
  __shared__ __attribute__((aligned(16))) unsigned char ulds[kUnionBytes];
  _Float16* ph = reinterpret_cast<_Float16*>(ulds);    // patch hi, lo: [row][col][ci]
  _Float16* pl = ph + kPatch;
  float* ct = reinterpret_cast<float*>(ulds);          // conv tile [289][kCtStride], after the MFMAs

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, fc = lane >> 4;

  // the weight pack, once per workgroup
  for (int q = tid; q < kWHalves / 8; q += kThreads) {
    const int sp = q >> 8, co = (q >> 2) & 63, ch = q & 3;
    *reinterpret_cast<uint4*>(wlds + sp * (kCout * 32) + swz(co, ch)) = a.wp[q];
  }

  // this lane's conv pixels: patch offset of tap (0, 0), channel 0
  int pbase[kTI];
#pragma unroll
  for (int i = 0; i < kTI; ++i) {
    int m = (wave + 8 * i) * 16 + fr;
    if (m >= kM) m = 0;
    const int cy = m / kCT, cx = m - cy * kCT;
    pbase[i] = (2 * cy * kPW + 2 * cx) * CIN;
  }

  // loader items: patch pixel rc = tid + 512 i (i < 3), every channel of it
  float xr[NP][CIN];
  auto load = [&](int tile) {
    const int n = tile / (a.TY * a.TX), r = tile - n * (a.TY * a.TX);
    const int ty = r / a.TX, tx = r - ty * a.TX;
    const int iy0 = kCore * ty - 5, ix0 = kCore * tx - 5;
    const size_t plane = (size_t)a.H * a.W;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const int rc = tid + kThreads * i;
      const int py = rc / kPW, px = rc - py * kPW;
      const int iy = iy0 + py, ix = ix0 + px;
      const bool in = rc < kPW * kPW && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
      const size_t pix = (size_t)iy * a.W + ix;
#pragma unroll
      for (int c = 0; c < CIN; ++c) {
        float v = 0.0f;
        if (in) {
          if (c < 3)
            v = a.frame[((size_t)n * 3 + c) * plane + pix];
          else if (c == 3)
            v = a.mask[(size_t)n * plane + pix];
          else if (a.other)
            v = a.other[(size_t)n * plane + pix];
        }
        xr[i][c] = v;
      }
    }
  };

  int bad = 0;
  auto store = [&]() {
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const int rc = tid + kThreads * i;
      if (rc >= kPW * kPW) continue;
      const int py = rc / kPW, px = rc - py * kPW;
      const bool core = (unsigned)(py - 5) < (unsigned)kCore && (unsigned)(px - 5) < (unsigned)kCore;
#pragma unroll
      for (int c = 0; c < CIN; ++c) {
        const float y = xr[i][c] * kActScale;
        bad += (core && !(fabsf(y) <= kF16Max)) ? 1 : 0;      // (outside the map: zeros, which pass)
        const float s = fminf(fmaxf(y, -kF16Max), kF16Max);
        const _Float16 h = (_Float16)s;
        ph[rc * CIN + c] = h;
        pl[rc * CIN + c] = (_Float16)(s - (float)h);
      }
    }
  };

  int tile = blockIdx.x;
  if (tile < a.tiles) load(tile);
  for (; tile < a.tiles; tile += gridDim.x) {
    __syncthreads();                      // (the pool of the tile before is done with ct; first pass: nothing)
    store();
    __syncthreads();

    f32x4 acc[kTI][4], accx[kTI][4];
#pragma unroll
    for (int i = 0; i < kTI; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = accx[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

#pragma unroll 1
    for (int s = 0; s < STEPS; ++s) {
      half8 ah[4], al[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int o = swz(j * 16 + fr, fc);
        ah[j] = *reinterpret_cast<const half8*>(wlds + (2 * s) * (kCout * 32) + o);
        al[j] = *reinterpret_cast<const half8*>(wlds + (2 * s + 1) * (kCout * 32) + o);
      }
      int off[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        int k = 32 * s + 8 * fc + e;
        k = k < KREAL ? k : 0;            // (zero weights there: any finite activation will do)
        off[e] = k + (k / (7 * CIN)) * kRowSkip;
      }
#pragma unroll
      for (int i = 0; i < kTI; ++i) {
        if ((wave + 8 * i) * 16 >= kM) continue;            // (wave-uniform: waves 3..7 have two tiles)
        half8 bh, bl;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          bh[e] = ph[pbase[i] + off[e]];
          bl[e] = pl[pbase[i] + off[e]];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[j], bh, acc[i][j], 0, 0, 0);
#pragma unroll
        for (int j = 0; j < 4; ++j) accx[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[j], bl, accx[i][j], 0, 0, 0);
#pragma unroll
        for (int j = 0; j < 4; ++j) accx[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[j], bh, accx[i][j], 0, 0, 0);
      }
    }
    __syncthreads();                      // every wave is done with the patch: ct takes its place
    const int next = tile + gridDim.x;
    if (next < a.tiles) load(next);       // (in flight during the epilogue and the pool; the weight fragments' registers are free now)

    const int n = tile / (a.TY * a.TX), r = tile - n * (a.TY * a.TX);
    const int ty = r / a.TX, tx = r - ty * a.TX;
    // D[co][px]: lane holds pixel fr of each M tile and channels 4 fc .. 4 fc + 3 of each 16-channel tile
#pragma unroll
    for (int i = 0; i < kTI; ++i) {
      const int m = (wave + 8 * i) * 16 + fr;
      if (m >= kM) continue;
      const int cy = m / kCT, cx = m - cy * kCT;
      const int gy = 2 * kPT * ty - 1 + cy, gx = 2 * kPT * tx - 1 + cx;
      const bool in = (unsigned)gy < (unsigned)a.Hc && (unsigned)gx < (unsigned)a.Wc;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int co = j * 16 + 4 * fc;
        const f32x4 us = *reinterpret_cast<const f32x4*>(a.unscale + co) * kActUnscale;
        const f32x4 b = a.shift ? *reinterpret_cast<const f32x4*>(a.shift + co) : f32x4{0.f, 0.f, 0.f, 0.f};
        f32x4 v = (acc[i][j] + accx[i][j]) * us + b;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = in ? (v[e] < 0.0f ? 0.0f : v[e]) : -INFINITY;      // (ReLU keeps NaN)
        *reinterpret_cast<f32x4*>(ct + m * kCtStride + co) = v;
      }
    }
    __syncthreads();

    // pool: one thread = 4 channels of one pooled pixel
    for (int it = tid; it < kPT * kPT * (kCout / 4); it += kThreads) {
      const int c4 = it & 15, pp = it >> 4;
      const int py = pp / kPT, px = pp - py * kPT;
      const int gy = kPT * ty + py, gx = kPT * tx + px;
      if (gy >= a.Hp || gx >= a.Wp) continue;
      f32x4 best = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
      bool nan[4] = {false, false, false, false};
#pragma unroll
      for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
          const f32x4 v = *reinterpret_cast<const f32x4*>(ct + ((2 * py + dy) * kCT + 2 * px + dx) * kCtStride + 4 * c4);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            nan[e] = nan[e] || v[e] != v[e];
            best[e] = v[e] > best[e] ? v[e] : best[e];
          }
        }
      const float qn = __builtin_nanf("");
#pragma unroll
      for (int e = 0; e < 4; ++e) best[e] = nan[e] ? qn : best[e];
      *reinterpret_cast<f32x4*>(a.out + (((size_t)n * a.Hp + gy) * a.Wp + gx) * kCout + 4 * c4) = best;
    }
  }
  if (a.range && bad) atomicAdd(a.range, bad);
}

}  // namespace
}  // namespace rmnet

extern "C" int rmnet_stem_split_f32(const float* frame, const float* mask, const float* other, const void* wpack,
                                    const float* w_unscale, const float* shift, int N, int H, int W, float* out,
                                    int32_t* range_word, void* stream) {
  using namespace rmnet;
  if (!frame || !wpack || !w_unscale || !out || N <= 0 || H <= 0 || W <= 0) return RMNET_E_INVALID_ARG;
  if (other && !mask) return RMNET_E_INVALID_ARG;
  if ((reinterpret_cast<uintptr_t>(wpack) | reinterpret_cast<uintptr_t>(w_unscale) | reinterpret_cast<uintptr_t>(shift) |
       reinterpret_cast<uintptr_t>(out)) & 15)
    return RMNET_E_INVALID_ARG;
  if ((reinterpret_cast<uintptr_t>(frame) | reinterpret_cast<uintptr_t>(mask) | reinterpret_cast<uintptr_t>(other)) & 3)
    return RMNET_E_INVALID_ARG;
  StemArgs a;
  a.Hc = (H - 1) / 2 + 1; a.Wc = (W - 1) / 2 + 1;
  a.Hp = (a.Hc - 1) / 2 + 1; a.Wp = (a.Wc - 1) / 2 + 1;
  a.TY = (a.Hp + kPT - 1) / kPT; a.TX = (a.Wp + kPT - 1) / kPT;
  const long long tiles = (long long)N * a.TY * a.TX;
  if ((long long)N * 3 * H * W >= (1LL << 31) || (long long)N * a.Hp * a.Wp * kCout >= (1LL << 31) || tiles >= (1LL << 31))
    return RMNET_E_UNSUPPORTED;
  a.frame = frame; a.mask = mask; a.other = other; a.wp = reinterpret_cast<const uint4*>(wpack); a.unscale = w_unscale;
  a.shift = shift; a.out = out; a.range = range_word; a.N = N; a.H = H; a.W = W; a.tiles = (int)tiles;
  // persistent workgroups, one per CU at a time (LDS): two per CU in all, so that a CU that finishes early takes another share
  const unsigned grid = (unsigned)(tiles < 2 * kNumCUs ? tiles : 2 * kNumCUs);
  hipStream_t st = (hipStream_t)stream;
  if (mask)
    hipLaunchKernelGGL(stem_split<5>, dim3(grid), dim3(kThreads), 0, st, a);
  else
    hipLaunchKernelGGL(stem_split<3>, dim3(grid), dim3(kThreads), 0, st, a);
  return check_launch();
}
