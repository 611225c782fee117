// late_objects.hip -- objects that are first annotated in the middle of a clip (the YouTube-VOS protocol): which ids a frame's label
// map holds, and the logit edits of models/rmnet.py:436-450 with the soft-max that follows them (include/rmnet_hip.h I1):
//
//   lo_presence   labels [N,H,W] u8 -> presence [N,8] u32, bit v & 31 of word v >> 5 of row n set exactly when byte value v occurs in
//                 frame n: what np.unique of every frame is needed for (utils/data_loaders.py:58-65, models/rmnet.py:400, 438)
//   lo_edit       per pixel and channel k of one frame: keep the logit, pin it to the absent logit -16.1181, or inject
//                 fl(fl(m * 32.0605f) - 16.1181f) with m = (lut[label] == k); then the soft-max over the K channels, written through
//                 a batch stride so that it lands in est[:, t]
//
// and the same two for a clip that runs at another scale, possibly mirrored (multi_scale_inference, utils/helpers.py:44-78;
// include/rmnet_hip.h I2), with the nearest-neighbour rule  src(d) = min((int)floorf((float)d * scale), in - 1)  per axis:
//
//   lo_presence_nearest   labels [N,Hs,Ws] u8 + S scales -> presence [S,N,8] u32: the ids that the nearest-resized map of every scale
//                         would hold, without writing a resized map
//   lo_edit_nearest       lo_edit with the label read at the sampled (and, per batch slot, mirrored) position of a full-size map
//
// Presence: a frame's bytes are cut into a head of up to 15 bytes in front of the first 16-byte boundary, 16-byte vectors and a
// tail of up to 15 bytes, so a label map at any address is read with dwordx4 loads in the body.  A lane keeps the 256-bit set in
// four 64-bit registers picked by compares (a dynamically indexed array would go to scratch), skips a byte that repeats its
// predecessor (label maps are long runs), and the wave's sets are OR-ed with DPP row operations and the permlane swaps: no LDS.
// One lane per wave then issues an atomicOr per non-zero word.  OR commutes and is idempotent: the same bits in any order.
//
// The injection must round its product and its difference separately, as torch does; hipcc contracts a * b + c into one fused
// operation in device code unless told otherwise, hence the pragma.
#include "common.h"

#pragma clang fp contract(off)

namespace rmnet {
namespace {

constexpr int kThreads = 256;
constexpr int kIter = 4;                                   // 16-byte vectors per lane
constexpr int kChunk = kThreads * kIter * 16;              // bytes of a frame's body per workgroup (launch_label_presence's chunk)
constexpr float kNewObjectScale = 32.0605f, kNewObjectShift = 16.1181f;      // models/rmnet.py:442
constexpr float kAbsentLogit = -kNewObjectShift;                              // models/rmnet.py:448

struct Set256 { unsigned long long w0, w1, w2, w3; };

__device__ inline void set_add(Set256& s, unsigned v) {
  const unsigned long long bit = 1ull << (v & 63u);
  const unsigned sel = v >> 6;
  s.w0 |= sel == 0u ? bit : 0ull;
  s.w1 |= sel == 1u ? bit : 0ull;
  s.w2 |= sel == 2u ? bit : 0ull;
  s.w3 |= sel == 3u ? bit : 0ull;
}

// every lane gets the OR over the 64 lanes (the steps of wave_max_fast, common.h)
__device__ inline unsigned wave_or(unsigned u) {
  int v = (int)u;
  v |= RMNET_DPP(v, v, 0xB1, 0xf, 0xf, false);
  v |= RMNET_DPP(v, v, 0x4E, 0xf, 0xf, false);
  v |= RMNET_DPP(v, v, 0x141, 0xf, 0xf, false);
  v |= RMNET_DPP(v, v, 0x140, 0xf, 0xf, false);
  auto r = __builtin_amdgcn_permlane16_swap((unsigned)v, (unsigned)v, false, false);
  const unsigned h = r[0] | r[1];
  r = __builtin_amdgcn_permlane32_swap(h, h, false, false);
  return r[0] | r[1];
}

// ------------------------------------------------------------------------------------------------ presence
// grid: N * bpf workgroups, frame = blockIdx.x / bpf.  Workgroup j of a frame takes the vectors [j * kThreads * kIter, ...) of the
// frame's body, lane l of it the vectors l, l + kThreads, ...; workgroup 0 also takes the head and the tail, a byte per lane.  No
// lane leaves before the reduction: the cross-lane steps read every lane of the wave.
__global__ __launch_bounds__(kThreads) void lo_presence(const uint8_t* __restrict__ labels, uint32_t* __restrict__ presence, long long HW,
                                                        unsigned bpf) {
  const long long n = blockIdx.x / bpf;
  const unsigned j = blockIdx.x % bpf;
  const uint8_t* frame = labels + n * HW;
  const long long to_boundary = (long long)((16u - (unsigned)(reinterpret_cast<uintptr_t>(frame) & 15u)) & 15u);
  const long long head = to_boundary < HW ? to_boundary : HW;
  const long long nvec = (HW - head) >> 4;
  const long long tail0 = head + (nvec << 4);
  Set256 s = {0ull, 0ull, 0ull, 0ull};
  const uint4* body = reinterpret_cast<const uint4*>(frame + head);
  const long long v0 = (long long)j * (kThreads * kIter) + threadIdx.x;
#pragma unroll
  for (int it = 0; it < kIter; ++it) {
    const long long v = v0 + (long long)it * kThreads;
    if (v < nvec) {
      const uint4 q = body[v];
      const uint32_t ws[4] = {q.x, q.y, q.z, q.w};
      unsigned prev = 256u;                                // no byte
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const unsigned b = (ws[i >> 2] >> (8 * (i & 3))) & 255u;
        if (b != prev) set_add(s, b);
        prev = b;
      }
    }
  }
  if (j == 0) {
    if ((long long)threadIdx.x < head) set_add(s, frame[threadIdx.x]);
    if (tail0 + threadIdx.x < HW) set_add(s, frame[tail0 + threadIdx.x]);
  }
  const unsigned long long w[4] = {s.w0, s.w1, s.w2, s.w3};
  uint32_t* row = presence + n * 8;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const unsigned word = wave_or((unsigned)(w[i >> 1] >> (32 * (i & 1))));
    if ((threadIdx.x & (RMNET_WAVE - 1)) == 0 && word != 0u) atomicOr(row + i, word);
  }
}

// ------------------------------------------------------------------------------------------------ nearest-resized presence
// The source index of output index d on an axis of `in` elements: torch's legacy 'nearest' rule with scale = (float)(1.0 / factor).
// d and in are at most 2^24, so (float)d and (float)(in - 1) are exact; the minimum is taken before the conversion, so a product
// beyond the int range is clamped like any other.  The result is in 0 .. in - 1 for every finite positive scale.
__device__ inline int nearest_src(int d, int in, float scale) { return (int)fminf(floorf((float)d * scale), (float)(in - 1)); }

constexpr int kNearestRows = 64;                           // output rows of one scale per workgroup
constexpr int kWaveRows = kNearestRows / (kThreads / RMNET_WAVE);      // consecutive output rows per wave

struct NearestScales {
  int hd[RMNET_TTA_MAX_ENTRIES], wd[RMNET_TTA_MAX_ENTRIES];
  float scale_h[RMNET_TTA_MAX_ENTRIES], scale_w[RMNET_TTA_MAX_ENTRIES];
};

// grid: x = ceil(max Hd / kNearestRows), y = min(N, 65535), z = S.  The sampled set of a scale is separable, the rows {src(y)} times
// the columns {src(x)}: workgroup j takes the output rows [j * kNearestRows, ...) of its scale, wave w of it kWaveRows consecutive
// ones of those, and a lane the output columns lane, lane + 64, ...; it keeps a column's source index over the walk down its rows.
// An output row that reads the source row of its predecessor (upscales) is skipped.  Workgroups and waves past a scale's last row
// and lanes past its last column add nothing, but no lane leaves before the reduction: the cross-lane steps read every lane.
__global__ __launch_bounds__(kThreads) void lo_presence_nearest(const uint8_t* __restrict__ labels, uint32_t* __restrict__ presence, NearestScales q,
                                                                int N, int Hs, int Ws) {
  const int s = blockIdx.z;
  const int hd = q.hd[s], wd = q.wd[s];
  const float scale_h = q.scale_h[s], scale_w = q.scale_w[s];
  const int lane = threadIdx.x & (RMNET_WAVE - 1), wave = threadIdx.x / RMNET_WAVE;
  const int y0 = (int)blockIdx.x * kNearestRows + wave * kWaveRows;
  const int y_end = min(y0 + kWaveRows, hd);
  const long long plane = (long long)Hs * Ws;
  for (int n = blockIdx.y; n < N; n += gridDim.y) {
    const uint8_t* frame = labels + n * plane;
    Set256 set = {0ull, 0ull, 0ull, 0ull};
    for (int x = lane; x < wd; x += RMNET_WAVE) {
      const uint8_t* col = frame + nearest_src(x, Ws, scale_w);
      unsigned prev = 256u;                                // no byte
      int prev_row = -1;
      for (int y = y0; y < y_end; ++y) {
        const int sy = nearest_src(y, Hs, scale_h);
        if (sy == prev_row) continue;
        prev_row = sy;
        const unsigned v = col[(long long)sy * Ws];
        if (v != prev) set_add(set, v);
        prev = v;
      }
    }
    const unsigned long long w[4] = {set.w0, set.w1, set.w2, set.w3};
    uint32_t* row = presence + ((long long)s * N + n) * 8;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const unsigned word = wave_or((unsigned)(w[i >> 1] >> (32 * (i & 1))));
      if (lane == 0 && word != 0u) atomicOr(row + i, word);
    }
  }
}

// ------------------------------------------------------------------------------------------------ edit + soft-max
template <int V> __device__ inline void load_f(const float* src, float (&v)[V]) {
  if constexpr (V == 4) {
    const float4 f = *reinterpret_cast<const float4*>(src);
    v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
  } else {
    v[0] = src[0];
  }
}

// The logit of channel k at V consecutive pixels after the edit; `r` holds lut[label] of those pixels (256: no label map)
template <int V>
__device__ inline void edited_logit(const float* src, int act, int k, const int (&r)[V], float (&l)[V]) {
  if (act == 1) {
#pragma unroll
    for (int i = 0; i < V; ++i) l[i] = kAbsentLogit;
  } else if (act == 2) {
#pragma unroll
    for (int i = 0; i < V; ++i) l[i] = (r[i] == k ? 1.0f : 0.0f) * kNewObjectScale - kNewObjectShift;
  } else {
    load_f<V>(src, l);
  }
}

template <int V> __device__ inline void store_f(float* dst, const float (&v)[V]) {
  if constexpr (V == 4) *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
  else dst[0] = v[0];
}

// The three walks of a lane over the K channels of its V consecutive pixels: the edit and the maximum, the exponentials (parked in
// prob) and their sum, the division.  `r` holds lut[label] of the pixels (256: no label map); the action row is wave-uniform.
template <int V>
__device__ inline void edit_walks(float* lg, float* pr, const uint8_t* act, const int (&r)[V], int K, long long HW) {
  float mx[V] = {};
  for (int k = 0; k < K; ++k) {
    const int a = act[k];
    float l[V];
    edited_logit<V>(lg + k * HW, a, k, r, l);
    if (a == 1 || a == 2) store_f<V>(lg + k * HW, l);        // a kept channel is not rewritten
#pragma unroll
    for (int i = 0; i < V; ++i) mx[i] = k == 0 ? l[i] : fmaxf(mx[i], l[i]);
  }
  float sum[V] = {};
  for (int k = 0; k < K; ++k) {
    float l[V], e[V];
    edited_logit<V>(lg + k * HW, act[k], k, r, l);
#pragma unroll
    for (int i = 0; i < V; ++i) {
      e[i] = expf(l[i] - mx[i]);
      sum[i] = k == 0 ? e[i] : sum[i] + e[i];
    }
    store_f<V>(pr + k * HW, e);
  }
  for (int k = 0; k < K; ++k) {
    float e[V];
    load_f<V>(pr + k * HW, e);
#pragma unroll
    for (int i = 0; i < V; ++i) e[i] = e[i] / sum[i];
    store_f<V>(pr + k * HW, e);
  }
}

// grid: x = ceil(H*W / (kThreads * V)), y = B.  A lane owns V consecutive pixels and walks the K channels three times (edit_walks).
template <int V>
__global__ __launch_bounds__(kThreads) void lo_edit(float* __restrict__ logit, long long logit_bs, const uint8_t* __restrict__ labels,
                                                    long long labels_bs, const uint8_t* __restrict__ lut, const uint8_t* __restrict__ action,
                                                    float* __restrict__ prob, long long prob_bs, int K, long long HW) {
  const long long p = ((long long)blockIdx.x * kThreads + threadIdx.x) * V;
  if (p >= HW) return;
  const int b = blockIdx.y;
  int r[V];
#pragma unroll
  for (int i = 0; i < V; ++i) r[i] = 256;
  if (labels) {
    const uint8_t* lab = labels + b * labels_bs + p;
    const uint8_t* table = lut + b * 256;
#pragma unroll
    for (int i = 0; i < V; ++i) r[i] = table[lab[i]];
  }
  edit_walks<V>(logit + b * logit_bs + p, prob + b * prob_bs + p, action + (long long)b * K, r, K, HW);
}

// The same grid and lanes on a frame of H x W whose labels are read from a full-size map [B,Hs,Ws]: pixel (y, x) of slot b takes
// labels[b][src(y)][src(flipped ? W - 1 - x : x)].  The V pixels of a lane are consecutive in the flattened frame; they stay inside
// one row when W % 4 == 0, and otherwise the step to the next pixel wraps into the next row, so (y, x) is formed per pixel.
template <int V>
__global__ __launch_bounds__(kThreads) void lo_edit_nearest(float* __restrict__ logit, long long logit_bs, const uint8_t* __restrict__ labels,
                                                            long long labels_bs, int Hs, int Ws, float scale_h, float scale_w,
                                                            unsigned long long flip_bits, const uint8_t* __restrict__ lut,
                                                            const uint8_t* __restrict__ action, float* __restrict__ prob, long long prob_bs, int K,
                                                            int W, long long HW) {
  const long long p = ((long long)blockIdx.x * kThreads + threadIdx.x) * V;
  if (p >= HW) return;
  const int b = blockIdx.y;
  int r[V];
#pragma unroll
  for (int i = 0; i < V; ++i) r[i] = 256;
  if (labels) {
    const uint8_t* lab = labels + b * labels_bs;
    const uint8_t* table = lut + b * 256;
    const bool flipped = (flip_bits >> b) & 1ull;
    int y = (int)(p / W), x = (int)(p - (long long)y * W);
#pragma unroll
    for (int i = 0; i < V; ++i) {
      const int xx = flipped ? W - 1 - x : x;
      r[i] = table[lab[(long long)nearest_src(y, Hs, scale_h) * Ws + nearest_src(xx, Ws, scale_w)]];
      if (++x == W) { x = 0; ++y; }
    }
  }
  edit_walks<V>(logit + b * logit_bs + p, prob + b * prob_bs + p, action + (long long)b * K, r, K, HW);
}

inline bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
inline bool good_scale(float s) { return s > 0.0f && s <= 3.0e38f; }        // finite and positive (false for a NaN)
constexpr int kMaxSide = 1 << 24;                          // every index of a side is exact as a float

}  // namespace

int label_presence_chunk() { return kChunk; }

int launch_label_presence(const uint8_t* labels, int N, int H, int W, uint32_t* presence, hipStream_t st) {
  if (!labels || !presence || N < 1 || H < 1 || W < 1 || !aligned(presence, 4)) return RMNET_E_INVALID_ARG;
  const long long HW = (long long)H * W;
  if (HW * N >= (1LL << 31)) return RMNET_E_UNSUPPORTED;
  long long bpf = ((HW >> 4) + kThreads * kIter - 1) / (kThreads * kIter);      // (the body has at most HW / 16 vectors)
  if (bpf < 1) bpf = 1;
  if (hipMemsetAsync(presence, 0, (size_t)N * 8 * sizeof(uint32_t), st) != hipSuccess) return RMNET_E_LAUNCH;
  hipLaunchKernelGGL(lo_presence, dim3((unsigned)(bpf * N)), dim3(kThreads), 0, st, labels, presence, HW, (unsigned)bpf);
  return check_launch();
}

int launch_object_edit_softmax(float* logit, long long logit_bs, const uint8_t* labels, long long labels_bs, const uint8_t* lut,
                               const uint8_t* action, float* prob, long long prob_bs, int B, int K, int H, int W, hipStream_t st) {
  if (!logit || !lut || !action || !prob || B < 1 || H < 1 || W < 1 || K < 1 || K > 255) return RMNET_E_INVALID_ARG;
  if (!aligned(logit, 4) || !aligned(prob, 4)) return RMNET_E_INVALID_ARG;
  const long long HW = (long long)H * W;
  if (logit_bs < K * HW || prob_bs < K * HW || (labels && labels_bs < HW)) return RMNET_E_INVALID_ARG;
  const long long lim = 1LL << 31;
  if (B > 65535 || K * HW >= lim || logit_bs >= lim || prob_bs >= lim || labels_bs >= lim) return RMNET_E_UNSUPPORTED;
  if ((B - 1) * logit_bs + K * HW >= lim || (B - 1) * prob_bs + K * HW >= lim || (labels && (B - 1) * labels_bs + HW >= lim))
    return RMNET_E_UNSUPPORTED;
  const bool vec = HW % 4 == 0 && aligned(logit, 16) && aligned(prob, 16) && logit_bs % 4 == 0 && prob_bs % 4 == 0;
  const long long per_block = (long long)kThreads * (vec ? 4 : 1);
  const dim3 grid((unsigned)((HW + per_block - 1) / per_block), (unsigned)B);
  if (vec) hipLaunchKernelGGL(lo_edit<4>, grid, dim3(kThreads), 0, st, logit, logit_bs, labels, labels_bs, lut, action, prob, prob_bs, K, HW);
  else hipLaunchKernelGGL(lo_edit<1>, grid, dim3(kThreads), 0, st, logit, logit_bs, labels, labels_bs, lut, action, prob, prob_bs, K, HW);
  return check_launch();
}

int label_presence_nearest_rows() { return kNearestRows; }

int launch_label_presence_nearest(const uint8_t* labels, int N, int Hs, int Ws, const int* hd, const int* wd, const float* scale_h,
                                  const float* scale_w, int S, uint32_t* presence, hipStream_t st) {
  if (!labels || !presence || !hd || !wd || !scale_h || !scale_w || N < 1 || Hs < 1 || Ws < 1 || !aligned(presence, 4))
    return RMNET_E_INVALID_ARG;
  if (S < 1 || S > RMNET_TTA_MAX_ENTRIES) return RMNET_E_INVALID_ARG;
  NearestScales q = {};
  int h_max = 0;
  for (int s = 0; s < S; ++s) {
    if (hd[s] < 1 || wd[s] < 1 || !good_scale(scale_h[s]) || !good_scale(scale_w[s])) return RMNET_E_INVALID_ARG;
    q.hd[s] = hd[s]; q.wd[s] = wd[s]; q.scale_h[s] = scale_h[s]; q.scale_w[s] = scale_w[s];
    h_max = hd[s] > h_max ? hd[s] : h_max;
  }
  if (Hs > kMaxSide || Ws > kMaxSide) return RMNET_E_UNSUPPORTED;
  for (int s = 0; s < S; ++s)
    if (hd[s] > kMaxSide || wd[s] > kMaxSide) return RMNET_E_UNSUPPORTED;
  if ((long long)Hs * Ws * N >= (1LL << 31)) return RMNET_E_UNSUPPORTED;
  if (hipMemsetAsync(presence, 0, (size_t)S * N * 8 * sizeof(uint32_t), st) != hipSuccess) return RMNET_E_LAUNCH;
  const dim3 grid((unsigned)((h_max + kNearestRows - 1) / kNearestRows), (unsigned)(N < 65535 ? N : 65535), (unsigned)S);
  hipLaunchKernelGGL(lo_presence_nearest, grid, dim3(kThreads), 0, st, labels, presence, q, N, Hs, Ws);
  return check_launch();
}

int launch_object_edit_softmax_nearest(float* logit, long long logit_bs, const uint8_t* labels, long long labels_bs, int Hs, int Ws,
                                       float scale_h, float scale_w, unsigned long long flip_bits, const uint8_t* lut, const uint8_t* action,
                                       float* prob, long long prob_bs, int B, int K, int H, int W, hipStream_t st) {
  if (!logit || !lut || !action || !prob || B < 1 || H < 1 || W < 1 || Hs < 1 || Ws < 1 || K < 1 || K > 255) return RMNET_E_INVALID_ARG;
  if (!aligned(logit, 4) || !aligned(prob, 4) || !good_scale(scale_h) || !good_scale(scale_w)) return RMNET_E_INVALID_ARG;
  const long long HW = (long long)H * W, HWs = (long long)Hs * Ws;
  if (logit_bs < K * HW || prob_bs < K * HW || (labels && labels_bs != 0 && labels_bs < HWs)) return RMNET_E_INVALID_ARG;      // (0: one map for every slot)
  const long long lim = 1LL << 31;
  if (B > 64 || H > kMaxSide || W > kMaxSide || Hs > kMaxSide || Ws > kMaxSide) return RMNET_E_UNSUPPORTED;      // (one flip bit per slot)
  if (K * HW >= lim || logit_bs >= lim || prob_bs >= lim || labels_bs >= lim || HWs >= lim) return RMNET_E_UNSUPPORTED;
  if ((B - 1) * logit_bs + K * HW >= lim || (B - 1) * prob_bs + K * HW >= lim || (labels && (B - 1) * labels_bs + HWs >= lim))
    return RMNET_E_UNSUPPORTED;
  const bool vec = HW % 4 == 0 && aligned(logit, 16) && aligned(prob, 16) && logit_bs % 4 == 0 && prob_bs % 4 == 0;
  const long long per_block = (long long)kThreads * (vec ? 4 : 1);
  const dim3 grid((unsigned)((HW + per_block - 1) / per_block), (unsigned)B);
  if (vec)
    hipLaunchKernelGGL(lo_edit_nearest<4>, grid, dim3(kThreads), 0, st, logit, logit_bs, labels, labels_bs, Hs, Ws, scale_h, scale_w, flip_bits,
                       lut, action, prob, prob_bs, K, W, HW);
  else
    hipLaunchKernelGGL(lo_edit_nearest<1>, grid, dim3(kThreads), 0, st, logit, logit_bs, labels, labels_bs, Hs, Ws, scale_h, scale_w, flip_bits,
                       lut, action, prob, prob_bs, K, W, HW);
  return check_launch();
}

}  // namespace rmnet
