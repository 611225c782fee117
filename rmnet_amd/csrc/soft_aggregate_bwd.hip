// soft_aggregate_bwd.hip -- the gradient of the decoder tail (soft_aggregate in epilogue.hip, then lo_edit in late_objects.hip on an
// edited frame) with respect to the decoder logits, in ONE streaming pass (include/rmnet_hip.h: rmnet_soft_aggregate_bwd_f32).
//
// Forward, per clip b and output pixel (models/rmnet.py:368-370, 289-302, 376-380, 436-450):
//   p_o = soft-max(z0, z1)[1] of object o,  bg = prod_o (1 - p_o),  logit_0 = L(clamp(bg)),  logit_{o+1} = L(clamp(p_o)),
//   L(e) = log(e / (1 - e)),  the channels n+1 .. K-1 and the edited ones are constants,  P = soft-max over the K channels.
// Backward, with g = d loss / d P, q = d loss / d logit (either may be absent) and the saved P:
//   s    = sum_k P_k g_k                                  over all K channels, in channel order
//   dl_k = P_k (g_k - s) + q_k                            (q_k alone without g: P is not read then)
//   live_k = k <= n and action[b][k] == 0,  pass(e) = 1e-7f <= e <= 1 - 1e-7f  (the forward's fp32 e; false for a NaN)
//   a0   = live_0 and pass(bg) ? dl_0 / (1 - bg) : 0
//   dz_o = (live_{o+1} and pass(p_o) ? dl_{o+1} : 0) - a0 p_o
//   grad_dec[o, 1] = dz_o,  grad_dec[o, 0] = -dz_o
// L(clamp(p_o)) is z1 - z0 where the clamp passes, so its derivative is 1, and d logit_0 / d (z1 - z0)_o = -p_o / (1 - bg): no
// prefix or suffix products and no 1 / (p (1 - p)).  The selects keep a NaN out of a masked term but not out of a0 p_o: a NaN in
// an object's logits makes P, hence dl, NaN at that pixel, and every object of the clip gets a NaN there unless its channel AND the
// background are masked, in which case it gets 0 -- never a finite non-zero value.
//
// A lane owns V consecutive pixels of the PADDED plane, so that every element of grad_dec [n_tot, 2, Hp, Wp] is written exactly
// once, zeros in the padding and for the objects at or beyond the cap K - 1 included: no memset, no atomics, the same bits on
// every call.  It walks the K channels for s, the n objects for bg, and the n objects again for dz; the second read of dec comes
// from the cache (a lane re-reads its own addresses).  V = 4 needs Wp % 4 == 0 (a lane's pixels stay in one row) and 16-byte
// aligned dec / grad_dec; P, g and q sit in the UN-padded plane, and are read with 16-byte loads only when that plane's rows keep
// the alignment too (PV: W % 4 == 0, pad_l % 4 == 0, aligned pointers and strides), one pixel at a time otherwise.
#include "common.h"

#pragma clang fp contract(off)   // P * (g - s) + q rounds product and sum separately, as tests/tail_backward_ref.py restates it

#include "soft_aggregate_parts.h"

namespace rmnet {
namespace {

constexpr int kThreads = 256;
constexpr int kMaxChunks = 1024;                          // workgroups per clip; a larger plane is walked grid-stride

// V values of one channel at the lane's pixels; a pixel outside the un-padded window reads 0 (and nothing from memory)
template <int V, bool PV>
__device__ inline void load_px(const float* __restrict__ chan, const long long (&idx)[V], const bool (&in)[V], float (&v)[V]) {
  if constexpr (V == 4 && PV) {                           // all four inside or none, and idx[0] is a multiple of 4
    const float4 f = in[0] ? *reinterpret_cast<const float4*>(chan + idx[0]) : float4{0.f, 0.f, 0.f, 0.f};
    v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
  } else {
#pragma unroll
    for (int i = 0; i < V; ++i) v[i] = in[i] ? chan[idx[i]] : 0.0f;
  }
}

template <int V> __device__ inline void load_v(const float* __restrict__ src, float (&v)[V]) {
  if constexpr (V == 4) {
    const float4 f = *reinterpret_cast<const float4*>(src);
    v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
  } else {
    v[0] = src[0];
  }
}

template <int V> __device__ inline void store_v(float* __restrict__ dst, const float (&v)[V]) {
  if constexpr (V == 4) *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
  else dst[0] = v[0];
}

// dl_k at the lane's pixels (see the head of the file)
template <int V, bool PV>
__device__ inline void dlogit(const float* __restrict__ prob, const float* __restrict__ gp, const float* __restrict__ gl, long long off,
                              const long long (&idx)[V], const bool (&in)[V], const float (&s)[V], float (&dl)[V]) {
  if (gp) {
    float P[V], g[V];
    load_px<V, PV>(prob + off, idx, in, P);
    load_px<V, PV>(gp + off, idx, in, g);
#pragma unroll
    for (int i = 0; i < V; ++i) dl[i] = P[i] * (g[i] - s[i]);
    if (gl) {
      float q[V];
      load_px<V, PV>(gl + off, idx, in, q);
#pragma unroll
      for (int i = 0; i < V; ++i) dl[i] = dl[i] + q[i];
    }
  } else {
    load_px<V, PV>(gl + off, idx, in, dl);
  }
}

// grid: x = min(ceil(Hp * Wp / (kThreads * V)), kMaxChunks), y = B
template <int V, bool PV>
__global__ __launch_bounds__(kThreads) void soft_aggregate_bwd(const float* __restrict__ dec, const int32_t* __restrict__ obj_begin, int K,
                                                               int Hp, int Wp, int pad_l, int pad_t, int H, int W,
                                                               const float* __restrict__ prob, long long prob_bs,
                                                               const float* __restrict__ gp, long long gp_bs,
                                                               const float* __restrict__ gl, long long gl_bs,
                                                               const uint8_t* __restrict__ action, float* __restrict__ grad_dec) {
  const int b = blockIdx.y;
  const int o0 = obj_begin[b], cnt = obj_begin[b + 1] - o0, n = min(cnt, K - 1);
  if (cnt <= 0) return;                                   // a clip without objects owns no plane of grad_dec
  const long long plane = (long long)Hp * Wp, oplane = (long long)H * W;
  const uint8_t* act = action ? action + (long long)b * K : nullptr;
  const float* pb = prob + b * prob_bs;
  const float* gpb = gp ? gp + b * gp_bs : nullptr;
  const float* glb = gl ? gl + b * gl_bs : nullptr;
  float zv[V];
#pragma unroll
  for (int i = 0; i < V; ++i) zv[i] = 0.0f;
  for (long long p = ((long long)blockIdx.x * kThreads + threadIdx.x) * V; p < plane; p += (long long)gridDim.x * kThreads * V) {
    const int y = (int)(p / Wp), x = (int)(p - (long long)y * Wp);
    const bool row_in = y >= pad_t && y < pad_t + H;
    bool in[V], any = false;
    long long idx[V];
#pragma unroll
    for (int i = 0; i < V; ++i) {                         // (V == 4: Wp % 4 == 0, the four pixels are in row y)
      in[i] = row_in && x + i >= pad_l && x + i < pad_l + W;
      idx[i] = in[i] ? (long long)(y - pad_t) * W + (x + i - pad_l) : 0;
      any = any || in[i];
    }
    const float* d = dec + (size_t)o0 * 2 * plane + p;
    float* gd = grad_dec + (size_t)o0 * 2 * plane + p;
    for (int o = any ? n : 0; o < cnt; ++o) {             // beyond the cap; in the padding, every object
      store_v<V>(gd + (size_t)o * 2 * plane, zv);
      store_v<V>(gd + (size_t)o * 2 * plane + plane, zv);
    }
    if (!any) continue;

    float s[V];
#pragma unroll
    for (int i = 0; i < V; ++i) s[i] = 0.0f;
    if (gpb) {
      for (int k = 0; k < K; ++k) {
        float P[V], g[V];
        load_px<V, PV>(pb + k * oplane, idx, in, P);
        load_px<V, PV>(gpb + k * oplane, idx, in, g);
#pragma unroll
        for (int i = 0; i < V; ++i) s[i] = k == 0 ? P[i] * g[i] : s[i] + P[i] * g[i];
      }
    }

    float bg[V];
#pragma unroll
    for (int i = 0; i < V; ++i) bg[i] = 1.0f;
    for (int o = 0; o < n; ++o) {
      float z0[V], z1[V];
      load_v<V>(d + (size_t)o * 2 * plane, z0);
      load_v<V>(d + (size_t)o * 2 * plane + plane, z1);
#pragma unroll
      for (int i = 0; i < V; ++i) bg[i] = bg[i] * (1.0f - sa::fg_prob_of(z0[i], z1[i]));
    }

    float a0[V];
    {
      float dl[V];
      dlogit<V, PV>(pb, gpb, glb, 0, idx, in, s, dl);
      const bool live = !act || act[0] == 0;
#pragma unroll
      for (int i = 0; i < V; ++i) a0[i] = live && sa::clamp_passes(bg[i]) ? dl[i] / (1.0f - bg[i]) : 0.0f;
    }

    for (int o = 0; o < n; ++o) {
      float z0[V], z1[V], dl[V], dz[V], nz[V];
      load_v<V>(d + (size_t)o * 2 * plane, z0);
      load_v<V>(d + (size_t)o * 2 * plane + plane, z1);
      dlogit<V, PV>(pb, gpb, glb, (o + 1) * oplane, idx, in, s, dl);
      const bool live = !act || act[o + 1] == 0;
#pragma unroll
      for (int i = 0; i < V; ++i) {
        const float po = sa::fg_prob_of(z0[i], z1[i]);
        const float t = live && sa::clamp_passes(po) ? dl[i] : 0.0f;
        const float v = t - a0[i] * po;
        dz[i] = in[i] ? v : 0.0f;
        nz[i] = in[i] ? -v : 0.0f;
      }
      store_v<V>(gd + (size_t)o * 2 * plane, nz);
      store_v<V>(gd + (size_t)o * 2 * plane + plane, dz);
    }
  }
}

inline bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

int launch_soft_aggregate_bwd(const float* dec, const int32_t* obj_begin, int B, int K, int Hp, int Wp, int pad_l, int pad_t, int H, int W,
                              const float* prob, long long prob_bs, const float* grad_prob, long long grad_prob_bs, const float* grad_logit,
                              long long grad_logit_bs, const uint8_t* action, float* grad_dec, hipStream_t st) {
  if (!dec || !obj_begin || !prob || !grad_dec || (!grad_prob && !grad_logit)) return RMNET_E_INVALID_ARG;
  if (B < 1 || K < 1 || K > 255 || H < 1 || W < 1 || Hp < 1 || Wp < 1) return RMNET_E_INVALID_ARG;
  if (pad_l < 0 || pad_t < 0 || pad_l > Wp - W || pad_t > Hp - H) return RMNET_E_INVALID_ARG;
  if (!aligned(dec, 4) || !aligned(obj_begin, 4) || !aligned(prob, 4) || !aligned(grad_prob, 4) || !aligned(grad_logit, 4) ||
      !aligned(grad_dec, 4))
    return RMNET_E_INVALID_ARG;
  const long long HW = (long long)H * W, plane = (long long)Hp * Wp, lim = 1LL << 31;
  if (prob_bs < K * HW || (grad_prob && grad_prob_bs < K * HW) || (grad_logit && grad_logit_bs < K * HW)) return RMNET_E_INVALID_ARG;
  if (B > 65535 || 2 * plane >= lim || K * HW >= lim) return RMNET_E_UNSUPPORTED;
  const long long strides[3] = {prob_bs, grad_prob ? grad_prob_bs : 0, grad_logit ? grad_logit_bs : 0};
  for (long long bs : strides)
    if (bs >= lim || (B - 1) * bs + K * HW >= lim) return RMNET_E_UNSUPPORTED;
  const bool vec = Wp % 4 == 0 && aligned(dec, 16) && aligned(grad_dec, 16);
  const bool pvec = vec && W % 4 == 0 && pad_l % 4 == 0 && aligned(prob, 16) && aligned(grad_prob, 16) && aligned(grad_logit, 16) &&
                    prob_bs % 4 == 0 && strides[1] % 4 == 0 && strides[2] % 4 == 0;
  const long long per_block = (long long)kThreads * (vec ? 4 : 1);
  long long chunks = (plane + per_block - 1) / per_block;
  if (chunks > kMaxChunks) chunks = kMaxChunks;
  const dim3 grid((unsigned)chunks, (unsigned)B);
#define RMNET_SAB(V, PV)                                                                                                             \
  hipLaunchKernelGGL((soft_aggregate_bwd<V, PV>), grid, dim3(kThreads), 0, st, dec, obj_begin, K, Hp, Wp, pad_l, pad_t, H, W, prob, \
                     prob_bs, grad_prob, grad_prob_bs, grad_logit, grad_logit_bs, action, grad_dec)
  if (pvec) RMNET_SAB(4, true);
  else if (vec) RMNET_SAB(4, false);
  else RMNET_SAB(1, false);
#undef RMNET_SAB
  return check_launch();
}

}  // namespace rmnet
