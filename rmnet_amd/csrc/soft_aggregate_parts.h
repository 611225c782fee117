// soft_aggregate_parts.h -- what the decoder tail (soft_aggregate, epilogue.hip) and its gradient (soft_aggregate_bwd.hip) share:
// the foreground probability of an object's two decoder logits and the clamp of models/rmnet.py:300.  Both files compile these
// with fp contract(off), so the backward re-creates the forward's fp32 p and bg bit for bit and its clamp test agrees with the
// forward's clamp at every value.
#pragma once
#include "common.h"

namespace rmnet {
namespace sa {

constexpr float kClampLo = 1e-7f, kClampHi = 1.0f - 1e-7f;

__device__ inline float fg_prob_of(float z0, float z1) {
  const float m = fmaxf(z0, z1);
  const float e0 = expf(z0 - m), e1 = expf(z1 - m);
  return e1 / (e0 + e1);
}
__device__ inline float fg_prob(const float* __restrict__ dec, size_t plane, size_t pix) {
  return fg_prob_of(dec[pix], dec[plane + pix]);
}
// comparisons, not fmaxf / fminf: those return the other operand for a NaN, which turned a NaN probability into the
// absent-channel logit; torch.clamp (models/rmnet.py:300) keeps it
__device__ inline float clamp_em(float em) {
  em = em < kClampLo ? kClampLo : em;
  em = em > kClampHi ? kClampHi : em;
  return em;
}
// where torch.clamp passes a gradient: the ends count as inside, a NaN does not
__device__ inline bool clamp_passes(float em) { return em >= kClampLo && em <= kClampHi; }

}  // namespace sa
}  // namespace rmnet
