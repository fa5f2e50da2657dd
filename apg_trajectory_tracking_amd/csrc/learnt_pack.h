// learnt_pack.h - the packed weight block of LearntDynamics (learnt_residual.h:
// what learnt_pack_kernel writes and the closed-loop kernels keep in LDS), as
// offsets and as a function of the element index, so that a host twin fills
// the very block the kernels read.
#pragma once
#include "apg_device.h"

namespace apg {

// [W1 [64][16] | b1 [64] | W2^T [64][12] | b2 [12] | A [4][4]]: a hidden unit's
// 16 input weights and its 12 output weights are 16-byte rows
constexpr int kLrW1 = 0, kLrB1 = 1024, kLrW2 = 1088, kLrB2 = 1856, kLrA = 1868,
              kLearntFloats = 1920;   // (a multiple of 64: whole DMA rows)

// element t of the block (t < kLearntFloats); linear_at NULL: the identity
inline float learnt_packed(int t, const ApgLearntResidual &m) {
  if (t < kLrB1) return m.w1[t];
  if (t < kLrW2) return m.b1[t - kLrB1];
  if (t < kLrB2) return m.w2[((t - kLrW2) % 12) * 64 + (t - kLrW2) / 12];
  if (t < kLrA) return m.b2[t - kLrB2];
  if (t < kLrA + 16) return m.linear_at ? m.linear_at[t - kLrA] : ((t - kLrA) % 5 == 0 ? 1.f : 0.f);
  return 0.f;
}

}  // namespace apg
