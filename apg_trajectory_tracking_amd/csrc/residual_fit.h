// residual_fit.h - what the simulator-fit steps of the learnt simulators share
// (wing_learnt.hip: apg_wing_learnt_fit_fwd_bwd; quad_fit.hip:
// apg_quad_learnt_fit_fwd_bwd).  Both modules carry the same 16 -> 64 -> 12
// residual network, so the cotangents of a hidden unit for one sample, the
// regulariser (four 2-norms, gradient t / |t|) and the fixed-order sum over the
// workgroups' partial rows are stated here once; where a unit's weights sit in
// its packed row and where a tensor starts in the flat gradient are template
// arguments of the system's own header (wing_learnt_math.h, quad_fit_math.h).
#pragma once
#include "apg_device.h"

namespace apg {
namespace {

constexpr int kResHidden = 64;
constexpr int kResFitUnit = 29;   // a unit's cotangents: dW1[m][0..15], dW2[0..11][m], db1[m]

// gw += hidden unit's 29 cotangents for one sample (z, lam): gw[j < 16] =
// dW1[m][j], gw[16 + o] = dW2[o][m], gw[28] = db1[m]; w = the unit's packed row:
// W1[m][0..15] at 0, W2[0..11][m] at W2, b1[m] at B1 (relu'(0) = 0, as torch's
// threshold backward)
template <int W2, int B1>
__host__ __device__ __forceinline__ void residual_unit_grads(const float *w,
                                                             const float (&z)[16],
                                                             const float (&lam)[12],
                                                             float (&gw)[kResFitUnit]) {
  float h = w[B1];
#pragma unroll
  for (int j = 0; j < 16; ++j) h = fmaf(w[j], z[j], h);
  float dh = 0.f;
#pragma unroll
  for (int o = 0; o < 12; ++o) dh = fmaf(w[W2 + o], lam[o], dh);
  dh = h > 0.f ? dh : 0.f;
  h = fmaxf(h, 0.f);
#pragma unroll
  for (int j = 0; j < 16; ++j) gw[j] = fmaf(dh, z[j], gw[j]);
#pragma unroll
  for (int o = 0; o < 12; ++o) gw[16 + o] = fmaf(lam[o], h, gw[16 + o]);
  gw[28] += dh;
}

// the regulariser's gradient l2_lambda t / |t| (0 where |t| = 0, as torch's
// norm backward) for element `dest` of a flat gradient whose residual tensors
// start at GW1 < GB1 < GW2 < GB2; norms = |W2|, |b2|, |W1|, |b1| (the order of
// _residual_weight_norm)
template <int GW1, int GB1, int GW2, int GB2>
__host__ __device__ __forceinline__ float residual_l2_grad(int dest, float l2_lambda,
                                                           const float *w1, const float *b1,
                                                           const float *w2, const float *b2,
                                                           const float *norms) {
  if (dest < GW1) return 0.f;
  float t, n;
  if (dest < GB1) t = w1[dest - GW1], n = norms[2];
  else if (dest < GW2) t = b1[dest - GB1], n = norms[3];
  else if (dest < GB2) t = w2[dest - GW2], n = norms[0];
  else t = b2[dest - GB2], n = norms[1];
  return n > 0.f ? l2_lambda * (t / n) : 0.f;
}

#if defined(__HIPCC__)
// |W2|, |b2|, |W1|, |b1| (2-norms) by one workgroup of 256: per-thread strided
// sums, then a fixed tree; thread q < 4 writes norms[q]
__device__ __forceinline__ void residual_norms(const float *w1, const float *b1,
                                               const float *w2, const float *b2,
                                               float (&part)[4][256], float *norms) {
  const float *tens[4] = {w2, b2, w1, b1};
  const int count[4] = {12 * kResHidden, 12, kResHidden * 16, kResHidden};
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    float acc = 0.f;
    for (int t = threadIdx.x; t < count[q]; t += 256) acc = fmaf(tens[q][t], tens[q][t], acc);
    part[q][threadIdx.x] = acc;
  }
  for (int half = 128; half >= 1; half >>= 1) {
    __syncthreads();
    if ((int)threadIdx.x < half)
#pragma unroll
      for (int q = 0; q < 4; ++q) part[q][threadIdx.x] += part[q][threadIdx.x + half];
  }
  if (threadIdx.x < 4) norms[threadIdx.x] = sqrtf(part[threadIdx.x][0]);
}

// Element c of the sum over `nrows` partial rows of ROW floats, by the 8
// threads (r = 0..7) that share column `col` of a workgroup: thread r adds rows
// r, r + 8, ... in order, then a fixed tree over the 8 sums.  The value is
// returned to thread r == 0 (the others get 0).
template <int ROW, int COLS>
__device__ __forceinline__ float fit_rows_sum(const float *__restrict__ rows, int nrows, int c,
                                              int col, int r, float (&part)[8][COLS]) {
  float acc = 0.f;
#pragma unroll 4
  for (int i = r; i < nrows; i += 8) acc += rows[(size_t)i * ROW + c];
  part[r][col] = acc;
  __syncthreads();
  if (r != 0) return 0.f;
  return ((part[0][col] + part[1][col]) + (part[2][col] + part[3][col])) +
         ((part[4][col] + part[5][col]) + (part[6][col] + part[7][col]));
}
#endif

}  // namespace
}  // namespace apg
