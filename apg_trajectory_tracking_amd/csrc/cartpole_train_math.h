// cartpole_train_math.h - per-sample arithmetic and the gradient layout of the
// fused controller step of the cart-pole (cartpole_train.hip:
// apg_cartpole_mlp_train_step; host twin in cpu_twins.hip): the controller
// branch of TrainCartpole.run_epoch (scripts/train_cartpole.py:127-155) with
// simple_model.Net (neural_control/models/simple_model.py:9-28) as policy,
//   actions = tanh(fc_out(tanh(fc3(tanh(fc2(tanh(fc1(tanh(fc0(x))))))))))
// (x = in_state with column 0 zeroed), the rollout of cartpole_rollout_math.h
// from state0, the cotangent chain back through the five tanh layers and every
// parameter's gradient summed over the batch, then (optionally) momentum SGD.
// A layer is stated once, cpt_dense: it serves the forward products (outputs x
// inputs) and the transposed ones of the reverse pass (inputs x outputs) alike.
#pragma once
#include "cartpole_rollout_math.h"

namespace apg {
namespace {

// simple_model.Net(4, H): 4 -> 32 -> 64 -> 64 -> 32 -> H
constexpr int kCptIn = 4, kCptH0 = 32, kCptH1 = 64, kCptH2 = 64, kCptH3 = 32;
// where a tensor starts in the flat gradient (named_parameters() order: fc0,
// fc1, fc2, fc3, fc_out, weight before bias); fc_out.bias starts at
// kCptGWout + 32 H, the whole gradient is cpt_grads(H) floats
constexpr int kCptGW0 = 0, kCptGB0 = kCptGW0 + kCptH0 * kCptIn;
constexpr int kCptGW1 = kCptGB0 + kCptH0, kCptGB1 = kCptGW1 + kCptH1 * kCptH0;
constexpr int kCptGW2 = kCptGB1 + kCptH1, kCptGB2 = kCptGW2 + kCptH2 * kCptH1;
constexpr int kCptGW3 = kCptGB2 + kCptH2, kCptGB3 = kCptGW3 + kCptH3 * kCptH2;
constexpr int kCptGWout = kCptGB3 + kCptH3;                                  // 8 512
__host__ __device__ __forceinline__ int cpt_grads(int H) { return kCptGWout + (kCptH3 + 1) * H; }

// z[u] += sum over j < K (ascending) of w(u, j) x(j); z arrives holding the
// bias (forward) or zero (the transposed product of the reverse pass)
template <int U, class W, class X>
__host__ __device__ __forceinline__ void cpt_dense(float (&z)[U], int K, W &&w, X &&x) {
#pragma unroll 8
  for (int j = 0; j < K; ++j) {
    const float xj = x(j);
#pragma unroll
    for (int u = 0; u < U; ++u) z[u] = fmaf(w(u, j), xj, z[u]);
  }
}

// cotangent of a tanh layer's pre-activation from that of its output y
__host__ __device__ __forceinline__ float cpt_dtanh(float g, float y) {
  return g * (1.f - y * y);
}

// one sample's share of a unit's weight cotangents: gw[j] += dz x(j), gb += dz
template <int KP, class X>
__host__ __device__ __forceinline__ void cpt_wgrad(float (&gw)[KP], float &gb, float dz,
                                                   X &&x) {
#pragma unroll
  for (int j = 0; j < KP; ++j) gw[j] = fmaf(dz, x(j), gw[j]);
  gb += dz;
}

// element c of the flat gradient: tensor q (0..9: w0, b0, ..., w_out, b_out)
// and the element's offset in it
__host__ __device__ __forceinline__ void cpt_locate(int c, int H, int &q, int &off) {
  const int start[10] = {kCptGW0, kCptGB0, kCptGW1, kCptGB1, kCptGW2,
                         kCptGB2, kCptGW3, kCptGB3, kCptGWout, kCptGWout + kCptH3 * H};
  q = 0;
  off = c;
#pragma unroll
  for (int i = 1; i < 10; ++i)
    if (c >= start[i]) q = i, off = c - start[i];
}

// torch.optim.SGD with momentum, as its fused kernel computes it: in double,
// rounded once each (the rule of ApgMlpSgdUpdate)
__host__ __device__ __forceinline__ void cpt_sgd(float g, double lr, double momentum, float &p,
                                                 float &buf) {
  buf = (float)(momentum * (double)buf + (double)g);
  p = (float)((double)p - lr * (double)buf);
}

}  // namespace
}  // namespace apg
