// mzgo_unroll.hpp -- the scalar pieces of the unroll's heads (mzgo_unroll.hip:
// the heads kernels and mzgo_unroll_heads_host run this text, so the formulas
// a CPU test checks are the kernels'): the tails of main.py's value head
// (PredictionNetwork, main.py:116-144: value_fc on the board mean of
// value_conv) and reward head (DynamicsNetwork, main.py:97-113:
// fc_reward_output(relu(fc_reward_hidden(.))) on the board mean of
// reward_conv), forward and backward, and one entry of a latent's gradient.
#pragma once
#include <hip/hip_runtime.h>

namespace mzgo {

constexpr int kRewardHidden = 16;       // fc_reward_hidden: Linear(1, 16)

// A (step, sample)'s partial sums for the thirteen head tensors, in one row of
// head_part_stride(C) floats: three C-vectors (policy_conv, value_conv and
// reward_conv weights at 0, C and 2 C), three 16-vectors, seven scalars.
__host__ __device__ __forceinline__ int head_part_fc1_w(int C) { return 3 * C; }
__host__ __device__ __forceinline__ int head_part_fc1_b(int C) { return 3 * C + 16; }
__host__ __device__ __forceinline__ int head_part_fc2_w(int C) { return 3 * C + 32; }
enum HeadScalar { HS_POLICY_B, HS_VALUE_B, HS_VFC_W, HS_VFC_B, HS_PASS, HS_REWARD_B, HS_FC2_B, HS_COUNT };
__host__ __device__ __forceinline__ int head_part_scalar(int C, int which) { return 3 * C + 48 + which; }
__host__ __device__ __forceinline__ int head_part_stride(int C) { return 3 * C + 64; }

// value = value_fc(vmean)
__host__ __device__ __forceinline__ float heads_value(float vmean, float vfc_w, float vfc_b) {
  return vfc_w * vmean + vfc_b;
}
// d value_fc.weight, d value_fc.bias and d vmean from dv = dL / d value
__host__ __device__ __forceinline__ float heads_value_grad(float dv, float vmean, float vfc_w, float* g_vfc_w,
                                                           float* g_vfc_b) {
  *g_vfc_w = dv * vmean;
  *g_vfc_b = dv;
  return dv * vfc_w;
}

// reward = fc_reward_output(relu(fc_reward_hidden(rmean))): the hidden units
// summed in index order
__host__ __device__ __forceinline__ float heads_reward(float rmean, const float* fc1_w, const float* fc1_b,
                                                       const float* fc2_w, float fc2_b) {
  float r = 0.f;
  for (int j = 0; j < kRewardHidden; ++j) {
    const float pre = fc1_w[j] * rmean + fc1_b[j];
    r += fc2_w[j] * (pre > 0.f ? pre : 0.f);
  }
  return r + fc2_b;
}
// The reward tail's backward from dr = dL / d reward: the three 16-vectors of
// gradients, d fc_reward_output.bias = dr itself, and the return value
// d rmean.  A hidden unit whose pre-activation is <= 0 (exactly 0 included)
// passes nothing back, as autograd's relu.
__host__ __device__ __forceinline__ float heads_reward_grad(float dr, float rmean, const float* fc1_w,
                                                            const float* fc1_b, const float* fc2_w, float* g_fc1_w,
                                                            float* g_fc1_b, float* g_fc2_w) {
  float drmean = 0.f;
  for (int j = 0; j < kRewardHidden; ++j) {
    const float pre = fc1_w[j] * rmean + fc1_b[j];
    const bool on = pre > 0.f;
    g_fc2_w[j] = dr * (on ? pre : 0.f);
    const float dpre = on ? dr * fc2_w[j] : 0.f;
    g_fc1_w[j] = dpre * rmean;
    g_fc1_b[j] = dpre;
    drmean += dpre * fc1_w[j];
  }
  return drmean;
}

// One entry of the heads' gradient into a latent: the policy map's cell
// gradient through policy_conv, and the two means' gradients spread evenly
// over the board's cells through value_conv and reward_conv
__host__ __device__ __forceinline__ float heads_latent_grad(float w_pol, float g_logit, float w_val, float dvmean,
                                                            float w_rew, float drmean, float cells) {
  return w_pol * g_logit + (w_val * dvmean + w_rew * drmean) / cells;
}

}  // namespace mzgo
