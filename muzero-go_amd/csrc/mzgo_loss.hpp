// mzgo_loss.hpp -- the scalar pieces of the unroll loss (mzgo_loss.hip:
// mzgo_unroll_loss and its host twin run this text, so the formulas a CPU test
// checks are the kernel's): main.py:66-69's value transform, its derivative
// as torch's autograd forms it, the xlogy term of F.kl_div, and one row's
// value and reward terms (main.py:431-482, mzgo.trainer's _unroll_step).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

namespace mzgo {

constexpr int kLossMinA = 2;
constexpr int kLossMaxA = 362;     // 19x19 + pass

// h(x) = sign(x) (sqrt(|x| + 1) - 1) + 0.001 x, sign(0) = 0
__host__ __device__ __forceinline__ float loss_transform(float x) {
  const float sg = x > 0.f ? 1.f : x < 0.f ? -1.f : 0.f;
  return sg * (sqrtf(fabsf(x) + 1.f) - 1.f) + 0.001f * x;
}
// h'(x) = 0.5 / sqrt(|x| + 1) + 0.001 for x != 0; at x == 0 autograd gives
// 0.001 alone (sign(0) = 0 multiplies the square-root branch away)
__host__ __device__ __forceinline__ float loss_transform_grad(float x) {
  return x != 0.f ? 0.5f / sqrtf(fabsf(x) + 1.f) + 0.001f : 0.001f;
}
// xlogy(t, t): a target entry of 0 contributes exactly 0
__host__ __device__ __forceinline__ float loss_xlogy(float t) { return t == 0.f ? 0.f : t * logf(t); }

// One entry of a policy row: xlogy(t, t) - t * logp, exactly 0 where t == 0
// (F.kl_div, also where logp = -inf)
__host__ __device__ __forceinline__ float loss_kl_entry(float t, float logp) {
  return t == 0.f ? 0.f : loss_xlogy(t) - t * logp;
}

// Value term of one row: loss w (h(v) - h(t))^2 (or w (v - t)^2), *g = d loss / d v
__host__ __device__ __forceinline__ float loss_value_term(float v, float t, float w, int transform, float* g) {
  const float d = transform ? loss_transform(v) - loss_transform(t) : v - t;
  const float dh = transform ? loss_transform_grad(v) : 1.f;
  *g = w * (2.f * d) * dh;
  return w * (d * d);
}
// Reward term of one row: loss w (r - t)^2, *g = d loss / d r
__host__ __device__ __forceinline__ float loss_reward_term(float r, float t, float w, float* g) {
  const float d = r - t;
  *g = w * (2.f * d);
  return w * (d * d);
}

// mzgo_capi.hip: set mzgo_last_error()'s text and return ``code``
int set_error(int code, const char* fmt, ...);

}  // namespace mzgo
