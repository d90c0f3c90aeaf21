// mzgo_ownership.hpp -- the scalar pieces of the ownership loss
// (mzgo_ownership.hip: the kernels and mzgo_ownership_loss_host run this text,
// so the formulas a CPU test checks are the kernels').
//
// The head is a 1x1 conv from the latent to one plane, x = sum_ch w[ch] lat[ch]
// + bias per cell, read as tanh(x) in [-1, 1]: +1 the mover owns the point, -1
// the opponent does.  The loss of a cell against its target t in {-1, 0, +1} is
// the cross entropy of (1 + tanh x) / 2 against (1 + t) / 2 (KataGo's ownership
// loss), up to a constant of t, in the form that cannot overflow:
//   l(x, t) = softplus(2 x) - (1 + t) x,  softplus(z) = max(z, 0) + log1p(exp(-|z|))
// whose derivative in x is exactly tanh(x) - t.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

namespace mzgo {

// l(x, t); *g = d l / d x = tanh(x) - t
__host__ __device__ __forceinline__ float own_loss_term(float x, float t, float* g) {
  const float z = 2.f * x;
  const float softplus = fmaxf(z, 0.f) + log1pf(expf(-fabsf(z)));
  *g = tanhf(x) - t;
  return softplus - (1.f + t) * x;
}
// what a row's cell gradients are scaled by: weight * mask / CELLS, in float32
__host__ __device__ __forceinline__ float own_row_scale(float weight, float mask, int CELLS) {
  return (weight * mask) / (float)CELLS;
}
// a row's share of its sample's loss from the f64 sum of its cells' terms
__host__ __device__ __forceinline__ double own_row_loss(float weight, float mask, int CELLS, double cell_sum) {
  return ((double)weight * (double)mask) * (cell_sum / (double)CELLS);
}

// The caller-owned workspace of a forward / backward pair, in doubles: the
// rows' losses [(K+1) B], then a row of C + 1 partial sums per (step, sample)
// for the head's weight (C) and bias (1).
__host__ __device__ __forceinline__ size_t own_work_rows(int B, int K) { return (((size_t)K + 1) * B + 7) / 8 * 8; }
__host__ __device__ __forceinline__ size_t own_work_doubles(int B, int K, int C) {
  return own_work_rows(B, K) + ((size_t)K + 1) * B * ((size_t)C + 1);
}

}  // namespace mzgo
