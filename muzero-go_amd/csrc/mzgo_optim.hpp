// mzgo_optim.hpp -- the scalar pieces of the device optimizer (mzgo_optim.hip:
// mzgo_optim_step and its host twin run this text, so the formulas a CPU test
// checks are the kernels'): torch's clip_grad_norm_ coefficient, StepLR's
// closed form, Adam's bias corrections and the elementwise Adam / AdamW update
// (torch/optim/adam.py, _single_tensor_adam), in f64 on f32 state.
//
// Only + - * / and sqrt of f64 are used (every one correctly rounded on the
// host and on the device, and the units are compiled with -ffp-contract=off),
// so the two sides give the same bits; the powers are integer powers by
// repeated squaring for that reason, not pow().
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/mzgo.h"

namespace mzgo {

constexpr int kOptimThreads = 256;                     // a workgroup of the chunk kernels
constexpr int kOptimPerThread = 4;                     // consecutive floats of a thread: one 16-byte access
constexpr int kOptimChunk = kOptimThreads * kOptimPerThread;   // elements of a (tensor, chunk) segment

// b ** e for e >= 0 by squaring, left to right in the bits of e from the lowest
__host__ __device__ __forceinline__ double optim_ipow(double b, int64_t e) {
  double r = 1.0;
  while (e > 0) {
    if (e & 1) r *= b;
    e >>= 1;
    if (e) b *= b;
  }
  return r;
}

// clip_grad_norm_: min(1, max_norm / (norm + 1e-6)), rounded to f32 once;
// max_norm <= 0 means no clipping
__host__ __device__ __forceinline__ float optim_coef(double norm, double max_norm) {
  if (!(max_norm > 0.0)) return 1.f;
  const double c = max_norm / (norm + 1e-6);
  return (float)(c < 1.0 ? c : 1.0);
}

// StepLR after ``sched`` scheduler steps: lr0 * gamma ** (sched / step_size)
__host__ __device__ __forceinline__ double optim_lr(const mzgo_optim_hyper& h, int64_t sched) {
  return h.lr0 * optim_ipow(h.gamma, sched / h.step_size);
}

// 1 - beta ** step
__host__ __device__ __forceinline__ double optim_bias_correction(double beta, int64_t step) {
  return 1.0 - optim_ipow(beta, step);
}

// What one tensor's elements share in a step
struct OptimConsts {
  float coef;
  int decoupled;
  double wd, omb1, b2, omb2, decay, step_size, sqrt_bc2, eps;
};
__host__ __device__ __forceinline__ OptimConsts optim_consts(const mzgo_optim_hyper& h, float coef, double lr,
                                                             double bc1, double bc2) {
  OptimConsts c;
  c.coef = coef;
  c.decoupled = h.decoupled != 0;
  c.wd = h.weight_decay;
  c.omb1 = 1.0 - h.beta1;
  c.b2 = h.beta2;
  c.omb2 = 1.0 - h.beta2;
  c.decay = 1.0 - lr * h.weight_decay;
  c.step_size = lr / bc1;
  c.sqrt_bc2 = sqrt(bc2);
  c.eps = h.eps;
  return c;
}

// One element: g is only read (the clipped gradient is not written back)
__host__ __device__ __forceinline__ void optim_update(const OptimConsts& c, float g, float* p_, float* m_, float* v_) {
  double p = (double)*p_;
  const double m = (double)*m_, v = (double)*v_;
  double gc = (double)(g * c.coef);                    // the gradient as torch leaves it after the clip
  if (c.wd != 0.0 && !c.decoupled) gc += c.wd * p;
  const double m1 = m + (gc - m) * c.omb1;             // exp_avg.lerp_(grad, 1 - beta1)
  const double v1 = c.b2 * v + c.omb2 * gc * gc;       // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, 1 - beta2)
  if (c.wd != 0.0 && c.decoupled) p *= c.decay;
  const double p1 = p - c.step_size * m1 / (sqrt(v1) / c.sqrt_bc2 + c.eps);
  *p_ = (float)p1;
  *m_ = (float)m1;
  *v_ = (float)v1;
}

// A thread's share of a chunk's sum of squares, in element order
__host__ __device__ __forceinline__ double optim_sumsq(const float x[kOptimPerThread]) {
  double s = 0.0;
  for (int k = 0; k < kOptimPerThread; ++k) s += (double)x[k] * (double)x[k];
  return s;
}

// mzgo_capi.hip: set mzgo_last_error()'s text and return ``code``
int set_error(int code, const char* fmt, ...);

}  // namespace mzgo
