// mzgo_loss.hip -- the trainer's unroll loss in one launch (mzgo.h:
// mzgo_unroll_loss, mzgo_unroll_loss_host).
//
// main.py:431-482 forms the loss of a trajectory step by step from small
// torch ops (log_softmax, kl_div, two value transforms, two mse_loss, the
// weights and sums); mzgo.trainer's batched step repeats that for B samples,
// K + 1 times.  Here the whole unroll's per-sample losses, the per-term totals
// and the gradients with respect to every head output come from one kernel,
// k_unroll_loss, and a one-workgroup reduction, k_unroll_loss_totals.
//
//   k_unroll_loss         a workgroup per sample, a wave per row (b, k): the
//                         row's max, sum of exponentials, target sum and KL
//                         sum are wave reductions; the value and reward terms
//                         are scalars of the row.  The sample's sum over k is
//                         formed by thread 0 in k order from LDS.
//   k_unroll_loss_totals  the B per-sample parts summed in f64 in a fixed
//                         order (a strided pass per thread, then a tree in
//                         LDS): two calls give the same bits.
//
// Plain vector loads and stores only; no atomics; workgroups never
// communicate.  expf / logf / sqrtf are the library's full-precision ones.
// Compiled with -ffp-contract=off like every unit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>

#include "../../include/mzgo.h"
#include "mzgo_loss.hpp"

using namespace mzgo;

#define LHIPCHK(expr)                                                                              \
  do {                                                                                             \
    hipError_t e_ = (expr);                                                                        \
    if (e_ != hipSuccess) return set_error(MZGO_EHIP, "%s: %s", #expr, hipGetErrorString(e_));     \
  } while (0)

namespace {

constexpr int kWaves = 8;                              // rows of one sample in flight
constexpr int kThreads = 64 * kWaves;
constexpr int kPasses = (kLossMaxA + 63) / 64;         // 6: a lane holds entries lane, lane + 64, ...
constexpr int kTotalsThreads = 256;

// butterfly over the 64 lanes: every lane ends with the same value, and the
// order of the additions does not depend on anything but the lane count
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

struct LossArgs {
  const float* logits;   // [K+1][B][A]
  const float* value;    // [K+1][B]
  const float* reward;   // [K][B]      (null when K == 0)
  const float* t_pol;    // [B][K+1][A]
  const float* t_val;    // [B][K+1]
  const float* t_rew;    // [B][K]      (null when K == 0)
  int B, K, A;
  float w_value, w_policy, w_reward;
  int transform;
  float* per_sample;     // [B]
  double* part;          // [B][3] value, policy, reward parts of a sample
  float* g_logits;       // [K+1][B][A]
  float* g_value;        // [K+1][B]
  float* g_reward;       // [K][B]      (null when K == 0)
};

__global__ void __launch_bounds__(kThreads) k_unroll_loss(LossArgs P) {
  __shared__ float term[kWaves][3];                    // a round's rows: value, policy, reward terms
  const int b = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int B = P.B, K = P.K, A = P.A;
  float per = 0.f;                                     // thread 0 only
  double sum_v = 0.0, sum_p = 0.0, sum_r = 0.0;

  for (int k0 = 0; k0 <= K; k0 += kWaves) {
    const int k = k0 + w;
    if (k <= K) {                                      // wave-uniform
      const size_t lrow = ((size_t)k * B + b) * A, trow = ((size_t)b * (K + 1) + k) * A;
      float x[kPasses], t[kPasses];
      float m = -INFINITY;
#pragma unroll
      for (int j = 0; j < kPasses; ++j) {
        const int a = lane + 64 * j;
        const bool in = a < A;
        x[j] = in ? P.logits[lrow + a] : -INFINITY;
        t[j] = in ? P.t_pol[trow + a] : 0.f;
        m = fmaxf(m, x[j]);
      }
      m = wave_max(m);
      float e[kPasses], s = 0.f, tsum = 0.f;
#pragma unroll
      for (int j = 0; j < kPasses; ++j) {
        e[j] = lane + 64 * j < A ? expf(x[j] - m) : 0.f;
        s += e[j];
        tsum += t[j];
      }
      s = wave_sum(s);
      tsum = wave_sum(tsum);
      const float log_s = logf(s);
      float kl = 0.f;
#pragma unroll
      for (int j = 0; j < kPasses; ++j) {
        const int a = lane + 64 * j;
        if (a < A) {
          kl += loss_kl_entry(t[j], (x[j] - m) - log_s);
          P.g_logits[lrow + a] = P.w_policy * ((e[j] / s) * tsum - t[j]);
        }
      }
      kl = wave_sum(kl);
      if (lane == 0) {
        const size_t vi = (size_t)k * B + b;
        float gv, gr = 0.f, r_l = 0.f;
        const float v_l = loss_value_term(P.value[vi], P.t_val[(size_t)b * (K + 1) + k], P.w_value, P.transform, &gv);
        P.g_value[vi] = gv;
        if (k >= 1) {
          const size_t ri = (size_t)(k - 1) * B + b;
          r_l = loss_reward_term(P.reward[ri], P.t_rew[(size_t)b * K + (k - 1)], P.w_reward, &gr);
          P.g_reward[ri] = gr;
        }
        term[w][0] = v_l;
        term[w][1] = P.w_policy * kl;
        term[w][2] = r_l;
      }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      const int n = min(kWaves, K + 1 - k0);
      for (int i = 0; i < n; ++i) {                    // _unroll_step's order: per + r_l + v_l + p_l
        const float v_l = term[i][0], p_l = term[i][1], r_l = term[i][2];
        per = k0 + i == 0 ? v_l + p_l : ((per + r_l) + v_l) + p_l;
        sum_v += (double)v_l;
        sum_p += (double)p_l;
        sum_r += (double)r_l;
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    P.per_sample[b] = per;
    P.part[(size_t)b * 3] = sum_v;
    P.part[(size_t)b * 3 + 1] = sum_p;
    P.part[(size_t)b * 3 + 2] = sum_r;
  }
}

// totals[0..3] = sum over b of per_sample, value, policy, reward parts, in f64
__global__ void __launch_bounds__(kTotalsThreads) k_unroll_loss_totals(const float* per_sample, const double* part,
                                                                      int B, double* totals) {
  __shared__ double acc[kTotalsThreads][4];
  const int tid = threadIdx.x;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (int b = tid; b < B; b += kTotalsThreads) {
    s[0] += (double)per_sample[b];
    s[1] += part[(size_t)b * 3];
    s[2] += part[(size_t)b * 3 + 1];
    s[3] += part[(size_t)b * 3 + 2];
  }
  for (int i = 0; i < 4; ++i) acc[tid][i] = s[i];
  __syncthreads();
  for (int o = kTotalsThreads / 2; o > 0; o >>= 1) {
    if (tid < o)
      for (int i = 0; i < 4; ++i) acc[tid][i] += acc[tid + o][i];
    __syncthreads();
  }
  if (tid < 4) totals[tid] = acc[0][tid];
}

// The per-sample parts between the two launches: one buffer per device, grown
// on demand (never inside a stream capture at the sizes a trainer uses: the
// first call allocates room for kPartMin samples).
constexpr int kMaxDevices = 64;
constexpr size_t kPartMin = 4096;
std::mutex g_part_lock;
double* g_part[kMaxDevices];
size_t g_part_cap[kMaxDevices];

int part_room(size_t B, hipStream_t s, double** out) {
  int dev = 0;
  LHIPCHK(hipGetDevice(&dev));
  if (dev < 0 || dev >= kMaxDevices) return set_error(MZGO_EINVAL, "mzgo_unroll_loss: device %d (0..%d)", dev, kMaxDevices - 1);
  std::lock_guard<std::mutex> hold(g_part_lock);
  if (B > g_part_cap[dev]) {
    if (g_part[dev]) {
      LHIPCHK(hipStreamSynchronize(s));                // (a launch may still read the old buffer)
      LHIPCHK(hipFree(g_part[dev]));
      g_part[dev] = nullptr;
      g_part_cap[dev] = 0;
    }
    const size_t cap = std::max(B, kPartMin);
    LHIPCHK(hipMalloc((void**)&g_part[dev], cap * 3 * sizeof(double)));
    g_part_cap[dev] = cap;
  }
  *out = g_part[dev];
  return MZGO_OK;
}

int check_args(const char* fn, const void* logits, const void* value, const void* reward, const void* t_pol,
               const void* t_val, const void* t_rew, int B, int K, int A, const void* per_sample, const void* totals,
               const void* g_logits, const void* g_value, const void* g_reward) {
  if (B < 1) return set_error(MZGO_EINVAL, "%s: B must be >= 1, got %d", fn, B);
  if (K < 0) return set_error(MZGO_EINVAL, "%s: K must be >= 0, got %d", fn, K);
  if (A < kLossMinA || A > kLossMaxA)
    return set_error(MZGO_EINVAL, "%s: A %d out of range (%d..%d)", fn, A, kLossMinA, kLossMaxA);
  const char* null = !logits ? "logits" : !value ? "value" : !t_pol ? "t_pol" : !t_val ? "t_val"
                     : !per_sample ? "per_sample" : !totals ? "totals" : !g_logits ? "g_logits"
                     : !g_value ? "g_value" : nullptr;
  if (!null && K > 0) null = !reward ? "reward" : !t_rew ? "t_rew" : !g_reward ? "g_reward" : nullptr;
  if (null) return set_error(MZGO_EINVAL, "%s: null %s", fn, null);
  return MZGO_OK;
}

}  // namespace

extern "C" {

int mzgo_unroll_loss(const float* logits, const float* value, const float* reward, const float* t_pol,
                     const float* t_val, const float* t_rew, int B, int K, int A, float w_value, float w_policy,
                     float w_reward, int value_transform, float* per_sample, double* totals, float* g_logits,
                     float* g_value, float* g_reward, void* stream) {
  if (int rc = check_args("mzgo_unroll_loss", logits, value, reward, t_pol, t_val, t_rew, B, K, A, per_sample, totals,
                          g_logits, g_value, g_reward))
    return rc;
  hipStream_t s = (hipStream_t)stream;
  double* part = nullptr;
  if (int rc = part_room((size_t)B, s, &part)) return rc;
  const LossArgs P{logits, value, reward, t_pol, t_val, t_rew, B, K, A, w_value, w_policy, w_reward,
                   value_transform != 0, per_sample, part, g_logits, g_value, g_reward};
  hipLaunchKernelGGL(k_unroll_loss, dim3((unsigned)B), dim3(kThreads), 0, s, P);
  LHIPCHK(hipGetLastError());
  hipLaunchKernelGGL(k_unroll_loss_totals, dim3(1), dim3(kTotalsThreads), 0, s, per_sample, part, B, totals);
  LHIPCHK(hipGetLastError());
  return MZGO_OK;
}

int mzgo_unroll_loss_host(const float* logits, const float* value, const float* reward, const float* t_pol,
                          const float* t_val, const float* t_rew, int B, int K, int A, float w_value, float w_policy,
                          float w_reward, int value_transform, float* per_sample, double* totals, float* g_logits,
                          float* g_value, float* g_reward) {
  if (int rc = check_args("mzgo_unroll_loss_host", logits, value, reward, t_pol, t_val, t_rew, B, K, A, per_sample,
                          totals, g_logits, g_value, g_reward))
    return rc;
  const int transform = value_transform != 0;
  double tot[4] = {0.0, 0.0, 0.0, 0.0};
  for (int b = 0; b < B; ++b) {
    float per = 0.f;
    for (int k = 0; k <= K; ++k) {
      const float* x = logits + ((size_t)k * B + b) * A;
      const float* t = t_pol + ((size_t)b * (K + 1) + k) * A;
      float* g = g_logits + ((size_t)k * B + b) * A;
      float m = -INFINITY, s = 0.f, tsum = 0.f, kl = 0.f;
      for (int a = 0; a < A; ++a) m = fmaxf(m, x[a]);
      for (int a = 0; a < A; ++a) {
        s += expf(x[a] - m);
        tsum += t[a];
      }
      const float log_s = logf(s);
      for (int a = 0; a < A; ++a) {
        kl += loss_kl_entry(t[a], (x[a] - m) - log_s);
        g[a] = w_policy * ((expf(x[a] - m) / s) * tsum - t[a]);
      }
      const size_t vi = (size_t)k * B + b;
      float r_l = 0.f;
      const float v_l = loss_value_term(value[vi], t_val[(size_t)b * (K + 1) + k], w_value, transform, &g_value[vi]);
      if (k >= 1) {
        const size_t ri = (size_t)(k - 1) * B + b;
        r_l = loss_reward_term(reward[ri], t_rew[(size_t)b * K + (k - 1)], w_reward, &g_reward[ri]);
      }
      const float p_l = w_policy * kl;
      per = k == 0 ? v_l + p_l : ((per + r_l) + v_l) + p_l;
      tot[1] += (double)v_l;
      tot[2] += (double)p_l;
      tot[3] += (double)r_l;
    }
    per_sample[b] = per;
    tot[0] += (double)per;
  }
  for (int i = 0; i < 4; ++i) totals[i] = tot[i];
  return MZGO_OK;
}

}  // extern "C"
