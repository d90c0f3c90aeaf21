// mzgo_optim.hip -- the trainer's optimizer tail in one call (mzgo.h:
// mzgo_optim_step, mzgo_optim_step_host).
//
// main.py:481-484 clips the gradient norm, steps Adam and (main.py:379) StepLR
// with torch ops over every parameter tensor: some two dozen small launches.
// Here the n tensors are cut once, at creation, into (tensor, chunk) segments
// of kOptimChunk elements, and a step is three launches on the caller's stream:
//
//   k_optim_sumsq   a workgroup per segment: a thread squares its four
//                   consecutive gradient entries in f64 and sums them in order,
//                   a tree in LDS sums the 256 threads; one f64 partial per
//                   segment, in the segment's own slot.
//   k_optim_record  one workgroup: the partials summed in index order (staged
//                   through LDS a tile at a time, added by thread 0), the norm,
//                   the clip coefficient, the learning rate, the refusal of a
//                   non-finite norm, the counters and every tensor's step count
//                   and bias corrections.
//   k_optim_apply   a workgroup per segment again: Adam's update in f64 on the
//                   f32 values; returns at once when the step was refused.
//
// The tensors' addresses reach the kernels by value, kOptimBlock tensors per
// launch (the gradients are fresh tensors every step, so there is no table in
// device memory that a step still in flight could be reading while the next
// one is written): n > kOptimBlock takes one sumsq and one apply launch per
// block of tensors.  Pointers need only f32 alignment: a segment uses 16-byte
// accesses when all of its addresses allow them and single floats otherwise,
// the same elements per thread, so the bits do not depend on the alignment.
// Plain vector loads and stores only; no atomics; workgroups never communicate
// within a launch.  Compiled with -ffp-contract=off like every unit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/mzgo.h"
#include "mzgo_optim.hpp"

using namespace mzgo;

#define OHIPCHK(expr)                                                                              \
  do {                                                                                             \
    hipError_t e_ = (expr);                                                                        \
    if (e_ != hipSuccess) return set_error(MZGO_EHIP, "%s: %s", #expr, hipGetErrorString(e_));     \
  } while (0)

namespace {

constexpr int kOptimBlock = 96;                        // tensors whose addresses one launch carries (4 x 768 B)
constexpr int kRecordTile = 1024;                      // partials staged in LDS at a time

struct GradBlock {
  const float* g[kOptimBlock];
};
struct TensorBlock {
  float* p[kOptimBlock];
  const float* g[kOptimBlock];
  float* m[kOptimBlock];
  float* v[kOptimBlock];
};
// the segment table: segment c belongs to tensor seg_tensor[c] and starts at
// element (c - first[t]) * kOptimChunk of its numel[t]
struct Segments {
  const int32_t* seg_tensor;   // [chunks]
  const int64_t* first;        // [n + 1]
  const int64_t* numel;        // [n]
};

__device__ __forceinline__ bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// elements e .. e + 3 of a segment of cnt elements; 0 past its end
__device__ __forceinline__ void load4(const float* base, int e, int cnt, bool vec, float x[kOptimPerThread]) {
  if (vec && e + kOptimPerThread <= cnt) {
    const float4 q = *reinterpret_cast<const float4*>(base + e);
    x[0] = q.x; x[1] = q.y; x[2] = q.z; x[3] = q.w;
  } else {
#pragma unroll
    for (int k = 0; k < kOptimPerThread; ++k) x[k] = e + k < cnt ? base[e + k] : 0.f;
  }
}
__device__ __forceinline__ void store4(float* base, int e, int cnt, bool vec, const float x[kOptimPerThread]) {
  if (vec && e + kOptimPerThread <= cnt) {
    *reinterpret_cast<float4*>(base + e) = make_float4(x[0], x[1], x[2], x[3]);
  } else {
#pragma unroll
    for (int k = 0; k < kOptimPerThread; ++k)
      if (e + k < cnt) base[e + k] = x[k];
  }
}

__global__ void __launch_bounds__(kOptimThreads) k_optim_sumsq(GradBlock G, Segments S, int t0, int64_t c0,
                                                               double* partial, int* has_grad) {
  __shared__ double acc[kOptimThreads];
  const int tid = threadIdx.x;
  const int64_t c = c0 + blockIdx.x;
  const int t = S.seg_tensor[c];
  const float* g = G.g[t - t0];
  const int64_t off = (c - S.first[t]) * kOptimChunk;
  if (tid == 0 && off == 0) has_grad[t] = g != nullptr;
  if (!g) {                                            // (workgroup-uniform)
    if (tid == 0) partial[c] = 0.0;
    return;
  }
  const int64_t left = S.numel[t] - off;
  const int cnt = left < kOptimChunk ? (int)left : kOptimChunk;
  float x[kOptimPerThread];
  load4(g + off, tid * kOptimPerThread, cnt, aligned16(g + off), x);
  acc[tid] = optim_sumsq(x);
  __syncthreads();
  for (int o = kOptimThreads / 2; o > 0; o >>= 1) {
    if (tid < o) acc[tid] += acc[tid + o];
    __syncthreads();
  }
  if (tid == 0) partial[c] = acc[0];
}

__global__ void __launch_bounds__(kOptimThreads) k_optim_record(const double* partial, int64_t chunks, int n,
                                                                const int* has_grad, mzgo_optim_hyper H,
                                                                int64_t* steps, int64_t* counts, double* bc,
                                                                double* record) {
  __shared__ double tile[kRecordTile];
  __shared__ int s_applied;
  const int tid = threadIdx.x;
  double sum = 0.0;                                    // thread 0 only
  for (int64_t base = 0; base < chunks; base += kRecordTile) {
    const int cnt = (int)(chunks - base < kRecordTile ? chunks - base : kRecordTile);
    for (int i = tid; i < cnt; i += kOptimThreads) tile[i] = partial[base + i];
    __syncthreads();
    if (tid == 0)
      for (int i = 0; i < cnt; ++i) sum += tile[i];
    __syncthreads();
  }
  if (tid == 0) {
    const double norm = sqrt(sum);
    const int applied = isfinite(norm) ? 1 : 0;
    const int64_t sched = counts[0];
    record[0] = norm;
    record[1] = (double)optim_coef(norm, H.max_norm);
    record[2] = optim_lr(H, sched);
    record[3] = (double)applied;
    counts[0] = sched + 1;
    if (!applied) counts[1] += 1;
    s_applied = applied;
  }
  __syncthreads();
  if (!s_applied) return;
  for (int t = tid; t < n; t += kOptimThreads) {
    if (!has_grad[t]) continue;
    const int64_t st = steps[t] + 1;
    steps[t] = st;
    bc[2 * t] = optim_bias_correction(H.beta1, st);
    bc[2 * t + 1] = optim_bias_correction(H.beta2, st);
  }
}

__global__ void __launch_bounds__(kOptimThreads) k_optim_apply(TensorBlock T, Segments S, int t0, int64_t c0,
                                                               mzgo_optim_hyper H, const double* bc,
                                                               const double* record) {
  if (record[3] == 0.0) return;                        // the step was refused
  const int tid = threadIdx.x;
  const int64_t c = c0 + blockIdx.x;
  const int t = S.seg_tensor[c];
  const float* g = T.g[t - t0];
  if (!g) return;
  const int64_t off = (c - S.first[t]) * kOptimChunk;
  const int64_t left = S.numel[t] - off;
  const int cnt = left < kOptimChunk ? (int)left : kOptimChunk;
  const int e = tid * kOptimPerThread;
  if (e >= cnt) return;
  g += off;
  float* p = T.p[t - t0] + off;
  float* m = T.m[t - t0] + off;
  float* v = T.v[t - t0] + off;
  const bool vec = aligned16(g) && aligned16(p) && aligned16(m) && aligned16(v);
  const OptimConsts C = optim_consts(H, (float)record[1], record[2], bc[2 * t], bc[2 * t + 1]);
  float xg[kOptimPerThread], xp[kOptimPerThread], xm[kOptimPerThread], xv[kOptimPerThread];
  load4(g, e, cnt, vec, xg);
  load4(p, e, cnt, vec, xp);
  load4(m, e, cnt, vec, xm);
  load4(v, e, cnt, vec, xv);
#pragma unroll
  for (int k = 0; k < kOptimPerThread; ++k) optim_update(C, xg[k], &xp[k], &xm[k], &xv[k]);
  store4(p, e, cnt, vec, xp);
  store4(m, e, cnt, vec, xm);
  store4(v, e, cnt, vec, xv);
}

int check_numels(const char* fn, int n, const int64_t* numels) {
  if (n < 1) return set_error(MZGO_EINVAL, "%s: n must be >= 1, got %d", fn, n);
  if (!numels) return set_error(MZGO_EINVAL, "%s: null numels", fn);
  for (int i = 0; i < n; ++i)
    if (numels[i] < 0)
      return set_error(MZGO_EINVAL, "%s: numels[%d] must be >= 0, got %lld", fn, i, (long long)numels[i]);
  return MZGO_OK;
}

int check_hyper(const char* fn, const mzgo_optim_hyper* h) {
  if (!h) return set_error(MZGO_EINVAL, "%s: null hyper", fn);
  if (!(h->lr0 >= 0.0) || !std::isfinite(h->lr0))
    return set_error(MZGO_EINVAL, "%s: lr0 must be finite and >= 0, got %g", fn, h->lr0);
  if (!(h->beta1 >= 0.0 && h->beta1 < 1.0))
    return set_error(MZGO_EINVAL, "%s: beta1 must be in [0, 1), got %g", fn, h->beta1);
  if (!(h->beta2 >= 0.0 && h->beta2 < 1.0))
    return set_error(MZGO_EINVAL, "%s: beta2 must be in [0, 1), got %g", fn, h->beta2);
  if (!(h->eps > 0.0) || !std::isfinite(h->eps))
    return set_error(MZGO_EINVAL, "%s: eps must be finite and > 0, got %g", fn, h->eps);
  if (!(h->weight_decay >= 0.0) || !std::isfinite(h->weight_decay))
    return set_error(MZGO_EINVAL, "%s: weight_decay must be finite and >= 0, got %g", fn, h->weight_decay);
  if (h->max_norm != h->max_norm) return set_error(MZGO_EINVAL, "%s: max_norm is NaN", fn);
  if (h->step_size < 1)
    return set_error(MZGO_EINVAL, "%s: step_size must be >= 1, got %lld", fn, (long long)h->step_size);
  if (!(h->gamma >= 0.0) || !std::isfinite(h->gamma))
    return set_error(MZGO_EINVAL, "%s: gamma must be finite and >= 0, got %g", fn, h->gamma);
  return MZGO_OK;
}

int check_tables(const char* fn, int n, float* const* params, const float* const* grads, float* const* exp_avg,
                 float* const* exp_avg_sq) {
  const char* null = !params ? "params" : !grads ? "grads" : !exp_avg ? "exp_avg" : !exp_avg_sq ? "exp_avg_sq"
                     : nullptr;
  if (null) return set_error(MZGO_EINVAL, "%s: null %s table", fn, null);
  for (int i = 0; i < n; ++i) {
    null = !params[i] ? "params" : !exp_avg[i] ? "exp_avg" : !exp_avg_sq[i] ? "exp_avg_sq" : nullptr;
    if (null) return set_error(MZGO_EINVAL, "%s: null %s[%d]", fn, null, i);
  }
  return MZGO_OK;
}

// chunks of a tensor: an empty one keeps a single empty chunk, so that every
// tensor owns a segment (the one that reports whether it has a gradient)
int64_t chunks_of(int64_t numel) { return std::max<int64_t>(1, (numel + kOptimChunk - 1) / kOptimChunk); }

}  // namespace

struct mzgo_optim {
  int device = 0, n = 0;
  int64_t chunks = 0;
  std::vector<int64_t> first;     // [n + 1] host copy of the table's prefix
  int32_t* seg_tensor = nullptr;
  int64_t* d_first = nullptr;
  int64_t* d_numel = nullptr;
  double* partial = nullptr;      // [chunks]
  int* has_grad = nullptr;        // [n]
  int64_t* steps = nullptr;       // [n]
  int64_t* counts = nullptr;      // scheduler count, skipped steps
  double* bc = nullptr;           // [n][2] bias corrections of the step in flight
  double* record = nullptr;       // [4]
  ~mzgo_optim() {
    for (void* p : {(void*)seg_tensor, (void*)d_first, (void*)d_numel, (void*)partial, (void*)has_grad, (void*)steps,
                    (void*)counts, (void*)bc, (void*)record})
      if (p) (void)hipFree(p);
  }
};

extern "C" {

int mzgo_optim_chunk(void) { return kOptimChunk; }

int mzgo_optim_create(int n, const int64_t* numels, int device, mzgo_optim** out) {
  if (!out) return set_error(MZGO_EINVAL, "mzgo_optim_create: null out");
  *out = nullptr;
  if (int rc = check_numels("mzgo_optim_create", n, numels)) return rc;
  std::vector<int64_t> first(n + 1, 0);
  for (int i = 0; i < n; ++i) {
    first[i + 1] = first[i] + chunks_of(numels[i]);
    if (first[i + 1] > INT32_MAX)
      return set_error(MZGO_EINVAL, "mzgo_optim_create: more than 2^31 - 1 chunks of %d elements", kOptimChunk);
  }
  const int64_t chunks = first[n];
  std::vector<int32_t> seg((size_t)chunks);
  for (int i = 0; i < n; ++i)
    for (int64_t c = first[i]; c < first[i + 1]; ++c) seg[(size_t)c] = i;
  OHIPCHK(hipSetDevice(device));
  mzgo_optim* o = new mzgo_optim;
  o->device = device;
  o->n = n;
  o->chunks = chunks;
  o->first = first;
  hipError_t e = hipSuccess;
  auto chk = [&](hipError_t x) { if (e == hipSuccess) e = x; };
  chk(hipMalloc((void**)&o->seg_tensor, (size_t)chunks * sizeof(int32_t)));
  chk(hipMalloc((void**)&o->d_first, (size_t)(n + 1) * sizeof(int64_t)));
  chk(hipMalloc((void**)&o->d_numel, (size_t)n * sizeof(int64_t)));
  chk(hipMalloc((void**)&o->partial, (size_t)chunks * sizeof(double)));
  chk(hipMalloc((void**)&o->has_grad, (size_t)n * sizeof(int)));
  chk(hipMalloc((void**)&o->steps, (size_t)n * sizeof(int64_t)));
  chk(hipMalloc((void**)&o->counts, 2 * sizeof(int64_t)));
  chk(hipMalloc((void**)&o->bc, (size_t)n * 2 * sizeof(double)));
  chk(hipMalloc((void**)&o->record, 4 * sizeof(double)));
  if (e == hipSuccess) {
    chk(hipMemcpy(o->seg_tensor, seg.data(), (size_t)chunks * sizeof(int32_t), hipMemcpyHostToDevice));
    chk(hipMemcpy(o->d_first, first.data(), (size_t)(n + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
    chk(hipMemcpy(o->d_numel, numels, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice));
    chk(hipMemset(o->partial, 0, (size_t)chunks * sizeof(double)));
    chk(hipMemset(o->has_grad, 0, (size_t)n * sizeof(int)));
    chk(hipMemset(o->steps, 0, (size_t)n * sizeof(int64_t)));
    chk(hipMemset(o->counts, 0, 2 * sizeof(int64_t)));
    chk(hipMemset(o->bc, 0, (size_t)n * 2 * sizeof(double)));
    chk(hipMemset(o->record, 0, 4 * sizeof(double)));
    chk(hipDeviceSynchronize());                       // (the null stream's memsets before any caller's stream)
  }
  if (e != hipSuccess) {
    delete o;
    return set_error(MZGO_EHIP, "mzgo_optim_create: %s", hipGetErrorString(e));
  }
  *out = o;
  return MZGO_OK;
}

void mzgo_optim_destroy(mzgo_optim* opt) { delete opt; }

int mzgo_optim_step(mzgo_optim* o, float* const* params, const float* const* grads, float* const* exp_avg,
                    float* const* exp_avg_sq, const mzgo_optim_hyper* hyper, void* stream) {
  if (!o) return set_error(MZGO_EINVAL, "mzgo_optim_step: null optimizer");
  if (int rc = check_tables("mzgo_optim_step", o->n, params, grads, exp_avg, exp_avg_sq)) return rc;
  if (int rc = check_hyper("mzgo_optim_step", hyper)) return rc;
  hipStream_t s = (hipStream_t)stream;
  const Segments S{o->seg_tensor, o->d_first, o->d_numel};
  const int n = o->n;
  for (int t0 = 0; t0 < n; t0 += kOptimBlock) {
    const int t1 = std::min(n, t0 + kOptimBlock);
    GradBlock G{};
    for (int t = t0; t < t1; ++t) G.g[t - t0] = grads[t];
    const int64_t c0 = o->first[t0], c1 = o->first[t1];
    hipLaunchKernelGGL(k_optim_sumsq, dim3((unsigned)(c1 - c0)), dim3(kOptimThreads), 0, s, G, S, t0, c0, o->partial,
                       o->has_grad);
    OHIPCHK(hipGetLastError());
  }
  hipLaunchKernelGGL(k_optim_record, dim3(1), dim3(kOptimThreads), 0, s, o->partial, o->chunks, n, o->has_grad, *hyper,
                     o->steps, o->counts, o->bc, o->record);
  OHIPCHK(hipGetLastError());
  for (int t0 = 0; t0 < n; t0 += kOptimBlock) {
    const int t1 = std::min(n, t0 + kOptimBlock);
    TensorBlock T{};
    for (int t = t0; t < t1; ++t) {
      T.p[t - t0] = params[t];
      T.g[t - t0] = grads[t];
      T.m[t - t0] = exp_avg[t];
      T.v[t - t0] = exp_avg_sq[t];
    }
    const int64_t c0 = o->first[t0], c1 = o->first[t1];
    hipLaunchKernelGGL(k_optim_apply, dim3((unsigned)(c1 - c0)), dim3(kOptimThreads), 0, s, T, S, t0, c0, *hyper,
                       o->bc, o->record);
    OHIPCHK(hipGetLastError());
  }
  return MZGO_OK;
}

int mzgo_optim_record(mzgo_optim* o, double** dev_ptr) {
  if (!o || !dev_ptr) return set_error(MZGO_EINVAL, "mzgo_optim_record: null %s", !o ? "optimizer" : "dev_ptr");
  *dev_ptr = o->record;
  return MZGO_OK;
}

int mzgo_optim_counts(mzgo_optim* o, int64_t* steps_host, int64_t* sched, int64_t* skipped, void* stream) {
  if (!o) return set_error(MZGO_EINVAL, "mzgo_optim_counts: null optimizer");
  hipStream_t s = (hipStream_t)stream;
  int64_t counts[2] = {0, 0};
  if (steps_host)
    OHIPCHK(hipMemcpyAsync(steps_host, o->steps, (size_t)o->n * sizeof(int64_t), hipMemcpyDeviceToHost, s));
  OHIPCHK(hipMemcpyAsync(counts, o->counts, sizeof(counts), hipMemcpyDeviceToHost, s));
  OHIPCHK(hipStreamSynchronize(s));
  if (sched) *sched = counts[0];
  if (skipped) *skipped = counts[1];
  return MZGO_OK;
}

int mzgo_optim_set_counts(mzgo_optim* o, const int64_t* steps_host, int64_t sched, int64_t skipped, void* stream) {
  if (!o) return set_error(MZGO_EINVAL, "mzgo_optim_set_counts: null optimizer");
  if (sched < 0 || skipped < 0)
    return set_error(MZGO_EINVAL, "mzgo_optim_set_counts: counts must be >= 0, got sched %lld, skipped %lld",
                     (long long)sched, (long long)skipped);
  if (steps_host)
    for (int i = 0; i < o->n; ++i)
      if (steps_host[i] < 0)
        return set_error(MZGO_EINVAL, "mzgo_optim_set_counts: steps[%d] must be >= 0, got %lld", i,
                         (long long)steps_host[i]);
  hipStream_t s = (hipStream_t)stream;
  const int64_t counts[2] = {sched, skipped};
  if (steps_host)
    OHIPCHK(hipMemcpyAsync(o->steps, steps_host, (size_t)o->n * sizeof(int64_t), hipMemcpyHostToDevice, s));
  else
    OHIPCHK(hipMemsetAsync(o->steps, 0, (size_t)o->n * sizeof(int64_t), s));
  OHIPCHK(hipMemcpyAsync(o->counts, counts, sizeof(counts), hipMemcpyHostToDevice, s));
  OHIPCHK(hipStreamSynchronize(s));
  return MZGO_OK;
}

int mzgo_optim_lr(const mzgo_optim_hyper* hyper, int64_t sched_count, double* lr) {
  if (!hyper || !lr) return set_error(MZGO_EINVAL, "mzgo_optim_lr: null %s", !hyper ? "hyper" : "lr");
  if (hyper->step_size < 1)
    return set_error(MZGO_EINVAL, "mzgo_optim_lr: step_size must be >= 1, got %lld", (long long)hyper->step_size);
  if (sched_count < 0)
    return set_error(MZGO_EINVAL, "mzgo_optim_lr: sched_count must be >= 0, got %lld", (long long)sched_count);
  *lr = optim_lr(*hyper, sched_count);
  return MZGO_OK;
}

int mzgo_optim_step_host(int n, const int64_t* numels, float* const* params, const float* const* grads,
                         float* const* exp_avg, float* const* exp_avg_sq, const mzgo_optim_hyper* hyper,
                         int64_t* steps, int64_t* sched, int64_t* skipped, double* record) {
  const char* fn = "mzgo_optim_step_host";
  if (int rc = check_numels(fn, n, numels)) return rc;
  if (int rc = check_tables(fn, n, params, grads, exp_avg, exp_avg_sq)) return rc;
  if (int rc = check_hyper(fn, hyper)) return rc;
  const char* null = !steps ? "steps" : !sched ? "sched" : !skipped ? "skipped" : !record ? "record" : nullptr;
  if (null) return set_error(MZGO_EINVAL, "%s: null %s", fn, null);
  const mzgo_optim_hyper& H = *hyper;
  // (a) the partials, segment by segment in the table's order, added as (b) adds them
  double sum = 0.0;
  for (int t = 0; t < n; ++t) {
    const float* g = grads[t];
    for (int64_t c = 0; c < chunks_of(numels[t]); ++c) {
      if (!g) {
        sum += 0.0;
        continue;
      }
      const int64_t off = c * kOptimChunk;
      const int64_t left = numels[t] - off;
      const int cnt = left < kOptimChunk ? (int)left : kOptimChunk;
      double acc[kOptimThreads];
      for (int tid = 0; tid < kOptimThreads; ++tid) {
        float x[kOptimPerThread];
        for (int k = 0; k < kOptimPerThread; ++k) {
          const int e = tid * kOptimPerThread + k;
          x[k] = e < cnt ? g[off + e] : 0.f;
        }
        acc[tid] = optim_sumsq(x);
      }
      for (int o = kOptimThreads / 2; o > 0; o >>= 1)
        for (int tid = 0; tid < o; ++tid) acc[tid] += acc[tid + o];
      sum += acc[0];
    }
  }
  // (b) the record and the counts
  const double norm = sqrt(sum);
  const int applied = std::isfinite(norm) ? 1 : 0;
  const float coef = optim_coef(norm, H.max_norm);
  const double lr = optim_lr(H, *sched);
  record[0] = norm;
  record[1] = (double)coef;
  record[2] = lr;
  record[3] = (double)applied;
  *sched += 1;
  if (!applied) {
    *skipped += 1;
    return MZGO_OK;
  }
  // (c) the update
  for (int t = 0; t < n; ++t) {
    const float* g = grads[t];
    if (!g) continue;
    steps[t] += 1;
    const OptimConsts C = optim_consts(H, coef, lr, optim_bias_correction(H.beta1, steps[t]),
                                       optim_bias_correction(H.beta2, steps[t]));
    for (int64_t i = 0; i < numels[t]; ++i) optim_update(C, g[i], &params[t][i], &exp_avg[t][i], &exp_avg_sq[t][i]);
  }
  return MZGO_OK;
}

}  // extern "C"
