// mzgo_ownership.hip -- the ownership head and its loss on the latents of the
// fused unroll (mzgo.h: mzgo_ownership_loss_workspace, mzgo_ownership_loss,
// mzgo_ownership_loss_backward, mzgo_ownership_loss_host).
//
// The head is one 1x1 conv (C -> 1) on each of the (K+1) B latents
// mzgo_unroll_latents hands out, step-major [K+1][B][C][CELLS]; the targets
// come sample-major from mzgo_replay_ownership_items, t_own [B][K+1][CELLS] in
// {-1, 0, +1} with own_mask [B][K+1].  The scalar formulas are
// mzgo_ownership.hpp's.
//
//   forward   k_ownership_loss, a workgroup per (step, sample) row: the row's
//             C x CELLS latent read once, coalesced along the cells (the channel
//             sum split over G = max(1, 256 / CELLS) channel groups, a thread per
//             (group, cell) summing its channels in order, then a thread per cell
//             summing the groups in order); the cell's logit, loss term and
//             gradient; the row's loss by wave 0 (a strided pass per lane, then a
//             butterfly).  k_ownership_loss_totals, one workgroup: per[b] = the
//             sample's K + 1 rows in step order, and the f64 total over b.
//   backward  k_ownership_loss_bwd, a workgroup per row: g_lat = g_per[b] *
//             w[ch] * g_x, and the row's partial sums for the head's weight and
//             bias (a wave per channel, the cells strided over the lanes, then a
//             butterfly); k_ownership_reduce sums the rows in a fixed order.
//
// Sums are accumulated in f64 (the kernels are bound by memory).  A row whose
// mask is 0 is not read: its loss, its g_x, its g_lat and its partials are
// exact zeros.  Plain vector loads and stores only; no atomics; workgroups
// never communicate; every sum has a fixed order, so the same inputs give the
// same bits.  Nothing here allocates or synchronises.  Compiled with
// -ffp-contract=off like every unit.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "../../include/mzgo.h"
#include "mzgo_ownership.hpp"

namespace mzgo {
int set_error(int code, const char* fmt, ...);           // mzgo_capi.hip
}
using namespace mzgo;

#define OHIPCHK(expr)                                                                              \
  do {                                                                                             \
    hipError_t e_ = (expr);                                                                        \
    if (e_ != hipSuccess) return set_error(MZGO_EHIP, "%s: %s", #expr, hipGetErrorString(e_));     \
  } while (0)

namespace {

constexpr int kThreads = 256;
constexpr int kMaxCells = 19 * 19;

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ void __launch_bounds__(kThreads) k_ownership_loss(const float* __restrict__ lat, const float* __restrict__ w,
                                                             const float* __restrict__ bias,
                                                             const float* __restrict__ t_own,
                                                             const float* __restrict__ own_mask, int B, int K, int C,
                                                             int CELLS, float weight, double* __restrict__ row_loss,
                                                             float* __restrict__ g_x) {
  __shared__ double part[kMaxCells + 7];                 // G * CELLS <= max(256, CELLS) entries
  __shared__ double cell[kMaxCells + 7];
  const int tid = threadIdx.x;
  const size_t sb = blockIdx.x;
  const int s = (int)(sb / B), b = (int)(sb - (size_t)s * B);
  const size_t tb = (size_t)b * (K + 1) + s;
  const float mask = own_mask[tb];
  float* gx = g_x + sb * CELLS;
  if (mask == 0.f) {                                     // (block-uniform) the row is not read
    for (int p = tid; p < CELLS; p += kThreads) gx[p] = 0.f;
    if (tid == 0) row_loss[sb] = 0.0;
    return;
  }
  const float* x = lat + sb * C * CELLS;
  const int G = max(1, kThreads / CELLS), Cg = (C + G - 1) / G;
  for (int i = tid; i < G * CELLS; i += kThreads) {
    const int g = i / CELLS, p = i - g * CELLS;
    const int c1 = min(C, (g + 1) * Cg);
    double a = 0.0;
    for (int c = g * Cg; c < c1; ++c) a += (double)w[c] * (double)x[(size_t)c * CELLS + p];
    part[i] = a;
  }
  __syncthreads();
  const float scale = own_row_scale(weight, mask, CELLS);
  const double bv = (double)*bias;
  for (int p = tid; p < CELLS; p += kThreads) {
    double sx = 0.0;
    for (int g = 0; g < G; ++g) sx += part[g * CELLS + p];
    float gv;
    const float l = own_loss_term((float)(sx + bv), t_own[tb * CELLS + p], &gv);
    gx[p] = scale * gv;
    cell[p] = (double)l;
  }
  __syncthreads();
  if (tid < 64) {
    double sl = 0.0;
    for (int p = tid; p < CELLS; p += 64) sl += cell[p];
    sl = wave_sum(sl);
    if (tid == 0) row_loss[sb] = own_row_loss(weight, mask, CELLS, sl);
  }
}

// per[b] = the sample's rows in step order; *total = the samples' f64 sums (a
// strided pass per thread, then a tree in LDS)
__global__ void __launch_bounds__(kThreads) k_ownership_loss_totals(const double* __restrict__ row_loss, int B, int K,
                                                                    float* __restrict__ per,
                                                                    double* __restrict__ total) {
  __shared__ double acc[kThreads];
  const int tid = threadIdx.x;
  double t = 0.0;
  for (int b = tid; b < B; b += kThreads) {
    double p = 0.0;
    for (int k = 0; k <= K; ++k) p += row_loss[(size_t)k * B + b];
    per[b] = (float)p;
    t += p;
  }
  acc[tid] = t;
  __syncthreads();
  for (int o = kThreads / 2; o > 0; o >>= 1) {
    if (tid < o) acc[tid] += acc[tid + o];
    __syncthreads();
  }
  if (tid == 0) *total = acc[0];
}

__global__ void __launch_bounds__(kThreads) k_ownership_loss_bwd(const float* __restrict__ lat,
                                                                 const float* __restrict__ w,
                                                                 const float* __restrict__ own_mask,
                                                                 const float* __restrict__ g_x,
                                                                 const float* __restrict__ g_per, int B, int K, int C,
                                                                 int CELLS, float* __restrict__ g_lat,
                                                                 double* __restrict__ hp) {
  __shared__ float gl[kMaxCells + 7];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t sb = blockIdx.x;
  const int s = (int)(sb / B), b = (int)(sb - (size_t)s * B);
  double* row = hp + sb * ((size_t)C + 1);
  float* gx = g_lat + sb * C * CELLS;
  if (own_mask[(size_t)b * (K + 1) + s] == 0.f) {        // (block-uniform) the row is not read
    for (size_t i = tid; i < (size_t)C * CELLS; i += kThreads) gx[i] = 0.f;
    for (int c = tid; c <= C; c += kThreads) row[c] = 0.0;
    return;
  }
  const float gp = g_per[b];
  for (int p = tid; p < CELLS; p += kThreads) gl[p] = gp * g_x[sb * CELLS + p];
  __syncthreads();
  if (wave == 0) {
    double sp = 0.0;
    for (int p = lane; p < CELLS; p += 64) sp += (double)gl[p];
    sp = wave_sum(sp);
    if (lane == 0) row[C] = sp;
  }
  const float* x = lat + sb * C * CELLS;
  for (int c = wave; c < C; c += kThreads / 64) {
    const float wv = w[c];
    double dot = 0.0;
    for (int p = lane; p < CELLS; p += 64) {
      dot += (double)gl[p] * (double)x[(size_t)c * CELLS + p];
      gx[(size_t)c * CELLS + p] = wv * gl[p];
    }
    dot = wave_sum(dot);
    if (lane == 0) row[c] = dot;
  }
}

// entry j = blockIdx.x of the rows summed over the (K+1) B latents: lane l sums
// rows l, l + 64, ... in order, then a butterfly
__global__ void __launch_bounds__(64) k_ownership_reduce(const double* __restrict__ hp, int rows, int C,
                                                         float* __restrict__ g_w, float* __restrict__ g_bias) {
  const int j = blockIdx.x, lane = threadIdx.x;
  double s = 0.0;
  for (int r = lane; r < rows; r += 64) s += hp[(size_t)r * ((size_t)C + 1) + j];
  s = wave_sum(s);
  if (lane != 0) return;
  if (j < C) g_w[j] = (float)s;
  else *g_bias = (float)s;
}

int check_dims(const char* fn, int B, int K, int C, int N) {
  if (B < 1) return set_error(MZGO_EINVAL, "%s: B must be >= 1, got %d", fn, B);
  if (K < 0) return set_error(MZGO_EINVAL, "%s: K must be >= 0, got %d", fn, K);
  if (C < 1 || C > (1 << 16)) return set_error(MZGO_EINVAL, "%s: C %d out of range (1..65536)", fn, C);
  if (N < 2 || N > 19) return set_error(MZGO_EINVAL, "%s: N %d out of range (2..19)", fn, N);
  if (((int64_t)K + 1) * B > INT32_MAX)                  // a workgroup per (step, sample)
    return set_error(MZGO_EINVAL, "%s: (K + 1) B = %lld exceeds 2^31 - 1", fn, (long long)(((int64_t)K + 1) * B));
  return MZGO_OK;
}

}  // namespace

extern "C" {

int mzgo_ownership_loss_workspace(int B, int K, int C, int64_t* work_bytes) {
  if (int rc = check_dims("mzgo_ownership_loss_workspace", B, K, C, 2)) return rc;
  if (!work_bytes) return set_error(MZGO_EINVAL, "mzgo_ownership_loss_workspace: null work_bytes");
  *work_bytes = (int64_t)(own_work_doubles(B, K, C) * sizeof(double));
  return MZGO_OK;
}

int mzgo_ownership_loss(const float* latents, const float* w, const float* bias, const float* t_own,
                        const float* own_mask, int B, int K, int C, int N, float weight, float* per, double* total,
                        float* g_x, void* work, int64_t work_bytes, void* stream) {
  const char* fn = "mzgo_ownership_loss";
  if (int rc = check_dims(fn, B, K, C, N)) return rc;
  const char* null = !latents ? "latents" : !w ? "w" : !bias ? "bias" : !t_own ? "t_own" : !own_mask ? "own_mask"
                     : !per ? "per" : !total ? "total" : !g_x ? "g_x" : !work ? "work" : nullptr;
  if (null) return set_error(MZGO_EINVAL, "%s: null %s", fn, null);
  if (work_bytes < (int64_t)(own_work_doubles(B, K, C) * sizeof(double)))
    return set_error(MZGO_EINVAL, "%s: work too small: %lld < %lld bytes", fn, (long long)work_bytes,
                     (long long)(own_work_doubles(B, K, C) * sizeof(double)));
  hipStream_t s = (hipStream_t)stream;
  double* row_loss = static_cast<double*>(work);
  const int rows = (K + 1) * B;
  hipLaunchKernelGGL(k_ownership_loss, dim3((unsigned)rows), dim3(kThreads), 0, s, latents, w, bias, t_own, own_mask, B,
                     K, C, N * N, weight, row_loss, g_x);
  OHIPCHK(hipGetLastError());
  hipLaunchKernelGGL(k_ownership_loss_totals, dim3(1), dim3(kThreads), 0, s, row_loss, B, K, per, total);
  OHIPCHK(hipGetLastError());
  return MZGO_OK;
}

int mzgo_ownership_loss_backward(const float* latents, const float* w, const float* own_mask, const float* g_x,
                                 const float* g_per, int B, int K, int C, int N, float* g_latents, float* g_w,
                                 float* g_bias, void* work, int64_t work_bytes, void* stream) {
  const char* fn = "mzgo_ownership_loss_backward";
  if (int rc = check_dims(fn, B, K, C, N)) return rc;
  const char* null = !latents ? "latents" : !w ? "w" : !own_mask ? "own_mask" : !g_x ? "g_x" : !g_per ? "g_per"
                     : !g_latents ? "g_latents" : !g_w ? "g_w" : !g_bias ? "g_bias" : !work ? "work" : nullptr;
  if (null) return set_error(MZGO_EINVAL, "%s: null %s", fn, null);
  if (work_bytes < (int64_t)(own_work_doubles(B, K, C) * sizeof(double)))
    return set_error(MZGO_EINVAL, "%s: work too small: %lld < %lld bytes", fn, (long long)work_bytes,
                     (long long)(own_work_doubles(B, K, C) * sizeof(double)));
  hipStream_t s = (hipStream_t)stream;
  double* hp = static_cast<double*>(work) + own_work_rows(B, K);
  const int rows = (K + 1) * B;
  hipLaunchKernelGGL(k_ownership_loss_bwd, dim3((unsigned)rows), dim3(kThreads), 0, s, latents, w, own_mask, g_x, g_per,
                     B, K, C, N * N, g_latents, hp);
  OHIPCHK(hipGetLastError());
  hipLaunchKernelGGL(k_ownership_reduce, dim3((unsigned)(C + 1)), dim3(64), 0, s, hp, rows, C, g_w, g_bias);
  OHIPCHK(hipGetLastError());
  return MZGO_OK;
}

int mzgo_ownership_loss_host(const float* latents, const float* w, const float* bias, const float* t_own,
                             const float* own_mask, const float* g_per, int B, int K, int C, int N, float weight,
                             float* per, double* total, float* g_x, float* g_latents, float* g_w, float* g_bias) {
  const char* fn = "mzgo_ownership_loss_host";
  if (int rc = check_dims(fn, B, K, C, N)) return rc;
  const char* null = !latents ? "latents" : !w ? "w" : !bias ? "bias" : !t_own ? "t_own" : !own_mask ? "own_mask"
                     : !g_per ? "g_per" : !per ? "per" : !total ? "total" : !g_x ? "g_x" : !g_latents ? "g_latents"
                     : !g_w ? "g_w" : !g_bias ? "g_bias" : nullptr;
  if (null) return set_error(MZGO_EINVAL, "%s: null %s", fn, null);
  const int CELLS = N * N;
  double tot = 0.0, gb = 0.0;
  double* gw = new double[C]();
  for (int b = 0; b < B; ++b) {
    double p = 0.0;
    for (int k = 0; k <= K; ++k) {
      const size_t sb = (size_t)k * B + b, tb = (size_t)b * (K + 1) + k;
      const float mask = own_mask[tb];
      const float* x = latents + sb * C * CELLS;
      float* gx = g_x + sb * CELLS;
      float* gl = g_latents + sb * C * CELLS;
      if (mask == 0.f) {
        for (int c = 0; c < CELLS; ++c) gx[c] = 0.f;
        for (size_t i = 0; i < (size_t)C * CELLS; ++i) gl[i] = 0.f;
        continue;
      }
      const float scale = own_row_scale(weight, mask, CELLS);
      double sl = 0.0;
      for (int c = 0; c < CELLS; ++c) {
        double sx = 0.0;
        for (int ch = 0; ch < C; ++ch) sx += (double)w[ch] * (double)x[(size_t)ch * CELLS + c];
        float gv;
        sl += (double)own_loss_term((float)(sx + (double)*bias), t_own[tb * CELLS + c], &gv);
        gx[c] = scale * gv;
      }
      p += own_row_loss(weight, mask, CELLS, sl);
      for (int c = 0; c < CELLS; ++c) gb += (double)(g_per[b] * gx[c]);
      for (int ch = 0; ch < C; ++ch) {
        double dot = 0.0;
        for (int c = 0; c < CELLS; ++c) {
          const float g = g_per[b] * gx[c];
          dot += (double)g * (double)x[(size_t)ch * CELLS + c];
          gl[(size_t)ch * CELLS + c] = w[ch] * g;
        }
        gw[ch] += dot;
      }
    }
    per[b] = (float)p;
    tot += p;
  }
  *total = tot;
  for (int ch = 0; ch < C; ++ch) g_w[ch] = (float)gw[ch];
  *g_bias = (float)gb;
  delete[] gw;
  return MZGO_OK;
}

}  // extern "C"
