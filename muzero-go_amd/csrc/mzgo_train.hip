// mzgo_train.hip -- the trainer's 3x3 conv layers on fp32 MFMA: forward
// (activation recomputation) and backward (main.py's
// training step, main.py:478-482's loss.backward() through
// RepresentationNetwork.forward, main.py:72-84, and DynamicsNetwork.forward,
// main.py:97-103).
//
// A layer:  y = relu(conv3x3(x) + b), padding 1, x [B][Cin][N][N] -- for the
// dynamics x = latent + emb[a] broadcast over the board (emb given).  Given
// g = dL/dy, with the ReLU mask taken from the saved output (gp = g * [y > 0]):
//
//   gx[b][ci][q]          = sum_{co,ky,kx} W[co][ci][ky][kx] gp[b][co][q - (ky-1, kx-1)]   (conv2d_input)
//   gw[co][ci][ky][kx]    = sum_{b,p} gp[b][co][p] x[b][ci][p + (ky-1, kx-1)]              (conv2d_weight)
//   gb[co]                = sum_{b,p} gp[b][co][p]
//
// All as implicit GEMMs on v_mfma_f32_16x16x4_f32 (exact f32 products, f32
// accumulation; the summation order differs from MIOpen's, so the tolerance
// against torch is fp32 rounding).  Channel counts need not be multiples of
// 16 (the representation's conv1 has Cin = 6): tiles are masked.
//   forward: one wave per (board, 16 cells, 16 co) tile, K = Cin x 9 taps.
//   gx:      one wave per (board, 16 cells, 16 ci) tile, K = 9 taps x Cout.
//   gw:      one workgroup of 9 waves (one per tap) per (16 co, 16 ci) tile and
//            chunk of boards: the chunk's gp rows and zero-haloed x planes are
//            staged in LDS with coalesced loads, K = the chunk's boards x
//            cells; the chunks' partial tiles land in a workspace and
//            k_conv_bwd_reduce sums them in chunk order (deterministic, no
//            atomics).
//   gb:      one workgroup per co, a fixed-order tree reduction.
//
// Operand fragments (16x16x4 f32): lane l holds A[l & 15][k = l >> 4] and
// B[k = l >> 4][l & 15]; the result C[(l >> 4) * 4 + r][l & 15] in register r.
//
// The layer entry points (mzgo.h: mzgo_conv3x3_relu_forward,
// mzgo_conv3x3_backward, mzgo_dyn_conv_backward and their workspace sizes) are
// at the end of this file.
#include "mzgo_train.hpp"

namespace mzgo {

constexpr int kMaxN = 19;

// y = relu(conv3x3(x (+ emb[action]) ) + bias); grid (ceil(CELLS/16), ceil(Cout/16), B), one wave
__global__ void __launch_bounds__(64) k_conv_fwd(const float* __restrict__ x, const int64_t* __restrict__ action,
                                                 const float* __restrict__ emb, const float* __restrict__ w,
                                                 const float* __restrict__ bias, float* __restrict__ y, int Cin,
                                                 int Cout, int N) {
  const int lane = threadIdx.x;
  const int CELLS = N * N;
  const int b = blockIdx.z, co0 = blockIdx.y * 16, p0 = blockIdx.x * 16;
  const int i = lane & 15, k = lane >> 4;
  const int p = p0 + i;                           // this lane's A row (cell)
  const int py = p / N, px = p - py * N;
  const bool prow = p < CELLS;
  const int co = co0 + i;                         // this lane's B column
  const bool ccol = co < Cout;
  const float* xb = x + (size_t)b * Cin * CELLS;
  const float* eb = emb ? emb + (size_t)action[b] * Cin : nullptr;
  f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
  for (int tap = 0; tap < 9; ++tap) {
    const int ky = tap / 3, kx = tap - ky * 3;
    const int sy = py + ky - 1, sx = px + kx - 1;
    const bool on = prow && sy >= 0 && sy < N && sx >= 0 && sx < N;
    for (int c0 = 0; c0 < Cin; c0 += 4) {
      const int ci = c0 + k;
      const bool okc = ci < Cin;
      const float a = on && okc ? xb[(size_t)ci * CELLS + sy * N + sx] + (eb ? eb[ci] : 0.f) : 0.f;
      const float bw = ccol && okc ? w[((size_t)co * Cin + ci) * 9 + tap] : 0.f;
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bw, acc, 0, 0, 0);
    }
  }
  const int col = co0 + (lane & 15);
  if (col < Cout) {
    const float bb = bias[col];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int pr = p0 + (lane >> 4) * 4 + r;
      const float v = acc[r] + bb;
      if (pr < CELLS) y[((size_t)b * Cout + col) * CELLS + pr] = v > 0.f ? v : 0.f;
    }
  }
}

// gx; grid (ceil(CELLS/16), ceil(Cin/16), B), one wave per block.  CHAIN (a step of the unroll's chain): the
// result is ADDED into dst (the previous latent's gradient, which already holds its heads' part), and the
// tile's sum over its 16 cells goes to bsum[b][ci][tile] for the embedding; Cin and Cout are multiples of 16
// there (the launcher refuses others), so the channel masks are compiled out: with them the ten steps of the
// chain at 6x6, C = 128, B = 128 measured 0.10 ms slower (profiles/unroll_timing_refactor_masked.json), and
// with the tap's board mask tested per K step instead of once per tap still 0.04 ms.  The loop is one load
// chain per MFMA (out, g and w, then the product), so every test in it is on the critical path.
template <bool CHAIN>
__global__ void __launch_bounds__(64) k_conv_bwd_input(const float* __restrict__ g, const float* __restrict__ out,
                                                       const float* __restrict__ w, float* __restrict__ dst,
                                                       float* __restrict__ bsum, int Cin, int Cout, int N) {
  const int lane = threadIdx.x;
  const int CELLS = N * N;
  const int b = blockIdx.z, ci0 = blockIdx.y * 16, p0 = blockIdx.x * 16;
  const int i = lane & 15, k = lane >> 4;
  const int p = p0 + i;                           // this lane's A row (cell)
  const int py = p / N, px = p - py * N;
  const bool prow = p < CELLS;
  const int ci = ci0 + i;                         // this lane's B column
  const bool ccol = CHAIN || ci < Cin;
  const size_t gplane = (size_t)b * Cout * CELLS;
  f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
  for (int tap = 0; tap < 9; ++tap) {
    const int ky = tap / 3, kx = tap - ky * 3;
    const int qy = py - ky + 1, qx = px - kx + 1;
    const bool on = prow && qy >= 0 && qy < N && qx >= 0 && qx < N;
    const size_t q = on ? (size_t)qy * N + qx : 0;
    for (int co0 = 0; co0 < Cout; co0 += 4) {
      const int co = co0 + k;
      const bool okc = CHAIN || co < Cout;
      float a = 0.f;                              // gp at the tap's cell, 0 off the board
      if (on && okc) {
        const size_t idx = gplane + (size_t)co * CELLS + q;
        a = out[idx] > 0.f ? g[idx] : 0.f;
      }
      const float bw = ccol && okc ? w[((size_t)co * Cin + ci) * 9 + tap] : 0.f;
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bw, acc, 0, 0, 0);
    }
  }
  float t = 0.f;                                  // rows past the board are exact zeros
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int pr = p0 + (lane >> 4) * 4 + r;
    if (ccol && pr < CELLS) {
      const size_t idx = ((size_t)b * Cin + ci) * CELLS + pr;
      dst[idx] = CHAIN ? dst[idx] + acc[r] : acc[r];
    }
    t += acc[r];
  }
  if (CHAIN) {
    t += __shfl_xor(t, 16, 64);
    t += __shfl_xor(t, 32, 64);
    if (bsum && lane < 16 && ccol) bsum[((size_t)b * Cin + ci) * gridDim.x + blockIdx.x] = t;
  }
}

// partial[chunk][co][ci][tap] over the chunk's `cb` boards; grid (coT * ciT, chunks),
// 9 waves (wave = tap)
constexpr int kGpStride = kMaxN * kMaxN + 3;            // gp row in LDS (cells, padded to a float4 of K)
constexpr int kXPlane = (kMaxN + 2) * (kMaxN + 2);      // zero-haloed x plane in LDS
__global__ void __launch_bounds__(576) k_conv_bwd_weight(const float* __restrict__ g, const float* __restrict__ out,
                                                         const float* __restrict__ x,
                                                         const int64_t* __restrict__ action,
                                                         const float* __restrict__ emb, float* __restrict__ part,
                                                         int B, int Cin, int Cout, int N, int cb) {
  __shared__ float gpl[16 * kGpStride];
  __shared__ float xl[16 * kXPlane];
  const int tid = threadIdx.x, lane = tid & 63, tap = tid >> 6;
  const int CELLS = N * N, PW = N + 2, PLANE = PW * PW;
  const int CT = (Cin + 15) / 16;
  const int co0 = (blockIdx.x / CT) * 16, ci0 = (blockIdx.x % CT) * 16;
  const int chunk = blockIdx.y;
  const int ky = tap / 3, kx = tap - ky * 3;
  const int i = lane & 15, k = lane >> 4;
  // zero halo of the x planes (interior rewritten per board) and the K pad of gp
  for (int j = tid; j < 16 * kXPlane; j += 576) xl[j] = 0.f;
  f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
  const int b1 = min(B, (chunk + 1) * cb);
  for (int b = chunk * cb; b < b1; ++b) {
    __syncthreads();                                  // the previous board's reads are done
    // stage: gp rows of the 16 co, x planes of the 16 ci (row-contiguous loads)
    for (int j = tid; j < 16 * CELLS; j += 576) {
      const int r = j / CELLS, p = j - r * CELLS;
      const int co = co0 + r, ci = ci0 + r;
      float gv = 0.f, xv = 0.f;
      if (co < Cout) {
        const size_t idx = ((size_t)b * Cout + co) * CELLS + p;
        gv = out[idx] > 0.f ? g[idx] : 0.f;
      }
      if (ci < Cin) xv = x[((size_t)b * Cin + ci) * CELLS + p] + (emb ? emb[(size_t)action[b] * Cin + ci] : 0.f);
      gpl[r * kGpStride + p] = gv;
      const int py = p / N, px = p - py * N;
      xl[r * kXPlane + (py + 1) * PW + px + 1] = xv;
    }
    for (int j = tid; j < 16 * 3; j += 576) gpl[(j / 3) * kGpStride + CELLS + j % 3] = 0.f;
    __syncthreads();
    for (int p0 = 0; p0 < CELLS; p0 += 4) {
      const int p = p0 + k;                           // K index: this lane's cell
      const float a = gpl[i * kGpStride + p];         // (p >= CELLS: the zero pad)
      float bx = 0.f;
      if (p < CELLS) {
        const int py = p / N, px = p - py * N;
        bx = xl[i * kXPlane + (py + ky) * PW + px + kx];
      }
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bx, acc, 0, 0, 0);
    }
  }
  (void)PLANE;
  const int ci = ci0 + (lane & 15);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int co = co0 + (lane >> 4) * 4 + r;
    if (co < Cout && ci < Cin) part[(((size_t)chunk * Cout + co) * Cin + ci) * 9 + tap] = acc[r];
  }
}

// gw = the chunks' partials summed in chunk order
__global__ void __launch_bounds__(256) k_conv_bwd_reduce(const float* __restrict__ part, float* __restrict__ gw,
                                                         int chunks, size_t n) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n) return;
  float s = 0.f;
  for (int c = 0; c < chunks; ++c) s += part[(size_t)c * n + idx];
  gw[idx] = s;
}

// gb[co] = sum_{b,p} gp: one workgroup per co; each thread sums a fixed
// strided subset in order, then a fixed-order tree (deterministic)
__global__ void __launch_bounds__(256) k_conv_bwd_bias(const float* __restrict__ g, const float* __restrict__ out,
                                                       float* __restrict__ gb, int B, int Cout, int N) {
  __shared__ float red[256];
  const int co = blockIdx.x, tid = threadIdx.x, CELLS = N * N;
  float s = 0.f;
  for (int j = tid; j < B * CELLS; j += 256) {
    const int b = j / CELLS, p = j - b * CELLS;
    const size_t idx = ((size_t)b * Cout + co) * CELLS + p;
    s += out[idx] > 0.f ? g[idx] : 0.f;
  }
  red[tid] = s;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (tid < h) red[tid] += red[tid + h];
    __syncthreads();
  }
  if (tid == 0) gb[co] = red[0];
}

hipError_t conv_forward(const float* x, const int64_t* action, const float* emb, const float* w, const float* bias,
                        int B, int Cin, int Cout, int N, float* y, hipStream_t s) {
  const int CELLS = N * N;
  hipLaunchKernelGGL(k_conv_fwd, dim3((CELLS + 15) / 16, (Cout + 15) / 16, B), dim3(64), 0, s, x, action, emb, w,
                     bias, y, Cin, Cout, N);
  return hipGetLastError();
}

hipError_t conv_input_grad(const float* g, const float* out, const float* w, int B, int Cin, int Cout, int N,
                           float* dst, int accumulate, float* bsum, hipStream_t s) {
  const dim3 grid((N * N + 15) / 16, (Cin + 15) / 16, B);
  if (accumulate && (Cin % 16 || Cout % 16)) return hipErrorInvalidValue;   // (its instantiation has no channel masks)
  if (accumulate)
    hipLaunchKernelGGL(k_conv_bwd_input<true>, grid, dim3(64), 0, s, g, out, w, dst, bsum, Cin, Cout, N);
  else
    hipLaunchKernelGGL(k_conv_bwd_input<false>, grid, dim3(64), 0, s, g, out, w, dst, (float*)nullptr, Cin, Cout, N);
  return hipGetLastError();
}

hipError_t conv_weight_partials(const float* g, const float* out, const float* x, const int64_t* action,
                                const float* emb, int B, int Cin, int Cout, int N, int cb, float* part,
                                hipStream_t s) {
  const int chunks = (B + cb - 1) / cb;
  hipLaunchKernelGGL(k_conv_bwd_weight, dim3(((Cout + 15) / 16) * ((Cin + 15) / 16), chunks), dim3(576), 0, s, g,
                     out, x, action, emb, part, B, Cin, Cout, N, cb);
  return hipGetLastError();
}

hipError_t conv_bwd_reduce(const float* part, float* gw, int chunks, size_t n, hipStream_t s) {
  hipLaunchKernelGGL(k_conv_bwd_reduce, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, part, gw, chunks, n);
  return hipGetLastError();
}

hipError_t conv_bwd_bias(const float* g, const float* out, float* gb, int B, int Cout, int N, hipStream_t s) {
  hipLaunchKernelGGL(k_conv_bwd_bias, dim3(Cout), dim3(256), 0, s, g, out, gb, B, Cout, N);
  return hipGetLastError();
}

hipError_t conv_backward(const float* g, const float* out, const float* x, const int64_t* action, const float* emb,
                         const float* w, int B, int Cin, int Cout, int N, float* gx, float* gw, float* gb,
                         void* workspace, hipStream_t s) {
  float* part = static_cast<float*>(workspace);
  hipError_t e = gx ? conv_input_grad(g, out, w, B, Cin, Cout, N, gx, 0, nullptr, s) : hipSuccess;
  if (e == hipSuccess) e = conv_weight_partials(g, out, x, action, emb, B, Cin, Cout, N, kBwdChunk, part, s);
  if (e == hipSuccess) e = conv_bwd_reduce(part, gw, (B + kBwdChunk - 1) / kBwdChunk, (size_t)Cout * Cin * 9, s);
  if (e == hipSuccess) e = conv_bwd_bias(g, out, gb, B, Cout, N, s);
  return e;
}

}  // namespace mzgo

using namespace mzgo;

extern "C" {

int mzgo_dyn_conv_backward_workspace(int B, int C, int64_t* bytes_host) {
  if (B < 1 || C < 16 || C % 16 || !bytes_host) return set_error(MZGO_EINVAL, "bad argument (B=%d, C=%d)", B, C);
  *bytes_host = (int64_t)conv_bwd_workspace_bytes(B, C, C);
  return MZGO_OK;
}

int mzgo_dyn_conv_backward(const float* grad_out, const float* out, const float* latent, const int64_t* action,
                           const float* emb, const float* weight, int B, int C, int N, float* grad_latent,
                           float* grad_weight, float* grad_bias, void* workspace, int64_t workspace_bytes,
                           void* stream) {
  if (!grad_out || !out || !latent || !action || !emb || !weight || !grad_latent || !grad_weight || !grad_bias ||
      !workspace || B < 1 || C < 16 || C % 16 || N < 2 || N > 19)
    return set_error(MZGO_EINVAL, "bad argument (B=%d, C=%d, N=%d)", B, C, N);
  if (B > kConvMaxBatch)
    return set_error(MZGO_EINVAL, "mzgo_dyn_conv_backward: B = %d exceeds the launch grid's z limit of %d", B,
                     kConvMaxBatch);
  if (workspace_bytes < (int64_t)conv_bwd_workspace_bytes(B, C, C))
    return set_error(MZGO_EINVAL, "workspace too small: %lld < %lld bytes", (long long)workspace_bytes,
                     (long long)conv_bwd_workspace_bytes(B, C, C));
  MZGO_HIPCHK(conv_backward(grad_out, out, latent, action, emb, weight, B, C, C, N, grad_latent, grad_weight,
                            grad_bias, workspace, (hipStream_t)stream));
  return MZGO_OK;
}

int mzgo_conv3x3_relu_forward(const float* x, const int64_t* action, const float* emb, const float* weight,
                              const float* bias, int B, int Cin, int Cout, int N, float* out, void* stream) {
  if (!x || !weight || !bias || !out || (emb && !action) || B < 1 || Cin < 1 || Cout < 1 || N < 2 || N > 19)
    return set_error(MZGO_EINVAL, "bad argument (B=%d, Cin=%d, Cout=%d, N=%d)", B, Cin, Cout, N);
  if (B > kConvMaxBatch)
    return set_error(MZGO_EINVAL, "mzgo_conv3x3_relu_forward: B = %d exceeds the launch grid's z limit of %d", B,
                     kConvMaxBatch);
  MZGO_HIPCHK(conv_forward(x, action, emb, weight, bias, B, Cin, Cout, N, out, (hipStream_t)stream));
  return MZGO_OK;
}

int mzgo_conv3x3_backward_workspace(int B, int Cin, int Cout, int64_t* bytes_host) {
  if (B < 1 || Cin < 1 || Cout < 1 || !bytes_host)
    return set_error(MZGO_EINVAL, "bad argument (B=%d, Cin=%d, Cout=%d)", B, Cin, Cout);
  *bytes_host = (int64_t)conv_bwd_workspace_bytes(B, Cin, Cout);
  return MZGO_OK;
}

int mzgo_conv3x3_backward(const float* grad_out, const float* out, const float* x, const int64_t* action,
                          const float* emb, const float* weight, int B, int Cin, int Cout, int N, float* grad_x,
                          float* grad_weight, float* grad_bias, void* workspace, int64_t workspace_bytes,
                          void* stream) {
  if (!grad_out || !out || !x || (emb && !action) || !weight || !grad_weight || !grad_bias || !workspace || B < 1 ||
      Cin < 1 || Cout < 1 || N < 2 || N > 19)
    return set_error(MZGO_EINVAL, "bad argument (B=%d, Cin=%d, Cout=%d, N=%d)", B, Cin, Cout, N);
  if (B > kConvMaxBatch)
    return set_error(MZGO_EINVAL, "mzgo_conv3x3_backward: B = %d exceeds the launch grid's z limit of %d", B,
                     kConvMaxBatch);
  if (workspace_bytes < (int64_t)conv_bwd_workspace_bytes(B, Cin, Cout))
    return set_error(MZGO_EINVAL, "workspace too small: %lld < %lld bytes", (long long)workspace_bytes,
                     (long long)conv_bwd_workspace_bytes(B, Cin, Cout));
  MZGO_HIPCHK(conv_backward(grad_out, out, x, action, emb, weight, B, Cin, Cout, N, grad_x, grad_weight, grad_bias,
                            workspace, (hipStream_t)stream));
  return MZGO_OK;
}

}  // extern "C"
