// mzgo_conv_bf16.hip -- the dynamics conv's three matrix products on
// v_mfma_f32_16x16x32_bf16 (mzgo.h: MZGO_PREC_BF16, mzgo_conv3x3_*_bf16,
// mzgo_bf16_round_host).
//
// With R = float32 -> bfloat16 round-to-nearest-even (mzgo_conv_bf16.hpp):
//
//   forward          y  = relu(conv3x3(R(x + emb[a]), R(W)) + b)
//   input gradient   gx = conv3x3^T(R(gp), R(W)),       gp = g [y > 0]
//   weight gradient  gw = corr(R(gp), R(x + emb[a]))
//
// Products of bf16 values are exact in float32 and the MFMA accumulates in
// float32; the add x + emb[a], the bias, the ReLU, every stored tensor and
// the bias gradient (mzgo_train.hip's k_conv_bwd_bias on the unrounded gp) are
// float32.  Cin and Cout are multiples of 32 (the MFMA's K), 2 <= N <= 19.
//
// Tiles (mzgo_conv_bf16.hpp has the arithmetic): every workgroup is 4 waves.
// Forward / input gradient: G boards x 32 output channels, G = max(1, 12 /
// ceil(N*N / 16)) (4 at 6x6, 1 from 10x10), 32-channel K slices, at most 6 x 2
// accumulators per wave, 62 720 bytes of LDS.  Weight pass: a (32 co, 32 ci)
// tile x a chunk of boards, staged min(384 / cells, 448 / (N + 2)^2) boards at
// a time, nine accumulators per wave, 56 704 bytes of LDS.  The forward and
// the input gradient are one kernel: an implicit GEMM whose A operand is the
// packed weight slice (rows: the 32 output channels) and whose B operand is
// the staged plane shifted by the tap (columns: 16 cells), so a lane's result
// registers are four channels of one cell and the stores run along the cells.
// The weight pass keeps mzgo_train.hip's scheme: partial tiles per chunk of
// boards into the workspace, summed by k_conv_bwd_reduce in chunk order.
//
// Fragments (16x16x32 bf16): lane l holds A[l & 15][8 (l >> 4) + j] and
// B[8 (l >> 4) + j][l & 15], j = 0..7; the result C[(l >> 4) * 4 + r][l & 15].
//
// Plain vector loads and stores only; no atomics; workgroups never
// communicate; every sum has a fixed order.  Nothing here allocates or
// synchronises.  Compiled with -ffp-contract=off like every unit.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/mzgo.h"
#include "mzgo_conv_bf16.hpp"
#include "mzgo_train.hpp"

namespace mzgo {

namespace {

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));

__device__ __forceinline__ bf16x8_t frag_ld(const uint16_t* p) { return *reinterpret_cast<const bf16x8_t*>(p); }

// W [Cout][Cin][3][3] -> R(W) as bf16 in wf [tap][co][ci] and wb [tap][ci][co]; a thread per entry
__global__ void __launch_bounds__(256) k_conv_bf16_pack(const float* __restrict__ w, uint16_t* __restrict__ wf,
                                                        uint16_t* __restrict__ wb, int Cin, int Cout) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)Cout * Cin * 9) return;
  const int tap = (int)(idx % 9);
  const size_t cc = idx / 9;
  const int ci = (int)(cc % Cin), co = (int)(cc / Cin);
  const uint16_t v = bf16_round_bits(w[idx]);
  wf[((size_t)tap * Cout + co) * Cin + ci] = v;
  wb[((size_t)tap * Cin + ci) * Cout + co] = v;
}

// The forward (BWD = false: src = x, CK = Cin, CO = Cout, weights [tap][co][ci]) and the input gradient
// (BWD = true: src = g masked by out > 0, CK = Cout, CO = Cin, weights [tap][ci][co], taps mirrored).
// WF32: the weights are the float32 tensor [CO][CK][9], rounded while staged (the forward's layer entry point,
// which has no workspace to pack into).  grid (ceil(B / G), CO / 32).
template <bool BWD, bool WF32>
__global__ void __launch_bounds__(kBf16Threads) k_conv_bf16(const float* __restrict__ src,
                                                            const float* __restrict__ out,
                                                            const int64_t* __restrict__ action,
                                                            const float* __restrict__ emb,
                                                            const void* __restrict__ wsrc,
                                                            const float* __restrict__ bias, float* __restrict__ dst,
                                                            float* __restrict__ bsum, int B, int CK, int CO, int N,
                                                            int G, int accumulate) {
  __shared__ __attribute__((aligned(16))) uint16_t xs[(kBf16Cells + kBf16ZeroCells) * kBf16Row];
  __shared__ __attribute__((aligned(16))) uint16_t ws[9 * kBf16CoTile * kBf16Row];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int CELLS = N * N, PW = N + 2, PLANE = PW * PW, CT = (CELLS + 15) / 16;
  const int b0 = blockIdx.x * G, nb = min(G, B - b0);
  const int co0 = blockIdx.y * kBf16CoTile;
  const int nmt = nb * CT;                          // this group's 16-cell tiles
  const int li = lane & 15, lk = lane >> 4;

  // the halos, the boards past B and the zero region: written once, never overwritten
  for (int i = tid; i < (kBf16Cells + kBf16ZeroCells) * kBf16Row / 2; i += kBf16Threads)
    reinterpret_cast<uint32_t*>(xs)[i] = 0u;

  // this lane's B columns: the top-left haloed cell of each tile's 3 x 3 window (masked: the zero region)
  int hb[kBf16WaveTiles];
#pragma unroll
  for (int j = 0; j < kBf16WaveTiles; ++j) {
    const int mt = wave + 4 * j;
    hb[j] = kBf16Cells;
    if (mt < nmt) {
      const int g = mt / CT, p = (mt - g * CT) * 16 + li;
      if (p < CELLS) {
        const int py = p / N, px = p - py * N;
        hb[j] = g * PLANE + py * PW + px;
      }
    }
  }
  f32x4_t acc[kBf16WaveTiles][2];
#pragma unroll
  for (int j = 0; j < kBf16WaveTiles; ++j)
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) acc[j][nt] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  for (int ck0 = 0; ck0 < CK; ck0 += 32) {
    __syncthreads();                                // the zeroing; the previous slice's reads
    // the boards' rounded planes of this slice: loads run along the cells
    for (int i = tid; i < nb * 32 * CELLS; i += kBf16Threads) {
      const int p = i % CELLS, r = i / CELLS, c = r & 31, g = r >> 5;
      const int b = b0 + g;
      const size_t idx = ((size_t)b * CK + ck0 + c) * CELLS + p;
      float v;
      if (BWD) {
        v = out[idx] > 0.f ? src[idx] : 0.f;
      } else {
        v = src[idx];
        if (emb) v = v + emb[(size_t)action[b] * CK + ck0 + c];
      }
      const int py = p / N, px = p - py * N;
      xs[(g * PLANE + (py + 1) * PW + px + 1) * kBf16Row + c] = bf16_round_bits(v);
    }
    // the slice's weights: 9 taps x 32 rows of 32 channels
    if (WF32) {
      const float* w = static_cast<const float*>(wsrc);
      for (int i = tid; i < 9 * 32 * 32; i += kBf16Threads) {
        const int tap = i % 9, rc = i / 9, c = rc & 31, r = rc >> 5;
        ws[(tap * 32 + r) * kBf16Row + c] = bf16_round_bits(w[((size_t)(co0 + r) * CK + ck0 + c) * 9 + tap]);
      }
    } else {
      const uint16_t* wp = static_cast<const uint16_t*>(wsrc);
      for (int i = tid; i < 9 * 32 * 4; i += kBf16Threads) {
        const int row = i >> 2, q = i & 3, tap = row >> 5, r = row & 31;
        const u32x4_t v = *reinterpret_cast<const u32x4_t*>(wp + ((size_t)tap * CO + co0 + r) * CK + ck0 + q * 8);
        *reinterpret_cast<u32x4_t*>(ws + row * kBf16Row + q * 8) = v;
      }
    }
    __syncthreads();
    for (int tap = 0; tap < 9; ++tap) {
      const int ky = tap / 3, kx = tap - ky * 3;
      const int off = BWD ? (2 - ky) * PW + (2 - kx) : ky * PW + kx;
      const bf16x8_t w0 = frag_ld(ws + (tap * 32 + li) * kBf16Row + 8 * lk);
      const bf16x8_t w1 = frag_ld(ws + (tap * 32 + 16 + li) * kBf16Row + 8 * lk);
#pragma unroll
      for (int j = 0; j < kBf16WaveTiles; ++j) {
        if (wave + 4 * j < nmt) {                   // (the same for the whole wave)
          const bf16x8_t xf = frag_ld(xs + (hb[j] + off) * kBf16Row + 8 * lk);
          acc[j][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w0, xf, acc[j][0], 0, 0, 0);
          acc[j][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w1, xf, acc[j][1], 0, 0, 0);
        }
      }
    }
  }

#pragma unroll
  for (int j = 0; j < kBf16WaveTiles; ++j) {
    const int mt = wave + 4 * j;
    if (mt >= nmt) continue;
    const int g = mt / CT, tile = mt - g * CT;
    const int b = b0 + g, p = tile * 16 + li;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int co = co0 + nt * 16 + lk * 4 + r;
        const float a = acc[j][nt][r];
        if (BWD) {
          if (p < CELLS) {
            const size_t idx = ((size_t)b * CO + co) * CELLS + p;
            dst[idx] = accumulate ? dst[idx] + a : a;
          }
          if (bsum) {                               // the tile's 16 cells: columns past the board are exact zeros
            float t = a;
            t += __shfl_xor(t, 1, 64);
            t += __shfl_xor(t, 2, 64);
            t += __shfl_xor(t, 4, 64);
            t += __shfl_xor(t, 8, 64);
            if (li == 0) bsum[((size_t)b * CO + co) * CT + tile] = t;
          }
        } else if (p < CELLS) {
          const float v = a + bias[co];
          dst[((size_t)b * CO + co) * CELLS + p] = v > 0.f ? v : 0.f;
        }
      }
    }
  }
}

// part[chunk][co][ci][tap] over the chunk's `cb` boards; grid ((Cout / 32) (Cin / 32), chunks); wave = a
// (16 co, 16 ci) tile of the workgroup's (32, 32), with its nine taps.  K = boards x cells runs in the staged
// boards' order; the pad of the last 32 reads zeros on both sides.
__global__ void __launch_bounds__(kBf16Threads) k_conv_bf16_wgrad(const float* __restrict__ g,
                                                                  const float* __restrict__ out,
                                                                  const float* __restrict__ x,
                                                                  const int64_t* __restrict__ action,
                                                                  const float* __restrict__ emb,
                                                                  float* __restrict__ part, int B, int Cin, int Cout,
                                                                  int N, int cb, int sb) {
  __shared__ __attribute__((aligned(16))) uint16_t gps[32 * kBf16GpRow];
  __shared__ __attribute__((aligned(16))) uint16_t xs[32 * kBf16XRow];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int CELLS = N * N, PW = N + 2, PLANE = PW * PW;
  const int CiT = Cin / 32;
  const int co0 = (blockIdx.x / CiT) * 32, ci0 = (blockIdx.x % CiT) * 32;
  const int chunk = blockIdx.y;
  const int mt = wave & 1, nt = wave >> 1;
  const int li = lane & 15, lk = lane >> 4;
  // the halos and the zero tail: written once
  for (int i = tid; i < 32 * kBf16XRow / 2; i += kBf16Threads) reinterpret_cast<uint32_t*>(xs)[i] = 0u;
  f32x4_t acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) acc[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  const int bend = min(B, (chunk + 1) * cb);
  for (int bs = chunk * cb; bs < bend; bs += sb) {
    const int n = min(sb, bend - bs);
    const int kact = n * CELLS, kpad = (kact + 31) / 32 * 32;
    __syncthreads();                                // the zeroing; the previous boards' reads
    for (int i = tid; i < n * 32 * CELLS; i += kBf16Threads) {
      const int p = i % CELLS, rr = i / CELLS, r = rr & 31, bl = rr >> 5;
      const int b = bs + bl;
      const size_t gi = ((size_t)b * Cout + co0 + r) * CELLS + p;
      gps[r * kBf16GpRow + bl * CELLS + p] = bf16_round_bits(out[gi] > 0.f ? g[gi] : 0.f);
      float xv = x[((size_t)b * Cin + ci0 + r) * CELLS + p];
      if (emb) xv = xv + emb[(size_t)action[b] * Cin + ci0 + r];
      const int py = p / N, px = p - py * N;
      xs[r * kBf16XRow + bl * PLANE + (py + 1) * PW + px + 1] = bf16_round_bits(xv);
    }
    const int npad = kpad - kact;
    for (int i = tid; i < 32 * npad; i += kBf16Threads) gps[(i / npad) * kBf16GpRow + kact + i % npad] = 0;
    __syncthreads();
    for (int k0 = 0; k0 < kpad; k0 += 32) {
      const int kb = k0 + 8 * lk;
      const bf16x8_t a = frag_ld(gps + (mt * 16 + li) * kBf16GpRow + kb);
      int ho[8];                                    // the top-left haloed cell of each K index's window
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int k = kb + j;
        ho[j] = kBf16Cells;                         // (the pad: the zero tail)
        if (k < kact) {
          const int bl = k / CELLS, p = k - bl * CELLS;
          const int py = p / N, px = p - py * N;
          ho[j] = bl * PLANE + py * PW + px;
        }
      }
      const uint16_t* xr = xs + (nt * 16 + li) * kBf16XRow;
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) {
        const int off = (tap / 3) * PW + tap % 3;
        u32x4_t u;
#pragma unroll
        for (int h = 0; h < 4; ++h)
          u[h] = (uint32_t)xr[ho[2 * h] + off] | ((uint32_t)xr[ho[2 * h + 1] + off] << 16);
        acc[tap] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, __builtin_bit_cast(bf16x8_t, u), acc[tap], 0, 0, 0);
      }
    }
  }
  const int ci = ci0 + nt * 16 + li;
#pragma unroll
  for (int tap = 0; tap < 9; ++tap)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int co = co0 + mt * 16 + lk * 4 + r;
      part[(((size_t)chunk * Cout + co) * Cin + ci) * 9 + tap] = acc[tap][r];
    }
}

size_t align256(size_t n) { return (n + 255) / 256 * 256; }

// the layer entry points' shape checks: MZGO_OK, or the error set
int check_layer(const char* fn, int B, int Cin, int Cout, int N) {
  if (B < 1) return set_error(MZGO_EINVAL, "%s: B must be >= 1, got %d", fn, B);
  if (Cin < 32 || Cin % 32)
    return set_error(MZGO_EINVAL, "%s: Cin must be a multiple of 32 in bf16 mode, got %d", fn, Cin);
  if (Cout < 32 || Cout % 32)
    return set_error(MZGO_EINVAL, "%s: Cout must be a multiple of 32 in bf16 mode, got %d", fn, Cout);
  if (N < 2 || N > 19) return set_error(MZGO_EINVAL, "%s: N %d out of range (2..19)", fn, N);
  if (B > kConvMaxBatch)
    return set_error(MZGO_EINVAL, "%s: B = %d exceeds the batch limit of %d", fn, B, kConvMaxBatch);
  return MZGO_OK;
}

}  // namespace

hipError_t conv_bf16_pack(const float* w, int Cin, int Cout, void* packed, hipStream_t s) {
  const size_t n = (size_t)Cout * Cin * 9;
  uint16_t* wf = static_cast<uint16_t*>(packed);
  hipLaunchKernelGGL(k_conv_bf16_pack, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, w, wf, wf + n, Cin, Cout);
  return hipGetLastError();
}

hipError_t conv_bf16_forward(const float* x, const int64_t* action, const float* emb, const void* packed,
                             const float* w, const float* bias, int B, int Cin, int Cout, int N, float* y,
                             hipStream_t s) {
  const int G = conv_bf16_group(N);
  const dim3 grid((unsigned)((B + G - 1) / G), (unsigned)(Cout / kBf16CoTile));
  if (packed)
    hipLaunchKernelGGL((k_conv_bf16<false, false>), grid, dim3(kBf16Threads), 0, s, x, (const float*)nullptr, action,
                       emb, packed, bias, y, (float*)nullptr, B, Cin, Cout, N, G, 0);
  else
    hipLaunchKernelGGL((k_conv_bf16<false, true>), grid, dim3(kBf16Threads), 0, s, x, (const float*)nullptr, action,
                       emb, (const void*)w, bias, y, (float*)nullptr, B, Cin, Cout, N, G, 0);
  return hipGetLastError();
}

hipError_t conv_bf16_input_grad(const float* g, const float* out, const void* packed, int B, int Cin, int Cout, int N,
                                float* dst, int accumulate, float* bsum, hipStream_t s) {
  const int G = conv_bf16_group(N);
  const dim3 grid((unsigned)((B + G - 1) / G), (unsigned)(Cin / kBf16CoTile));
  const uint16_t* wb = static_cast<const uint16_t*>(packed) + (size_t)9 * Cin * Cout;
  hipLaunchKernelGGL((k_conv_bf16<true, false>), grid, dim3(kBf16Threads), 0, s, g, out, (const int64_t*)nullptr,
                     (const float*)nullptr, (const void*)wb, (const float*)nullptr, dst, bsum, B, Cout, Cin, N, G,
                     accumulate);
  return hipGetLastError();
}

hipError_t conv_bf16_weight_partials(const float* g, const float* out, const float* x, const int64_t* action,
                                     const float* emb, int B, int Cin, int Cout, int N, int cb, float* part,
                                     hipStream_t s) {
  const int chunks = (B + cb - 1) / cb;
  hipLaunchKernelGGL(k_conv_bf16_wgrad, dim3((unsigned)((Cout / 32) * (Cin / 32)), (unsigned)chunks),
                     dim3(kBf16Threads), 0, s, g, out, x, action, emb, part, B, Cin, Cout, N, cb,
                     conv_bf16_stage_boards(N));
  return hipGetLastError();
}

}  // namespace mzgo

using namespace mzgo;

extern "C" {

int mzgo_bf16_round_host(const float* in, int64_t n, float* out) {
  if (n < 0 || (n > 0 && (!in || !out)))
    return set_error(MZGO_EINVAL, "mzgo_bf16_round_host: bad argument (n = %lld)", (long long)n);
  for (int64_t i = 0; i < n; ++i) out[i] = bf16_round(in[i]);
  return MZGO_OK;
}

int mzgo_conv3x3_relu_forward_bf16(const float* x, const int64_t* action, const float* emb, const float* weight,
                                   const float* bias, int B, int Cin, int Cout, int N, float* out, void* stream) {
  const char* fn = "mzgo_conv3x3_relu_forward_bf16";
  if (int rc = check_layer(fn, B, Cin, Cout, N)) return rc;
  if (!x || !weight || !bias || !out || (emb && !action)) return set_error(MZGO_EINVAL, "%s: null argument", fn);
  MZGO_HIPCHK(conv_bf16_forward(x, action, emb, nullptr, weight, bias, B, Cin, Cout, N, out, (hipStream_t)stream));
  return MZGO_OK;
}

int mzgo_conv3x3_backward_bf16_workspace(int B, int Cin, int Cout, int64_t* bytes_host) {
  const char* fn = "mzgo_conv3x3_backward_bf16_workspace";
  if (int rc = check_layer(fn, B, Cin, Cout, 2)) return rc;
  if (!bytes_host) return set_error(MZGO_EINVAL, "%s: null bytes_host", fn);
  *bytes_host = (int64_t)(align256(conv_bwd_workspace_bytes(B, Cin, Cout)) + conv_bf16_packed_bytes(Cin, Cout));
  return MZGO_OK;
}

int mzgo_conv3x3_backward_bf16(const float* grad_out, const float* out, const float* x, const int64_t* action,
                               const float* emb, const float* weight, int B, int Cin, int Cout, int N, float* grad_x,
                               float* grad_weight, float* grad_bias, void* workspace, int64_t workspace_bytes,
                               void* stream) {
  const char* fn = "mzgo_conv3x3_backward_bf16";
  if (int rc = check_layer(fn, B, Cin, Cout, N)) return rc;
  if (!grad_out || !out || !x || (emb && !action) || !weight || !grad_weight || !grad_bias || !workspace)
    return set_error(MZGO_EINVAL, "%s: null argument", fn);
  const size_t parts = align256(conv_bwd_workspace_bytes(B, Cin, Cout));
  const size_t need = parts + conv_bf16_packed_bytes(Cin, Cout);
  if (workspace_bytes < (int64_t)need)
    return set_error(MZGO_EINVAL, "%s: workspace too small: %lld < %lld bytes", fn, (long long)workspace_bytes,
                     (long long)need);
  if (reinterpret_cast<uintptr_t>(workspace) % 16)
    return set_error(MZGO_EINVAL, "%s: workspace must be 16-byte aligned", fn);
  hipStream_t s = (hipStream_t)stream;
  float* part = static_cast<float*>(workspace);
  void* packed = static_cast<char*>(workspace) + parts;
  const int chunks = (B + kBwdChunk - 1) / kBwdChunk;
  if (grad_x) {
    MZGO_HIPCHK(conv_bf16_pack(weight, Cin, Cout, packed, s));
    MZGO_HIPCHK(conv_bf16_input_grad(grad_out, out, packed, B, Cin, Cout, N, grad_x, 0, nullptr, s));
  }
  MZGO_HIPCHK(conv_bf16_weight_partials(grad_out, out, x, action, emb, B, Cin, Cout, N, kBwdChunk, part, s));
  MZGO_HIPCHK(conv_bwd_reduce(part, grad_weight, chunks, (size_t)Cout * Cin * 9, s));
  MZGO_HIPCHK(conv_bwd_bias(grad_out, out, grad_bias, B, Cout, N, s));
  return MZGO_OK;
}

}  // extern "C"
