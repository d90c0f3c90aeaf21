// mzgo_consistency.hip -- the consistency head and its loss on the latents of
// the fused unroll (mzgo.h: mzgo_consistency_loss_workspace,
// mzgo_consistency_loss, mzgo_consistency_loss_backward,
// mzgo_consistency_loss_host).
//
// The head is two 1x1 convs, proj (C -> P) and pred (P -> P).  Row (k, b),
// k = 1..K, pulls p = pred(relu(proj(s_k))) towards z = proj(target_k), the
// projection of the representation's latent of the real board at start + k
// (no gradient through z), by 1 - cos(p, z) over the P CELLS entries; the
// scalar formulas are mzgo_consistency.hpp's.  latents are the unroll's
// [K+1][B][C][CELLS] taken whole (step 0 takes no part), targets [K][B][C][CELLS],
// mask [B][K].
//
// The 1x1 convs are small GEMMs on v_mfma_f32_16x16x4_f32 (exact f32, an fmaf
// chain per output): lane l = 16 g + n gives A[n][g] and B[g][n] and holds
// D[4 g + r][n] in register r.  A product D[M][N] is consumed by the next one
// without leaving its registers when that one contracts over M: at K step s
// lane group g supplies row 4 g + s, its register s, and the other operand is
// read for the same row -- the sum's order is (s, g) instead of 4 s + g, fixed
// all the same.
//
//   forward   k_consistency_fwd, a workgroup per row, a wave per 16-cell tile
//             (cells past the board read as zeros and are left out of every
//             store and sum): proj's weights go to LDS once and serve both
//             branches, the latent and the target stream from memory once as
//             the B operands of u and z, p follows from relu(u) in registers;
//             u, p, z go to the workspace for the backward, and the three row
//             sums <p,z>, |p|^2, |z|^2 are f64: a lane's entries over its
//             tiles, a butterfly, then the four waves in order.
//             k_consistency_totals: per[b] = the sample's rows in step order,
//             and the f64 total over b.
//   backward  k_consistency_bwd, a workgroup per chunk of rows walked in order
//             (cons_chunk_rows): every wave walks every tile of a row and owns
//             the channel blocks cb = wave, wave + 4, ... of g_latents and of
//             proj's weight gradient, and the tiles t = wave, wave + 4, ... of
//             pred's; g_r = pred.W^T g_p is formed twice per tile from the
//             same two operands swapped, feature-major for g_latents =
//             proj.W^T g_u and cell-major for the weight gradient's
//             contraction over the cells.  The gradients of the parameters
//             stay in registers over the chunk and leave as ONE partial per
//             chunk; k_consistency_reduce sums the chunks in order in f64.
//             The workgroups also write step 0's zeros between them.
//
// A row whose mask is 0 is not read: its loss, its g_latents and its partials
// are exact zeros; so is a degenerate row's gradient.  Plain vector loads and
// stores only; no atomics; workgroups never communicate; every sum has a fixed
// order, so the same inputs give the same bits.  Nothing here allocates or
// synchronises.  Compiled with -ffp-contract=off like every unit.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>
#include <vector>

#include "../../include/mzgo.h"
#include "mzgo_consistency.hpp"

namespace mzgo {
int set_error(int code, const char* fmt, ...);           // mzgo_capi.hip
}
using namespace mzgo;

#define CHIPCHK(expr)                                                                              \
  do {                                                                                             \
    hipError_t e_ = (expr);                                                                        \
    if (e_ != hipSuccess) return set_error(MZGO_EHIP, "%s: %s", #expr, hipGetErrorString(e_));     \
  } while (0)

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
// The kernels are compiled per PB = P / 16 feature blocks (1..4) and, the
// backward, per Q = the channel blocks a wave owns, ceil(C / 16 / 4) (1..4), so
// that the register arrays below have their real sizes.
constexpr int kMaxBlocks = 4;
static_assert(kConsMaxP == 16 * kMaxBlocks && kConsMaxC == 16 * kWaves * kMaxBlocks, "the launch tables below");

#define MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

// LDS: proj.weight [P][C + 4], pred.weight [P][P + 4] (the + 4 spreads a
// column's rows over the banks), the two biases, the forward's wave sums
__host__ __device__ inline size_t lds_floats(int C, int P) {
  return (size_t)P * (C + 4) + (size_t)P * (P + 4) + 2 * (size_t)P + 2 * 3 * kWaves;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// the sum over the 16 lanes that share l >> 4
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ void stage_weights(float* lds, const float* __restrict__ w1, const float* __restrict__ b1,
                                              const float* __restrict__ w2, const float* __restrict__ b2, int C,
                                              int P) {
  const int S1 = C + 4, S2 = P + 4;
  float *sW1 = lds, *sW2 = sW1 + P * S1, *sB1 = sW2 + P * S2, *sB2 = sB1 + P;
  for (int i = threadIdx.x; i < P * C; i += kThreads) sW1[(i / C) * S1 + i % C] = w1[i];
  for (int i = threadIdx.x; i < P * P; i += kThreads) sW2[(i / P) * S2 + i % P] = w2[i];
  for (int i = threadIdx.x; i < P; i += kThreads) {
    sB1[i] = b1[i];
    sB2[i] = b2[i];
  }
}

template <int PB>
__global__ void __launch_bounds__(kThreads) k_consistency_fwd(
    const float* __restrict__ lat, const float* __restrict__ tgt, const float* __restrict__ mask,
    const float* __restrict__ w1, const float* __restrict__ b1, const float* __restrict__ w2,
    const float* __restrict__ b2, int B, int K, int C, int P, int CELLS, float weight, double* __restrict__ scal,
    float* __restrict__ saved) {
  extern __shared__ float lds[];
  const int S1 = C + 4, S2 = P + 4;
  const float *sW1 = lds, *sW2 = sW1 + P * S1, *sB1 = sW2 + P * S2, *sB2 = sB1 + P;
  double* red = reinterpret_cast<double*>(lds + (size_t)P * S1 + (size_t)P * S2 + 2 * P);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, n = lane & 15;
  const size_t row = blockIdx.x;
  const int k = (int)(row / B) + 1, b = (int)(row % B);
  const float m = mask[(size_t)b * K + k - 1];
  if (m == 0.f) {                                        // (block-uniform) the row is not read
    if (tid < CS_COUNT) scal[row * CS_COUNT + tid] = 0.0;
    return;
  }
  stage_weights(lds, w1, b1, w2, b2, C, P);
  __syncthreads();
  const size_t PC = (size_t)P * CELLS;
  const float* x = lat + ((size_t)k * B + b) * C * CELLS;
  const float* t = tgt + ((k - 1) * B + b) * C * CELLS;
  float *su = saved + row * 3 * PC, *sp = su + PC, *sz = sp + PC;
  double dot = 0.0, pp = 0.0, zz = 0.0;
  for (int tile = wave; tile * 16 < CELLS; tile += kWaves) {
    const int cell = tile * 16 + n;
    const bool valid = cell < CELLS;
    f32x4 au[PB], az[PB], ap[PB];
#pragma unroll
    for (int ib = 0; ib < PB; ++ib)
      if (ib < PB) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          au[ib][r] = az[ib][r] = sB1[ib * 16 + 4 * g + r];
          ap[ib][r] = sB2[ib * 16 + 4 * g + r];
        }
      }
#pragma unroll 4
    for (int c0 = 0; c0 < C; c0 += 4) {                  // u = proj(x), z = proj(t): the same A operand
      const int c = c0 + g;
      const float xv = valid ? x[c * CELLS + cell] : 0.f;
      const float tv = valid ? t[c * CELLS + cell] : 0.f;
#pragma unroll
      for (int ib = 0; ib < PB; ++ib)
        if (ib < PB) {
          const float a = sW1[(ib * 16 + n) * S1 + c];
          au[ib] = MFMA(a, xv, au[ib]);
          az[ib] = MFMA(a, tv, az[ib]);
        }
    }
#pragma unroll
    for (int jb = 0; jb < PB; ++jb)                     // p = pred(relu(u)): u's registers are the B operand
      if (jb < PB) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const int j = jb * 16 + 4 * g + s;
          const float rv = fmaxf(au[jb][s], 0.f);
#pragma unroll
          for (int ib = 0; ib < PB; ++ib)
            if (ib < PB) ap[ib] = MFMA(sW2[(ib * 16 + n) * S2 + j], rv, ap[ib]);
        }
      }
    if (valid) {
#pragma unroll
      for (int ib = 0; ib < PB; ++ib)
        if (ib < PB) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int o = (ib * 16 + 4 * g + r) * CELLS + cell;
            const float uv = au[ib][r], pv = ap[ib][r], zv = az[ib][r];
            su[o] = uv;
            sp[o] = pv;
            sz[o] = zv;
            dot += (double)pv * (double)zv;
            pp += (double)pv * (double)pv;
            zz += (double)zv * (double)zv;
          }
        }
    }
  }
  dot = wave_sum(dot);
  pp = wave_sum(pp);
  zz = wave_sum(zz);
  if (lane == 0) {
    red[wave * 3] = dot;
    red[wave * 3 + 1] = pp;
    red[wave * 3 + 2] = zz;
  }
  __syncthreads();
  if (tid == 0) {
    double d = 0.0, a = 0.0, c = 0.0;
    for (int w = 0; w < kWaves; ++w) {
      d += red[w * 3];
      a += red[w * 3 + 1];
      c += red[w * 3 + 2];
    }
    double out[CS_COUNT];
    cons_row_scalars(d, a, c, weight, m, out);
    for (int i = 0; i < CS_COUNT; ++i) scal[row * CS_COUNT + i] = out[i];
  }
}

// per[b] = the sample's rows in step order; *total = the samples' f64 sums (a
// strided pass per thread, then a tree in LDS)
__global__ void __launch_bounds__(kThreads) k_consistency_totals(const double* __restrict__ scal, int B, int K,
                                                                 float* __restrict__ per,
                                                                 double* __restrict__ total) {
  __shared__ double acc[kThreads];
  const int tid = threadIdx.x;
  double t = 0.0;
  for (int b = tid; b < B; b += kThreads) {
    double p = 0.0;
    for (int k = 0; k < K; ++k) p += scal[((size_t)k * B + b) * CS_COUNT + CS_LOSS];
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

template <int PB, int Q>
__global__ void __launch_bounds__(kThreads) k_consistency_bwd(
    const float* __restrict__ lat, const float* __restrict__ mask, const float* __restrict__ g_per,
    const float* __restrict__ w1, const float* __restrict__ w2, const double* __restrict__ scal,
    const float* __restrict__ saved, int B, int K, int C, int P, int CELLS, float weight, int chunk_rows,
    float* __restrict__ g_lat, float* __restrict__ part) {
  extern __shared__ float lds[];
  constexpr int QW = (PB * PB + kWaves - 1) / kWaves;    // pred's weight-gradient tiles a wave owns
  const int S1 = C + 4, S2 = P + 4, CB = C / 16;
  const float *sW1 = lds, *sW2 = sW1 + P * S1;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, n = lane & 15;
  stage_weights(lds, w1, w1, w2, w2, C, P);              // (the biases take no part: any P floats)
  // step 0 takes no part: its gradient's zeros, shared out over the workgroups
  const size_t step = (size_t)B * C * CELLS;
  for (size_t i = (size_t)blockIdx.x * kThreads + tid; i < step; i += (size_t)gridDim.x * kThreads) g_lat[i] = 0.f;
  __syncthreads();

  f32x4 aW1[PB][Q], aW2[QW];
  float gb1[PB][4], gb2[PB][4];
#pragma unroll
  for (int q = 0; q < QW; ++q) aW2[q] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int q = 0; q < Q; ++q)
#pragma unroll
    for (int ib = 0; ib < PB; ++ib) aW1[ib][q] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ib = 0; ib < PB; ++ib)
#pragma unroll
    for (int r = 0; r < 4; ++r) gb1[ib][r] = gb2[ib][r] = 0.f;

  const size_t rows = (size_t)K * B, PC = (size_t)P * CELLS;
  const size_t row0 = (size_t)blockIdx.x * chunk_rows;
  const size_t row1 = row0 + chunk_rows < rows ? row0 + chunk_rows : rows;
  for (size_t row = row0; row < row1; ++row) {
    const int k = (int)(row / B) + 1, b = (int)(row % B);
    const float m = mask[(size_t)b * K + k - 1];
    float* gx = g_lat + ((size_t)k * B + b) * C * CELLS;
    // (block-uniform) a masked row is not read; a degenerate one has no gradient
    if (m == 0.f || scal[row * CS_COUNT + CS_LIVE] == 0.0) {
      for (size_t i = tid; i < (size_t)C * CELLS; i += kThreads) gx[i] = 0.f;
      continue;
    }
    const float coef = cons_row_coef(g_per[b], weight, m);
    const float ca = (float)scal[row * CS_COUNT + CS_A], cb_ = (float)scal[row * CS_COUNT + CS_B];
    const float* x = lat + ((size_t)k * B + b) * C * CELLS;
    const float *su = saved + row * 3 * PC, *sp = su + PC, *sz = sp + PC;
    for (int tile = 0; tile * 16 < CELLS; ++tile) {
      const int cell = tile * 16 + n;
      const bool valid = cell < CELLS;
      // g_p[j][cell] for j = 16 jb + 4 s + g: the B operand of g_r feature-major and the A operand of it cell-major
      float gp[PB][4];
#pragma unroll
      for (int jb = 0; jb < PB; ++jb)
        if (jb < PB) {
#pragma unroll
          for (int s = 0; s < 4; ++s) {
            const int o = (jb * 16 + 4 * s + g) * CELLS + cell;
            gp[jb][s] = valid ? cons_gp(coef, ca, cb_, sp[o], sz[o]) : 0.f;
            gb2[jb][s] += gp[jb][s];
          }
        }
      f32x4 rA[PB], rB[PB];
#pragma unroll
      for (int ib = 0; ib < PB; ++ib) rA[ib] = rB[ib] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int jb = 0; jb < PB; ++jb)
        if (jb < PB) {
#pragma unroll
          for (int s = 0; s < 4; ++s) {
            const int j = jb * 16 + 4 * s + g;
#pragma unroll
            for (int ib = 0; ib < PB; ++ib)
              if (ib < PB) {
                const float wv = sW2[j * S2 + ib * 16 + n];
                rA[ib] = MFMA(wv, gp[jb][s], rA[ib]);    // g_r[16 ib + 4 g + r][cell n]
                rB[ib] = MFMA(gp[jb][s], wv, rB[ib]);    // g_r[16 ib + n][cell 4 g + r]
              }
          }
        }
      // g_u = g_r [u > 0], in both layouts
#pragma unroll
      for (int ib = 0; ib < PB; ++ib)
        if (ib < PB) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float ua = valid ? su[(ib * 16 + 4 * g + r) * CELLS + cell] : 0.f;
            rA[ib][r] = ua > 0.f ? rA[ib][r] : 0.f;
            gb1[ib][r] += rA[ib][r];
            const int cellb = tile * 16 + 4 * g + r;
            const float ub = cellb < CELLS ? su[(ib * 16 + n) * CELLS + cellb] : 0.f;
            rB[ib][r] = ub > 0.f ? rB[ib][r] : 0.f;
          }
        }
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        const int cb = wave + kWaves * q;
        if (cb < CB) {                                   // (wave-uniform)
          // g_latents[c][cell] = sum_i proj.W[i][c] g_u[i][cell]
          f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int ib = 0; ib < PB; ++ib)
            if (ib < PB) {
#pragma unroll
              for (int s = 0; s < 4; ++s)
                acc = MFMA(sW1[(ib * 16 + 4 * g + s) * S1 + cb * 16 + n], rA[ib][s], acc);
            }
          if (valid) {
#pragma unroll
            for (int r = 0; r < 4; ++r) gx[(cb * 16 + 4 * g + r) * CELLS + cell] = acc[r];
          }
          // g proj.W[i][c] += sum_cell g_u[i][cell] x[c][cell]
#pragma unroll
          for (int s = 0; s < 4; ++s) {
            const int cellb = tile * 16 + 4 * g + s;
            const float xv = cellb < CELLS ? x[(cb * 16 + n) * CELLS + cellb] : 0.f;
#pragma unroll
            for (int ib = 0; ib < PB; ++ib)
              if (ib < PB) aW1[ib][q] = MFMA(rB[ib][s], xv, aW1[ib][q]);
          }
        }
      }
      // g pred.W[i][j] += sum_cell g_p[i][cell] relu(u)[j][cell]: the 16 x 16 tile t = ib PB + jb
#pragma unroll
      for (int q = 0; q < QW; ++q) {
        const int t = wave + kWaves * q;
        if (t < PB * PB) {                               // (wave-uniform)
          const int ib = t / PB, jb = t - ib * PB;
#pragma unroll
          for (int s = 0; s < 4; ++s) {
            const int cellb = tile * 16 + 4 * s + g;
            const bool ok = cellb < CELLS;
            const int oi = (ib * 16 + n) * CELLS + cellb, oj = (jb * 16 + n) * CELLS + cellb;
            const float av = ok ? cons_gp(coef, ca, cb_, sp[oi], sz[oi]) : 0.f;
            const float bv = ok ? fmaxf(su[oj], 0.f) : 0.f;
            aW2[q] = MFMA(av, bv, aW2[q]);
          }
        }
      }
    }
  }

  // the chunk's one partial
  float* pc = part + (size_t)blockIdx.x * cons_part_floats(P, C);
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const int cb = wave + kWaves * q;
    if (cb < CB) {
#pragma unroll
      for (int ib = 0; ib < PB; ++ib)
        if (ib < PB) {
#pragma unroll
          for (int r = 0; r < 4; ++r) pc[(ib * 16 + 4 * g + r) * C + cb * 16 + n] = aW1[ib][q][r];
        }
    }
  }
#pragma unroll
  for (int q = 0; q < QW; ++q) {
    const int t = wave + kWaves * q;
    if (t < PB * PB) {
      const int ib = t / PB, jb = t - ib * PB;
#pragma unroll
      for (int r = 0; r < 4; ++r) pc[cons_part_w2(P, C) + (ib * 16 + 4 * g + r) * P + jb * 16 + n] = aW2[q][r];
    }
  }
  // every wave walked every tile: wave 0's bias sums are the chunk's (a lane's cells, then its 16-lane group)
#pragma unroll
  for (int ib = 0; ib < PB; ++ib)
    if (ib < PB) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float s1 = group_sum(gb1[ib][r]), s2 = group_sum(gb2[ib][r]);
        if (wave == 0 && n == 0) {
          pc[cons_part_b1(P, C) + ib * 16 + 4 * g + r] = s1;
          pc[cons_part_b2(P, C) + ib * 16 + 4 * r + g] = s2;
        }
      }
    }
}

// entry e of the four gradients: the chunks' partials in order, in f64
__global__ void __launch_bounds__(kThreads) k_consistency_reduce(const float* __restrict__ part, int chunks, int P,
                                                                 int C, float* __restrict__ g_w1,
                                                                 float* __restrict__ g_b1, float* __restrict__ g_w2,
                                                                 float* __restrict__ g_b2) {
  const size_t n = cons_part_floats(P, C);
  const size_t e = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (e >= n) return;
  double s = 0.0;
  for (int c = 0; c < chunks; ++c) s += (double)part[(size_t)c * n + e];
  const float v = (float)s;
  if (e < cons_part_b1(P, C)) g_w1[e] = v;
  else if (e < cons_part_w2(P, C)) g_b1[e - cons_part_b1(P, C)] = v;
  else if (e < cons_part_b2(P, C)) g_w2[e - cons_part_w2(P, C)] = v;
  else g_b2[e - cons_part_b2(P, C)] = v;
}

int check_dims(const char* fn, int B, int K, int C, int P, int N) {
  if (B < 1) return set_error(MZGO_EINVAL, "%s: B must be >= 1, got %d", fn, B);
  if (K < 1) return set_error(MZGO_EINVAL, "%s: K must be >= 1, got %d (step 0 takes no part)", fn, K);
  if (C < 16 || C % 16 || C > kConsMaxC)
    return set_error(MZGO_EINVAL, "%s: C must be a multiple of 16 in 16..%d, got %d", fn, kConsMaxC, C);
  if (P < 16 || P % 16 || P > kConsMaxP)
    return set_error(MZGO_EINVAL, "%s: P must be one of 16, 32, 48, 64, got %d", fn, P);
  if (N < 2 || N > 19) return set_error(MZGO_EINVAL, "%s: N %d out of range (2..19)", fn, N);
  if ((int64_t)K * B > INT32_MAX)                        // a workgroup per (step, sample)
    return set_error(MZGO_EINVAL, "%s: K B = %lld exceeds 2^31 - 1", fn, (long long)((int64_t)K * B));
  return MZGO_OK;
}

struct Work {
  double* scal;
  float *saved, *part;
};
Work carve(void* work, int B, int K, int P, int N) {
  const long long rows = (long long)K * B;
  Work w;
  w.scal = static_cast<double*>(work);
  w.saved = reinterpret_cast<float*>(w.scal + cons_work_scalars(rows));
  w.part = w.saved + cons_work_saved(rows, P, N * N);
  return w;
}

// a kernel's dynamic LDS may pass the default limit: proj's weights alone are 65 KB at C = 256, P = 64
int lds_limit(const void* kern, size_t bytes) {
  if (bytes > (48u << 10))
    CHIPCHK(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  return MZGO_OK;
}

typedef void (*FwdKernel)(const float*, const float*, const float*, const float*, const float*, const float*,
                          const float*, int, int, int, int, int, float, double*, float*);
typedef void (*BwdKernel)(const float*, const float*, const float*, const float*, const float*, const double*,
                          const float*, int, int, int, int, int, float, int, float*, float*);
FwdKernel fwd_kernel(int P) {
  static const FwdKernel table[kMaxBlocks] = {k_consistency_fwd<1>, k_consistency_fwd<2>, k_consistency_fwd<3>,
                                              k_consistency_fwd<4>};
  return table[P / 16 - 1];
}
BwdKernel bwd_kernel(int P, int C) {
#define MZGO_CONS_ROW(pb) \
  { k_consistency_bwd<pb, 1>, k_consistency_bwd<pb, 2>, k_consistency_bwd<pb, 3>, k_consistency_bwd<pb, 4> }
  static const BwdKernel table[kMaxBlocks][kMaxBlocks] = {MZGO_CONS_ROW(1), MZGO_CONS_ROW(2), MZGO_CONS_ROW(3),
                                                          MZGO_CONS_ROW(4)};
#undef MZGO_CONS_ROW
  return table[P / 16 - 1][(C / 16 + kWaves - 1) / kWaves - 1];
}

}  // namespace

extern "C" {

int mzgo_consistency_loss_workspace(int B, int K, int C, int P, int N, int64_t* work_bytes) {
  if (int rc = check_dims("mzgo_consistency_loss_workspace", B, K, C, P, N)) return rc;
  if (!work_bytes) return set_error(MZGO_EINVAL, "mzgo_consistency_loss_workspace: null work_bytes");
  *work_bytes = (int64_t)cons_work_bytes(B, K, C, P, N);
  return MZGO_OK;
}

int mzgo_consistency_loss(const float* latents, const float* targets, const float* mask, const float* proj_w,
                          const float* proj_b, const float* pred_w, const float* pred_b, int B, int K, int C, int P,
                          int N, float weight, float* per, double* total, void* work, int64_t work_bytes,
                          void* stream) {
  const char* fn = "mzgo_consistency_loss";
  if (int rc = check_dims(fn, B, K, C, P, N)) return rc;
  const char* null = !latents ? "latents" : !targets ? "targets" : !mask ? "mask" : !proj_w ? "proj_w"
                     : !proj_b ? "proj_b" : !pred_w ? "pred_w" : !pred_b ? "pred_b" : !per ? "per"
                     : !total ? "total" : !work ? "work" : nullptr;
  if (null) return set_error(MZGO_EINVAL, "%s: null %s", fn, null);
  if (work_bytes < (int64_t)cons_work_bytes(B, K, C, P, N))
    return set_error(MZGO_EINVAL, "%s: work too small: %lld < %lld bytes", fn, (long long)work_bytes,
                     (long long)cons_work_bytes(B, K, C, P, N));
  hipStream_t s = (hipStream_t)stream;
  const Work w = carve(work, B, K, P, N);
  const size_t lds = lds_floats(C, P) * sizeof(float);
  const FwdKernel kern = fwd_kernel(P);
  if (int rc = lds_limit(reinterpret_cast<const void*>(kern), lds)) return rc;
  hipLaunchKernelGGL(kern, dim3((unsigned)(K * B)), dim3(kThreads), lds, s, latents, targets, mask, proj_w,
                     proj_b, pred_w, pred_b, B, K, C, P, N * N, weight, w.scal, w.saved);
  CHIPCHK(hipGetLastError());
  hipLaunchKernelGGL(k_consistency_totals, dim3(1), dim3(kThreads), 0, s, w.scal, B, K, per, total);
  CHIPCHK(hipGetLastError());
  return MZGO_OK;
}

int mzgo_consistency_loss_backward(const float* latents, const float* mask, const float* g_per, const float* proj_w,
                                   const float* pred_w, int B, int K, int C, int P, int N, float weight,
                                   float* g_latents, float* g_proj_w, float* g_proj_b, float* g_pred_w,
                                   float* g_pred_b, void* work, int64_t work_bytes, void* stream) {
  const char* fn = "mzgo_consistency_loss_backward";
  if (int rc = check_dims(fn, B, K, C, P, N)) return rc;
  const char* null = !latents ? "latents" : !mask ? "mask" : !g_per ? "g_per" : !proj_w ? "proj_w"
                     : !pred_w ? "pred_w" : !g_latents ? "g_latents" : !g_proj_w ? "g_proj_w"
                     : !g_proj_b ? "g_proj_b" : !g_pred_w ? "g_pred_w" : !g_pred_b ? "g_pred_b" : !work ? "work"
                     : nullptr;
  if (null) return set_error(MZGO_EINVAL, "%s: null %s", fn, null);
  if (work_bytes < (int64_t)cons_work_bytes(B, K, C, P, N))
    return set_error(MZGO_EINVAL, "%s: work too small: %lld < %lld bytes", fn, (long long)work_bytes,
                     (long long)cons_work_bytes(B, K, C, P, N));
  hipStream_t s = (hipStream_t)stream;
  const Work w = carve(work, B, K, P, N);
  const long long rows = (long long)K * B;
  const int chunk_rows = cons_chunk_rows(rows, P, C), chunks = (int)cons_chunks(rows, P, C);
  const size_t lds = lds_floats(C, P) * sizeof(float);
  const BwdKernel kern = bwd_kernel(P, C);
  if (int rc = lds_limit(reinterpret_cast<const void*>(kern), lds)) return rc;
  hipLaunchKernelGGL(kern, dim3((unsigned)chunks), dim3(kThreads), lds, s, latents, mask, g_per, proj_w,
                     pred_w, w.scal, w.saved, B, K, C, P, N * N, weight, chunk_rows, g_latents, w.part);
  CHIPCHK(hipGetLastError());
  const size_t n = cons_part_floats(P, C);
  hipLaunchKernelGGL(k_consistency_reduce, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, w.part,
                     chunks, P, C, g_proj_w, g_proj_b, g_pred_w, g_pred_b);
  CHIPCHK(hipGetLastError());
  return MZGO_OK;
}

int mzgo_consistency_loss_host(const float* latents, const float* targets, const float* mask, const float* proj_w,
                               const float* proj_b, const float* pred_w, const float* pred_b, const float* g_per,
                               int B, int K, int C, int P, int N, float weight, float* per, double* total,
                               float* g_latents, float* g_proj_w, float* g_proj_b, float* g_pred_w,
                               float* g_pred_b) {
  const char* fn = "mzgo_consistency_loss_host";
  if (int rc = check_dims(fn, B, K, C, P, N)) return rc;
  const char* null = !latents ? "latents" : !targets ? "targets" : !mask ? "mask" : !proj_w ? "proj_w"
                     : !proj_b ? "proj_b" : !pred_w ? "pred_w" : !pred_b ? "pred_b" : !g_per ? "g_per"
                     : !per ? "per" : !total ? "total" : !g_latents ? "g_latents" : !g_proj_w ? "g_proj_w"
                     : !g_proj_b ? "g_proj_b" : !g_pred_w ? "g_pred_w" : !g_pred_b ? "g_pred_b" : nullptr;
  if (null) return set_error(MZGO_EINVAL, "%s: null %s", fn, null);
  const int CELLS = N * N;
  const size_t PC = (size_t)P * CELLS, CC = (size_t)C * CELLS;
  std::vector<float> u(PC), p(PC), z(PC), gp(PC), gu(PC);
  std::vector<double> gw1((size_t)P * C, 0.0), gb1(P, 0.0), gw2((size_t)P * P, 0.0), gb2(P, 0.0);
  for (size_t i = 0; i < (size_t)B * CC; ++i) g_latents[i] = 0.f;       // step 0 takes no part
  double tot = 0.0;
  for (int b = 0; b < B; ++b) {
    double ps = 0.0;
    for (int k = 1; k <= K; ++k) {
      const float m = mask[(size_t)b * K + k - 1];
      const float* x = latents + ((size_t)k * B + b) * CC;
      const float* t = targets + ((size_t)(k - 1) * B + b) * CC;
      float* gx = g_latents + ((size_t)k * B + b) * CC;
      for (size_t i = 0; i < CC; ++i) gx[i] = 0.f;
      if (m == 0.f) continue;                            // the row is not read
      for (int i = 0; i < P; ++i)
        for (int c = 0; c < CELLS; ++c) {
          float a = proj_b[i], az = proj_b[i];
          for (int ch = 0; ch < C; ++ch) {
            a = fmaf(proj_w[(size_t)i * C + ch], x[(size_t)ch * CELLS + c], a);
            az = fmaf(proj_w[(size_t)i * C + ch], t[(size_t)ch * CELLS + c], az);
          }
          u[(size_t)i * CELLS + c] = a;
          z[(size_t)i * CELLS + c] = az;
        }
      double dot = 0.0, pp = 0.0, zz = 0.0;
      for (int i = 0; i < P; ++i)
        for (int c = 0; c < CELLS; ++c) {
          float a = pred_b[i];
          for (int j = 0; j < P; ++j) a = fmaf(pred_w[(size_t)i * P + j], fmaxf(u[(size_t)j * CELLS + c], 0.f), a);
          p[(size_t)i * CELLS + c] = a;
          const double pv = a, zv = z[(size_t)i * CELLS + c];
          dot += pv * zv;
          pp += pv * pv;
          zz += zv * zv;
        }
      double sc[CS_COUNT];
      cons_row_scalars(dot, pp, zz, weight, m, sc);
      ps += sc[CS_LOSS];
      if (sc[CS_LIVE] == 0.0) continue;                  // degenerate: no gradient
      const float coef = cons_row_coef(g_per[b], weight, m), ca = (float)sc[CS_A], cb = (float)sc[CS_B];
      for (size_t i = 0; i < PC; ++i) gp[i] = cons_gp(coef, ca, cb, p[i], z[i]);
      for (int i = 0; i < P; ++i)
        for (int c = 0; c < CELLS; ++c) {
          const double gv = gp[(size_t)i * CELLS + c];
          gb2[i] += gv;
          for (int j = 0; j < P; ++j) gw2[(size_t)i * P + j] += gv * (double)fmaxf(u[(size_t)j * CELLS + c], 0.f);
        }
      for (int j = 0; j < P; ++j)
        for (int c = 0; c < CELLS; ++c) {
          float a = 0.f;
          for (int i = 0; i < P; ++i) a = fmaf(pred_w[(size_t)i * P + j], gp[(size_t)i * CELLS + c], a);
          const float gv = u[(size_t)j * CELLS + c] > 0.f ? a : 0.f;
          gu[(size_t)j * CELLS + c] = gv;
          gb1[j] += (double)gv;
          for (int ch = 0; ch < C; ++ch) gw1[(size_t)j * C + ch] += (double)gv * (double)x[(size_t)ch * CELLS + c];
        }
      for (int ch = 0; ch < C; ++ch)
        for (int c = 0; c < CELLS; ++c) {
          float a = 0.f;
          for (int i = 0; i < P; ++i) a = fmaf(proj_w[(size_t)i * C + ch], gu[(size_t)i * CELLS + c], a);
          gx[(size_t)ch * CELLS + c] = a;
        }
    }
    per[b] = (float)ps;
    tot += ps;
  }
  *total = tot;
  for (size_t i = 0; i < (size_t)P * C; ++i) g_proj_w[i] = (float)gw1[i];
  for (size_t i = 0; i < (size_t)P * P; ++i) g_pred_w[i] = (float)gw2[i];
  for (int i = 0; i < P; ++i) {
    g_proj_b[i] = (float)gb1[i];
    g_pred_b[i] = (float)gb2[i];
  }
  return MZGO_OK;
}

}  // extern "C"
