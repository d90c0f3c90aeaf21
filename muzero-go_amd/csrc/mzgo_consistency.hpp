// mzgo_consistency.hpp -- the scalar pieces of the latent consistency loss
// (mzgo_consistency.hip: the kernels and mzgo_consistency_loss_host run this
// text, so the formulas a CPU test checks are the kernels').
//
// EfficientZero's temporal consistency loss (SimSiam's form) on the fused
// unroll's latents: for the row (k, b), k = 1..K, with the head's two 1x1
// convs proj (C -> P) and pred (P -> P),
//   u = proj(s_k),  p = pred(relu(u)),  z = proj(target_k)   (no gradient through z)
//   cos = <p, z> / (|p| |z|) over the D = P N N entries,  row = mask (1 - cos)
// and per[b] = weight * sum_k row.  A row with |p| < 1e-8 or |z| < 1e-8 is
// degenerate: cos := 0 and its gradient is exactly 0.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

namespace mzgo {

constexpr int kConsMaxC = 256;                           // proj's weights are staged in LDS whole
constexpr int kConsMaxP = 64;
constexpr double kConsEps = 1e-8;                        // the degenerate norm
constexpr size_t kConsPartialCap = (size_t)32 << 20;     // bytes of the backward's weight-gradient partials
constexpr int kConsChunks = 512;                         // ... and the chunks aimed at below that cap

// What a row keeps for its backward, four doubles: its share of the sample's
// loss, the two coefficients of g_p, and whether any gradient flows.
enum ConsScalar { CS_LOSS, CS_A, CS_B, CS_LIVE, CS_COUNT };

// The row's scalars from the three f64 sums <p,z>, |p|^2, |z|^2.
__host__ __device__ __forceinline__ void cons_row_scalars(double dot, double pp, double zz, float weight, float mask,
                                                          double* out) {
  const double np = sqrt(pp), nz = sqrt(zz);
  const bool live = np >= kConsEps && nz >= kConsEps;
  const double cos = live ? dot / (np * nz) : 0.0;
  out[CS_LOSS] = ((double)weight * (double)mask) * (1.0 - cos);
  out[CS_A] = live ? 1.0 / (np * nz) : 0.0;              // d cos / d p = z a - p b
  out[CS_B] = live ? cos / pp : 0.0;
  out[CS_LIVE] = live ? 1.0 : 0.0;
}
// what the incoming gradient of per[b] becomes on the row's cosine: -g_per * weight * mask, in float32
__host__ __device__ __forceinline__ float cons_row_coef(float g_per, float weight, float mask) {
  return -(g_per * (weight * mask));
}
// one entry of g_p = coef (z a - p b)
__host__ __device__ __forceinline__ float cons_gp(float coef, float a, float b, float p, float z) {
  return coef * (z * a - p * b);
}

// One set of the four parameter gradients' partial sums, in floats: proj.weight
// [P][C], proj.bias [P], pred.weight [P][P], pred.bias [P].
__host__ __device__ __forceinline__ size_t cons_part_b1(int P, int C) { return (size_t)P * C; }
__host__ __device__ __forceinline__ size_t cons_part_w2(int P, int C) { return (size_t)P * C + P; }
__host__ __device__ __forceinline__ size_t cons_part_b2(int P, int C) { return (size_t)P * C + P + (size_t)P * P; }
__host__ __device__ __forceinline__ size_t cons_part_floats(int P, int C) {
  return (size_t)P * C + 2 * (size_t)P + (size_t)P * P;
}
// Rows a backward workgroup walks in order into one partial: the fewest that
// keep the chunks at kConsChunks or below and their partials under the cap,
// so the partials never grow as rows x P x C.
__host__ __device__ __forceinline__ int cons_chunk_rows(long long rows, int P, int C) {
  const long long most = (long long)(kConsPartialCap / (cons_part_floats(P, C) * sizeof(float)));
  const long long chunks = most < kConsChunks ? (most < 1 ? 1 : most) : kConsChunks;
  const long long r = (rows + chunks - 1) / chunks;
  return (int)(r < 1 ? 1 : r);
}
__host__ __device__ __forceinline__ long long cons_chunks(long long rows, int P, int C) {
  const int r = cons_chunk_rows(rows, P, C);
  return (rows + r - 1) / r;
}

// The caller-owned workspace of a forward / backward pair: CS_COUNT doubles
// per row (K B rows), then u, p and z of every row in floats [rows][3][P][CELLS],
// then the backward's partials [chunks][cons_part_floats].
__host__ __device__ __forceinline__ size_t cons_work_scalars(long long rows) { return (size_t)rows * CS_COUNT; }
__host__ __device__ __forceinline__ size_t cons_work_saved(long long rows, int P, int CELLS) {
  return ((size_t)rows * 3 * P * CELLS + 3) / 4 * 4;
}
__host__ __device__ __forceinline__ size_t cons_work_bytes(int B, int K, int C, int P, int N) {
  const long long rows = (long long)K * B;
  return cons_work_scalars(rows) * sizeof(double) +
         (cons_work_saved(rows, P, N * N) + (size_t)cons_chunks(rows, P, C) * cons_part_floats(P, C)) * sizeof(float);
}

}  // namespace mzgo
