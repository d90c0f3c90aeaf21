// mzgo_train.hpp -- what mzgo_train.hip offers the trainer's other units
// (mzgo_unroll.hip, mzgo_conv_bf16.hip): the float32 3x3 conv layer's forward
// and the four parts of its backward as host launchers, the sizes of the
// weight pass's workspace, and the error plumbing the trainer's entry points
// share.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/mzgo.h"

namespace mzgo {

typedef float f32x4_t __attribute__((ext_vector_type(4)));   // an MFMA's result registers of a lane

constexpr int kBwdChunk = 8;   // boards per gw partial (a chunk's K = 8 x cells); a caller may ask for more
// k_conv_fwd and k_conv_bwd_input put the batch in gridDim.z: HIP's portable limit of that dimension.  The entry
// points refuse a larger batch before any launch.
constexpr int kConvMaxBatch = 65535;

// mzgo_capi.hip: set mzgo_last_error()'s text and return ``code``
int set_error(int code, const char* fmt, ...);

// in an entry point: a failed HIP call becomes MZGO_EHIP with the call's text
#define MZGO_HIPCHK(expr)                                                                          \
  do {                                                                                             \
    hipError_t e_ = (expr);                                                                        \
    if (e_ != hipSuccess) return set_error(MZGO_EHIP, "%s: %s", #expr, hipGetErrorString(e_));     \
  } while (0)

// bytes of the weight pass's partials [chunk][Cout][Cin][9] at `cb` boards per chunk
inline size_t conv_bwd_workspace_bytes_chunk(int B, int Cin, int Cout, int cb) {
  const size_t chunks = (size_t)(B + cb - 1) / cb;
  return chunks * (size_t)Cout * Cin * 9 * sizeof(float);
}
inline size_t conv_bwd_workspace_bytes(int B, int Cin, int Cout) {
  return conv_bwd_workspace_bytes_chunk(B, Cin, Cout, kBwdChunk);
}

// y = relu(conv3x3(x (+ emb[action])) + bias)
hipError_t conv_forward(const float* x, const int64_t* action, const float* emb, const float* w, const float* bias,
                        int B, int Cin, int Cout, int N, float* y, hipStream_t s);

// The backward's parts, with gp = g [out > 0]:
// gx = conv3x3^T(gp, w): stored to dst, or added into it (accumulate); bsum, when given (with accumulate only),
// [B][Cin][ceil(N*N / 16)] gets every 16-cell tile's sum
hipError_t conv_input_grad(const float* g, const float* out, const float* w, int B, int Cin, int Cout, int N,
                           float* dst, int accumulate, float* bsum, hipStream_t s);
// part[chunk][co][ci][tap] over chunks of `cb` boards: corr(gp, x (+ emb[action])); the partials' order is fixed
// by (B, cb) alone
hipError_t conv_weight_partials(const float* g, const float* out, const float* x, const int64_t* action,
                                const float* emb, int B, int Cin, int Cout, int N, int cb, float* part,
                                hipStream_t s);
// gw[n] = the chunks' partials summed in chunk order (the bf16 weight pass's partials have the same layout)
hipError_t conv_bwd_reduce(const float* part, float* gw, int chunks, size_t n, hipStream_t s);
// gb[co] = sum_{b,p} gp
hipError_t conv_bwd_bias(const float* g, const float* out, float* gb, int B, int Cout, int N, hipStream_t s);

// the four in that order (the input gradient only if gx) at kBwdChunk boards per chunk; the workspace holds
// conv_bwd_workspace_bytes(B, Cin, Cout)
hipError_t conv_backward(const float* g, const float* out, const float* x, const int64_t* action, const float* emb,
                         const float* w, int B, int Cin, int Cout, int N, float* gx, float* gw, float* gb,
                         void* workspace, hipStream_t s);

}  // namespace mzgo
