// mzgo_conv_bf16.hpp -- the trainer's dynamics conv in bf16 mixed precision
// (mzgo_conv_bf16.hip): the rounding R every kernel and mzgo_bf16_round_host
// share, the kernels' tile constants, and the host launchers mzgo_unroll.hip
// and the layer entry points call.
//
// Tiles (256 threads = 4 waves per workgroup everywhere):
//
//   forward / input gradient (k_conv_bf16): a workgroup owns G boards x 32
//   output channels, G = conv_bf16_group(N) = max(1, 12 / ceil(N*N / 16)):
//   12, 12, 12, 6, 4, 3, 3, 2 boards for N = 2 .. 9 and 1 board for N >= 10, so
//   a group is at most 23 16-cell tiles and a wave holds at most 6 x 2
//   accumulators.  Per 32-channel K slice the group's rounded operand planes
//   are staged zero-haloed as [cell][32 channels] (80-byte rows: 16-byte
//   fragment reads without bank conflicts) with a 48-cell zero region for
//   masked rows: 496 x 80 = 39 680 bytes; the slice's 9 x 32 weight rows take
//   9 x 32 x 80 = 23 040 bytes.  62 720 bytes of LDS.
//
//   weight pass (k_conv_bf16_wgrad): a workgroup owns a (32 co, 32 ci) tile
//   and a chunk of boards, a wave a (16 co, 16 ci) tile with its nine taps'
//   accumulators.  The chunk is staged conv_bf16_stage_boards(N) = min(384 /
//   cells, 448 / (N + 2)^2) boards at a time: the rounded gp rows [32][392]
//   (25 088 bytes; K = boards x cells, zero-padded to a multiple of 32) and
//   the rounded zero-haloed input planes [32][494] (31 616 bytes, with a zero
//   tail the K pad reads).  56 704 bytes of LDS.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace mzgo {

// R: float32 -> bfloat16, round to nearest even, as bits.  NaN gives the quiet NaN 0x7fc0
// (torch's conversion), overflow rounds to inf.  Integer arithmetic only, so the host and the
// device run the same text.
__host__ __device__ __forceinline__ uint16_t bf16_round_bits(float v) {
  uint32_t u;
  __builtin_memcpy(&u, &v, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0;
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
__host__ __device__ __forceinline__ float bf16_round(float v) {
  const uint32_t u = (uint32_t)bf16_round_bits(v) << 16;
  float r;
  __builtin_memcpy(&r, &u, 4);
  return r;
}

constexpr int kBf16Threads = 256;
constexpr int kBf16CoTile = 32;          // output channels of a forward / input-gradient workgroup
constexpr int kBf16WaveTiles = 6;        // 16-cell tiles of a wave, at most
constexpr int kBf16Row = 40;             // bf16 per staged row: 32 channels + 8 of padding
constexpr int kBf16Cells = 448;          // staged haloed cells, at most (19 x 19: 441)
constexpr int kBf16ZeroCells = 48;       // the zero region behind them (a 3 x 3 window's extent: 2 (N + 2) + 3 <= 45)
constexpr int kBf16GpRow = 392;          // weight pass: a gp row's K (<= 384) + 8 of padding
constexpr int kBf16XRow = 494;           // weight pass: a channel's haloed planes (<= 448) + the zero tail

// boards of a forward / input-gradient workgroup
inline int conv_bf16_group(int N) {
  const int ct = (N * N + 15) / 16;
  return ct <= 12 ? 12 / ct : 1;
}
// boards the weight pass stages at a time
inline int conv_bf16_stage_boards(int N) {
  const int a = 384 / (N * N), b = kBf16Cells / ((N + 2) * (N + 2));
  const int n = a < b ? a : b;
  return n < 1 ? 1 : n;
}

// bytes of the two packed weight layouts ([tap][co][ci] then [tap][ci][co], bf16)
inline size_t conv_bf16_packed_bytes(int Cin, int Cout) { return (size_t)2 * 9 * Cin * Cout * sizeof(uint16_t); }

// mzgo_conv_bf16.hip.  `packed` is conv_bf16_packed_bytes(Cin, Cout), 16-byte aligned.
hipError_t conv_bf16_pack(const float* w, int Cin, int Cout, void* packed, hipStream_t s);
// y = relu(conv3x3(R(x (+ emb[action])), R(w)) + bias); the weights from `packed`, or rounded on the fly from
// the float32 `w` when `packed` is null
hipError_t conv_bf16_forward(const float* x, const int64_t* action, const float* emb, const void* packed,
                             const float* w, const float* bias, int B, int Cin, int Cout, int N, float* y,
                             hipStream_t s);
// gx = conv3x3^T(R(g [out > 0]), R(w)): stored to dst, or added into it (accumulate); bsum, when given,
// [B][Cin][ceil(N*N / 16)] gets every 16-cell tile's sum
hipError_t conv_bf16_input_grad(const float* g, const float* out, const void* packed, int B, int Cin, int Cout, int N,
                                float* dst, int accumulate, float* bsum, hipStream_t s);
// part[chunk][co][ci][tap] over chunks of `cb` boards: corr(R(g [out > 0]), R(x (+ emb[action])))
hipError_t conv_bf16_weight_partials(const float* g, const float* out, const float* x, const int64_t* action,
                                     const float* emb, int B, int Cin, int Cout, int N, int cb, float* part,
                                     hipStream_t s);

}  // namespace mzgo
