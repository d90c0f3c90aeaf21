// mzgo_weights.hip -- the engine's weight blob packed on the device: the 22
// state_dict tensors (float32 in device memory, e.g. the optimizer's output)
// go straight into the layout of mzgo_weights.hpp in ONE launch, without a
// host copy.  Each job below restates one host packer of mzgo_capi.hip
// (pack_conv, pack_wino, action_taps, the plain copies) as a gather: one
// thread per output element (per (action, cout) for the tap table), so every
// element has one writer and every f64 sum runs in the host's order inside
// one thread -- the blob is bit-identical to the host path's (the library is
// built with -ffp-contract=off; tests/test_gpu_weights_device.py compares
// the bytes).  Writes are coalesced (thread o writes element o); the gathered
// reads hit L2 (the largest source is 9 C^2 floats).
#include <hip/hip_runtime.h>

#include "mzgo_weights.hpp"
#include "mzgo_wino.hpp"

namespace mzgo {
namespace {

constexpr int kPackThreads = 256;
constexpr int kMaxPackJobs = 24;   // the tap table, 4 convs, 18 copies = 23

enum PackKind { PK_TAPS, PK_CONV, PK_WINO, PK_COPY };

struct PackJob {
  const float* src;
  const float* src2;   // PK_TAPS: the embedding
  float* dst;
  unsigned count;      // threads of the job
  unsigned block0;     // its first block
  int kind;
  int COUT, CIN;       // PK_CONV / PK_WINO; PK_TAPS: C, A
  int cog_major, ksplit;
};

struct PackJobs {
  PackJob job[kMaxPackJobs];
  int n;
};

// G2 of F(2,3) and G3 of F(3,3): pack_wino's constants (mzgo_capi.hip)
__device__ __constant__ const double kG2[4][3] = {{1, 0, 0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0, 0, 1}};
__device__ __constant__ const double kG3[5][3] = {{0.5, 0, 0},
                                                  {1.0 / 6, 1.0 / 6, 1.0 / 6},
                                                  {0.5, -0.5, 0.5},
                                                  {1.0 / 6, -1.0 / 3, 2.0 / 3},
                                                  {0, 0, 1}};

// pack_conv's element o: packed[(frag * 64 + lane) * MGP + mi]
__device__ __forceinline__ float conv_element(const PackJob& j, unsigned o) {
  const int COUT = j.COUT, CIN = j.CIN;
  const int CINP = (CIN + 3) / 4 * 4, CQ = CINP / 4, CQH = CQ / j.ksplit, MT = COUT / 16;
  const int MG = (MT % 3 == 0) ? 3 : ((MT % 4 == 0 && MT >= 8) ? 4 : 2);
  const int MGP = MG == 3 ? 4 : MG, NCOG = MT / MG;
  const int mi = o % MGP, lane = (o / MGP) % 64;
  const int frag = o / (MGP * 64);
  if (mi >= MG) return 0.f;                        // the MG == 3 pad slot
  int t, c4, cog;
  if (j.cog_major) {                               // frag = ((cog * ksplit + half) * 9 + t) * CQH + c4h
    const int c4h = frag % CQH, half = (frag / (CQH * 9)) % j.ksplit;
    t = (frag / CQH) % 9;
    cog = frag / (CQH * 9 * j.ksplit);
    c4 = half * CQH + c4h;
  } else {                                         // frag = s * NCOG + cog, s = t * CQ + c4
    const int s = frag / NCOG;
    cog = frag % NCOG;
    t = s / CQ;
    c4 = s % CQ;
  }
  const int cout = (cog * MG + mi) * 16 + (lane & 15);
  const int cin = c4 * 4 + (lane >> 4);
  return cin < CIN ? j.src[((size_t)cout * CIN + cin) * 9 + t] : 0.f;   // padded input channels
}

// pack_wino's element o (khalf order): packed[(((m*2 + h)*L + pos)*64 + lane)*4 + e]
__device__ __forceinline__ float wino_element(const PackJob& j, unsigned o) {
  const int CIN = j.CIN;
  const int CH = CIN / 2, S4 = CH / 16, KP = CIN / 16, L = 10 * KP, KH = KP / 2, NG = 10 / kWinoXG;
  const int e = o % 4, lane = (o / 4) % 64;
  const int pos = (o / 256) % L, h = (o / (256 * L)) % 2, m = o / (512 * L);
  // pos = ((kh * NG + xl / XG) * KH + k % KH) * XG + xl % XG
  const int xr = pos % kWinoXG, kk = (pos / kWinoXG) % KH, xg = (pos / (kWinoXG * KH)) % NG;
  const int kh = pos / (kWinoXG * KH * NG);
  const int k = kh * KH + kk, xl = xg * kWinoXG + xr;
  const int xi = h * 10 + xl, i = xi / 5, jj = xi % 5;
  const int hh = k / S4, s4 = k % S4;
  const int co = 16 * m + (lane & 15), ci = hh * CH + 4 * (4 * s4 + e) + (lane >> 4);
  const float* g = j.src + ((size_t)co * CIN + ci) * 9;
  double u = 0.0;
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) u += kG2[i][a] * (double)g[a * 3 + b] * kG3[jj][b];
  return (float)u;
}

// action_taps for thread o = a * C + co: the nine tap sums over ci (ascending)
// in nine accumulators, then the nine region sums in the host's ky, kx order
__device__ __forceinline__ void taps_thread(const PackJob& j, unsigned o) {
  const int C = j.COUT;
  const int a = o / C, co = o % C;
  const float* W = j.src + (size_t)co * C * 9;
  const float* e = j.src2 + (size_t)a * C;
  double u[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) u[t] = 0.0;
  for (int ci = 0; ci < C; ++ci) {
    const double ev = (double)e[ci];
#pragma unroll
    for (int t = 0; t < 9; ++t) u[t] += (double)W[ci * 9 + t] * ev;
  }
#pragma unroll
  for (int r = 0; r < 9; ++r) {
    const int ry = r / 3, rx = r % 3;
    double s = 0.0;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
      if ((ry == 0 && ky == 0) || (ry == 2 && ky == 2)) continue;   // row y-1 / y+1 off the board
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        if ((rx == 0 && kx == 0) || (rx == 2 && kx == 2)) continue;
        s += u[ky * 3 + kx];
      }
    }
    j.dst[((size_t)a * 9 + r) * C + co] = (float)s;
  }
}

__global__ __launch_bounds__(kPackThreads) void k_pack_weights(const PackJobs J) {
  int ji = 0;
  while (ji + 1 < J.n && blockIdx.x >= J.job[ji + 1].block0) ++ji;   // block-uniform
  const PackJob& j = J.job[ji];
  const unsigned o = (blockIdx.x - j.block0) * kPackThreads + threadIdx.x;
  if (o >= j.count) return;
  switch (j.kind) {
    case PK_TAPS: taps_thread(j, o); break;
    case PK_CONV: j.dst[o] = conv_element(j, o); break;
    case PK_WINO: j.dst[o] = wino_element(j, o); break;
    default: j.dst[o] = j.src[o]; break;
  }
}

}  // namespace

hipError_t pack_weights_device(const WeightLayout& L, const float* const* src, float* blob, hipStream_t s) {
  PackJobs J{};
  unsigned blocks = 0;
  auto add = [&](int kind, const float* a, const float* b, float* dst, size_t count, int cout, int cin,
                 int cog_major, int ksplit) {
    PackJob& j = J.job[J.n++];
    j = PackJob{a, b, dst, (unsigned)count, blocks, kind, cout, cin, cog_major, ksplit};
    blocks += (unsigned)((count + kPackThreads - 1) / kPackThreads);
  };
  const int C = L.C, A = L.A;
  // the tap table first: its threads run longest
  add(PK_TAPS, src[WK_DYN_W], src[WK_EMB], blob + L.off[WP_ETAB], (size_t)A * C, C, A, 0, 1);
  add(PK_CONV, src[WK_CONV1_W], nullptr, blob + L.off[WP_CONV1_W], L.size[WP_CONV1_W], 64, 6, 0, 1);
  const int lk = L.wino ? PK_WINO : PK_CONV;
  add(lk, src[WK_CONV2_W], nullptr, blob + L.off[WP_CONV2_W], L.size[WP_CONV2_W], 64, 64, 1, L.ksplit);
  add(lk, src[WK_CONV3_W], nullptr, blob + L.off[WP_CONV3_W], L.size[WP_CONV3_W], C, 64, 1, L.ksplit);
  add(lk, src[WK_DYN_W], nullptr, blob + L.off[WP_DYN_W], L.size[WP_DYN_W], C, C, 1, L.ksplit);
  auto copy = [&](WeightKey k, float* dst, size_t n) { add(PK_COPY, src[k], nullptr, dst, n, 0, 0, 0, 1); };
  copy(WK_CONV1_B, blob + L.off[WP_CONV1_B], L.size[WP_CONV1_B]);
  copy(WK_CONV2_B, blob + L.off[WP_CONV2_B], L.size[WP_CONV2_B]);
  copy(WK_CONV3_B, blob + L.off[WP_CONV3_B], L.size[WP_CONV3_B]);
  copy(WK_DYN_B, blob + L.off[WP_DYN_B], L.size[WP_DYN_B]);
  copy(WK_EMB, blob + L.off[WP_EMB], L.size[WP_EMB]);               // the first A rows
  for (int h = 0; h < 3; ++h) copy(kHeadKeys[h], blob + L.off[WP_HEAD_W] + (size_t)h * C, (size_t)C);
  for (int i = 0; i < 10; ++i) copy(kScalarKeys[i], blob + L.off[WP_REWARD_B + i], L.size[WP_REWARD_B + i]);
  static_assert(5 + 4 + 1 + 3 + 10 <= kMaxPackJobs, "job table too small");
  hipLaunchKernelGGL(k_pack_weights, dim3(blocks), dim3(kPackThreads), 0, s, J);
  return hipGetLastError();
}

}  // namespace mzgo
