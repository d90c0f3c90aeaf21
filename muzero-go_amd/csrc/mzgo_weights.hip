// mzgo_weights.hip -- the two walks of the weight blob's pack plan
// (mzgo_weights.hpp).  On the device the 22 state_dict tensors (float32 in
// device memory, e.g. the optimizer's output) go into the blob in ONE launch,
// without a host copy: one thread per output element (per (action, cout)
// column of the tap table), so every element has one writer and every f64 sum
// runs inside one thread; writes are coalesced (thread o writes element o) and
// the gathered reads hit L2 (the largest source is 9 C^2 floats).  On the host
// the same plan is walked serially, one decode per fragment.  Both run the
// element rules of mzgo_weights.hpp, so the blobs are bit-identical (the
// library is built with -ffp-contract=off; tests/test_weights_pack.py and
// tests/test_gpu_weights_device.py hold both to recorded hashes).
#include <hip/hip_runtime.h>

#include <cstring>

#include "../../include/mzgo.h"
#include "mzgo_weights.hpp"

namespace mzgo {
namespace {

constexpr int kPackThreads = 256;

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
  PackJob job[kMaxPackSteps];
  int n;
};

__global__ __launch_bounds__(kPackThreads) void k_pack_weights(const PackJobs J) {
  int ji = 0;
  while (ji + 1 < J.n && blockIdx.x >= J.job[ji + 1].block0) ++ji;   // block-uniform
  const PackJob& j = J.job[ji];
  const unsigned o = (blockIdx.x - j.block0) * kPackThreads + threadIdx.x;
  if (o >= j.count) return;
  switch (j.kind) {
    case PK_TAPS: taps_column(j.src, j.src2, j.COUT, o / j.COUT, o % j.COUT, j.dst); break;
    case PK_CONV: {
      const ConvPackGeo g = conv_pack_geo(j.COUT, j.CIN);
      const int mi = o % g.MGP, lane = (o / g.MGP) % 64;
      j.dst[o] = conv_value(j.src, j.CIN, g, conv_frag(g, j.cog_major, j.ksplit, o / (g.MGP * 64)), lane, mi);
      break;
    }
    case PK_WINO: j.dst[o] = wino_value(j.src, j.CIN, wino_frag(j.CIN, o / 256), (o / 4) % 64, o % 4); break;
    default: j.dst[o] = j.src[o]; break;
  }
}

}  // namespace

hipError_t pack_weights_device(const WeightLayout& L, const float* const* src, float* blob, hipStream_t s) {
  const PackPlan P = pack_plan(L);
  PackJobs J{};
  unsigned blocks = 0;
  for (; J.n < P.n; ++J.n) {
    const PackStep& p = P.step[J.n];
    J.job[J.n] = PackJob{src[p.key], src[p.key2], blob + p.off, (unsigned)p.count, blocks, p.kind,
                         p.COUT, p.CIN, p.cog_major, p.ksplit};
    blocks += (unsigned)((p.count + kPackThreads - 1) / kPackThreads);
  }
  hipLaunchKernelGGL(k_pack_weights, dim3(blocks), dim3(kPackThreads), 0, s, J);
  return hipGetLastError();
}

void pack_weights_host(const WeightLayout& L, const float* const* src, float* blob) {
  const PackPlan P = pack_plan(L);
  for (int i = 0; i < P.n; ++i) {
    const PackStep& p = P.step[i];
    const float* W = src[p.key];
    float* dst = blob + p.off;
    switch (p.kind) {
      case PK_TAPS: action_taps(W, src[p.key2], p.COUT, p.CIN, dst); break;
      case PK_CONV: {
        const ConvPackGeo g = conv_pack_geo(p.COUT, p.CIN);
        const int frags = (int)(p.count / (64 * g.MGP));
        for (int f = 0; f < frags; ++f) {
          const ConvFrag cf = conv_frag(g, p.cog_major, p.ksplit, f);
          for (int lane = 0; lane < 64; ++lane)
            for (int mi = 0; mi < g.MGP; ++mi) *dst++ = conv_value(W, p.CIN, g, cf, lane, mi);
        }
        break;
      }
      case PK_WINO: {
        const int frags = (int)(p.count / 256);
        for (int f = 0; f < frags; ++f) {
          const WinoFrag wf = wino_frag(p.CIN, f);
          for (int lane = 0; lane < 64; ++lane)
            for (int e = 0; e < 4; ++e) *dst++ = wino_value(W, p.CIN, wf, lane, e);
        }
        break;
      }
      default: std::memcpy(dst, W, p.count * sizeof(float)); break;
    }
  }
}

int weight_table(const char* fn, const char* const* keys, const float* const* data, const int64_t* const* shapes,
                 const int* ndims, int n, int C, int A, const float** src) {
  if (!keys || !data || !shapes || !ndims) return set_error(MZGO_EINVAL, "%s: null argument", fn);
  for (int k = 0; k < WK_COUNT; ++k) src[k] = nullptr;
  for (int i = 0; i < n; ++i) {
    if (!keys[i] || !data[i] || (!shapes[i] && ndims[i] > 0))
      return set_error(MZGO_EINVAL, "%s: null entry %d ('%s')", fn, i, keys[i] ? keys[i] : "?");
    int k = 0;
    while (k < WK_COUNT && std::strcmp(kWeightKeyNames[k], keys[i]) != 0) ++k;
    if (k == WK_COUNT) return set_error(MZGO_EINVAL, "unexpected key '%s' in state_dict", keys[i]);
    if (src[k]) return set_error(MZGO_EINVAL, "duplicate key '%s'", keys[i]);
    const WeightShape sh = weight_key_shape(k, C, A);
    if (sh.nd != ndims[i]) return set_error(MZGO_EINVAL, "'%s': expected %d dims, got %d", keys[i], sh.nd, ndims[i]);
    for (int d = 0; d < sh.nd; ++d)
      if ((long long)shapes[i][d] != sh.d[d])
        return set_error(MZGO_EINVAL, "'%s': dim %d is %lld, expected %lld", keys[i], d, (long long)shapes[i][d], sh.d[d]);
    src[k] = data[i];
  }
  for (int k = 0; k < WK_COUNT; ++k)
    if (!src[k]) return set_error(MZGO_EINVAL, "missing weight '%s'", kWeightKeyNames[k]);
  return MZGO_OK;
}

}  // namespace mzgo

using namespace mzgo;

int mzgo_weights_pack_host(int board_size, int latent_dim, const char* const* keys, const float* const* data_host,
                           const int64_t* const* shapes, const int* ndims, int n, float* blob, int64_t cap,
                           int64_t* n_floats) {
  const char* fn = "mzgo_weights_pack_host";
  if (!n_floats) return set_error(MZGO_EINVAL, "%s: null argument", fn);
  if (!find_kernels(board_size, latent_dim))
    return set_error(MZGO_EINVAL, "%s: no kernels built for board_size %d, latent_dim %d", fn, board_size, latent_dim);
  const WeightLayout L = weight_layout(board_size, latent_dim, board_size * board_size + 1);
  const float* src[WK_COUNT];
  if (int rc = weight_table(fn, keys, data_host, shapes, ndims, n, L.C, L.A, src)) return rc;
  *n_floats = (int64_t)L.total;
  if (!blob) return MZGO_OK;
  if (cap < *n_floats) return set_error(MZGO_EINVAL, "%s: cap %lld < %lld floats", fn, (long long)cap, (long long)*n_floats);
  std::memset(blob, 0, L.total * sizeof(float));            // the parts' padding
  pack_weights_host(L, src, blob);
  return MZGO_OK;
}
