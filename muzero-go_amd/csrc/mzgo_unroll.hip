// mzgo_unroll.hip -- the trainer's whole K-step unroll in one forward and one
// backward call (mzgo.h: mzgo_unroll_workspace, mzgo_unroll_forward,
// mzgo_unroll_backward, mzgo_unroll_latents, mzgo_unroll_backward_l,
// mzgo_unroll_heads_host).
//
// main.py:431-482 unrolls a trajectory step by step: the representation
// (main.py:72-84), then K times the dynamics conv (main.py:97-103) with the
// reward head, and the prediction heads (main.py:116-144) on every latent.
// mzgo.trainer's batched step does that for B samples with some forty torch
// ops per unroll step, each with its autograd node.  Only the conv chain is
// sequential; the heads of all K + 1 latents are independent of one another.
// So here:
//
//   forward   k_unroll_stage (the observations kept, the actions step-major),
//             the 3 + K convs on conv_forward (mzgo_train.hip) writing every
//             latent step-major into `saved`, then ONE k_unroll_heads launch
//             over all (K+1) B latents: K + 5 launches.
//   backward  ONE k_unroll_heads_bwd launch (every latent's gradient from the
//             heads, and a row of partial sums per latent for the thirteen
//             head tensors), k_unroll_heads_reduce (the rows summed in a fixed
//             order), K conv_input_grad launches in its accumulating form
//             (the dynamics conv's input gradient of step s added into step
//             s - 1's, with its board sums), the dynamics conv's weight and
//             bias gradients in ONE pass over the K B boards
//             (conv_weight_partials, conv_bwd_reduce, conv_bwd_bias),
//             k_unroll_emb_grad, and the representation's three layers on
//             conv_backward from the saved activations: K + 17 launches.
//             mzgo_unroll_backward_l with a latent gradient (an auxiliary
//             loss on the latents, mzgo_unroll_latents) adds it to the heads'
//             after the first two: one elementwise launch more.
//
// fp32 throughout, unless the _p entry points are given MZGO_PREC_BF16: then
// the dynamics conv's three matrix products -- the K forward convs, the K
// chain steps and the weight pass's partials, the three dyn_* helpers below --
// run on mzgo_conv_bf16.hip's bf16 MFMA kernels from weights packed once per
// forward call into `saved` (one more launch); everything else, stored tensors
// included, is the same float32 and the same sequence of launches.  Plain
// vector loads and stores only; no atomics; workgroups never communicate;
// every sum has a fixed order, so the same inputs give the same bits.  Nothing
// here allocates or synchronises.  Compiled with -ffp-contract=off like every
// unit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstring>

#include "../../include/mzgo.h"
#include "mzgo_conv_bf16.hpp"
#include "mzgo_train.hpp"
#include "mzgo_unroll.hpp"
#include "mzgo_weights.hpp"

using namespace mzgo;

namespace {

constexpr int kHeadThreads = 256;
constexpr int kMaxCells = 19 * 19;
constexpr int kRepC = 64;                               // the representation's hidden width (main.py:72-84)
constexpr size_t kDynWorkspaceCap = (size_t)32 << 20;   // the K B pass: more boards per chunk past this

constexpr unsigned bit(int k) { return 1u << k; }
constexpr unsigned kAllSet = (1u << WK_COUNT) - 1;
// the dynamics' tensors: no gradient at K = 0
constexpr unsigned kDynSet = bit(WK_EMB) | bit(WK_DYN_W) | bit(WK_DYN_B) | bit(WK_REWARD_W) | bit(WK_REWARD_B) |
                              bit(WK_FC1_W) | bit(WK_FC1_B) | bit(WK_FC2_W) | bit(WK_FC2_B);
constexpr unsigned kTrunkSet = bit(WK_CONV1_W) | bit(WK_CONV1_B) | bit(WK_CONV2_W) | bit(WK_CONV2_B) |
                                bit(WK_CONV3_W) | bit(WK_CONV3_B) | bit(WK_EMB) | bit(WK_DYN_W) | bit(WK_DYN_B);
constexpr unsigned kHeadSet = kAllSet & ~kTrunkSet;

// keys / data / shapes / ndims (mzgo_set_weights_device's convention) -> P[WK_*];
// `grads`, when given, is parallel to `keys` -> Gd[WK_*].  Keys outside `allow`
// are refused, every key of `need` must be there, and every key of `need_grad`
// must have a gradient pointer.
int resolve(const char* fn, const char* const* keys, const float* const* data, const int64_t* const* shapes,
            const int* ndims, float* const* grads, int n, int C, int emb_rows, unsigned allow, unsigned need,
            unsigned need_grad, const float** P, float** Gd) {
  if (!keys || !data || !shapes || !ndims) return set_error(MZGO_EINVAL, "%s: null parameter table", fn);
  for (int k = 0; k < WK_COUNT; ++k) {
    P[k] = nullptr;
    if (Gd) Gd[k] = nullptr;
  }
  for (int i = 0; i < n; ++i) {
    if (!keys[i] || !data[i] || (!shapes[i] && ndims[i] > 0))
      return set_error(MZGO_EINVAL, "%s: null entry %d ('%s')", fn, i, keys[i] ? keys[i] : "?");
    int k = 0;
    while (k < WK_COUNT && strcmp(kWeightKeyNames[k], keys[i]) != 0) ++k;
    if (k == WK_COUNT || !(allow & bit(k))) return set_error(MZGO_EINVAL, "%s: unexpected key '%s'", fn, keys[i]);
    if (P[k]) return set_error(MZGO_EINVAL, "%s: duplicate key '%s'", fn, keys[i]);
    const WeightShape sh = weight_key_shape(k, C, emb_rows);
    if (sh.nd != ndims[i]) return set_error(MZGO_EINVAL, "%s: '%s': expected %d dims, got %d", fn, keys[i], sh.nd, ndims[i]);
    for (int d = 0; d < sh.nd; ++d)
      if ((long long)shapes[i][d] != sh.d[d])
        return set_error(MZGO_EINVAL, "%s: '%s': dim %d is %lld, expected %lld", fn, keys[i], d, (long long)shapes[i][d],
                         sh.d[d]);
    P[k] = data[i];
    if (grads && Gd) Gd[k] = grads[i];
  }
  for (int k = 0; k < WK_COUNT; ++k) {
    if ((need & bit(k)) && !P[k]) return set_error(MZGO_EINVAL, "%s: missing weight '%s'", fn, kWeightKeyNames[k]);
    if ((need_grad & bit(k)) && !(Gd && Gd[k])) return set_error(MZGO_EINVAL, "%s: null gradient for '%s'", fn, kWeightKeyNames[k]);
  }
  return MZGO_OK;
}

int check_dims(const char* fn, int B, int K, int C, int N, int emb_rows) {
  if (B < 1) return set_error(MZGO_EINVAL, "%s: B must be >= 1, got %d", fn, B);
  if (K < 0) return set_error(MZGO_EINVAL, "%s: K must be >= 0, got %d", fn, K);
  if (C < 16 || C % 16) return set_error(MZGO_EINVAL, "%s: C must be a multiple of 16, got %d", fn, C);
  if (N < 2 || N > 19) return set_error(MZGO_EINVAL, "%s: N %d out of range (2..19)", fn, N);
  if (emb_rows < N * N + 1)
    return set_error(MZGO_EINVAL, "%s: emb_rows %d < N*N + 1 = %d actions", fn, emb_rows, N * N + 1);
  if (((int64_t)K + 1) * B > INT32_MAX)                  // a workgroup per (step, sample); int indices
    return set_error(MZGO_EINVAL, "%s: (K + 1) B = %lld exceeds 2^31 - 1", fn, (long long)(((int64_t)K + 1) * B));
  if (B > kConvMaxBatch)                                 // the convs and the chain launch a grid with z = B
    return set_error(MZGO_EINVAL, "%s: B = %d exceeds the launch grid's z limit of %d", fn, B, kConvMaxBatch);
  return MZGO_OK;
}

int check_precision(const char* fn, int precision, int C) {
  if (precision != MZGO_PREC_F32 && precision != MZGO_PREC_BF16)
    return set_error(MZGO_EINVAL, "%s: unknown precision %d (MZGO_PREC_F32 = 0, MZGO_PREC_BF16 = 1)", fn, precision);
  if (precision == MZGO_PREC_BF16 && C % 32)
    return set_error(MZGO_EINVAL, "%s: C must be a multiple of 32 in bf16 mode, got %d", fn, C);
  return MZGO_OK;
}

// ---------------------------------------------------------------------------
// the two caller-owned buffers: offsets in floats, every part a multiple of 64
// ---------------------------------------------------------------------------
struct Layout {
  size_t LS;                                            // floats of one step's latents [B][C][CELLS]
  int CT;                                               // 16-cell tiles of a board
  int dyn_cb;                                           // boards per chunk of the dynamics' weight pass
  // saved
  size_t s_obs, s_x1, s_x2, s_lat, s_vmean, s_rmean, s_acts, s_wpk, saved_floats;
  // work
  size_t w_G, w_g2, w_g1, w_bsum, w_hp, w_conv, work_floats;
};

size_t pad64(size_t n) { return (n + 63) / 64 * 64; }

Layout layout(int B, int K, int C, int N, int precision) {
  Layout L{};
  const size_t CELLS = (size_t)N * N, S = (size_t)K + 1;
  L.LS = (size_t)B * C * CELLS;
  L.CT = (int)((CELLS + 15) / 16);
  size_t o = 0;
  auto take = [&](size_t n) { const size_t at = o; o += pad64(n); return at; };
  L.s_obs = take((size_t)B * 6 * CELLS);
  L.s_x1 = take((size_t)B * kRepC * CELLS);
  L.s_x2 = take((size_t)B * kRepC * CELLS);
  L.s_lat = take(S * L.LS);
  L.s_vmean = take(S * B);
  L.s_rmean = take(S * B);
  L.s_acts = take((size_t)2 * K * B);                    // int64 [K][B]
  L.s_wpk = o;                                           // bf16 mode: the dynamics conv's two packed layouts
  if (precision == MZGO_PREC_BF16) take(conv_bf16_packed_bytes(C, C) / sizeof(float));
  L.saved_floats = o;
  o = 0;
  L.w_G = take(S * L.LS);
  L.w_g2 = take((size_t)B * kRepC * CELLS);
  L.w_g1 = take((size_t)B * kRepC * CELLS);
  L.w_bsum = take((size_t)K * B * C * L.CT);
  L.w_hp = take(S * B * head_part_stride(C));
  // the conv weight partials: one region, used by one layer at a time
  L.dyn_cb = 8;
  size_t cw = std::max(conv_bwd_workspace_bytes(B, kRepC, C),
                       std::max(conv_bwd_workspace_bytes(B, kRepC, kRepC), conv_bwd_workspace_bytes(B, 6, kRepC)));
  if (K > 0) {
    // (one chunk of all K B boards is the least there is: a wide C stays above the cap)
    while (L.dyn_cb < K * B && conv_bwd_workspace_bytes_chunk(K * B, C, C, L.dyn_cb) > kDynWorkspaceCap)
      L.dyn_cb += 8;
    cw = std::max(cw, conv_bwd_workspace_bytes_chunk(K * B, C, C, L.dyn_cb));
  }
  L.w_conv = take(cw / sizeof(float));
  L.work_floats = o;
  return L;
}

// ---------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

struct HeadW {
  const float *pol_w, *pol_b, *val_w, *val_b, *vfc_w, *vfc_b, *pass, *rew_w, *rew_b, *fc1_w, *fc1_b, *fc2_w, *fc2_b;
};
struct HeadG {
  float *pol_w, *pol_b, *val_w, *val_b, *vfc_w, *vfc_b, *pass, *rew_w, *rew_b, *fc1_w, *fc1_b, *fc2_w, *fc2_b;
};

// the observations kept for the backward, and acts [B][K] -> acts_t [K][B]
__global__ void __launch_bounds__(256) k_unroll_stage(const float* __restrict__ obs0, size_t n_obs,
                                                      float* __restrict__ obs, const int64_t* __restrict__ acts,
                                                      int B, int K, int64_t* __restrict__ acts_t) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n_obs) obs[i] = obs0[i];
  if (i < (size_t)K * B) {
    const int k = (int)(i / B), b = (int)(i - (size_t)k * B);
    acts_t[i] = acts[(size_t)b * K + k];
  }
}

// The three heads of latent (s, b) = blockIdx.x.  The 1x1 convs' channel sums
// are split over G = max(1, 256 / CELLS) channel groups, a thread per (group,
// cell) summing its channels in order; then a thread per cell sums the groups
// in order, and wave 0 forms the two board means (a strided pass per lane,
// then a butterfly).  All orders depend on (C, CELLS) alone.
__global__ void __launch_bounds__(kHeadThreads) k_unroll_heads(HeadW W, const float* __restrict__ lat, int B, int C,
                                                               int CELLS, float* __restrict__ logits,
                                                               float* __restrict__ value, float* __restrict__ reward,
                                                               float* __restrict__ vmean, float* __restrict__ rmean) {
  __shared__ float part[3][kMaxCells + 7];               // G * CELLS <= max(256, CELLS) entries
  __shared__ float cellv[2][kMaxCells + 7];
  const int tid = threadIdx.x;
  const size_t sb = blockIdx.x;
  const int s = (int)(sb / B), b = (int)(sb - (size_t)s * B);
  const int A = CELLS + 1;
  const float* x = lat + sb * C * CELLS;
  const int G = max(1, kHeadThreads / CELLS), Cg = (C + G - 1) / G;
  for (int i = tid; i < G * CELLS; i += kHeadThreads) {
    const int g = i / CELLS, p = i - g * CELLS;
    const int c1 = min(C, (g + 1) * Cg);
    float ap = 0.f, av = 0.f, ar = 0.f;
    for (int c = g * Cg; c < c1; ++c) {
      const float xv = x[(size_t)c * CELLS + p];
      ap += W.pol_w[c] * xv;
      av += W.val_w[c] * xv;
      ar += W.rew_w[c] * xv;
    }
    part[0][i] = ap;
    part[1][i] = av;
    part[2][i] = ar;
  }
  __syncthreads();
  const float pol_b = *W.pol_b, val_b = *W.val_b, rew_b = *W.rew_b;
  for (int p = tid; p < CELLS; p += kHeadThreads) {
    float sp = 0.f, sv = 0.f, sr = 0.f;
    for (int g = 0; g < G; ++g) {
      sp += part[0][g * CELLS + p];
      sv += part[1][g * CELLS + p];
      sr += part[2][g * CELLS + p];
    }
    logits[sb * A + p] = sp + pol_b;
    cellv[0][p] = sv + val_b;
    cellv[1][p] = sr + rew_b;
  }
  __syncthreads();
  if (tid < 64) {
    float sv = 0.f, sr = 0.f;
    for (int p = tid; p < CELLS; p += 64) {
      sv += cellv[0][p];
      sr += cellv[1][p];
    }
    sv = wave_sum(sv);
    sr = wave_sum(sr);
    if (tid == 0) {
      const float vm = sv / (float)CELLS, rm = sr / (float)CELLS;
      vmean[sb] = vm;
      rmean[sb] = rm;
      value[sb] = heads_value(vm, *W.vfc_w, *W.vfc_b);
      logits[sb * A + CELLS] = *W.pass;
      if (s > 0) reward[(size_t)(s - 1) * B + b] = heads_reward(rm, W.fc1_w, W.fc1_b, W.fc2_w, *W.fc2_b);
    }
  }
}

// The heads' backward of latent (s, b) = blockIdx.x: G[s][b] (every entry
// written), and the latent's row of partial sums for the head tensors.  A wave
// per channel (c = wave, wave + 4, ...): the cells strided over the lanes,
// then a butterfly.
__global__ void __launch_bounds__(kHeadThreads) k_unroll_heads_bwd(HeadW W, const float* __restrict__ lat,
                                                                   const float* __restrict__ g_logits,
                                                                   const float* __restrict__ g_value,
                                                                   const float* __restrict__ g_reward,
                                                                   const float* __restrict__ vmean,
                                                                   const float* __restrict__ rmean, int B, int C,
                                                                   int CELLS, float* __restrict__ G,
                                                                   float* __restrict__ hp) {
  __shared__ float gl[kMaxCells + 7];
  __shared__ float sc[2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t sb = blockIdx.x;
  const int s = (int)(sb / B), b = (int)(sb - (size_t)s * B);
  const int A = CELLS + 1;
  float* row = hp + sb * head_part_stride(C);
  for (int p = tid; p < CELLS; p += kHeadThreads) gl[p] = g_logits[sb * A + p];
  if (tid == 0) {
    const float dvmean = heads_value_grad(g_value[sb], vmean[sb], *W.vfc_w, &row[head_part_scalar(C, HS_VFC_W)],
                                          &row[head_part_scalar(C, HS_VFC_B)]);
    row[head_part_scalar(C, HS_VALUE_B)] = dvmean;
    row[head_part_scalar(C, HS_PASS)] = g_logits[sb * A + CELLS];
    float drmean = 0.f, dr = 0.f;
    float* g1w = row + head_part_fc1_w(C);
    float* g1b = row + head_part_fc1_b(C);
    float* g2w = row + head_part_fc2_w(C);
    if (s > 0) {
      dr = g_reward[(size_t)(s - 1) * B + b];
      drmean = heads_reward_grad(dr, rmean[sb], W.fc1_w, W.fc1_b, W.fc2_w, g1w, g1b, g2w);
    } else {
      for (int j = 0; j < kRewardHidden; ++j) g1w[j] = g1b[j] = g2w[j] = 0.f;
    }
    row[head_part_scalar(C, HS_FC2_B)] = dr;
    row[head_part_scalar(C, HS_REWARD_B)] = drmean;
    sc[0] = dvmean;
    sc[1] = drmean;
  }
  __syncthreads();
  const float dvmean = sc[0], drmean = sc[1], cells = (float)CELLS;
  if (wave == 0) {
    float sp = 0.f;
    for (int p = lane; p < CELLS; p += 64) sp += gl[p];
    sp = wave_sum(sp);
    if (lane == 0) row[head_part_scalar(C, HS_POLICY_B)] = sp;
  }
  const float* x = lat + sb * C * CELLS;
  float* Gx = G + sb * C * CELLS;
  for (int c = wave; c < C; c += kHeadThreads / 64) {
    const float wp = W.pol_w[c], wv = W.val_w[c], wr = W.rew_w[c];
    float dot = 0.f, xs = 0.f;
    for (int p = lane; p < CELLS; p += 64) {
      const float xv = x[(size_t)c * CELLS + p];
      dot += gl[p] * xv;
      xs += xv;
      Gx[(size_t)c * CELLS + p] = heads_latent_grad(wp, gl[p], wv, dvmean, wr, drmean, cells);
    }
    dot = wave_sum(dot);
    xs = wave_sum(xs);
    if (lane == 0) {
      row[c] = dot;
      row[C + c] = (dvmean / cells) * xs;
      row[2 * C + c] = (drmean / cells) * xs;
    }
  }
}

// entry j = blockIdx.x of the rows summed over the (K+1) B latents: lane l
// sums rows l, l + 64, ... in order, then a butterfly; a null destination (the
// reward head at K = 0) is skipped
__global__ void __launch_bounds__(64) k_unroll_heads_reduce(const float* __restrict__ hp, int rows, int C, HeadG D) {
  const int j = blockIdx.x, lane = threadIdx.x;
  const int stride = head_part_stride(C);
  float s = 0.f;
  for (int r = lane; r < rows; r += 64) s += hp[(size_t)r * stride + j];
  s = wave_sum(s);
  if (lane != 0) return;
  float* dst;
  if (j < C) dst = D.pol_w ? D.pol_w + j : nullptr;
  else if (j < 2 * C) dst = D.val_w ? D.val_w + (j - C) : nullptr;
  else if (j < 3 * C) dst = D.rew_w ? D.rew_w + (j - 2 * C) : nullptr;
  else if (j < 3 * C + 16) dst = D.fc1_w ? D.fc1_w + (j - 3 * C) : nullptr;
  else if (j < 3 * C + 32) dst = D.fc1_b ? D.fc1_b + (j - 3 * C - 16) : nullptr;
  else if (j < 3 * C + 48) dst = D.fc2_w ? D.fc2_w + (j - 3 * C - 32) : nullptr;
  else {
    switch (j - 3 * C - 48) {
      case HS_POLICY_B: dst = D.pol_b; break;
      case HS_VALUE_B: dst = D.val_b; break;
      case HS_VFC_W: dst = D.vfc_w; break;
      case HS_VFC_B: dst = D.vfc_b; break;
      case HS_PASS: dst = D.pass; break;
      case HS_REWARD_B: dst = D.rew_b; break;
      default: dst = D.fc2_b; break;
    }
  }
  if (dst) *dst = s;
}

// gemb[row][c] = the board sums of the (step, sample) pairs whose action is
// `row`, in (step, sample) order; every other row 0.  A thread per entry.
__global__ void __launch_bounds__(256) k_unroll_emb_grad(const float* __restrict__ bsum,
                                                         const int64_t* __restrict__ acts_t, int KB, int C, int CT,
                                                         int emb_rows, float* __restrict__ gemb) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)emb_rows * C) return;
  const int64_t row = (int64_t)(idx / C);
  const int c = (int)(idx - (size_t)row * C);
  float s = 0.f;
  for (int i = 0; i < KB; ++i) {
    if (acts_t[i] != row) continue;
    const float* t = bsum + ((size_t)i * C + c) * CT;
    float bs = 0.f;
    for (int j = 0; j < CT; ++j) bs += t[j];
    s += bs;
  }
  gemb[idx] = s;
}

// G += g: the caller's gradient with respect to the latents added to the heads', before the chain.  A thread
// per four floats (n4 of them: every step's latents are a multiple of 16 floats, both bases 16-byte aligned).
__global__ void __launch_bounds__(256) k_unroll_latent_grad_add(float4* __restrict__ G, const float4* __restrict__ g,
                                                                size_t n4) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  const float4 a = G[i], b = g[i];
  G[i] = make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
}

HeadW head_weights(const float* const* P) {
  return HeadW{P[WK_POLICY_W], P[WK_POLICY_B], P[WK_VALUE_W], P[WK_VALUE_B], P[WK_VFC_W], P[WK_VFC_B],
               P[WK_PASS_LOGIT], P[WK_REWARD_W], P[WK_REWARD_B], P[WK_FC1_W], P[WK_FC1_B], P[WK_FC2_W], P[WK_FC2_B]};
}
HeadG head_grads(float* const* G) {
  return HeadG{G[WK_POLICY_W], G[WK_POLICY_B], G[WK_VALUE_W], G[WK_VALUE_B], G[WK_VFC_W], G[WK_VFC_B],
               G[WK_PASS_LOGIT], G[WK_REWARD_W], G[WK_REWARD_B], G[WK_FC1_W], G[WK_FC1_B], G[WK_FC2_W], G[WK_FC2_B]};
}

// The dynamics conv's weights in the call's precision, and its three matrix products on them: mzgo_train.hip's
// float32 launchers from `w`, or mzgo_conv_bf16.hip's from `packed` (conv_bf16_pack's two layouts, in `saved`)
struct DynConv {
  int precision;
  const float* w;
  const void* packed;
};

// latent [B][C][N][N] (+ emb[action]) -> y
hipError_t dyn_forward(const DynConv& d, const float* x, const int64_t* action, const float* emb, const float* bias,
                       int B, int C, int N, float* y, hipStream_t s) {
  if (d.precision == MZGO_PREC_BF16)
    return conv_bf16_forward(x, action, emb, d.packed, nullptr, bias, B, C, C, N, y, s);
  return conv_forward(x, action, emb, d.w, bias, B, C, C, N, y, s);
}

// a step of the chain: the input gradient from g [out > 0] ADDED into dst, its 16-cell tile sums to bsum
hipError_t dyn_input_grad(const DynConv& d, const float* g, const float* out, int B, int C, int N, float* dst,
                          float* bsum, hipStream_t s) {
  if (d.precision == MZGO_PREC_BF16)
    return conv_bf16_input_grad(g, out, d.packed, B, C, C, N, dst, 1, bsum, s);
  return conv_input_grad(g, out, d.w, B, C, C, N, dst, 1, bsum, s);
}

// the weight gradient's partials over chunks of `cb` of the `boards` boards
hipError_t dyn_weight_partials(const DynConv& d, const float* g, const float* out, const float* x,
                               const int64_t* action, const float* emb, int boards, int C, int N, int cb, float* part,
                               hipStream_t s) {
  if (d.precision == MZGO_PREC_BF16)
    return conv_bf16_weight_partials(g, out, x, action, emb, boards, C, C, N, cb, part, s);
  return conv_weight_partials(g, out, x, action, emb, boards, C, C, N, cb, part, s);
}

}  // namespace

extern "C" {

int mzgo_unroll_workspace(int B, int K, int C, int N, int emb_rows, int64_t* saved_bytes, int64_t* work_bytes) {
  return mzgo_unroll_workspace_p(B, K, C, N, emb_rows, MZGO_PREC_F32, saved_bytes, work_bytes);
}

int mzgo_unroll_workspace_p(int B, int K, int C, int N, int emb_rows, int precision, int64_t* saved_bytes,
                            int64_t* work_bytes) {
  if (int rc = check_dims("mzgo_unroll_workspace", B, K, C, N, emb_rows)) return rc;
  if (int rc = check_precision("mzgo_unroll_workspace", precision, C)) return rc;
  if (!saved_bytes || !work_bytes)
    return set_error(MZGO_EINVAL, "mzgo_unroll_workspace: null %s", !saved_bytes ? "saved_bytes" : "work_bytes");
  const Layout L = layout(B, K, C, N, precision);
  *saved_bytes = (int64_t)(L.saved_floats * sizeof(float));
  *work_bytes = (int64_t)(L.work_floats * sizeof(float));
  return MZGO_OK;
}

int mzgo_unroll_latents(int B, int K, int C, int N, int emb_rows, int precision, int64_t* offset_bytes,
                        int64_t* bytes) {
  if (int rc = check_dims("mzgo_unroll_latents", B, K, C, N, emb_rows)) return rc;
  if (int rc = check_precision("mzgo_unroll_latents", precision, C)) return rc;
  if (!offset_bytes || !bytes)
    return set_error(MZGO_EINVAL, "mzgo_unroll_latents: null %s", !offset_bytes ? "offset_bytes" : "bytes");
  const Layout L = layout(B, K, C, N, precision);
  *offset_bytes = (int64_t)(L.s_lat * sizeof(float));
  *bytes = (int64_t)(((size_t)K + 1) * L.LS * sizeof(float));
  return MZGO_OK;
}

int mzgo_unroll_forward(const char* const* keys, const float* const* params, const int64_t* const* shapes,
                        const int* ndims, int n_params, const float* obs0, const int64_t* acts, int B, int K, int C,
                        int N, int emb_rows, void* saved, int64_t saved_bytes, float* logits, float* value,
                        float* reward, void* stream) {
  return mzgo_unroll_forward_p(keys, params, shapes, ndims, n_params, obs0, acts, B, K, C, N, emb_rows, saved,
                               saved_bytes, logits, value, reward, MZGO_PREC_F32, stream);
}

int mzgo_unroll_forward_p(const char* const* keys, const float* const* params, const int64_t* const* shapes,
                          const int* ndims, int n_params, const float* obs0, const int64_t* acts, int B, int K, int C,
                          int N, int emb_rows, void* saved, int64_t saved_bytes, float* logits, float* value,
                          float* reward, int precision, void* stream) {
  const char* fn = "mzgo_unroll_forward";
  if (int rc = check_dims(fn, B, K, C, N, emb_rows)) return rc;
  if (int rc = check_precision(fn, precision, C)) return rc;
  const char* null = !obs0 ? "obs0" : !saved ? "saved" : !logits ? "logits" : !value ? "value" : nullptr;
  if (!null && K > 0) null = !acts ? "acts" : !reward ? "reward" : nullptr;
  if (null) return set_error(MZGO_EINVAL, "%s: null %s", fn, null);
  const float* P[WK_COUNT];
  if (int rc = resolve(fn, keys, params, shapes, ndims, nullptr, n_params, C, emb_rows, kAllSet, kAllSet, 0, P,
                       nullptr))
    return rc;
  const Layout L = layout(B, K, C, N, precision);
  if (saved_bytes < (int64_t)(L.saved_floats * sizeof(float)))
    return set_error(MZGO_EINVAL, "%s: saved too small: %lld < %lld bytes", fn, (long long)saved_bytes,
                     (long long)(L.saved_floats * sizeof(float)));
  hipStream_t s = (hipStream_t)stream;
  float* sv = static_cast<float*>(saved);
  float *obs = sv + L.s_obs, *x1 = sv + L.s_x1, *x2 = sv + L.s_x2, *lat = sv + L.s_lat;
  int64_t* acts_t = reinterpret_cast<int64_t*>(sv + L.s_acts);
  const int CELLS = N * N;
  const size_t n_obs = (size_t)B * 6 * CELLS, n_stage = std::max(n_obs, (size_t)K * B);
  hipLaunchKernelGGL(k_unroll_stage, dim3((unsigned)((n_stage + 255) / 256)), dim3(256), 0, s, obs0, n_obs, obs, acts, B,
                     K, acts_t);
  MZGO_HIPCHK(hipGetLastError());
  MZGO_HIPCHK(conv_forward(obs, nullptr, nullptr, P[WK_CONV1_W], P[WK_CONV1_B], B, 6, kRepC, N, x1, s));
  MZGO_HIPCHK(conv_forward(x1, nullptr, nullptr, P[WK_CONV2_W], P[WK_CONV2_B], B, kRepC, kRepC, N, x2, s));
  MZGO_HIPCHK(conv_forward(x2, nullptr, nullptr, P[WK_CONV3_W], P[WK_CONV3_B], B, kRepC, C, N, lat, s));
  // bf16: R(W) once, in the forward's and the input gradient's layouts; the backward call reads them from `saved`
  if (precision == MZGO_PREC_BF16 && K > 0) MZGO_HIPCHK(conv_bf16_pack(P[WK_DYN_W], C, C, sv + L.s_wpk, s));
  const DynConv dyn{precision, P[WK_DYN_W], sv + L.s_wpk};
  for (int k = 1; k <= K; ++k)
    MZGO_HIPCHK(dyn_forward(dyn, lat + (size_t)(k - 1) * L.LS, acts_t + (size_t)(k - 1) * B, P[WK_EMB], P[WK_DYN_B], B,
                            C, N, lat + (size_t)k * L.LS, s));
  hipLaunchKernelGGL(k_unroll_heads, dim3((unsigned)((K + 1) * B)), dim3(kHeadThreads), 0, s, head_weights(P), lat, B, C,
                     CELLS, logits, value, reward, sv + L.s_vmean, sv + L.s_rmean);
  MZGO_HIPCHK(hipGetLastError());
  return MZGO_OK;
}

// The representation alone (the consistency loss's targets): the forward's three
// convs without the staging copy, the heads and the saved buffer.  A batch past
// the convs' grid limit goes through in chunks of kConvMaxBatch boards; a
// board's conv does not depend on its neighbours, so the bits are the unroll's.
static int encode_check(const char* fn, int B, int C, int N, int emb_rows) {
  if (int rc = check_dims(fn, 1, 0, C, N, emb_rows)) return rc;
  if (B < 1) return set_error(MZGO_EINVAL, "%s: B must be >= 1, got %d", fn, B);
  return MZGO_OK;
}
static size_t encode_work_floats(int B, int N) {
  return 2 * (size_t)std::min(B, kConvMaxBatch) * kRepC * N * N;
}

int mzgo_encode_workspace(int B, int C, int N, int64_t* work_bytes) {
  if (int rc = encode_check("mzgo_encode_workspace", B, C, N, N * N + 1)) return rc;
  if (!work_bytes) return set_error(MZGO_EINVAL, "mzgo_encode_workspace: null work_bytes");
  *work_bytes = (int64_t)(encode_work_floats(B, N) * sizeof(float));
  return MZGO_OK;
}

int mzgo_encode(const char* const* keys, const float* const* params, const int64_t* const* shapes, const int* ndims,
                int n_params, const float* obs, int B, int C, int N, int emb_rows, float* latents, void* work,
                int64_t work_bytes, void* stream) {
  const char* fn = "mzgo_encode";
  if (int rc = encode_check(fn, B, C, N, emb_rows)) return rc;
  const char* null = !obs ? "obs" : !latents ? "latents" : !work ? "work" : nullptr;
  if (null) return set_error(MZGO_EINVAL, "%s: null %s", fn, null);
  const float* P[WK_COUNT];
  constexpr unsigned kRepSet = bit(WK_CONV1_W) | bit(WK_CONV1_B) | bit(WK_CONV2_W) | bit(WK_CONV2_B) |
                               bit(WK_CONV3_W) | bit(WK_CONV3_B);
  if (int rc = resolve(fn, keys, params, shapes, ndims, nullptr, n_params, C, emb_rows, kAllSet, kRepSet, 0, P, nullptr))
    return rc;
  if (work_bytes < (int64_t)(encode_work_floats(B, N) * sizeof(float)))
    return set_error(MZGO_EINVAL, "%s: work too small: %lld < %lld bytes", fn, (long long)work_bytes,
                     (long long)(encode_work_floats(B, N) * sizeof(float)));
  hipStream_t s = (hipStream_t)stream;
  const int CELLS = N * N;
  float* x1 = static_cast<float*>(work);
  float* x2 = x1 + (size_t)std::min(B, kConvMaxBatch) * kRepC * CELLS;
  for (int b0 = 0; b0 < B; b0 += kConvMaxBatch) {
    const int cb = std::min(B - b0, kConvMaxBatch);
    MZGO_HIPCHK(conv_forward(obs + (size_t)b0 * 6 * CELLS, nullptr, nullptr, P[WK_CONV1_W], P[WK_CONV1_B], cb, 6, kRepC,
                             N, x1, s));
    MZGO_HIPCHK(conv_forward(x1, nullptr, nullptr, P[WK_CONV2_W], P[WK_CONV2_B], cb, kRepC, kRepC, N, x2, s));
    MZGO_HIPCHK(conv_forward(x2, nullptr, nullptr, P[WK_CONV3_W], P[WK_CONV3_B], cb, kRepC, C, N,
                             latents + (size_t)b0 * C * CELLS, s));
  }
  return MZGO_OK;
}

int mzgo_unroll_backward(const char* const* keys, const float* const* params, const int64_t* const* shapes,
                         const int* ndims, float* const* grads, int n_params, const void* saved, int64_t saved_bytes,
                         const float* g_logits, const float* g_value, const float* g_reward, int B, int K, int C, int N,
                         int emb_rows, void* work, int64_t work_bytes, void* stream) {
  return mzgo_unroll_backward_p(keys, params, shapes, ndims, grads, n_params, saved, saved_bytes, g_logits, g_value,
                                g_reward, B, K, C, N, emb_rows, work, work_bytes, MZGO_PREC_F32, stream);
}

int mzgo_unroll_backward_p(const char* const* keys, const float* const* params, const int64_t* const* shapes,
                           const int* ndims, float* const* grads, int n_params, const void* saved,
                           int64_t saved_bytes, const float* g_logits, const float* g_value, const float* g_reward,
                           int B, int K, int C, int N, int emb_rows, void* work, int64_t work_bytes, int precision,
                           void* stream) {
  return mzgo_unroll_backward_l(keys, params, shapes, ndims, grads, n_params, saved, saved_bytes, g_logits, g_value,
                                g_reward, nullptr, B, K, C, N, emb_rows, work, work_bytes, precision, stream);
}

int mzgo_unroll_backward_l(const char* const* keys, const float* const* params, const int64_t* const* shapes,
                           const int* ndims, float* const* grads, int n_params, const void* saved,
                           int64_t saved_bytes, const float* g_logits, const float* g_value, const float* g_reward,
                           const float* g_latent, int B, int K, int C, int N, int emb_rows, void* work,
                           int64_t work_bytes, int precision, void* stream) {
  const char* fn = "mzgo_unroll_backward";
  if (int rc = check_dims(fn, B, K, C, N, emb_rows)) return rc;
  if (int rc = check_precision(fn, precision, C)) return rc;
  const char* null = !saved ? "saved" : !g_logits ? "g_logits" : !g_value ? "g_value" : !work ? "work"
                     : !grads ? "grads" : nullptr;
  if (!null && K > 0 && !g_reward) null = "g_reward";
  if (null) return set_error(MZGO_EINVAL, "%s: null %s", fn, null);
  if (g_latent && ((uintptr_t)g_latent & 15 || (uintptr_t)work & 15))
    return set_error(MZGO_EINVAL, "%s: g_latent and work must be 16-byte aligned", fn);
  const float* P[WK_COUNT];
  float* Gd[WK_COUNT];
  if (int rc = resolve(fn, keys, params, shapes, ndims, grads, n_params, C, emb_rows, kAllSet, kAllSet,
                       K > 0 ? kAllSet : kAllSet & ~kDynSet, P, Gd))
    return rc;
  const Layout L = layout(B, K, C, N, precision);
  if (saved_bytes < (int64_t)(L.saved_floats * sizeof(float)))
    return set_error(MZGO_EINVAL, "%s: saved too small: %lld < %lld bytes", fn, (long long)saved_bytes,
                     (long long)(L.saved_floats * sizeof(float)));
  if (work_bytes < (int64_t)(L.work_floats * sizeof(float)))
    return set_error(MZGO_EINVAL, "%s: work too small: %lld < %lld bytes", fn, (long long)work_bytes,
                     (long long)(L.work_floats * sizeof(float)));
  hipStream_t s = (hipStream_t)stream;
  const float* sv = static_cast<const float*>(saved);
  const float *obs = sv + L.s_obs, *x1 = sv + L.s_x1, *x2 = sv + L.s_x2, *lat = sv + L.s_lat;
  const int64_t* acts_t = reinterpret_cast<const int64_t*>(sv + L.s_acts);
  float* wk = static_cast<float*>(work);
  float *G = wk + L.w_G, *g2 = wk + L.w_g2, *g1 = wk + L.w_g1, *bsum = wk + L.w_bsum, *hp = wk + L.w_hp;
  float* cw = wk + L.w_conv;                          // the conv weight partials
  const int CELLS = N * N, rows = (K + 1) * B;
  if (K == 0)                                           // (the reward head has no gradient: skipped by the reduce)
    for (int k = 0; k < WK_COUNT; ++k)
      if (kDynSet & bit(k)) Gd[k] = nullptr;

  // (a) the heads
  hipLaunchKernelGGL(k_unroll_heads_bwd, dim3((unsigned)rows), dim3(kHeadThreads), 0, s, head_weights(P), lat, g_logits,
                     g_value, g_reward, sv + L.s_vmean, sv + L.s_rmean, B, C, CELLS, G, hp);
  MZGO_HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(k_unroll_heads_reduce, dim3((unsigned)(3 * C + 48 + HS_COUNT)), dim3(64), 0, s, hp, rows, C,
                     head_grads(Gd));
  MZGO_HIPCHK(hipGetLastError());
  if (g_latent) {
    // (a') the caller's latent gradient, laid out like the latents: G is the gradient with respect to the post-ReLU
    // latents and the chain and the representation mask with the saved latents, so an addition is all it takes
    const size_t n4 = ((size_t)K + 1) * L.LS / 4;
    hipLaunchKernelGGL(k_unroll_latent_grad_add, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s,
                       reinterpret_cast<float4*>(G), reinterpret_cast<const float4*>(g_latent), n4);
    MZGO_HIPCHK(hipGetLastError());
  }
  if (K > 0) {
    // (b) the chain: step s's input gradient into step s - 1's latent gradient (bf16: from the packed weights the
    // forward left in `saved`)
    const DynConv dyn{precision, P[WK_DYN_W], sv + L.s_wpk};
    for (int st = K; st >= 1; --st)
      MZGO_HIPCHK(dyn_input_grad(dyn, G + (size_t)st * L.LS, lat + (size_t)st * L.LS, B, C, N,
                                 G + (size_t)(st - 1) * L.LS, bsum + (size_t)(st - 1) * B * C * L.CT, s));
    // (c) the dynamics conv's weight and bias: steps 0..K-1 are the inputs, 1..K the outputs of K B boards; the
    // reduce and the bias gradient are float32 in both precisions
    const int chunks = (K * B + L.dyn_cb - 1) / L.dyn_cb;
    MZGO_HIPCHK(dyn_weight_partials(dyn, G + L.LS, lat + L.LS, lat, acts_t, P[WK_EMB], K * B, C, N, L.dyn_cb, cw, s));
    MZGO_HIPCHK(conv_bwd_reduce(cw, Gd[WK_DYN_W], chunks, (size_t)C * C * 9, s));
    MZGO_HIPCHK(conv_bwd_bias(G + L.LS, lat + L.LS, Gd[WK_DYN_B], K * B, C, N, s));
    // (d) the embedding
    const size_t n_emb = (size_t)emb_rows * C;
    hipLaunchKernelGGL(k_unroll_emb_grad, dim3((unsigned)((n_emb + 255) / 256)), dim3(256), 0, s, bsum, acts_t, K * B, C,
                       L.CT, emb_rows, Gd[WK_EMB]);
    MZGO_HIPCHK(hipGetLastError());
  }
  // (e) the representation, from the saved activations
  MZGO_HIPCHK(conv_backward(G, lat, x2, nullptr, nullptr, P[WK_CONV3_W], B, kRepC, C, N, g2, Gd[WK_CONV3_W],
                            Gd[WK_CONV3_B], cw, s));
  MZGO_HIPCHK(conv_backward(g2, x2, x1, nullptr, nullptr, P[WK_CONV2_W], B, kRepC, kRepC, N, g1, Gd[WK_CONV2_W],
                            Gd[WK_CONV2_B], cw, s));
  MZGO_HIPCHK(conv_backward(g1, x1, obs, nullptr, nullptr, P[WK_CONV1_W], B, 6, kRepC, N, nullptr, Gd[WK_CONV1_W],
                            Gd[WK_CONV1_B], cw, s));
  return MZGO_OK;
}

int mzgo_unroll_heads_host(const char* const* keys, const float* const* params, const int64_t* const* shapes,
                           const int* ndims, float* const* grads, int n_params, const float* latents, int S, int B,
                           int C, int N, float* logits, float* value, float* reward, const float* g_logits,
                           const float* g_value, const float* g_reward, float* g_latent) {
  const char* fn = "mzgo_unroll_heads_host";
  if (S < 1) return set_error(MZGO_EINVAL, "%s: S must be >= 1, got %d", fn, S);
  if (int rc = check_dims(fn, B, S - 1, C, N, N * N + 1)) return rc;
  const char* null = !latents ? "latents" : !logits ? "logits" : !value ? "value" : !g_logits ? "g_logits"
                     : !g_value ? "g_value" : !g_latent ? "g_latent" : !grads ? "grads" : nullptr;
  if (!null && S > 1) null = !reward ? "reward" : !g_reward ? "g_reward" : nullptr;
  if (null) return set_error(MZGO_EINVAL, "%s: null %s", fn, null);
  const float* P[WK_COUNT];
  float* Gd[WK_COUNT];
  if (int rc = resolve(fn, keys, params, shapes, ndims, grads, n_params, C, N * N + 1, kHeadSet, kHeadSet,
                       S > 1 ? kHeadSet : kHeadSet & ~kDynSet, P, Gd))
    return rc;
  const int CELLS = N * N, A = CELLS + 1;
  const HeadW W = head_weights(P);
  const HeadG D = head_grads(Gd);
  const bool rew = S > 1;
  for (int c = 0; c < C; ++c) {
    D.pol_w[c] = D.val_w[c] = 0.f;
    if (rew) D.rew_w[c] = 0.f;
  }
  *D.pol_b = *D.val_b = *D.vfc_w = *D.vfc_b = *D.pass = 0.f;
  if (rew) {
    *D.rew_b = *D.fc2_b = 0.f;
    for (int j = 0; j < kRewardHidden; ++j) D.fc1_w[j] = D.fc1_b[j] = D.fc2_w[j] = 0.f;
  }
  const float cells = (float)CELLS;
  for (size_t sb = 0; sb < (size_t)S * B; ++sb) {
    const int s = (int)(sb / B), b = (int)(sb % B);
    const float* x = latents + sb * C * CELLS;
    // forward
    float sv = 0.f, sr = 0.f;
    for (int p = 0; p < CELLS; ++p) {
      float ap = 0.f, av = 0.f, ar = 0.f;
      for (int c = 0; c < C; ++c) {
        const float xv = x[(size_t)c * CELLS + p];
        ap += W.pol_w[c] * xv;
        av += W.val_w[c] * xv;
        ar += W.rew_w[c] * xv;
      }
      logits[sb * A + p] = ap + *W.pol_b;
      sv += av + *W.val_b;
      sr += ar + *W.rew_b;
    }
    logits[sb * A + CELLS] = *W.pass;
    const float vm = sv / cells, rm = sr / cells;
    value[sb] = heads_value(vm, *W.vfc_w, *W.vfc_b);
    if (s > 0) reward[(size_t)(s - 1) * B + b] = heads_reward(rm, W.fc1_w, W.fc1_b, W.fc2_w, *W.fc2_b);
    // backward
    const float* gl = g_logits + sb * A;
    float gw, gb;
    const float dvmean = heads_value_grad(g_value[sb], vm, *W.vfc_w, &gw, &gb);
    *D.vfc_w += gw;
    *D.vfc_b += gb;
    *D.val_b += dvmean;
    *D.pass += gl[CELLS];
    float drmean = 0.f;
    if (s > 0) {
      const float dr = g_reward[(size_t)(s - 1) * B + b];
      float g1w[kRewardHidden], g1b[kRewardHidden], g2w[kRewardHidden];
      drmean = heads_reward_grad(dr, rm, W.fc1_w, W.fc1_b, W.fc2_w, g1w, g1b, g2w);
      for (int j = 0; j < kRewardHidden; ++j) {
        D.fc1_w[j] += g1w[j];
        D.fc1_b[j] += g1b[j];
        D.fc2_w[j] += g2w[j];
      }
      *D.fc2_b += dr;
      *D.rew_b += drmean;
    }
    float sp = 0.f;
    for (int p = 0; p < CELLS; ++p) sp += gl[p];
    *D.pol_b += sp;
    for (int c = 0; c < C; ++c) {
      float dot = 0.f, xs = 0.f;
      for (int p = 0; p < CELLS; ++p) {
        const float xv = x[(size_t)c * CELLS + p];
        dot += gl[p] * xv;
        xs += xv;
        g_latent[(sb * C + c) * CELLS + p] =
            heads_latent_grad(W.pol_w[c], gl[p], W.val_w[c], dvmean, W.rew_w[c], drmean, cells);
      }
      D.pol_w[c] += dot;
      D.val_w[c] += (dvmean / cells) * xs;
      if (rew) D.rew_w[c] += (drmean / cells) * xs;
    }
  }
  return MZGO_OK;
}

}  // extern "C"
