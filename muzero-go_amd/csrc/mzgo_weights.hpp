// mzgo_weights.hpp -- an engine's packed weight blob (reference network,
// tower = 0): its layout, the rules that say which float stands at each packed
// index, and the plan that lists the blob's pack jobs.
//
// The blob is a list of parts, each padded with zeros to a multiple of 64
// floats.  weight_layout() is the one place that says which parts exist, in
// which order and how long they are; pack_plan() is the one place that says
// which state_dict tensor feeds which part and how.  The element rules
// (conv_frag / conv_value, wino_frag / wino_value, taps_column) are
// __host__ __device__ text: k_pack_weights (mzgo_weights.hip) runs them one
// thread per element, pack_weights_host() walks the same plan through the same
// rules serially, so the two paths cannot disagree in a bit.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "mzgo_wino.hpp"

namespace mzgo {

// The 22 reference state_dict tensors, in the order of specs() (mzgo_capi.hip)
enum WeightKey {
  WK_CONV1_W, WK_CONV1_B, WK_CONV2_W, WK_CONV2_B, WK_CONV3_W, WK_CONV3_B,
  WK_EMB, WK_DYN_W, WK_DYN_B,
  WK_REWARD_W, WK_REWARD_B, WK_FC1_W, WK_FC1_B, WK_FC2_W, WK_FC2_B,
  WK_PASS_LOGIT, WK_VALUE_W, WK_VALUE_B, WK_VFC_W, WK_VFC_B, WK_POLICY_W, WK_POLICY_B,
  WK_COUNT
};

// Their state_dict keys and shapes (latent_dim C, A embedding rows): the one
// table behind specs() (mzgo_capi.hip) and the unroll's parameter tables
// (mzgo_unroll.hip)
constexpr const char* kWeightKeyNames[] = {
    "representation.conv1.weight", "representation.conv1.bias", "representation.conv2.weight",
    "representation.conv2.bias", "representation.conv3.weight", "representation.conv3.bias",
    "dynamics.action_embedding.weight", "dynamics.conv.weight", "dynamics.conv.bias",
    "dynamics.reward_conv.weight", "dynamics.reward_conv.bias", "dynamics.fc_reward_hidden.weight",
    "dynamics.fc_reward_hidden.bias", "dynamics.fc_reward_output.weight", "dynamics.fc_reward_output.bias",
    "prediction.pass_logit", "prediction.value_conv.weight", "prediction.value_conv.bias",
    "prediction.value_fc.weight", "prediction.value_fc.bias", "prediction.policy_conv.weight",
    "prediction.policy_conv.bias"};
static_assert(sizeof(kWeightKeyNames) / sizeof(kWeightKeyNames[0]) == WK_COUNT, "a name per WeightKey");

struct WeightShape {
  int nd;
  long long d[4];
};
inline WeightShape weight_key_shape(int k, long long C, long long A) {
  switch (k) {
    case WK_CONV1_W: return {4, {64, 6, 3, 3}};
    case WK_CONV2_W: return {4, {64, 64, 3, 3}};
    case WK_CONV3_W: return {4, {C, 64, 3, 3}};
    case WK_CONV1_B: case WK_CONV2_B: return {1, {64}};
    case WK_CONV3_B: case WK_DYN_B: return {1, {C}};
    case WK_EMB: return {2, {A, C}};
    case WK_DYN_W: return {4, {C, C, 3, 3}};
    case WK_REWARD_W: case WK_VALUE_W: case WK_POLICY_W: return {4, {1, C, 1, 1}};
    case WK_FC1_W: return {2, {16, 1}};
    case WK_FC1_B: return {1, {16}};
    case WK_FC2_W: return {2, {1, 16}};
    case WK_VFC_W: return {2, {1, 1}};
    default: return {1, {1}};   // the scalar biases and pass_logit
  }
}

// The blob's parts, in blob order
enum WeightPart {
  WP_CONV1_W, WP_CONV1_B, WP_CONV2_W, WP_CONV2_B, WP_CONV3_W, WP_CONV3_B, WP_DYN_W, WP_DYN_B,
  WP_EMB, WP_HEAD_W, WP_ETAB,
  WP_REWARD_B, WP_FC1_W, WP_FC1_B, WP_FC2_W, WP_FC2_B, WP_VALUE_B, WP_VFC_W, WP_VFC_B, WP_POLICY_B,
  WP_PASS_LOGIT,
  WP_COUNT
};

// the state_dict tensor behind each scalar part WP_REWARD_B .. WP_PASS_LOGIT
constexpr WeightKey kScalarKeys[10] = {WK_REWARD_B, WK_FC1_W, WK_FC1_B, WK_FC2_W, WK_FC2_B,
                                       WK_VALUE_B, WK_VFC_W, WK_VFC_B, WK_POLICY_B, WK_PASS_LOGIT};
// the three 1x1 head convs concatenated in WP_HEAD_W
constexpr WeightKey kHeadKeys[3] = {WK_REWARD_W, WK_VALUE_W, WK_POLICY_W};

// ---- a direct / ring conv: MFMA A-fragment order of mzgo_conv.hpp ----------
// conv weight W[cout][cin][3][3] -> packed[(frag * 64 + lane) * MGP + mi] =
// W[cout][cin][tap] with cout = (cog*MG + mi)*16 + (lane & 15), cin = c4*4 +
// (lane >> 4); zero in the MG == 3 pad slot (mi == 3) and for the padded input
// channels (conv1's cin 6, 7).  A fragment is one (tap, cin quad c4, cout
// group cog).  Plain order (conv3x3_direct): frag = s * NCOG + cog with k-step
// s = tap * CQ + c4.  cog_major (conv3x3_ring, ksplit = Geo::KSPLIT): frag =
// ((cog * ksplit + half) * 9 + tap) * (CQ / ksplit) + c4 % (CQ / ksplit), one
// contiguous stream per (cout group, k-half) for the per-wave DMA rings.
struct ConvPackGeo {
  int CQ, KS, MG, MGP, NCOG;
  size_t floats;
};
__host__ __device__ __forceinline__ ConvPackGeo conv_pack_geo(int COUT, int CIN) {
  ConvPackGeo g;
  const int CINP = (CIN + 3) / 4 * 4, MT = COUT / 16;
  g.CQ = CINP / 4;
  g.KS = 9 * g.CQ;
  g.MG = (MT % 3 == 0) ? 3 : ((MT % 4 == 0 && MT >= 8) ? 4 : 2);
  g.MGP = g.MG == 3 ? 4 : g.MG;
  g.NCOG = MT / g.MG;
  g.floats = (size_t)g.KS * g.NCOG * 64 * g.MGP;
  return g;
}
struct ConvFrag {
  int t, c4, cog;   // tap, cin quad, cout group
};
__host__ __device__ __forceinline__ ConvFrag conv_frag(const ConvPackGeo& g, int cog_major, int ksplit, int frag) {
  ConvFrag f;
  if (cog_major) {
    const int CQH = g.CQ / ksplit;
    const int c4h = frag % CQH, half = (frag / (CQH * 9)) % ksplit;
    f.t = (frag / CQH) % 9;
    f.cog = frag / (CQH * 9 * ksplit);
    f.c4 = half * CQH + c4h;
  } else {
    const int s = frag / g.NCOG;
    f.cog = frag % g.NCOG;
    f.t = s / g.CQ;
    f.c4 = s % g.CQ;
  }
  return f;
}
__host__ __device__ __forceinline__ float conv_value(const float* W, int CIN, const ConvPackGeo& g, const ConvFrag& f,
                                                     int lane, int mi) {
  if (mi >= g.MG) return 0.f;
  const int cout = (f.cog * g.MG + mi) * 16 + (lane & 15);
  const int cin = f.c4 * 4 + (lane >> 4);
  return cin < CIN ? W[((size_t)cout * CIN + cin) * 9 + f.t] : 0.f;
}

// ---- a Winograd conv: the U stream of mzgo_wino.hpp ------------------------
// U_xi[cout][cin] = (G2 g G3^T)[i][j], g = W[cout][cin], xi = i*5 + j, with
// G2 of F(2,3) (points 0, 1, -1, inf) on kernel rows and G3 of F(3,3)
// (points 0, 1, -1, -2, inf) on kernel columns, summed in double over a, then
// b, and rounded once.  packed[(((m*2 + h)*L + pos)*64 + lane)*4 + e] =
// U_xi[16m + (lane & 15)][hh*CIN/2 + 4*(4*s4 + e) + (lane >> 4)] for xi =
// h*10 + xl and k-position k = hh*S4 + s4 (S4 = CIN/32, KP = CIN/16, L = 10 KP):
// one contiguous float4 stream per (cout tile m, xi half h) wave.  A fragment
// is one (m, h, pos); pos is wino_conv's consumption order -- K half, xi group
// (kWinoXG), k-position within the half, xi within the group: the GEMM runs
// the first half of CIN for every xi before the second, so the rebuilt input's
// second channel slab is transformed under the first half's MFMAs.
constexpr double kWinoG2[4][3] = {{1, 0, 0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0, 0, 1}};
constexpr double kWinoG3[5][3] = {{0.5, 0, 0},
                                  {1.0 / 6, 1.0 / 6, 1.0 / 6},
                                  {0.5, -0.5, 0.5},
                                  {1.0 / 6, -1.0 / 3, 2.0 / 3},
                                  {0, 0, 1}};
__host__ __device__ __forceinline__ size_t wino_pack_floats(int COUT, int CIN) {
  return (size_t)(COUT / 16) * 2 * (10 * (CIN / 16)) * 64 * 4;
}
struct WinoFrag {
  int i, j, co0, ci0;   // rows of G2 / G3; the fragment's first cout and cin
};
__host__ __device__ __forceinline__ WinoFrag wino_frag(int CIN, int frag) {
  const int CH = CIN / 2, S4 = CH / 16, KP = CIN / 16, L = 10 * KP, KH = KP / 2, NG = 10 / kWinoXG;
  const int pos = frag % L, h = (frag / L) % 2, m = frag / (2 * L);
  // pos = ((kh * NG + xl / XG) * KH + k % KH) * XG + xl % XG
  const int xr = pos % kWinoXG, kk = (pos / kWinoXG) % KH, xg = (pos / (kWinoXG * KH)) % NG;
  const int kh = pos / (kWinoXG * KH * NG);
  const int k = kh * KH + kk, xi = h * 10 + xg * kWinoXG + xr;
  return WinoFrag{xi / 5, xi % 5, 16 * m, (k / S4) * CH + 16 * (k % S4)};
}
__host__ __device__ __forceinline__ float wino_value(const float* W, int CIN, const WinoFrag& f, int lane, int e) {
  const int co = f.co0 + (lane & 15), ci = f.ci0 + 4 * e + (lane >> 4);
  const float* g = W + ((size_t)co * CIN + ci) * 9;
  double u = 0.0;
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) u += kWinoG2[f.i][a] * (double)g[a * 3 + b] * kWinoG3[f.j][b];
  return (float)u;
}

// ---- the action-tap table of the factored expansion (mzgo_expand.hpp) ------
// E[a][r][co] = sum over the taps (ky, kx) on the board for a cell of region
// r = ry*3 + rx (ry, rx in {first, interior, last} row / column) of
// sum_ci W[co][ci][ky][kx] * emb[a][ci], so that conv3x3(x + emb[a]) =
// conv3x3(x) + E[a][region] under zero padding.  One column (a, co): the nine
// tap sums over ascending ci in nine f64 accumulators, then the nine region
// sums in ky, kx order, each rounded once.
__host__ __device__ __forceinline__ void taps_column(const float* W, const float* emb, int C, int a, int co,
                                                     float* etab) {
  const float* w = W + (size_t)co * C * 9;
  const float* e = emb + (size_t)a * C;
  double u[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) u[t] = 0.0;
  for (int ci = 0; ci < C; ++ci) {
    const double ev = (double)e[ci];
#pragma unroll
    for (int t = 0; t < 9; ++t) u[t] += (double)w[ci * 9 + t] * ev;
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
    etab[((size_t)a * 9 + r) * C + co] = (float)s;
  }
}
// the whole table etab[A][9][C] on the host
inline void action_taps(const float* W, const float* emb, int C, int A, float* etab) {
  for (int a = 0; a < A; ++a)
    for (int co = 0; co < C; ++co) taps_column(W, emb, C, a, co, etab);
}

// ---- the layout ------------------------------------------------------------
struct WeightLayout {
  int N = 0, C = 0, A = 0;
  bool wino = false;           // the three latent convs in Winograd form (Geo::WINO)
  int ksplit = 1;              // k-range split of the ring conv (Geo::KSPLIT)
  size_t size[WP_COUNT] = {};  // floats of each part (unpadded)
  size_t off[WP_COUNT] = {};   // its offset in the blob, in floats
  size_t total = 0;            // floats of the blob
};

inline WeightLayout weight_layout(int N, int C, int A) {
  WeightLayout L;
  L.N = N; L.C = C; L.A = A;
  // k-range split of the ring conv: 2 when the board runs 8 waves (Geo::KSPLIT)
  const int ct = (N * N + 15) / 16, ng = ct >= 3 ? 3 : ct, ncg = (ct + ng - 1) / ng;
  L.ksplit = ncg <= 2 ? 2 : 1;
  L.wino = N == 9 || N == 19;
  auto latent = [&](int cout, int cin) { return L.wino ? wino_pack_floats(cout, cin) : conv_pack_geo(cout, cin).floats; };
  L.size[WP_CONV1_W] = conv_pack_geo(64, 6).floats; L.size[WP_CONV1_B] = 64;
  L.size[WP_CONV2_W] = latent(64, 64);              L.size[WP_CONV2_B] = 64;
  L.size[WP_CONV3_W] = latent(C, 64);               L.size[WP_CONV3_B] = (size_t)C;
  L.size[WP_DYN_W] = latent(C, C);                  L.size[WP_DYN_B] = (size_t)C;
  L.size[WP_EMB] = (size_t)A * C;
  L.size[WP_HEAD_W] = (size_t)3 * C;
  L.size[WP_ETAB] = (size_t)A * 9 * C;
  for (int p = WP_REWARD_B; p < WP_COUNT; ++p) L.size[p] = 1;
  L.size[WP_FC1_W] = L.size[WP_FC1_B] = L.size[WP_FC2_W] = 16;
  for (int p = 0; p < WP_COUNT; ++p) { L.off[p] = L.total; L.total += (L.size[p] + 63) / 64 * 64; }
  return L;
}

// ---- the plan: which tensor feeds which part, and by which rule -------------
enum PackKind { PK_TAPS, PK_CONV, PK_WINO, PK_COPY };
struct PackStep {
  int kind;
  int key, key2;       // the source tensors (WeightKey); key2: PK_TAPS' embedding
  size_t off, count;   // the destination's offset in the blob; its work items: floats (PK_TAPS: columns of 9)
  int COUT, CIN;       // PK_CONV / PK_WINO; PK_TAPS: C, A
  int cog_major, ksplit;
};
constexpr int kMaxPackSteps = 24;   // the tap table, 4 convs, 18 copies = 23
struct PackPlan {
  PackStep step[kMaxPackSteps];
  int n = 0;
};
inline PackPlan pack_plan(const WeightLayout& L) {
  PackPlan P;
  auto add = [&](int kind, int key, int key2, size_t off, size_t count, int cout, int cin, int cog_major, int ksplit) {
    P.step[P.n++] = PackStep{kind, key, key2, off, count, cout, cin, cog_major, ksplit};
  };
  auto conv = [&](int kind, WeightKey k, WeightPart p, int cout, int cin, int cog_major, int ksplit) {
    add(kind, k, k, L.off[p], L.size[p], cout, cin, cog_major, ksplit);
  };
  auto copy = [&](WeightKey k, size_t off, size_t n) { add(PK_COPY, k, k, off, n, 0, 0, 0, 1); };
  const int C = L.C, A = L.A;
  // the tap table first: on the device its threads run longest
  add(PK_TAPS, WK_DYN_W, WK_EMB, L.off[WP_ETAB], (size_t)A * C, C, A, 0, 1);
  conv(PK_CONV, WK_CONV1_W, WP_CONV1_W, 64, 6, 0, 1);
  const int lk = L.wino ? PK_WINO : PK_CONV;
  conv(lk, WK_CONV2_W, WP_CONV2_W, 64, 64, 1, L.ksplit);
  conv(lk, WK_CONV3_W, WP_CONV3_W, C, 64, 1, L.ksplit);
  conv(lk, WK_DYN_W, WP_DYN_W, C, C, 1, L.ksplit);
  copy(WK_CONV1_B, L.off[WP_CONV1_B], L.size[WP_CONV1_B]);
  copy(WK_CONV2_B, L.off[WP_CONV2_B], L.size[WP_CONV2_B]);
  copy(WK_CONV3_B, L.off[WP_CONV3_B], L.size[WP_CONV3_B]);
  copy(WK_DYN_B, L.off[WP_DYN_B], L.size[WP_DYN_B]);
  copy(WK_EMB, L.off[WP_EMB], L.size[WP_EMB]);               // the first A rows
  for (int h = 0; h < 3; ++h) copy(kHeadKeys[h], L.off[WP_HEAD_W] + (size_t)h * C, (size_t)C);
  for (int i = 0; i < 10; ++i) copy(kScalarKeys[i], L.off[WP_REWARD_B + i], L.size[WP_REWARD_B + i]);
  static_assert(5 + 4 + 1 + 3 + 10 <= kMaxPackSteps, "plan too small");
  return P;
}

// The plan's two walks (mzgo_weights.hip).  `blob` has layout L and its padding
// is already zero; src[WK_*] are the 22 state_dict tensors (float32,
// contiguous, specs() shapes).  On the device: one launch on `s`, no host copy,
// no synchronisation.  On the host: serially, the same floats bit for bit (the
// library is built with -ffp-contract=off).
hipError_t pack_weights_device(const WeightLayout& L, const float* const* src, float* blob, hipStream_t s);
void pack_weights_host(const WeightLayout& L, const float* const* src, float* blob);

// keys / data / shapes / ndims (n entries) -> src[WK_*]: every key once, with
// its shape for latent_dim C and A embedding rows.  The checks of
// mzgo_set_weights_device and mzgo_weights_pack_host (`fn` names the caller).
int weight_table(const char* fn, const char* const* keys, const float* const* data, const int64_t* const* shapes,
                 const int* ndims, int n, int C, int A, const float** src);

// (mzgo_capi.hip's, for the units that do not see it)
int set_error(int code, const char* fmt, ...);
struct KernelSet;
const KernelSet* find_kernels(int N, int C);

}  // namespace mzgo
