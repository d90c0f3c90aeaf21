// mzgo_weights.hpp -- the layout of an engine's packed weight blob (reference
// network, tower = 0) and the device packers of mzgo_weights.hip.
//
// The blob is a list of parts, each padded with zeros to a multiple of 64
// floats.  weight_layout() is the one place that says which parts exist, in
// which order and how long they are: the host path (mzgo_engine::sync_weights,
// mzgo_capi.hip) places what pack_conv / pack_wino / action_taps return at
// these offsets, and pack_weights_device() writes the same floats there from
// the state_dict tensors in device memory.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

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

// MFMA cout-tile grouping of a direct / ring conv (pack_conv, mzgo_conv.hpp)
struct ConvPackGeo {
  int CQ, KS, MG, MGP, NCOG;
  size_t floats;
};
inline ConvPackGeo conv_pack_geo(int COUT, int CIN) {
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
// floats of a Winograd-packed conv (pack_wino, mzgo_wino.hpp)
inline size_t wino_pack_floats(int COUT, int CIN) { return (size_t)(COUT / 16) * 2 * (10 * (CIN / 16)) * 64 * 4; }

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

// Every part of the blob `blob` (layout L; its padding already zero) from the 22
// state_dict tensors src[WK_*] (device float32, contiguous, specs() shapes):
// one launch on `s`, no host copy, no synchronisation.  Bit-identical to the
// host packers of mzgo_capi.hip (f64 sums in their order, rounded once).
hipError_t pack_weights_device(const WeightLayout& L, const float* const* src, float* blob, hipStream_t s);

}  // namespace mzgo
