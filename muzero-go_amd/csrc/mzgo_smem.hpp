// mzgo_smem.hpp -- what every engine kernel holds: the network parameters,
// the workgroup's LDS (Smem), the latent convs over it and a game's node pool.
#pragma once
#include "mzgo_board.hpp"
#include "mzgo_conv.hpp"
#include "mzgo_expand.hpp"
#include "mzgo_move.hpp"
#include "mzgo_search.hpp"
#include "mzgo_wino.hpp"

namespace mzgo {

// Network parameters on the device (packed by mzgo_capi.cpp).
struct NetParams {
  const float* w_conv1; const float* b_conv1;   // representation.conv1 (6 -> 64)
  const float* w_conv2; const float* b_conv2;   // representation.conv2 (64 -> 64)
  const float* w_conv3; const float* b_conv3;   // representation.conv3 (64 -> C)
  const float* w_dyn;   const float* b_dyn;     // dynamics.conv (C -> C)
  const float* emb;                             // dynamics.action_embedding [A][C]
  const float* head_w;                          // [3][C]: reward_conv, value_conv, policy_conv
  const float* etab;                            // [A][9][C] action-tap table (mzgo_expand.hpp)
  HeadScalars hs;
};

// b ? x : y, field by field (kernel-argument pointers stay known-global, so
// their loads are global loads, not flat ones)
__device__ __forceinline__ NetParams select_params(bool b, const NetParams& x, const NetParams& y) {
  NetParams n;
#define MZGO_SEL(f) n.f = b ? x.f : y.f;
  MZGO_SEL(w_conv1) MZGO_SEL(b_conv1) MZGO_SEL(w_conv2) MZGO_SEL(b_conv2) MZGO_SEL(w_conv3) MZGO_SEL(b_conv3)
  MZGO_SEL(w_dyn) MZGO_SEL(b_dyn) MZGO_SEL(emb) MZGO_SEL(head_w) MZGO_SEL(etab)
  MZGO_SEL(hs.reward_b) MZGO_SEL(hs.fc1_w) MZGO_SEL(hs.fc1_b) MZGO_SEL(hs.fc2_w) MZGO_SEL(hs.fc2_b)
  MZGO_SEL(hs.value_b) MZGO_SEL(hs.vfc_w) MZGO_SEL(hs.vfc_b) MZGO_SEL(hs.policy_b) MZGO_SEL(hs.pass_logit)
#undef MZGO_SEL
  return n;
}

// A kernel-argument pointer made opaque to the optimizer at this point of the
// program (an empty asm on its SGPR pair) and re-marked global: address
// arithmetic derived from it cannot be hoisted above the point.  The
// whole-game k_selfplay_move launders its arguments at the head of every move,
// so per-lane addresses are formed per move instead of once at the kernel
// entry and kept (spilled) across the whole game.
template <class T>
__device__ __forceinline__ T* launder_global(T* p) {
  unsigned long long x = reinterpret_cast<unsigned long long>(p);
  asm volatile("" : "+s"(x));
  return (T*)reinterpret_cast<__attribute__((address_space(1))) T*>(x);
}
// The search's f64 parameters made opaque per move as well: the constants
// derived from them (the Gamma sampler's d and 1 / sqrt(9 d), f32 1 - eps)
// are then formed per move instead of being hoisted to the kernel entry and
// kept (spilled, k_selfplay_move<19,96>) across the whole game
__device__ __forceinline__ double launder_f64(double v) {
  unsigned long long x = (unsigned long long)__double_as_longlong(v);
  asm volatile("" : "+s"(x));
  return __longlong_as_double((long long)x);
}
__device__ __forceinline__ SearchParams launder_search(const SearchParams& p) {
  SearchParams r = p;
  r.c_puct = launder_f64(p.c_puct);
  r.discount = launder_f64(p.discount);
  r.dirichlet_alpha = launder_f64(p.dirichlet_alpha);
  r.dirichlet_epsilon = launder_f64(p.dirichlet_epsilon);
  r.pass_epsilon = launder_f64(p.pass_epsilon);
  return r;
}
__device__ __forceinline__ NetParams launder_params(const NetParams& n) {
  NetParams r;
#define MZGO_L(f) r.f = launder_global(n.f);
  MZGO_L(w_conv1) MZGO_L(b_conv1) MZGO_L(w_conv2) MZGO_L(b_conv2) MZGO_L(w_conv3) MZGO_L(b_conv3)
  MZGO_L(w_dyn) MZGO_L(b_dyn) MZGO_L(emb) MZGO_L(head_w) MZGO_L(etab)
  MZGO_L(hs.reward_b) MZGO_L(hs.fc1_w) MZGO_L(hs.fc1_b) MZGO_L(hs.fc2_w) MZGO_L(hs.fc2_b)
  MZGO_L(hs.value_b) MZGO_L(hs.vfc_w) MZGO_L(hs.vfc_b) MZGO_L(hs.policy_b) MZGO_L(hs.pass_logit)
#undef MZGO_L
  return r;
}

__device__ __forceinline__ EngineArrays launder_arrays(const EngineArrays& e) {
  EngineArrays r = e;
#define MZGO_L(f) r.f = launder_global(e.f);
  MZGO_L(pool) MZGO_L(prior) MZGO_L(child) MZGO_L(visits) MZGO_L(wsum) MZGO_L(root_prior) MZGO_L(path)
  MZGO_L(nodes) MZGO_L(nact) MZGO_L(stones) MZGO_L(invd) MZGO_L(meta) MZGO_L(rec_stones) MZGO_L(rec_invd)
  MZGO_L(rec_flags) MZGO_L(rec_action) MZGO_L(rec_value) MZGO_L(rec_policy) MZGO_L(rec_reward) MZGO_L(game_len)
  MZGO_L(final_reward) MZGO_L(status) MZGO_L(jobs) MZGO_L(mpq) MZGO_L(counters) MZGO_L(stamps)
#undef MZGO_L
  return r;
}

template <class G>
struct TreeViewOf {
  __device__ __forceinline__ static TreeView make(const EngineArrays& E, int g) {
    const size_t n1 = (size_t)E.S + 1;
    TreeView T;
    T.prior = E.prior + (size_t)g * n1 * G::A;
    T.child = E.child + (size_t)g * n1 * G::A;
    T.visits = E.visits + (size_t)g * n1;
    T.wsum = E.wsum + (size_t)g * n1;
    T.root_prior = E.root_prior + (size_t)g * G::A;
    T.path = E.path + (size_t)g * (n1 + 1);
    return T;
  }
};

// LDS of one game's workgroup: direct-conv boards (weight DMA rings) ...
template <class G, bool W = G::WINO>
struct Smem {
  union alignas(16) {
    float in[G::CINMAX * G::CPAD];                       // conv staging
    float hp[2 * 3 * G::CS];                             // head partials (after the conv loop)
    struct { int label[G::CELLS], libs[G::CELLS], gsize[G::CELLS]; } scr;  // board step
    ExpandLds<G, G::CINMAX * G::CPAD> f;   // factored expansion
  } u;
  alignas(16) float ring[RingBytes<G>::value / 4];       // weight DMA ring
  TreeLds<G> t;
  int8_t stone[G::CELLS];
  uint8_t invd[G::CELLS];
  int killed[4];
  int misc[8];
  int bc[8];                                             // broadcast slots
  // a batching configuration's buffers were sized to the union's budget
  // a batching configuration's buffers were sized to the union's budget (a
  // non-batching one may grow the union: the kernels assert the whole Smem
  // fits one CU's LDS)
  static_assert(!ExpandLds<G, G::CINMAX * G::CPAD>::BATCH ||
                    sizeof(ExpandLds<G, G::CINMAX * G::CPAD>) <= sizeof(float) * G::CINMAX * G::CPAD,
                "the batched expansion's LDS must fit the conv staging it overlays");
  __device__ float* heads() { return u.hp; }
  __device__ float* ulds() { return u.in; }             // the union as scratch
  static constexpr bool GLOBAL_Y = ExpandLds<G, G::CINMAX * G::CPAD>::GLOBAL_Y;
  static constexpr int HEAD_PARTS = ConvShape<G::C>::NCOG;
};

// ... and Winograd boards (transformed input; exchange buffer + head partials)
template <class G>
struct Smem<G, true> {
  union alignas(16) {
    float in[8 * G::CPAD];                               // conv1 input (6 planes + 2 zero)
    float v[Wino<G>::template v_floats<G::CINMAX>()];    // transformed conv input
    struct {
      float red[Wino<G>::template red_floats<G::C>()];
      float hp[(G::C / 16) * 3 * Wino<G>::HS];   // head partials of one strip
      alignas(16) float outs[G::C * Wino<G>::OUT_STRIDE];   // conv output staging
    } x;
    struct { int label[G::CELLS], libs[G::CELLS], gsize[G::CELLS]; } scr;  // board step
    ExpandLds<G, Wino<G>::template v_floats<G::CINMAX>()> f;
  } u;
  alignas(16) float raw[WinoRaw<G>::FLOATS];              // per-wave staging of conv input rows
  static constexpr bool STRIPS = Wino<G>::NSTRIP > 1;
  alignas(16) float hfin[STRIPS ? 3 * G::CS : 4];         // strip boards: summed head partials
  TreeLds<G> t;
  int8_t stone[G::CELLS];
  uint8_t invd[G::CELLS];
  int killed[4];
  int misc[8];
  int bc[8];
  static_assert(!ExpandLds<G, Wino<G>::template v_floats<G::CINMAX>()>::BATCH ||
                    sizeof(ExpandLds<G, Wino<G>::template v_floats<G::CINMAX>()>) <=
                        sizeof(float) * Wino<G>::template v_floats<G::CINMAX>(),
                "the batched expansion's LDS must fit the Winograd input it overlays");
  __device__ float* heads() { return STRIPS ? hfin : u.x.hp; }
  __device__ float* ulds() { return u.v; }              // the union as scratch
  static constexpr bool GLOBAL_Y = ExpandLds<G, Wino<G>::template v_floats<G::CINMAX>()>::GLOBAL_Y;
  static constexpr int HEAD_PARTS = STRIPS ? 1 : G::C / 16;
};

// One latent conv: src ([CIN][src_stride], global) (+ emb per channel) ->
// dst ([COUT][dst_stride], cells < out_cells), NH fused 1x1 head partials left
// in sm.heads().  All threads; returns synchronised.
// Factored Y of a conv (YM) written to LDS too, as the expansion's copy L.yc
// (CACHE boards, one strip): yc overlays only the exchange buffer, which is
// dead when the epilogue stores (wino_conv's YM store loop reads outs).
template <class G>
__device__ __forceinline__ float* y_lds_target(Smem<G>& sm) {
  if constexpr (G::WINO && decltype(sm.u.f)::CACHE && Wino<G>::NSTRIP == 1) {
    static_assert(sizeof(sm.u.f.yc) <= sizeof(sm.u.x.red), "the LDS Y copy overlays only the exchange buffer");
    return sm.u.f.yc;
  } else {
    return nullptr;
  }
}
// the head weights of the expansion (the rest of load_y, after a conv that
// left Y in L.yc)
template <class G>
__device__ __forceinline__ void load_hw(Smem<G>& sm, const float* head_w) {
  for (int i = tid_local(); i < 3 * G::C; i += G::THREADS) sm.u.f.hw[i] = head_w[i];
}

template <class G, int CIN, int COUT, int NH, bool YM = false>
__device__ __forceinline__ void latent_conv(Smem<G>& sm, const float* __restrict__ w, const float* __restrict__ b,
                                            const float* src, int src_stride, const float* emb, float* dst,
                                            int dst_stride, int out_cells, const float* head_w,
                                            Stamp* st = nullptr, float* ylds = nullptr) {
  if constexpr (G::WINO) {
    // row strips (19x19): strip s reads rows s*SROWS-1 .. (s+1)*SROWS of src,
    // so src must not alias dst (representation ping-pongs through scratch)
    for (int s = 0; s < Wino<G>::NSTRIP; ++s) {
      wino_input<G, CIN>(sm.u.v, sm.raw, src, src_stride, emb, s, st);
      if (st) st->lap(1);
      wino_conv<G, CIN, COUT, NH, YM>(sm.u.v, sm.u.x.red, sm.u.x.hp, sm.u.x.outs, sm.hfin, w, b, dst, dst_stride,
                                  out_cells, head_w, s, st, ylds);
    }
    if constexpr (Wino<G>::NSTRIP > 1) __syncthreads();   // hfin complete
  } else {
    stage_board<G>(sm.u.in, src, src_stride, CIN, emb);
    __syncthreads();
    if (st) st->lap(1);
    conv3x3_ring<G, CIN, COUT, NH, YM>(sm.u.in, sm.ring, w, b, dst, dst_stride, out_cells, head_w, sm.u.hp, st);
  }
}

// The dynamics conv of a node whose latent is rebuilt from its parent's Y
// and E[a] (Winograd boards): latent_conv with wino_input_rebuilt as the
// input transform -- no materialized copy of the latent.  All threads;
// returns synchronised (strip boards) / with the stores issued (one strip).
// pre / mid (one-strip boards only; wino_conv_rebuilt): the caller's work at
// the conv's head, while the parent's Y is still in LDS, and under the GEMM's
// second K half.
template <class G, class Pre = WinoNoMid, class Mid = WinoNoMid>
__device__ __forceinline__ void latent_conv_rebuilt(Smem<G>& sm, const NetParams& np, const float* ypar,
                                                    const float* ea, float* dst, Stamp* st = nullptr,
                                                    float* ylds = nullptr, bool par_in_lds = false,
                                                    Pre pre = Pre{}, Mid mid = Mid{}) {
  if constexpr (G::WINO && Wino<G>::NSTRIP == 1) {
    // (the second channel slab transformed under the GEMM's first K half)
    wino_conv_rebuilt<G>(sm.u.v, sm.raw, sm.u.x.red, sm.u.x.hp, sm.u.x.outs, sm.hfin, ypar, ea, np.w_dyn, np.b_dyn,
                         dst, st, ylds, par_in_lds ? ylds : nullptr, 0, 0, G::C / 16, pre, mid);
  } else if constexpr (G::WINO) {
    for (int s = 0; s < Wino<G>::NSTRIP; ++s)
      wino_conv_rebuilt<G>(sm.u.v, sm.raw, sm.u.x.red, sm.u.x.hp, sm.u.x.outs, sm.hfin, ypar, ea, np.w_dyn,
                           np.b_dyn, dst, st, ylds, par_in_lds ? ylds : nullptr, s);
    if constexpr (Wino<G>::NSTRIP > 1) __syncthreads();
  }
}

template <class G>
__device__ __forceinline__ BoardLds<G> board_lds(Smem<G>& sm) {
  return make_board_lds<G>(sm.stone, sm.invd, sm.u.scr.label, sm.u.scr.libs, sm.u.scr.gsize, sm.killed, sm.misc);
}

// Game g's node slots: S+1 nodes + one scratch latent (slot S+1).
template <class G>
__device__ __forceinline__ float* pool_of(const EngineArrays& E, int g) {
  return E.pool + (size_t)g * ((size_t)E.S + 2) * G::C * G::CS;
}

// Node n's Y (global, [CELLS][C]) and the head weights into the LDS copies
// (GLOBAL_Y boards: the head weights and expand_wave's region-offset table
// only).  All threads; the caller synchronises.
template <class G>
__device__ __forceinline__ void load_y(Smem<G>& sm, const float* y, const float* head_w) {
  auto& L = sm.u.f;
  typedef decltype(sm.u.f) XL;
  if constexpr (XL::CACHE) {
    const f32x4* src = reinterpret_cast<const f32x4*>(y);
    f32x4* dst = reinterpret_cast<f32x4*>(L.yc);
    for (int i = tid_local(); i < G::CELLS * G::C / 4; i += G::THREADS) dst[i] = src[i];
  }
  if constexpr (XL::CACHE || XL::BATCH)
    for (int i = tid_local(); i < 3 * G::C; i += G::THREADS) L.hw[i] = head_w[i];
  if constexpr (XL::GLOBAL_Y)
    for (int i = tid_local(); i < XL::RPAIRS; i += G::THREADS) L.rpair[i] = ExpandPlan<G>::pair_entry(i >> 3, i & 7);
}

}  // namespace mzgo
