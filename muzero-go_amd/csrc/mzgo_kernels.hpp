// mzgo_kernels.hpp -- the engine's kernels, templated on board size N and
// latent_dim C and instantiated per (N, C) in mzgo_kernels_N*.hip.
//
// Every kernel runs one workgroup (4 waves) per game / batch element; games
// never talk to each other, so the only inter-workgroup synchronisation is a
// game's with its helper workgroups: the job protocol, mzgo_jobs.hpp (which
// brings in Smem and the conv wrappers, mzgo_smem.hpp).
#pragma once
#include "mzgo_jobs.hpp"
#include "mzgo_replay.hpp"

namespace mzgo {

// ---------------------------------------------------------------------------
// representation (self_play.py:70-74) + prediction heads (:104-113).
// planes(c, cell) gives the f32 observation.  The latent is written to
// ``lat`` ([C][lat_stride]), which also serves as scratch for conv1/conv2;
// strip boards put conv2's output in ``scr`` ([64][lat_stride]) instead (a
// strip conv cannot run in place).
// Leaves the logits in sm.t.logits and the value in sm.t.value.
// ---------------------------------------------------------------------------
template <class G>
constexpr bool rep_needs_scratch() {
  if constexpr (G::WINO) return Wino<G>::NSTRIP > 1;
  else return false;
}

// conv2 / conv3 of the representation as jobs (run_search's RepJobs on
// 19x19 with helper workgroups): jobs(k) runs conv k and returns true, or
// returns false for the workgroup's own latent_conv.
struct NoRepJobs {
  __device__ bool operator()(int) const { return false; }
};

template <class G, class PlaneFn, class Jobs = NoRepJobs>
__device__ __forceinline__ void representation(Smem<G>& sm, const NetParams& np, PlaneFn planes, float* lat,
                                      int lat_stride, float* scr, unsigned long long* ts = nullptr,
                                      Jobs jobs = Jobs{}) {
  float* mid = rep_needs_scratch<G>() ? scr : lat;
  for (int i = tid_local(); i < 6 * G::CELLS; i += G::THREADS) {
    const int c = i / G::CELLS, j = i - c * G::CELLS;
    sm.u.in[c * G::CPAD + j] = planes(c, j);
  }
  zero_channels<G>(sm.u.in, 6, 8);
  stage_head_scalars(np.hs, sm.t.hsc);
  __syncthreads();
  HeadPart<G> hp{nullptr};
  const int oc = lat_stride == G::CS ? G::CS : G::CELLS;   // pooled latents also write their 0 pads
  conv3x3_direct<G, 6, 64, 0, 1>(sm.u.in, np.w_conv1, np.b_conv1, lat, lat_stride, oc, nullptr, hp);
  __syncthreads();
#ifdef MZGO_STAMPS
  if (ts) ts[0] = __builtin_amdgcn_s_memtime();
#endif
  if (!jobs(2))
    latent_conv<G, 64, 64, 0>(sm, np.w_conv2, np.b_conv2, lat, lat_stride, nullptr, mid, lat_stride, oc, nullptr);
  __syncthreads();                                         // conv2's stores before conv3 reads them
#ifdef MZGO_STAMPS
  if (ts) ts[1] = __builtin_amdgcn_s_memtime();
#endif
  if (!jobs(3))
    latent_conv<G, 64, G::C, 2>(sm, np.w_conv3, np.b_conv3, mid, lat_stride, nullptr, lat, lat_stride, oc,
                                np.head_w + G::C);
  if (wave_id() == 0)
    finalize_heads<G, Smem<G>::HEAD_PARTS>(sm.heads(), false, sm.t.hsc, sm.t.logits, &sm.t.reward, &sm.t.value);
  __syncthreads();
}

// dynamics (self_play.py:85-95) + prediction: ``src`` latent + emb[action]
// -> ``dst`` latent; logits/reward/value left in sm.t.
template <class G>
__device__ __forceinline__ void dynamics(Smem<G>& sm, const NetParams& np, const float* src, int src_stride,
                                int action, float* dst, int dst_stride) {
  stage_head_scalars(np.hs, sm.t.hsc);
  latent_conv<G, G::C, G::C, 3>(sm, np.w_dyn, np.b_dyn, src, src_stride, np.emb + (size_t)action * G::C, dst,
                                dst_stride, dst_stride == G::CS ? G::CS : G::CELLS, np.head_w);
  if (wave_id() == 0)
    finalize_heads<G, Smem<G>::HEAD_PARTS>(sm.heads(), true, sm.t.hsc, sm.t.logits, &sm.t.reward, &sm.t.value);
  __syncthreads();
}

// ---------------------------------------------------------------------------
// Batched drop-in inference (self_play.py:121-128)
// ---------------------------------------------------------------------------
template <int N, int C>
__global__ void __launch_bounds__((Geo<N, C>::THREADS)) __attribute__((amdgpu_waves_per_eu(Geo<N, C>::WPE, Geo<N, C>::WPE))) k_initial_inference(NetParams np, const float* __restrict__ obs,
                                                                 float* latent, float* value, float* logits,
                                                                 float* scratch) {
  typedef Geo<N, C> G;
  __shared__ Smem<G> sm;
  static_assert(sizeof(Smem<G>) <= 160 * 1024, "one workgroup per CU: the whole LDS at most");
  if constexpr (G::WINO) wino_raw_zero<G>(sm.raw);        // zero halo of the conv input planes
  const int b = blockIdx.x;
  const float* o = obs + (size_t)b * 6 * G::CELLS;
  float* lat = latent + (size_t)b * G::C * G::CELLS;
  float* scr = scratch ? scratch + (size_t)b * 64 * G::CELLS : nullptr;
  representation<G>(sm, np, [&](int c, int j) { return o[c * G::CELLS + j]; }, lat, G::CELLS, scr);
  for (int a = tid_local(); a < G::A; a += G::THREADS) logits[(size_t)b * G::A + a] = sm.t.logits[a];
  if (tid_local() == 0) value[b] = sm.t.value;
}

template <int N, int C>
__global__ void __launch_bounds__((Geo<N, C>::THREADS)) __attribute__((amdgpu_waves_per_eu(Geo<N, C>::WPE, Geo<N, C>::WPE))) k_recurrent_inference(NetParams np, const float* __restrict__ latent,
                                                                   const int64_t* __restrict__ action,
                                                                   float* next_latent, float* reward,
                                                                   float* value, float* logits, int* err) {
  typedef Geo<N, C> G;
  __shared__ Smem<G> sm;
  static_assert(sizeof(Smem<G>) <= 160 * 1024, "one workgroup per CU: the whole LDS at most");
  if constexpr (G::WINO) wino_raw_zero<G>(sm.raw);        // zero halo of the conv input planes
  const int b = blockIdx.x;
  int64_t a = action[b];
  if (a < 0 || a >= G::A) {            // nn.Embedding would raise IndexError
    if (tid_local() == 0) atomicOr(err, 1);
    a = 0;
  }
  dynamics<G>(sm, np, latent + (size_t)b * G::C * G::CELLS, G::CELLS, (int)a,
              next_latent + (size_t)b * G::C * G::CELLS, G::CELLS);
  for (int i = tid_local(); i < G::A; i += G::THREADS) logits[(size_t)b * G::A + i] = sm.t.logits[i];
  if (tid_local() == 0) { reward[b] = sm.t.reward; value[b] = sm.t.value; }
}

// ---------------------------------------------------------------------------
// One full MCTS.run (self_play.py:148-237) for game slot g.
// ---------------------------------------------------------------------------
// Batch expansion (factored dynamics): children i < B of one parent whose Y
// is in L.yc (and the head weights in L.hw), child i = node nid0 + i via
// action L.acts[i]; one wave per child: E[a] into LDS, heads, the child's
// prior row and child row (LAZY: neither -- the lazy policy head, see
// TreeLds::rawp), L.bv[i] = its backup value r + discount * v.  Each wave claims the next child
// (sm.t.ngrab, reset with sm.t.npick by the caller) and waits until
// sm.t.npick > k (wave 0 publishes the actions, pick_sequence, before it
// joins).  All threads; the caller synchronises.
template <class G, bool LAZY>
__device__ __forceinline__ void batch_expand(Smem<G>& sm, const NetParams& np, const SearchParams& sp,
                                             const TreeView& TV, int B, int nid0, const float* yg,
                                             Stamp* st = nullptr) {
  auto& L = sm.u.f;
  typedef decltype(sm.u.f) XL;
  if (st && tid_local() == 0) { st->wave_add(48, 1); st->wave_add(55, (unsigned long long)B); }   // batches, children
  if constexpr (XL::GLOBAL_Y && !LAZY) {
    // Y streamed from L2 (19x19): a wave claims two children at a time and
    // reads the parent's Y once for both (expand_wave2)
    const int wave = __builtin_amdgcn_readfirstlane(wave_id());
    const int lane = lane_id_local();
    auto& W = L.wv[wave];
    ExpandPlan<G> plan;
    plan.init(L.rpair);
    constexpr int E4N = 9 * G::C / 4;
    f32x4* ew0 = reinterpret_cast<f32x4*>(W.ew);
    f32x4* ew1 = reinterpret_cast<f32x4*>(W.ew2);
    // the child's heads, prior row and child row from its totals and the
    // policy sums in W.xw (as the one-child loop below)
    auto child_rows = [&](int k, float rsum, float vsum) {
      const int nid = nid0 + k;
      float r, v;
      heads_from_totals<G>(rsum, vsum, sm.t.hsc, r, v);
      float x[G::AP];
      policy_logits<G>(W.xw + XL::PROW, sm.t.hsc, x);
      int* crow = TV.child + (size_t)nid * G::A;
      for (int i = lane; i < G::A; i += 64) crow[i] = -1;
      child_priors<G>(sm.t, x, TV.prior + (size_t)nid * G::A, -1, sp.variant, W.fscratch(), W.dscratch());
      if (lane == 0) L.bv[k] = (double)r + sp.discount * (double)v;
    };
    // the lazy policy head (sp.lazy_rows; self-play): the totals only, and
    // the sentinel kLazyRow in child-row entry 0 -- a select that first
    // reaches the node forms its logits and priors (expand_child's LAZYH)
    auto lazy_child = [&](int k, float rsum, float vsum) {
      float r, v;
      heads_from_totals<G>(rsum, vsum, sm.t.hsc, r, v);
      if (lane == 0) {
        TV.child[(size_t)(nid0 + k) * G::A] = kLazyRow;
        L.bv[k] = (double)r + sp.discount * (double)v;
      }
    };
    const bool lazy = sp.lazy_rows != 0;
    for (;;) {
      int k = 0;
      if (lane == 0) k = atomicAdd(&sm.t.ngrab, 2);
      k = __builtin_amdgcn_readfirstlane(k);
      if (k >= B) break;
      const bool two = k + 1 < B;
      const int need = two ? k + 1 : k;
      while (__hip_atomic_load(&sm.t.npick, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) <= need)
        __builtin_amdgcn_s_sleep(2);
      const int a0 = __builtin_amdgcn_readfirstlane(L.acts[k]);
      const f32x4* e0 = reinterpret_cast<const f32x4*>(np.etab + (size_t)a0 * 9 * G::C);
      for (int i = lane; i < E4N; i += 64) ew0[i] = e0[i];
      if (two) {
        const int a1 = __builtin_amdgcn_readfirstlane(L.acts[k + 1]);
        const f32x4* e1 = reinterpret_cast<const f32x4*>(np.etab + (size_t)a1 * 9 * G::C);
        for (int i = lane; i < E4N; i += 64) ew1[i] = e1[i];
      }
      wave_lds_sync();
      if (lazy) {
        if (two) {
          float r0, v0, r1, v1;
          Pol2<G> pol;
          expand_wave2<G, XL::PROW, false>(W.xw, yg, W.ew, W.ew2, L.hw, plan, r0, v0, r1, v1, pol);
          lazy_child(k, r0, v0);
          lazy_child(k + 1, r1, v1);
        } else {
          float rsum, vsum;
          expand_wave<G, XL::PROW, false>(W.xw, yg, W.ew, L.hw, plan, rsum, vsum);
          lazy_child(k, rsum, vsum);
        }
      } else if (two) {
        float r0, v0, r1, v1;
        Pol2<G> pol;
        expand_wave2<G, XL::PROW>(W.xw, yg, W.ew, W.ew2, L.hw, plan, r0, v0, r1, v1, pol);
        wave_lds_sync();
        child_rows(k, r0, v0);
        wave_lds_sync();                     // child k's reads of W.xw / W.ew before child k + 1's
        store_policy2<G, XL::PROW>(W.xw, pol);
        wave_lds_sync();
        child_rows(k + 1, r1, v1);
      } else {
        float rsum, vsum;
        expand_wave<G, XL::PROW, true>(W.xw, yg, W.ew, L.hw, plan, rsum, vsum);
        wave_lds_sync();
        child_rows(k, rsum, vsum);
      }
      if (st) st->wave_add(68, two ? 2 : 1);
      wave_lds_sync();                       // W.ew / W.xw reused by the wave's next pair
    }
  } else if constexpr (XL::BATCH) {
    const int wave = __builtin_amdgcn_readfirstlane(wave_id());
    const int lane = lane_id_local();
    auto& W = L.wv[wave];
    ExpandPlan<G> plan;
    plan.init(L.rpair);
    // E[a] of the wave's next child, loaded into registers while the current
    // child's heads and rows are written (its action is published by then
    // unless the picks are late; the copy then reads E at the top)
    constexpr int E4N = 9 * G::C / 4, EP = (E4N + 63) / 64;
    f32x4 epre[EP];
    int epre_a = -1;
    f32x4* ewl = reinterpret_cast<f32x4*>(W.ew);
    // children are claimed one at a time (wave 0 joins late, after the picks)
    auto grab = [&]() {
      int v = 0;
      if (lane == 0) v = atomicAdd(&sm.t.ngrab, 1);
      return __builtin_amdgcn_readfirstlane(v);
    };
    for (int k = grab(), kn; k < B; k = kn) {
      while (__hip_atomic_load(&sm.t.npick, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) <= k)
        __builtin_amdgcn_s_sleep(2);
      unsigned long long t0 = st ? st->now() : 0, t1;
      const int a = __builtin_amdgcn_readfirstlane(L.acts[k]), nid = nid0 + k;
      if (a == epre_a) {
#pragma unroll
        for (int e = 0; e < EP; ++e)
          if (lane + 64 * e < E4N) ewl[lane + 64 * e] = epre[e];
      } else {
        const f32x4* e4 = reinterpret_cast<const f32x4*>(np.etab + (size_t)a * 9 * G::C);
        for (int i = lane; i < E4N; i += 64) ewl[i] = e4[i];
      }
      wave_lds_sync();
      if (st) { t1 = st->now(); st->wave_add(64, t1 - t0); t0 = t1; }
      float rsum, vsum;
      if constexpr (XL::GLOBAL_Y) expand_wave<G, XL::PROW, !LAZY>(W.xw, yg, W.ew, L.hw, plan, rsum, vsum);
      else expand_wave<G, XL::PROW, !LAZY>(W.xw, L.yc, W.ew, L.hw, plan, rsum, vsum);
      wave_lds_sync();
      epre_a = -1;
      kn = grab();
      {
        if (kn < B && __hip_atomic_load(&sm.t.npick, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) > kn) {
          epre_a = __builtin_amdgcn_readfirstlane(L.acts[kn]);
          const f32x4* e4 = reinterpret_cast<const f32x4*>(np.etab + (size_t)epre_a * 9 * G::C);
#pragma unroll
          for (int e = 0; e < EP; ++e) epre[e] = e4[lane + 64 * e < E4N ? lane + 64 * e : 0];
        }
      }
      if (st) { t1 = st->now(); st->wave_add(65, t1 - t0); t0 = t1; }
      float r, v;
      heads_from_totals<G>(rsum, vsum, sm.t.hsc, r, v);
      if (st) { t1 = st->now(); st->wave_add(66, t1 - t0); t0 = t1; }
      if constexpr (LAZY) {
        // no policy head: a select that first reaches the child forms its
        // logits (select_leaf -> kNeedLogits -> policy_sums_wg); most never do
        if (lane == 0) atomicOr(&sm.t.rawp[nid >> 5], 1u << (nid & 31));
      } else {
        float x[G::AP];
        policy_logits<G>(W.xw + XL::PROW, sm.t.hsc, x);
        int* crow = TV.child + (size_t)nid * G::A;
        for (int i = lane; i < G::A; i += 64) crow[i] = -1;
        child_priors<G>(sm.t, x, TV.prior + (size_t)nid * G::A, -1, sp.variant, W.fscratch(), W.dscratch());
      }
      if (lane == 0) L.bv[k] = (double)r + sp.discount * (double)v;
      wave_lds_sync();                     // W.ew / W.xw reused by the wave's next child
      if (st) { t1 = st->now(); st->wave_add(67, t1 - t0); st->wave_add(68, 1); }
    }
  }
}

// One child of a batch by ONE wave (batch_expand's per-child work): E[a]
// into W.ew, expand_wave over Y, the heads, the child's prior row and child
// row; returns the backup value r + discount * v (every lane).  Lazy policy
// head: LAZY (LDS trees) writes neither row (TreeLds::rawp), LAZYH (HBM
// trees, the shared batches) only the sentinel kLazyRow into child-row entry
// 0; a select that first reaches the node forms its logits and priors (most
// never are).
template <class G, bool LAZY, bool LAZYH = false>
__device__ __forceinline__ double expand_child(Smem<G>& sm, const NetParams& np, const SearchParams& sp,
                                               const TreeView& TV, const float* yg, const ExpandPlan<G>& plan,
                                               int a, int nid, Stamp* st = nullptr) {
  // (st: wave 0's phase cycles in slots 64-66, 68)
  unsigned long long t0 = st ? st->now() : 0, t1;
  auto& L = sm.u.f;
  typedef decltype(sm.u.f) XL;
  const int lane = lane_id_local();
  auto& W = L.wv[__builtin_amdgcn_readfirstlane(wave_id())];
  constexpr int E4N = 9 * G::C / 4;
  f32x4* ewl = reinterpret_cast<f32x4*>(W.ew);
  const f32x4* e4 = reinterpret_cast<const f32x4*>(np.etab + (size_t)a * 9 * G::C);
  for (int i = lane; i < E4N; i += 64) ewl[i] = e4[i];
  wave_lds_sync();
  if (st && wave_id() == 0) { t1 = st->now(); st->wave_add(64, t1 - t0); t0 = t1; }
  float rsum, vsum;
  constexpr bool POL = !LAZY && !LAZYH;
  if constexpr (XL::GLOBAL_Y) expand_wave<G, XL::PROW, POL>(W.xw, yg, W.ew, L.hw, plan, rsum, vsum);
  else expand_wave<G, XL::PROW, POL>(W.xw, L.yc, W.ew, L.hw, plan, rsum, vsum);
  wave_lds_sync();
  if (st && wave_id() == 0) { t1 = st->now(); st->wave_add(65, t1 - t0); t0 = t1; }
  float r, v;
  heads_from_totals<G>(rsum, vsum, sm.t.hsc, r, v);
  if (st && wave_id() == 0) { t1 = st->now(); st->wave_add(66, t1 - t0); t0 = t1; }
  if constexpr (LAZY) {
    if (lane == 0) atomicOr(&sm.t.rawp[nid >> 5], 1u << (nid & 31));
  } else if constexpr (LAZYH) {
    if (lane == 0) TV.child[(size_t)nid * G::A] = kLazyRow;
  } else {
    float x[G::AP];
    policy_logits<G>(W.xw + XL::PROW, sm.t.hsc, x);
    int* crow = TV.child + (size_t)nid * G::A;
    for (int i = lane; i < G::A; i += 64) crow[i] = -1;
    child_priors<G>(sm.t, x, TV.prior + (size_t)nid * G::A, -1, sp.variant, W.fscratch(), W.dscratch());
  }
  wave_lds_sync();                     // W.ew / W.xw reused by the wave's next child
  if (st && wave_id() == 0) { st->wave_add(68, st->now() - t0); }
  return (double)r + sp.discount * (double)v;
}

// The children of job J (batch bseq, B children, node ids nid0 + k, actions
// in L.acts) a round of WAVES at a time, claimed by CAS; each child's backup
// value goes to J.bv (HBM).  Returns this workgroup's count.  All threads.
// (kJobBatch's share; declared with its defaults in mzgo_jobs.hpp)
template <class G, bool LAZY, bool LAZYH>
__device__ __forceinline__ int job_rounds(Smem<G>& sm, const NetParams& np, const SearchParams& sp,
                                          const TreeView& TV, const float* yg, const JobView& J, unsigned bseq,
                                          int B, int nid0, bool helper, Stamp* st) {
  auto& L = sm.u.f;
  const int wave = __builtin_amdgcn_readfirstlane(wave_id());
  ExpandPlan<G> plan;
  plan.init(L.rpair);
  double* bvg = J.bv(G::A);
  int mine = 0;
  for (;;) {
    const int c0 = job_claim(sm, J, bseq, B, G::WAVES);
    if (c0 < 0) break;
    const int k = c0 + wave;
    if (k < B) {
      int a;
      if (helper) {                                  // (a helper may claim before the game's wave 0 picked it)
        unsigned long long t = __hip_atomic_load(J.acts() + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        while ((unsigned)(t >> 32) != bseq) {
          __builtin_amdgcn_s_sleep(2);
          t = __hip_atomic_load(J.acts() + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        a = __builtin_amdgcn_readfirstlane((int)(unsigned)t);
      } else {
        a = __builtin_amdgcn_readfirstlane(L.acts[k]);
      }
      const double bv = expand_child<G, LAZY, LAZYH>(sm, np, sp, TV, yg, plan, a, nid0 + k, st);
      if (lane_id_local() == 0) bvg[k] = bv;
    }
    mine += (B - c0 < G::WAVES ? B - c0 : G::WAVES);
  }
  return mine;
}

// The game's workgroup: batch_expand over the job machinery (B children of
// leaf `leaf` whose Y is yg, actions in L.acts, node ids nid0 + k); L.bv
// gets every child's backup value.
template <class G, bool LAZY, class Wait = NoExtra>
__device__ __forceinline__ void batch_expand_shared(Smem<G>& sm, const NetParams& np, const SearchParams& sp,
                                                    const EngineArrays& E, int g, const TreeView& TV, int B,
                                                    int nid0, int leaf, int net, const float* yg,
                                                    const uint64_t (&m)[G::AP], int n, int i0, uint64_t key,
                                                    int sim0, Stamp* st = nullptr, bool prepicked = false,
                                                    Wait pre_wait = Wait{}) {
  auto& L = sm.u.f;
  const JobView J = job_of<G>(E, g);
  const JobInfo I = job_info(kJobBatch, B, nid0, leaf, net);
  // the job first (geometry, the root's mask, the actions known already:
  // i0 of them), then the picks (pick_all, wave 0; tagged entries: a helper
  // that claims a round before they are out waits for its entry)
  const unsigned bseq = job_post(J, I, 0, [&](unsigned bs) {
    for (int a = tid_local(); a < G::A; a += G::THREADS) J.valid(G::A)[a] = sm.t.valid[a];
    if (tid_local() == 0) {
      J.h->pass_prior = sm.t.pass_prior;
      for (int k = 0; k < i0; ++k)
        __hip_atomic_store(J.acts() + k, (unsigned long long)bs << 32 | (unsigned)L.acts[k], __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
    }
  });
  if (st) st->lap(40);
  // (prepicked: the actions i0.. went out during the parent's conv job,
  // tagged for this batch; the workgroup reads them from the job like a
  // helper and copies them back into L.acts, which the conv overwrote)
  if (!prepicked && wave_id() == 0)
    pick_all<G>(m, n, i0, B - i0, key, sim0, L.acts, st, J.acts(), bseq);
  __syncthreads();                                   // every pick made (in LDS too)
  if (st) st->lap(41);
  const int mine = job_rounds<G, LAZY, !LAZY>(sm, np, sp, TV, yg, J, bseq, B, nid0, prepicked, st);
  if (st) st->lap(42);
  if (prepicked)
    for (int k = tid_local(); k < B; k += G::THREADS)
      L.acts[k] = (int)(unsigned)__hip_atomic_load(J.acts() + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  pre_wait(bseq);                                    // (the replay checks' first level rows, verify_preload)
  job_wait(J, mine, B);
  const double* bvg = J.bv(G::A);
  for (int k = tid_local(); k < B; k += G::THREADS) L.bv[k] = bvg[k];
  __syncthreads();
  if (st) st->lap(43);
}

// dst[0] = w0, dst[k + 1] = dst[k] + (neg ? -v[k] : v[k]) for k < B: the
// sequential f64 sums (lane 0), 8 at a time without branches, the next 8
// loads in flight: v is read up to 15 and dst written up to 7 entries past B
// (those sums are never read).  Wave-level.
template <class G>
__device__ __forceinline__ double prefix_sums(double w0, const double* __restrict__ v, int B, bool neg,
                                              double* __restrict__ dst) {
  double w = w0;
  if (lane_id_local() == 0) {
    if (dst) dst[0] = w;
    double x[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) x[u] = v[u];
    for (int k0 = 0; k0 < B; k0 += 8) {
      double y[8];                                 // the next chunk's loads, in flight during the chain
#pragma unroll
      for (int u = 0; u < 8; ++u) y[u] = v[k0 + 8 + u];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        if (k0 + u < B) w = w + (neg ? -x[u] : x[u]);
        if (dst) dst[k0 + u + 1] = w;
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) x[u] = y[u];
    }
  }
  return w;                                        // lane 0: the sum over all B
}

// Batched root phase.  While the root has unexpanded eligible children,
// select_leaf (self_play.py:283-287; main.py's select the same) picks one of
// them by the simulation's draw alone -- no value enters the choice -- so the
// first K = min(S, #eligible root children) simulations expand K distinct
// root children in an order fixed before any of them is evaluated.  They run
// as one batch: the root's conv once, batch_expand, then the K backups in
// simulation order, so every sum is the sequential one and the tree is the
// same node for node.  Returns K (0: no batch).
template <class G, class Acc>
__device__ __forceinline__ int root_batch(Smem<G>& sm, const NetParams& np, const SearchParams& sp,
                                          const EngineArrays& E, int g, const TreeView& TV, Acc& T, float* pool,
                                          float* scratch, int* nact, uint64_t key, Stamp* st = nullptr) {
  auto& L = sm.u.f;
  if constexpr (!decltype(sm.u.f)::BATCH) {
    return 0;
  } else {
    const int S = sp.num_simulations;
    // eligible root children (prior > 0, as select_leaf decides)
    if (wave_id() == 0) {
      int n = 0;
#pragma unroll
      for (int j = 0; j < G::AP; ++j) {
        const int a = lane_id_local() + 64 * j;
        n += __popcll(__ballot(a < G::A && T.root_prior(a) > 0.0));
      }
      if (lane_id_local() == 0) sm.t.bcast = n < S ? n : S;
    }
    __syncthreads();
    const int K = sm.t.bcast;
    if (K == 0) return 0;
    // the simulations' choices: sim k takes the r_k-th (ascending) of the
    // n - k eligible root children not taken yet, r_k = randbelow(draw_k, n - k)
    uint64_t el[G::AP];
    int n = 0;
    if (wave_id() == 0) {
      const int lane = lane_id_local();
#pragma unroll
      for (int j = 0; j < G::AP; ++j) {
        const int a = lane + 64 * j;
        el[j] = __ballot(a < G::A && T.root_prior(a) > 0.0);
        n += __popcll(el[j]);
      }
    }
    // the root's conv Y (its latent is in the scratch slot), then Y and the
    // head weights into LDS.  The conv overwrites the whole union, so the
    // batch's LDS buffers are filled only after it.  (Shared jobs: the picks
    // go out while the helpers run the conv's strips.)
    if (shared_jobs<G>(sp)) {
      conv_shared<G>(sm, np, E, g, 0, sp.net, st, -1, 0, [&](unsigned cb) {
        if (wave_id() == 0) pick_all<G>(el, n, 0, K, key, 0, L.acts, st, job_of<G>(E, g).acts(), cb + 1);
      });
    } else {
      latent_conv<G, G::C, G::C, 0, true>(sm, np.w_dyn, np.b_dyn, scratch, G::CS, nullptr, pool, G::CS, G::CS,
                                          nullptr, nullptr, y_lds_target<G>(sm));
    }
    __syncthreads();
    if (st) st->lap(60);
    if (y_lds_target<G>(sm) != nullptr && !shared_jobs<G>(sp)) load_hw<G>(sm, np.head_w);   // (Y in L.yc already)
    else load_y<G>(sm, pool, np.head_w);
    if (tid_local() == 0) { sm.t.npick = 0; sm.t.ngrab = 0; }
    __syncthreads();
    if (st) st->lap(61);
    if (shared_jobs<G>(sp)) {
      batch_expand_shared<G, Acc::LDS>(sm, np, sp, E, g, TV, K, 1, 0, sp.net, pool, el, n, 0, key, 0, nullptr, true);
    } else {
      if (wave_id() == 0) pick_sequence<G>(el, n, 0, K, key, 0, L.acts, &sm.t.npick, G::WAVES);
      batch_expand<G, Acc::LDS>(sm, np, sp, TV, K, 1, pool, st);
    }
    __syncthreads();
    if (st) st->lap(62);
    if (wave_id() == 0) {
      const int lane = lane_id_local();
      // the K backups of backpropagate(path + [child], v) (self_play.py:337-343)
      for (int k = lane; k < K; k += 64) {
        const int a = L.acts[k], nid = 1 + k;
        const double v = L.bv[k];
        T.init(nid);
        T.add(nid, v);
        T.set_child(0, a, nid);
        T.add_root_child(a, v);
        nact[nid] = a;
      }
      if (lane == 0) {
        const bool alt = sp.variant == 0;   // main.py:366-368 does not alternate
        // the root's sum in simulation order: the same f64 additions, the
        // running sum in a register (prefix_sums' chain) instead of LDS
        const double wroot = prefix_sums<G>(T.ws(0), L.bv, K, alt, nullptr);
        T.set(0, T.vis(0) + K, wroot);
        sm.t.newest = -1;                    // every prior row is in HBM already
        sm.t.ycache = 0;                     // L.yc holds the root's Y
      }
    }
    __syncthreads();
    return K;
  }
}

// Parallel replay of a speculative batch (factored dynamics, LDS trees).
//
// The batch's B children of `leaf` (depth D, path p_0 = root .. p_D = leaf)
// stand for simulations sim .. sim + B - 1; simulation sim + i (i >= 1)
// reaches the leaf again iff, at every level l < D, p_l's PUCT still picks
// the path child x_l = p_(l+1) after the i earlier simulations were backed
// up (it then takes acts[i] at the leaf: its draw, by construction).  Those
// i backups are known in advance (their values are the batch's), so every
// check (i, l) is independent: the state it sees is p_l's children as they
// are now, except x_l with n_x + i visits and value sum W_x(i) (the prefix
// sum, in simulation order, of its shares), and p_l with N + i visits.  All
// (i, l) checks run at once over the workgroup with puct_pick's operations
// and first-maximum rule; the batch is accepted up to the first failing i,
// and the tree takes the accepted simulations' sums.  Returns the number of
// accepted simulations m >= 1 (all threads; synchronised).
template <class G, int DMAX>
struct VerifyLds {
  double cP[DMAX][64 * G::AP];      // c_puct * P as puct_pick forms it
  double q[DMAX][64 * G::AP];       // W / N of every child, now
  double inv1n[DMAX][64 * G::AP];   // 1 / (1 + N) of every child, now (the screening pass)
  int n[DMAX][64 * G::AP];
  // per (level, i): x's q after i accepted simulations, 1 / (hi - lo) of the
  // level's q range then (0: no spread), the sqrt term, and x's exact score
  double qx[DMAX][G::A + 1], invr[DMAX][G::A + 1], sq[DMAX][G::A + 1], sx[DMAX][G::A + 1];
  uint64_t elig[DMAX][G::AP];
  double lo_o[DMAX], hi_o[DMAX];    // min / max of q over eligible children other than x
  double cpx[DMAX];                 // x's c_puct * P
  int x[DMAX], n0[DMAX], N0[DMAX];
  double wpre[DMAX][G::A + 9];      // x_l's value sum after i accepted simulations (+ prefix_sums' tail)
  double wroot[G::A + 9];           // the root's value sum after i
  uint64_t failm[G::AP];            // simulations i whose walk leaves the batch (bit i)
  uint64_t exactm[DMAX][G::AP];     // (level, i) checks the screening left open
  int fail;
};
// levels verify_batch holds at once (its arrays are per level; a deeper path
// is checked in groups of this many levels): 8 at 9x9 and below, 2 at 19x19
template <class G>
constexpr int verify_depth() { return G::AP > 2 ? 2 : 8; }
// A speculative batch of B children of a leaf at depth D is replayed one
// select at a time (B - 1 walks of D + 1 levels) while (B - 1) * (D + 1) <
// kSeqK, else by the parallel replay (verify_batch; the trees are the same
// either way).  Measured, 9x9 / 256 / 200 epoch, same call: K = 8 / 12 / 16 /
// 24: 77.1 / 78.1 / 79.0 / 77.8 M sims/s (a minimum-B rule at its best, 6:
// 77.0-77.2); HBM trees with helper workgroups (shared jobs, 19x19): K = 0 /
// 8 / 16 / 32 / 64: 37.8 / 37.8 / 38.0 / 38.3 / 37.7 M
// (profiles/r4x_shared_seq_ab.txt).  With the value cache (sim_loop) a
// re-batch no longer pays an expansion; measured again, same call, three runs
// each: K = 8 / 16 / 24: 137.6-137.9 / 139.1-139.4 / 137.3-137.6 M
// (profiles/vc_knobs.txt)
constexpr int kSeqK = 16, kSharedSeqK = 32;
__device__ __forceinline__ bool replay_sequential(int B, int depth) { return (B - 1) * (depth + 1) < kSeqK; }
__device__ __forceinline__ bool replay_parallel(bool shared, int B, int depth) {
  if (shared) return (B - 1) * (depth + 1) >= kSharedSeqK;
  return !replay_sequential(B, depth);
}

// Phase 1a of verify_batch for one path level l (row k of vl): its
// children's c_puct * P, q, 1 / (1 + n), n and eligibility, the min / max of
// q over the eligible children other than x_l, and x_l's terms.  Reads the
// tree only (not the batch's values), so it may run before the batch is
// done.  Wave-level.
template <class G, class Acc, class V>
__device__ __forceinline__ void verify_load_level(Smem<G>& sm, const SearchParams& sp, const TreeView& TV,
                                                  const Acc& T, const int* nact, V& vl, int k, int l, int ract) {
  const int lane = lane_id_local();
  const int p = T.path(l);
  const int xa = l == 0 ? ract : nact[T.path(l + 1)];
  double lo = INFINITY, hi = -INFINITY, cpx = 0.0;
  int nx = 0;
#pragma unroll
  for (int j = 0; j < G::AP; ++j) {
    const int a = lane + 64 * j;
    const bool in = a < G::A;
    double P, w = 0.0;
    int n = 0;
    if (l == 0) {
      P = in ? T.root_prior(a) : 0.0;
      if constexpr (Acc::LDS) {
        if (in) { n = sm.t.rvis[a]; w = sm.t.rws[a]; }     // the root-child mirror
      } else {
        const int c = in ? T.child(0, a) : -1;
        if (c >= 0) { n = T.vis(c); w = T.ws(c); }
      }
    } else {
      P = in ? (double)TV.prior[(size_t)p * G::A + a] : 0.0;
      const int c = in ? TV.child[(size_t)p * G::A + a] : -1;
      if (c >= 0) { n = T.vis(c); w = T.ws(c); }
    }
    const bool e = P > 0.0;
    const uint64_t el = __ballot(e);
    const double q = e ? (n > 0 ? ddiv(w, (double)n) : 0.0) : 0.0;
    const double cp = l == 0 ? sp.c_puct * P : (double)((float)sp.c_puct * (float)P);
    vl.cP[k][a] = cp;
    vl.q[k][a] = q;
    vl.inv1n[k][a] = 1.0 / (double)(1 + n);
    vl.n[k][a] = n;
    if (lane == 0) vl.elig[k][j] = el;
    if (e && a != xa) { lo = fmin_(lo, q); hi = fmax_(hi, q); }
    if (j == (xa >> 6)) {
      nx = __builtin_amdgcn_readlane(n, xa & 63);
      cpx = dpp::lane(cp, xa & 63);
    }
  }
  wave_minmax(lo, hi);
  if (lane == 0) {
    vl.lo_o[k] = lo;
    vl.hi_o[k] = hi;
    vl.x[k] = xa;
    vl.n0[k] = nx;
    vl.N0[k] = T.vis(p);
    vl.cpx[k] = cpx;
  }
}

// verify_batch's checks of path levels l0 .. l0 + nl - 1 (nl <= DV): phases
// 1a-2 and the exact fallback; failing simulations are OR-ed into vl.failm
// (the caller zeroes it once).  with_root: also the root's value sums
// (vl.wroot) on a spare wave.  ract: the root action on the path.  loaded:
// the levels' rows are in vl already (verify_preload).  All threads;
// returns synchronised.
template <class G, class Acc>
__device__ __forceinline__ void verify_levels(Smem<G>& sm, const SearchParams& sp, const TreeView& TV, const Acc& T,
                                              const int* nact, int D, int B, int l0, int nl, int ract,
                                              bool with_root, Stamp* st = nullptr, bool loaded = false,
                                              int BE = 0) {
  constexpr int DV = verify_depth<G>();
  typedef VerifyLds<G, DV> V;
  V& vl = *reinterpret_cast<V*>(&sm.u.f.wv[0]);
  const int wave = __builtin_amdgcn_readfirstlane(wave_id());
  const int lane = lane_id_local();
  const bool alt = sp.variant == 0;
  const double* bv = sm.u.f.bv;
  if (BE < B) BE = B;                             // (B + 1: simulation sim + B's walk is checked too)
  if (tid_local() < DV * G::AP) (&vl.exactm[0][0])[tid_local()] = 0;
  // ---- 1a. jobs 0..nl-1: level l0 + k's children (one wave each); jobs
  // nl..2nl-1: x's sequential value sums for those levels, and in the first
  // group job 2nl: the root's, on other waves at the same time ----
  const int njobs = 2 * nl + (with_root ? 1 : 0);
  for (int job = wave; job < njobs; job += G::WAVES) {
    if (job == 2 * nl) {                          // the root's value sum after i simulations
      prefix_sums<G>(T.ws(0), bv, B, alt && ((D + 1) & 1), vl.wroot);
      continue;
    }
    if (job >= nl) {                              // x_l = p_(l+1), depth l + 1
      const int k = job - nl, l = l0 + k;
      prefix_sums<G>(T.ws(T.path(l + 1)), bv, B, alt && ((D - l) & 1), vl.wpre[k]);
      continue;
    }
    if (!loaded) verify_load_level<G, Acc>(sm, sp, TV, T, nact, vl, job, l0 + job, ract);
    if (st) st->lap(75);
  }
  __syncthreads();
  if (st) st->lap(76);
  // ---- 1b. per level, per simulation i (lane i = lane + 64 j): the level
  // as simulation i's select finds it, and x's score exactly as puct_pick
  // forms it; a score that is not finite fails i ----
  for (int k = wave; k < nl; k += G::WAVES) {
    const int nx = vl.n0[k], N0 = vl.N0[k];
    const double lo = vl.lo_o[k], hi = vl.hi_o[k], cpx = vl.cpx[k];
#pragma unroll
    for (int j = 0; j < G::AP; ++j) {
      const int i = lane + 64 * j;
      bool bad = false;
      if (i <= B) {
        const int n1 = nx + i, Ni = N0 + i;
        const double qxi = n1 > 0 ? ddiv(vl.wpre[k][i], (double)n1) : 0.0;
        const double loi = fmin_(lo, qxi), hii = fmax_(hi, qxi);
        const double sqi = dsqrt((double)(sp.variant == 1 ? Ni + 1 : (Ni > 1 ? Ni : 1)));
        const double sxi = (hii > loi ? ddiv(qxi - loi, hii - loi) : qxi) + ddiv(cpx * sqi, (double)(1 + n1));
        vl.qx[k][i] = qxi;
        vl.invr[k][i] = hii > loi ? 1.0 / (hii - loi) : 0.0;
        vl.sq[k][i] = sqi;
        vl.sx[k][i] = sxi;
        bad = i >= 1 && i < BE && !(sxi > -INFINITY);
      }
      const uint64_t bb = __ballot(bad);
      if (lane == 0 && bb) atomicOr(reinterpret_cast<unsigned long long*>(&vl.failm[j]), (unsigned long long)bb);
    }
    if (st) st->lap(77);
  }
  __syncthreads();
  if (st) st->lap(72);
  // ---- 2. every (i, l) check at once, transposed: lanes are simulations
  // i = lane + 64 j, each wave takes every WAVES-th child a of each level.
  // Screening: the two divisions of a's score as products with reciprocals
  // (a few ulp off); a decides (l, i) only if its score is clear of x's by
  // far more than that, else (l, i) is redone below with puct_pick's exact
  // operations.  i fails if any eligible a != x beats x (puct_pick's first
  // maximum: a higher score, or an equal one at a lower action). ----
  const unsigned long long ts0 = st ? st->now() : 0;
  for (int k = 0; k < nl; ++k) {
    const int xa = vl.x[k];
    const double lo_o = vl.lo_o[k], hi_o = vl.hi_o[k];
    double loi[G::AP], invr[G::AP], sqi[G::AP], sxi[G::AP], tol[G::AP];
    bool spread[G::AP];
    uint64_t beaten[G::AP], close[G::AP];
#pragma unroll
    for (int j = 0; j < G::AP; ++j) {
      const int i = lane + 64 * j;
      const int ii = i <= B ? i : B;
      const double qxi = vl.qx[k][ii];
      loi[j] = fmin_(lo_o, qxi);
      spread[j] = fmax_(hi_o, qxi) > loi[j];
      invr[j] = vl.invr[k][ii];
      sqi[j] = vl.sq[k][ii];
      sxi[j] = vl.sx[k][ii];
      tol[j] = 1e-12 * (1.0 + fabs(sxi[j]));
      beaten[j] = 0;
      close[j] = 0;
    }
    // the wave's children a = wave + WAVES k, one per lane k, loaded in one
    // round trip; the loop broadcasts them with readlane
    constexpr int KW = (G::A + G::WAVES - 1) / G::WAVES;
    static_assert(KW <= 64, "one lane per child of the wave");
    const int amine = wave + G::WAVES * lane;
    const bool mine = lane < KW && amine < G::A && amine != xa &&
                      ((vl.elig[k][(amine < G::A ? amine : 0) >> 6] >> (amine & 63)) & 1ull);
    const int ac = mine ? amine : 0;
    const double qa_l = vl.q[k][ac], cpa_l = vl.cP[k][ac], ia_l = vl.inv1n[k][ac];
    const uint64_t todo = __ballot(mine);
    for (uint64_t mm = todo; mm; mm &= mm - 1) {
      const int kk = __builtin_ctzll(mm);
      const double qa = dpp::lane(qa_l, kk), cpa = dpp::lane(cpa_l, kk), ia = dpp::lane(ia_l, kk);
#pragma unroll
      for (int j = 0; j < G::AP; ++j) {
        if (64 * j >= BE) break;                    // (uniform) no simulation i in this register
        const double sc = (spread[j] ? (qa - loi[j]) * invr[j] : qa) + (cpa * sqi[j]) * ia;
        beaten[j] |= __ballot(sc > sxi[j] + tol[j]);
        close[j] |= __ballot(!(fabs(sc - sxi[j]) > tol[j]));
      }
    }
    if (lane == 0) {
#pragma unroll
      for (int j = 0; j < G::AP; ++j) {
        if (beaten[j]) atomicOr(reinterpret_cast<unsigned long long*>(&vl.failm[j]), (unsigned long long)beaten[j]);
        if (close[j] & ~beaten[j])
          atomicOr(reinterpret_cast<unsigned long long*>(&vl.exactm[k][j]), (unsigned long long)(close[j] & ~beaten[j]));
      }
    }
  }
  if (st) st->wave_add(80, st->now() - ts0);
  __syncthreads();
  if (st) st->lap(78);
  // the open (l, i) checks with puct_pick's exact operations (rare)
  for (int k = 0; k < nl; ++k) {
    uint64_t open[G::AP];
#pragma unroll
    for (int j = 0; j < G::AP; ++j) {
      const uint64_t o = vl.exactm[k][j] & ~vl.failm[j];
      open[j] = ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(o >> 32)) << 32) |
                __builtin_amdgcn_readfirstlane((uint32_t)o);
    }
    int c = 0;
#pragma unroll
    for (int j = 0; j < G::AP; ++j) {
      for (uint64_t mm = open[j]; mm; mm &= mm - 1, ++c) {
        if (c % G::WAVES != wave) continue;
        const int i = 64 * j + __builtin_ctzll(mm);
        if (i < 1 || i >= BE) continue;
        const int xa = vl.x[k];
        const int nx = vl.n0[k] + i;
        const double qx = vl.qx[k][i];
        const double lo = fmin_(vl.lo_o[k], qx), hi = fmax_(vl.hi_o[k], qx);
        const double sq = vl.sq[k][i], sx = vl.sx[k][i];
        uint64_t beat = 0;
#pragma unroll
        for (int jj = 0; jj < G::AP; ++jj) {
          const int a = lane + 64 * jj;
          const bool el = (vl.elig[k][jj] >> lane) & 1ull;
          const bool isx = a == xa;
          const double q = isx ? qx : vl.q[k][a];
          const int n = isx ? nx : vl.n[k][a];
          const double qn = hi > lo ? ddiv(q - lo, hi - lo) : q;
          const double sc = qn + ddiv(vl.cP[k][a] * sq, (double)(1 + n));
          beat |= __ballot(el && !isx && (sc > sx || (sc == sx && a < xa)));
        }
        if (beat && lane == 0)
          atomicOr(reinterpret_cast<unsigned long long*>(&vl.failm[i >> 6]), 1ull << (i & 63));
      }
    }
  }
  __syncthreads();
  if (st) st->lap(79);
}

// How verify_batch splits a depth-D path: groups of gs levels; shared: the
// groups are a job (HBM trees with helper workgroups): one level per group
// while the groups do not outnumber the 4 workgroups, else DV; otherwise
// the game's workgroup checks groups of DV itself.  g0: group 0's levels.
struct VerifyPlan {
  int gs, ngroups, g0;
  bool shared;
};
template <class G, class Acc>
__device__ __forceinline__ VerifyPlan verify_plan(const SearchParams& sp, int D) {
  constexpr int DV = verify_depth<G>();
  VerifyPlan v;
  v.gs = D <= 4 ? 1 : DV;
  v.ngroups = (D + v.gs - 1) / v.gs;
  v.shared = !Acc::LDS && shared_jobs<G>(sp) && v.ngroups > 1;
  if (!v.shared) { v.gs = DV; v.ngroups = (D + DV - 1) / DV; }
  v.g0 = D < v.gs ? D : v.gs;
  return v;
}

// verify_batch's group-0 level rows (phase 1a's tree loads), made while the
// batch's last children are still being expanded (they read the tree, not
// the batch's values; vl overlays the batch's wave buffers, which the game's
// workgroup is done with).  All threads; no barrier.
template <class G, class Acc>
__device__ __forceinline__ void verify_preload(Smem<G>& sm, const SearchParams& sp, const TreeView& TV, const Acc& T,
                                               const int* nact, int D) {
  if constexpr (decltype(sm.u.f)::BATCH) {
    typedef VerifyLds<G, verify_depth<G>()> V;
    V& vl = *reinterpret_cast<V*>(&sm.u.f.wv[0]);
    const VerifyPlan v = verify_plan<G, Acc>(sp, D);
    for (int k = __builtin_amdgcn_readfirstlane(wave_id()); k < v.g0; k += G::WAVES)
      verify_load_level<G, Acc>(sm, sp, TV, T, nact, vl, k, k, sm.t.ract);
  }
}

// kJobReplay's share: groups of I.group() levels of the depth-I.depth path,
// claimed one at a time (preloaded: group 0 first, its level rows are in vl
// and its unit was taken at the post); the failing simulations this
// workgroup found are ORed into J.failm.  Returns its groups.  All threads.
template <class G, class Acc>
__device__ __forceinline__ int replay_share(Smem<G>& sm, const SearchParams& sp, const TreeView& TV, const Acc& T,
                                            const int* nact, const JobView& J, const JobInfo& I, unsigned bseq,
                                            Stamp* st = nullptr, bool preloaded = false) {
  typedef VerifyLds<G, verify_depth<G>()> V;
  V& vl = *reinterpret_cast<V*>(&sm.u.f.wv[0]);
  const int gs = I.group(), D = I.depth;
  int mine = 0;
  if (preloaded) {
    verify_levels<G, Acc>(sm, sp, TV, T, nact, D, I.batch, 0, min(gs, D), I.act, false, st, true);
    ++mine;
  }
  for (int grp; (grp = job_claim(sm, J, bseq, I.units, 1)) >= 0; ++mine)
    verify_levels<G, Acc>(sm, sp, TV, T, nact, D, I.batch, grp * gs, min(gs, D - grp * gs), I.act, false, st);
  if (mine > 0 && tid_local() < G::AP && vl.failm[tid_local()])
    __hip_atomic_fetch_or(J.h->failm + tid_local(), (unsigned long long)vl.failm[tid_local()], __ATOMIC_RELAXED,
                          __HIP_MEMORY_SCOPE_AGENT);
  return mine;
}
// A helper's share (declared in mzgo_jobs.hpp): the batch's values and an
// empty fail mask into its LDS first.
template <class G>
__device__ __forceinline__ int replay_help(Smem<G>& sm, const SearchParams& sp, const EngineArrays& E, int g,
                                           const TreeView& TV, const JobView& J, const JobInfo& I, unsigned bseq) {
  typedef VerifyLds<G, verify_depth<G>()> V;
  V& vl = *reinterpret_cast<V*>(&sm.u.f.wv[0]);
  const double* bvg = J.bv(G::A);
  for (int k = tid_local(); k < I.batch; k += G::THREADS) sm.u.f.bv[k] = bvg[k];
  if (tid_local() < G::AP) vl.failm[tid_local()] = 0;
  __syncthreads();
  const TreeAcc<G, false> T(TV, sm.t);
  return replay_share<G, TreeAcc<G, false>>(sm, sp, TV, T, E.nact + (size_t)g * ((size_t)E.S + 1), J, I, bseq);
}

template <class G, class Acc>
__device__ __forceinline__ int verify_batch(Smem<G>& sm, const SearchParams& sp, const EngineArrays& E, int g,
                                            const TreeView& TV, Acc& T, int* nact, int leaf, int D, int B, int nid,
                                            Stamp* st = nullptr, bool preloaded = false, bool ext = false,
                                            bool* resume = nullptr, bool yleaf_lds = true) {
  // ext (LDS trees; the batch takes every unexpanded child of the leaf and
  // the search goes on after it): column i = B is checked as well -- the walk
  // of simulation sim + B, after all B backups -- and *resume tells whether
  // that walk reaches the leaf again (only if the batch is accepted in full):
  // the caller's next select then starts at the leaf, on the path as it is.
  // yleaf_lds: L.yc holds the leaf's Y (false: a batch whose values came from
  // the value cache, which loads no Y)
  if constexpr (!decltype(sm.u.f)::BATCH) {
    return 0;                                       // (no speculative batches without the batch LDS)
  } else {
  constexpr int DV = verify_depth<G>();
  typedef VerifyLds<G, DV> V;
  static_assert(sizeof(V) <= sizeof(sm.u.f.wv), "verification arrays overlay the batch buffers");
  V& vl = *reinterpret_cast<V*>(&sm.u.f.wv[0]);
  const int lane = lane_id_local();
  const bool alt = sp.variant == 0;
  const double* bv = sm.u.f.bv;
  // the node at depth d takes the share v (-1)^(D + 1 - d) of a batch child's backup
  if (tid_local() < G::AP) vl.failm[tid_local()] = 0;
  // Levels l0 .. l0 + nl - 1 at a time (every (i, l) check is independent of
  // the others; a failing i is recorded in failm whichever group finds it).
  // With helper workgroups (HBM trees), several groups are a job: each
  // workgroup claims groups and ORs its failing simulations into J.failm.
  // (preloaded: group 0's level rows are in vl already -- the game's
  // workgroup checks group 0 itself, first)
  const VerifyPlan vp = verify_plan<G, Acc>(sp, D);
  if (vp.shared) {
    const JobView J = job_of<G>(E, g);
    const JobInfo I = job_info(kJobReplay, vp.ngroups, nid, leaf, vp.gs, sm.t.ract, D, B);
    const unsigned bseq = job_post(J, I, preloaded ? 1u : 0u, [&](unsigned) {   // (J.bv holds the values already)
      if (tid_local() < G::AP)
        __hip_atomic_store(J.h->failm + tid_local(), 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    });
    const int mine = replay_share<G, Acc>(sm, sp, TV, T, nact, J, I, bseq, st, preloaded);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    job_wait(J, mine, I.units);
    if (tid_local() < G::AP)
      vl.failm[tid_local()] = __hip_atomic_load(J.h->failm + tid_local(), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  } else {
    for (int l0 = 0; l0 < D; l0 += DV)
      verify_levels<G, Acc>(sm, sp, TV, T, nact, D, B, l0, D - l0 < DV ? D - l0 : DV, sm.t.ract, l0 == 0, st,
                            preloaded && l0 == 0, ext ? B + 1 : B);
  }
  if ((D == 0 || vp.shared) && tid_local() == 0) prefix_sums<G>(T.ws(0), bv, B, alt && ((D + 1) & 1), vl.wroot);
  if (tid_local() == 0) {
    int f = 64 * G::AP;                                // the first failing simulation (none: past every i)
#pragma unroll
    for (int j = G::AP - 1; j >= 0; --j) {
      uint64_t mm = vl.failm[j];
      if (j == 0) mm &= ~1ull;                         // (simulation i = 0 reached the leaf already)
      if (mm) f = 64 * j + __builtin_ctzll(mm);
    }
    // (B + 1: all B accepted and, ext, column B passed at every level too;
    // without ext the bits from B on hold no check)
    vl.fail = f < B ? f : (ext && !vp.shared && f > B ? B + 1 : B);
  }
  __syncthreads();
  if (st) st->lap(73);
  const int m = vl.fail < B ? vl.fail : B;
  if (resume) *resume = vl.fail > B;
  // ---- 3. the tree takes the m accepted simulations: path node p_d (d >= 1)
  // gets m visits and the first m of its shares, summed in simulation order
  // (prefix_sums' f64 chain, one lane per node) ----
  if (wave_id() == 0) {
    for (int d = lane; d <= D; d += 64) {
      if (d == 0) {
        T.set(0, T.vis(0) + m, vl.wroot[m]);
      } else {
        const int p = T.path(d);
        const bool neg = alt && ((D + 1 - d) & 1);
        double w = T.ws(p);
#pragma unroll 8
        for (int k = 0; k < m; ++k) w = w + (neg ? -bv[k] : bv[k]);
        const int n = T.vis(p) + m;
        T.set(p, n, w);
        if constexpr (Acc::LDS)
          if (d == 1) { sm.t.rvis[sm.t.ract] = n; sm.t.rws[sm.t.ract] = w; }
      }
    }
    wave_lds_sync();
    for (int i = lane; i < m; i += 64) {            // the new children
      const int ai = sm.u.f.acts[i], n2 = nid + i;
      const double v = 0.0 + bv[i];
      T.set(n2, 1, v);
      nact[n2] = ai;
      T.set_child(leaf, ai, n2);
      if (leaf == 0) T.add_root_child(ai, v);       // (set_child zeroed the mirror)
    }
    if (lane == 0) { sm.t.newest = -1; if (yleaf_lds) sm.t.ycache = leaf; }
  }
  __syncthreads();
  if (st) st->lap(74);
  return m;
  }
}

// The simulations of one search with the tree accessor Acc (LDS or HBM stats).
//
// Factored dynamics also batch SPECULATIVELY: once a simulation's select ends
// at a leaf with u >= 2 unexpanded eligible children, the next simulations
// will pick further unexpanded children of the same leaf -- in an order fixed
// by their draws -- as long as the select walk from the root reaches that
// leaf again.  In the reference's trees it does ~99 % of the time (the same
// depth-1 node keeps the root's PUCT maximum).  So B children of the leaf are
// expanded as one batch (batch_expand), and wave 0 then replays the
// simulations one by one: select from the root (exactly as the sequential
// loop would, on the tree as it stands); if it reaches the predicted (leaf,
// action), the precomputed child is attached and backed up; at the first
// miss the batch's remaining children are dropped (their node ids and rows
// are reused) and the loop continues from that select.  The tree is the
// sequential one node for node.
template <class G, class Acc>
__device__ __forceinline__ void sim_loop(Smem<G>& sm, const NetParams& np, const SearchParams& sp,
                                         const EngineArrays& E, int g, const TreeView& TV, uint64_t key) {
  float* pool = pool_of<G>(E, g);
  const size_t node_floats = (size_t)G::C * G::CS;
  float* scratch = pool + (size_t)(E.S + 1) * node_floats;
  int* nact = E.nact + (size_t)g * ((size_t)E.S + 1);
  const int S = sp.num_simulations;
  const bool factored = sp.factored != 0;
  constexpr bool BATCH = decltype(sm.u.f)::BATCH;
  Acc T(TV, sm.t);
  tree_reset_root<G>(T);
  if (tid_local() == 0) {
    sm.t.newest = -1; sm.t.newp_node = -1; sm.t.ycache = -1; sm.t.rowc_node = -1; sm.t.lognode = -1;
  }
  __syncthreads();

  int nodes = 1, convs = 0;
  // The value cache (LDS trees with the batch LDS, factored dynamics).  A
  // batch at leaf L takes every unexpanded child of L unless the search ends
  // inside it, and a child's backup value depends on L's Y and its action
  // only.  So when the replay cuts such a batch at m < B, the children still
  // unexpanded at L are exactly the dropped ones: their values go to
  // E.cval[L][action] and L's bit in sm.t.cvm is set (cleared with the tree,
  // tree_reset_root).  The next batch at L takes its values from there: no Y
  // reload, no expansion.  Stored at the cut only, by waves other than wave 0
  // (whose next loads are the pending select's): an accepted batch pays
  // nothing.  A single expansion (B == 1) at such a leaf keeps expand_heads:
  // its value is summed per cell, in another fp32 order than expand_wave's
  // channel-first totals, so the cached value would differ in its last bits.
  constexpr bool VCACHE = Acc::LDS && BATCH && decltype(sm.u.f)::CACHE;
  const bool vcache = VCACHE && factored && sp.value_cache != 0 && E.cval != nullptr && !shared_jobs<G>(sp);
  int nbcomp = 0, nbcache = 0, ncut = 0;              // batch children expanded / from the cache, batches cut
  // The arrival conv (LDS trees with the LDS Y copy and the one-strip
  // Winograd conv: 9x9; self_play.py's select).  A select that reaches a
  // lazily expanded node X for the first time ends there: X gets its priors
  // and the simulation picks one of its children, all unexpanded, so X's
  // parent conv always follows (a settled node has an eligible child: pass is
  // valid, and child_prior_regs falls back to the uniform row).  That conv
  // needs the parent's Y and E[a_X] only, so it starts at once: X's policy
  // sums are formed at its head, and wave 0 settles X and picks (the rest of
  // the select, settle_arrival) between the MFMA groups of the GEMM's second
  // K half, while its SIMD's other two waves keep the matrix core fed -- in
  // place of sums, barrier, the resumed select on wave 0 with eleven waves
  // idle, barrier, and only then the conv.  (The following batch's picks in
  // the same place measured slower: DESIGN §7.)  The same operations on the same
  // data: trees, records and counters are the sequential ones.  main.py's
  // select (variant 1) can end at a settled node without an action, where no
  // conv runs, and a tail conv job (sp.tail) is handed to helpers: both keep
  // the resumed select.
  constexpr bool ARRIVAL = Acc::LDS && BATCH && G::WINO && decltype(sm.u.f)::CACHE && Wino<G>::NSTRIP == 1;
  const bool arrival = ARRIVAL && factored && sp.arrival_conv != 0 && sp.variant == 0 && !sp.tail &&
                       !shared_jobs<G>(sp);
  int narr_lds = 0, narr_l2 = 0;                      // arrival convs whose parent's Y came from LDS / from L2
  // the batch of every unexpanded child of `leaf` was cut at m of B: keep the
  // dropped children's values (a leaf whose values are stored already, or a
  // batch the search's end shortened, stores nothing).  All threads.
  auto cache_cut = [&](int leaf, int m, int B) {
    double* cv = E.cval + ((size_t)g * ((size_t)E.S + 1) + (size_t)leaf) * G::A;
    for (int i = m + tid_local() - 64; tid_local() >= 64 && i < B; i += G::THREADS - 64)
      cv[sm.u.f.acts[i]] = sm.u.f.bv[i];
    if (tid_local() == 0) sm.t.cvm[leaf >> 5] |= 1u << (leaf & 31);
    __syncthreads();                                  // (the bit, before the next batch's entry reads it)
  };
  // prior rows formed (HBM writes of a node's priors + child row): eager
  // expansions, and lazily expanded nodes on a select's first arrival
  int rows = 0;
  // (batched children with eager rows: the HBM trees' non-shared batches
  // unless self-play keeps their policy head lazy, sp.lazy_rows)
  const bool eager_rows = !(Acc::LDS || shared_jobs<G>(sp) || (decltype(sm.u.f)::GLOBAL_Y && sp.lazy_rows));
  Stamp st(E.stamps);
  int sim = 0;
  if (factored) {
    sim = root_batch<G, Acc>(sm, np, sp, E, g, TV, T, pool, scratch, nact, key, &st);
    if (eager_rows) rows += sim;
    nodes += sim;
    convs += sim > 0 ? 1 : 0;
    st.lap(4);
  }
  bool pending = false;                                   // a select for `sim` is already in sm.t
  // where the next select starts: the root, or the last batch's leaf when its
  // replay showed that the walk comes down to it again (verify_batch, ext;
  // the path entries and t.ract are that walk's already)
  int node0 = 0, depth0 = 0;
  while (sim < S) {
    if (!pending) {
      if (wave_id() == 0) {
        const int a = select_leaf<G>(sm.t, T, sp, key, sim, &st, node0, depth0);
        if (lane_id_local() == 0) sm.t.action = a;
        st.wave_add(92, 1);
        st.wave_add(95, (unsigned long long)sm.t.depth);
      }
      __syncthreads();
    }
    pending = false;
    node0 = 0;
    depth0 = 0;
    // the walk reached a lazily expanded node for the first time: its policy
    // sums from its parent's Y and E[a] by the whole workgroup, then wave 0
    // resumes the walk there (it settles the node's priors and goes on)
    bool arrive = false;                                  // ... or, the arrival conv: under X's parent conv
    while (sm.t.action == kNeedLogits) {
      if (arrival) { arrive = true; break; }
      const int xn = sm.t.leaf, xd = sm.t.depth;
      st.lap(0);
      // the parent is nearly always the last batch's leaf, whose Y and head
      // weights the expansion's LDS copies still hold (sm.t.ycache; the
      // replay's arrays overlay the batch buffers only): the same sums from
      // LDS instead of L2.  A workgroup-uniform branch; each side's loads
      // keep their address space.
      if (y_lds_target<G>(sm) != nullptr && sm.t.ycache == sm.t.lpar)
        policy_sums_wg<G>(sm.t.logits, sm.u.f.yc, np.etab + (size_t)sm.t.lact * 9 * G::C, sm.u.f.hw);
      else
        policy_sums_wg<G>(sm.t.logits, pool + (size_t)sm.t.lpar * node_floats,
                          np.etab + (size_t)sm.t.lact * 9 * G::C, np.head_w);
      if (tid_local() == 0) sm.t.lognode = xn;
      ++rows;
      __syncthreads();
      st.lap(32);
      if (tid_local() == 0) st.wave_add(34, 1);
      if (wave_id() == 0) {
        const int a = select_leaf<G>(sm.t, T, sp, key, sim, &st, xn, xd);
        if (lane_id_local() == 0) sm.t.action = a;
      }
      __syncthreads();
      st.lap(33);
    }
    st.lap(0);
    // (arrival conv: leaf = X and its depth; the action and the leaf's
    // unexpanded children are known once wave 0 has picked, under the conv)
    int a = sm.t.action;
    const int leaf = sm.t.leaf, depth = sm.t.depth;
    if (a < 0 && !arrive) {                              // terminal leaf: backup 0 (:188-191)
      // self_play.py: terminal leaf -> backup 0 (:188-191); main.py: nothing (:296)
      if (wave_id() == 0 && a == -1) backup<G>(T, depth, -1, 0.0);
      __syncthreads();
      ++sim;
      continue;
    }
    const float* heads;
    const int nid = nodes;
    if (factored) {
      // the leaf's conv Y exists once it has a child; otherwise compute it now
      // (from its latent, rebuilt from its parent's Y unless it is the root)
      float* yleaf = pool + (size_t)leaf * node_floats;
      int yc = sm.t.ycache;
      bool prepicked = false;                            // the batch's picks went out during the conv job
      static_assert(!decltype(sm.u.f)::CACHE || 3 * G::C <= G::THREADS, "one head weight per thread");
      float hwpre = 0.f;                                 // this thread's head weight, fetched before the conv
      bool hwready = false;
      if (arrive || !sm.t.yready) {
        const bool sj = shared_jobs<G>(sp);
        // Winograd boards rebuild the latent inside the conv's input
        // transform (wino_input_rebuilt); the others materialize it first
        if (leaf != 0 && !sj && !G::WINO) {
          const int par = T.path(depth - 1);
          materialize<G>(scratch, pool + (size_t)par * node_floats, np.etab + (size_t)nact[leaf] * 9 * G::C,
                         sm.ulds());
        }
        st.lap(81);
        if (sj) {
          // (the strips read the parent's Y and E rows themselves; the batch's
          // picks are made while the helpers start on them)
          const int nun0 = sm.t.nunexp, B0 = BATCH ? (nun0 < S - sim ? nun0 : S - sim) : 1;
          prepicked = BATCH && B0 >= 2;
          conv_shared<G>(sm, np, E, g, leaf, sp.net, &st, leaf != 0 ? T.path(depth - 1) : -1,
                         leaf != 0 ? nact[leaf] : 0, [&](unsigned cb) {
                           if (prepicked && wave_id() == 0) {
                             uint64_t um0[G::AP];
#pragma unroll
                             for (int j = 0; j < G::AP; ++j)
                               um0[j] = sm.t.umask[j] & ((a >> 6) == j ? ~(1ull << (a & 63)) : ~0ull);
                             pick_all<G>(um0, nun0 - 1, 1, B0 - 1, key, sim + 1, sm.u.f.acts, &st,
                                         job_of<G>(E, g).acts(), cb + 1);
                           }
                         });
        } else if (G::WINO && leaf != 0) {
          const int par = T.path(depth - 1);
          // the expansion's head weights (L.hw, which the conv overwrites) are
          // fetched before the conv and stored after it: the L2 round trip
          // runs under the conv instead of after it
          if constexpr (decltype(sm.u.f)::CACHE) hwpre = tid_local() < 3 * G::C ? np.head_w[tid_local()] : 0.f;
          // a tail helper registered with this game: the conv as a tail job
          bool tail = false;
          if constexpr (TailConvs<G>::value) {
            if (sp.tail) {
              if (tid_local() == 0)
                sm.bc[3] = __hip_atomic_load(&job_of<G>(E, g).h->nhelp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > 0;
              __syncthreads();
              tail = sm.bc[3] != 0;
            }
          }
          if (tail) {
            conv_tail<G>(sm, np, E, g, leaf, par, nact[leaf], sp.net, y_lds_target<G>(sm),
                         y_lds_target<G>(sm) != nullptr && yc == par, &st);
          } else if constexpr (ARRIVAL) {
            const float* ypar = pool + (size_t)par * node_floats;
            const float* ea = np.etab + (size_t)nact[leaf] * 9 * G::C;
            latent_conv_rebuilt<G>(
                sm, np, ypar, ea, yleaf, &st, y_lds_target<G>(sm), yc == par,
                // the arrival conv: X's policy sums from its parent's Y, the LDS
                // copy (before the transform overwrites it) or L2 -- a uniform
                // branch, each side's loads keep their address space
                [&]() {
                  if (arrive) {
                    if (yc == par) policy_sums_wg<G>(sm.t.logits, sm.u.f.yc, ea, sm.u.f.hw);
                    else policy_sums_wg<G>(sm.t.logits, ypar, ea, np.head_w);
                  }
                },
                // ... and the rest of the select on wave 0, under the second K half
                [&]() {
                  if (arrive && __builtin_amdgcn_readfirstlane(wave_id()) == 0) {
                    const unsigned long long t_a = st.now();
                    if (lane_id_local() == 0) sm.t.lognode = leaf;
                    const int ax = settle_arrival<G>(sm.t, T, sp, key, sim, nullptr, leaf, depth);
                    if (lane_id_local() == 0) sm.t.action = ax;
                    st.wave_add(49, st.now() - t_a);
                    st.wave_add(50, 1);
                  }
                });
            if (arrive) {
              ++rows;
              if (yc == par) ++narr_lds; else ++narr_l2;
            }
          } else {
            latent_conv_rebuilt<G>(sm, np, pool + (size_t)par * node_floats, np.etab + (size_t)nact[leaf] * 9 * G::C,
                                   yleaf, &st, y_lds_target<G>(sm), y_lds_target<G>(sm) != nullptr && yc == par);
          }
          hwready = true;
        } else {
          latent_conv<G, G::C, G::C, 0, true>(sm, np.w_dyn, np.b_dyn, scratch, G::CS, nullptr, yleaf, G::CS,
                                              G::CS, nullptr, &st, G::WINO ? y_lds_target<G>(sm) : nullptr);
        }
        __syncthreads();                                 // Y stores before the expansion reads them
        st.lap(82);
        // (wave 0's pick at X: always an action, see above; published by the
        // conv's barriers behind the GEMM, like t.nunexp and t.umask)
        if (arrive) a = sm.t.action;
        // the conv overwrote the union; one-strip Winograd boards got the
        // leaf's Y into L.yc by the conv itself (only the head weights reload)
        if (!sj && G::WINO && y_lds_target<G>(sm) != nullptr) {
          if (hwready) {
            if (tid_local() < 3 * G::C) sm.u.f.hw[tid_local()] = hwpre;
          } else {
            load_hw<G>(sm, np.head_w);
          }
          if (tid_local() == 0) sm.t.ycache = leaf;
          yc = leaf;
          // (a batch follows: its entry's barrier, below, orders these writes
          // too -- nothing reads them before it)
          const int nun1 = sm.t.nunexp;
          if (!(BATCH && (nun1 < S - sim ? nun1 : S - sim) >= 2)) __syncthreads();
        } else {
          yc = -1;
        }
        if (tid_local() == 0) { st.wave_add(59, 1); ++convs; }   // convs run
      }
      const int nun = sm.t.nunexp;
      const int B = BATCH ? (nun < S - sim ? nun : S - sim) : 1;
      if (BATCH && B >= 2) {
        // ---- speculative batch of B children of `leaf` ----
        st.lap(69);
        // a batch at this leaf was cut before: its unexpanded children's
        // backup values are in E.cval (the value cache, above).  L.yc is then
        // left as it is: nothing of this batch reads Y (reloading it anyway, so
        // that a later arrival finds it in LDS, measured 137.0 against 139.3 M
        // sims/s on the 9x9 epoch, profiles/vc_knobs.txt)
        bool cached = false;
        if constexpr (VCACHE) cached = vcache && sm.t.is_cached(leaf);
        if (!cached && yc != leaf) load_y<G>(sm, yleaf, np.head_w);
        if constexpr (Acc::LDS) {
          // the replay's selects read leaf's rows from LDS.  The select that
          // chose the leaf left them there already (select_leaf, keep_rows)
          // unless the leaf is the newest node, whose priors wave 1 wrote
          if (leaf != 0 && sm.t.rowc_node != leaf) {
            for (int i = tid_local(); i < G::A; i += G::THREADS) {
              sm.t.rowc_child[i] = TV.child[(size_t)leaf * G::A + i];
              sm.t.rowc_prior[i] = TV.prior[(size_t)leaf * G::A + i];
            }
            __syncthreads();
            if (tid_local() == 0) sm.t.rowc_node = leaf;
          }
        }
        if (tid_local() == 0) { sm.u.f.acts[0] = a; sm.t.npick = 1; sm.t.ngrab = 0; }
        __syncthreads();
        st.lap(70);
        uint64_t um[G::AP];
#pragma unroll
        for (int j = 0; j < G::AP; ++j) um[j] = sm.t.umask[j];
#pragma unroll
        for (int j = 0; j < G::AP; ++j)
          if ((a >> 6) == j) um[j] &= ~(1ull << (a & 63));
        if (shared_jobs<G>(sp)) {
          batch_expand_shared<G, Acc::LDS>(sm, np, sp, E, g, TV, B, nid, leaf, sp.net, yleaf, um, nun - 1, 1, key,
                                           sim + 1, &st, prepicked, [&](unsigned) {
                                             if (replay_parallel(true, B, depth))
                                               verify_preload<G, Acc>(sm, sp, TV, T, nact, depth);
                                           });
          st.lap(71);
        } else if (cached) {
          // the same picks (same draws, same acts); every picked child is one
          // the cut batch dropped, so its value is the one batch_expand would
          // form again (it depends on the leaf's Y and the action only) and
          // its node takes the lazy mark batch_expand<.., LAZY> would set
          if (wave_id() == 0) {
            pick_all<G>(um, nun - 1, 1, B - 1, key, sim + 1, sm.u.f.acts, &st);
            wave_lds_sync();
            st.lap(71);
            const double* cv = E.cval + ((size_t)g * ((size_t)E.S + 1) + (size_t)leaf) * G::A;
            for (int i = lane_id_local(); i < B; i += 64) {
              sm.u.f.bv[i] = cv[sm.u.f.acts[i]];
              atomicOr(&sm.t.rawp[(nid + i) >> 5], 1u << ((nid + i) & 31));
            }
          }
          nbcache += B;
        } else {
          nbcomp += B;
          if (wave_id() == 0) {
            // every pick at once (pick_all), then published together
            pick_all<G>(um, nun - 1, 1, B - 1, key, sim + 1, sm.u.f.acts, &st);
            wave_lds_sync();
            if (lane_id_local() == 0) __hip_atomic_store(&sm.t.npick, B, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
            st.lap(71);
          }
          batch_expand<G, Acc::LDS>(sm, np, sp, TV, B, nid, yleaf, &st);
        }
        __syncthreads();
        st.lap(5);
        if (eager_rows) rows += B;
        if (replay_parallel(shared_jobs<G>(sp), B, depth)) {
          // the batch takes the leaf's last unexpanded children and another
          // simulation follows: the replay also checks that one's walk down
          // to the leaf, and the next select resumes there if it holds
          const bool ext = Acc::LDS && B == nun && sim + B < S;
          bool resume = false;
          const int m = verify_batch<G, Acc>(sm, sp, E, g, TV, T, nact, leaf, depth, B, nid, &st, shared_jobs<G>(sp),
                                             ext, &resume, !cached);
          if (resume) { node0 = leaf; depth0 = depth; }
          if constexpr (VCACHE)
            if (m < B) {
              if (vcache && !cached && B == nun) cache_cut(leaf, m, B);
              ++ncut;
            }
          nodes += m;
          sim += m;
          st.lap(63);
          if (tid_local() == 0) { st.wave_add(31, 1); st.wave_add(28, (unsigned long long)m); }
          continue;
        }
        if (wave_id() == 0) {
          const int lane = lane_id_local();
          if (lane == 0) { sm.t.newest = -1; if (!cached) sm.t.ycache = leaf; }
          wave_lds_sync();
          int m = 0;
          const bool alt = sp.variant == 0;
          {
            for (int i = 0; i < B; ++i) {
              const int ai = sm.u.f.acts[i];
              if (i > 0) {
                const int a2 = select_leaf<G>(sm.t, T, sp, key, sim + i, &st);
                st.wave_add(92, 1);
                st.wave_add(95, (unsigned long long)sm.t.depth);
                if (a2 != ai || sm.t.leaf != leaf) {           // prediction ends: a2 is sim + i's select
                  if (lane == 0) sm.t.action = a2;
                  break;
                }
              }
              const int n2 = nid + i;
              if (lane == 0) { T.init(n2); nact[n2] = ai; }
              if (lane == (ai & 63)) T.set_child(leaf, ai, n2);
              // the next select reads leaf's child row: from LDS (rowc) on LDS
              // trees; otherwise let the HBM store land first
              if constexpr (!Acc::LDS) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
              backup<G>(T, depth, n2, sm.u.f.bv[i], alt);
              ++m;
            }
          }
          if (lane == 0) sm.t.bcast = m;
          st.wave_add(93, 1);
          st.wave_add(94, (unsigned long long)m);
        }
        __syncthreads();
        const int m = sm.t.bcast;
        if constexpr (VCACHE)
          if (m < B) {
            if (vcache && !cached && B == nun) cache_cut(leaf, m, B);
            ++ncut;
          }
        nodes += m;
        sim += m;
        pending = m < B;
        st.lap(63);
        if (tid_local() == 0) { st.wave_add(31, 1); st.wave_add(28, (unsigned long long)m); }
        continue;
      }
      // ---- one expansion ----
      // (nid may be the id of a dropped batch child: clear its lazy mark, the
      // eager priors below are this node's)
      if (tid_local() == 0) {
        T.init(nid);
        sm.t.newest = nid;
        if constexpr (G::TREE_CAP > 0)
          if (nid < G::TREE_CAP) sm.t.rawp[nid >> 5] &= ~(1u << (nid & 31));
      }
      const unsigned long long t_x = st.now();
      expand_heads<G>(sm.u.f, yleaf, yc == leaf, np.etab + (size_t)a * 9 * G::C, np.head_w);
      if (tid_local() == 0) st.wave_add(56, st.now() - t_x);
      ++rows;
      __syncthreads();
      if (tid_local() == 0 && decltype(sm.u.f)::CACHE) sm.t.ycache = leaf;   // read by all before the barrier
      heads = sm.u.f.xh;
    } else {
      if (tid_local() == 0) { T.init(nid); sm.t.newest = nid; }
      latent_conv<G, G::C, G::C, 3>(sm, np.w_dyn, np.b_dyn, pool + (size_t)leaf * node_floats, G::CS,
                                    np.emb + (size_t)a * G::C, pool + (size_t)nid * node_floats, G::CS, G::CS,
                                    np.head_w, &st);
      heads = sm.heads();
    }
    nodes += 1;
    st.lap(2);
    // wave 1: policy logits -> the new node's priors (published in LDS for a
    // select that reaches it); wave 0, meanwhile: value/reward heads, backup
    // and (next iteration) the next select.  Wave 0 issues no HBM stores, so
    // its tree loads never wait for store acks.  The select barrier joins them.
    if (wave_id() == 1) {
      const unsigned long long t1 = st.now();
      int* crow = TV.child + (size_t)nid * G::A;        // the new node: no children yet
      for (int i = lane_id_local(); i < G::A; i += 64) crow[i] = -1;   // (before its priors are published)
      float x[G::AP];
      if (factored) logits_regs<G, 1>(heads, true, sm.t.hsc, x);
      else logits_regs<G, Smem<G>::HEAD_PARTS>(heads, true, sm.t.hsc, x);
      const unsigned long long t2 = st.now();
      child_priors<G>(sm.t, x, TV.prior + (size_t)nid * G::A, nid, sp.variant);
      st.wave_add(57, t2 - t1);
      st.wave_add(58, st.now() - t2);
    }
    if (wave_id() == 0) {
      float r, v;
      if (factored) heads_value<G, 1>(heads, true, sm.t.hsc, r, v);
      else heads_value<G, Smem<G>::HEAD_PARTS>(heads, true, sm.t.hsc, r, v);
      if (lane_id_local() == (a & 63)) T.set_child(leaf, a, nid);
      if (lane_id_local() == 0) nact[nid] = a;
      backup<G>(T, depth, nid, (double)r + sp.discount * (double)v, sp.variant == 0);
    }
    st.lap(3);
    ++sim;
  }
  __syncthreads();
  st.flush();
  tree_flush<G>(T, nodes);
  if (tid_local() == 0) {
    E.nodes[g] = nodes;
    // direct dynamics: one conv per expansion
    atomicAdd(&E.counters[3], (unsigned long long)(factored ? convs : nodes - 1));
    atomicAdd(&E.counters[5], (unsigned long long)(factored ? rows : nodes - 1));
    if (nbcomp) atomicAdd(&E.counters[9], (unsigned long long)nbcomp);
    if (nbcache) atomicAdd(&E.counters[10], (unsigned long long)nbcache);
    if (ncut) atomicAdd(&E.counters[11], (unsigned long long)ncut);
    if (narr_lds) atomicAdd(&E.counters[12], (unsigned long long)narr_lds);
    if (narr_l2) atomicAdd(&E.counters[13], (unsigned long long)narr_l2);
  }
  __syncthreads();
}

template <class G, class PlaneFn>
__device__ __forceinline__ void run_search(Smem<G>& sm, const NetParams& np, const SearchParams& sp,
                                  const EngineArrays& E, int g, PlaneFn planes, const double* noise,
                                  uint64_t key, unsigned long long* ts = nullptr, double* noise_out = nullptr) {
  const TreeView TV = TreeViewOf<G>::make(E, g);
  if (tid_local() == 0) sm.t.ngrab = 0;             // draw_dirichlet's counter (build_mask's barrier orders it)
  build_mask<G>(sm.t, sp.pass_epsilon, [&](int a) { return planes(3, a); });
  float* pool = pool_of<G>(E, g);
  const size_t node_floats = (size_t)G::C * G::CS;
  // root latent: node 0's slot (direct; node 1's slot is strip-conv scratch) or
  // the scratch slot (factored: node 0's slot receives its conv Y)
  if (sp.factored && shared_jobs<G>(sp))
    representation<G>(sm, np, planes, pool + (size_t)(E.S + 1) * node_floats, G::CS, pool, ts ? ts + 3 : nullptr,
                      [&](int k) { rep_shared<G>(sm, np, E, g, sp.net, k); return true; });
  else if (sp.factored)
    representation<G>(sm, np, planes, pool + (size_t)(E.S + 1) * node_floats, G::CS, pool, ts ? ts + 3 : nullptr);
  else
    representation<G>(sm, np, planes, pool, G::CS, pool + node_floats, ts ? ts + 3 : nullptr);
#ifdef MZGO_STAMPS
  if (ts) ts[0] = __builtin_amdgcn_s_memtime();
#endif
  if (noise) {
    if (wave_id() == 0) root_priors<G>(sm.t, TV, sp, noise, key, nullptr, noise_out);
  } else {
    static_assert(G::AP < G::WAVES, "a wave per 64 Gamma draws besides wave 0");
    draw_dirichlet<G>(sm.t, key, sp.dirichlet_alpha, &sm.t.ngrab);
    if (wave_id() == 0) root_priors<G>(sm.t, TV, sp, noise, key, &sm.t.ngrab, noise_out);
  }
  __syncthreads();
#ifdef MZGO_STAMPS
  if (ts) ts[1] = __builtin_amdgcn_s_memtime();
#endif
  if constexpr (G::TREE_CAP > 0) {
    if (sp.num_simulations + 2 <= G::TREE_CAP) {
      sim_loop<G, TreeAcc<G, true>>(sm, np, sp, E, g, TV, key);
      return;
    }
  }
  sim_loop<G, TreeAcc<G, false>>(sm, np, sp, E, g, TV, key);
}

// root-child visit counts and root value of the finished search
template <class G>
__device__ __forceinline__ void search_outputs(const EngineArrays& E, int g, int* out_visits, double* out_value) {
  const TreeView T = TreeViewOf<G>::make(E, g);
  for (int a = tid_local(); a < G::A; a += G::THREADS) {
    const int c = T.child[a];
    if (out_visits) out_visits[(size_t)g * G::A + a] = c >= 0 ? T.visits[c] : 0;
  }
  if (tid_local() == 0 && out_value) out_value[g] = root_value(T);
}

// Form the priors of every lazily expanded node no select reached
// (TreeLds::rawp): the search API exports whole trees (mzgo_tree_export),
// self-play does not and skips this.  Each wave takes parents p = wave,
// wave + WAVES, ... and every raw child c = child[p][a]: its policy sums
// from p's Y and E[a] (policy_sums_wave), then settle_lazy.  All threads;
// the batch buffers serve as per-wave scratch.
template <class G>
__device__ __forceinline__ void settle_all_priors(Smem<G>& sm, const NetParams& np, const EngineArrays& E, int g,
                                                  int nodes, int variant) {
  if constexpr (decltype(sm.u.f)::BATCH && G::TREE_CAP > 0) {
    const TreeView TV = TreeViewOf<G>::make(E, g);
    const float* pool = pool_of<G>(E, g);
    const int wave = __builtin_amdgcn_readfirstlane(wave_id());
    const int lane = lane_id_local();
    auto& W = sm.u.f.wv[wave];
    static_assert(sizeof(W.xw) >= sizeof(float) * G::CELLS, "a wave's head rows hold one node's policy sums");
    const int lim = nodes < G::TREE_CAP ? nodes : G::TREE_CAP;
    if (wave == 0 && lane == 0) sm.t.lognode = -1;
    for (int p = wave; p < lim; p += G::WAVES) {
      if (sm.t.is_raw(p)) continue;                  // (no children)
      for (int a0 = 0; a0 < G::A; a0 += 64) {
        const int a = a0 + lane;
        const int c = a < G::A ? TV.child[(size_t)p * G::A + a] : -1;
        for (uint64_t m = __ballot(c > 0 && c < lim && sm.t.is_raw(c)); m; m &= m - 1) {
          const int l = __builtin_ctzll(m);
          const int cc = __builtin_amdgcn_readlane(c, l), ca = a0 + l;
          policy_sums_wave<G>(W.xw, pool + (size_t)p * G::C * G::CS, np.etab + (size_t)ca * 9 * G::C, np.head_w);
          wave_lds_sync();
          float x[G::AP], q[G::AP];
          policy_logits<G>(W.xw, sm.t.hsc, x);
          child_prior_regs<G>(sm.t, x, q, variant, W.fb, W.db);
#pragma unroll
          for (int j = 0; j < G::AP; ++j)
            if (lane + 64 * j < G::A) {
              TV.prior[(size_t)cc * G::A + lane + 64 * j] = q[j];
              TV.child[(size_t)cc * G::A + lane + 64 * j] = -1;
            }
          wave_lds_sync();
        }
      }
    }
    __syncthreads();
    for (int i = tid_local(); i < (G::TREE_CAP + 31) / 32; i += G::THREADS) sm.t.rawp[i] = 0u;
  }
  __syncthreads();
}

template <int N, int C>
__global__ void __launch_bounds__((Geo<N, C>::THREADS)) __attribute__((amdgpu_waves_per_eu(Geo<N, C>::WPE, Geo<N, C>::WPE))) k_search(NetParams np_arg, SearchParams sp, EngineArrays E_arg,
                                                      const float* __restrict__ root_obs,
                                                      const double* __restrict__ noise, int game_base,
                                                      int move_index, int* out_visits, double* out_value) {
  typedef Geo<N, C> G;
  __shared__ Smem<G> sm;
  static_assert(sizeof(Smem<G>) <= 160 * 1024, "one workgroup per CU: the whole LDS at most");
  if constexpr (G::WINO) wino_raw_zero<G>(sm.raw);        // zero halo of the conv input planes
  // (as k_selfplay_move: no address arithmetic hoisted into registers kept
  // live across the whole search -- it spilled, 68 B/lane at 19x19)
  const EngineArrays E = launder_arrays(E_arg);
  const NetParams np = launder_params(np_arg);
  const int g = blockIdx.x;
  const float* o = root_obs + (size_t)g * 6 * G::CELLS;
  const uint64_t key = stream_key(sp.seed, (uint32_t)(game_base + g), (uint32_t)move_index);
  run_search<G>(sm, np, sp, E, g, [&](int c, int j) { return o[c * G::CELLS + j]; },
                noise ? noise + (size_t)g * G::A : nullptr, key);
  settle_all_priors<G>(sm, np, E, g, E.nodes[g], sp.variant);
  search_outputs<G>(E, g, out_visits, out_value);
}

// ---------------------------------------------------------------------------
// Boards
// ---------------------------------------------------------------------------
// slot g <- an empty board and a game not yet begun
template <class G>
__device__ __forceinline__ void board_reset_slot(const EngineArrays& E, int g) {
  for (int c = tid_local(); c < G::CELLS; c += G::THREADS) {
    E.stones[(size_t)g * G::CELLS + c] = 0;
    E.invd[(size_t)g * G::CELLS + c] = 0;
  }
  if (tid_local() < 4) E.meta[g * 4 + tid_local()] = 0;
  if (tid_local() == 0) { E.status[g] = 0; E.game_len[g] = 0; E.final_reward[g] = 0.0; }
}

template <int N, int C>
__global__ void __launch_bounds__((Geo<N, C>::THREADS)) __attribute__((amdgpu_waves_per_eu(Geo<N, C>::WPE, Geo<N, C>::WPE))) k_board_reset(EngineArrays E) {
  board_reset_slot<Geo<N, C>>(E, blockIdx.x);
}

// Step every slot with actions[g] >= 0 (gogame.next_state); status[g] gets a
// BOARD_* code; winner[g] = GoEnv.winner() after the step (0 unless ended).
template <int N, int C>
__global__ void __launch_bounds__((Geo<N, C>::THREADS)) __attribute__((amdgpu_waves_per_eu(Geo<N, C>::WPE, Geo<N, C>::WPE))) k_board_step(EngineArrays E, const int* __restrict__ actions,
                                                          int* status, double* winner, double komi) {
  typedef Geo<N, C> G;
  __shared__ Smem<G> sm;
  static_assert(sizeof(Smem<G>) <= 160 * 1024, "one workgroup per CU: the whole LDS at most");
  const int g = blockIdx.x;
  const int a = actions[g];
  if (a < 0) return;
  BoardMeta m;
  board_load<G>(sm.stone, sm.invd, E, g, m);
  BoardLds<G> b = board_lds<G>(sm);
  const int st = board_step<G>(b, m, a);
  __syncthreads();
  if (st == BOARD_OK) board_store<G>(sm.stone, sm.invd, E, g, m);
  double w = 0.0;
  if (st == BOARD_OK && m.done) w = board_winning<G>(b, komi);
  if (tid_local() == 0) {
    if (status) status[g] = st;
    if (winner) winner[g] = w;
  }
}

// f64 observation planes [G][6][CELLS] of the current boards (GoEnv state)
template <int N, int C>
__global__ void __launch_bounds__((Geo<N, C>::THREADS)) __attribute__((amdgpu_waves_per_eu(Geo<N, C>::WPE, Geo<N, C>::WPE))) k_board_planes(EngineArrays E, double* planes) {
  typedef Geo<N, C> G;
  const int g = blockIdx.x;
  const int* mm = E.meta + g * 4;
  double* p = planes + (size_t)g * 6 * G::CELLS;
  for (int j = tid_local(); j < G::CELLS; j += G::THREADS) {
    const int s = E.stones[(size_t)g * G::CELLS + j];
    p[j] = s == 1; p[G::CELLS + j] = s == 2; p[2 * G::CELLS + j] = mm[0];
    p[3 * G::CELLS + j] = E.invd[(size_t)g * G::CELLS + j];
    p[4 * G::CELLS + j] = mm[1]; p[5 * G::CELLS + j] = mm[2];
  }
}

// ---------------------------------------------------------------------------
// One self-play move of the game in slot g (run_self_play_game's loop body,
// self_play.py:465-507): record the observation, search, choose, step the
// board, record the result.  The board is in LDS (sm.stone, sm.invd, m) and
// stays there; slot g is where the game is stored -- its tree, board and
// record rows -- and key_id() (a game_key_id) is who the game is: its RNG keys
// come from that id alone.  (pp.arena and the noise hooks index by slot: their
// launches store game g of one epoch in slot g.)  All threads; returns
// whether the game is over (finish_move).  The kernels that play whole games
// a workgroup each call this: k_selfplay_move and k_selfplay_games.
// CAPS: the launch set playout caps (SearchParams::fast_simulations > 0): the
// move's simulations are move_budget's; without it the instantiation is the
// code it was before the caps existed (the budget is sp.num_simulations at
// compile time), so an engine without caps pays nothing for them.
// (The id is a callable, evaluated where the key is formed: as a value
// computed by the caller it is live across the move's laundered arguments,
// and k_selfplay_move<19,96> spilled a second VGPR, 8 -> 12 B/lane.)
// ---------------------------------------------------------------------------
template <class G, bool CAPS, class KeyId>
__device__ __forceinline__ bool selfplay_one_move(Smem<G>& sm, const NetParams& np_a_arg, const NetParams& np_b_arg,
                                                  const SearchParams& sp, const PlayParams& pp,
                                                  const EngineArrays& E_arg, int g, KeyId key_id, BoardMeta& m) {
#ifdef MZGO_STAMPS
  unsigned long long tm[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  tm[0] = __builtin_amdgcn_s_memtime();
#else
  unsigned long long* tm = nullptr;
#endif
  const int mv = m.moves;
  // this move's view of the arguments (launder_global: no address arithmetic
  // of the move is hoisted above this point)
  const EngineArrays E = launder_arrays(E_arg);
  const NetParams np_a = launder_params(np_a_arg), np_b = launder_params(np_b_arg);
  // arena (main.py:535-549): turn 0 = "current" (np_a), 1 = "best" (np_b); game
  // i starts with turn i % 2 (evaluate, :597-599)
  // (field by field: a reference chosen between the two by-value kernel
  // arguments would copy both to scratch)
  const NetParams np = select_params(pp.arena && (((pp.game_base + g) + mv) & 1), np_b, np_a);
  const size_t rec = (size_t)g * E.max_moves + mv;
  const uint64_t key = move_key(sp, key_id(), mv);
  // playout cap randomization: this move's simulations, the engine's unless
  // the launch set a fast budget (wave-uniform: a scalar register)
  const int budget = move_budget<CAPS>(sp, key);
  record_observation<G>(E, rec, sm.stone, sm.invd, m, CAPS && budget != sp.num_simulations);
  const BoardMeta m0 = m;
  const double* noise = pp.noise ? pp.noise + ((size_t)g * E.max_moves + mv) * G::A : nullptr;
  double* noise_out = pp.noise_out ? pp.noise_out + ((size_t)g * E.max_moves + mv) * G::A : nullptr;
#ifdef MZGO_STAMPS
  tm[1] = __builtin_amdgcn_s_memtime();
#endif
  SearchParams spm = launder_search(sp);
  spm.net = (pp.arena && (((pp.game_base + g) + mv) & 1)) ? 1 : 0;
  if constexpr (CAPS) spm.num_simulations = budget;
  run_search<G>(sm, np, spm, E, g, [&](int c, int j) { return board_plane<G>(sm.stone, sm.invd, m0, c, j); },
                noise, key, tm ? tm + 2 : nullptr, noise_out);
#ifdef MZGO_STAMPS
  tm[4] = __builtin_amdgcn_s_memtime();
#endif

  const TreeView T = TreeViewOf<G>::make(E, g);
  if (wave_id() == 0) {
    const int a = choose_move_action<G>(sm.t, T, sp, pp, mv, key, E.rec_policy + rec * G::A);
    if (lane_id_local() == 0) {
      sm.bc[0] = a;
      E.rec_action[rec] = a;
      E.rec_value[rec] = root_value(T);
    }
  }
  __syncthreads();
  BoardLds<G> b = board_lds<G>(sm);
  double w;
  const int st = play_action<G>(E, g, b, m, sm.bc[0], pp.komi, w);
#ifdef MZGO_STAMPS
  // move phases (slots 83-87): board load + record, representation, root
  // priors, the simulations, action choice + board step
  if (tid_local() == 0 && E.stamps) {
    const unsigned long long t5 = __builtin_amdgcn_s_memtime();
    unsigned long long* sl = E.stamps + (size_t)blockIdx.x * kStampPhases;
    sl[83] += tm[1] - tm[0];
    sl[84] += tm[2] - tm[1];
    sl[85] += tm[3] - tm[2];
    sl[86] += tm[4] - tm[3];
    sl[87] += t5 - tm[4];
    sl[88] += tm[5] - tm[1];                     // representation: board planes + conv1
    sl[89] += tm[6] - tm[5];                     //   conv2
    sl[90] += tm[2] - tm[6];                     //   conv3 + heads
  }
#endif
  return finish_move<G>(E, budget, g, rec, st, m, w);
}

// ---------------------------------------------------------------------------
// One self-play move for every unfinished slot (run_self_play_game's loop
// body, self_play.py:465-507): record the observation, search, choose, step
// the board, record the result; finish the game on double pass or N*N moves.
// ---------------------------------------------------------------------------
template <int N, int C, bool CAPS = false>
__global__ void __launch_bounds__((Geo<N, C>::THREADS)) __attribute__((amdgpu_waves_per_eu(Geo<N, C>::WPE, Geo<N, C>::WPE))) k_selfplay_move(NetParams np_a_arg, NetParams np_b_arg,
                                                             SearchParams sp, PlayParams pp, EngineArrays E_arg) {
  typedef Geo<N, C> G;
  __shared__ Smem<G> sm;
  static_assert(sizeof(Smem<G>) <= 160 * 1024, "one workgroup per CU: the whole LDS at most");
  // blocks past the games are helper workgroups (batch_expand_shared): helper h
  // serves game h % games.  Under round-robin dispatch that is the game's XCD
  // when games % 8 == 0 (every bench and test shape: 64, 256); otherwise a
  // helper may sit on another XCD -- a speed matter only, the job hand-offs
  // are agent-scope release / acquire and placement-independent.
  const int games = gridDim.x - sp.helpers;
  if ((int)blockIdx.x >= games) {
    if constexpr (Smem<G>::GLOBAL_Y && G::WINO) {
      wino_raw_zero<G>(sm.raw);                          // the conv strips' zero halo
      int t = (blockIdx.x - games) % games;
      for (;;) {
        helper_loop<G>(sm, np_a_arg, np_b_arg, sp, E_arg, t);
        if (!sp.tail) break;
        t = join_running_game<G>(sm, E_arg, games, t);   // its game ended: the epoch tail
        if (t < 0) break;
      }
    }
    return;
  }
  const int g = blockIdx.x;
  const EngineArrays& E = E_arg;
  // (every game workgroup counts itself resident: mzgo_stream_wait_started)
  if (tid_local() == 0) atomicAdd(&E_arg.counters[6], 1ull);
  auto release_helpers = [&]() {
    if ((sp.helpers > 0 || sp.tail) && tid_local() == 0) job_exit(job_of<G>(E_arg, g));
  };
  // an ended game's workgroup serves running games: their parent convs (9x9)
  // or all their jobs as one more helper (19x19)
  auto tail_phase = [&]() {
    if constexpr (Smem<G>::GLOBAL_Y && G::WINO) {
      if (sp.tail) {
        __syncthreads();
        for (int t = g; (t = join_running_game<G>(sm, E_arg, games, t)) >= 0;)
          helper_loop<G>(sm, np_a_arg, np_b_arg, sp, E_arg, t);
      }
    }
    if constexpr (TailConvs<G>::value)
      if (sp.tail) {
        __syncthreads();
#ifdef MZGO_STAMPS
        const unsigned long long th = __builtin_amdgcn_s_memtime();
#endif
        tail_help<G>(sm, np_a_arg, np_b_arg, E_arg, g, games);
#ifdef MZGO_STAMPS
        // slot 47: the workgroup's cycles in the tail phase (serving + waiting)
        if (tid_local() == 0 && E_arg.stamps) E_arg.stamps[(size_t)blockIdx.x * kStampPhases + 47] +=
            __builtin_amdgcn_s_memtime() - th;
#endif
      }
  };
  if (E.status[g] != 0) { release_helpers(); tail_phase(); return; }
  if ((sp.helpers > 0 || sp.tail) && tid_local() == 0) job_mark_started(job_of<G>(E_arg, g));
  if constexpr (G::WINO) wino_raw_zero<G>(sm.raw);        // zero halo of the conv input planes
  BoardMeta m;
  board_load<G>(sm.stone, sm.invd, E, g, m);
  // pp.moves moves of this game in one launch (the board stays in LDS between
  // them): a game's moves run back to back on its CU instead of every move of
  // every game waiting for the slowest game's move at a launch boundary
  for (int step = 0; step < pp.moves; ++step) {
    if (selfplay_one_move<G, CAPS>(sm, np_a_arg, np_b_arg, sp, pp, E_arg, g,
                             [&]() { return game_key_id(pp.game_base, g, pp.epoch); }, m))
      break;
    __syncthreads();                               // this move's LDS reads before the next move's writes
  }
  release_helpers();
  tail_phase();
}

// ---------------------------------------------------------------------------
// The move-parallel epoch, first launch: every game's moves without their
// searches (record, legal mask, action, board step, result).  A game's
// moves are a serial chain of board steps, each a dozen passes over the board
// with a barrier apiece, so the step's latency is
// the launch's: a workgroup of BoardsGeo::THREADS (one cell per lane, 2 waves
// at 9x9) with a few KB of LDS instead of k_selfplay_move's 12 waves and 159
// KB.  The move is mzgo_move.hpp's, with this workgroup as the team; what
// only a launch of several moves can do is done here: the board and its
// groups stay in LDS and are updated per move (play_action's HELD), and the
// slot's board and the counters are written once per game.
// ---------------------------------------------------------------------------
template <class G>
struct BoardsGeo {
  static constexpr int THREADS = (G::CELLS + 63) / 64 * 64 < 512 ? (G::CELLS + 63) / 64 * 64 : 512;
  static constexpr int WAVES = THREADS / 64;
};
// The boards launch's team.  Its barriers order LDS only: a wave waits for its
// own LDS operations (lgkmcnt), never for the move's global stores (the
// records, the policy row: nothing in the launch reads them back, and the
// kernel's end publishes them), then joins the workgroup barrier.  (On gfx950
// __syncthreads compiles to the same wait; the fence says so by name.  What
// the team saves is in any(): one barrier and a flag per wave, where
// __syncthreads_or takes two barriers round an LDS reduction -- once per
// labelling round and per legal mask.)  A team of one wave (up to 64 cells)
// needs no barrier: its LDS operations complete in order.
template <class G>
struct BoardsTeam {
  static constexpr int SIZE = BoardsGeo<G>::THREADS;
  static constexpr int WAVES = BoardsGeo<G>::WAVES;
  __device__ static int id() { return tid_local(); }
  __device__ static void sync() {
    if constexpr (WAVES == 1) {
      wave_lds_sync();
    } else {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
    }
  }
  // a flag per wave and phase parity: call k + 2 rewrites call k's flags, and
  // call k + 1's barrier lies between that and every wave's read of them
  __device__ static bool any(int v, int phase = 0) {
    const bool mine = __ballot(v != 0) != 0;
    if constexpr (WAVES == 1) {
      wave_lds_sync();
      return mine;
    } else {
      __shared__ int flag[2][WAVES];
      if (lane_id_local() == 0) flag[phase & 1][wave_id()] = mine;
      sync();
      int r = 0;
#pragma unroll
      for (int w = 0; w < WAVES; ++w) r |= flag[phase & 1][w];
      return r != 0;
    }
  }
  __device__ static bool leader() { return tid_local() == 0; }
};
template <class G>
struct BoardsSmem {
  TreeLds<G> t;                                          // choose_action's mask and scratch
  int label[G::CELLS], libs[G::CELLS], gsize[G::CELLS];
  int8_t stone[G::CELLS];
  uint8_t invd[G::CELLS];
  int killed[4];
  int misc[8];
  int bc[8];
};

template <int N, int C, bool CAPS = false>
__global__ void __launch_bounds__((BoardsGeo<Geo<N, C>>::THREADS)) k_selfplay_boards(SearchParams sp, PlayParams pp,
                                                                                    EngineArrays E) {
  typedef Geo<N, C> G;
  typedef BoardsTeam<G> T;
  __shared__ BoardsSmem<G> sm;
  const int g = blockIdx.x;
  const int tid = tid_local();
  if (tid == 0) {
    atomicAdd(&E.counters[6], 1ull);
    E.mpq[2 * g + 1] = 0;
  }
  if (E.status[g] != 0) return;
  BoardMeta m;
  board_load<G, T>(sm.stone, sm.invd, E, g, m);
  BoardLds<G> b = make_board_lds<G>(sm.stone, sm.invd, sm.label, sm.libs, sm.gsize, sm.killed, sm.misc);
  board_groups<G, T>(b);                                 // kept from move to move (play_action's HELD)
  // MZGO_STAMPS: thread 0's cycles per phase of a move, summed over the launch's moves (slots: below)
#ifdef MZGO_STAMPS
  unsigned long long lapc[6] = {}, lapt = __builtin_amdgcn_s_memtime();
  auto lap = [&](int k) {
    const unsigned long long now = __builtin_amdgcn_s_memtime();
    lapc[k] += now - lapt;
    lapt = now;
  };
#else
  auto lap = [](int) {};
#endif
  const int mv_first = m.moves;
  int played = 0, finished = 0;
  unsigned long long sims = 0;
  const TreeView TV = TreeViewOf<G>::make(E, g);         // (compat "reference" reads no tree)
  for (int step = 0; step < pp.moves; ++step) {
    const int mv = m.moves;
    const size_t rec = (size_t)g * E.max_moves + mv;
    const uint64_t key = move_key(sp, pp, g, mv);
    const int budget = move_budget<CAPS>(sp, key);       // (k_search_queue derives the same from the same key)
    record_observation<G, T>(E, rec, sm.stone, sm.invd, m, CAPS && budget != sp.num_simulations);
    lap(0);
    ++played;
    sims += (unsigned long long)budget;
    build_mask<G, T>(sm.t, sp.pass_epsilon, [&](int a) { return sm.invd[a]; });
    lap(1);
    if (wave_id() == 0) {
      // (the host launches this schedule for search variant 0 only: choose_move_action's self_play.py arm)
      const int a = choose_action<G>(sm.t, TV, sp.compat, move_temperature(pp, mv), key, E.rec_policy + rec * G::A);
      if (lane_id_local() == 0) {
        sm.bc[0] = a;
        E.rec_action[rec] = a;
      }
    }
    T::sync();
    lap(move_temperature(pp, mv) != 0.0 ? 2 : 3);
    double w;
    const int st = play_action<G, T, true>(E, g, b, m, sm.bc[0], pp.komi, w);
    lap(4);
    finished += game_finished(E, st, m);
    if (finish_move<G, T, false>(E, budget, g, rec, st, m, w)) break;
    T::sync();                                     // this move's LDS reads before the next move's writes
    lap(5);
  }
  // the slot's board, the launch's counters and the queue's (first move, moves played): once per game
  board_store<G, T>(sm.stone, sm.invd, E, g, m);
  if (tid == 0) {
    count_moves(E, sims, played, finished);
#ifdef MZGO_STAMPS
    // 83 record, 84 legal mask, 85 / 86 action choice with / without temperature, 87 board step and
    // winner, 47 result + the move's last barrier, 45 moves
    if (E.stamps) {
      unsigned long long* row = E.stamps + (size_t)g * kStampPhases;
      row[83] += lapc[0]; row[84] += lapc[1]; row[85] += lapc[2]; row[86] += lapc[3];
      row[87] += lapc[4]; row[47] += lapc[5]; row[45] += (unsigned long long)played;
    }
#endif
    E.mpq[2 * g] = mv_first;
    E.mpq[2 * g + 1] = played;
  }
}

// ---------------------------------------------------------------------------
// The move-parallel epoch, second launch (compat "reference", SURVEY.md §0.6:
// the action is a uniform draw over the legal moves and the policy target is
// mask / sum, so a game's board sequence never reads its searches and every
// (game, move) search is independent once the boards are played).  A
// persistent grid of one workgroup per CU claims (game, move) items from one
// queue -- the moves of every game, latest first -- and runs each search in
// its own tree slot (blockIdx.x) from the recorded observation; the search's
// root value is the record's.  The same searches, keys and noise as the
// game-per-workgroup launch, so the records are identical; the epoch's tail
// (a game's whole remaining move sequence on one CU while the others idle)
// shrinks to one search.
// ---------------------------------------------------------------------------
template <int N, int C, bool CAPS = false>
__global__ void __launch_bounds__((Geo<N, C>::THREADS)) __attribute__((amdgpu_waves_per_eu(Geo<N, C>::WPE, Geo<N, C>::WPE))) k_search_queue(NetParams np_arg, SearchParams sp, PlayParams pp,
                                                            EngineArrays E_arg, int games) {
  typedef Geo<N, C> G;
  __shared__ Smem<G> sm;
  static_assert(sizeof(Smem<G>) <= 160 * 1024, "one workgroup per CU: the whole LDS at most");
  if constexpr (G::WINO) wino_raw_zero<G>(sm.raw);        // zero halo of the conv input planes
  // sp.helpers > 0 (19x19, MZGO_QUEUE_HELPERS): the first gridDim.x /
  // (1 + helpers per leader) workgroups claim searches, the others serve a
  // leader's batch expansions and parent convs as jobs (helper_loop) for the
  // whole launch, as a game's helpers do in the game-per-workgroup launch
  const int leaders = (int)gridDim.x - sp.helpers;
  if ((int)blockIdx.x >= leaders) {
    if constexpr (Smem<G>::GLOBAL_Y && G::WINO)
      helper_loop<G>(sm, np_arg, np_arg, sp, E_arg, ((int)blockIdx.x - leaders) % leaders);
    return;
  }
  const int slot = blockIdx.x;
  const int items = games * pp.moves;
  for (;;) {
    if (tid_local() == 0) sm.bc[0] = (int)atomicAdd((unsigned*)&E_arg.mpq[2 * games], 1u);
    __syncthreads();
    const int k = sm.bc[0];
    __syncthreads();                               // (sm.bc is the search's scratch too)
    if (k >= items) break;
    const int j = k / games, g = k % games;
    const int mv0 = __builtin_amdgcn_readfirstlane(E_arg.mpq[2 * g]);
    const int nmv = __builtin_amdgcn_readfirstlane(E_arg.mpq[2 * g + 1]);
    if (j >= nmv) continue;
    const int mv = mv0 + nmv - 1 - j;
    const EngineArrays E = launder_arrays(E_arg);
    const NetParams np = launder_params(np_arg);
    const size_t rec = (size_t)g * E.max_moves + mv;
    for (int c = tid_local(); c < G::CELLS; c += G::THREADS) {   // record_observation's inverse
      sm.stone[c] = E.rec_stones[rec * G::CELLS + c];
      sm.invd[c] = E.rec_invd[rec * G::CELLS + c];
    }
    const BoardMeta m0 = flags_unpack(E.rec_flags[rec], mv);
    __syncthreads();
    const uint64_t key = move_key(sp, pp, g, mv);
    const double* noise = pp.noise ? pp.noise + rec * G::A : nullptr;
    double* noise_out = pp.noise_out ? pp.noise_out + rec * G::A : nullptr;
    SearchParams spm = launder_search(sp);
    spm.net = 0;
    if constexpr (CAPS) spm.num_simulations = move_budget<CAPS>(sp, key);   // the budget k_selfplay_boards recorded
    run_search<G>(sm, np, spm, E, slot, [&](int c, int jj) { return board_plane<G>(sm.stone, sm.invd, m0, c, jj); },
                  noise, key, nullptr, noise_out);
    if (tid_local() == 0) E.rec_value[rec] = root_value(TreeViewOf<G>::make(E, slot));
    __syncthreads();                               // this search's LDS reads before the next board
  }
  if (sp.helpers > 0 && tid_local() == 0) job_exit(job_of<G>(E_arg, slot));
}

// ---------------------------------------------------------------------------
// Reanalysis (MuZero Reanalyse; no reference counterpart): search n stored
// positions -- any n, not the engine's games -- from one queue and return what
// a trainer consumes.  The schedule is k_search_queue's: a persistent grid,
// workgroup b owns tree slot b and claims the next item until the queue is
// empty.  The items are caller buffers in the record format
// (record_observation), the key of item i is (seed, ids[i][0], ids[i][1]) --
// a self-play record's own search when ids[i] = (move_key's game id, move) --
// and the outputs are indexed by item: the root's true child visit counts
// (search_outputs' rule), the root value and, when asked for, the policy
// target the engine's move rule records under compat "fixed" (visit_policy;
// main.py's rule draws no action here, so a search whose legal children have
// no visits gives an all-zero row, not choose_action_main's one-hot).  The
// engine's boards, records, mpq and job slots are neither read nor written;
// the counters run_search advances advance.
// ---------------------------------------------------------------------------
struct ReanalyseArgs {
  const int8_t* stones;    // [n][CELLS] 0 / 1 black / 2 white
  const uint8_t* invd;     // [n][CELLS]
  const uint8_t* flags;    // [n] flags_pack
  const int* ids;          // [n][2] key game id, move index
  const double* noise;     // [n][A] injected Dirichlet samples, or null
  int n;
  unsigned* head;          // the queue head (zeroed before the launch)
  int* visits;             // [n][A]
  double* value;           // [n]
  double* policy;          // [n][A], or null
};

// ---------------------------------------------------------------------------
// INPLACE (mzgo_replay_reanalyse_sample): the items are rows of the device
// replay store, ReanalyseStoreArgs (mzgo_replay.hpp).  Item i = (slot, t) of
// the list a launch before this one built, whose length is a device word: the
// grid is the host's upper bound, and a workgroup that claims i >= *n leaves.
// The position is read from the store's own rows, the key is (seed,
// key_gid[slot], t) -- mzgo_replay_reanalyse's for the same position -- and the
// policy row and root value go straight into the store's: no visits, no
// staging.  A search reads position rows and writes policy and value rows,
// never the other way round, with one exception: it clears bit 3 (kFlagFast)
// of the flags byte of the position row it read.  Bits 0-2, all a search
// reads of that byte, never change, and every writer of a row stores the same
// byte, so a row listed twice (overlapping windows) may be read by one
// workgroup while another clears its bit without either seeing a difference.
// Otherwise distinct items share nothing; the queue head stays the only word
// two workgroups contend for.
// ---------------------------------------------------------------------------
template <int N, int C, bool INPLACE = false>
__global__ void __launch_bounds__((Geo<N, C>::THREADS)) __attribute__((amdgpu_waves_per_eu(Geo<N, C>::WPE, Geo<N, C>::WPE))) k_reanalyse_queue(NetParams np_arg, SearchParams sp,
                                                               EngineArrays E_arg, typename std::conditional<INPLACE, ReanalyseStoreArgs, ReanalyseArgs>::type ra) {
  typedef Geo<N, C> G;
  __shared__ Smem<G> sm;
  static_assert(sizeof(Smem<G>) <= 160 * 1024, "one workgroup per CU: the whole LDS at most");
  if constexpr (G::WINO) wino_raw_zero<G>(sm.raw);        // zero halo of the conv input planes
  const int slot = blockIdx.x;
  if constexpr (INPLACE) {
    for (;;) {
      if (tid_local() == 0) sm.bc[0] = (int)atomicAdd(ra.head, 1u);
      __syncthreads();
      const int i = sm.bc[0];
      __syncthreads();                             // (sm.bc is the search's scratch too)
      if (i >= *launder_global(ra.n)) break;
      const EngineArrays E = launder_arrays(E_arg);
      const NetParams np = launder_params(np_arg);
      const int* it = launder_global(ra.items) + 2 * (size_t)i;
      const int rs = it[0], t = it[1];             // ring slot, move
      const size_t q = (size_t)rs * (ra.R.M + 1) + t;
      const int8_t* st = launder_global(ra.R.stones) + q * G::CELLS;
      const uint8_t* iv = launder_global(ra.R.invd) + q * G::CELLS;
      for (int c = tid_local(); c < G::CELLS; c += G::THREADS) {
        sm.stone[c] = st[c];
        sm.invd[c] = iv[c];
      }
      const BoardMeta m0 = flags_unpack(launder_global(ra.R.flags)[q], t);
      __syncthreads();
      const uint64_t key = stream_key(sp.seed, (uint32_t)launder_global(ra.R.key_gid)[rs], (uint32_t)t);
      SearchParams spm = launder_search(sp);
      spm.net = 0;
      spm.helpers = 0;
      run_search<G>(sm, np, spm, E, slot, [&](int c, int jj) { return board_plane<G>(sm.stone, sm.invd, m0, c, jj); },
                    nullptr, key);
      const TreeView T = TreeViewOf<G>::make(E, slot);
      const size_t o = (size_t)rs * ra.R.M + t;
      if (tid_local() == 0) {
        launder_global(ra.R.root_value)[o] = root_value(T);
        // the row is a full-budget search's now: no longer a fast one (a row listed twice gets the same byte twice)
        uint8_t* fl = launder_global(ra.R.flags) + q;
        if (*fl & kFlagFast) *fl = (uint8_t)(*fl & ~kFlagFast);
      }
      if (wave_id() == 0) {
        double vc[G::AP], msum;
        visit_policy<G>(sm.t, T, sp.variant, 1, launder_global(ra.R.policy) + o * G::A, vc, msum);
      }
      __syncthreads();                             // this search's LDS reads before the next board
    }
  } else
  for (;;) {
    if (tid_local() == 0) sm.bc[0] = (int)atomicAdd(ra.head, 1u);
    __syncthreads();
    const int i = sm.bc[0];
    __syncthreads();                               // (sm.bc is the search's scratch too)
    if (i >= ra.n) break;
    // (as k_search_queue: this item's view of the arguments, no address
    // arithmetic kept live across the searches)
    const EngineArrays E = launder_arrays(E_arg);
    const NetParams np = launder_params(np_arg);
    const int8_t* st = launder_global(ra.stones) + (size_t)i * G::CELLS;
    const uint8_t* iv = launder_global(ra.invd) + (size_t)i * G::CELLS;
    for (int c = tid_local(); c < G::CELLS; c += G::THREADS) {   // record_observation's inverse
      sm.stone[c] = st[c];
      sm.invd[c] = iv[c];
    }
    const int* id = launder_global(ra.ids) + 2 * (size_t)i;
    const BoardMeta m0 = flags_unpack(launder_global(ra.flags)[i], id[1]);
    __syncthreads();
    const uint64_t key = stream_key(sp.seed, (uint32_t)id[0], (uint32_t)id[1]);
    const double* noise = ra.noise ? launder_global(ra.noise) + (size_t)i * G::A : nullptr;
    SearchParams spm = launder_search(sp);
    spm.net = 0;
    spm.helpers = 0;
    run_search<G>(sm, np, spm, E, slot, [&](int c, int jj) { return board_plane<G>(sm.stone, sm.invd, m0, c, jj); },
                  noise, key);
    const TreeView T = TreeViewOf<G>::make(E, slot);
    int* ov = launder_global(ra.visits) + (size_t)i * G::A;
    for (int a = tid_local(); a < G::A; a += G::THREADS) {
      const int c = T.child[a];
      ov[a] = c >= 0 ? T.visits[c] : 0;
    }
    if (tid_local() == 0) launder_global(ra.value)[i] = root_value(T);
    if (ra.policy && wave_id() == 0) {
      double vc[G::AP], msum;
      visit_policy<G>(sm.t, T, sp.variant, 1, launder_global(ra.policy) + (size_t)i * G::A, vc, msum);
    }
    __syncthreads();                               // this search's LDS reads before the next board
  }
}

// ---------------------------------------------------------------------------
// Continuous self-play (mzgo_replay_play_games): any n games on the engine's
// G slots from one queue, finished games going straight into the replay
// store.  The schedule is k_search_queue's with whole games as the items: a
// persistent grid of min(n, G, CUs) workgroups, workgroup b owning slot b --
// tree, board and record rows -- for the whole launch and claiming the next
// game, in index order, when its own ends; the launch's tail (the last games
// running while other CUs idle) is paid once per call, not once per G games.
//
// Queue game j IS slot j % G of epoch epoch0 + j / G: its key id is
// game_key_id(game_base, j % G, epoch0 + j / G), so its moves, searches and
// record are those of ceil(n / G) epochs of reset + whole-game launch +
// ingest, whichever workgroup plays it.  The slot that stores it (b) is not
// its identity (selfplay_one_move).  Its ring slot, (first + j) % cap, is
// fixed by j as well: the store's order does not depend on who finished first.
//
// No helper workgroups, no tail phase (sp.helpers = sp.tail = 0: 19x19 runs
// its batch expansions on the game's own workgroup, as k_reanalyse_queue), one
// network (pp.arena = 0), no noise hooks (they index by slot).  Workgroups
// share one word, the queue head.  The ingest reads what this workgroup's own
// threads stored, so the barrier before it (workgroup scope) is all it needs.
// ---------------------------------------------------------------------------
template <int N, int C, bool CAPS = false>
__global__ void __launch_bounds__((Geo<N, C>::THREADS)) __attribute__((amdgpu_waves_per_eu(Geo<N, C>::WPE, Geo<N, C>::WPE))) k_selfplay_games(NetParams np_arg, SearchParams sp, PlayParams pp,
                                                              EngineArrays E_arg, GamesArgs ga) {
  typedef Geo<N, C> G;
  __shared__ Smem<G> sm;
  static_assert(sizeof(Smem<G>) <= 160 * 1024, "one workgroup per CU: the whole LDS at most");
  if constexpr (G::WINO) wino_raw_zero<G>(sm.raw);        // zero halo of the conv input planes
  const int slot = blockIdx.x;
  if (tid_local() == 0) atomicAdd(&E_arg.counters[6], 1ull);
  for (;;) {
    if (tid_local() == 0) sm.bc[0] = (int)atomicAdd(ga.head, 1u);
    __syncthreads();
    const int j = __builtin_amdgcn_readfirstlane(sm.bc[0]);
    __syncthreads();                               // (sm.bc is the search's scratch too)
    if (j >= ga.n) break;
    const uint32_t kid = game_key_id(pp.game_base, j % ga.G, ga.epoch0 + j / ga.G);
    // a new game in the slot: k_board_reset's state, and its board in LDS
    board_reset_slot<G>(E_arg, slot);
    for (int c = tid_local(); c < G::CELLS; c += G::THREADS) {
      sm.stone[c] = 0;
      sm.invd[c] = 0;
    }
    BoardMeta m{0, 0, 0, 0};
    __syncthreads();
    for (int step = 0; step < pp.moves; ++step) {
      if (selfplay_one_move<G, CAPS>(sm, np_arg, np_arg, sp, pp, E_arg, slot, [&]() { return kid; }, m)) break;
      __syncthreads();                             // this move's LDS reads before the next move's writes
    }
    __syncthreads();                               // the game's record and board: every thread's stores
    // (tid 0 is finish_move's leader: it reads its own store)
    if (tid_local() == 0 && E_arg.status[slot] >= 16) atomicMin(ga.error, j);
    const ReplayEngineView V{N, ga.G, E_arg.max_moves, C, 0, pp.game_base, 0,
                             E_arg.stones, E_arg.invd, E_arg.meta, E_arg.rec_stones, E_arg.rec_invd,
                             E_arg.rec_flags, E_arg.rec_action, E_arg.rec_value, E_arg.rec_policy,
                             E_arg.rec_reward, E_arg.final_reward};
    replay_ingest_game(ga.R, V, slot, (ga.first + j) % ga.R.cap, (int)kid, tid_local(), G::THREADS);
    __syncthreads();                               // the ingest's reads before the next game's records
  }
}

}  // namespace mzgo
