// mzgo_jobs.hpp -- the job protocol: how a game's workgroup shares work with
// helper workgroups.  One definition of a job's memory (JobHeader + four
// regions sized by A), of what a job says (JobKind, JobInfo) and of the five
// steps: the game posts (job_post), every workgroup claims units (job_claim)
// and computes its share (one function per kind, called by the game's
// workgroup and by helpers alike), helpers hand their units in (job_done) and
// wait for the next job (job_next), the game waits for all units (job_wait).
#pragma once
#include <cstddef>

#include "mzgo_smem.hpp"

namespace mzgo {

// ---------------------------------------------------------------------------
// Batch expansions shared with helper workgroups (GLOBAL_Y boards, 19x19).
// A 19x19 game has one workgroup, so with 64 games 192 CUs would idle; the
// self-play launch adds sp.helpers workgroups (3 per game), and a game's
// batch expansion (up to A children, each an L2 stream of its leaf's Y)
// becomes a job that its workgroup and its helpers share: the game's
// workgroup publishes the job (the actions, the leaf, the children's node
// ids), every workgroup claims children a round of WAVES at a time, computes
// them exactly as batch_expand does (the same function per child) and writes
// the rows and backup values to HBM; the game's workgroup waits until all B
// are done, then continues.  It never waits for a helper to START (it claims
// children itself until none are left), so nothing depends on helpers being
// resident.  Hand-offs: agent-scope release / relaxed flag / agent-scope
// acquire (cdna_hip_programming.md Guideline 16); claims: a CAS on one
// 64-bit word (batch number << 32 | next child), so a claim of a finished
// batch fails.
// ---------------------------------------------------------------------------
enum JobKind : int {
  kJobBatch = 0,         // the children of a batch expansion (job_rounds)
  kJobConvSrc = 1,       // a parent's conv, its latent in the scratch slot (the root)
  kJobConvRebuilt = 2,   // a parent's conv, its latent rebuilt from its own parent's Y
  kJobReplay = 3,        // a batch's replay checks, in groups of levels (verify_batch)
  kJobRepConv2 = 4,      // the representation's conv2
  kJobRepConv3 = 5,      // the representation's conv3
  kJobTailConv = 6,      // a parent's conv in units of cout tiles (the 9x9 epoch tail)
};

// What a job says.  The game's thread 0 writes it whole before the publish;
// helpers read it with plain loads after their acquire (see job_post for why
// a stale read is harmless).
struct JobInfo {
  int units;             // what there is to claim: children, strips, groups or tail units
  int node;              // a batch: its first child's node id; a conv: the leaf's parent (-1: none)
  int leaf;              // the node whose children / whose Y the job computes
  int net;               // the network (arena: 1 = "best"); kJobReplay: levels per group (group())
  int kind;              // JobKind
  int act;               // a conv: the action that led to the leaf; kJobReplay: the root action
  int depth;             // kJobReplay: the leaf's depth
  int batch;             // kJobReplay: the batch's size
  __device__ int group() const { return net; }
};
static_assert(sizeof(JobInfo) == 32, "eight ints");
__device__ __forceinline__ JobInfo job_info(JobKind kind, int units, int node, int leaf, int net_or_group,
                                            int act = 0, int depth = 0, int batch = 0) {
  return JobInfo{units, node, leaf, net_or_group, kind, act, depth, batch};
}

// A job slot's fixed part.  claim, seq, done, started and nhelp are polled or
// CASed by other workgroups: each sits alone on its 64-byte line.
struct JobHeader {
  alignas(64) unsigned long long claim;    // batch number << 32 | total << 16 | next unit (job_post)
  alignas(64) unsigned seq;                // the published batch number; kJobExit once the game is through
  alignas(64) unsigned done;               // units handed in
  alignas(64) JobInfo info;
  double pass_prior;                       // the root's (child_priors reads it)
  // replay checks: the failing simulations found by every workgroup (bit i)
  alignas(64) unsigned long long failm[16];
  // 1 once the game's workgroup runs (zeroed by the host before the launch):
  // tail helpers join only started games -- one not yet dispatched may be
  // waiting for the very CU a helper holds
  alignas(64) unsigned started;
  // helpers of ended games registered with this game (tail_help, join_running_game)
  alignas(64) unsigned nhelp;
};
static_assert(sizeof(JobHeader) == 512 && offsetof(JobHeader, seq) == 64 && offsetof(JobHeader, done) == 128 &&
                  offsetof(JobHeader, info) == 192 && offsetof(JobHeader, pass_prior) == 224 &&
                  offsetof(JobHeader, failm) == 256 && offsetof(JobHeader, started) == 384 && offsetof(JobHeader, nhelp) == 448,
              "the job slot's fixed layout");

// The four regions after the header, each rounded to 256 bytes:
//   acts   u64[A]       the actions, tagged: batch number << 32 | action (an entry is valid for
//                       the batch whose number it carries: no separate progress counter)
//   bv     f64[A]       the children's backup values
//   valid  u8[A]        the root's valid mask (child_priors reads it)
//   hfin   f32[3][CS]   representation conv3: the head sums per cell of every strip
__host__ __device__ constexpr int job_round(int bytes) { return (bytes + 255) / 256 * 256; }
__host__ __device__ constexpr int job_bv_at(int A) { return (int)sizeof(JobHeader) + job_round(A * 8); }
__host__ __device__ constexpr int job_valid_at(int A) { return job_bv_at(A) + job_round(A * 8); }
__host__ __device__ constexpr int job_hfin_at(int A) { return job_valid_at(A) + job_round(A); }
__host__ __device__ constexpr int job_bytes(int A) { return job_hfin_at(A) + job_round((A - 1 + 15) / 16 * 16 * 12); }
// (the boards instantiated: the bytes the host has allocated and zeroed per slot since the jobs exist)
static_assert(job_bytes(26) == 1792 && job_bytes(37) == 2560 && job_bytes(82) == 3584 && job_bytes(362) == 11776 &&
              job_valid_at(362) == 512 + 2 * 3072 && job_hfin_at(362) + 3 * 368 * 4 <= job_bytes(362));

// seq once the game is through; job_next's answer when its bounded wait ran out (0 is never a batch number)
constexpr unsigned kJobExit = 0xFFFFFFFFu, kJobExpired = 0;
// s_sleep units (64 clocks) between polls: a game waiting for its job's units,
// a helper waiting for the next job ((1, 2) measured the same)
constexpr int kJobWaitSleep = 4, kJobPollSleep = 8;

struct JobView {
  JobHeader* h;
  __device__ uint8_t* at(int off) const { return reinterpret_cast<uint8_t*>(h) + off; }
  __device__ unsigned long long* acts() const { return reinterpret_cast<unsigned long long*>(at(sizeof(JobHeader))); }
  __device__ double* bv(int A) const { return reinterpret_cast<double*>(at(job_bv_at(A))); }
  __device__ uint8_t* valid(int A) const { return at(job_valid_at(A)); }
  __device__ float* hfin(int A) const { return reinterpret_cast<float*>(at(job_hfin_at(A))); }
};
template <class G>
__device__ __forceinline__ JobView job_of(const EngineArrays& E, int g) {
  static_assert(G::AP <= 16, "JobHeader::failm holds a word per 64 actions");
  return JobView{reinterpret_cast<JobHeader*>(E.jobs + (size_t)g * job_bytes(G::A))};
}

// the parent convs and batch expansions go through jobs: 19x19 (Y streamed
// from L2, strip convs) with helper workgroups in the launch
template <class G>
__device__ __forceinline__ bool shared_jobs(const SearchParams& sp) {
  if constexpr (Smem<G>::GLOBAL_Y && G::WINO) return Wino<G>::NSTRIP > 1 && sp.helpers > 0;
  else return false;
}

// ---------------------------------------------------------------------------
// The steps.
// ---------------------------------------------------------------------------
// A job's batch number (unique within a launch: the host zeroes the jobs
// before it) with the claim word and the done counter reset for it.
//
// The claim word is batch << 32 | total << 16 | next: a claim is decided by
// the word alone, never by the job's info block.  A helper that acquired
// batch s can read info rows the game's workgroup is already rewriting for
// s + 1 (the game claims every unit of s itself when no helper comes, waits
// for them and begins s + 1 at once); its CAS on the word of s then fails
// whatever total that info says, because s's word is exhausted (next >=
// total) before the game can begin s + 1, and the new word carries s + 1.
// A successful claim of s therefore means s is still open, so every info
// row the helper read belongs to s, and no stale done add can reach s + 1.
//
// Then the info (thread 0), whatever else the kind puts into the slot
// (fill(bseq), all threads), every store of the workgroup drained, and
// (release) the batch number.  Units from `first` on are open.  Returns the
// batch number.  All threads.
struct NoExtra {
  __device__ void operator()(unsigned) const {}
};
template <class Fill = NoExtra>
__device__ __forceinline__ unsigned job_post(const JobView& J, const JobInfo& I, unsigned first = 0,
                                             Fill fill = Fill{}) {
  const unsigned bseq = __hip_atomic_load(&J.h->seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1;
  if (tid_local() == 0) {
    __hip_atomic_store(&J.h->done, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&J.h->claim, (unsigned long long)bseq << 32 | (unsigned)I.units << 16 | first,
                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    JobInfo* o = &J.h->info;                           // (field by field: I stays in registers)
    o->units = I.units; o->node = I.node; o->leaf = I.leaf; o->net = I.net; o->kind = I.kind; o->act = I.act;
    if (I.kind == kJobReplay) { o->depth = I.depth; o->batch = I.batch; }   // (no other kind reads them)
  }
  fill(bseq);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid_local() == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // (ROCm 7.2 may drop the fence's own wait)
    __hip_atomic_store(&J.h->seq, bseq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  return bseq;
}
// this workgroup's `mine` units added; wait until all `total` are done
// (every helper adds after its release), then acquire.  All threads.
__device__ __forceinline__ void job_wait(const JobView& J, int mine, int total) {
  if (tid_local() == 0) {
    unsigned d = __hip_atomic_fetch_add(&J.h->done, (unsigned)mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + mine;
    while (d < (unsigned)total) {
      __builtin_amdgcn_s_sleep(kJobWaitSleep);
      d = __hip_atomic_load(&J.h->done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  __syncthreads();
}
// claim the next unit of batch bseq (of total): -1 when none is left.  Thread 0
// claims, the workgroup gets it through LDS.  All threads.
template <class G>
__device__ __forceinline__ int job_claim(Smem<G>& sm, const JobView& J, unsigned bseq, int total, int step) {
  if (tid_local() == 0) {
    int c0 = -1;
    unsigned long long c = __hip_atomic_load(&J.h->claim, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (;;) {                                       // (a failed CAS means another claim succeeded)
      // (the word's own total decides: see job_post; `total` is the caller's copy)
      if ((unsigned)(c >> 32) != bseq || (int)(c & 0xFFFFu) >= (int)((c >> 16) & 0xFFFFu)) break;
      if (__hip_atomic_compare_exchange_strong(&J.h->claim, &c, c + step, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_AGENT)) {
        c0 = (int)(c & 0xFFFFu);
        break;
      }
    }
    sm.bc[1] = c0;
  }
  __syncthreads();
  const int c0 = sm.bc[1];
  __syncthreads();                                   // (bc[1] is rewritten by the next claim)
  return c0;
}
// A helper hands in its `mine` units: every store of the workgroup drained,
// then (release) the done count.  All threads.
__device__ __forceinline__ void job_done(const JobView& J, int mine) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid_local() == 0 && mine > 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // (ROCm 7.2 may drop the fence's own wait)
    __hip_atomic_fetch_add(&J.h->done, (unsigned)mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}
// A helper waits for the batch after `last`: returns its number (acquired),
// kJobExit, or kJobExpired when none came within spin_max polls.  Thread 0
// polls, the workgroup gets the answer through LDS (bc[2]: the caller has a
// barrier before the next call).  All threads.
template <class G>
__device__ __forceinline__ unsigned job_next(Smem<G>& sm, const JobView& J, unsigned last, long long spin_max) {
  if (tid_local() == 0) {
    unsigned s = __hip_atomic_load(&J.h->seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (long long spins = 0; (s == last || s == 0) && spins < spin_max; ++spins) {
      __builtin_amdgcn_s_sleep(kJobPollSleep);
      s = __hip_atomic_load(&J.h->seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (s == last || s == 0) s = kJobExpired;
    else if (s != kJobExit) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    sm.bc[2] = (int)s;
  }
  __syncthreads();
  return (unsigned)sm.bc[2];
}
// The game's workgroup runs / is through with its moves.  Thread 0.
__device__ __forceinline__ void job_mark_started(const JobView& J) {
  __hip_atomic_store(&J.h->started, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void job_exit(const JobView& J) {
  __hip_atomic_store(&J.h->seq, kJobExit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// a game that helpers of ended games may join: its workgroup runs and is not through
__device__ __forceinline__ bool job_running(const JobView& J) {
  return __hip_atomic_load(&J.h->started, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0 &&
         __hip_atomic_load(&J.h->seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != kJobExit;
}

// ---------------------------------------------------------------------------
// A workgroup's share of job (I, bseq) of game g, one function per kind: the
// game's workgroup and its helpers call the same one with the same
// arguments, so what a job reads and writes is derived from its JobInfo once.
// Each claims units until none is left and returns its count.  All threads.
// ---------------------------------------------------------------------------
// kJobConvSrc / kJobConvRebuilt: the dynamics conv of node I.leaf (19x19: 5
// row strips, each independent given the input): its input -- the latent in
// the scratch slot or, rebuilt, the latent formed from parent I.node's Y and
// action I.act's E rows (wino_input_rebuilt: no materialized copy) -- -> its
// Y ([CELLS][C], its pool slot); strips claimed one at a time.
template <class G>
__device__ __forceinline__ int conv_share(Smem<G>& sm, const NetParams& np, const EngineArrays& E, int g,
                                          const JobView& J, const JobInfo& I, unsigned bseq) {
  int mine = 0;
  if constexpr (G::WINO) {
    float* pool = pool_of<G>(E, g);
    float* dst = pool + (size_t)I.leaf * G::C * G::CS;
    const float* ypar = I.kind == kJobConvRebuilt ? pool + (size_t)I.node * G::C * G::CS : nullptr;
    for (int s; (s = job_claim(sm, J, bseq, Wino<G>::NSTRIP, 1)) >= 0; ++mine) {
      if (ypar) {
        // (the second channel slab transformed under the GEMM's first K half)
        wino_conv_rebuilt<G>(sm.u.v, sm.raw, sm.u.x.red, sm.u.x.hp, sm.u.x.outs, sm.hfin, ypar,
                             np.etab + (size_t)I.act * 9 * G::C, np.w_dyn, np.b_dyn, dst, nullptr, nullptr, nullptr, s);
      } else {
        wino_input<G, G::C>(sm.u.v, sm.raw, pool + (size_t)(E.S + 1) * G::C * G::CS, G::CS, nullptr, s);
        wino_conv<G, G::C, G::C, 0, true>(sm.u.v, sm.u.x.red, sm.u.x.hp, sm.u.x.outs, sm.hfin, np.w_dyn, np.b_dyn,
                                           dst, G::CS, G::CS, nullptr, s);
      }
    }
  }
  __syncthreads();
  return mine;
}

// kJobRepConv2 / kJobRepConv3: the representation's conv2 (64 -> 64, the
// scratch slot -> node 0's slot) and conv3 (64 -> C, back; value and policy
// head sums per cell into J.hfin) of a 19x19 root, in strips.
template <class G, int CIN, int COUT, int NH>
__device__ __forceinline__ int rep_strips(Smem<G>& sm, const JobView& J, unsigned bseq, const float* w,
                                          const float* b, const float* src, float* dst, const float* head_w,
                                          float* hfin) {
  int mine = 0;
  if constexpr (G::WINO) {
    for (int s; (s = job_claim(sm, J, bseq, Wino<G>::NSTRIP, 1)) >= 0; ++mine) {
      wino_input<G, CIN>(sm.u.v, sm.raw, src, G::CS, nullptr, s);
      wino_conv<G, CIN, COUT, NH>(sm.u.v, sm.u.x.red, sm.u.x.hp, sm.u.x.outs, hfin, w, b, dst, G::CS, G::CS,
                                  head_w, s);
    }
  }
  __syncthreads();
  return mine;
}
template <class G>
__device__ __forceinline__ int rep_share(Smem<G>& sm, const NetParams& np, const EngineArrays& E, int g,
                                         const JobView& J, const JobInfo& I, unsigned bseq) {
  float* pool = pool_of<G>(E, g);
  float* lat = pool + (size_t)(E.S + 1) * G::C * G::CS;
  return I.kind == kJobRepConv2
             ? rep_strips<G, 64, 64, 0>(sm, J, bseq, np.w_conv2, np.b_conv2, lat, pool, nullptr, sm.hfin)
             : rep_strips<G, 64, G::C, 2>(sm, J, bseq, np.w_conv3, np.b_conv3, pool, lat, np.head_w + G::C,
                                          J.hfin(G::A));
}

// kJobBatch and kJobReplay run the search's own code (expand_child,
// verify_levels): their shares are defined with it, in mzgo_kernels.hpp.
// job_rounds: the children of a batch; replay_help: a helper's groups of a
// batch's replay checks.
template <class G, bool LAZY, bool LAZYH = false>
__device__ __forceinline__ int job_rounds(Smem<G>& sm, const NetParams& np, const SearchParams& sp,
                                          const TreeView& TV, const float* yg, const JobView& J, unsigned bseq,
                                          int B, int nid0, bool helper = false, Stamp* st = nullptr);
template <class G>
__device__ __forceinline__ int replay_help(Smem<G>& sm, const SearchParams& sp, const EngineArrays& E, int g,
                                           const TreeView& TV, const JobView& J, const JobInfo& I, unsigned bseq);

// ---------------------------------------------------------------------------
// The game's workgroup: a conv as a job.
// ---------------------------------------------------------------------------
// The conv of node `leaf` (dst = its pool slot).  Input: the scratch slot
// (par < 0) or the latent rebuilt from parent par's Y and action act's E
// rows.  All threads; returns synchronised with dst complete and acquired.
// pre(bseq): work of the game's workgroup between the publish and its
// first strip claim (the next batch's picks: pick_all, wave 0), while the
// helpers start on the strips.
template <class G, class Pre = NoExtra>
__device__ __forceinline__ void conv_shared(Smem<G>& sm, const NetParams& np, const EngineArrays& E, int g,
                                            int leaf, int net, Stamp* st = nullptr, int par = -1, int act = 0,
                                            Pre pre = Pre{}) {
  const JobView J = job_of<G>(E, g);
  const JobInfo I = job_info(par >= 0 ? kJobConvRebuilt : kJobConvSrc, Wino<G>::NSTRIP, par, leaf, net, act);
  const unsigned bseq = job_post(J, I);              // (src / the parent's Y reach the helpers)
  pre(bseq);
  if (st) st->lap(52);
  const int mine = conv_share<G>(sm, np, E, g, J, I, bseq);
  if (st) st->lap(53);
  job_wait(J, mine, I.units);
  if (st) st->lap(54);
}

// The game's workgroup: representation conv k (2 or 3) over the job
// machinery; conv3's head sums come back into sm.hfin.  All threads;
// returns synchronised.
template <class G>
__device__ __forceinline__ void rep_shared(Smem<G>& sm, const NetParams& np, const EngineArrays& E, int g, int net,
                                           int k) {
  if constexpr (G::WINO && Wino<G>::NSTRIP > 1) {
    const JobView J = job_of<G>(E, g);
    const JobInfo I = job_info(k == 2 ? kJobRepConv2 : kJobRepConv3, Wino<G>::NSTRIP, 0, 0, net);
    const unsigned bseq = job_post(J, I);            // (conv k's input reaches the helpers)
    const int mine = rep_share<G>(sm, np, E, g, J, I, bseq);
    job_wait(J, mine, I.units);
    if (k == 3)
      for (int i = tid_local(); i < 2 * G::CS; i += G::THREADS) sm.hfin[i] = J.hfin(G::A)[i];
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------
// The epoch tail at 9x9 (one-strip Winograd boards, the tree in LDS): in a
// whole-game launch the games end at different moves, and the last ones
// finish alone on their CUs (~29 % of an epoch's CU-time idle).  A workgroup
// whose game has ended registers (JobHeader::nhelp) with a running game that
// has fewer than kTailHelpers helpers and serves its parent convs: a game
// that sees a helper registered publishes its next parent conv as a job of
// kTailUnits units -- unit u = cout tiles 2u, 2u + 1 (wino_conv's m0 / nm) --
// claims units itself too (it never waits for a helper to start), waits for
// all, and loads the whole Y from L2 into its LDS copy.  Every workgroup
// computes the full Winograd input (from the parent's Y in the pool; the
// second slab under its first unit's GEMM, wino_conv_rebuilt) once per job and
// each unit's tiles' GEMM + epilogue exactly as the whole conv does,
// so the records do not depend on who computed what (MZGO_TAIL_HELPERS=0 A/B).
// Hand-offs: the job machinery above (release / relaxed flag / acquire).
// ---------------------------------------------------------------------------
constexpr int kTailUnits = 3;           // (granularity measured)
constexpr unsigned kTailHelpers = 2;
constexpr int kTailTiles = 6 / kTailUnits;     // cout tiles per unit

template <class G>
struct TailConvs {
  static constexpr bool value = [] {
    if constexpr (G::WINO) return Wino<G>::NSTRIP == 1 && !Smem<G>::GLOBAL_Y && G::C == 6 * 16;
    else return false;
  }();
};

// kJobTailConv: V from parent I.node's Y (ylds_par: the game's LDS copy of
// it) once, then each claimed unit's two cout tiles of node I.leaf's Y (red
// in the raw planes: the caller restores their zero halo after a barrier).
template <class G>
__device__ __forceinline__ int tail_share(Smem<G>& sm, const NetParams& np, const EngineArrays& E, int g,
                                          const JobView& J, const JobInfo& I, unsigned bseq,
                                          const float* ylds_par = nullptr) {
  int mine = 0;
  if constexpr (TailConvs<G>::value) {
    float* pool = pool_of<G>(E, g);
    float* dst = pool + (size_t)I.leaf * G::C * G::CS;
    for (int u; (u = job_claim(sm, J, bseq, kTailUnits, 1)) >= 0; ++mine) {
      if (mine == 0)   // (the second slab transformed under the first unit's GEMM, by every wave)
        wino_conv_rebuilt<G>(sm.u.v, sm.raw, sm.raw, sm.u.x.hp, sm.u.x.outs, sm.hfin, pool + (size_t)I.node * G::C * G::CS,
                             np.etab + (size_t)I.act * 9 * G::C, np.w_dyn, np.b_dyn, dst, nullptr, nullptr, ylds_par, 0,
                             kTailTiles * u, kTailTiles);
      else
        wino_conv<G, G::C, G::C, 0, true>(sm.u.v, sm.raw, sm.u.x.hp, sm.u.x.outs, sm.hfin, np.w_dyn, np.b_dyn, dst,
                                          G::CS, G::CS, nullptr, 0, nullptr, nullptr, kTailTiles * u, kTailTiles);
    }
  }
  return mine;
}

// The game's workgroup: the parent conv of node `leaf` (its latent rebuilt
// from parent par's Y and action act's E rows) as a tail job; returns with
// Y in the pool slot and, when ylds, in the expansion's LDS copy.  All threads.
template <class G>
__device__ __forceinline__ void conv_tail(Smem<G>& sm, const NetParams& np, const EngineArrays& E, int g, int leaf,
                                          int par, int act, int net, float* ylds, bool par_in_lds,
                                          Stamp* st = nullptr) {
  if constexpr (TailConvs<G>::value) {
    const JobView J = job_of<G>(E, g);
    const JobInfo I = job_info(kJobTailConv, kTailUnits, par, leaf, net, act);
    const unsigned bseq = job_post(J, I);            // (the parent's Y in the pool reaches the helpers)
    if (st) st->lap(52);
    const int mine = tail_share<G>(sm, np, E, g, J, I, bseq, par_in_lds ? ylds : nullptr);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this workgroup's Y stores done
    __syncthreads();
    if (mine > 0) wino_raw_zero<G>(sm.raw);
    if (st) st->lap(53);
    job_wait(J, mine, I.units);
    if (st) st->lap(54);
    if (tid_local() == 0) atomicAdd(&E.counters[4], 1ull);
    if (ylds) {
      const f32x4* src = reinterpret_cast<const f32x4*>(pool_of<G>(E, g) + (size_t)leaf * G::C * G::CS);
      f32x4* d = reinterpret_cast<f32x4*>(ylds);
      for (int i = tid_local(); i < G::CELLS * G::C / 4; i += G::THREADS) d[i] = src[i];
    }
    __syncthreads();
  }
}

// A workgroup whose game has ended: serve running games' tail conv jobs until
// none is left to register with.  All threads.
template <class G>
__device__ __forceinline__ void tail_help(Smem<G>& sm, const NetParams& np_a, const NetParams& np_b,
                                          const EngineArrays& E, int self, int games) {
  if constexpr (TailConvs<G>::value) {
    wino_raw_zero<G>(sm.raw);                          // (an ended slot's workgroup never zeroed its planes)
    for (;;) {
      // a running game with fewer than kTailHelpers helpers, the nearest after this one
      if (tid_local() == 0) {
        int pick = -1;
        for (int k = 1; k < games && pick < 0; ++k) {
          const int t = (self + k) % games;
          const JobView Jt = job_of<G>(E, t);
          if (!job_running(Jt)) continue;
          unsigned c = __hip_atomic_load(&Jt.h->nhelp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          while (c < kTailHelpers &&
                 !__hip_atomic_compare_exchange_strong(&Jt.h->nhelp, &c, c + 1, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                       __HIP_MEMORY_SCOPE_AGENT)) {
          }
          if (c < kTailHelpers) pick = t;
        }
        sm.bc[2] = pick;
      }
      __syncthreads();
      const int t = sm.bc[2];
      __syncthreads();
      if (t < 0) return;
      const JobView J = job_of<G>(E, t);
      unsigned last = 0;
      for (;;) {
        const unsigned s = job_next(sm, J, last, 1ll << 24);
        __syncthreads();                               // (bc[2] is rewritten by the next wait)
        if (s == kJobExpired) {                        // (leave, and exit -- no re-registering)
          if (tid_local() == 0) {
            __hip_atomic_fetch_sub(&J.h->nhelp, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            atomicAdd(&E.counters[7], 1ull);           // (counted: bench lines report expiries)
          }
          return;
        }
        if (s == kJobExit) break;
        last = s;
        const JobInfo I = J.h->info;
        if (I.kind != kJobTailConv) continue;
        const NetParams np = select_params(I.net != 0, np_b, np_a);
#ifdef MZGO_STAMPS
        const unsigned long long tu = __builtin_amdgcn_s_memtime();
#endif
        const int mine = tail_share<G>(sm, np, E, t, J, I, s);
#ifdef MZGO_STAMPS
        // slots 44-46: a helper's cycles computing tail units, units, jobs served
        if (tid_local() == 0 && E.stamps) {
          unsigned long long* sl = E.stamps + (size_t)blockIdx.x * kStampPhases;
          sl[44] += __builtin_amdgcn_s_memtime() - tu;
          sl[45] += (unsigned long long)mine;
          sl[46] += mine > 0 ? 1ull : 0ull;
        }
#endif
        job_done(J, mine);
        if (mine > 0) wino_raw_zero<G>(sm.raw);
      }
    }
  }
}

// ---------------------------------------------------------------------------
// Helper workgroups (19x19).
// ---------------------------------------------------------------------------
// A helper workgroup of game g (k_selfplay_move's blocks past the games):
// jobs until the game's workgroup posts kJobExit (or none comes for ~seconds):
// batch expansions, parent convs, representation convs and replay checks.
template <class G>
__device__ __forceinline__ void helper_loop(Smem<G>& sm, const NetParams& np_a, const NetParams& np_b,
                                            const SearchParams& sp, const EngineArrays& E, int g) {
  const JobView J = job_of<G>(E, g);
  const TreeView TV = TreeViewOf<G>::make(E, g);
  unsigned last = 0;
  for (;;) {
    const unsigned s = job_next(sm, J, last, 1ll << 26);
    if (s == kJobExit || s == kJobExpired) return;     // (bounded wait: give up)
    last = s;
    const JobInfo I = J.h->info;
    const NetParams np = select_params(I.net != 0, np_b, np_a);
    int mine = 0;
    switch (I.kind) {
      case kJobBatch:
        for (int a = tid_local(); a < G::A; a += G::THREADS) sm.t.valid[a] = J.valid(G::A)[a];
        if (tid_local() == 0) sm.t.pass_prior = J.h->pass_prior;
        stage_head_scalars(np.hs, sm.t.hsc);
        load_y<G>(sm, nullptr, np.head_w);             // (GLOBAL_Y: the head weights only)
        __syncthreads();
        mine = job_rounds<G, false, true>(sm, np, sp, TV, pool_of<G>(E, g) + (size_t)I.leaf * G::C * G::CS, J, s,
                                          I.units, I.node, true);
        break;
      case kJobConvSrc: case kJobConvRebuilt: mine = conv_share<G>(sm, np, E, g, J, I, s); break;
      case kJobReplay: mine = replay_help<G>(sm, sp, E, g, TV, J, I, s); break;
      case kJobRepConv2: case kJobRepConv3: mine = rep_share<G>(sm, np, E, g, J, I, s); break;
      // (kJobTailConv: one-strip boards only, tail_help)
    }
    job_done(J, mine);                                 // (every wave's row, value and Y stores)
  }
}

// 19x19 epoch tail (sp.tail, whole-game launches): a helper workgroup whose
// game has ended -- and the game's own workgroup -- move on to the running
// game with the fewest re-assigned helpers (JobHeader::nhelp; the nearest after
// `hint` among ties) and serve its jobs.  Every job kind takes any number of
// workgroups (claims are dynamic), so this changes who computes, not what.
// Returns the game or -1 when none is running.  All threads.
template <class G>
__device__ __forceinline__ int join_running_game(Smem<G>& sm, const EngineArrays& E, int games, int hint) {
  if (wave_id() == 0) {
    const int lane = lane_id_local();
    unsigned best = 0xFFFFFFFFu;
    int pick = -1;
    for (int k0 = 1; k0 <= games; k0 += 64) {
      const int k = k0 + lane;
      const int t = (hint + k) % games;
      unsigned key = 0xFFFFFFFFu;
      if (k <= games) {
        const JobView Jt = job_of<G>(E, t);
        if (job_running(Jt)) key = __hip_atomic_load(&Jt.h->nhelp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      // (helpers, distance) lexicographic: the fewest helpers, then the nearest
      unsigned long long v = (unsigned long long)key << 32 | (unsigned)k;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long w = __shfl_xor(v, o);
        v = w < v ? w : v;
      }
      if ((unsigned)(v >> 32) < best) { best = (unsigned)(v >> 32); pick = (hint + (int)(v & 0xFFFFFFFFu)) % games; }
    }
    if (lane == 0) {
      if (pick >= 0) __hip_atomic_fetch_add(&job_of<G>(E, pick).h->nhelp, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      sm.bc[2] = pick;
    }
  }
  __syncthreads();
  const int t = sm.bc[2];
  __syncthreads();
  return t;
}

}  // namespace mzgo
