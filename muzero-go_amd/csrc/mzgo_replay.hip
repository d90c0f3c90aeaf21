// mzgo_replay.hip -- the device replay store (mzgo.h: mzgo_replay_*).
//
// Finished games stay in HBM in the self-play record format (stones i8, invd
// u8, flags u8: 2 N^2 + 1 bytes per position) in a FIFO ring of game slots;
// the trainer's targets (main.py:381-522, mzgo.trainer's batched step) are
// assembled from them by one launch per batch, k_replay_batch, which also
// applies one of the eight board symmetries as an index permutation.  The
// host keeps only each game's length and key id (and, in Python, its
// priority): sampling stays main.py's np.random sequence -- unless the caller
// opts for the device ledger (a weight and a generation per slot) and its
// sampler further down: successive sampling without replacement from a 64-ary
// sum tree (k_replay_sample_build, k_replay_sample_draw), batches assembled
// from the sampler's device items, priorities written back by a launch -- and,
// between the draw and the assembly, the sampled windows' positions searched
// again in place (k_replay_window_items, then the engine's in-place queue).
// Opt-in on top of that ledger, a weight per stored position (PosLedger) and a
// sampler that draws from the same tree and carries one draw's target through
// two more levels inside the picked game (k_replay_possample_build,
// k_replay_possample_draw), with the
// positions' weights written back from the step's value errors.  Next to the
// batch assembly, one more launch on the same items turns the games' final
// boards into the ownership head's targets (k_replay_ownership), and another
// gives the real boards of the windows' steps 1..K for the consistency loss
// (k_replay_window_obs).
//
// Kernels here use plain vector loads and stores only (and one vector atomic,
// the count of refused priority updates); workgroups never communicate.  Compiled with -ffp-contract=off like every unit: the value
// targets repeat the host's f64 operations one by one (no fused multiply-add).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/mzgo.h"
#include "mzgo_move.hpp"
#include "mzgo_replay.hpp"

using namespace mzgo;

#define RHIPCHK(expr)                                                                              \
  do {                                                                                             \
    hipError_t e_ = (expr);                                                                        \
    if (e_ != hipSuccess) return set_error(MZGO_EHIP, "%s: %s", #expr, hipGetErrorString(e_));     \
  } while (0)

namespace {

constexpr int kThreads = 256;      // the workgroup of the ingest and of every kernel that takes a sample of an item
                                   // list (mzgo_replay.hpp: "An item list") per workgroup
constexpr int kMaxBoard = 19;
constexpr int kMaxUnroll = 63;     // wave 0 of k_replay_batch holds the K + 1 value targets

// ---------------------------------------------------------------------------
// Ingest: engine slots g0 .. g0+n-1 -> ring slots (first + i) % cap, one
// workgroup per game (replay_ingest_game, mzgo_replay.hpp).
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads) k_replay_ingest(Store R, ReplayEngineView E, int g0, int first) {
  const int g = g0 + blockIdx.x;
  replay_ingest_game(R, E, g, (first + blockIdx.x) % R.cap, (int)game_key_id(E.game_base, g, E.epoch), threadIdx.x,
                     kThreads);
}

// ---------------------------------------------------------------------------
// Batch assembly: one workgroup per sample of the item list (mzgo_replay.hpp:
// sample_window decodes it, window_position / window_move say which rows of the
// store may be read; a row that may not is the row past a game's end).
//   wave 0     the K + 1 value targets, a thread each (_discounted's loop: at
//              most K multiply-adds in f64, in its order)
//   wave 1     the K actions and rewards
//   all waves  the (K + 2) x 6 planes and the (K + 1) policy rows, element e
//              of the sample's output on thread e % 256: every store is
//              contiguous across the workgroup; the symmetry is a gather
//              through the cell permutation in LDS
// SEARCH (search-value targets, mzgo_replay_batch_items_values): wave 0 writes
// t_val itself from the stored root values (search_value_target,
// mzgo_replay.hpp: at most ``td`` multiply-adds), the plane loop covers the
// start position alone and boot_obs, val, factor and has_boot are not written
// (null).
// A sample whose slot is not the ring's comes out as an empty game's: zero
// planes, pass actions, rewards 0, uniform policy rows, val 0, factor 1,
// has_boot 0, t_val 0; so does a row before a game's first (start + k < 0).
// ---------------------------------------------------------------------------
struct BatchOut {
  float* obs0;        // [B][6][CELLS]
  float* boot_obs;    // [B][K+1][6][CELLS]
  int64_t* acts;      // [B][K]
  float* t_rew;       // [B][K]
  float* t_pol;       // [B][K+1][A]
  double* val;        // [B][K+1]
  double* factor;     // [B][K+1]
  uint8_t* has_boot;  // [B][K+1]
  float* t_val;       // [B][K+1]  SEARCH only
};

template <bool SEARCH>
__global__ void __launch_bounds__(kThreads) k_replay_batch(Store R, const int* items, int K, int td, double discount,
                                                           BatchOut O) {
  __shared__ int perm[kMaxBoard * kMaxBoard];
  const int b = blockIdx.x, tid = threadIdx.x;
  const SampleWindow w = sample_window(R, items, b);
  const int CELLS = R.CELLS, A = R.A, N = R.N, L = w.L;
  const long long start = w.start;
  const size_t pos = w.pos, mv = w.mv;
  for (int c = tid; c < CELLS; c += kThreads) perm[c] = sym_src(N, w.sym, c);

  if (SEARCH && tid <= K) {                               // wave 0 (K <= 63)
    const long long i = start + tid;                       // (every index past L has the target 0)
    O.t_val[(size_t)b * (K + 1) + tid] =
        window_position(w, i) ? search_value_target(R.reward + pos, R.root_value + mv, L, (int)i, td, discount) : 0.f;
  } else if (tid <= K) {
    const long long index = start + tid;
    double target = 0.0, factor = 1.0;
    for (int k = 0; k < K; ++k) {
      const long long j = index + k;
      if (!window_position(w, j)) break;
      target += factor * R.reward[pos + j];
      factor *= discount;
    }
    const size_t o = (size_t)b * (K + 1) + tid;
    O.val[o] = target;
    O.factor[o] = factor;
    O.has_boot[o] = window_position(w, index + K);
  } else if (tid >= 64 && tid - 64 < K) {                  // wave 1
    const int k = tid - 64;
    const long long j = start + k;
    const size_t o = (size_t)b * K + k;
    O.acts[o] = window_move(w, j) ? sym_dst(N, w.sym, R.action[mv + j]) : A - 1;     // pass past the end
    O.t_rew[o] = window_position(w, j) ? (float)R.reward[pos + j] : 0.f;
  }
  __syncthreads();

  const int plane = 6 * CELLS;
  for (int e = tid; e < (SEARCH ? 1 : K + 2) * plane; e += kThreads) {
    const int row = e / plane, rem = e - row * plane;
    const int p = rem / CELLS, c = rem - p * CELLS;
    // row 0: the start position; row k + 1: the bootstrap position of unroll step k
    const long long at = row == 0 ? start : start + row - 1 + K;
    float v = 0.f;
    if (window_position(w, at)) {
      const size_t q = pos + (size_t)at;
      v = observation_plane(R.stones + q * CELLS, R.invd + q * CELLS, R.flags[q], p, perm[c]);
    }
    if (row == 0) O.obs0[(size_t)b * plane + rem] = v;
    else O.boot_obs[((size_t)b * (K + 1) + row - 1) * plane + rem] = v;
  }

  const float uniform = (float)(1.0 / A);
  for (int e = tid; e < (K + 1) * A; e += kThreads) {
    const int k = e / A, a = e - k * A;
    const long long i = start + k;
    float v = uniform;
    // a position searched with the fast budget (kFlagFast) is no policy target: an all-zero row,
    // on which the loss and its gradient are exactly 0
    if (window_move(w, i))
      v = (R.flags[pos + i] & kFlagFast) ? 0.f : (float)R.policy[(mv + i) * A + (a < CELLS ? perm[a] : a)];
    O.t_pol[(size_t)b * (K + 1) * A + e] = v;
  }
}

// t_val = (float)(val + factor * (double)v) where a bootstrap position exists
__global__ void __launch_bounds__(kThreads) k_replay_finish(const double* val, const double* factor,
                                                            const uint8_t* has_boot, const float* v, int n,
                                                            float* t_val) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  t_val[i] = has_boot[i] ? (float)(val[i] + factor[i] * (double)v[i]) : (float)val[i];
}

// ---------------------------------------------------------------------------
// Ownership targets: one workgroup per sample of the item list.  The
// final board (row L) goes to LDS; the reached-colour masks of its empty cells
// are iterated to their fixed point in two LDS buffers, a pass reading one and
// writing the other, with the barrier that also ORs the threads' "changed"
// between passes (own_reach_step, mzgo_replay.hpp; at most CELLS + 1 passes,
// whatever the board holds); then the K + 1 rows are written, element e on
// thread e % 256, through the symmetry's cell permutation.  A game that did
// not end, a slot outside the ring and a row past the final board give zeros
// and mask 0.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads) k_replay_ownership(Store R, const int* items, int K,
                                                               float* __restrict__ t_own,
                                                               float* __restrict__ own_mask) {
  __shared__ int8_t st[kMaxBoard * kMaxBoard];
  __shared__ uint8_t reach[2][kMaxBoard * kMaxBoard];
  __shared__ int perm[kMaxBoard * kMaxBoard];
  const int b = blockIdx.x, tid = threadIdx.x;
  const SampleWindow w = sample_window(R, items, b);
  const int CELLS = R.CELLS, N = R.N, start = w.start, sym = w.sym, L = w.L;
  const size_t pos = w.pos;
  const int final_flags = window_position(w, L) ? R.flags[pos + L] : 0;
  float* out = t_own + (size_t)b * (K + 1) * CELLS;
  if (tid <= K) own_mask[(size_t)b * (K + 1) + tid] = own_row_valid((long long)start + tid, L, final_flags) ? 1.f : 0.f;
  if (!own_row_valid(start < 0 ? 0 : start, L, final_flags)) {    // (block-uniform) no row of the sample has a target
    for (int e = tid; e < (K + 1) * CELLS; e += kThreads) out[e] = 0.f;
    return;
  }
  for (int c = tid; c < CELLS; c += kThreads) {
    st[c] = R.stones[(pos + L) * CELLS + c];
    reach[0][c] = 0;
    perm[c] = sym_src(N, sym, c);
  }
  __syncthreads();
  int cur = 0;
  for (int pass = 0; pass <= CELLS; ++pass) {
    int changed = 0;
    for (int c = tid; c < CELLS; c += kThreads) {
      const int m = st[c] ? 0 : own_reach_step(st, reach[cur], N, c);
      changed |= m != reach[cur][c];
      reach[cur ^ 1][c] = (uint8_t)m;
    }
    cur ^= 1;
    if (!__syncthreads_or(changed)) break;                // (the same answer on every thread)
  }
  // the owners over the stones (each thread its own cells: the passes are done with st)
  for (int c = tid; c < CELLS; c += kThreads) reach[cur ^ 1][c] = (uint8_t)own_owner(st[c], reach[cur][c]);
  __syncthreads();
  const uint8_t* owner = reach[cur ^ 1];
  for (int e = tid; e < (K + 1) * CELLS; e += kThreads) {
    const int k = e / CELLS, c = e - k * CELLS;
    const long long at = (long long)start + k;
    float v = 0.f;
    if (own_row_valid(at, L, final_flags)) v = own_target(owner[perm[c]], 1 + (R.flags[pos + at] & 1));
    out[e] = v;
  }
}

// ---------------------------------------------------------------------------
// The real boards of a sampled window (the consistency loss's targets' inputs):
// one workgroup per sample of the item list.  obs[k-1][b] is the six
// planes of position start + k, k = 1..K, exactly as k_replay_batch writes obs0
// for that position (the same planes through the same cell permutation),
// step-major [K][B][6][CELLS]; window_mask[b][k-1] = start + k <= L (row L, the
// final board, is stored and counts).  Past the final board and for a slot
// outside the ring: zeros and mask 0.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads) k_replay_window_obs(Store R, const int* items, int B, int K,
                                                                float* __restrict__ obs,
                                                                float* __restrict__ window_mask) {
  __shared__ int perm[kMaxBoard * kMaxBoard];
  const int b = blockIdx.x, tid = threadIdx.x;
  const SampleWindow w = sample_window(R, items, b);
  const int CELLS = R.CELLS, N = R.N;
  const long long start = w.start;
  for (int c = tid; c < CELLS; c += kThreads) perm[c] = sym_src(N, w.sym, c);
  if (tid < K) window_mask[(size_t)b * K + tid] = window_position(w, start + tid + 1) ? 1.f : 0.f;
  __syncthreads();
  const int plane = 6 * CELLS;
  for (int e = tid; e < K * plane; e += kThreads) {
    const int k = e / plane, rem = e - k * plane;
    const int p = rem / CELLS, c = rem - p * CELLS;
    const long long at = start + k + 1;
    float v = 0.f;
    if (window_position(w, at)) {
      const size_t q = w.pos + (size_t)at;
      v = observation_plane(R.stones + q * CELLS, R.invd + q * CELLS, R.flags[q], p, perm[c]);
    }
    obs[((size_t)k * B + b) * plane + rem] = v;
  }
}

// ---------------------------------------------------------------------------
// Reanalysis in place: stored positions -> contiguous staging (mzgo_reanalyse's
// inputs), and its policy rows and root values back.  items [n][2] = (slot,
// move); one wave per item.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(64) k_replay_gather(Store R, const int* items, int8_t* stones, uint8_t* invd,
                                                      uint8_t* flags, int* ids) {
  const int i = blockIdx.x, slot = items[2 * i], t = items[2 * i + 1];
  const size_t q = (size_t)slot * (R.M + 1) + t;
  for (int c = threadIdx.x; c < R.CELLS; c += 64) {
    stones[(size_t)i * R.CELLS + c] = R.stones[q * R.CELLS + c];
    invd[(size_t)i * R.CELLS + c] = R.invd[q * R.CELLS + c];
  }
  if (threadIdx.x == 0) {
    flags[i] = R.flags[q];
    ids[2 * i] = R.key_gid[slot];
    ids[2 * i + 1] = t;
  }
}

__global__ void __launch_bounds__(64) k_replay_scatter(Store R, const int* items, const double* policy,
                                                       const double* value) {
  const int i = blockIdx.x, slot = items[2 * i], t = items[2 * i + 1];
  const size_t q = (size_t)slot * R.M + t;
  for (int a = threadIdx.x; a < R.A; a += 64) R.policy[q * R.A + a] = policy[(size_t)i * R.A + a];
  if (threadIdx.x == 0) {
    R.root_value[q] = value[i];
    // the row is a full-budget search's now (bits 0-2 never change: a row listed twice gets the same byte twice)
    uint8_t* fl = R.flags + (size_t)slot * (R.M + 1) + t;
    if (*fl & kFlagFast) *fl = (uint8_t)(*fl & ~kFlagFast);
  }
}

// ---------------------------------------------------------------------------
// The item list of a sampled batch's windows (mzgo_replay.hpp: window_rows,
// window_has), latest first, built where the sampler left its triples.  One
// workgroup and no atomics: thread t % 256 owns move t, counts the windows
// that hold it, takes the sum of the later moves' counts as its first index and
// writes its (slot, t) pairs in batch order -- the list is a function of the
// inputs alone.  The B windows pass through LDS 256 at a time.
//   cnt [2][M]   scratch: the counts, then each move's next free index
//   out [B (K + 1)][2], n_out [1]; n_copy: a second word for the count, or null
// VALUES (search-value targets, td >= 1): a sample's rows are its window and
// its value rows (value_rows, sample_has), each once; out [2 B (K + 1)][2].
// ---------------------------------------------------------------------------
template <bool VALUES>
__global__ void __launch_bounds__(kThreads) k_replay_window_items(Store R, const int* items, int B, int K, int td,
                                                                  int* cnt, int* out, int* n_out, int* n_copy) {
  __shared__ int w_slot[kThreads], w_start[kThreads], w_rows[kThreads];
  __shared__ int w_vfirst[VALUES ? kThreads : 1], w_vrows[VALUES ? kThreads : 1];
  // whether sample i of the chunk in LDS lists move t
  auto has = [&](int i, int t) {
    if constexpr (VALUES) return sample_has(w_start[i], w_rows[i], w_vfirst[i], w_vrows[i], t);
    return window_has(w_start[i], w_rows[i], t);
  };
  const int tid = threadIdx.x, M = R.M;
  int* next = cnt + M;
  for (int t = tid; t < M; t += kThreads) cnt[t] = 0;
  for (int pass = 0; pass < 2; ++pass) {
    for (int b0 = 0; b0 < B; b0 += kThreads) {
      const int nb = min(kThreads, B - b0);
      __syncthreads();                                     // (the chunk before: every thread has read it)
      if (tid < nb) {
        const int slot = items[3 * (b0 + tid)], start = items[3 * (b0 + tid) + 1];
        w_slot[tid] = slot;
        w_start[tid] = start;
        w_rows[tid] = window_rows(R.length, R.cap, slot, start, K);
        if constexpr (VALUES) w_vrows[tid] = value_rows(R.length, R.cap, slot, start, K, td, &w_vfirst[tid]);
      }
      __syncthreads();
      for (int t = tid; t < M; t += kThreads) {            // (a game holds at most M moves: t < M)
        if (pass == 0) {
          int c = cnt[t];
          for (int i = 0; i < nb; ++i) c += has(i, t);
          cnt[t] = c;
        } else {
          int at = next[t];
          for (int i = 0; i < nb; ++i)
            if (has(i, t)) {
              out[2 * (size_t)at] = w_slot[i];
              out[2 * (size_t)at + 1] = t;
              ++at;
            }
          next[t] = at;
        }
      }
    }
    if (pass == 1) break;
    __syncthreads();                                       // every move's count, workgroup-wide
    for (int t = tid; t < M; t += kThreads) {
      int first = 0;
      for (int u = t + 1; u < M; ++u) first += cnt[u];
      next[t] = first;
      if (t == 0) {
        *n_out = first + cnt[0];
        if (n_copy) *n_copy = first + cnt[0];
      }
    }
  }
}

// ---------------------------------------------------------------------------
// The priority ledger.  New games: weight 1.0 and the slot's generation + 1,
// a thread per game, after the launch (or copies) that wrote them.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads) k_replay_new_games(Ledger L, int first, int n) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const int slot = (first + i) % L.cap;
  L.prio[slot] = 1.0;
  L.gen[slot] += 1u;
}

// ---------------------------------------------------------------------------
// The samplers: successive sampling without replacement from a 64-ary sum tree
// (leaves = slots, level 1 = sums of 64 leaves, level 2 = sums of 64 of those;
// every sum is element 63 of mzgo_replay.hpp's six-step scan).  The tree_*
// functions below are the tree on one wave, once, for the game sampler's
// kernels and the position sampler's (SumTreeHost, mzgo_replay.hpp, is their
// serial form); a kernel adds what is its own: its leaves, how a picked game's
// start is found, the population of its importance weights.
// ---------------------------------------------------------------------------
__device__ __forceinline__ double wave_scan64(double v, int lane) {
  for (int d = 1; d < 64; d <<= 1) {
    const double below = __shfl_up(v, d);                  // lane i - d's (lanes < d: their own, unused)
    v = scan_step(lane, d, v, below);
  }
  return v;
}
// one level of the descent over the wave's 64 entries x with inclusive prefix
// p; *target becomes the remainder for the level below
__device__ __forceinline__ int wave_pick(double x, double p, double* target) {
  const uint64_t nonzero = __ballot(x > 0.0), over = __ballot(x > 0.0 && p > *target);
  const int j = pick_entry(over, nonzero);
  const double below = __shfl(p, j > 0 ? j - 1 : 0);
  *target = *target - (j > 0 ? below : 0.0);
  return j;
}

// the build kernels' tail, on one wave: lane i's leaf of group g (the slots past the store's end: 0) and the group's sum
__device__ __forceinline__ void tree_build_group(const SumTree& T, int g, double x, int lane) {
  const int i = g * 64 + lane;
  if (i < T.cap) T.leaf[i] = x;
  const double p = wave_scan64(x, lane);
  if (lane == 63) T.l1[g] = p;
}
// the draw kernels' prologue, on their one wave: level 1 into s1 [64 * 64] (LDS), level 2 a lane each (returned)
__device__ __forceinline__ double tree_prologue(const SumTree& T, double* s1, int lane) {
  const int n1 = T.n1, n2 = (n1 + 63) / 64;
  for (int i = lane; i < n2 * 64; i += 64) s1[i] = i < n1 ? T.l1[i] : 0.0;
  __syncthreads();
  double x2 = 0.0;                                         // lane i: level-2 entry i
  for (int g = 0; g < n2; ++g) {
    const double s = __shfl(wave_scan64(s1[g * 64 + lane], lane), 63);
    if (lane == g) x2 = s;
  }
  return x2;
}
// one draw: target = u x total descends the three levels; the picked leaf is
// removed and its two ancestors (s1, *x2) are summed again, never subtracted
// from.  The caller syncs before the next draw reads the leaf and s1.
__device__ __forceinline__ TreePick tree_draw(const SumTree& T, double* s1, double* x2, double u, int lane) {
  const double p2 = wave_scan64(*x2, lane);
  TreePick d;
  d.total = __shfl(p2, 63);
  d.target = u * d.total;
  const int j2 = wave_pick(*x2, p2, &d.target);
  const double x1 = s1[j2 * 64 + lane];
  const int j1 = wave_pick(x1, wave_scan64(x1, lane), &d.target);
  const int g1 = j2 * 64 + j1, i0 = g1 * 64 + lane;
  double x0 = i0 < T.cap ? T.leaf[i0] : 0.0;
  const int j0 = wave_pick(x0, wave_scan64(x0, lane), &d.target);
  d.slot = min(g1 * 64 + j0, T.cap - 1);
  d.w = __shfl(x0, j0);
  if (lane == j0) {
    x0 = 0.0;
    T.leaf[d.slot] = 0.0;
  }
  const double sum0 = __shfl(wave_scan64(x0, lane), 63);
  const double sum1 = __shfl(wave_scan64(lane == j1 ? sum0 : x1, lane), 63);
  if (lane == j1) s1[g1] = sum0;
  if (lane == j2) *x2 = sum1;
  return d;
}
// the draw kernels' epilogue: importance weights out of a population of n, from
// the picked weights (T.pick_w) and the total before any removal, over the batch's largest
__device__ __forceinline__ void tree_weights(const SumTree& T, int B, int n, double total0, double beta, float* weight,
                                             int lane) {
  double vmax = 0.0;
  for (int b = lane; b < B; b += 64) vmax = fmax(vmax, pow((double)n * T.pick_w[b] / total0, -beta));
  for (int d = 32; d > 0; d >>= 1) vmax = fmax(vmax, __shfl_xor(vmax, d));
  for (int b = lane; b < B; b += 64) weight[b] = (float)(pow((double)n * T.pick_w[b] / total0, -beta) / vmax);
}

// a wave per group of 64 slots: the working leaves and the group's sum
__global__ void __launch_bounds__(kThreads) k_replay_sample_build(SumTree T, const double* prio, const int* length) {
  const int lane = threadIdx.x & 63, g = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  if (g >= T.n1) return;                                   // (the whole wave)
  const int i = g * 64 + lane;
  tree_build_group(T, g, i < T.cap && length[i] > 0 ? prio[i] : 0.0, lane);
}

struct SampleOut {
  int* items;          // [B][3] slot, start, symmetry (k_replay_batch's)
  int* index;          // [B]    logical, oldest = 0
  uint32_t* gen;       // [B]    the slot's generation at the draw
  float* weight;       // [B]    importance weights (may be null)
};
// draw t's outputs (one lane): the sample, and its picked weight for the epilogue
__device__ __forceinline__ void sample_write(const SampleOut& O, const SumTree& T, int t, int slot, int start,
                                             int symmetry, int head, const uint32_t* gen, double w) {
  O.items[3 * t] = slot;
  O.items[3 * t + 1] = start;
  O.items[3 * t + 2] = symmetry;
  O.index[t] = (slot - head + T.cap) % T.cap;
  O.gen[t] = gen[slot];
  T.pick_w[t] = w;
}

// one workgroup of one wave: level 1 in LDS, level 2 a lane each, B draws
__global__ void __launch_bounds__(64) k_replay_sample_draw(SumTree T, const uint32_t* gen, const int* length, int head,
                                                           int B, uint64_t key, int symmetries, double beta,
                                                           int n_valid, SampleOut O) {
  __shared__ double s1[64 * 64];
  const int lane = threadIdx.x;
  double x2 = tree_prologue(T, s1, lane);
  double total0 = 0.0;
  for (int t = 0; t < B; ++t) {
    const TreePick d = tree_draw(T, s1, &x2, sample_u(key, t), lane);
    if (t == 0) total0 = d.total;
    if (lane == 0)                                         // the start: uniform over the game's moves
      sample_write(O, T, t, d.slot, sample_start(key, t, length[d.slot]), sample_symmetry(key, t, symmetries), head,
                   gen, d.w);
    __syncthreads();                                       // (the leaf and s1 before the next draw reads them)
  }
  if (O.weight) tree_weights(T, B, n_valid, total0, beta, O.weight, lane);
}

// a thread per sample: the sampled slot's new priority, unless the slot has
// taken another game since (its generation moved on).  ``per`` f32 [B]: each
// sample's own loss; or ``mean`` f64 [1]: one value for all B.
__global__ void __launch_bounds__(kThreads) k_replay_update_priorities(Ledger L, const int* items, const uint32_t* gen,
                                                                       const float* per, const double* mean, int B,
                                                                       double alpha) {
  const int b = blockIdx.x * kThreads + threadIdx.x;
  if (b >= B) return;
  const int slot = items[3 * b];
  if (slot < 0 || slot >= L.cap || L.gen[slot] != gen[b]) return;
  const double p = per ? (double)per[b] : *mean;
  if (!(p >= 0.0 && p <= kDoubleMax)) {                    // NaN, inf or negative: the slot keeps its weight
    atomicAdd(L.skipped, 1u);
    return;
  }
  L.prio[slot] = priority_of(p, alpha);
}

// ---------------------------------------------------------------------------
// The position ledger (PosLedger, mzgo_replay.hpp).  New games: a thread per
// (game, position), after the launch (or copies) that wrote the games and next
// to k_replay_new_games: the |root value - n-step target| of the position,
// floored and raised to alpha (POS_INIT_TD), or 1.0 (POS_INIT_UNIFORM).
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads) k_replay_new_positions(Store R, PosLedger P, int first, int n) {
  const long long e = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (e >= (long long)n * P.M) return;
  const int i = (int)(e / P.M), t = (int)(e - (long long)i * P.M);
  const int slot = (first + i) % P.cap;
  const int L = R.length[slot];
  if (t >= L) return;
  P.pprio[(size_t)slot * P.M + t] =
      P.init_mode == POS_INIT_UNIFORM
          ? 1.0
          : position_td_priority(R.reward + (size_t)slot * (R.M + 1), R.root_value + (size_t)slot * R.M, L, t,
                                 P.td_steps, P.discount, P.floor, P.alpha);
}

// a game's weight from its position weights row[0..len), on one wave: the chunk
// sums land a lane each (lane c: chunk c; the rest 0) in *chunks, the weight is
// returned on every lane (len <= 64 * 64)
__device__ __forceinline__ double wave_game_weight(const double* row, int len, int lane, double* chunks) {
  double xc = 0.0;
  for (int c = 0; c * 64 < len; ++c) {
    const int t = c * 64 + lane;
    const double s = __shfl(wave_scan64(t < len ? row[t] : 0.0, lane), 63);
    if (lane == c) xc = s;
  }
  *chunks = xc;
  return __shfl(wave_scan64(xc, lane), 63);
}

// a workgroup per group of 64 slots, a wave per 16 of them: the working leaves
// (the games' weights), the group's sum and the group's count of positions
__global__ void __launch_bounds__(kThreads) k_replay_possample_build(SumTree T, PosLedger P, const int* length) {
  __shared__ double s_w[64];
  __shared__ int s_len[64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = blockIdx.x;
  for (int k = wave; k < 64; k += kThreads / 64) {
    const int slot = g * 64 + k;                           // (uniform over the wave)
    const int len = slot < P.cap ? min(max(length[slot], 0), P.M) : 0;
    double chunks;
    const double w = len > 0 ? wave_game_weight(P.pprio + (size_t)slot * P.M, len, lane, &chunks) : 0.0;
    if (lane == 0) {
      s_w[k] = w;
      s_len[k] = len;
    }
  }
  __syncthreads();
  if (wave != 0) return;
  tree_build_group(T, g, s_w[lane], lane);
  int np = s_len[lane];
  for (int d = 32; d > 0; d >>= 1) np += __shfl_xor(np, d);
  if (lane == 63) P.npos1[g] = np;
}

// k_replay_sample_draw over the games' weights, then the remainder of the same
// target through the picked game's chunk sums and the picked chunk's positions:
// one u picks (game, position).  One workgroup of one wave.
__global__ void __launch_bounds__(64) k_replay_possample_draw(SumTree T, PosLedger P, const uint32_t* gen,
                                                              const int* length, int head, int B, uint64_t key,
                                                              int symmetries, double beta, SampleOut O) {
  __shared__ double s1[64 * 64];
  const int lane = threadIdx.x;
  int n_pos = 0;                                           // the population of the importance weights
  for (int i = lane; i < T.n1; i += 64) n_pos += P.npos1[i];
  for (int d = 32; d > 0; d >>= 1) n_pos += __shfl_xor(n_pos, d);
  if (lane == 0) *P.n_pos = n_pos;
  double x2 = tree_prologue(T, s1, lane);
  double total0 = 0.0;
  for (int t = 0; t < B; ++t) {
    TreePick d = tree_draw(T, s1, &x2, sample_u(key, t), lane);
    if (t == 0) total0 = d.total;
    // the start, inside the game: its chunk sums (the build's additions again), then the chunk's positions
    const int len = min(max(length[d.slot], 0), P.M);
    const double* row = P.pprio + (size_t)d.slot * P.M;
    double xc;
    (void)wave_game_weight(row, len, lane, &xc);
    const int jc = wave_pick(xc, wave_scan64(xc, lane), &d.target);
    const int tt = jc * 64 + lane;
    const double xt = tt < len ? row[tt] : 0.0;
    const int jt = wave_pick(xt, wave_scan64(xt, lane), &d.target);
    const double w = __shfl(xt, jt);
    if (lane == 0)
      sample_write(O, T, t, d.slot, max(min(jc * 64 + jt, len - 1), 0), sample_symmetry(key, t, symmetries), head, gen,
                   w);
    __syncthreads();                                       // (the leaf and s1 before the next draw reads them)
  }
  if (O.weight) tree_weights(T, B, n_pos, total0, beta, O.weight, lane);
}

// a thread per (sample b, unroll step k): position start_b + k of the sampled
// game gets the weight of |value - t_val| (f32 [B][K + 1] both, raw head outputs
// and raw targets), unless the slot has taken another game since the draw or
// the row lies past the game's end.  Samples are distinct games: no two
// threads write one word.
__global__ void __launch_bounds__(kThreads) k_replay_update_position_priorities(PosLedger P, const uint32_t* slot_gen,
                                                                                unsigned* skipped, const int* length,
                                                                                const int* items, const uint32_t* gen,
                                                                                const float* value, const float* t_val,
                                                                                int B, int K1) {
  const int e = blockIdx.x * kThreads + threadIdx.x;
  if (e >= B * K1) return;
  const int b = e / K1, k = e - b * K1;
  const int slot = items[3 * b], start = items[3 * b + 1];
  if (slot < 0 || slot >= P.cap || start < 0 || slot_gen[slot] != gen[b]) return;
  const int t = start + k;
  if (t >= length[slot] || t >= P.M) return;
  const double err = fabs((double)value[e] - (double)t_val[e]);
  if (!(err <= kDoubleMax)) {                              // NaN or inf: the position keeps its weight
    atomicAdd(skipped, 1u);
    return;
  }
  P.pprio[(size_t)slot * P.M + t] = position_priority_of(err, P.floor, P.alpha);
}

}  // namespace

// ---------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------
struct mzgo_replay {
  Store R{};
  int device = 0;
  int head = 0, size = 0;                 // logical game i lives in slot (head + i) % cap
  std::vector<int> len, gid;              // per SLOT: host mirrors of R.length / R.key_gid
  std::vector<void*> allocs;
  // index staging: pinned host words -> device words (mzgo_replay_items: the caller's; the reanalysis: d_items)
  int* h_items = nullptr;
  int* d_items = nullptr;
  size_t items_cap = 0;
  hipEvent_t items_read = nullptr;        // the last upload from h_items has been read
  // reanalysis staging (grown on demand)
  void* stage = nullptr;
  size_t stage_bytes = 0;
  unsigned* games_q = nullptr;            // mzgo_replay_play_games: the queue head, then the error word
  // mzgo_replay_reanalyse_sample: the window items' count, the builder's scratch [2][M], the list (grown on demand)
  int* win_n = nullptr;
  int* win_cnt = nullptr;
  int* win_items = nullptr;
  size_t win_cap = 0;                     // pairs win_items holds
  Ledger L{};                             // device priorities and generations
  SumTree T{};                            // the sampler's scratch: both samplers build it and draw from it
  int n_valid = 0;                      // slots whose mirrored length is > 0 (the sampler's population)
  PosLedger P{};                          // the position ledger (mzgo_replay_enable_positions)
  bool positions = false;                 // whether P is allocated and kept

  int slot_of(int i) const { return (head + i) % R.cap; }
  void set_len(int slot, int length) {
    n_valid += (length > 0) - (len[slot] > 0);
    len[slot] = length;
  }
  // weight 1.0 and the next generation for the n games from ring slot ``first`` (n <= cap)
  int new_games(int first, int n, hipStream_t s) {
    if (n < 1) return MZGO_OK;
    hipLaunchKernelGGL(k_replay_new_games, dim3((n + kThreads - 1) / kThreads), dim3(kThreads), 0, s, L, first, n);
    RHIPCHK(hipGetLastError());
    return positions ? new_positions(first, n, s) : MZGO_OK;
  }
  // the position weights of the n games from ring slot ``first`` (n <= cap), from the lengths on the device
  int new_positions(int first, int n, hipStream_t s) {
    const long long threads = (long long)n * P.M;
    hipLaunchKernelGGL(k_replay_new_positions, dim3((unsigned)((threads + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                       s, R, P, first, n);
    RHIPCHK(hipGetLastError());
    return MZGO_OK;
  }

  template <class T>
  int alloc(T** p, size_t n) {
    void* v = nullptr;
    hipError_t e = hipMalloc(&v, n * sizeof(T) + 256);
    if (e != hipSuccess) return set_error(MZGO_EHIP, "hipMalloc(%zu): %s", n * sizeof(T), hipGetErrorString(e));
    allocs.push_back(v);
    *p = reinterpret_cast<T*>(v);
    return MZGO_OK;
  }
  ~mzgo_replay() {
    for (void* p : allocs) (void)hipFree(p);
    if (d_items) (void)hipFree(d_items);
    if (h_items) (void)hipHostFree(h_items);
    if (stage) (void)hipFree(stage);
    if (win_items) (void)hipFree(win_items);
    if (items_read) (void)hipEventDestroy(items_read);
  }

  // room for n index words on both sides; waits until the previous upload left h_items
  int items_room(size_t n, hipStream_t s) {
    RHIPCHK(hipEventSynchronize(items_read));
    if (n <= items_cap) return MZGO_OK;
    RHIPCHK(hipStreamSynchronize(s));                      // (a launch may still read d_items)
    if (d_items) RHIPCHK(hipFree(d_items));
    if (h_items) RHIPCHK(hipHostFree(h_items));
    d_items = h_items = nullptr;
    items_cap = 0;
    const size_t cap = std::max<size_t>(n, 1024);
    RHIPCHK(hipMalloc((void**)&d_items, cap * sizeof(int)));
    RHIPCHK(hipHostMalloc((void**)&h_items, cap * sizeof(int), hipHostMallocDefault));
    items_cap = cap;
    return MZGO_OK;
  }
  int items_upload(int* dst, size_t n, hipStream_t s) {
    RHIPCHK(hipMemcpyAsync(dst, h_items, n * sizeof(int), hipMemcpyHostToDevice, s));
    RHIPCHK(hipEventRecord(items_read, s));
    return MZGO_OK;
  }
  // make room for n more games at the ring's end (FIFO eviction); returns the first new slot
  int push(int n) {
    const int first = (head + size) % R.cap;
    const int evict = std::max(0, size + n - R.cap);
    head = (head + evict) % R.cap;
    size = size + n - evict;
    return first;
  }
};

extern "C" {

int mzgo_replay_create(int board_size, int capacity, int max_moves, int device, mzgo_replay** out) {
  if (!out) return set_error(MZGO_EINVAL, "mzgo_replay_create: null out");
  *out = nullptr;
  if (board_size < 2 || board_size > kMaxBoard)
    return set_error(MZGO_EINVAL, "mzgo_replay_create: board_size %d (2..%d)", board_size, kMaxBoard);
  if (capacity < 1) return set_error(MZGO_EINVAL, "mzgo_replay_create: capacity must be >= 1, got %d", capacity);
  if (max_moves < 1) return set_error(MZGO_EINVAL, "mzgo_replay_create: max_moves must be >= 1, got %d", max_moves);
  RHIPCHK(hipSetDevice(device));
  mzgo_replay* r = new mzgo_replay;
  r->device = device;
  Store& R = r->R;
  R.N = board_size; R.CELLS = board_size * board_size; R.A = R.CELLS + 1; R.M = max_moves; R.cap = capacity;
  const size_t cap = capacity, M = max_moves, C = R.CELLS, A = R.A;
  int rc = MZGO_OK;
  auto chk = [&](int x) { if (rc == MZGO_OK) rc = x; };
  chk(r->alloc(&R.stones, cap * (M + 1) * C));
  chk(r->alloc(&R.invd, cap * (M + 1) * C));
  chk(r->alloc(&R.flags, cap * (M + 1)));
  chk(r->alloc(&R.action, cap * M));
  chk(r->alloc(&R.policy, cap * M * A));
  chk(r->alloc(&R.reward, cap * (M + 1)));
  chk(r->alloc(&R.root_value, cap * M));
  chk(r->alloc(&R.length, cap));
  chk(r->alloc(&R.key_gid, cap));
  chk(r->alloc(&r->games_q, 2));
  chk(r->alloc(&r->win_n, 1));
  chk(r->alloc(&r->win_cnt, 2 * M));
  Ledger& L = r->L;
  L.cap = capacity;
  chk(r->alloc(&L.prio, cap));
  chk(r->alloc(&L.gen, cap));
  chk(r->alloc(&L.skipped, 1));
  SumTree& T = r->T;
  T.cap = capacity;
  T.n1 = (capacity + 63) / 64;
  chk(r->alloc(&T.leaf, cap));
  chk(r->alloc(&T.l1, (size_t)T.n1));
  chk(r->alloc(&T.pick_w, cap));
  if (rc == MZGO_OK && (hipMemset(R.length, 0, cap * sizeof(int)) != hipSuccess ||
                        hipMemset(L.prio, 0, cap * sizeof(double)) != hipSuccess ||
                        hipMemset(L.gen, 0, cap * sizeof(uint32_t)) != hipSuccess ||
                        hipMemset(L.skipped, 0, sizeof(unsigned)) != hipSuccess))
    rc = set_error(MZGO_EHIP, "mzgo_replay_create: hipMemset failed");
  if (rc == MZGO_OK && hipEventCreateWithFlags(&r->items_read, hipEventDisableTiming) != hipSuccess)
    rc = set_error(MZGO_EHIP, "mzgo_replay_create: hipEventCreate failed");
  if (rc != MZGO_OK) { delete r; return rc; }
  r->len.assign(cap, 0);
  r->gid.assign(cap, 0);
  *out = r;
  return MZGO_OK;
}

void mzgo_replay_destroy(mzgo_replay* r) { delete r; }

int mzgo_replay_info(const mzgo_replay* r, int32_t* size_host, int32_t* head_host, int32_t* lengths_host,
                     int32_t* key_gid_host) {
  if (!r) return set_error(MZGO_EINVAL, "mzgo_replay_info: null replay");
  if (size_host) *size_host = r->size;
  if (head_host) *head_host = r->head;
  for (int i = 0; i < r->size; ++i) {
    if (lengths_host) lengths_host[i] = r->len[r->slot_of(i)];
    if (key_gid_host) key_gid_host[i] = r->gid[r->slot_of(i)];
  }
  return MZGO_OK;
}

int mzgo_replay_add_games(mzgo_replay* r, mzgo_engine* eng, void* stream) {
  if (!r || !eng) return set_error(MZGO_EINVAL, "mzgo_replay_add_games: null %s", !r ? "replay" : "engine");
  ReplayEngineView E;
  replay_engine_view(eng, &E);
  if (E.latent_dim == 0)
    return set_error(MZGO_EINVAL, "mzgo_replay_add_games: board-only engine (latent_dim 0) has no game records");
  if (E.tower) return set_error(MZGO_EINVAL, "mzgo_replay_add_games: tower engines (tower = 1) are not supported");
  if (E.N != r->R.N)
    return set_error(MZGO_EINVAL, "mzgo_replay_add_games: board size mismatch (store %d, engine %d)", r->R.N, E.N);
  if (E.M != r->R.M)
    return set_error(MZGO_EINVAL, "mzgo_replay_add_games: max_moves mismatch (store %d, engine %d)", r->R.M, E.M);
  hipStream_t s = (hipStream_t)stream;
  // G games pushed one after another: when G exceeds the capacity only the
  // last ``capacity`` survive, so only those are copied (no slot written twice)
  const int n = std::min(E.G, r->R.cap), g0 = E.G - n;
  r->push(g0);
  const int first = r->push(n);
  hipLaunchKernelGGL(k_replay_ingest, dim3(n), dim3(kThreads), 0, s, r->R, E, g0, first);
  RHIPCHK(hipGetLastError());
  if (int rc = r->new_games(first, n, s)) return rc;
  std::vector<int> meta((size_t)E.G * 4);
  RHIPCHK(hipMemcpyAsync(meta.data(), E.meta, meta.size() * sizeof(int), hipMemcpyDeviceToHost, s));
  RHIPCHK(hipStreamSynchronize(s));
  for (int i = 0; i < n; ++i) {
    const int g = g0 + i, slot = (first + i) % r->R.cap;
    r->set_len(slot, std::min(std::max(meta[(size_t)g * 4 + 3], 0), r->R.M));
    r->gid[slot] = (int)game_key_id(E.game_base, g, E.epoch);
  }
  return MZGO_OK;
}

int mzgo_replay_play_games(mzgo_replay* r, mzgo_engine* eng, int n_games, int first_epoch, void* stream) {
  if (!r || !eng) return set_error(MZGO_EINVAL, "mzgo_replay_play_games: null %s", !r ? "replay" : "engine");
  if (n_games < 1) return set_error(MZGO_EINVAL, "mzgo_replay_play_games: n_games must be >= 1, got %d", n_games);
  if (n_games > r->R.cap)
    return set_error(MZGO_EINVAL, "mzgo_replay_play_games: n_games %d exceeds the capacity %d (a ring slot would be "
                     "written twice in one launch)", n_games, r->R.cap);
  ReplayEngineView E;
  replay_engine_view(eng, &E);
  if (E.latent_dim == 0)
    return set_error(MZGO_EINVAL, "mzgo_replay_play_games: board-only engine (latent_dim 0) plays no games");
  if (E.tower) return set_error(MZGO_EINVAL, "mzgo_replay_play_games: tower engines (tower = 1) are not supported");
  if (E.N != r->R.N)
    return set_error(MZGO_EINVAL, "mzgo_replay_play_games: board size mismatch (store %d, engine %d)", r->R.N, E.N);
  if (E.M != r->R.M)
    return set_error(MZGO_EINVAL, "mzgo_replay_play_games: max_moves mismatch (store %d, engine %d)", r->R.M, E.M);
  if (engine_noise_hooked(eng))
    return set_error(MZGO_EINVAL, "mzgo_replay_play_games: a noise hook is set on the engine (injected and recorded "
                     "noise are indexed by slot, a slot plays several games here)");
  hipStream_t s = (hipStream_t)stream;
  const int n = n_games, cap = r->R.cap;
  const int first = (r->head + r->size) % cap;              // (push(n)'s answer: n <= cap)
  const GamesArgs ga{n, E.G, first_epoch, first, r->games_q, (int*)(r->games_q + 1), r->R};
  if (int rc = engine_play_games(eng, ga, s)) return rc;
  r->push(n);
  if (int rc = r->new_games(first, n, s)) return rc;
  // one synchronisation: the n lengths (the ring may wrap) and the error word
  std::vector<int> len(n);
  int err = 0;
  const int run = std::min(n, cap - first);
  RHIPCHK(hipMemcpyAsync(len.data(), r->R.length + first, (size_t)run * sizeof(int), hipMemcpyDeviceToHost, s));
  if (run < n)
    RHIPCHK(hipMemcpyAsync(len.data() + run, r->R.length, (size_t)(n - run) * sizeof(int), hipMemcpyDeviceToHost, s));
  RHIPCHK(hipMemcpyAsync(&err, ga.error, sizeof(int), hipMemcpyDeviceToHost, s));
  RHIPCHK(hipStreamSynchronize(s));
  for (int j = 0; j < n; ++j) {
    const int slot = (first + j) % cap;
    r->set_len(slot, len[j]);
    r->gid[slot] = (int)game_key_id(E.game_base, j % E.G, first_epoch + j / E.G);
  }
  if (err < n)
    return set_error(MZGO_EHIP, "mzgo_replay_play_games: game %d stopped on a board error (stored with the moves it "
                     "has)", err);
  return MZGO_OK;
}

int mzgo_replay_add(mzgo_replay* r, int length, const int8_t* stones_host, const uint8_t* invd_host,
                    const uint8_t* flags_host, const int32_t* action_host, const double* policy_host,
                    const double* reward_host, const double* root_value_host, int32_t key_gid, void* stream) {
  if (!r) return set_error(MZGO_EINVAL, "mzgo_replay_add: null replay");
  if (length < 0 || length > r->R.M)
    return set_error(MZGO_EINVAL, "mzgo_replay_add: length %d out of range (0..max_moves = %d)", length, r->R.M);
  if (!stones_host || !invd_host || !flags_host || !reward_host || (length > 0 && (!action_host || !policy_host)))
    return set_error(MZGO_EINVAL, "mzgo_replay_add: null %s",
                     !stones_host ? "stones" : !invd_host ? "invd" : !flags_host ? "flags" : !reward_host ? "reward"
                     : !action_host ? "action" : "policy");
  hipStream_t s = (hipStream_t)stream;
  const Store& R = r->R;
  const size_t L = length, C = R.CELLS, A = R.A;
  const int slot = r->push(1);
  const size_t pos = (size_t)slot * (R.M + 1), mv = (size_t)slot * R.M;
  RHIPCHK(hipMemcpyAsync(R.stones + pos * C, stones_host, (L + 1) * C, hipMemcpyHostToDevice, s));
  RHIPCHK(hipMemcpyAsync(R.invd + pos * C, invd_host, (L + 1) * C, hipMemcpyHostToDevice, s));
  RHIPCHK(hipMemcpyAsync(R.flags + pos, flags_host, L + 1, hipMemcpyHostToDevice, s));
  RHIPCHK(hipMemcpyAsync(R.reward + pos, reward_host, (L + 1) * 8, hipMemcpyHostToDevice, s));
  if (L > 0) {
    RHIPCHK(hipMemcpyAsync(R.action + mv, action_host, L * 4, hipMemcpyHostToDevice, s));
    RHIPCHK(hipMemcpyAsync(R.policy + mv * A, policy_host, L * A * 8, hipMemcpyHostToDevice, s));
    if (root_value_host) RHIPCHK(hipMemcpyAsync(R.root_value + mv, root_value_host, L * 8, hipMemcpyHostToDevice, s));
    else RHIPCHK(hipMemsetAsync(R.root_value + mv, 0, L * 8, s));
  }
  RHIPCHK(hipMemcpyAsync(R.length + slot, &length, 4, hipMemcpyHostToDevice, s));
  RHIPCHK(hipMemcpyAsync(R.key_gid + slot, &key_gid, 4, hipMemcpyHostToDevice, s));
  if (int rc = r->new_games(slot, 1, s)) return rc;
  RHIPCHK(hipStreamSynchronize(s));                         // (the host buffers are the caller's)
  r->set_len(slot, length);
  r->gid[slot] = key_gid;
  return MZGO_OK;
}

int mzgo_replay_export(mzgo_replay* r, int i, int32_t* length_host, int32_t* key_gid_host, int8_t* stones_host,
                       uint8_t* invd_host, uint8_t* flags_host, int32_t* action_host, double* policy_host,
                       double* reward_host, double* root_value_host, void* stream) {
  if (!r) return set_error(MZGO_EINVAL, "mzgo_replay_export: null replay");
  if (i < 0 || i >= r->size)
    return set_error(MZGO_EINVAL, "mzgo_replay_export: game %d out of range (the store holds %d)", i, r->size);
  hipStream_t s = (hipStream_t)stream;
  const Store& R = r->R;
  const int slot = r->slot_of(i);
  const size_t L = r->len[slot], C = R.CELLS, A = R.A;
  const size_t pos = (size_t)slot * (R.M + 1), mv = (size_t)slot * R.M;
  if (length_host) *length_host = (int32_t)L;
  if (key_gid_host) *key_gid_host = r->gid[slot];
  if (stones_host) RHIPCHK(hipMemcpyAsync(stones_host, R.stones + pos * C, (L + 1) * C, hipMemcpyDeviceToHost, s));
  if (invd_host) RHIPCHK(hipMemcpyAsync(invd_host, R.invd + pos * C, (L + 1) * C, hipMemcpyDeviceToHost, s));
  if (flags_host) RHIPCHK(hipMemcpyAsync(flags_host, R.flags + pos, L + 1, hipMemcpyDeviceToHost, s));
  if (reward_host) RHIPCHK(hipMemcpyAsync(reward_host, R.reward + pos, (L + 1) * 8, hipMemcpyDeviceToHost, s));
  if (L > 0) {
    if (action_host) RHIPCHK(hipMemcpyAsync(action_host, R.action + mv, L * 4, hipMemcpyDeviceToHost, s));
    if (policy_host) RHIPCHK(hipMemcpyAsync(policy_host, R.policy + mv * A, L * A * 8, hipMemcpyDeviceToHost, s));
    if (root_value_host) RHIPCHK(hipMemcpyAsync(root_value_host, R.root_value + mv, L * 8, hipMemcpyDeviceToHost, s));
  }
  RHIPCHK(hipStreamSynchronize(s));
  return MZGO_OK;
}

int mzgo_replay_items(mzgo_replay* r, const int32_t* indices_host, const int32_t* starts_host,
                      const int32_t* symmetries_host, int B, int32_t* items, void* stream) {
  const char* who = "mzgo_replay_items";
  if (!r) return set_error(MZGO_EINVAL, "%s: null replay", who);
  if (B < 1) return set_error(MZGO_EINVAL, "%s: B must be >= 1, got %d", who, B);
  if (!indices_host || !starts_host || !items)
    return set_error(MZGO_EINVAL, "%s: null %s", who, !indices_host ? "indices" : !starts_host ? "starts" : "items");
  for (int b = 0; b < B; ++b) {
    const int i = indices_host[b];
    if (i < 0 || i >= r->size)
      return set_error(MZGO_EINVAL, "%s: sample %d: game %d is not in the store (it holds %d)", who, b, i, r->size);
    const int L = r->len[r->slot_of(i)];
    if (starts_host[b] < 0 || starts_host[b] >= L)
      return set_error(MZGO_EINVAL, "%s: sample %d: start %d outside game %d's %d moves", who, b, starts_host[b], i, L);
    if (symmetries_host && (symmetries_host[b] < 0 || symmetries_host[b] > 7))
      return set_error(MZGO_EINVAL, "%s: sample %d: symmetry %d (0..7)", who, b, symmetries_host[b]);
  }
  hipStream_t s = (hipStream_t)stream;
  if (int rc = r->items_room((size_t)B * 3, s)) return rc;
  for (int b = 0; b < B; ++b) {
    r->h_items[3 * b] = r->slot_of(indices_host[b]);
    r->h_items[3 * b + 1] = starts_host[b];
    r->h_items[3 * b + 2] = symmetries_host ? symmetries_host[b] : 0;
  }
  return r->items_upload(items, (size_t)B * 3, s);
}

int mzgo_replay_batch_items_values(mzgo_replay* r, const int32_t* items, int B, int unroll_steps, int td_steps,
                                   double discount, float* obs0, int64_t* acts, float* t_rew, float* t_pol,
                                   float* t_val, void* stream) {
  const char* who = "mzgo_replay_batch_items_values";
  if (!r) return set_error(MZGO_EINVAL, "%s: null replay", who);
  if (B < 1) return set_error(MZGO_EINVAL, "%s: B must be >= 1, got %d", who, B);
  if (unroll_steps < 1 || unroll_steps > kMaxUnroll)
    return set_error(MZGO_EINVAL, "%s: unroll_steps %d out of range (1..%d)", who, unroll_steps, kMaxUnroll);
  if (td_steps < 1) return set_error(MZGO_EINVAL, "%s: td_steps must be >= 1, got %d", who, td_steps);
  if (!items || !obs0 || !acts || !t_rew || !t_pol || !t_val)
    return set_error(MZGO_EINVAL, "%s: null %s", who,
                     !items ? "items" : !obs0 ? "obs0" : !acts ? "acts" : !t_rew ? "t_rew" : !t_pol ? "t_pol" : "t_val");
  const BatchOut O{obs0, nullptr, acts, t_rew, t_pol, nullptr, nullptr, nullptr, t_val};
  hipLaunchKernelGGL(k_replay_batch<true>, dim3(B), dim3(kThreads), 0, (hipStream_t)stream, r->R, items, unroll_steps,
                     td_steps, discount, O);
  RHIPCHK(hipGetLastError());
  return MZGO_OK;
}

int mzgo_replay_value_targets_host(const double* reward, const double* root_value, int L, int start, int unroll_steps,
                                   int td_steps, double discount, float* t_val) {
  const char* who = "mzgo_replay_value_targets_host";
  if (!reward || !t_val || (L > 0 && !root_value))
    return set_error(MZGO_EINVAL, "%s: null %s", who, !reward ? "reward" : !t_val ? "t_val" : "root_value");
  if (L < 0 || L > (1 << 30)) return set_error(MZGO_EINVAL, "%s: L %d outside 0..2^30", who, L);
  if (start < 0) return set_error(MZGO_EINVAL, "%s: start must be >= 0, got %d", who, start);
  if (unroll_steps < 1 || unroll_steps > kMaxUnroll)
    return set_error(MZGO_EINVAL, "%s: unroll_steps %d out of range (1..%d)", who, unroll_steps, kMaxUnroll);
  if (td_steps < 1) return set_error(MZGO_EINVAL, "%s: td_steps must be >= 1, got %d", who, td_steps);
  for (int k = 0; k <= unroll_steps; ++k) {
    const long long i = (long long)start + k;              // (every index past L has the target 0)
    t_val[k] = search_value_target(reward, root_value, L, i > L ? L + 1 : (int)i, td_steps, discount);
  }
  return MZGO_OK;
}

int mzgo_replay_finish_values(const double* val, const double* factor, const uint8_t* has_boot, const float* value,
                              int n, float* t_val, void* stream) {
  if (n < 1) return set_error(MZGO_EINVAL, "mzgo_replay_finish_values: n must be >= 1, got %d", n);
  if (!val || !factor || !has_boot || !value || !t_val)
    return set_error(MZGO_EINVAL, "mzgo_replay_finish_values: null %s",
                     !val ? "val" : !factor ? "factor" : !has_boot ? "has_boot" : !value ? "value" : "t_val");
  hipLaunchKernelGGL(k_replay_finish, dim3((n + kThreads - 1) / kThreads), dim3(kThreads), 0, (hipStream_t)stream, val,
                     factor, has_boot, value, n, t_val);
  RHIPCHK(hipGetLastError());
  return MZGO_OK;
}

int mzgo_replay_reanalyse(mzgo_replay* r, mzgo_engine* eng, const int32_t* games_host, int n_games, void* stream) {
  if (!r || !eng) return set_error(MZGO_EINVAL, "mzgo_replay_reanalyse: null %s", !r ? "replay" : "engine");
  ReplayEngineView E;
  replay_engine_view(eng, &E);
  if (E.N != r->R.N)
    return set_error(MZGO_EINVAL, "mzgo_replay_reanalyse: board size mismatch (store %d, engine %d)", r->R.N, E.N);
  if (games_host && n_games < 0) return set_error(MZGO_EINVAL, "mzgo_replay_reanalyse: n_games %d", n_games);
  const int ng = games_host ? n_games : r->size;
  std::vector<int> items;                                   // (slot, move), the games' own order
  for (int k = 0; k < ng; ++k) {
    const int i = games_host ? games_host[k] : k;
    if (i < 0 || i >= r->size)
      return set_error(MZGO_EINVAL, "mzgo_replay_reanalyse: game %d is not in the store (it holds %d)", i, r->size);
    const int slot = r->slot_of(i);
    for (int t = 0; t < r->len[slot]; ++t) { items.push_back(slot); items.push_back(t); }
  }
  const size_t n = items.size() / 2;
  if (n == 0) return MZGO_OK;
  // latest move first (mzgo.reanalyse.latest_first): the queue's longest searches start first
  std::vector<int> order(n);
  for (size_t i = 0; i < n; ++i) order[i] = (int)i;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return items[2 * a + 1] > items[2 * b + 1]; });
  hipStream_t s = (hipStream_t)stream;
  if (int rc = r->items_room(2 * n, s)) return rc;
  for (size_t i = 0; i < n; ++i) {
    r->h_items[2 * i] = items[2 * order[i]];
    r->h_items[2 * i + 1] = items[2 * order[i] + 1];
  }
  if (int rc = r->items_upload(r->d_items, 2 * n, s)) return rc;
  // staging, each field on a 256-byte boundary
  const size_t C = r->R.CELLS, A = r->R.A;
  const size_t sizes[] = {n * C, n * C, n, n * 2 * 4, n * A * 4, n * 8, n * A * 8};
  size_t off[8] = {0};
  for (int i = 0; i < 7; ++i) off[i + 1] = off[i] + (sizes[i] + 255) / 256 * 256;
  if (off[7] > r->stage_bytes) {
    RHIPCHK(hipStreamSynchronize(s));
    if (r->stage) RHIPCHK(hipFree(r->stage));
    r->stage = nullptr;
    r->stage_bytes = 0;
    RHIPCHK(hipMalloc(&r->stage, off[7]));
    r->stage_bytes = off[7];
  }
  uint8_t* base = (uint8_t*)r->stage;
  int8_t* st = (int8_t*)(base + off[0]);
  uint8_t* iv = base + off[1];
  uint8_t* fl = base + off[2];
  int* ids = (int*)(base + off[3]);
  int32_t* visits = (int32_t*)(base + off[4]);
  double* value = (double*)(base + off[5]);
  double* policy = (double*)(base + off[6]);
  hipLaunchKernelGGL(k_replay_gather, dim3((unsigned)n), dim3(64), 0, s, r->R, r->d_items, st, iv, fl, ids);
  RHIPCHK(hipGetLastError());
  if (int rc = mzgo_reanalyse(eng, st, iv, fl, ids, nullptr, (int)n, visits, value, policy, stream)) return rc;
  hipLaunchKernelGGL(k_replay_scatter, dim3((unsigned)n), dim3(64), 0, s, r->R, r->d_items, policy, value);
  RHIPCHK(hipGetLastError());
  return MZGO_OK;
}

// the two item-list twins (td_steps 0: the windows alone)
static int window_items_host(const char* who, const int32_t* length, int cap, const int32_t* items, int B,
                             int unroll_steps, int td_steps, int32_t* out, int32_t* n) {
  if (!length || !items || !out || !n)
    return set_error(MZGO_EINVAL, "%s: null %s", who, !length ? "length" : !items ? "items" : !out ? "out" : "n");
  if (cap < 1) return set_error(MZGO_EINVAL, "%s: capacity must be >= 1, got %d", who, cap);
  if (B < 1) return set_error(MZGO_EINVAL, "%s: B must be >= 1, got %d", who, B);
  if (unroll_steps < 1 || unroll_steps > kMaxUnroll)
    return set_error(MZGO_EINVAL, "%s: unroll_steps %d out of range (1..%d)", who, unroll_steps, kMaxUnroll);
  std::vector<int> rows((size_t)B), vfirst((size_t)B, 0), vrows((size_t)B, 0);
  int t_max = -1;
  for (int b = 0; b < B; ++b) {
    rows[b] = window_rows(length, cap, items[3 * b], items[3 * b + 1], unroll_steps);
    if (rows[b] > 0) t_max = std::max(t_max, items[3 * b + 1] + rows[b] - 1);
    if (td_steps > 0)
      vrows[b] = value_rows(length, cap, items[3 * b], items[3 * b + 1], unroll_steps, td_steps, &vfirst[b]);
    if (vrows[b] > 0) t_max = std::max(t_max, vfirst[b] + vrows[b] - 1);
  }
  int at = 0;
  for (int t = t_max; t >= 0; --t)
    for (int b = 0; b < B; ++b)
      if (sample_has(items[3 * b + 1], rows[b], vfirst[b], vrows[b], t)) {
        out[2 * at] = items[3 * b];
        out[2 * at + 1] = t;
        ++at;
      }
  *n = at;
  return MZGO_OK;
}

int mzgo_replay_window_items_host(const int32_t* length, int cap, const int32_t* items, int B, int unroll_steps,
                                  int32_t* out, int32_t* n) {
  return window_items_host("mzgo_replay_window_items_host", length, cap, items, B, unroll_steps, 0, out, n);
}

int mzgo_replay_window_items_values_host(const int32_t* length, int cap, const int32_t* items, int B, int unroll_steps,
                                         int td_steps, int32_t* out, int32_t* n) {
  const char* who = "mzgo_replay_window_items_values_host";
  if (td_steps < 1) return set_error(MZGO_EINVAL, "%s: td_steps must be >= 1, got %d", who, td_steps);
  return window_items_host(who, length, cap, items, B, unroll_steps, td_steps, out, n);
}

// mzgo_replay_reanalyse_sample (td_steps 0: the windows alone) and its _values form
static int reanalyse_sample(const char* who, mzgo_replay* r, mzgo_engine* eng, const int32_t* items, int B,
                            int unroll_steps, int td_steps, int32_t* n_searched, void* stream) {
  if (!r || !eng || !items)
    return set_error(MZGO_EINVAL, "%s: null %s", who, !r ? "replay" : !eng ? "engine" : "items");
  if (B < 1) return set_error(MZGO_EINVAL, "%s: B must be >= 1, got %d", who, B);
  if (unroll_steps < 1 || unroll_steps > kMaxUnroll)
    return set_error(MZGO_EINVAL, "%s: unroll_steps %d out of range (1..%d)", who, unroll_steps, kMaxUnroll);
  ReplayEngineView E;
  replay_engine_view(eng, &E);
  if (E.N != r->R.N) return set_error(MZGO_EINVAL, "%s: board size mismatch (store %d, engine %d)", who, r->R.N, E.N);
  if (E.latent_dim == 0) return set_error(MZGO_EINVAL, "%s: board-only engine (latent_dim 0) has no network", who);
  if (E.tower) return set_error(MZGO_EINVAL, "%s: tower engines (tower = 1) are not supported", who);
  hipStream_t s = (hipStream_t)stream;
  // the host's bound on the list: a window's K + 1 rows and, with value rows, K + 1 more
  const size_t most = (size_t)B * (unroll_steps + 1) * (td_steps > 0 ? 2 : 1);
  if (most > r->win_cap) {
    RHIPCHK(hipStreamSynchronize(s));                      // (a launch may still read the list)
    if (r->win_items) RHIPCHK(hipFree(r->win_items));
    r->win_items = nullptr;
    r->win_cap = 0;
    RHIPCHK(hipMalloc((void**)&r->win_items, most * 2 * sizeof(int)));
    r->win_cap = most;
  }
  if (td_steps > 0)
    hipLaunchKernelGGL(k_replay_window_items<true>, dim3(1), dim3(kThreads), 0, s, r->R, items, B, unroll_steps,
                       td_steps, r->win_cnt, r->win_items, r->win_n, n_searched);
  else
    hipLaunchKernelGGL(k_replay_window_items<false>, dim3(1), dim3(kThreads), 0, s, r->R, items, B, unroll_steps, 0,
                       r->win_cnt, r->win_items, r->win_n, n_searched);
  RHIPCHK(hipGetLastError());
  // (an engine without weights is refused below: the builder wrote the store's scratch only)
  const ReanalyseStoreArgs ra{r->win_items, r->win_n, nullptr, r->R};
  return engine_reanalyse_store(eng, ra, (int)std::min<size_t>(most, 1u << 30), s);
}

int mzgo_replay_reanalyse_sample(mzgo_replay* r, mzgo_engine* eng, const int32_t* items, int B, int unroll_steps,
                                 int32_t* n_searched, void* stream) {
  return reanalyse_sample("mzgo_replay_reanalyse_sample", r, eng, items, B, unroll_steps, 0, n_searched, stream);
}

int mzgo_replay_reanalyse_sample_values(mzgo_replay* r, mzgo_engine* eng, const int32_t* items, int B,
                                        int unroll_steps, int td_steps, int32_t* n_searched, void* stream) {
  const char* who = "mzgo_replay_reanalyse_sample_values";
  if (td_steps < 1) return set_error(MZGO_EINVAL, "%s: td_steps must be >= 1, got %d", who, td_steps);
  return reanalyse_sample(who, r, eng, items, B, unroll_steps, td_steps, n_searched, stream);
}

int mzgo_replay_batch_items(mzgo_replay* r, const int32_t* items, int B, int unroll_steps, double discount,
                            float* obs0, float* boot_obs, int64_t* acts, float* t_rew, float* t_pol, double* val,
                            double* factor, uint8_t* has_boot, void* stream) {
  if (!r) return set_error(MZGO_EINVAL, "mzgo_replay_batch_items: null replay");
  if (B < 1) return set_error(MZGO_EINVAL, "mzgo_replay_batch_items: B must be >= 1, got %d", B);
  if (unroll_steps < 1 || unroll_steps > kMaxUnroll)
    return set_error(MZGO_EINVAL, "mzgo_replay_batch_items: unroll_steps %d out of range (1..%d)", unroll_steps,
                     kMaxUnroll);
  if (!items || !obs0 || !boot_obs || !acts || !t_rew || !t_pol || !val || !factor || !has_boot)
    return set_error(MZGO_EINVAL, "mzgo_replay_batch_items: null %s",
                     !items ? "items" : !obs0 ? "obs0" : !boot_obs ? "boot_obs" : !acts ? "acts" : !t_rew ? "t_rew"
                     : !t_pol ? "t_pol" : !val ? "val" : !factor ? "factor" : "has_boot");
  const BatchOut O{obs0, boot_obs, acts, t_rew, t_pol, val, factor, has_boot, nullptr};
  hipLaunchKernelGGL(k_replay_batch<false>, dim3(B), dim3(kThreads), 0, (hipStream_t)stream, r->R, items, unroll_steps,
                     0, discount, O);
  RHIPCHK(hipGetLastError());
  return MZGO_OK;
}

int mzgo_replay_ownership_items(mzgo_replay* r, const int32_t* items, int B, int unroll_steps, float* t_own,
                                float* own_mask, void* stream) {
  const char* who = "mzgo_replay_ownership_items";
  if (!r) return set_error(MZGO_EINVAL, "%s: null replay", who);
  if (B < 1) return set_error(MZGO_EINVAL, "%s: B must be >= 1, got %d", who, B);
  if (unroll_steps < 0 || unroll_steps > kMaxUnroll)
    return set_error(MZGO_EINVAL, "%s: unroll_steps %d out of range (0..%d)", who, unroll_steps, kMaxUnroll);
  if (!t_own || !own_mask) return set_error(MZGO_EINVAL, "%s: null %s", who, !t_own ? "t_own" : "own_mask");
  if (!items) return set_error(MZGO_EINVAL, "%s: null items", who);
  hipLaunchKernelGGL(k_replay_ownership, dim3(B), dim3(kThreads), 0, (hipStream_t)stream, r->R, items, unroll_steps,
                     t_own, own_mask);
  RHIPCHK(hipGetLastError());
  return MZGO_OK;
}

int mzgo_replay_window_obs_items(mzgo_replay* r, const int32_t* items, int B, int unroll_steps, float* obs,
                                 float* window_mask, void* stream) {
  const char* who = "mzgo_replay_window_obs_items";
  if (!r) return set_error(MZGO_EINVAL, "%s: null replay", who);
  if (B < 1) return set_error(MZGO_EINVAL, "%s: B must be >= 1, got %d", who, B);
  if (unroll_steps < 0 || unroll_steps > kMaxUnroll)
    return set_error(MZGO_EINVAL, "%s: unroll_steps %d out of range (0..%d)", who, unroll_steps, kMaxUnroll);
  if (unroll_steps > 0 && (!obs || !window_mask))
    return set_error(MZGO_EINVAL, "%s: null %s", who, !obs ? "obs" : "window_mask");
  if (!items) return set_error(MZGO_EINVAL, "%s: null items", who);
  if (unroll_steps == 0) return MZGO_OK;                    // (no rows: no launch)
  hipLaunchKernelGGL(k_replay_window_obs, dim3(B), dim3(kThreads), 0, (hipStream_t)stream, r->R, items, B,
                     unroll_steps, obs, window_mask);
  RHIPCHK(hipGetLastError());
  return MZGO_OK;
}

int mzgo_ownership_host(const int8_t* stones, int board_size, int8_t* owner) {
  const char* who = "mzgo_ownership_host";
  if (board_size < 2 || board_size > kMaxBoard)
    return set_error(MZGO_EINVAL, "%s: board_size %d (2..%d)", who, board_size, kMaxBoard);
  if (!stones || !owner) return set_error(MZGO_EINVAL, "%s: null %s", who, !stones ? "stones" : "owner");
  ownership_host(stones, board_size, owner);
  return MZGO_OK;
}

int mzgo_ownership_targets_host(const int8_t* final_stones, const uint8_t* flags, int L, int board_size, int start,
                                int symmetry, int unroll_steps, float* t_own, float* own_mask) {
  const char* who = "mzgo_ownership_targets_host";
  if (board_size < 2 || board_size > kMaxBoard)
    return set_error(MZGO_EINVAL, "%s: board_size %d (2..%d)", who, board_size, kMaxBoard);
  if (!final_stones || !flags || !t_own || !own_mask)
    return set_error(MZGO_EINVAL, "%s: null %s", who,
                     !final_stones ? "final_stones" : !flags ? "flags" : !t_own ? "t_own" : "own_mask");
  if (L < 0 || L > (1 << 30)) return set_error(MZGO_EINVAL, "%s: L %d outside 0..2^30", who, L);
  if (symmetry < 0 || symmetry > 7) return set_error(MZGO_EINVAL, "%s: symmetry %d (0..7)", who, symmetry);
  if (unroll_steps < 0 || unroll_steps > kMaxUnroll)
    return set_error(MZGO_EINVAL, "%s: unroll_steps %d out of range (0..%d)", who, unroll_steps, kMaxUnroll);
  const int N = board_size, CELLS = N * N;
  int8_t owner[kMaxBoard * kMaxBoard];
  ownership_host(final_stones, N, owner);
  for (int k = 0; k <= unroll_steps; ++k) {
    const long long at = (long long)start + k;
    const bool valid = own_row_valid(at, L, flags[L]);
    own_mask[k] = valid ? 1.f : 0.f;
    for (int c = 0; c < CELLS; ++c)
      t_own[(size_t)k * CELLS + c] = valid ? own_target(owner[sym_src(N, symmetry, c)], 1 + (flags[at] & 1)) : 0.f;
  }
  return MZGO_OK;
}

// every device call of the position ledger on a store that has none
static int positions_check(const mzgo_replay* r, const char* who) {
  if (!r) return set_error(MZGO_EINVAL, "%s: null replay", who);
  if (!r->positions)
    return set_error(MZGO_EINVAL, "%s: the store keeps no position weights (call mzgo_replay_enable_positions first)",
                     who);
  return MZGO_OK;
}

// the sampler's checks and its two launches (``who``: the entry point's name);
// ``positions``: the position sampler's two (mzgo_replay_sample_positions)
static int sample_launch(mzgo_replay* r, const char* who, bool positions, int B, uint64_t seed, uint32_t step,
                         int symmetries, double beta, int32_t* items, int32_t* index, uint32_t* gen, float* weight,
                         hipStream_t s) {
  if (!r) return set_error(MZGO_EINVAL, "%s: null replay", who);
  if (positions)
    if (int rc = positions_check(r, who)) return rc;
  if (B < 1) return set_error(MZGO_EINVAL, "%s: B must be >= 1, got %d", who, B);
  if (r->R.cap > kSampleMaxCap)
    return set_error(MZGO_EINVAL, "%s: capacity %d exceeds the sampler's 64^3 = %d slots", who, r->R.cap,
                     kSampleMaxCap);
  if (B > r->n_valid)
    return set_error(MZGO_EINVAL, "%s: B %d exceeds the %d stored games that have moves", who, B, r->n_valid);
  if (!(beta >= 0.0) || std::isinf(beta)) return set_error(MZGO_EINVAL, "%s: beta must be finite and >= 0", who);
  if (!items || !index || !gen)
    return set_error(MZGO_EINVAL, "%s: null %s", who, !items ? "items" : !index ? "index" : "gen");
  const SampleOut O{items, index, gen, weight};
  const uint64_t key = stream_key(seed, kSamplerDomain, step);
  const SumTree& T = r->T;
  if (positions) {
    hipLaunchKernelGGL(k_replay_possample_build, dim3(T.n1), dim3(kThreads), 0, s, T, r->P, r->R.length);
    RHIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_replay_possample_draw, dim3(1), dim3(64), 0, s, T, r->P, r->L.gen, r->R.length, r->head, B,
                       key, symmetries != 0, beta, O);
    RHIPCHK(hipGetLastError());
    return MZGO_OK;
  }
  hipLaunchKernelGGL(k_replay_sample_build, dim3((T.n1 + kThreads / 64 - 1) / (kThreads / 64)), dim3(kThreads), 0, s,
                     T, r->L.prio, r->R.length);
  RHIPCHK(hipGetLastError());
  hipLaunchKernelGGL(k_replay_sample_draw, dim3(1), dim3(64), 0, s, T, r->L.gen, r->R.length, r->head, B, key,
                     symmetries != 0, beta, r->n_valid, O);
  RHIPCHK(hipGetLastError());
  return MZGO_OK;
}

int mzgo_replay_sample(mzgo_replay* r, int B, uint64_t seed, uint32_t step, int symmetries, double beta,
                       int32_t* items, int32_t* index, uint32_t* gen, float* weight, void* stream) {
  return sample_launch(r, "mzgo_replay_sample", false, B, seed, step, symmetries, beta, items, index, gen, weight,
                       (hipStream_t)stream);
}

int mzgo_replay_sample_positions(mzgo_replay* r, int B, uint64_t seed, uint32_t step, int symmetries, double beta,
                                 int32_t* items, int32_t* index, uint32_t* gen, float* weight, void* stream) {
  return sample_launch(r, "mzgo_replay_sample_positions", true, B, seed, step, symmetries, beta, items, index, gen,
                       weight, (hipStream_t)stream);
}

// the two sampler twins' common argument checks (``wname``: what the weights
// ``w`` are called); *n_valid: the slots whose game has moves
static int sample_host_check(const char* who, int cap, const char* wname, const double* w, const int32_t* length,
                             const int32_t* items, const int32_t* index, int head, int B, double beta, int* n_valid) {
  if (cap < 1 || cap > kSampleMaxCap)
    return set_error(MZGO_EINVAL, "%s: capacity %d outside 1..64^3 = %d", who, cap, kSampleMaxCap);
  if (!w || !length || !items || !index)
    return set_error(MZGO_EINVAL, "%s: null %s", who, !w ? wname : !length ? "length" : !items ? "items" : "index");
  if (head < 0 || head >= cap) return set_error(MZGO_EINVAL, "%s: head %d outside 0..%d", who, head, cap - 1);
  if (B < 1) return set_error(MZGO_EINVAL, "%s: B must be >= 1, got %d", who, B);
  if (!(beta >= 0.0) || std::isinf(beta)) return set_error(MZGO_EINVAL, "%s: beta must be finite and >= 0", who);
  *n_valid = 0;
  for (int i = 0; i < cap; ++i) *n_valid += length[i] > 0;
  if (B > *n_valid)
    return set_error(MZGO_EINVAL, "%s: B %d exceeds the %d stored games that have moves", who, B, *n_valid);
  return MZGO_OK;
}
// draw t's outputs, as the draw kernels write them
static void sample_host_write(int32_t* items, int32_t* index, int t, int slot, int start, uint64_t key, int symmetries,
                              int head, int cap) {
  items[3 * t] = slot;
  items[3 * t + 1] = start;
  items[3 * t + 2] = sample_symmetry(key, t, symmetries != 0);
  index[t] = (slot - head + cap) % cap;
}

int mzgo_replay_sample_host(const double* prio, const int32_t* length, int cap, int head, int B, uint64_t seed,
                            uint32_t step, int symmetries, double beta, int32_t* items, int32_t* index,
                            float* weight) {
  const char* who = "mzgo_replay_sample_host";
  int n_valid = 0;
  if (int rc = sample_host_check(who, cap, "prio", prio, length, items, index, head, B, beta, &n_valid)) return rc;
  std::vector<double> leaf((size_t)cap);
  for (int i = 0; i < cap; ++i) {
    leaf[i] = length[i] > 0 ? prio[i] : 0.0;
    if (length[i] > 0 && !(prio[i] > 0.0 && !std::isinf(prio[i])))
      return set_error(MZGO_EINVAL, "%s: slot %d: weight %g (finite and > 0)", who, i, prio[i]);
  }
  SumTreeHost tree(std::move(leaf));                        // k_replay_sample_build and the draw kernel's prologue
  const uint64_t key = stream_key(seed, kSamplerDomain, step);
  std::vector<double> pick_w((size_t)B);
  double total0 = 0.0;
  for (int t = 0; t < B; ++t) {
    const TreePick d = tree.draw(sample_u(key, t));
    if (t == 0) total0 = d.total;
    pick_w[t] = d.w;
    sample_host_write(items, index, t, d.slot, sample_start(key, t, length[d.slot]), key, symmetries, head, cap);
  }
  if (weight) importance_weights_host(pick_w.data(), B, (double)n_valid, total0, beta, weight);
  return MZGO_OK;
}

int mzgo_replay_update_priorities(mzgo_replay* r, const int32_t* items, const uint32_t* gen, const float* per,
                                  const double* mean, int B, double alpha, void* stream) {
  if (!r) return set_error(MZGO_EINVAL, "mzgo_replay_update_priorities: null replay");
  if (B < 1) return set_error(MZGO_EINVAL, "mzgo_replay_update_priorities: B must be >= 1, got %d", B);
  if (!items || !gen)
    return set_error(MZGO_EINVAL, "mzgo_replay_update_priorities: null %s", !items ? "items" : "gen");
  if ((per != nullptr) == (mean != nullptr))
    return set_error(MZGO_EINVAL, "mzgo_replay_update_priorities: give per (a loss per sample) or mean (one value), "
                     "not %s", per ? "both" : "neither");
  if (!(alpha > 0.0) || std::isinf(alpha))
    return set_error(MZGO_EINVAL, "mzgo_replay_update_priorities: alpha must be finite and > 0");
  hipLaunchKernelGGL(k_replay_update_priorities, dim3((B + kThreads - 1) / kThreads), dim3(kThreads), 0,
                     (hipStream_t)stream, r->L, items, gen, per, mean, B, alpha);
  RHIPCHK(hipGetLastError());
  return MZGO_OK;
}

// logical order = the ring from ``head``: at most two runs of slots
// (entries of ``width`` bytes)
static int copy_logical(mzgo_replay* r, void* logical, void* slots, size_t width, bool to_slots, hipMemcpyKind kind,
                        hipStream_t s) {
  const int run = std::min(r->size, r->R.cap - r->head);
  const int n[2] = {run, r->size - run}, at[2] = {r->head, 0};
  for (int k = 0, done = 0; k < 2; done += n[k], ++k) {
    if (n[k] == 0) continue;
    char *a = (char*)logical + (size_t)done * width, *b = (char*)slots + (size_t)at[k] * width;
    RHIPCHK(hipMemcpyAsync(to_slots ? b : a, to_slots ? a : b, (size_t)n[k] * width, kind, s));
  }
  return MZGO_OK;
}

int mzgo_replay_priorities(mzgo_replay* r, double* prio, uint32_t* gen, void* stream) {
  if (!r) return set_error(MZGO_EINVAL, "mzgo_replay_priorities: null replay");
  hipStream_t s = (hipStream_t)stream;
  if (prio)
    if (int rc = copy_logical(r, prio, r->L.prio, sizeof(double), false, hipMemcpyDeviceToDevice, s)) return rc;
  if (gen)
    if (int rc = copy_logical(r, gen, r->L.gen, sizeof(uint32_t), false, hipMemcpyDeviceToDevice, s)) return rc;
  return MZGO_OK;
}

int mzgo_replay_set_priorities(mzgo_replay* r, const double* values_host, int n, void* stream) {
  if (!r) return set_error(MZGO_EINVAL, "mzgo_replay_set_priorities: null replay");
  if (!values_host) return set_error(MZGO_EINVAL, "mzgo_replay_set_priorities: null values");
  if (n != r->size)
    return set_error(MZGO_EINVAL, "mzgo_replay_set_priorities: %d values for the %d games held", n, r->size);
  for (int i = 0; i < n; ++i)
    if (!(values_host[i] > 0.0) || std::isinf(values_host[i]))
      return set_error(MZGO_EINVAL, "mzgo_replay_set_priorities: game %d: %g (finite values > 0 only)", i,
                       values_host[i]);
  hipStream_t s = (hipStream_t)stream;
  if (int rc = copy_logical(r, const_cast<double*>(values_host), r->L.prio, sizeof(double), true, hipMemcpyHostToDevice, s)) return rc;
  RHIPCHK(hipStreamSynchronize(s));                         // (the host buffer is the caller's)
  return MZGO_OK;
}

int mzgo_replay_skipped_updates(mzgo_replay* r, int64_t* count_host, void* stream) {
  if (!r || !count_host)
    return set_error(MZGO_EINVAL, "mzgo_replay_skipped_updates: null %s", !r ? "replay" : "count");
  unsigned c = 0;
  RHIPCHK(hipMemcpyAsync(&c, r->L.skipped, sizeof(c), hipMemcpyDeviceToHost, (hipStream_t)stream));
  RHIPCHK(hipStreamSynchronize((hipStream_t)stream));
  *count_host = c;
  return MZGO_OK;
}

// ---------------------------------------------------------------------------
// The position ledger's entry points
// ---------------------------------------------------------------------------
int mzgo_replay_enable_positions(mzgo_replay* r, int td_steps, double discount, double alpha, double floor,
                                 int init_mode, void* stream) {
  const char* who = "mzgo_replay_enable_positions";
  if (!r) return set_error(MZGO_EINVAL, "%s: null replay", who);
  if (r->R.M > kPositionMaxMoves)
    return set_error(MZGO_EINVAL, "%s: max_moves %d exceeds the two levels of 64 inside a game (%d)", who, r->R.M,
                     kPositionMaxMoves);
  if (r->R.cap > kSampleMaxCap)
    return set_error(MZGO_EINVAL, "%s: capacity %d exceeds the sampler's 64^3 = %d slots", who, r->R.cap,
                     kSampleMaxCap);
  if (td_steps < 1) return set_error(MZGO_EINVAL, "%s: td_steps must be >= 1, got %d", who, td_steps);
  if (!std::isfinite(discount)) return set_error(MZGO_EINVAL, "%s: discount must be finite", who);
  if (!(alpha > 0.0) || std::isinf(alpha)) return set_error(MZGO_EINVAL, "%s: alpha must be finite and > 0", who);
  if (!(floor >= 0.0) || std::isinf(floor))
    return set_error(MZGO_EINVAL, "%s: floor must be finite and >= 0 (0 = float32's smallest normal)", who);
  if (init_mode != POS_INIT_TD && init_mode != POS_INIT_UNIFORM)
    return set_error(MZGO_EINVAL, "%s: init_mode %d (0 = td, 1 = uniform)", who, init_mode);
  if (floor == 0.0) floor = kPriorityFloor;
  PosLedger& P = r->P;
  if (r->positions) {
    if (P.td_steps != td_steps || P.discount != discount || P.alpha != alpha || P.floor != floor ||
        P.init_mode != init_mode)
      return set_error(MZGO_EINVAL, "%s: already enabled with other parameters (td_steps %d, discount %g, alpha %g, "
                       "floor %g, init_mode %d)", who, P.td_steps, P.discount, P.alpha, P.floor, P.init_mode);
    return MZGO_OK;
  }
  hipStream_t s = (hipStream_t)stream;
  const size_t cap = r->R.cap, M = r->R.M;
  PosLedger Q{};
  Q.cap = r->R.cap; Q.M = r->R.M;
  Q.td_steps = td_steps; Q.init_mode = init_mode; Q.discount = discount; Q.alpha = alpha; Q.floor = floor;
  int rc = MZGO_OK;
  auto chk = [&](int x) { if (rc == MZGO_OK) rc = x; };
  chk(r->alloc(&Q.pprio, cap * M));
  chk(r->alloc(&Q.npos1, (size_t)r->T.n1));
  chk(r->alloc(&Q.n_pos, 1));
  if (rc != MZGO_OK) return rc;                             // (what was allocated is freed with the store)
  RHIPCHK(hipMemsetAsync(Q.pprio, 0, cap * M * sizeof(double), s));
  RHIPCHK(hipMemsetAsync(Q.n_pos, 0, sizeof(int), s));
  P = Q;
  r->positions = true;
  // the games the store already holds: the new-game rule, from the ring's head
  if (r->size > 0) return r->new_positions(r->head, r->size, s);
  return MZGO_OK;
}

int mzgo_replay_update_position_priorities(mzgo_replay* r, const int32_t* items, const uint32_t* gen,
                                           const float* value, const float* t_val, int B, int unroll_steps,
                                           void* stream) {
  const char* who = "mzgo_replay_update_position_priorities";
  if (int rc = positions_check(r, who)) return rc;
  if (B < 1) return set_error(MZGO_EINVAL, "%s: B must be >= 1, got %d", who, B);
  if (unroll_steps < 1 || unroll_steps > kMaxUnroll)
    return set_error(MZGO_EINVAL, "%s: unroll_steps %d out of range (1..%d)", who, unroll_steps, kMaxUnroll);
  if (B > (1 << 24)) return set_error(MZGO_EINVAL, "%s: B %d exceeds 2^24", who, B);
  if (!items || !gen || !value || !t_val)
    return set_error(MZGO_EINVAL, "%s: null %s", who, !items ? "items" : !gen ? "gen" : !value ? "value" : "t_val");
  const int K1 = unroll_steps + 1;
  hipLaunchKernelGGL(k_replay_update_position_priorities, dim3((B * K1 + kThreads - 1) / kThreads), dim3(kThreads), 0,
                     (hipStream_t)stream, r->P, r->L.gen, r->L.skipped, r->R.length, items, gen, value, t_val, B, K1);
  RHIPCHK(hipGetLastError());
  return MZGO_OK;
}

int mzgo_replay_position_priorities(mzgo_replay* r, double* pprio, void* stream) {
  const char* who = "mzgo_replay_position_priorities";
  if (int rc = positions_check(r, who)) return rc;
  if (!pprio) return set_error(MZGO_EINVAL, "%s: null pprio", who);
  return copy_logical(r, pprio, r->P.pprio, (size_t)r->P.M * sizeof(double), false, hipMemcpyDeviceToDevice,
                      (hipStream_t)stream);
}

int mzgo_replay_set_position_priorities(mzgo_replay* r, const double* values_host, int n, void* stream) {
  const char* who = "mzgo_replay_set_position_priorities";
  if (int rc = positions_check(r, who)) return rc;
  if (!values_host) return set_error(MZGO_EINVAL, "%s: null values", who);
  if (n != r->size) return set_error(MZGO_EINVAL, "%s: %d rows for the %d games held", who, n, r->size);
  const size_t M = r->P.M;
  for (int i = 0; i < n; ++i) {
    const int L = r->len[r->slot_of(i)];
    bool positive = false;
    for (int t = 0; t < L; ++t) {
      const double v = values_host[(size_t)i * M + t];
      if (!(v >= 0.0) || std::isinf(v))
        return set_error(MZGO_EINVAL, "%s: game %d, position %d: %g (finite values >= 0 only)", who, i, t, v);
      positive = positive || v > 0.0;
    }
    if (L > 0 && !positive)
      return set_error(MZGO_EINVAL, "%s: game %d has no position with a weight > 0", who, i);
  }
  hipStream_t s = (hipStream_t)stream;
  if (int rc = copy_logical(r, const_cast<double*>(values_host), r->P.pprio, M * sizeof(double), true,
                            hipMemcpyHostToDevice, s))
    return rc;
  RHIPCHK(hipStreamSynchronize(s));                         // (the host buffer is the caller's)
  return MZGO_OK;
}

int mzgo_replay_position_priorities_host(const double* reward, const double* root_value, int L, int td_steps,
                                         double discount, double alpha, double floor, double* pprio) {
  const char* who = "mzgo_replay_position_priorities_host";
  if (L < 0 || L > kPositionMaxMoves) return set_error(MZGO_EINVAL, "%s: L %d outside 0..%d", who, L, kPositionMaxMoves);
  if (!reward || (L > 0 && (!root_value || !pprio)))
    return set_error(MZGO_EINVAL, "%s: null %s", who, !reward ? "reward" : !root_value ? "root_value" : "pprio");
  if (td_steps < 1) return set_error(MZGO_EINVAL, "%s: td_steps must be >= 1, got %d", who, td_steps);
  if (!(alpha > 0.0) || std::isinf(alpha)) return set_error(MZGO_EINVAL, "%s: alpha must be finite and > 0", who);
  if (!(floor >= 0.0) || std::isinf(floor)) return set_error(MZGO_EINVAL, "%s: floor must be finite and >= 0", who);
  if (floor == 0.0) floor = kPriorityFloor;
  for (int t = 0; t < L; ++t)
    pprio[t] = position_td_priority(reward, root_value, L, t, td_steps, discount, floor, alpha);
  return MZGO_OK;
}

int mzgo_replay_sample_positions_host(const double* pprio, const int32_t* length, int cap, int M, int head, int B,
                                      uint64_t seed, uint32_t step, int symmetries, double beta, int32_t* items,
                                      int32_t* index, float* weight) {
  const char* who = "mzgo_replay_sample_positions_host";
  if (M < 1 || M > kPositionMaxMoves)
    return set_error(MZGO_EINVAL, "%s: max_moves %d outside 1..%d", who, M, kPositionMaxMoves);
  int n_valid = 0;
  if (int rc = sample_host_check(who, cap, "pprio", pprio, length, items, index, head, B, beta, &n_valid)) return rc;
  auto len_of = [&](int i) { return std::min(std::max(length[i], 0), M); };
  // k_replay_possample_build and the draw kernel's prologue
  long long n_pos = 0;
  std::vector<double> leaf((size_t)cap);
  double csum[64];
  for (int i = 0; i < cap; ++i) {
    const int L = len_of(i);
    const double* row = pprio + (size_t)i * M;
    for (int t = 0; t < L; ++t)
      if (!(row[t] >= 0.0) || std::isinf(row[t]))
        return set_error(MZGO_EINVAL, "%s: slot %d, position %d: weight %g (finite and >= 0)", who, i, t, row[t]);
    leaf[i] = L > 0 ? game_weight_host(row, L, csum) : 0.0;
    if (L > 0 && !(leaf[i] > 0.0 && !std::isinf(leaf[i])))
      return set_error(MZGO_EINVAL, "%s: slot %d: the game's weight is %g (finite and > 0)", who, i, leaf[i]);
    n_pos += L;
  }
  SumTreeHost tree(std::move(leaf));
  const uint64_t key = stream_key(seed, kSamplerDomain, step);
  std::vector<double> pick_w((size_t)B);
  double total0 = 0.0;
  for (int t = 0; t < B; ++t) {
    TreePick d = tree.draw(sample_u(key, t));
    if (t == 0) total0 = d.total;
    // the start, inside the game: its chunk sums, then the chunk's positions
    const int L = len_of(d.slot);
    const double* row = pprio + (size_t)d.slot * M;
    (void)game_weight_host(row, L, csum);
    const int jc = pick64_host(csum, 64, &d.target);
    const int nt = std::max(0, std::min(64, L - jc * 64));
    const int jt = pick64_host(nt > 0 ? row + (size_t)jc * 64 : row, nt, &d.target);
    pick_w[t] = jt < nt ? row[(size_t)jc * 64 + jt] : 0.0;
    sample_host_write(items, index, t, d.slot, std::max(std::min(jc * 64 + jt, L - 1), 0), key, symmetries, head, cap);
  }
  if (weight) importance_weights_host(pick_w.data(), B, (double)n_pos, total0, beta, weight);
  return MZGO_OK;
}

int mzgo_replay_symmetry_table(int board_size, int symmetry, int32_t* src_host, int32_t* dst_host) {
  if (board_size < 2 || board_size > kMaxBoard || symmetry < 0 || symmetry > 7)
    return set_error(MZGO_EINVAL, "mzgo_replay_symmetry_table: board_size %d (2..%d), symmetry %d (0..7)", board_size,
                     kMaxBoard, symmetry);
  const int cells = board_size * board_size;
  for (int c = 0; c < cells; ++c)
    if (src_host) src_host[c] = sym_src(board_size, symmetry, c);
  for (int a = 0; a <= cells; ++a)
    if (dst_host) dst_host[a] = sym_dst(board_size, symmetry, a);
  return MZGO_OK;
}

}  // extern "C"
