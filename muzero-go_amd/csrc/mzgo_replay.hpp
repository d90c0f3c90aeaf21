// mzgo_replay.hpp -- what the device replay store (mzgo_replay.hip) shares
// with the rest of the library: the eight board symmetries as index maps
// (host and device, so that the tables a test reads are the kernel's), and the
// ring's arrays and the ingest of one game (a device function: the store's
// own ingest kernel and k_selfplay_games run the same text), the device
// priority ledger, the one sum tree both samplers draw from (its scratch, its
// order of additions, descent rule and fallback, host and device; its host
// serial form -- build, one draw with the leaf's removal, importance weights
// -- which both samplers' host twins run), the position
// ledger and its weight rules (host and device likewise), the item list the
// assembly kernels take with its one decode, its two row predicates and the
// plane rule of a stored row (host and device likewise), the window
// of a sample and the item list of a batch's windows (host and device
// likewise) with the in-place reanalysis queue's arguments, the search-value
// target rule and the value rows it reads (host and device), the ownership
// rule of a final board and its targets (host and device), and the engine's
// side of the store's engine-facing calls (mzgo_capi.hip owns struct
// mzgo_engine and the thread-local error string).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <utility>
#include <vector>

#include "mzgo_common.hpp"

struct mzgo_engine;

namespace mzgo {

// Symmetry s (0..7) maps a plane x [N][N] to
//   y = np.rot90(x, s & 3, axes=(-2, -1)), then np.flip(y, axis=-1) if s & 4.
// sym_src: the cell of x that output cell c of y shows (y.flat[c] = x.flat[sym_src]).
__host__ __device__ __forceinline__ int sym_src(int N, int s, int c) {
  int i = c / N, j = c - i * N;
  if (s & 4) j = N - 1 - j;
  for (int k = s & 3; k > 0; --k) {      // one rot90: y[i][j] = x[j][N-1-i]
    const int t = i;
    i = j;
    j = N - 1 - t;
  }
  return i * N + j;
}
// sym_dst: where cell a of x lands in y (the inverse map: an action's one-hot);
// the pass action N*N stays put.
__host__ __device__ __forceinline__ int sym_dst(int N, int s, int a) {
  if (a >= N * N) return a;
  int i = a / N, j = a - i * N;
  for (int k = s & 3; k > 0; --k) {      // x[i][j] shows at y[N-1-j][i]
    const int t = i;
    i = N - 1 - j;
    j = t;
  }
  if (s & 4) j = N - 1 - j;
  return i * N + j;
}

// The finished games of an engine's slots, as the store's ingest kernel reads
// them (EngineArrays' record fields and board slots; mzgo_move.hpp).
struct ReplayEngineView {
  int N, G, M;                 // board size, game slots, max_moves
  int latent_dim, tower;       // 0 = board-only engine; 1 = tower engine
  int game_base, epoch;        // the games' RNG key: (game_base + g) ^ (epoch << 24)
  const int8_t* stones;        // [G][CELLS]   the boards after the last move
  const uint8_t* invd;         // [G][CELLS]
  const int* meta;             // [G][4] turn, passed, done, moves
  const int8_t* rec_stones;    // [G][M][CELLS]
  const uint8_t* rec_invd;     // [G][M][CELLS]
  const uint8_t* rec_flags;    // [G][M]
  const int* rec_action;       // [G][M]
  const double* rec_value;     // [G][M]
  const double* rec_policy;    // [G][M][A]
  const double* rec_reward;    // [G][M]
  const double* final_reward;  // [G]
};

// The ring's arrays (device), one allocation per field over all slots.
// M = max_moves, CELLS = N^2, A = CELLS + 1; a game of length L uses position
// rows 0..L (the L searched positions, then the final board), L actions,
// policy rows and root values, and L + 1 rewards (the winner last).
struct Store {
  int N, CELLS, A, M, cap;
  int8_t* stones;      // [cap][M+1][CELLS]
  uint8_t* invd;       // [cap][M+1][CELLS]
  uint8_t* flags;      // [cap][M+1]
  int* action;         // [cap][M]
  double* policy;      // [cap][M][A]
  double* reward;      // [cap][M+1]
  double* root_value;  // [cap][M]
  int* length;         // [cap]
  int* key_gid;        // [cap]
};

// Ingest of one game: engine slot g -> ring slot ``slot`` under the key id
// ``key_gid`` (trajectory_from_record's rules, mzgo/trainer.py), by a team of
// ``nt`` threads, this one ``tid``: k_replay_ingest's workgroup (one per game
// after the launch that played it) and k_selfplay_games' (the game's own, at
// the game's end).  The caller has made the slot's record and board visible
// to the team.
__device__ __forceinline__ void replay_ingest_game(const Store& R, const ReplayEngineView& E, int g, int slot,
                                                   int key_gid, int tid, int nt) {
  const int* mm = E.meta + (size_t)g * 4;
  const int done = mm[2] != 0;
  int L = mm[3];
  L = L < 0 ? 0 : L > R.M ? R.M : L;
  const int CELLS = R.CELLS, A = R.A;
  const size_t src = (size_t)g * E.M, pos = (size_t)slot * (R.M + 1), mv = (size_t)slot * R.M;
  for (int i = tid; i < L * CELLS; i += nt) {
    R.stones[pos * CELLS + i] = E.rec_stones[src * CELLS + i];
    R.invd[pos * CELLS + i] = E.rec_invd[src * CELLS + i];
  }
  for (int c = tid; c < CELLS; c += nt) {                 // the board after the last move
    R.stones[(pos + L) * CELLS + c] = E.stones[(size_t)g * CELLS + c];
    R.invd[(pos + L) * CELLS + c] = E.invd[(size_t)g * CELLS + c];
  }
  for (int i = tid; i < L * A; i += nt) R.policy[mv * A + i] = E.rec_policy[src * A + i];
  // -0.5 on the last move of a game that hit the move cap (main.py:699-702)
  const bool capped = !done && L >= E.M && L > 0;
  for (int t = tid; t < L; t += nt) {
    R.flags[pos + t] = E.rec_flags[src + t];
    R.action[mv + t] = E.rec_action[src + t];
    R.root_value[mv + t] = E.rec_value[src + t];
    const double r = E.rec_reward[src + t];
    R.reward[pos + t] = capped && t == L - 1 ? r + -0.5 : r;
  }
  if (tid == 0) {
    R.flags[pos + L] = (uint8_t)((mm[0] & 1) | ((mm[1] & 1) << 1) | (done << 2));
    R.reward[pos + L] = done ? E.final_reward[g] : 0.0;       // env.winner(): 0 unless ended
    R.length[slot] = L;
    R.key_gid[slot] = key_gid;
  }
}

// One mzgo_replay_play_games call: the game queue of k_selfplay_games
// (mzgo_kernels.hpp).  Queue game j is slot j % G of epoch epoch0 + j / G and
// lands in ring slot (first + j) % R.cap.
struct GamesArgs {
  int n;             // games in the queue
  int G;             // the engine's game slots
  int epoch0;        // the call's first epoch
  int first;         // ring slot of game 0
  unsigned* head;    // the queue head (zeroed before the launch)
  int* error;        // the smallest j whose game stopped on a board error (>= n before the launch)
  Store R;
};

// ---------------------------------------------------------------------------
// An item list: i32 [B][3] on the device, sample b = (slot, start, symmetry) --
// a ring slot, the move the sample starts from and one of the eight symmetries
// above.  mzgo_replay_items writes one from host (game, start, symmetry) triples
// it has checked against the host mirror, the samplers write one from their
// draws; the three assembly kernels (k_replay_batch, k_replay_ownership,
// k_replay_window_obs) and the priority updates read one, a workgroup per
// sample.  The kernels check nothing else: sample_window is their one decode,
// and a row of the store is read only where one of the two predicates below
// holds, whatever the list holds.  Host and device: tools/replay_twins_check.cpp
// runs them on a store image in host memory.
// ---------------------------------------------------------------------------
struct SampleWindow {
  int slot, start, sym;  // the triple; sym & 7
  bool held;             // the slot is one of the ring's
  int L;                 // the game's moves, 0..M (0 when not held)
  size_t pos, mv;        // the game's first position row and first move row (0 when not held)
};
__host__ __device__ __forceinline__ SampleWindow sample_window(const Store& R, const int* items, int b) {
  SampleWindow w;
  w.slot = items[3 * b];
  w.start = items[3 * b + 1];
  w.sym = items[3 * b + 2] & 7;
  w.held = w.slot >= 0 && w.slot < R.cap;
  const int L = w.held ? R.length[w.slot] : 0;
  w.L = L < 0 ? 0 : L > R.M ? R.M : L;
  w.pos = w.held ? (size_t)w.slot * (R.M + 1) : 0;
  w.mv = w.held ? (size_t)w.slot * R.M : 0;
  return w;
}
// position row ``at`` (stones, invd, flags, reward: rows 0..L, the final board last) may be read
__host__ __device__ __forceinline__ bool window_position(const SampleWindow& w, long long at) {
  return w.held && at >= 0 && at <= w.L;
}
// move row ``j`` (action, policy, root_value: rows 0..L-1) may be read
__host__ __device__ __forceinline__ bool window_move(const SampleWindow& w, long long j) {
  return w.held && j >= 0 && j < w.L;
}

// Plane p (0..5: black, white, turn, invalid, passed, done) of the observation
// of a stored position, at the row's cell ``src``: ``stones`` and ``invd`` are
// the row's [CELLS], ``flags`` its byte.  mzgo.reanalyse.observation_planes is
// the same rule on the host.
__host__ __device__ __forceinline__ float observation_plane(const int8_t* stones, const uint8_t* invd, int flags, int p,
                                                            int src) {
  switch (p) {
    case 0: return stones[src] == 1;
    case 1: return stones[src] == 2;
    case 2: return flags & 1;
    case 3: return invd[src];
    case 4: return (flags >> 1) & 1;
    default: return (flags >> 2) & 1;
  }
}

// ---------------------------------------------------------------------------
// The window of a sample (slot, start, symmetry) under K unroll steps: the
// stored policy rows k_replay_batch reads for it, t = start .. min(start + K,
// L - 1) with L = length[slot] (rows past the game's end are the uniform row
// and are not stored).  A triple whose slot is outside 0 .. cap - 1, whose game
// is empty (L <= 0) or whose start is outside 0 .. L - 1 has no window.  The
// item list of a batch is every (slot, t) of every window by falling t, equal
// t by batch position b: latest first (mzgo.reanalyse.latest_first), the order
// mzgo_replay_reanalyse queues whole games in.  Host and device: the builder
// kernel (k_replay_window_items) and its host twin run these.
// ---------------------------------------------------------------------------
// the window's rows (its first is ``start``); 0 = the triple contributes nothing
__host__ __device__ __forceinline__ int window_rows(const int* length, int cap, int slot, int start, int K) {
  if (slot < 0 || slot >= cap) return 0;
  const int L = length[slot];
  if (L <= 0 || start < 0 || start >= L) return 0;
  const int last = start + K < L - 1 ? start + K : L - 1;
  return last - start + 1;
}
// whether row t belongs to the window of ``rows`` rows from ``start`` (rows > 0: 0 <= start)
__host__ __device__ __forceinline__ bool window_has(int start, int rows, int t) {
  return rows > 0 && t >= start && t - start < rows;
}

// ---------------------------------------------------------------------------
// Search-value targets (mzgo.h: mzgo_replay_batch_items_values): the n-step return of
// trajectory index i >= 0 of a game of L moves, bootstrapped from the stored
// root value of the position n = td_steps >= 1 moves on.  reward [L + 1] (the
// winner last), root_value [L].  f64, one multiply and one add per step in
// this order (no contraction: the unit's -ffp-contract=off), so the float is
// defined bit for bit; k_replay_batch<true> and the host twin run this text.
//   i + n <= L - 1   a searched position: its root value
//   i + n == L       the final board was never searched: r[L], all that is
//                    left of its return (network targets evaluate that board)
//   i + n >  L       nothing past the rewards
// ---------------------------------------------------------------------------
__host__ __device__ __forceinline__ float search_value_target(const double* reward, const double* root_value, int L,
                                                              int i, int n, double discount) {
  double target = 0.0, factor = 1.0;
  for (int k = 0; k < n; ++k) {
    const long long j = (long long)i + k;
    if (j > L) break;
    target += factor * reward[j];
    factor *= discount;
  }
  const long long at = (long long)i + n;
  if (at <= L - 1) target += factor * root_value[at];
  else if (at == L) target += factor * reward[L];
  return (float)target;
}
// The value rows of a sample under search-value targets: the stored root values
// its K + 1 targets read, t = start + n .. min(start + K + n, L - 1), for a
// triple that has a window (window_rows > 0).  Returns their count (0 = none:
// start + n > L - 1) and their first in *first.  A sample's rows are its
// window together with its value rows, each row once: for n <= K + 1 the two
// ranges overlap or touch, for n > K + 1 a gap lies between them.
__host__ __device__ __forceinline__ int value_rows(const int* length, int cap, int slot, int start, int K, int n,
                                                   int* first) {
  *first = 0;
  if (window_rows(length, cap, slot, start, K) == 0) return 0;
  const int L = length[slot];
  const long long lo = (long long)start + n, hi = lo + K;
  if (lo > L - 1) return 0;
  *first = (int)lo;
  return (int)((hi < L - 1 ? hi : L - 1) - lo) + 1;
}
// whether row t is one of a sample's rows (its window, or its value rows past the window)
__host__ __device__ __forceinline__ bool sample_has(int start, int rows, int vfirst, int vrows, int t) {
  return window_has(start, rows, t) || window_has(vfirst, vrows, t);
}

// ---------------------------------------------------------------------------
// Ownership targets (mzgo.h: mzgo_replay_ownership_items): who owns each point of a
// game's final board under the area rule (oracle/gogame.py: areas, cell by
// cell).  A stone is owned by its colour (1 black, 2 white); an empty point by
// the one colour its empty region touches, by nobody (0) when the region
// touches both or none.  The region's colours are found as a fixed point: a
// mask of reached colours per empty cell (bit 0 black, bit 1 white -- a stone's
// colour IS its mask), each pass OR-ing in the four neighbours' masks of the
// pass before, until a pass changes nothing.  OR is monotone, so the fixed
// point does not depend on the order of visits, and at most CELLS passes reach
// it.  k_replay_ownership and the host twin run these functions.
// ---------------------------------------------------------------------------
// what a neighbour hands on: its colour if it is a stone, its reached mask if empty
__host__ __device__ __forceinline__ int own_seen(const int8_t* stones, const uint8_t* reach, int n) {
  return stones[n] ? (stones[n] & 3) : reach[n];
}
// one pass at the empty cell c: the masks of its neighbours OR-ed into its own
__host__ __device__ __forceinline__ int own_reach_step(const int8_t* stones, const uint8_t* reach, int N, int c) {
  const int i = c / N, j = c - i * N;
  int m = reach[c];
  if (i > 0) m |= own_seen(stones, reach, c - N);
  if (i < N - 1) m |= own_seen(stones, reach, c + N);
  if (j > 0) m |= own_seen(stones, reach, c - 1);
  if (j < N - 1) m |= own_seen(stones, reach, c + 1);
  return m;
}
// the owner of a cell from its stone and, where it is empty, its region's mask at the fixed point
__host__ __device__ __forceinline__ int own_owner(int stone, int reach) {
  return stone ? (stone & 3) : reach == 1 ? 1 : reach == 2 ? 2 : 0;
}
// whether unroll step k of a sample has an ownership target: position at = start + k is one of the game's
// L + 1 rows and the game ended (the done bit of the final row's flags: the condition for reward[L] = the winner)
__host__ __device__ __forceinline__ bool own_row_valid(long long at, int L, int final_flags) {
  return at >= 0 && at <= L && ((final_flags >> 2) & 1);
}
// the target of a cell owned by ``owner`` (0 nobody) seen by ``mover``, the colour to move (1 or 2)
__host__ __device__ __forceinline__ float own_target(int owner, int mover) {
  return owner == 0 ? 0.f : owner == mover ? 1.f : -1.f;
}
// host serial form: owner [CELLS] of stones [CELLS]; two buffers, a pass reads one and writes the other
inline void ownership_host(const int8_t* stones, int N, int8_t* owner) {
  const int CELLS = N * N;
  uint8_t reach[2][19 * 19] = {};
  int cur = 0;
  for (int pass = 0; pass <= CELLS; ++pass) {
    bool changed = false;
    for (int c = 0; c < CELLS; ++c) {
      const int m = stones[c] ? 0 : own_reach_step(stones, reach[cur], N, c);
      changed |= m != reach[cur][c];
      reach[cur ^ 1][c] = (uint8_t)m;
    }
    cur ^= 1;
    if (!changed) break;
  }
  for (int c = 0; c < CELLS; ++c) owner[c] = (int8_t)own_owner(stones[c], reach[cur][c]);
}

// One mzgo_replay_reanalyse_sample call: the in-place form of the reanalysis
// queue (k_reanalyse_queue<N, C, true>, mzgo_kernels.hpp).  Item i is row
// items[i][1] of ring slot items[i][0]: the position is read from R's rows, the
// fresh policy row and root value are written into R's.
struct ReanalyseStoreArgs {
  const int* items;  // [*n][2] (slot, t): k_replay_window_items' list
  const int* n;      // the list's length, a device word
  unsigned* head;    // the queue head (zeroed before the launch)
  Store R;
};

// ---------------------------------------------------------------------------
// The device priority ledger and its sampler (mzgo_replay.hip: k_replay_sample_*,
// k_replay_update_priorities; mzgo.h: mzgo_replay_sample).  Kept apart from
// Store, which the ingest and self-play kernels take by value.
// ---------------------------------------------------------------------------
struct Ledger {
  int cap;             // slots
  double* prio;        // [cap]  the sampling weight (already raised to alpha); 1.0 for a new game
  uint32_t* gen;       // [cap]  + 1 whenever a game is written into the slot
  unsigned* skipped;   // [1]    priority updates refused (a loss that is not finite or < 0)
};
// The sampler's scratch and nothing else: the 64-ary sum tree a draw descends
// (leaves = slots, level 1 = sums of 64 leaves; level 2, sums of 64 of those,
// lives in the draw kernel's lanes).  The store owns one; the game sampler and
// the position sampler both build it and draw from it (calls on one store are
// ordered, mzgo.h), each with its own leaves: a game's weight.
struct SumTree {
  int cap, n1;         // slots; level-1 entries = ceil(cap / 64)
  double* leaf;        // [cap]  length > 0 ? the game's weight : 0, picked leaves zeroed
  double* l1;          // [n1]   the sums of 64 leaves
  double* pick_w;      // [cap]  the picked games' (or positions') weights, in draw order
};
// one draw from the tree (host and device forms: SumTreeHost::draw, tree_draw in mzgo_replay.hip)
struct TreePick {
  int slot;            // the picked leaf
  double w;            // its weight, before the draw removed it
  double target;       // what is left of the target below the leaf: the position sampler descends on with it
  double total;        // the tree's total before the draw
};

constexpr double kDoubleMax = 1.79769313486231570815e308;   // x <= kDoubleMax: x is finite (and no NaN)
constexpr uint32_t kSamplerDomain = 0x53414D50u;   // stream_key's "game" word of the sampler's draws
constexpr int kSampleMaxCap = 64 * 64 * 64;        // three levels of 64
enum : uint32_t { TAG_SAMPLE = 5, TAG_START = 6, TAG_SYM = 7 };

// The sampler adds 64 entries x[0..63] (past the array's end: 0) in ONE order,
// the inclusive scan p of six steps d = 1, 2, 4, 8, 16, 32:
//   p[i] <- (i >= d ? p[i - d] : 0) + p[i]      for all i at once, from p = x
// (a wave does a step with one lane shift; the host twin with a copy).  The
// sum of the 64 is p[63].  Only + on doubles: the same bits everywhere.
__host__ __device__ __forceinline__ double scan_step(int i, int d, double own, double below) {
  return i >= d ? below + own : own;
}
// The descent rule at one level, from two 64-bit masks over the entries:
// ``over`` = entry is non-zero and its inclusive prefix exceeds the target,
// ``nonzero`` = entry is non-zero.  The first ``over`` entry; if rounding left
// none, the last non-zero one; 0 for an all-zero group (which the callers
// exclude: no more draws than games with a weight).
__host__ __device__ __forceinline__ int pick_entry(uint64_t over, uint64_t nonzero) {
  if (over) return __builtin_ctzll(over);
  if (nonzero) return 63 - __builtin_clzll(nonzero);
  return 0;
}
// the draws of sample t under ``key`` = stream_key(seed, kSamplerDomain, step)
__host__ __device__ __forceinline__ double sample_u(uint64_t key, int t) { return u01(draw(key, TAG_SAMPLE, (uint64_t)t)); }
__host__ __device__ __forceinline__ int sample_start(uint64_t key, int t, int length) {
  return (int)randbelow(draw(key, TAG_START, (uint64_t)t), (uint32_t)length);
}
__host__ __device__ __forceinline__ int sample_symmetry(uint64_t key, int t, int symmetries) {
  return symmetries ? (int)randbelow(draw(key, TAG_SYM, (uint64_t)t), 8u) : 0;
}
constexpr double kPriorityFloor = 1.17549435082228750797e-38;   // float32's smallest normal
// the stored priority of a loss ``p`` (finite, >= 0): floored at float32's
// smallest normal, then raised to alpha (exactly the floored value at alpha 1)
__host__ __device__ __forceinline__ double priority_of(double p, double alpha) {
  const double v = p > kPriorityFloor ? p : kPriorityFloor;
  return alpha == 1.0 ? v : pow(v, alpha);
}

// ---------------------------------------------------------------------------
// The position ledger (opt-in: mzgo_replay_enable_positions): a sampling weight
// per stored POSITION, and a sampler that draws (game, start) with probability
// w[game][start] / total (mzgo_replay.hip: k_replay_new_positions,
// k_replay_possample_*, k_replay_update_position_priorities).  Kept apart from
// Store and Ledger, which the existing kernels take by value; allocated only
// when enabled.  The generations and the count of refused updates are Ledger's,
// the tree the draw descends over the games' weights is the store's SumTree.
//
// A game's weight is not stored: it is formed from rows 0 .. L - 1 of its pprio
// row in the sampler's one order of additions -- chunks of 64 positions, a
// chunk's sum element 63 of the six-step scan, the game's weight element 63 of
// the scan over its <= 64 chunk sums, entries past the end 0 -- by the build
// kernel and again by the draw, so both hold the same bits.
// ---------------------------------------------------------------------------
constexpr int kPositionMaxMoves = 64 * 64;         // two levels of 64 inside a game
enum : int { POS_INIT_TD = 0, POS_INIT_UNIFORM = 1 };
struct PosLedger {
  int cap, M;          // slots; max_moves (pprio's row length)
  int td_steps;        // the n of a new position's |root value - n-step target|
  int init_mode;       // POS_INIT_TD, or POS_INIT_UNIFORM: 1.0 for every new position
  double discount, alpha, floor;
  double* pprio;       // [cap][M]  position t's sampling weight (already raised to alpha); rows t >= length: never read
  int* npos1;          // [ceil(cap / 64)]  sampler scratch: the moves of 64 slots' games
  int* n_pos;          // [1]    the stored positions at the last draw (the sum of npos1)
};
// the stored weight of a position whose value error is ``err`` (finite, >= 0):
// floored, then raised to alpha (exactly the floored value at alpha 1)
__host__ __device__ __forceinline__ double position_priority_of(double err, double floor, double alpha) {
  const double v = err > floor ? err : floor;
  return alpha == 1.0 ? v : pow(v, alpha);
}
// a new position's weight under POS_INIT_TD: position t of a game of L moves
// (reward [L + 1], root_value [L]), from search_value_target itself
__host__ __device__ __forceinline__ double position_td_priority(const double* reward, const double* root_value, int L,
                                                                int t, int td_steps, double discount, double floor,
                                                                double alpha) {
  const double err = fabs(root_value[t] - (double)search_value_target(reward, root_value, L, t, td_steps, discount));
  // (a stored value that is not finite: the floor, so that the position can still be drawn)
  return position_priority_of(err <= kDoubleMax ? err : floor, floor, alpha);
}

// host serial forms of the scan and of one level's pick (the twin's)
inline void scan64_host(const double* x, int n, double* p) {
  double a[64], b[64];
  for (int i = 0; i < 64; ++i) a[i] = i < n ? x[i] : 0.0;
  for (int d = 1; d < 64; d <<= 1) {
    for (int i = 0; i < 64; ++i) b[i] = scan_step(i, d, a[i], i >= d ? a[i - d] : 0.0);
    for (int i = 0; i < 64; ++i) a[i] = b[i];
  }
  for (int i = 0; i < 64; ++i) p[i] = a[i];
}
// picks among x[0..n) for *target; on return *target is the remainder for the level below
inline int pick64_host(const double* x, int n, double* target) {
  double p[64];
  scan64_host(x, n, p);
  uint64_t over = 0, nonzero = 0;
  for (int i = 0; i < n && i < 64; ++i) {
    if (x[i] > 0.0) nonzero |= 1ull << i;
    if (x[i] > 0.0 && p[i] > *target) over |= 1ull << i;
  }
  const int j = pick_entry(over, nonzero);
  *target = *target - (j > 0 ? p[j - 1] : 0.0);
  return j;
}

// host serial form of a game's weight from its position weights row[0..L): the
// <= 64 chunk sums in csum[64] (the rest 0), the weight returned
inline double game_weight_host(const double* row, int L, double* csum) {
  double p[64];
  for (int c = 0; c < 64; ++c) csum[c] = 0.0;
  for (int c = 0; c < 64 && c * 64 < L; ++c) {
    scan64_host(row + (size_t)c * 64, L - c * 64 < 64 ? L - c * 64 : 64, p);
    csum[c] = p[63];
  }
  scan64_host(csum, 64, p);
  return p[63];
}

// host serial form of the tree (both twins'): the build kernels' tail and the
// draw kernels' prologue, one draw, and the importance weights
struct SumTreeHost {
  int cap;
  std::vector<double> leaf, l1;          // [cap]; [n2 * 64], the entries past ceil(cap / 64): 0
  double x2[64] = {0.0};                 // level 2
  explicit SumTreeHost(std::vector<double> leaves) : cap((int)leaves.size()), leaf(std::move(leaves)) {
    const int n1 = (cap + 63) / 64, n2 = (n1 + 63) / 64;
    double p[64];
    l1.assign((size_t)n2 * 64, 0.0);
    for (int g = 0; g < n1; ++g) {
      scan64_host(leaf.data() + (size_t)g * 64, cap - g * 64 < 64 ? cap - g * 64 : 64, p);
      l1[g] = p[63];
    }
    for (int g = 0; g < n2; ++g) {
      scan64_host(l1.data() + (size_t)g * 64, 64, p);
      x2[g] = p[63];
    }
  }
  // target = u x total descends the three levels; the picked leaf is removed
  // and its two ancestors are summed again, never subtracted from
  TreePick draw(double u) {
    double p[64];
    scan64_host(x2, 64, p);
    TreePick d{0, 0.0, u * p[63], p[63]};
    const int j2 = pick64_host(x2, 64, &d.target);
    const int j1 = pick64_host(l1.data() + (size_t)j2 * 64, 64, &d.target);
    const int g1 = j2 * 64 + j1;
    const int n0 = cap - g1 * 64 < 0 ? 0 : cap - g1 * 64 < 64 ? cap - g1 * 64 : 64;
    const int j0 = pick64_host(leaf.data() + (size_t)g1 * 64, n0, &d.target);
    d.slot = g1 * 64 + j0 < cap - 1 ? g1 * 64 + j0 : cap - 1;
    d.w = leaf[d.slot];
    leaf[d.slot] = 0.0;
    scan64_host(leaf.data() + (size_t)g1 * 64, n0, p);
    l1[g1] = p[63];
    scan64_host(l1.data() + (size_t)j2 * 64, 64, p);
    x2[j2] = p[63];
    return d;
  }
};
// the importance weights of B draws from their picked weights, out of a
// population of n and the total before any removal: (n w / total0)^-beta over
// the batch's largest
inline void importance_weights_host(const double* pick_w, int B, double n, double total0, double beta, float* weight) {
  double vmax = 0.0;
  for (int b = 0; b < B; ++b) vmax = std::max(vmax, std::pow(n * pick_w[b] / total0, -beta));
  for (int b = 0; b < B; ++b) weight[b] = (float)(std::pow(n * pick_w[b] / total0, -beta) / vmax);
}

// mzgo_capi.hip: fill *v from an engine (no checks beyond the null pointer)
void replay_engine_view(const mzgo_engine* eng, ReplayEngineView* v);
// mzgo_capi.hip: whether a noise hook (mzgo_selfplay_inject_noise / _record_noise) is set
bool engine_noise_hooked(const mzgo_engine* eng);
// mzgo_capi.hip: enqueue k_selfplay_games for ga (head and error are set here)
// and move the engine's epoch to the last one the call plays
int engine_play_games(mzgo_engine* eng, const GamesArgs& ga, hipStream_t s);
// mzgo_capi.hip: enqueue the in-place reanalysis queue for ra (the head is set
// here) on min(max_items, CUs, tree slots) workgroups, after the weights'
// upload if one is due (MZGO_ENOWEIGHTS as mzgo_search); a reference-network
// engine only (the caller refuses the others)
int engine_reanalyse_store(mzgo_engine* eng, const ReanalyseStoreArgs& ra, int max_items, hipStream_t s);
// mzgo_capi.hip: set mzgo_last_error()'s text and return ``code``
int set_error(int code, const char* fmt, ...);

}  // namespace mzgo
