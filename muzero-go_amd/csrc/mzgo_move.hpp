// mzgo_move.hpp -- one self-play move's record protocol (run_self_play_game's
// loop body, self_play.py:465-507), defined once for every schedule that
// plays moves: k_selfplay_move (a workgroup per game), k_selfplay_games (a
// workgroup per slot, games from a queue), k_selfplay_boards + k_search_queue
// (the move-parallel epoch) and the tower engine's k_tobs + k_tchoose.
//
// A move is: record the observation, derive the move's RNG key, build the
// legal mask, (search,) choose and record the action, step and score the
// board, write the status, result and counters.  Everything here is a
// contract with the host, which reads it back in mzgo_records_export,
// mzgo_records_pack and mzgo_selfplay_counters -- so the kernels call these
// functions and spell none of it out themselves.
//
// The team parameter T (mzgo_board.hpp: id, SIZE, sync, any, leader) is the
// set of threads that runs a function: BoardWG<G>, the whole workgroup of
// G::THREADS, unless the caller says otherwise.
#pragma once
#include "mzgo_board.hpp"
#include "mzgo_search.hpp"

namespace mzgo {

constexpr int kCounters = 14;   // EngineArrays::counters

// Per-slot device state of an engine (sizes fixed at engine creation).
struct EngineArrays {
  int S;                 // simulations per move this engine was sized for
  int max_moves;
  // search state
  float* pool;           // [G][S+2][C*CS] per node: latent [C][CS] (direct dynamics) or conv
                         // output Y [CELLS][C] (factored); slot S+1: scratch latent
  float* prior;          // [G][S+1][A]
  int* child;            // [G][S+1][A]
  int* visits;           // [G][S+1]
  double* wsum;          // [G][S+1]
  double* root_prior;    // [G][A]
  int* path;             // [G][S+2]
  int* nodes;            // [G]  nodes used by the last search
  int* nact;             // [G][S+1] action that created each node (factored: rebuilds its latent)
  double* cval;          // [G][S+1][A] per (leaf, action): the child's backup value, kept when a batch at
                         // the leaf was cut (LDS trees; null: no value cache, 19x19 and direct dynamics)
  // boards
  int8_t* stones;        // [G][CELLS]
  uint8_t* invd;         // [G][CELLS]
  int* meta;             // [G][4] BoardMeta
  // self-play records
  int8_t* rec_stones;    // [G][M][CELLS]
  uint8_t* rec_invd;     // [G][M][CELLS]
  uint8_t* rec_flags;    // [G][M]   bit0 turn, bit1 passed, bit2 done, bit3 searched with the fast budget
  int* rec_action;       // [G][M]
  double* rec_value;     // [G][M]
  double* rec_policy;    // [G][M][A]
  double* rec_reward;    // [G][M]
  int* game_len;         // [G]
  double* final_reward;  // [G]
  int* status;           // [G]  0 playing, 1 finished, >=16 error
  unsigned char* jobs;   // [G][job_bytes(A)] a job slot per game (mzgo_jobs.hpp: JobHeader + regions): the
                         // work a game's workgroup shares with helper workgroups
  int* mpq;              // [2G + 1] move-parallel epoch (k_search_queue): per game (first move,
                         // moves played) of k_selfplay_boards, then the queue head
  unsigned long long* counters;  // [kCounters] 0: simulations run, 1: moves played, 2: games finished,
                                 //     3: dynamics convs run (factored: one per new parent; tower
                                 //     engines: towers evaluated, speculative ones included),
                                 //     4: of those, tail conv jobs (conv_tail), 5: prior rows formed,
                                 //     6: game workgroups started (k_selfplay_move, k_selfplay_games),
                                 //     7: tail helpers whose bounded wait for a job expired (tail_help), 8: expired
                                 //     mzgo_stream_wait_started gates (reported, then cleared),
                                 //     9: children of sim_loop's speculative batches expanded, 10: of such
                                 //     batches' children, taken from cval instead, 11: such batches cut short
                                 //     by their replay (mzgo_search_stats), 12 / 13: arrival convs
                                 //     (sim_loop) whose parent's Y came from its LDS copy / from L2
                                 //     (mzgo_search_stats2)
  unsigned long long* stamps;    // [G][kStampPhases] phase cycles (MZGO_STAMPS builds only)
};

struct PlayParams {
  double temperature;     // 1.0
  int temperature_moves;  // 15
  double komi;            // 0
  int game_base;          // global id of slot 0 (multi-GPU sharding)
  int epoch;              // game generation (slot restarts), part of the RNG key
  const double* noise;    // test hook: injected Dirichlet samples [G][M][A], or null
  double* noise_out;      // test hook: every root's normalised Dirichlet sample [G][M][A], or null
  int arena;              // 0: one network; 1: main.py's evaluator -- game i's first
                          // mover is network (i % 2), then the networks alternate
  int moves;              // moves per game in this launch (each game stops at its end)
};

// ---------------------------------------------------------------------------
// Board slot <-> LDS
// ---------------------------------------------------------------------------
template <class G>
__device__ __forceinline__ BoardLds<G> make_board_lds(int8_t* stone, uint8_t* invd, int* label, int* libs,
                                                      int* gsize, int* killed, int* misc) {
  return BoardLds<G>{stone, invd, label, libs, gsize, killed, misc};
}

// slot g's board -> stone / invd (LDS) and m; returns synchronised
template <class G, class T = BoardWG<G>>
__device__ __forceinline__ void board_load(int8_t* stone, uint8_t* invd, const EngineArrays& E, int g,
                                           BoardMeta& m) {
  for (int c = T::id(); c < G::CELLS; c += T::SIZE) {
    stone[c] = E.stones[(size_t)g * G::CELLS + c];
    invd[c] = E.invd[(size_t)g * G::CELLS + c];
  }
  const int* mm = E.meta + g * 4;
  m.turn = mm[0]; m.passed = mm[1]; m.done = mm[2]; m.moves = mm[3];
  T::sync();
}

// ... and back (no barrier: nothing in the launch reads the slot again)
template <class G, class T = BoardWG<G>>
__device__ __forceinline__ void board_store(const int8_t* stone, const uint8_t* invd, const EngineArrays& E, int g,
                                            const BoardMeta& m) {
  for (int c = T::id(); c < G::CELLS; c += T::SIZE) {
    E.stones[(size_t)g * G::CELLS + c] = stone[c];
    E.invd[(size_t)g * G::CELLS + c] = invd[c];
  }
  if (T::leader()) {
    int* mm = E.meta + g * 4;
    mm[0] = m.turn; mm[1] = m.passed; mm[2] = m.done; mm[3] = m.moves;
  }
}

// observation plane c at cell j (GoEnv state: black, white, turn, INVD, pass, done)
template <class G>
__device__ __forceinline__ float board_plane(const int8_t* stone, const uint8_t* invd, const BoardMeta& m, int c,
                                             int j) {
  switch (c) {
    case 0: return stone[j] == 1 ? 1.f : 0.f;
    case 1: return stone[j] == 2 ? 1.f : 0.f;
    case 2: return (float)m.turn;
    case 3: return (float)invd[j];
    case 4: return (float)m.passed;
    default: return (float)m.done;
  }
}

// ---------------------------------------------------------------------------
// Start of a move: the observation record and the move's RNG key
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint8_t flags_pack(const BoardMeta& m) {
  return (uint8_t)(m.turn | (m.passed << 1) | (m.done << 2));
}
__device__ __forceinline__ BoardMeta flags_unpack(int fl, int mv) {
  return BoardMeta{fl & 1, (fl >> 1) & 1, (fl >> 2) & 1, mv};
}

// bit 3 of a record's flags: the move was searched with the fast budget
// (playout cap randomization), so its policy row is no training target.  The
// board bits 0-2 are all flags_unpack reads.
constexpr int kFlagFast = 8;

// record ``rec`` (= g * max_moves + move) <- the board before the move; fast:
// the move's search runs on the fast budget (move_budget)
template <class G, class T = BoardWG<G>>
__device__ __forceinline__ void record_observation(const EngineArrays& E, size_t rec, const int8_t* stone,
                                                   const uint8_t* invd, const BoardMeta& m, bool fast = false) {
  for (int c = T::id(); c < G::CELLS; c += T::SIZE) {
    E.rec_stones[rec * G::CELLS + c] = stone[c];
    E.rec_invd[rec * G::CELLS + c] = invd[c];
  }
  if (T::leader()) E.rec_flags[rec] = (uint8_t)(flags_pack(m) | (fast ? kFlagFast : 0));
}

// A game's key id: its global id and generation.  The id, not the slot that
// stores the game, is the game's identity: k_selfplay_games plays games of
// several epochs in one slot.  (Host and device: the replay store's mirror of
// a game's id is this function's value.)
__host__ __device__ __forceinline__ uint32_t game_key_id(int game_base, int g, int epoch) {
  return (uint32_t)(game_base + g) ^ ((uint32_t)epoch << 24);
}
// the RNG key of move mv of the game with key id ``kid``
__device__ __forceinline__ uint64_t move_key(const SearchParams& sp, uint32_t kid, int mv) {
  return stream_key(sp.seed, kid, (uint32_t)mv);
}
// ... of slot g's move mv, where slot g holds game g of epoch pp.epoch
__device__ __forceinline__ uint64_t move_key(const SearchParams& sp, const PlayParams& pp, int g, int mv) {
  return move_key(sp, game_key_id(pp.game_base, g, pp.epoch), mv);
}

// The simulations of the self-play move with key ``key`` (playout_budget,
// mzgo_search.hpp).  CAPS: the kernel instantiation of launches that set the
// caps (sp.fast_simulations > 0; the host picks it, mzgo_dispatch.hpp); the
// other one is sp.num_simulations at compile time -- the code without caps.
// The same value on every thread, in a scalar register.
template <bool CAPS>
__device__ __forceinline__ int move_budget(const SearchParams& sp, uint64_t key) {
  if constexpr (!CAPS) return sp.num_simulations;
  else return __builtin_amdgcn_readfirstlane(
      playout_budget(key, sp.num_simulations, sp.fast_simulations, sp.full_search_prob));
}

// valid_mask from the INVD plane (self_play.py:152-158); call with all of T
template <class G, class T = BoardWG<G>, class InvdFn>
__device__ __forceinline__ void build_mask(TreeLds<G>& t, double pass_epsilon, InvdFn invd) {
  int any = 0;
  for (int a = T::id(); a < G::A; a += T::SIZE) {
    uint8_t v = a < G::CELLS ? (invd(a) == 0 ? 1 : 0) : 1;
    t.valid[a] = v;
    any |= (a < G::CELLS) && v;
  }
  any = T::any(any);
  if (T::leader()) t.pass_prior = any ? pass_epsilon : 1.0;
  T::sync();
}

// ---------------------------------------------------------------------------
// Action choice (MuZeroAgent.select_action, self_play.py:357-402).  One wave.
// Writes the policy target to pol[A]; returns the action.
// ---------------------------------------------------------------------------
// random.choice(valid actions) with the draw h: the k-th valid action, k = randbelow(h, #valid)
template <class G>
__device__ __forceinline__ int pick_valid(const TreeLds<G>& t, uint64_t h) {
  const int lane = lane_id_local();
  uint64_t vb[G::AP];
  int nvalid = 0;
#pragma unroll
  for (int j = 0; j < G::AP; ++j) {
    const int a = lane + 64 * j;
    vb[j] = __ballot(a < G::A && mask_of<G>(t, a) > 0);
    nvalid += __popcll(vb[j]);
  }
  uint32_t k = randbelow(h, (uint32_t)nvalid);
  int action = -1;
#pragma unroll
  for (int j = 0; j < G::AP; ++j) {
    const uint32_t c = __popcll(vb[j]);
    if (action < 0 && k < c) {
      uint64_t mm = vb[j];
      for (uint32_t i = 0; i < k; ++i) mm &= mm - 1;
      action = 64 * j + __ffsll((long long)mm) - 1;
    } else if (action < 0) {
      k -= c;
    }
  }
  return action;
}

// argmax over the actions of v (a lane's v[j] belongs to a = lane + 64 j), first max wins
template <class G>
__device__ __forceinline__ int argmax_action(const double (&v)[G::AP]) {
  const int lane = lane_id_local();
  double bv = -1.0;
  int ba = 0x7fffffff, payload = 0;
#pragma unroll
  for (int j = 0; j < G::AP; ++j) {
    const int a = lane + 64 * j;
    if (a < G::A && (v[j] > bv || (v[j] == bv && a < ba))) { bv = v[j]; ba = a; }
  }
  wave_argmax(bv, ba, payload);
  return ba;
}

// The visit-count policy target of a finished search, by the engine's move
// rule (variant: SearchParams::variant).  One wave; writes pol[A].
//   0, self_play.py: visit_counts * valid_mask / sum (np.sum's pairwise order),
//      or mask / sum(mask) when that sum is 0 -- always under compat
//      "reference", whose visit counts are zeros;
//   1, main.py: counts / sum of the child visit counts where valid_mask > 0;
//      when the sum is 0 the row is all zeros (choose_action_main then draws
//      an action and makes the row one-hot; reanalysis draws none).
// vc[j] = the masked count of action lane + 64 j; msum = sum(mask) (variant 0);
// returns the counts' sum.
template <class G>
__device__ __forceinline__ double visit_policy(TreeLds<G>& t, const TreeView& T, int variant, int compat,
                                               double* pol, double (&vc)[G::AP], double& msum) {
  const int lane = lane_id_local();
  if (variant == 1) {
    double tot = 0.0;
#pragma unroll
    for (int j = 0; j < G::AP; ++j) {
      const int a = lane + 64 * j;
      vc[j] = 0.0;
      if (a < G::A && mask_of<G>(t, a) > 0) { const int c = T.child[a]; vc[j] = c >= 0 ? (double)T.visits[c] : 0.0; }
      tot += vc[j];
    }
    tot = wave_sum(tot);                          // integer counts: exact in any order
#pragma unroll
    for (int j = 0; j < G::AP; ++j) {
      const int a = lane + 64 * j;
      if (a < G::A) pol[a] = tot > 0 ? vc[j] / tot : 0.0;
    }
    msum = 0.0;
    return tot;
  }
  // visit_counts * valid_mask (zeros under compat "reference", §0.6)
  for (int a = lane; a < G::A; a += 64) {
    double v = 0.0;
    if (compat == 1) { const int c = T.child[a]; v = c >= 0 ? (double)T.visits[c] : 0.0; }
    t.dbuf[a] = v * mask_of<G>(t, a);
  }
  wave_lds_sync();
  const double vsum = np_pairwise_sum<double, G::A>(t.dbuf);
#pragma unroll
  for (int j = 0; j < G::AP; ++j) { const int a = lane + 64 * j; vc[j] = a < G::A ? t.dbuf[a] : 0.0; }
  wave_lds_sync();
  for (int a = lane; a < G::A; a += 64) t.dbuf[a] = mask_of<G>(t, a);
  wave_lds_sync();
  msum = np_pairwise_sum<double, G::A>(t.dbuf);
#pragma unroll
  for (int j = 0; j < G::AP; ++j) {
    const int a = lane + 64 * j;
    if (a < G::A) pol[a] = vsum > 0 ? vc[j] / vsum : mask_of<G>(t, a) / msum;
  }
  return vsum;
}

// main.py's move rule (self-play :660-673 and the arena evaluator :552-565):
// visit_counts = child visit counts where valid_mask > 0; argmax (first max)
// with policy = counts / sum, else random.choice(valid actions) with a one-hot
// policy.  Temperature plays no part.
template <class G>
__device__ __forceinline__ int choose_action_main(TreeLds<G>& t, const TreeView& T, uint64_t key, double* pol) {
  const int lane = lane_id_local();
  double vc[G::AP], msum;
  const double tot = visit_policy<G>(t, T, 1, 1, pol, vc, msum);
  if (tot > 0) return argmax_action<G>(vc);
  const int action = pick_valid<G>(t, draw(key, TAG_ACTION, 0));
#pragma unroll
  for (int j = 0; j < G::AP; ++j) {
    const int a = lane + 64 * j;
    if (a < G::A) pol[a] = a == action ? 1.0 : 0.0;
  }
  return action;
}

template <class G>
__device__ __forceinline__ int choose_action(TreeLds<G>& t, const TreeView& T, int compat, double temperature,
                                    uint64_t key, double* pol) {
  const int lane = lane_id_local();
  double vcm[G::AP], msum;
  const double vsum = visit_policy<G>(t, T, 0, compat, pol, vcm, msum);
  const uint64_t h = draw(key, TAG_ACTION, 0);
  if (temperature == 0.0) return vsum > 0 ? argmax_action<G>(vcm) : pick_valid<G>(t, h);
  // probabilities = (vc**(1/T) * mask) / sum, or mask / sum(mask); then
  // np.random.choice's inverse CDF on a cumulative sum
  const double e = 1.0 / temperature;
#pragma unroll
  for (int j = 0; j < G::AP; ++j) {
    const int a = lane + 64 * j;
    if (a < G::A) t.dbuf[a] = (e == 1.0 ? vcm[j] : pow(vcm[j], e)) * mask_of<G>(t, a);
  }
  wave_lds_sync();
  const double ts = np_pairwise_sum<double, G::A>(t.dbuf);
  wave_lds_sync();
  // np.cumsum is a sequential f64 sum over a = 0 .. A-1: every lane runs it on
  // the probabilities read lane by lane from the registers that hold them
  // (p[j]: action lane + 64 j), and keeps the prefix of its own actions.  The
  // test cdf[a] / cdf[-1] <= u is then formed for all actions at once, with
  // the same division and comparison per entry; the index is one past the
  // highest action that passes (searchsorted(side="right") on a
  // non-decreasing cdf).
  double p[G::AP], pre[G::AP];
#pragma unroll
  for (int j = 0; j < G::AP; ++j) {
    const int a = lane + 64 * j;
    p[j] = a < G::A ? (ts > 0 ? t.dbuf[a] / ts : mask_of<G>(t, a) / msum) : 0.0;
    pre[j] = 0.0;
  }
  double run = 0.0;
#pragma unroll
  for (int j = 0; j < G::AP; ++j) {
#pragma unroll
    for (int l = 0; l < 64; ++l) {
      if (64 * j + l < G::A) {
        run += dpp::lane(p[j], l);
        if (lane == l) pre[j] = run;
      }
    }
  }
  const double total = run, u = u01(h);
  int idx = 0;
#pragma unroll
  for (int j = 0; j < G::AP; ++j) {
    const uint64_t ok = __ballot(lane + 64 * j < G::A && pre[j] / total <= u);
    if (ok) idx = 64 * j + 64 - __clzll((long long)ok);
  }
  return idx;
}

// the temperature schedule (self_play.py:471) and the action of move mv by the engine's rule (sp.variant)
__device__ __forceinline__ double move_temperature(const PlayParams& pp, int mv) {
  return mv < pp.temperature_moves ? pp.temperature : 0.0;
}
template <class G>
__device__ __forceinline__ int choose_move_action(TreeLds<G>& t, const TreeView& T, const SearchParams& sp,
                                                  const PlayParams& pp, int mv, uint64_t key, double* pol) {
  return sp.variant == 1 ? choose_action_main<G>(t, T, key, pol)
                         : choose_action<G>(t, T, sp.compat, move_temperature(pp, mv), key, pol);
}

// root value of a finished search (the record's value, mzgo_search's out_value)
__device__ __forceinline__ double root_value(const TreeView& T) {
  const int n = T.visits[0];
  return n > 0 ? T.wsum[0] / (double)n : 0.0;
}

// ---------------------------------------------------------------------------
// End of a move
// ---------------------------------------------------------------------------
// env.step(action) and env.winner() (self_play.py:479, :502) on the LDS board,
// stored back to slot g.  Returns the BOARD_* status; w = the winner once the
// game has ended, else 0.  All of T.
// HELD (k_selfplay_boards): the board and its groups stay in LDS from move to
// move of the launch -- board_groups once after board_load, then every step
// updates them (board_step's KEEP), and the caller stores the board once, when
// the game's loop ends.  (board_winning runs only on the game's last move, so
// no step follows its use of the group arrays.)
template <class G, class T = BoardWG<G>, bool HELD = false>
__device__ __forceinline__ int play_action(const EngineArrays& E, int g, BoardLds<G>& b, BoardMeta& m, int action,
                                           double komi, double& w) {
  const int st = board_step<G, T, HELD>(b, m, action);
  T::sync();
  w = (st == BOARD_OK && m.done) ? board_winning<G, T>(b, komi) : 0.0;
  if constexpr (!HELD) board_store<G, T>(b.stone, b.invd, E, g, m);
  return st;
}

// The move's reward record, the counters it bumps (sims: the simulations its
// search ran, move_budget), and the slot's status,
// length and final reward when the game ends (double pass, max_moves moves or
// a board error, status 16 + BOARD_*).  All of T call it, the leader writes;
// returns whether the game is over.
// COUNT = false: the caller adds counters 0-2 itself (count_moves), once for
// all the moves it played in the launch.
template <class G, class T = BoardWG<G>, bool COUNT = true>
__device__ __forceinline__ bool finish_move(const EngineArrays& E, int sims, int g, size_t rec, int st,
                                            const BoardMeta& m, double w) {
  const bool ended = m.done || m.moves >= E.max_moves;
  if (T::leader()) {
    E.rec_reward[rec] = w;
    if constexpr (COUNT) {
      atomicAdd(&E.counters[0], (unsigned long long)sims);
      atomicAdd(&E.counters[1], 1ull);
    }
    if (st != BOARD_OK) {
      E.status[g] = 16 + st;
    } else if (ended) {
      E.status[g] = 1;
      E.game_len[g] = m.moves;
      E.final_reward[g] = m.done ? w : 0.0;      // env.winner() is 0 unless ended
      if constexpr (COUNT) atomicAdd(&E.counters[2], 1ull);
    }
  }
  return st != BOARD_OK || ended;
}
// whether finish_move(st, m) counted a finished game (counter 2)
__device__ __forceinline__ bool game_finished(const EngineArrays& E, int st, const BoardMeta& m) {
  return st == BOARD_OK && (m.done || m.moves >= E.max_moves);
}
// what finish_move<.., false> left out, for a launch's moves of one game: one thread
__device__ __forceinline__ void count_moves(const EngineArrays& E, unsigned long long sims, int moves, int finished) {
  if (moves) {
    atomicAdd(&E.counters[0], sims);
    atomicAdd(&E.counters[1], (unsigned long long)moves);
  }
  if (finished) atomicAdd(&E.counters[2], (unsigned long long)finished);
}

}  // namespace mzgo
